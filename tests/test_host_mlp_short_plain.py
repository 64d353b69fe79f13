"""The fused MLP path's input table on the host (build_input_table of csrc/mlp_desc.h, through the host-only diagnostic
fv3hip_diag_mlp_input_table): where the partial plain chunk goes and how many k-pair slots the kernels are told to run.

The partial chunk becomes the plain block's FIRST -- its real rows in unchanged order, then the zero rows, then the full
chunks -- where it holds at most 26 real rows (13 slots), another plain chunk follows and the chunk ahead of the block
is none or the 8-slot last log chunk; everywhere else the table is what it was: log rows, their padding, plain rows."""
import ctypes

import numpy as np
import pytest

from fv3net_amd import _lib


def _table(n_log, n_plain):
    """perm, n_log_padded, short_plain_slots of a model with n_log log-transformed features ahead of n_plain plain ones."""
    lib = _lib.load()
    fn = lib.fv3hip_diag_mlp_input_table
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    blocks = [(n, t) for n, t in ((n_log, _lib.TRANSFORM_LOG), (n_plain, _lib.TRANSFORM_NONE)) if n]
    arrays = {"in_source": np.zeros(len(blocks), np.intc), "in_feat_start": np.zeros(len(blocks), np.intc),
              "in_nfeat": np.array([n for n, _ in blocks], np.intc), "in_transform": np.array([t for _, t in blocks], np.intc),
              "out_nfeat": np.array([3], np.intc)}
    eps = np.full(len(blocks), 1e-8, np.float32)
    d = _lib.MlpDesc()
    d.n_sources, d.n_inputs, d.n_hidden, d.width, d.n_outputs, d.n_residual = 1, len(blocks), 1, 256, 1, 0
    d.hidden_activation = _lib.ACT_RELU
    for k, a in arrays.items():
        setattr(d, k, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    d.in_eps = eps.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    cap = 32 * ((n_log + n_plain + 31) // 32)
    perm = (ctypes.c_int * cap)()
    nlp, slots = ctypes.c_int(-7), ctypes.c_int(-7)
    assert fn(ctypes.byref(d), perm, cap - 1, ctypes.byref(nlp), ctypes.byref(slots)) == -1  # (too small a buffer)
    assert fn(ctypes.byref(d), perm, cap, ctypes.byref(nlp), ctypes.byref(slots)) == cap
    return list(perm), nlp.value, slots.value


def _expected(n_log, n_plain, log_padded, short):
    """The table written out: log rows, their padding if `log_padded`; the plain rows with the zero rows behind the
    partial chunk's real rows if `short`, else behind all of them."""
    n_ktab = 32 * ((n_log + n_plain + 31) // 32)
    perm = list(range(n_log)) + [-1] * ((-n_log) % 32 if log_padded else 0)
    plain = list(range(n_log, n_log + n_plain))
    n_zero = n_ktab - len(perm) - n_plain
    rows = 32 - n_zero
    perm += plain[:rows] + [-1] * n_zero + plain[rows:] if short else plain + [-1] * n_zero
    assert len(perm) == n_ktab
    return perm


@pytest.mark.parametrize("n_log,n_plain,log_padded,short", [
    (0, 33, False, True), (0, 45, False, True), (0, 58, False, True), (0, 90, False, True),   # 1, 13, 26, 26 real rows
    (0, 59, False, False), (0, 63, False, False),                                               # 27, 31 rows: 14 and 16 slots
    (13, 58, True, True), (16, 49, True, True), (237, 474, True, True),                         # behind an 8-slot log chunk
    (13, 63, True, False),                                                                      # ... 31 rows
    (32, 33, False, False), (20, 45, True, False), (20, 58, True, False), (17, 58, True, False),  # a full log chunk ahead
    (13, 33, False, False), (13, 45, False, False),                                             # no room to pad the log block
    (45, 0, True, False), (13, 0, True, False), (0, 26, False, False), (0, 32, False, False), (13, 26, True, False),
    (0, 64, False, False),                                                                      # nothing partial
], ids=lambda v: str(v))
def test_partial_plain_chunk_in_the_table(n_log, n_plain, log_padded, short):
    perm, n_log_padded, slots = _table(n_log, n_plain)
    assert perm == _expected(n_log, n_plain, log_padded, short)
    assert n_log_padded == (32 * ((n_log + 31) // 32) if log_padded else n_log)
    assert slots == (13 if short else 0)
    real = [k for k in perm if k >= 0]
    assert real == list(range(n_log + n_plain))  # every feature once, each block in its own order


def test_the_flagship_table():
    """The Zhao-Carr emulator: 237 log rows + 19, then 26 plain rows + 6 zero rows, then 14 full chunks."""
    perm, n_log_padded, slots = _table(237, 474)
    assert (len(perm), n_log_padded, slots) == (736, 256, 13)
    assert perm[237:256] == [-1] * 19 and perm[256:282] == list(range(237, 263)) and perm[282:288] == [-1] * 6
    assert perm[288:] == list(range(263, 711))


def test_refuses_a_bad_descriptor():
    lib = _lib.load()
    out = (ctypes.c_int * 64)()
    n = ctypes.c_int()
    lib.fv3hip_diag_mlp_input_table.restype = ctypes.c_int
    lib.fv3hip_diag_mlp_input_table.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                ctypes.POINTER(ctypes.c_int)]
    assert lib.fv3hip_diag_mlp_input_table(None, out, 64, ctypes.byref(n), ctypes.byref(n)) == -1
