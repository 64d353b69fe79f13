"""The two FMR training entry points check every argument on the host, before any HIP call: each spoiled argument list returns
``EINVAL`` / ``EUNSUPPORTED`` with a message on a machine without a GPU (the pointers are made-up addresses; the good arguments
themselves are never passed).  Also the workspace queries."""
import pytest

from fv3net_amd import _lib
from fv3net_amd._lib import EINVAL, EUNSUPPORTED

REGULAR, STRIDED, TRANSPOSED = _lib.CYCLEGAN_CONV_REGULAR, _lib.CYCLEGAN_CONV_STRIDED, _lib.CYCLEGAN_CONV_TRANSPOSED
CUBE = _lib.CYCLEGAN_HALO_CUBE
MSE, MAE = _lib.FMR_LOSS_MSE, _lib.FMR_LOSS_MAE
A, B, C, D, E, F, G, H = (0x10000000 * i for i in range(1, 9))   # far apart: no two buffers overlap

# S = 2 samples of an 8 x 8 face, 3 (+ 3 per-cell + 2 uniform) -> 5 channels, regular 3 x 3, cube halos: two chunks
WEIGHT_BYTES = 2 * (9 * (3 + 5) + 2) * 5 * 4
# 2 windows of 3 times of 6 * 4 * 4 * 3 = 288 floats, window-major: 1728 elements, one block
GOOD = {
    "fv3hip_cyclegan_train_backward_weight_context": [
        ("x", A), ("x_ld", 3), ("x_off", 0), ("x_ss", 0), ("dy", B), ("dy_ld", 5), ("dy_off", 0), ("dy_ss", 0), ("ctx_cell", F), ("c_cell", 3),
        ("ctx_uniform", G), ("c_uni", 2), ("dw", C), ("dw_ctx", H), ("db", D), ("workspace", E), ("workspace_bytes", WEIGHT_BYTES),
        ("n_samples", 2), ("n", 8), ("c_in", 3), ("c_out", 5), ("kind", REGULAR), ("k", 3), ("halo", CUBE), ("stream", None)],
    "fv3hip_fmr_loss_grad": [
        ("fake", A), ("fake_ws", 864), ("fake_ts", 288), ("real", B), ("real_ws", 864), ("real_ts", 288), ("dgan", C), ("dfake", D),
        ("n_windows", 2), ("n_times", 3), ("n_elements", 288), ("identity_kind", MAE), ("identity_weight", 0.5), ("target_kind", MSE),
        ("target_weight", 10.0), ("values", E), ("workspace", F), ("workspace_bytes", 16), ("stream", None)],
}

CASES = {
    "fv3hip_cyclegan_train_backward_weight_context": [
        ({"kind": STRIDED, "k": 3}, EUNSUPPORTED), ({"kind": STRIDED, "k": 4}, EUNSUPPORTED), ({"kind": TRANSPOSED, "k": 4}, EUNSUPPORTED),
        ({"kind": REGULAR, "k": 4}, EUNSUPPORTED), ({"kind": REGULAR, "k": 7, "n": 2}, EINVAL), ({"halo": 2}, EINVAL),
        ({"x": None}, EINVAL), ({"dy": None}, EINVAL), ({"dw": None}, EINVAL), ({"workspace": None}, EINVAL),
        ({"workspace_bytes": WEIGHT_BYTES - 1}, EINVAL), ({"n_samples": 0}, EINVAL), ({"x_ld": 2}, EINVAL), ({"c_in": 0}, EINVAL),
        ({"ctx_cell": None}, EINVAL), ({"c_cell": 0}, EINVAL), ({"ctx_uniform": None}, EINVAL), ({"c_uni": 0}, EINVAL),
        ({"dw_ctx": None}, EINVAL), ({"c_cell": -1}, EINVAL), ({"c_uni": (1 << 12) + 1}, EINVAL),
        ({"ctx_cell": None, "c_cell": 0, "ctx_uniform": None, "c_uni": 0}, EINVAL),            # dw_ctx without a context
        ({"dw": A}, EINVAL), ({"db": B}, EINVAL), ({"workspace": C}, EINVAL), ({"dw_ctx": F}, EINVAL), ({"dw_ctx": C}, EINVAL),
        ({"dw_ctx": G}, EINVAL), ({"workspace": H}, EINVAL)],
    "fv3hip_fmr_loss_grad": [
        ({"fake": None}, EINVAL), ({"real": None}, EINVAL), ({"values": None}, EINVAL), ({"workspace": None}, EINVAL),
        ({"workspace_bytes": 15}, EINVAL), ({"n_times": 1}, EINVAL), ({"n_windows": 0}, EINVAL), ({"n_elements": 0}, EINVAL),
        ({"identity_kind": 2}, EINVAL), ({"target_kind": -1}, EINVAL), ({"identity_weight": float("nan")}, EINVAL),
        ({"target_weight": float("inf")}, EINVAL), ({"dfake": None}, EINVAL),                   # dgan without dfake
        ({"fake_ts": 287}, EINVAL), ({"fake_ws": 863}, EINVAL), ({"real_ts": 0}, EINVAL),      # the grid folds onto itself
        ({"fake_ws": 288, "fake_ts": 575}, EINVAL),                                             # time-major needs ts >= 2 * 288
        ({"dfake": A}, EINVAL), ({"dfake": B}, EINVAL), ({"dgan": D + 4}, EINVAL),             # dgan overlaps dfake without being it
        ({"values": D}, EINVAL), ({"workspace": D}, EINVAL), ({"workspace": E}, EINVAL)],
}


def test_the_tables_match_the_signatures():
    for name, good in GOOD.items():
        assert len(good) == len(_lib.SIGNATURES[name][1]), name
        names = [arg for arg, _ in good]
        assert all(k in names for changes, _ in CASES[name] for k in changes), name


@pytest.mark.parametrize("name", sorted(GOOD))
def test_argument_checks(name):
    lib = _lib.load()
    fn, wrong = getattr(lib, name), []
    for changes, expected in CASES[name]:
        rc = fn(*[changes.get(arg, good) for arg, good in GOOD[name]])
        message = lib.fv3hip_last_error()
        if rc != expected or not message:
            wrong.append((changes, rc, expected, message))
    assert not wrong, wrong


def test_refusals_name_the_offending_value():
    lib = _lib.load()
    spoil = lambda name, **changes: getattr(lib, name)(*[changes.get(arg, good) for arg, good in GOOD[name]])   # noqa: E731
    assert spoil("fv3hip_cyclegan_train_backward_weight_context", kind=STRIDED, k=4) == EUNSUPPORTED
    assert b"context channels are built for the regular convolution, got kind 1" in lib.fv3hip_last_error()
    assert spoil("fv3hip_fmr_loss_grad", n_times=1) == EINVAL
    assert b"n_times must be in [2, 2^20]" in lib.fv3hip_last_error() and b"got 1" in lib.fv3hip_last_error()
    assert spoil("fv3hip_fmr_loss_grad", identity_kind=7) == EINVAL
    assert b"unknown loss kind 7" in lib.fv3hip_last_error()


def test_workspace_queries():
    lib, S, n, ci, co = _lib.load(), 3, 12, 20, 70
    chunk = lib.fv3hip_cyclegan_train_chunk_cells()
    chunks = -(-S * 864 // chunk)
    context = lib.fv3hip_cyclegan_train_backward_weight_context_workspace_bytes
    plain = lib.fv3hip_cyclegan_train_backward_weight_workspace_bytes
    assert context(S, n, ci, 3, 2, co, 3) == chunks * (9 * (ci + 5) + 2) * co * 4     # the context rows have their own term
    assert context(S, n, ci, 0, 0, co, 5) == plain(S, n, ci, co, REGULAR, 5)
    assert context(S, n, ci, 3, 2, co, 4) == 0 and context(S, n, ci, -1, 2, co, 3) == 0
    loss = lib.fv3hip_fmr_loss_grad_workspace_bytes
    assert loss(2, 3, 288) == 16 and loss(1, 4, 6 * 48 * 48 * 4) == -(-4 * 6 * 48 * 48 * 4 // 2048) * 16
    assert loss(2, 1, 288) == 0 and loss(0, 3, 288) == 0
