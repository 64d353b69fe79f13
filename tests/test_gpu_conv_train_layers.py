"""The entry points of csrc/conv_train.hip, one by one, against the float64 restatement (tests/conv_train_np.py).

Shapes are the smallest at which the 64 x 64 tiling over pixels and filters / channels (a tile of at most 32 live columns
shares its contraction between the wave pairs, a wider one does not: F and C on both sides of 32), the MFMA's k-step of 2,
the 32-deep contraction chunks over (tap, channel) and the ``train_conv_chunk_pixels()`` pixel chunks can go wrong.  Every
operand is a view of a wider buffer -- sample, x, y strides and the kernel's leading dimension all longer than the extents; the padding holds NaN
on inputs and a sentinel on outputs, which must be untouched afterwards.  Every case runs without and with a sample table; the
table has a repeat, a descending run and an entry outside the resident samples (which reads as zeros) where the batch is long
enough to hold them.

Gates (derived, DESIGN.md sections 21 and 23): a contraction of length n, ``2 n 2^-24 sum |a_i| |b_i| + 1e-37`` with
n = k k C (+ 1 with a bias) for the forward, k k F for backward data and the batch's pixel count for dW and db.  Every test
prints its worst fraction of its gate."""
import ctypes

import numpy as np
import pytest
import torch

import conv_train_np as C
import train_np as T

pytestmark = pytest.mark.gpu

SENTINEL = -777.0


def _ops():
    from fv3net_amd import ops

    return ops


def padded(a, device, fill=float("nan")):
    """``a`` (4-D) on the device as a view of a buffer that is longer along every axis; the padding holds ``fill``."""
    a = np.asarray(a, np.float32)
    buf = torch.full((a.shape[0] + 1, a.shape[1] + 1, a.shape[2] + 2, a.shape[3] + 3), fill, dtype=torch.float32, device=device)
    view = buf[:a.shape[0], :a.shape[1], :a.shape[2], :a.shape[3]]
    view.copy_(torch.from_numpy(a))
    return buf, view


def padded_kernel(w, device, fill=float("nan")):
    """A kernel ``[k, k, c, f]`` as a matrix ``[k k c][f]`` with a leading dimension of f + 5."""
    w = np.asarray(w, np.float32)
    buf = torch.full(w.shape[:3] + (w.shape[3] + 5,), fill, dtype=torch.float32, device=device)
    view = buf[..., :w.shape[3]]
    view.copy_(torch.from_numpy(w))
    return buf, view


def out_view(shape, device):
    return padded(np.full(shape, SENTINEL, np.float32), device, fill=SENTINEL)


def untouched(buf, view):
    """Everything of ``buf`` outside ``view`` still holds the sentinel."""
    keep = view.clone()
    view.fill_(SENTINEL)
    ok = bool(torch.all(buf == SENTINEL))
    view.copy_(keep)
    return ok


def worst(got, want, gate):
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.abs(np.asarray(got, np.float64) - want) / gate
    assert np.all(np.isfinite(got)), "non-finite result"
    return float(np.max(frac))


def make_idx(n, table, device):
    """n = 5: a repeat, then a descending run whose first entry lies outside the table; shorter batches hold what fits."""
    idx = {1: [table - 1], 2: [table - 1, 0]}.get(n, [1, 1, table + 3, table - 1, 0][:n] + [2] * max(0, n - 5))
    idx = np.asarray(idx, np.int64)
    return idx, torch.from_numpy(idx).to(device)


def factor(p):
    """(x, y) with x y = p, as square as it gets."""
    x = max(d for d in range(1, int(p ** 0.5) + 1) if p % d == 0)
    return x, p // x


# (k, C, F, output extent, batch): a covering subset of k in {1, 3, 5} x C in {1, 3, 7, 33, 159} x F in {1, 8, 32, 33, 65} x
# extents {1 x 1, 1 x 5, 5 x 1, 7 x 9, 16 x 16, 17 x 15} x batch in {1, 2, 5}
SHAPES = [(1, 1, 1, (1, 1), 1), (3, 3, 8, (1, 5), 2), (5, 7, 33, (5, 1), 1), (3, 33, 32, (7, 9), 5), (3, 159, 32, (16, 16), 2),
          (1, 159, 65, (17, 15), 1), (5, 3, 65, (17, 15), 2), (3, 7, 1, (16, 16), 5), (3, 1, 33, (7, 9), 2), (5, 33, 8, (7, 9), 1),
          (1, 7, 8, (5, 1), 5)]


def chunk_shapes():
    """Batches of chunk - 1, chunk and chunk + 1 output pixels (one sample), and two samples of chunk + 1 (three chunks)."""
    chunk = _ops().train_conv_chunk_pixels()
    return [(3, 3, 8, factor(chunk - 1), 1), (3, 3, 8, factor(chunk), 1), (3, 3, 8, factor(chunk + 1), 1), (1, 7, 33, factor(chunk + 1), 2)]


def _inputs(rng, k, c, f, ext, n, use_idx):
    X, Y = ext[0] + k - 1, ext[1] + k - 1
    table = n + 3 if use_idx else n
    a = rng.normal(0, 1, (table, X, Y, c)).astype(np.float32)
    w = (rng.normal(0, 1, (k, k, c, f)) / np.sqrt(k * k * c)).astype(np.float32)
    return a, w


def _forward_case(device, k, c, f, ext, n, use_idx):
    ops = _ops()
    rng = np.random.default_rng(k * 1000 + c * 10 + f + n)
    a, w = _inputs(rng, k, c, f, ext, n, use_idx)
    b = rng.normal(0, 1, f).astype(np.float32)
    idx, idx_d = make_idx(n, a.shape[0], device) if use_idx else (None, None)
    a_d, w_d = padded(a, device)[1], padded_kernel(w, device)[1]
    for relu, bias in ((False, True), (True, True), (True, False)):
        buf, out = out_view((n,) + tuple(ext) + (f,), device)
        b_d = torch.from_numpy(b).to(device) if bias else None
        ops.train_conv_forward(a_d, w_d, b_d, out, idx=idx_d, relu=relu)
        got = out.cpu().numpy()
        want, mag = C.conv_forward(a, w, b if bias else None, idx, relu)
        frac = worst(got, want, T.dot_bound(k * k * c + (1 if bias else 0), mag))
        print(f"conv forward k={k} C={c} F={f} out={ext} n={n} idx={use_idx} relu={relu} bias={bias}: {frac:.3f} of the gate")
        assert frac <= 1.0 and untouched(buf, out)
        ops.train_conv_forward(a_d, w_d, b_d, out, idx=idx_d, relu=relu)
        assert np.array_equal(got.view(np.uint32), out.cpu().numpy().view(np.uint32)), "the same call twice gives the same bits"
        if use_idx and n >= 3 and relu and bias:
            assert np.array_equal(got[2], np.broadcast_to(np.where(b < 0, np.float32(0), b), got[2].shape)), \
                "a sample outside the table reads as zeros"


@pytest.mark.parametrize("k,c,f,ext,n", SHAPES)
@pytest.mark.parametrize("use_idx", [False, True])
def test_forward(device, k, c, f, ext, n, use_idx):
    _forward_case(device, k, c, f, ext, n, use_idx)


def _backward_data_case(device, k, c, f, ext, n, mask):
    ops = _ops()
    rng = np.random.default_rng(k * 1000 + c * 10 + f + n + 1)
    X, Y = ext[0] + k - 1, ext[1] + k - 1
    dh = rng.normal(0, 1, (n,) + tuple(ext) + (f,)).astype(np.float32)
    w = (rng.normal(0, 1, (k, k, c, f)) / np.sqrt(k * k * f)).astype(np.float32)
    p = None
    if mask:
        p = np.maximum(rng.normal(0, 1, (n, X, Y, c)), 0).astype(np.float32)
        p[0, 0, 0, 0] = 0.0             # an activation of exactly 0 masks
        p[-1, -1, -1, -1] = np.nan      # and so does a NaN
    dh_d, w_d = padded(dh, device)[1], padded_kernel(w, device)[1]
    p_d = None if p is None else padded(p, device)[1]
    buf, out = out_view((n, X, Y, c), device)
    ops.train_conv_backward_data(dh_d, w_d, p_d, out)
    got = out.cpu().numpy()
    want, mag = C.conv_backward_data(dh, w, p)
    frac = worst(got, want, T.dot_bound(k * k * f, mag))
    print(f"conv backward data k={k} C={c} F={f} out={ext} n={n} mask={mask}: {frac:.3f} of the gate")
    assert frac <= 1.0 and untouched(buf, out)
    if p is not None:
        assert np.all(got[~(p > 0)].view(np.uint32) == 0), "relu'(0) = 0: a masked element is exactly +0"
    ops.train_conv_backward_data(dh_d, w_d, p_d, out)
    assert np.array_equal(got.view(np.uint32), out.cpu().numpy().view(np.uint32)), "the same call twice gives the same bits"


@pytest.mark.parametrize("k,c,f,ext,n", SHAPES)
@pytest.mark.parametrize("mask", [False, True])
def test_backward_data(device, k, c, f, ext, n, mask):
    _backward_data_case(device, k, c, f, ext, n, mask)


def _backward_weight(ops, device, a_d, dh_d, idx_d, n, k, c, f, with_db=True):
    X, Y = int(a_d.shape[1]), int(a_d.shape[2])
    bufw, dw = padded_kernel(np.full((k, k, c, f), SENTINEL, np.float32), device, fill=SENTINEL)
    db = torch.full((f,), SENTINEL, dtype=torch.float32, device=device) if with_db else None
    floats = ops.train_conv_backward_weight_workspace_floats(n, X, Y, k, c, f)
    ws = torch.full((floats,), float("nan"), dtype=torch.float32, device=device) if floats else None
    ops.train_conv_backward_weight(a_d, dh_d, dw, db, idx=idx_d, workspace=ws)
    return bufw, dw, dw.cpu().numpy(), (db.cpu().numpy() if with_db else None)


def _backward_weight_case(device, k, c, f, ext, n, use_idx):
    ops = _ops()
    rng = np.random.default_rng(k * 1000 + c * 10 + f + n + 2)
    a, _ = _inputs(rng, k, c, f, ext, n, use_idx)
    dh = rng.normal(0, 1, (n,) + tuple(ext) + (f,)).astype(np.float32)
    idx, idx_d = make_idx(n, a.shape[0], device) if use_idx else (None, None)
    a_d, dh_d = padded(a, device)[1], padded(dh, device)[1]
    bufw, dw_view, dw, db = _backward_weight(ops, device, a_d, dh_d, idx_d, n, k, c, f)
    want_w, want_b, mag_w, mag_b = C.conv_backward_weight(a, dh, k, idx)
    pixels = n * ext[0] * ext[1]
    fw, fb = worst(dw, want_w, T.dot_bound(pixels, mag_w)), worst(db, want_b, T.dot_bound(pixels, mag_b))
    print(f"conv backward weight k={k} C={c} F={f} out={ext} n={n} idx={use_idx} ({pixels} pixels): dW {fw:.3f}, db {fb:.3f} of the gate")
    assert fw <= 1.0 and fb <= 1.0 and untouched(bufw, dw_view)
    _, _, dw2, db2 = _backward_weight(ops, device, a_d, dh_d, idx_d, n, k, c, f)
    assert np.array_equal(dw.view(np.uint32), dw2.view(np.uint32)) and np.array_equal(db.view(np.uint32), db2.view(np.uint32))
    _, _, dw3, none = _backward_weight(ops, device, a_d, dh_d, idx_d, n, k, c, f, with_db=False)   # db may be skipped
    assert none is None and np.array_equal(dw.view(np.uint32), dw3.view(np.uint32))


@pytest.mark.parametrize("k,c,f,ext,n", SHAPES)
@pytest.mark.parametrize("use_idx", [False, True])
def test_backward_weight(device, k, c, f, ext, n, use_idx):
    _backward_weight_case(device, k, c, f, ext, n, use_idx)


@pytest.mark.parametrize("which", range(4))
def test_pixel_chunks(device, which):
    """chunk - 1, chunk, chunk + 1 output pixels and three chunks: the forward's and backward data's tiling over the same pixel
    counts, and the weight gradient's one-chunk / workspace paths."""
    ops = _ops()
    k, c, f, ext, n = chunk_shapes()[which]
    chunk = ops.train_conv_chunk_pixels()
    pixels = n * ext[0] * ext[1]
    X, Y = ext[0] + k - 1, ext[1] + k - 1
    floats = ops.train_conv_backward_weight_workspace_floats(n, X, Y, k, c, f)
    assert floats == (0 if pixels <= chunk else -(-pixels // chunk) * (k * k * c + 1) * f)
    for use_idx in (False, True):
        _backward_weight_case(device, k, c, f, ext, n, use_idx)
    _forward_case(device, k, c, f, ext, n, False)
    _backward_data_case(device, k, c, f, ext, n, True)


def test_a_short_workspace_is_refused(device):
    ops = _ops()
    k, c, f, ext, n = chunk_shapes()[2]
    a_d = torch.zeros((n, ext[0] + k - 1, ext[1] + k - 1, c), dtype=torch.float32, device=device)
    dh_d = torch.zeros((n,) + tuple(ext) + (f,), dtype=torch.float32, device=device)
    dw, db = torch.zeros((k, k, c, f), dtype=torch.float32, device=device), torch.zeros(f, dtype=torch.float32, device=device)
    need = ops.train_conv_backward_weight_workspace_floats(n, int(a_d.shape[1]), int(a_d.shape[2]), k, c, f)
    for ws in (None, torch.zeros(need - 1, dtype=torch.float32, device=device)):
        with pytest.raises(Exception, match="needs a workspace"):
            ops.train_conv_backward_weight(a_d, dh_d, dw, db, workspace=ws)


def test_one_nan_reaches_exactly_its_stencil_column_and_bias(device):
    """One NaN in dH: in dA the cells whose stencil holds it (all channels), in dW its filter's column, in db its filter; every
    other element keeps its bits.  Three pixel chunks, so the partial sums and their addition are covered."""
    ops = _ops()
    k, c, f, n = 3, 7, 33, 2
    ext = factor(ops.train_conv_chunk_pixels() + 1)
    rng = np.random.default_rng(11)
    a, w = _inputs(rng, k, c, f, ext, n, False)
    dh = rng.normal(0, 1, (n,) + tuple(ext) + (f,)).astype(np.float32)
    s0, x0, y0, f0 = 1, ext[0] // 2, ext[1] - 1, 20
    bad = dh.copy()
    bad[s0, x0, y0, f0] = np.nan
    a_d, w_d = padded(a, device)[1], padded_kernel(w, device)[1]
    results = []
    for cot in (dh, bad):
        d_d = padded(cot, device)[1]
        _, out = out_view(a.shape, device)
        ops.train_conv_backward_data(d_d, w_d, None, out)
        _, _, dw, db = _backward_weight(ops, device, a_d, d_d, None, n, k, c, f)
        results.append((out.cpu().numpy(), dw, db))
    (da0, dw0, db0), (da1, dw1, db1) = results
    hit = np.zeros(a.shape, bool)
    hit[s0, x0:x0 + k, y0:y0 + k, :] = True
    assert np.all(np.isnan(da1[hit])) and np.array_equal(da1[~hit].view(np.uint32), da0[~hit].view(np.uint32))
    col = np.zeros(dw0.shape, bool)
    col[..., f0] = True
    assert np.all(np.isnan(dw1[col])) and np.array_equal(dw1[~col].view(np.uint32), dw0[~col].view(np.uint32))
    assert np.isnan(db1[f0]) and np.array_equal(np.delete(db1, f0).view(np.uint32), np.delete(db0, f0).view(np.uint32))
    assert np.all(np.isfinite(da0)) and np.all(np.isfinite(dw0)) and np.all(np.isfinite(db0))


def test_relu_keeps_a_nan(device):
    ops = _ops()
    a = np.ones((1, 3, 3, 2), np.float32)
    a[0, 1, 1, 0] = np.nan
    out = torch.zeros((1, 1, 1, 4), dtype=torch.float32, device=device)
    ops.train_conv_forward(torch.from_numpy(a).to(device), torch.ones((3, 3, 2, 4), dtype=torch.float32, device=device), None, out,
                           relu=True)
    assert bool(torch.all(torch.isnan(out)))


@pytest.mark.parametrize("k,c,f", [(1, 3, 2), (3, 1, 1), (3, 7, 33), (5, 33, 8), (3, 159, 32)])
def test_constraint_is_bitwise_torch(device, k, c, f):
    ops = _ops()
    w = np.random.default_rng(k + c + f).normal(0, 1, (k, k, c, f)).astype(np.float32)
    tw = torch.from_numpy(w)
    want = (0.5 * (tw + tw.transpose(0, 1))).numpy()
    buf, view = padded_kernel(w, device, fill=SENTINEL)
    ops.train_conv_constrain(view)
    got = view.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got.view(np.uint32), C.constrain(w).view(np.uint32))
    assert np.array_equal(got.view(np.uint32), got.transpose(1, 0, 2, 3).view(np.uint32)), "bitwise symmetric"
    assert untouched(buf, view)


def test_chunk_pixels_is_the_documented_constant():
    assert _ops().train_conv_chunk_pixels() == 512   # as include/fv3hip.h documents it


def test_bad_shapes_are_refused_before_any_launch(device):
    """A negative k, an even k and an extent smaller than k: a negative status and a message, the output untouched."""
    from fv3net_amd import _lib

    lib = _lib.load()
    a = torch.zeros((1, 4, 4, 2), dtype=torch.float32, device=device)
    w = torch.zeros(5 * 5 * 2 * 3, dtype=torch.float32, device=device)
    out = torch.full((1, 4, 4, 3), SENTINEL, dtype=torch.float32, device=device)
    dw = torch.full((5 * 5 * 2 * 3,), SENTINEL, dtype=torch.float32, device=device)
    db = torch.full((3,), SENTINEL, dtype=torch.float32, device=device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    sa, so = (32, 8, 2), (48, 12, 3)
    for k, X, Y, text in ((-1, 4, 4, "kernel_size must be odd"), (2, 4, 4, "kernel_size must be odd"), (5, 4, 4, "does not hold a 5 x 5 kernel"),
                          (3, 4, 2, "does not hold a 3 x 3 kernel")):
        codes = [lib.fv3hip_train_conv_forward(p(a), *sa, 1, None, p(w), 3, None, p(out), *so, 1, X, Y, k, 2, 3, _lib.ACT_RELU, None),
                 lib.fv3hip_train_conv_backward_data(p(out), *so, p(w), 3, None, 0, 0, 0, p(a), *sa, 1, X, Y, k, 2, 3, None),
                 lib.fv3hip_train_conv_backward_weight(p(a), *sa, 1, None, p(out), *so, p(dw), 3, p(db), None, 0, 1, X, Y, k, 2, 3, None)]
        assert all(code < 0 for code in codes), (k, X, Y, codes)
        assert text in lib.fv3hip_last_error().decode()
    assert lib.fv3hip_train_conv_constrain(p(dw), 3, 2, 2, 3, None) < 0 and lib.fv3hip_train_conv_constrain(p(dw), 3, -3, 2, 3, None) < 0
    assert lib.fv3hip_train_conv_forward(p(a), *sa, 1, None, p(w), 3, None, p(out), *so, 1, 4, 4, 3, 2, 3, _lib.ACT_TANH, None) < 0
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENTINEL)) and bool(torch.all(dw == SENTINEL)) and bool(torch.all(db == SENTINEL))
