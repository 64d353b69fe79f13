"""The entry points of csrc/mlp_train.hip, one by one, against the float64 restatement (tests/train_np.py).

Shapes are the smallest at which the 64 x 64 tiling, the MFMA's k-step of 2, the 16-row contraction chunks and the
``train_chunk_rows()`` batch chunks can go wrong.  Every operand is a view with a row stride longer than its features; the
padding holds NaN on inputs and a sentinel on outputs.

Gates (derived): a contraction of length n (+ 1 with a bias) ``2 n 2^-24 sum |a_i| |b_i| + 1e-37``; the
loss gradient, elementwise, ``8 2^-24 (|yhat scale| + |center| + |t|) |2 inv_cstd2 scale wnorm|``; the loss, a float64 sum of
squared float32 differences d known to within ``ed = 4 2^-24 (|yhat scale| + |center| + |t|)``: the sum of
``(2 |d| ed + ed^2) inv_cstd2 wnorm``.  Every test prints its worst fraction of its gate."""
import numpy as np
import pytest
import torch

import train_np as T

pytestmark = pytest.mark.gpu

SENTINEL = -777.0


def _ops():
    from fv3net_amd import ops

    return ops


def padded(a, device, pad=3):
    """``a`` on the device as a view of a wider buffer whose padding is NaN."""
    a = np.asarray(a, np.float32)
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32, device=device)
    view = buf[:, :a.shape[1]]
    view.copy_(torch.from_numpy(a))
    return view


def out_view(rows, feats, device, pad=5):
    buf = torch.full((rows, feats + pad), SENTINEL, dtype=torch.float32, device=device)
    return buf, buf[:, :feats]


def untouched(buf, feats):
    return bool(torch.all(buf[:, feats:] == SENTINEL))


def worst(got, want, gate):
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.abs(np.asarray(got, np.float64) - want) / gate
    assert np.all(np.isfinite(got)), "non-finite result"
    return float(np.max(frac))


def make_idx(rng, n, table_rows, device):
    """Row numbers with repeats and a descending run."""
    idx = rng.integers(0, table_rows, n)
    if n >= 4:
        idx[1] = idx[0]
        idx[-3:] = np.sort(idx[-3:])[::-1]
    return idx, torch.from_numpy(idx.astype(np.int64)).to(device)


# (K, O, batch): a covering subset of K in {1, 3, 159, 711} x O in {1, 8, 12, 33, 256, 396} x batch in {1, 31, 33, 512}
SHAPES = [(1, 1, 1), (1, 256, 31), (3, 8, 33), (3, 33, 512), (159, 8, 512), (159, 12, 31), (159, 396, 33), (711, 1, 33), (711, 256, 31),
          (711, 396, 1), (711, 33, 512), (3, 12, 1)]


@pytest.mark.parametrize("k,o,n", SHAPES)
@pytest.mark.parametrize("use_idx", [False, True])
def test_forward(device, k, o, n, use_idx):
    ops = _ops()
    rng = np.random.default_rng(k * 1000 + o + n)
    table = n + 7 if use_idx else n
    a, w, b = rng.normal(0, 1, (table, k)).astype(np.float32), (rng.normal(0, 1, (k, o)) / np.sqrt(k)).astype(np.float32), \
        rng.normal(0, 1, o).astype(np.float32)
    idx, idx_d = make_idx(rng, n, table, device) if use_idx else (None, None)
    for relu in (False, True):
        buf, out = out_view(n, o, device)
        ops.train_linear_forward(padded(a, device), padded(w, device), torch.from_numpy(b).to(device), out, idx=idx_d, relu=relu)
        want, mag = T.linear_forward(a, w, b, idx, relu)
        frac = worst(out.cpu().numpy(), want, T.dot_bound(k + 1, mag))
        print(f"forward k={k} o={o} n={n} idx={use_idx} relu={relu}: {frac:.3f} of the gate")
        assert frac <= 1.0 and untouched(buf, o)


@pytest.mark.parametrize("k,o,n", SHAPES)
@pytest.mark.parametrize("mask", ["none", "rows", "shared"])
def test_backward_data(device, k, o, n, mask):
    ops = _ops()
    rng = np.random.default_rng(k * 1000 + o + n + 1)
    dh, w = rng.normal(0, 1, (n, o)).astype(np.float32), (rng.normal(0, 1, (k, o)) / np.sqrt(o)).astype(np.float32)
    p = None
    if mask != "none":
        p = np.maximum(rng.normal(0, 1, (1 if mask == "shared" else n, k)), 0).astype(np.float32)
        p[0, 0] = 0.0   # an activation of exactly 0 masks
    buf, out = out_view(n, k, device)
    ops.train_linear_backward_data(padded(dh, device), padded(w, device), None if p is None else padded(p, device), out,
                                   shared_p=mask == "shared")
    want, mag = T.linear_backward_data(dh, w, p, shared_p=mask == "shared")
    got = out.cpu().numpy()
    frac = worst(got, want, T.dot_bound(o, mag) )
    print(f"backward data k={k} o={o} n={n} mask={mask}: {frac:.3f} of the gate")
    assert frac <= 1.0 and untouched(buf, k)
    if p is not None:
        masked = np.broadcast_to(p <= 0, got.shape)
        assert np.all(got[masked] == 0), "relu'(0) = 0: a masked element is exactly 0"


def _backward_weight(ops, device, a, dh, idx_d, n, k, o):
    bufw, dw = out_view(k, o, device)
    db = torch.full((o,), SENTINEL, dtype=torch.float32, device=device)
    floats = ops.train_backward_weight_workspace_floats(n, k, o)
    ws = torch.full((floats,), float("nan"), dtype=torch.float32, device=device) if floats else None
    ops.train_linear_backward_weight(padded(a, device), padded(dh, device), dw, db, idx=idx_d, workspace=ws)
    return bufw, dw.cpu().numpy(), db.cpu().numpy()


CHUNK = 512   # fv3hip_train_chunk_rows(), as include/fv3hip.h documents it
CHUNK_SHAPES = [(3, 12, CHUNK - 1), (3, 12, CHUNK), (3, 12, CHUNK + 1), (159, 8, CHUNK + 1), (33, 33, 2 * CHUNK + 31)]


def test_chunk_rows_is_the_documented_constant():
    assert _ops().train_chunk_rows() == CHUNK
    assert _ops().train_backward_weight_workspace_floats(CHUNK, 3, 12) == 0
    assert _ops().train_backward_weight_workspace_floats(CHUNK + 1, 3, 12) == 2 * 4 * 12


@pytest.mark.parametrize("k,o,n", SHAPES + CHUNK_SHAPES)
@pytest.mark.parametrize("use_idx", [False, True])
def test_backward_weight(device, k, o, n, use_idx):
    ops = _ops()
    rng = np.random.default_rng(k * 1000 + o + n + 2)
    table = n + 7 if use_idx else n
    a, dh = rng.normal(0, 1, (table, k)).astype(np.float32), rng.normal(0, 1, (n, o)).astype(np.float32)
    idx, idx_d = make_idx(rng, n, table, device) if use_idx else (None, None)
    bufw, dw, db = _backward_weight(ops, device, a, dh, idx_d, n, k, o)
    want_w, want_b, mag_w, mag_b = T.linear_backward_weight(a, dh, idx)
    fw, fb = worst(dw, want_w, T.dot_bound(n, mag_w)), worst(db, want_b, T.dot_bound(n, mag_b))
    print(f"backward weight k={k} o={o} n={n} idx={use_idx}: dW {fw:.3f}, db {fb:.3f} of the gate")
    assert fw <= 1.0 and fb <= 1.0 and untouched(bufw, o)
    # bitwise reproducible
    _, dw2, db2 = _backward_weight(ops, device, a, dh, idx_d, n, k, o)
    assert np.array_equal(dw, dw2) and np.array_equal(db, db2)


def test_backward_weight_row_order_changes_rounding_only(device):
    """Another order of the same rows: the same sums within the gate (not bitwise: float32 addition does not associate)."""
    ops = _ops()
    rng = np.random.default_rng(5)
    n, k, o = ops.train_chunk_rows() + 40, 12, 33
    a, dh_table = rng.normal(0, 1, (n, k)).astype(np.float32), rng.normal(0, 1, (n, o)).astype(np.float32)
    want_w, want_b, mag_w, mag_b = T.linear_backward_weight(a, dh_table)
    for order in (np.arange(n), rng.permutation(n), np.arange(n)[::-1].copy()):
        _, dw, db = _backward_weight(ops, device, a, dh_table[order], torch.from_numpy(order.astype(np.int64)).to(device), n, k, o)
        assert worst(dw, want_w, T.dot_bound(n, mag_w)) <= 1.0 and worst(db, want_b, T.dot_bound(n, mag_b)) <= 1.0


def test_one_nan_stays_in_its_column_and_row(device):
    ops = _ops()
    rng = np.random.default_rng(6)
    n, k, o = ops.train_chunk_rows() + 9, 70, 37
    n0, o0 = n - 4, 35
    a, dh, w = rng.normal(0, 1, (n, k)).astype(np.float32), rng.normal(0, 1, (n, o)).astype(np.float32), \
        rng.normal(0, 1, (k, o)).astype(np.float32)
    dh[n0, o0] = np.nan
    _, dw, db = _backward_weight(ops, device, a, dh, None, n, k, o)
    assert np.all(np.isnan(dw[:, o0])) and np.isnan(db[o0])
    assert np.all(np.isfinite(np.delete(dw, o0, axis=1))) and np.all(np.isfinite(np.delete(db, o0)))
    p = rng.uniform(0.5, 1, (n, k)).astype(np.float32)
    _, out = out_view(n, k, device)
    ops.train_linear_backward_data(padded(dh, device), padded(w, device), padded(p, device), out)
    da = out.cpu().numpy()
    assert np.all(np.isnan(da[n0])) and np.all(np.isfinite(np.delete(da, n0, axis=0)))


# ---- loss ------------------------------------------------------------------------------------------------------------------------
def _mse(ops, device, yhat, per_feature, targets, idx_d, n):
    f = yhat.shape[1]
    buf, dy = out_view(n, f, device)
    loss = torch.zeros(1, dtype=torch.float64, device=device)
    ws = torch.zeros(ops.train_loss_workspace_doubles(), dtype=torch.float64, device=device)
    vecs = [torch.from_numpy(np.asarray(v, np.float32)).to(device) for v in per_feature]
    ops.train_mse_grad(padded(yhat, device), *vecs, padded(targets, device), dy, loss, ws, idx=idx_d, n=n)
    return buf, dy.cpu().numpy(), float(loss.cpu()[0])


def _per_feature(rng, f, limits=True):
    keep = (rng.uniform(0, 1, f) > 0.25).astype(np.float32)
    keep[0] = 1.0
    if f > 1:
        keep[-1] = 0.0
    scale, center = rng.uniform(0.5, 2, f).astype(np.float32), rng.normal(0, 1, f).astype(np.float32)
    inv = (keep / rng.uniform(0.5, 2, f) ** 2).astype(np.float32)
    lo = np.where(rng.uniform(0, 1, f) < 0.5, -0.8, -np.inf).astype(np.float32) if limits else np.full(f, -np.inf, np.float32)
    hi = np.where(rng.uniform(0, 1, f) < 0.5, 0.9, np.inf).astype(np.float32) if limits else np.full(f, np.inf, np.float32)
    return scale, center, inv, lo, hi, keep


@pytest.mark.parametrize("n,f", [(1, 1), (31, 8), (33, 33), (512, 158), (512, 396), (2050, 12)])
def test_mse_grad(device, n, f):
    ops = _ops()
    rng = np.random.default_rng(n + f)
    scale, center, inv, lo, hi, keep = _per_feature(rng, f)
    wnorm = (1.0 / (n * max(keep.sum(), 1.0)) * np.ones(f)).astype(np.float32)
    yhat, table = rng.normal(0, 1, (n, f)).astype(np.float32), rng.normal(0, 1, (n + 5, f)).astype(np.float32)
    table[:, keep == 0] = np.nan   # a clipped-away target is never read
    idx, idx_d = make_idx(rng, n, n + 5, device)
    buf, dy, loss = _mse(ops, device, yhat, (scale, center, inv, lo, hi, keep, wnorm), table, idx_d, n)
    want, want_loss, bound = T.mse_grad(yhat, scale, center, inv, lo, hi, keep, wnorm, table, idx)
    # an element within rounding of a limit may fall on either side of it: there the gate is the whole term
    p = yhat.astype(np.float64) * scale + center
    near = (np.abs(p - lo) <= 4 * T.U * (np.abs(p) + np.abs(center))) | (np.abs(p - hi) <= 4 * T.U * (np.abs(p) + np.abs(center)))
    assert not near.any(), "the random case should sit clear of its limits"
    frac = worst(dy, want, bound + 1e-37)
    # the loss: d = clamp(p) - t is float32, known to within ed = 4 2^-24 (|yhat scale| + |center| + |t|); its square is
    # summed in float64, so a term is off by at most (2 |d| ed + ed^2) inv_cstd2 wnorm
    t64 = np.nan_to_num(T.rows(table, idx))
    d, ed = np.abs(np.clip(p, lo, hi) - t64), 4 * T.U * (np.abs(yhat.astype(np.float64) * scale) + np.abs(center) + np.abs(t64))
    loss_gate = np.sum(np.where(keep != 0, (2 * d * ed + ed * ed) * inv * wnorm, 0.0)) + 1e-14 * abs(want_loss)
    print(f"mse grad n={n} f={f}: {frac:.3f} of the gate; loss {loss} vs {want_loss}, {abs(loss - want_loss) / loss_gate:.3f} of its gate")
    assert frac <= 1.0 and untouched(buf, f)
    assert abs(loss - want_loss) <= loss_gate
    assert np.all(dy[:, keep == 0] == 0), "a clipped-away feature has an exact 0 gradient"
    buf2, dy2, loss2 = _mse(ops, device, yhat, (scale, center, inv, lo, hi, keep, wnorm), table, idx_d, n)
    assert np.array_equal(dy, dy2) and loss == loss2, "bitwise reproducible"


def test_mse_grad_limits_are_inclusive(device):
    """scale 1, center 0: p is yhat exactly.  At lo and at hi the gradient passes; one ulp outside it does not."""
    ops = _ops()
    lo, hi = np.float32(-0.5), np.float32(0.75)
    yhat = np.array([[lo, hi, np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(1)), 0.1]], np.float32)
    f = yhat.shape[1]
    t = np.full((1, f), 2.0, np.float32)
    one = np.ones(f, np.float32)
    _, dy, loss = _mse(ops, device, yhat, (one, 0 * one, one, lo * one, hi * one, one, one / f), t, None, 1)
    want = 2 * (np.clip(yhat, lo, hi).astype(np.float64) - 2.0) / f
    assert dy[0, 2] == 0 and dy[0, 3] == 0
    assert np.allclose(dy[0, [0, 1, 4]], want[0, [0, 1, 4]], rtol=8 * T.U, atol=0)
    assert abs(loss - np.sum((np.clip(yhat, lo, hi).astype(np.float64) - 2.0) ** 2) / f) <= 1e-6


def test_mse_grad_keep_and_denominator(device):
    """keep = 0 gives an exact 0 and the loss is the mean over the kept features only."""
    ops = _ops()
    f, n = 4, 3
    one = np.ones(f, np.float32)
    keep = np.float32([1, 0, 1, 0])
    yhat, t = np.float32([[1, 50, 2, 50]] * n), np.float32([[0, np.inf, 0, np.nan]] * n)
    _, dy, loss = _mse(ops, device, yhat, (one, 0 * one, one, -np.inf * one, np.inf * one, keep, one / (n * 2)), t, None, n)
    assert np.all(dy[:, [1, 3]] == 0) and loss == pytest.approx((1 + 4) / 2, rel=1e-7)
    assert np.allclose(dy[:, 0], 2 * 1 / (n * 2)) and np.allclose(dy[:, 2], 2 * 2 / (n * 2))


def test_mse_grad_inf_target(device):
    ops = _ops()
    f, n = 3, 40
    one = np.ones(f, np.float32)
    yhat, t = np.zeros((n, f), np.float32), np.zeros((n, f), np.float32)
    t[17, 1] = np.inf
    _, dy, loss = _mse(ops, device, yhat, (one, 0 * one, one, -np.inf * one, np.inf * one, one, one / (n * f)), t, None, n)
    assert loss == np.inf and dy[17, 1] == -np.inf and np.all(np.isfinite(np.delete(dy.reshape(-1), 17 * f + 1)))


# ---- Adam ------------------------------------------------------------------------------------------------------------------------
def _adam_case(rng, count=1000):
    p0 = rng.normal(0, 1, count).astype(np.float32)
    grads = []
    for _ in range(3):
        g = (rng.normal(0, 1, count) * 10.0 ** rng.integers(-4, 2, count)).astype(np.float32)
        g[:8] = [0.0, 1e-20, -1e-20, 1e4, -1e4, 0.0, 1e4, -1e-20]
        grads.append(g)
    return p0, grads


def test_adam_matches_torch(device):
    ops = _ops()
    p0, grads = _adam_case(np.random.default_rng(7))
    tp = torch.from_numpy(p0.copy()).requires_grad_()
    opt = torch.optim.Adam([tp], lr=1e-3)
    p = torch.from_numpy(p0.copy()).to(device)
    m, v, step = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(1, dtype=torch.int64, device=device)
    for t, g in enumerate(grads, start=1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        ops.train_adam(p, torch.from_numpy(g).to(device), m, v, step)
        want = tp.detach().numpy()
        ulps = np.abs(p.cpu().numpy().astype(np.float64) - want) / np.spacing(np.abs(want))
        print(f"adam step {t}: worst {ulps.max():.2f} ulp")
        assert ulps.max() <= 2.0
        assert int(step.cpu()[0]) == t


def test_adam_replay_advances_the_step(device):
    ops = _ops()
    p0, grads = _adam_case(np.random.default_rng(8))
    g = torch.from_numpy(grads[0]).to(device)

    def fresh():
        p = torch.from_numpy(p0.copy()).to(device)
        return p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros(1, dtype=torch.int64, device=device)

    p, m, v, step = fresh()
    for _ in range(3):
        ops.train_adam(p, g, m, v, step)
    eager = p.cpu().numpy()

    p, m, v, step = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.train_adam(p, g, m, v, step)
    assert int(step.cpu()[0]) == 0, "capturing runs nothing"
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(step.cpu()[0]) == 3
    assert np.array_equal(p.cpu().numpy(), eager)
