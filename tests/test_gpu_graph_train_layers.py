"""The entry points of csrc/graph_train.hip and ``fv3hip_train_adamw``, one by one, against the float64 restatement
(tests/graph_train_np.py).

Shapes are the smallest at which the kernels can go wrong: nx in {2, 4, 6, 16, 18, 34} (every cell one step from a seam; the
16 x 16 spatial tile's edge and one past it), channels in {1, 3, 8, 9, 32, 33, 65} (the 8-channel chunk, the 32 / 64 column
tiles and one past them), S in {1, 2}, and batches of fewer cells than ``graph_train_chunk_cells()`` (512), of a whole number of
chunks (nx = 16: 1536) and of one chunk and a few cells (nx = 2, S = 22: 528; a cube has 6 n^2 cells, so no batch has exactly
512).  Every operand sits at a channel offset of a wider buffer whose other channels are NaN (inputs) or a sentinel (outputs).

Gates (derived): a float32 contraction of length n in any order ``2 n 2^-24 sum |a_i| |b_i|``; mean5 six
roundings on ``mean5(|x|)``; the tanh mask four roundings on ``|v| (1 + p^2)``; a sum of two terms one rounding each way.  The
stored activation P is the same float32 array on both sides, so no mask is in doubt here.  Every test prints its worst
fraction of its gate."""
import numpy as np
import pytest
import torch

import graph_train_np as G

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
ACT = {"linear": 0, "relu": 1, "tanh": 2}


def _ops():
    from fv3net_amd import ops

    return ops


def _slice(t, ld, off=0):
    from fv3net_amd.cube import _Slice

    return _Slice(t, ld, off)


def placed(a, device, off=2, pad=3, fill=float("nan")):
    """``a`` ``[S, 6, n, n, c]`` on the device at channel ``off`` of a buffer ``off + c + pad`` wide -> (slice, buffer)."""
    a = np.asarray(a, np.float32)
    buf = torch.full(a.shape[:-1] + (off + a.shape[-1] + pad,), fill, dtype=torch.float32, device=device)
    buf[..., off:off + a.shape[-1]] = torch.from_numpy(a).to(device)
    return _slice(buf, buf.shape[-1], off), buf


def taken(buf, off, c):
    """(the slice's values, whether everything else still holds the sentinel)"""
    host = buf.cpu().numpy()
    rest = np.concatenate([host[..., :off], host[..., off + c:]], axis=-1)
    return host[..., off:off + c], bool(np.all(rest == SENTINEL))


def worst(got, want, gate):
    assert np.all(np.isfinite(got)), "non-finite result"
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / gate))


def f32(a):
    return np.asarray(a, np.float32)


def post_activation(rng, shape, act):
    """A stored output of ``act``: relu with exact zeros, tanh inside (-1, 1)."""
    z = rng.normal(0, 1, shape)
    return f32(np.maximum(z, 0) if act == "relu" else np.tanh(z) if act == "tanh" else z)


# (nx, c_in, c_out, S)
SAGE = [(2, 1, 1, 1), (4, 3, 8, 2), (6, 9, 3, 1), (16, 8, 33, 1), (18, 33, 9, 2), (34, 65, 32, 1), (6, 32, 65, 2), (4, 65, 65, 1),
        (2, 3, 3, 21), (2, 3, 3, 22)]


@pytest.mark.parametrize("act", ["relu", "tanh", None])
@pytest.mark.parametrize("n,ci,co,S", SAGE)
def test_sage_backward_data(device, n, ci, co, S, act):
    ops, rng = _ops(), np.random.default_rng(n * 1000 + ci * 10 + co)
    dh = f32(rng.normal(0, 1, (S, 6, n, n, co)))
    ws, wn = (f32(rng.normal(0, 1, (ci, co)) / np.sqrt(2 * co)) for _ in range(2))
    p = post_activation(rng, (S, 6, n, n, ci), act) if act else None
    want, gate = G.sage_backward_data(dh, ws, wn, p, act or "linear")
    dh_s, _ = placed(dh, device)
    p_s = placed(p, device, off=1, pad=2)[0] if act else None
    dst_s, dst = placed(np.zeros((S, 6, n, n, ci)), device, off=3, pad=1, fill=SENTINEL)
    dst[..., 3:3 + ci] = SENTINEL
    up = lambda a: torch.from_numpy(a).to(device)
    ops.graph_sage_backward_data(dh_s, up(ws), up(wn), p_s, ACT[act or "linear"], dst_s, S, n, ci, co)
    got, clean = taken(dst, 3, ci)
    frac = worst(got, want, gate)
    print(f"sage backward data nx {n} {ci}<-{co} S {S} {act}: worst {frac:.3f} of the gate")
    assert clean and frac <= 1.0
    if act == "relu":
        assert np.all(got[p <= 0] == 0)   # relu'(0) = 0


def test_sage_backward_data_accumulates(device):
    ops, rng = _ops(), np.random.default_rng(0)
    n, ci, co, S = 6, 3, 9, 2
    dh, old = f32(rng.normal(0, 1, (S, 6, n, n, co))), f32(rng.normal(0, 1, (S, 6, n, n, ci)))
    ws, wn = (f32(rng.normal(0, 1, (ci, co)) / np.sqrt(2 * co)) for _ in range(2))
    want, gate = G.sage_backward_data(dh, ws, wn)
    dst_s, dst = placed(old, device, off=1, pad=1, fill=SENTINEL)
    up = lambda a: torch.from_numpy(a).to(device)
    ops.graph_sage_backward_data(placed(dh, device)[0], up(ws), up(wn), None, 0, dst_s, S, n, ci, co, accumulate=True)
    got, clean = taken(dst, 1, ci)
    frac = worst(got, old + want, gate + 2 * G.U * np.abs(old + want))
    print(f"accumulated: worst {frac:.3f} of the gate")
    assert clean and frac <= 1.0


# accumulation on one direct and one chunked shape
@pytest.mark.parametrize("n,ci,co,S,accumulate", [c + (False,) for c in SAGE] + [(4, 3, 8, 2, True), (16, 8, 33, 1, True)])
def test_sage_backward_weight(device, n, ci, co, S, accumulate):
    ops, rng = _ops(), np.random.default_rng(n * 1000 + ci * 10 + co)
    x, g = f32(rng.normal(0, 1, (S, 6, n, n, ci))), f32(rng.normal(0, 1, (S, 6, n, n, co)))
    dws, dwn, db, gs, gn, gb = G.sage_backward_weight(x, g)
    old = [f32(rng.normal(0, 1, a.shape)) if accumulate else np.zeros(a.shape, np.float32) for a in (dws, dwn, db)]
    outs = [torch.from_numpy(o.copy()).to(device) if accumulate else torch.full(o.shape, SENTINEL, device=device) for o in old]
    floats = ops.graph_sage_backward_weight_workspace_floats(S, n, ci, co)
    cells = S * 6 * n * n
    assert (floats == 0) == (cells <= ops.graph_train_chunk_cells())
    ws = torch.full((floats,), float("nan"), device=device) if floats else None
    ops.graph_sage_backward_weight(placed(x, device)[0], placed(g, device, off=1)[0], *outs, S, n, ci, co, workspace=ws,
                                   accumulate=accumulate)
    for name, got, want, gate, o in zip(("dW_self", "dW_neigh", "db"), outs, (dws, dwn, db), (gs, gn, gb), old):
        frac = worst(got.cpu().numpy(), o + want, gate + (2 * G.U * np.abs(o + want) if accumulate else 0))
        print(f"sage backward weight nx {n} {ci}->{co} S {S} ({cells} cells) {name}: worst {frac:.3f} of the gate")
        assert frac <= 1.0


def test_sage_backward_weight_without_bias(device):
    ops, rng = _ops(), np.random.default_rng(1)
    n, ci, co, S = 4, 3, 5, 1
    x, g = f32(rng.normal(0, 1, (S, 6, n, n, ci))), f32(rng.normal(0, 1, (S, 6, n, n, co)))
    a, b = (torch.full((ci, co), SENTINEL, device=device) for _ in range(2))
    ops.graph_sage_backward_weight(placed(x, device)[0], placed(g, device)[0], a, b, None, S, n, ci, co)
    dws, dwn, _, gs, gn, _ = G.sage_backward_weight(x, g)
    assert worst(a.cpu().numpy(), dws, gs) <= 1.0 and worst(b.cpu().numpy(), dwn, gn) <= 1.0


# (n of low, c_in, c_out, S): the gradient lives on 2 n cells per edge
UP = [(1, 1, 1, 1), (2, 8, 3, 2), (3, 9, 8, 1), (8, 33, 9, 1), (9, 32, 33, 2), (17, 65, 8, 1), (3, 3, 65, 2), (1, 3, 3, 86)]


@pytest.mark.parametrize("act", ["relu", "tanh", None])
@pytest.mark.parametrize("n,ci,co,S", UP)
def test_up2_backward_data(device, n, ci, co, S, act):
    ops, rng = _ops(), np.random.default_rng(n * 1000 + ci * 10 + co)
    dcat = f32(rng.normal(0, 1, (S, 6, 2 * n, 2 * n, co)))
    w = f32(rng.normal(0, 1, (ci, 2, 2, co)) / np.sqrt(4 * co))
    p = post_activation(rng, (S, 6, n, n, ci), act) if act else None
    want, gate = G.up2_backward_data(dcat, w, p, act or "linear")
    dst_s, dst = placed(np.zeros((S, 6, n, n, ci)), device, off=2, pad=2, fill=SENTINEL)
    dst[..., 2:2 + ci] = SENTINEL
    ops.graph_up2_backward_data(placed(dcat, device, off=co)[0], torch.from_numpy(w).to(device),
                                placed(p, device, off=1)[0] if act else None, ACT[act or "linear"], dst_s, S, n, ci, co)
    got, clean = taken(dst, 2, ci)
    frac = worst(got, want, gate)
    print(f"up2 backward data n {n} {ci}<-{co} S {S} {act}: worst {frac:.3f} of the gate")
    assert clean and frac <= 1.0


# accumulation on a one-chunk and a many-chunk shape
@pytest.mark.parametrize("n,ci,co,S,accumulate", [c + (False,) for c in UP] + [(2, 8, 3, 2, True), (17, 65, 8, 1, True)])
def test_up2_backward_weight(device, n, ci, co, S, accumulate):
    ops, rng = _ops(), np.random.default_rng(n * 1000 + ci * 10 + co)
    low, dcat = f32(rng.normal(0, 1, (S, 6, n, n, ci))), f32(rng.normal(0, 1, (S, 6, 2 * n, 2 * n, co)))
    dw, db, gw, gb = G.up2_backward_weight(low, dcat)
    old = [f32(rng.normal(0, 1, a.shape)) if accumulate else np.zeros(a.shape, np.float32) for a in (dw, db)]
    outs = [torch.from_numpy(o.copy()).to(device) if accumulate else torch.full(o.shape, SENTINEL, device=device) for o in old]
    ws = torch.full((ops.graph_up2_backward_weight_workspace_floats(S, n, ci, co),), float("nan"), device=device)
    ops.graph_up2_backward_weight(placed(low, device)[0], placed(dcat, device, off=co)[0], *outs, S, n, ci, co, ws, accumulate=accumulate)
    for name, got, want, gate, o in zip(("dW", "db"), outs, (dw, db), (gw, gb), old):
        frac = worst(got.cpu().numpy(), o + want, gate + (2 * G.U * np.abs(o + want) if accumulate else 0))
        print(f"up2 backward weight n {n} {ci}->{co} S {S} {name}: worst {frac:.3f} of the gate")
        assert frac <= 1.0


@pytest.mark.parametrize("act", ["relu", "tanh", None])
@pytest.mark.parametrize("n,c,S", [(2, 1, 1), (4, 3, 2), (6, 9, 1), (18, 33, 2), (34, 8, 1)])
def test_pool2_backward(device, n, c, S, act):
    ops, rng = _ops(), np.random.default_rng(n * 100 + c)
    old, dpool = f32(rng.normal(0, 1, (S, 6, n, n, c))), f32(rng.normal(0, 1, (S, 6, n // 2, n // 2, c)))
    p = post_activation(rng, old.shape, act) if act else None
    want, gate = G.pool2_backward(old, dpool, p, act or "linear")
    dst_s, dst = placed(old, device, off=0, pad=c, fill=SENTINEL)   # the first half of a cat gradient
    ops.graph_pool2_backward(placed(dpool, device)[0], placed(p, device, off=0, pad=c)[0] if act else None, ACT[act or "linear"], dst_s,
                             S, n, c)
    got, clean = taken(dst, 0, c)
    frac = worst(got, want, gate)
    print(f"pool2 backward nx {n} c {c} S {S} {act}: worst {frac:.3f} of the gate")
    assert clean and frac <= 1.0
    if act is None:   # one exact product and one sum: the float32 expression itself
        spread = np.repeat(np.repeat(dpool, 2, axis=2), 2, axis=3)
        assert np.array_equal(got, old + np.float32(0.25) * spread)


@pytest.mark.parametrize("n", [2, 4, 6, 16, 18, 34])
def test_five_cell_sums_are_exact_in_the_adjoint_direction(device, n):
    """W_self = 0, W_neigh = 5 I (its transpose likewise), integer G: dX is the exact five-cell sum of G across the seams."""
    ops, rng = _ops(), np.random.default_rng(n)
    c, S = 3, 2
    g = rng.integers(-50, 51, (S, 6, n, n, c)).astype(np.float32)
    dst = torch.full((S, 6, n, n, c), SENTINEL, device=device)
    ops.graph_sage_backward_data(placed(g, device)[0], torch.zeros((c, c), device=device), 5 * torch.eye(c, device=device), None, 0,
                                 _slice(dst, c), S, n, c, c)
    assert np.array_equal(dst.cpu().numpy(), G.sum5(g))


def test_one_nan_reaches_its_cell_its_neighbours_and_its_column(device):
    ops, rng = _ops(), np.random.default_rng(4)
    n, ci, co, S = 18, 9, 33, 2
    x, g = f32(rng.normal(0, 1, (S, 6, n, n, ci))), f32(rng.normal(0, 1, (S, 6, n, n, co)))
    ws, wn = (f32(rng.normal(0, 1, (ci, co))) for _ in range(2))
    s0, t0, x0, y0, ch = 1, 2, 0, 17, 32   # a corner cell: two of its neighbours lie on other tiles
    bad = g.copy()
    bad[s0, t0, x0, y0, ch] = np.nan
    up = lambda a: torch.from_numpy(a).to(device)
    floats = ops.graph_sage_backward_weight_workspace_floats(S, n, ci, co)

    def run(grad):
        dx = torch.zeros((S, 6, n, n, ci), device=device)
        dws, dwn, db = torch.zeros((ci, co), device=device), torch.zeros((ci, co), device=device), torch.zeros(co, device=device)
        ops.graph_sage_backward_data(placed(grad, device)[0], up(ws), up(wn), None, 0, _slice(dx, ci), S, n, ci, co)
        ops.graph_sage_backward_weight(placed(x, device)[0], placed(grad, device)[0], dws, dwn, db, S, n, ci, co,
                                       workspace=torch.zeros(floats, device=device))
        return [t.cpu().numpy() for t in (dx, dws, dwn, db)]

    clean, dirty = run(g), run(bad)
    cells = G.table(n)[(t0 * n + x0) * n + y0]
    hit = np.zeros((S, 6 * n * n), bool)
    hit[s0, cells] = True
    assert len(set(cells.tolist())) == 5
    nan_dx = np.isnan(dirty[0]).reshape(S, 6 * n * n, ci)
    assert np.array_equal(nan_dx, np.broadcast_to(hit[:, :, None], nan_dx.shape))
    assert np.array_equal(dirty[0].reshape(S, -1, ci)[~hit], clean[0].reshape(S, -1, ci)[~hit])
    for d, c in zip(dirty[1:3], clean[1:3]):
        assert np.all(np.isnan(d[:, ch])) and np.array_equal(np.delete(d, ch, axis=1), np.delete(c, ch, axis=1))
    assert np.isnan(dirty[3][ch]) and np.array_equal(np.delete(dirty[3], ch), np.delete(clean[3], ch))
    assert not any(np.isnan(c).any() for c in clean)


def test_a_layer_that_reads_what_it_writes_is_refused(device):
    from fv3net_amd import _lib

    ops = _ops()
    n, c, S = 4, 3, 1
    buf = torch.zeros((S, 6, n, n, 2 * c), device=device)
    w = torch.zeros((c, c), device=device)
    with pytest.raises(_lib.Fv3HipError, match="overlap") as e:
        ops.graph_sage_backward_data(_slice(buf, 2 * c, 0), w, w, None, 0, _slice(buf, 2 * c, 1), S, n, c, c)
    assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.Fv3HipError, match="overlap"):
        ops.graph_pool2_backward(_slice(buf, 2 * c, 0), None, 0, _slice(buf, 2 * c, 0), S, 2, c)
    with pytest.raises(_lib.Fv3HipError) as e:
        ops.graph_sage_backward_data(_slice(buf, 2 * c, 0), w, w, None, 7, _slice(buf, 2 * c, c), S, n, c, c)
    assert e.value.code == _lib.EUNSUPPORTED
    ops.graph_sage_backward_data(_slice(buf, 2 * c, 0), w, w, None, 0, _slice(buf, 2 * c, c), S, n, c, c)   # disjoint halves: fine
    torch.cuda.synchronize(device)


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_adamw_matches_torch(device, weight_decay):
    """Three steps with gradients 0, +-1e-20, +-1e4: bit-identical to the float32 restatement of torch's CPU kernels (which
    tests/test_host_graph_train.py holds bitwise to torch's single-tensor path) and within 2 float32 ulp of
    ``torch.optim.AdamW`` on the host CPU (section 21's gate).  The ulp is the result's, so the parameters start at 1 <= |p| < 2,
    where an update of at most 3e-3 cannot cancel them: torch's AVX512 kernels associate ``step_size m / denom`` differently
    from its scalar ones, one rounding of the update, which is several ulp of a result that has shrunk below the update (with
    p ~ N(0, 1): 4 ulp at 3 of 1000 elements, all with |p| < 3e-3, the moments bitwise equal)."""
    ops, rng = _ops(), np.random.default_rng(6)
    count = 1000
    p0 = f32(rng.choice([-1.0, 1.0], count) * rng.uniform(1, 2, count))
    ref = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=weight_decay)
    p, m, v = torch.from_numpy(p0.copy()).to(device), torch.zeros(count, device=device), torch.zeros(count, device=device)
    step = torch.zeros(1, dtype=torch.int64, device=device)
    mine, mm, vv = p0.copy(), np.zeros(count, np.float32), np.zeros(count, np.float32)
    for t in range(1, 4):
        g = rng.choice(np.array([0.0, 1e-20, -1e-20, 1e4, -1e4], np.float32), count)
        ref.grad = torch.from_numpy(g.copy())
        opt.step()
        ops.train_adamw(p, torch.from_numpy(g).to(device), m, v, step, weight_decay=weight_decay)
        mine, mm, vv = G.adamw_f32(mine, g, mm, vv, t, weight_decay=weight_decay)
        got, want = p.cpu().numpy(), ref.detach().numpy()
        ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want))
        print(f"adamw step {t}, weight decay {weight_decay}: worst {ulps.max():.2f} ulp; bitwise {np.array_equal(got, mine)}")
        assert ulps.max() <= 2.0
        assert np.array_equal(got, mine) and np.array_equal(m.cpu().numpy(), mm) and np.array_equal(v.cpu().numpy(), vv)
    assert int(step.cpu()[0]) == 3
