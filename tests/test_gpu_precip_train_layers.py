"""``fv3hip_train_precip_loss_grad`` on its own (csrc/mlp_train.hip) against tests/precip_train_np.py.

The kernel gives one wave to a batch row, four rows to a block and walks the levels 64 at a time; the grid holds at most 1 024
blocks, so a batch of more than 4 096 rows takes the grid-stride path.  The shapes sit at those edges: levels 1, 2, 63, 64, 65, 79
and 130 (three strips), rows 1 to 5, 255 to 257, 513 and 4 097.  Every level count runs with two row counts and every row count
with 79 levels; the leading dimensions, the row table, the coupling and the regulariser cycle over the cases and
``test_every_argument_is_exercised`` checks that each value occurs."""
import numpy as np
import pytest
import torch

import precip_train_cases as C
import precip_train_np as PT
import precipitative_cases as PC
import precipitative_np as P
from fv3net_amd import _lib, ops

pytestmark = pytest.mark.gpu

NZS = (1, 2, 63, 64, 65, 79, 130)
NS = (1, 2, 3, 4, 5, 255, 256, 257, 513)
SHAPES = [(n, nz) for nz in NZS for n in (5, 257)] + [(n, 79) for n in NS if n not in (5, 257)] + [(4097, 2)]
PADS = (0, 3)
IDX_KINDS = ("none", "repeats", "out_of_range")
REGS = {"none": (0.0, 0.0, False), "l1": (0.01, 0.0, True), "l2": (0.0, 0.01, True), "l1_l2": (0.02, 0.01, True), "no_dead_l2": (0.0, 0.01, False),
        "dead_unregularised": (0.0, 0.0, True)}
SENTINEL = 7.5


def variant(i):
    """(padding of every leading dimension, row table, couple, regulariser) of case ``i``."""
    return PADS[i % 2], IDX_KINDS[i % 3], (i // 2) % 2 == 0, list(REGS)[(i // 3) % len(REGS)]


CASES = [(n, nz) + variant(i) for i, (n, nz) in enumerate(SHAPES)]


def test_every_argument_is_exercised():
    for pos, values in ((2, PADS), (3, IDX_KINDS), (4, (True, False)), (5, tuple(REGS))):
        assert {c[pos] for c in CASES} == set(values)


def _padded(a, pad, device):
    """``a`` [rows, f] as a view of a [rows, f + pad] device tensor filled with the sentinel."""
    full = torch.full((a.shape[0], a.shape[1] + pad), SENTINEL, dtype=torch.float32, device=device)
    full[:, :a.shape[1]] = torch.from_numpy(a).to(device)
    return full, full[:, :a.shape[1]]


def launch(a, device, idx=None, couple=True, has_dead=False, l1=0.0, l2=0.0, pad=0, predictions=True):
    """One launch on the arrays of ``precip_train_cases.launch_inputs``; everything read back as numpy."""
    n, f = a["yhat"].shape
    nz = a["scale1"].shape[0]
    dv = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(device)   # noqa: E731
    _, yhat = _padded(a["yhat"], pad, device)
    _, delp = _padded(a["delp"], pad, device)
    _, t12 = _padded(np.concatenate([a["t1"], a["t2"]], axis=1), pad, device)
    dy_full, dy = _padded(np.full((n, f), SENTINEL, np.float32), pad, device)
    loss = torch.zeros(1, dtype=torch.float64, device=device)
    ws = torch.zeros(ops.train_loss_workspace_doubles(), dtype=torch.float64, device=device)
    dq1 = torch.full((n, nz), SENTINEL, dtype=torch.float32, device=device) if predictions else None
    dq2 = torch.full((n, nz), SENTINEL, dtype=torch.float32, device=device) if predictions else None
    precip = torch.full((n,), SENTINEL, dtype=torch.float32, device=device) if predictions else None
    ops.train_precip_loss_grad(yhat, dv(a["scale1"]), dv(a["center1"]), dv(a["scale2"]), dv(a["center2"]), dv(a["inv1"]), dv(a["inv2"]),
                               a["inv3"], delp, dv(a["pp"]), t12[:, :nz], t12[:, nz:], dv(a["t3"]), dy, loss, ws,
                               idx=None if idx is None else dv(np.asarray(idx, np.int64)), couple=couple, has_dead=has_dead, l1=l1, l2=l2,
                               dq1=dq1, dq2=dq2, precip=precip)
    torch.cuda.synchronize()
    out = dict(dy_full=dy_full.cpu().numpy(), dy=dy.cpu().numpy(), loss=float(loss.cpu()[0]))
    if predictions:
        out.update(dq1=dq1.cpu().numpy(), dq2=dq2.cpu().numpy(), precip=precip.cpu().numpy())
    return out


def heads32(a, has_dead):
    """The de-normalised heads ``[nz, n]`` as a float32 product and sum give them (what the kernel hands its closure)."""
    nz = a["scale1"].shape[0]
    y = a["yhat"]
    cp0 = 2 * nz + int(has_dead)
    return ((y[:, :nz] * a["scale1"] + a["center1"]).T, (y[:, nz:2 * nz] * a["scale2"] + a["center2"]).T,
            (y[:, cp0:] * a["scale2"] + a["center2"]).T)


def resident(a, idx):
    """(delp [n, nz], pp [n]) as the batch reads them: rows ``idx``, zeros for an index out of range."""
    if idx is None:
        n = a["yhat"].shape[0]
        return a["delp"][:n], a["pp"][:n]
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < a["delp"].shape[0])
    safe = np.where(ok, idx, 0)
    return np.where(ok[:, None], a["delp"][safe], np.float32(0)), np.where(ok, a["pp"][safe], np.float32(0))


def assert_within(got, want, gate, what):
    """Elementwise ``|got - want| <= gate``; a NaN of the reference must be a NaN of the kernel.  Returns the worst fraction."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs in other places than the reference's"
    if nan.all():
        return 0.0
    frac = float(np.max(np.abs(got - want)[~nan] / gate[~nan]))
    assert frac <= 1.0, f"{what}: {frac:.3f} of the gate"
    return frac


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("n,nz,pad,idx_kind,couple,reg", CASES, ids=[f"n{c[0]}-nz{c[1]}-pad{c[2]}-{c[3]}-{'coupled' if c[4] else 'uncoupled'}-{c[5]}" for c in CASES])
def test_loss_grad(device, n, nz, pad, idx_kind, couple, reg):
    l1, l2, has_dead = REGS[reg]
    rows = n if idx_kind == "none" else n + 3
    a = C.launch_inputs(n, nz, has_dead=has_dead, rows=rows, seed=1)
    idx = None
    if idx_kind != "none":
        idx = np.random.default_rng([n, nz]).integers(0, rows, n)
        idx[: n // 2] = idx[n // 2: 2 * (n // 2)]   # repeats for certain
        if idx_kind == "out_of_range":
            idx[n // 3] = rows if n % 2 else -1
    got = launch(a, device, idx=idx, couple=couple, has_dead=has_dead, l1=l1, l2=l2, pad=pad)
    want, loss, gate, loss_gate, _ = PT.loss_grad(*C.reference_args(a), idx=idx, couple=couple, has_dead=has_dead, l1=l1, l2=l2)

    frac = assert_within(got["dy"], want, gate, "dY")
    finite = np.isfinite(want)
    rel = float(np.max(gate[finite]) / np.max(np.abs(want[finite]))) if finite.any() else float("nan")
    print(f"dY: {frac:.3f} of the gate (the gate is {rel:.1e} of the largest entry)")
    if idx_kind == "out_of_range":
        bad = n // 3
        assert np.isnan(got["loss"]) and np.isnan(loss), "a target row out of range reads as NaN"
        assert np.all(np.isnan(got["dy"][bad, 2 * nz + int(has_dead):]))
        assert np.all(np.isfinite(np.delete(got["dy"], bad, axis=0)))
    else:
        print(f"loss {got['loss']} vs {loss}: {abs(got['loss'] - loss) / loss_gate:.3f} of its gate")
        assert abs(got["loss"] - loss) <= loss_gate
        assert np.all(np.isfinite(got["dy"]))
    if has_dead and not (l1 or l2):
        assert np.all(got["dy"][:, 2 * nz] == 0)

    # the predictions: the predictor's bits on the same heads (out of range: zero thickness, zero physics_precip)
    t_res, q_res, cp = heads32(a, has_dead)
    delp, pp = resident(a, idx)
    dq1, dq2, precip = P.closure32(t_res, q_res, cp, delp.T, pp, couple)
    assert np.array_equal(bits(got["precip"]), bits(precip))
    assert np.array_equal(bits(got["dq1"]), bits(dq1.T)) and np.array_equal(bits(got["dq2"]), bits(dq2.T))

    again = launch(a, device, idx=idx, couple=couple, has_dead=has_dead, l1=l1, l2=l2, pad=pad, predictions=False)
    assert np.array_equal(bits(again["dy"]), bits(got["dy"])), "two launches, one result (and the prediction outputs are optional)"
    assert np.array_equal(np.float64(again["loss"]).view(np.uint64), np.float64(got["loss"]).view(np.uint64))
    assert np.all(got["dy_full"][:, 3 * nz + int(has_dead):] == SENTINEL), "the padding columns of dY are not written"


def _pairwise(x):
    """A float32 tree sum over axis 0."""
    x = [r for r in x]
    while len(x) > 1:
        x = [x[i] + x[i + 1] if i + 1 < len(x) else x[i] for i in range(0, len(x), 2)]
    return x[0]


def test_integral_is_the_predictors_sequential_sum(device):
    """A case where a contracted multiply-add and a tree sum give other bits than the sequential float32 sum of rounded
    products (checked here on the host first, as tests/precipitative_cases.py does for the predictor)."""
    n, nz = 64, 79
    a = C.launch_inputs(n, nz, seed=5)
    _, _, cp = heads32(a, False)
    _, _, want = P.closure32(None, None, cp, a["delp"].T, a["pp"], couple=False)
    fma = PC.fma_precip(cp, a["delp"].T, a["pp"])
    tree = a["pp"] + P.C_G * _pairwise(cp * a["delp"].T)
    assert tree.dtype == np.float32 and np.mean(bits(fma) != bits(want)) > 0.25 and np.mean(bits(tree) != bits(want)) > 0.25
    got = launch(a, device, couple=False)
    assert np.array_equal(bits(got["precip"]), bits(want))


def test_sign_of_zero_is_zero(device):
    n, nz = 5, 3
    a = C.launch_inputs(n, nz, has_dead=True, seed=2)
    a["yhat"][0, 0], a["yhat"][1, 0], a["yhat"][2, 2 * nz] = 0.0, -0.0, 0.0
    l1 = 0.5
    got = launch(a, device, has_dead=True, l1=l1)
    want, loss, gate, loss_gate, _ = PT.loss_grad(*C.reference_args(a), has_dead=True, l1=l1)
    assert_within(got["dy"], want, gate, "dY")
    plain = launch(a, device, has_dead=True)
    for r in (0, 1):   # l1 * 0 / n adds nothing to g1 * scale1
        assert got["dy"][r, 0] == plain["dy"][r, 0] and got["dy"][r, 1] != plain["dy"][r, 1]
    assert got["dy"][2, 2 * nz] == 0 and np.all(np.abs(np.delete(got["dy"][:, 2 * nz], 2)) == np.float32(l1) / np.float32(n))
    assert abs(got["loss"] - loss) <= loss_gate


NONFINITE = [("t", np.nan), ("cp", np.inf), ("delp", -np.inf), ("t1", np.inf), ("t3", np.nan), ("q", -np.inf), ("delp", np.nan), ("t2", np.nan)]


@pytest.mark.parametrize("which,value", NONFINITE, ids=[f"{w}-{v}" for w, v in NONFINITE])
def test_nonfinite_stays_in_its_row(device, which, value):
    """One NaN or inf in ``yhat``, ``delp`` or a target: that row's gradient and the loss are not finite, every other row has the
    bits of the clean launch."""
    n, nz, row, level = 9, 65, 6, 64   # the second wave of the second block, the second strip of levels
    a = C.launch_inputs(n, nz, seed=4)
    clean = launch(a, device)
    column = {"t": level, "q": nz + level, "cp": 2 * nz + level}
    if which in column:
        a["yhat"][row, column[which]] = value
    elif which == "t3":
        a["t3"][row] = value
    else:
        a[which][row, level] = value
    got = launch(a, device)
    others = np.arange(n) != row
    assert np.array_equal(bits(got["dy"][others]), bits(clean["dy"][others]))
    assert not np.isfinite(got["loss"])
    whole_cp_block = which in ("cp", "delp", "t3")   # through the integral into every level of the column-precipitation head
    hit = got["dy"][row, 2 * nz:] if whole_cp_block else got["dy"][row, [{"t": level, "t1": level, "q": nz + level, "t2": nz + level}[which], 2 * nz + level]]
    assert not np.any(np.isfinite(hit)), (which, value)
    want, _, _, _, _ = PT.loss_grad(*C.reference_args(a))
    assert np.array_equal(np.isfinite(got["dy"][row]), np.isfinite(want[row]))


# ---- bad arguments: a negative status, nothing launched ---------------------------------------------------------------------------
def _raw_arguments(device, n=4, nz=3):
    a = C.launch_inputs(n, nz, seed=6)
    f = 3 * nz
    t = {k: torch.from_numpy(np.ascontiguousarray(a[k])).to(device) for k in ("yhat", "scale1", "center1", "scale2", "center2", "inv1", "inv2",
                                                                                "delp", "pp", "t1", "t2", "t3")}
    t["dy"] = torch.full((n, f), SENTINEL, dtype=torch.float32, device=device)
    t["loss"] = torch.full((1,), SENTINEL, dtype=torch.float64, device=device)
    t["ws"] = torch.zeros(ops.train_loss_workspace_doubles(), dtype=torch.float64, device=device)
    p = lambda k: t[k].data_ptr()   # noqa: E731
    args = dict(yhat=p("yhat"), ldy=f, scale1=p("scale1"), center1=p("center1"), scale2=p("scale2"), center2=p("center2"), inv1=p("inv1"),
                inv2=p("inv2"), inv3=a["inv3"], delp=p("delp"), ldd=nz, pp=p("pp"), t1=p("t1"), t2=p("t2"), ldt=nz, t3=p("t3"), rows=n,
                idx=None, couple=1, has_dead=0, l1=0.0, l2=0.0, dy=p("dy"), lddy=f, loss=p("loss"), ws=p("ws"), dq1=None, dq2=None,
                precip=None, n=n, nz=nz, stream=None)
    return args, t


BAD = {"null yhat": dict(yhat=None), "no levels": dict(nz=0), "ldy too small": dict(ldy=8), "negative l1": dict(l1=-0.01),
       "negative l2": dict(l2=-1.0), "NaN l1": dict(l1=float("nan")), "null dY": dict(dy=None), "lddy too small": dict(lddy=8),
       "ldd too small": dict(ldd=2), "ldt too small": dict(ldt=2), "null delp": dict(delp=None), "null T3": dict(t3=None),
       "null loss": dict(loss=None), "null workspace": dict(ws=None), "no rows": dict(n=0), "fewer resident rows than the batch": dict(rows=3),
       "couple 2": dict(couple=2), "has_dead 2": dict(has_dead=2), "null scale2": dict(scale2=None)}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_arguments_are_refused_before_any_launch(device, name):
    ops._require_device(torch.empty(1, device=device))
    lib = _lib.load()
    args, t = _raw_arguments(device)
    assert lib.fv3hip_train_precip_loss_grad(*args.values()) == 0, "the arguments are good before one is spoiled"
    torch.cuda.synchronize()
    assert not np.any(t["dy"].cpu().numpy() == SENTINEL)
    t["dy"].fill_(SENTINEL)
    t["loss"].fill_(SENTINEL)
    args.update(BAD[name])
    status = lib.fv3hip_train_precip_loss_grad(*args.values())
    torch.cuda.synchronize()
    assert status < 0 and lib.fv3hip_last_error(), name
    assert np.all(t["dy"].cpu().numpy() == SENTINEL) and float(t["loss"].cpu()[0]) == SENTINEL, "nothing was launched"


def test_wrapper_checks_shapes(device):
    a = C.launch_inputs(4, 3, seed=6)
    dv = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(device)   # noqa: E731
    good = dict(yhat=dv(a["yhat"]), dy=torch.zeros((4, 9), dtype=torch.float32, device=device), loss=torch.zeros(1, dtype=torch.float64, device=device),
                ws=torch.zeros(ops.train_loss_workspace_doubles(), dtype=torch.float64, device=device))

    def call(**kw):
        g = dict(good, **kw)
        return ops.train_precip_loss_grad(g["yhat"], dv(a["scale1"]), dv(a["center1"]), dv(a["scale2"]), dv(a["center2"]), dv(a["inv1"]),
                                          dv(a["inv2"]), a["inv3"], dv(a["delp"]), dv(a["pp"]), dv(a["t1"]), dv(a["t2"]), dv(a["t3"]), g["dy"],
                                          g["loss"], g["ws"], has_dead=g.get("has_dead", False), l1=g.get("l1", 0.0))

    call()
    with pytest.raises(ValueError):
        call(has_dead=True)        # 9 features are not 3 nz + 1
    with pytest.raises(ValueError):
        call(dy=torch.zeros((4, 10), dtype=torch.float32, device=device))
    with pytest.raises(ValueError):
        call(ws=torch.zeros(3, dtype=torch.float64, device=device))
    with pytest.raises(_lib.Fv3HipError):
        call(l1=-1.0)
    with pytest.raises(RuntimeError):
        call(yhat=torch.from_numpy(a["yhat"]))   # host memory
