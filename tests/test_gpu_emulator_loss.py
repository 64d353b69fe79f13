"""``fv3hip_train_emulator_loss_grad`` on its own (csrc/mlp_train.hip) against tests/emulator_train_np.py.

The kernel gives every head a run of at most 64 blocks of 256 threads, one (network row, column) or one cross-entropy point per
thread, so a head of more than 16 384 elements takes the grid-stride path; the head table holds 16 heads.  The shapes sit at those
edges: batch rows 1, 2, 63, 65, 255, 257 and one count past the grid-stride limit; features / levels 1, 3, 64, 65, 79, 130; 2, 4, 5
and 32 channels; one head and sixteen.  The leading dimensions and the row table cycle over the cases and
``test_every_argument_is_exercised`` checks that each value occurs."""
import dataclasses

import numpy as np
import pytest
import torch

import emulator_train_cases as C
import emulator_train_np as E
from fv3net_amd import _lib, ops

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
NS = (1, 2, 63, 65, 255, 257)
SIZES = (1, 3, 64, 65, 79, 130)
CHANNELS = (2, 4, 5, 32)
PADS = (0, 3)
IDX_KINDS = ("none", "repeats", "out_of_range")
BOTH = dict(scaled=True, direct=("loss", 2.0), after=("loss", 0.5))


def dense_layout(name, nfeat):
    if name == "one":
        return [("mse", nfeat, BOTH)]
    if name == "mixed":
        return [("mse", nfeat, BOTH), ("mse", nfeat, dict(scaled=True, direct=("loss", 1.0), after=("metric", 1.0))),
                ("mse", 1, dict(direct=("loss", 3.0))), ("mse", nfeat, dict(scaled=True)), ("mse", 2, dict(scaled=True, direct=("metric", 1.0)))]
    assert name == "capacity"
    kinds = [BOTH, dict(scaled=True, direct=("loss", 1.0)), dict(direct=("metric", 1.0)), dict(scaled=True, after=("loss", 0.3))]
    return [("mse", 1 + (h % 3) if nfeat > 1 else 1, kinds[h % 4]) for h in range(_lib.EMULATOR_MAX_HEADS)]


def local_layout(channels):
    return [("mse_local", 1, dict(scaled=True, direct=("loss", 1.5), after=("loss", 0.25))),
            ("mse_local", 1, dict(scaled=True, direct=("loss", 0.7), single_level=True)),
            ("xent", channels, dict(direct=("loss", 2.0))), ("mse_local", 1, dict())]


def _cases():
    shapes = [("dense", n, 3, "mixed") for n in NS] + [("dense", 5, f, "mixed") for f in SIZES] + \
             [("dense", 5462, 3, "one"), ("dense", 65, 3, "capacity"), ("dense", 2, 1, "capacity"), ("dense", 257, 79, "one")] + \
             [("local", n, 3, 4) for n in NS] + [("local", 5, nz, 4) for nz in SIZES] + [("local", 3, 5, c) for c in CHANNELS] + \
             [("local", 257, 65, 5)]     # 16 705 points: past the grid-stride limit
    return [s + (PADS[i % 2], IDX_KINDS[i % 3]) for i, s in enumerate(shapes)]


CASES = _cases()


def test_every_argument_is_exercised():
    assert {c[4] for c in CASES} == set(PADS) and {c[5] for c in CASES} == set(IDX_KINDS)
    assert {c[1] for c in CASES} >= set(NS) and {c[2] for c in CASES} >= set(SIZES)
    assert {c[3] for c in CASES if c[0] == "local"} == set(CHANNELS) and {c[3] for c in CASES if c[0] == "dense"} == {"one", "mixed", "capacity"}
    limit = 64 * 256
    assert any(c[0] == "dense" and c[1] * c[2] > limit for c in CASES) and any(c[0] == "local" and c[1] * c[2] > limit for c in CASES)


def build(mode, n, size, layout, idx_kind, seed=0):
    """``(heads, levels, F, yhat, idx)`` as numpy."""
    rng = np.random.default_rng(seed)
    levels = size if mode == "local" else 1
    rows = n if idx_kind == "none" else max(2, n // 2 + 1)
    heads, f = C.make_heads(rng, rows, levels, dense_layout(layout, size) if mode == "dense" else local_layout(layout))
    yhat = rng.normal(0, 1, (n * levels, f)).astype(np.float32)
    idx = None
    if idx_kind != "none":
        idx = rng.integers(0, rows, n).astype(np.int64)
        if idx_kind == "out_of_range":
            idx[n // 2] = rows if n % 2 else -1
    return heads, levels, f, yhat, idx


def _padded(a, pad, device):
    """``a`` [rows, ...] as a view of a [rows, size + pad] device tensor filled with the sentinel."""
    flat = a.reshape(a.shape[0], -1)
    full = torch.full((flat.shape[0], flat.shape[1] + pad), SENTINEL, dtype=torch.float32, device=device)
    full[:, :flat.shape[1]] = torch.from_numpy(np.ascontiguousarray(flat)).to(device)
    view = full[:, :flat.shape[1]]
    return full, (view.unflatten(1, a.shape[1:]) if a.ndim > 2 else view)


def device_table(heads, levels, pad, device):
    dv = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(device)   # noqa: E731
    res = lambda v: None if v is None else _padded(v if v.ndim > 1 else v[:, None], pad, device)[1]   # noqa: E731
    moved = [dataclasses.replace(h, scale=dv(h.scale), center=dv(h.center), inv=dv(h.inv), inv_after=dv(h.inv_after), target=res(h.target),
                                 before=res(h.before), target_after=res(h.target_after)) for h in heads]
    return ops.EmulatorHeadTable(moved, levels)


def launch(heads, levels, f, yhat, idx, device, pad=0, with_dy=True, accum=None, table=None, repeat=1):
    """``repeat`` launches on one set of buffers; everything read back as numpy."""
    table = table or device_table(heads, levels, pad, device)
    m = yhat.shape[0]
    _, y = _padded(yhat, pad, device)
    dy_full = torch.full((m + 2, f + pad), SENTINEL, dtype=torch.float32, device=device)
    values = torch.zeros(max(table.n_slots, 1), dtype=torch.float64, device=device)
    loss = torch.zeros(1, dtype=torch.float64, device=device)
    ws = torch.zeros(ops.train_emulator_loss_workspace_doubles(), dtype=torch.float64, device=device)
    didx = None if idx is None else torch.from_numpy(idx).to(device)
    for _ in range(repeat):
        ops.train_emulator_loss_grad(y, table, dy_full[:m, :f] if with_dy else None, values, loss, ws, idx=didx, accum=accum,
                                     n=m // levels)
    torch.cuda.synchronize()
    return dict(dy_full=dy_full.cpu().numpy(), dy=dy_full[:m, :f].cpu().numpy(), values=values.cpu().numpy()[:table.n_slots],
                loss=float(loss.cpu()[0]))


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
    a = np.ascontiguousarray(x)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def weighted_sum(heads, values):
    """``loss`` as the finish kernel forms it: the loss slots in slot order, float64."""
    terms = {}
    for h in heads:
        for slot, w, il in ((h.slot, h.weight, h.is_loss), (h.slot_after, h.weight_after, h.is_loss_after)):
            if slot is not None and il:
                terms[slot] = float(w)
    total = 0.0
    for slot in sorted(terms):
        total += terms[slot] * float(values[slot])
    return total


@pytest.mark.parametrize("mode,n,size,layout,pad,idx_kind", CASES, ids=[f"{c[0]}-n{c[1]}-s{c[2]}-{c[3]}-pad{c[4]}-{c[5]}" for c in CASES])
def test_gradient_and_values_within_the_gates(mode, n, size, layout, pad, idx_kind, device):
    heads, levels, f, yhat, idx = build(mode, n, size, layout, idx_kind)
    want_dy, want_values, want_loss, gate, vgate, lgate = E.loss_grad(yhat, heads, levels, idx=idx)
    got = launch(heads, levels, f, yhat, idx, device, pad=pad)
    frac = assert_within(got["dy"], want_dy, gate, "dY")
    vfrac = assert_within(got["values"], want_values, vgate, "values")
    print(f"dY {frac:.3f} of its gate, values {vfrac:.3f}")
    if np.isnan(want_loss):
        assert np.isnan(got["loss"])
    else:
        assert abs(got["loss"] - want_loss) <= lgate
        ws = weighted_sum(heads, got["values"])
        assert abs(got["loss"] - ws) <= 1e-15 * abs(ws)
    assert np.all(got["dy_full"][:, f:] == SENTINEL) and np.all(got["dy_full"][yhat.shape[0]:] == SENTINEL)     # padding, rows past n L
    for h in heads:
        cols = got["dy"][:, h.col0:h.col0 + h.ncol]
        no_loss = not ((h.slot is not None and h.is_loss) or (h.slot_after is not None and h.is_loss_after))
        if h.slot is None and h.slot_after is None:
            assert not bits(cols).any(), "a head without a term must give exact zeros"
        elif no_loss:   # a metric-only head: its values are reported, dY is zero whatever its targets hold
            assert not cols.any()
        if h.single_level:
            assert not bits(cols.reshape(n, levels)[:, 1:]).any()


def test_two_launches_are_bitwise_equal_and_dy_may_be_null(device):
    heads, levels, f, yhat, idx = build("local", 257, 3, 4, "repeats")
    a = launch(heads, levels, f, yhat, idx, device)
    b = launch(heads, levels, f, yhat, idx, device, pad=3)
    c = launch(heads, levels, f, yhat, idx, device, with_dy=False)
    assert np.array_equal(bits(a["dy"]), bits(b["dy"])) and np.array_equal(bits(a["values"]), bits(b["values"])) and a["loss"] == b["loss"]
    assert np.array_equal(bits(a["values"]), bits(c["values"])) and a["loss"] == c["loss"]
    assert np.all(c["dy_full"] == SENTINEL)


def test_accumulator_adds_three_launches_in_order(device):
    heads, levels, f, yhat, idx = build("dense", 65, 3, "mixed", "none")
    one = launch(heads, levels, f, yhat, idx, device)
    ns = len(one["values"])
    accum = torch.zeros(1 + ns, dtype=torch.float64, device=device)
    launch(heads, levels, f, yhat, idx, device, accum=accum, repeat=3)
    want = np.zeros(1 + ns)
    for _ in range(3):
        want = want + np.concatenate([[one["loss"]], one["values"]])
    assert np.array_equal(bits(accum.cpu().numpy()), bits(want))


def test_a_metric_term_leaves_the_gradient_bitwise_unchanged(device):
    heads, levels, f, yhat, idx = build("dense", 65, 3, "mixed", "none")
    with_metric = launch(heads, levels, f, yhat, idx, device)
    stripped = [dataclasses.replace(h) for h in heads]
    h = stripped[1]
    assert h.slot_after is not None and not h.is_loss_after
    last = max(s for k in stripped for s in (k.slot, k.slot_after) if s is not None)
    removed = h.slot_after
    h.slot_after = h.before = h.target_after = h.inv_after = None
    for k in stripped:   # keep the slots 0 .. n - 1: the last one takes the freed number
        if k.slot == last:
            k.slot = removed
        if k.slot_after == last:
            k.slot_after = removed
    without = launch(stripped, levels, f, yhat, idx, device)
    assert np.array_equal(bits(with_metric["dy"]), bits(without["dy"]))
    assert len(without["values"]) == len(with_metric["values"]) - 1


def test_a_nan_target_and_an_inf_logit_stay_where_they_are(device):
    heads, levels, f, yhat, idx = build("local", 5, 3, 4, "none")
    clean = launch(heads, levels, f, yhat, idx, device)
    dirty = [dataclasses.replace(h) for h in heads]
    dirty[0].target = dirty[0].target.copy()
    dirty[0].target[2, 1] = np.nan                       # batch row 2, level 1 of the first head's direct term
    y2 = yhat.copy()
    xent = heads[2]
    y2[4 * levels + 2, xent.col0 + 1] = np.inf           # batch row 4, level 2, channel 1
    got = launch(dirty, levels, f, y2, idx, device)
    bad = np.zeros(got["dy"].shape, bool)
    bad[2 * levels + 1, heads[0].col0] = True
    bad[4 * levels + 2, xent.col0:xent.col0 + xent.ncol] = True
    assert np.array_equal(np.isnan(got["dy"]), bad)
    assert np.array_equal(bits(got["dy"][~bad]), bits(clean["dy"][~bad]))
    bad_slots = np.zeros(len(got["values"]), bool)
    bad_slots[[heads[0].slot, xent.slot]] = True
    assert np.array_equal(np.isnan(got["values"]), bad_slots) and np.isnan(got["loss"])
    assert np.array_equal(bits(got["values"][~bad_slots]), bits(clean["values"][~bad_slots]))
    # a NaN in a metric slot stays out of the loss
    metric = [dataclasses.replace(h) for h in dirty]
    metric[0].is_loss = False
    metric[2] = heads[2]
    metric[0].is_loss_after = False
    got = launch(metric, levels, f, yhat, idx, device)
    assert np.isnan(got["values"][heads[0].slot]) and np.isfinite(got["loss"])
    assert np.isfinite(got["dy"]).all() and not got["dy"][:, heads[0].col0].any()     # nor into dY: a metric sends nothing there


def test_extreme_logits_are_finite(device):
    rng = np.random.default_rng(5)
    heads, f = C.make_heads(rng, 3, 2, [("xent", 4, dict(direct=("loss", 1.0)))])
    heads[0].target[:] = np.eye(4, dtype=np.float32)[[[1, 1], [2, 3], [1, 1]]]
    yhat = np.array([[1e4, -1e4, 0, 3], [-1e4, 1e4, 1e4, -1e4], [88.8, 0, -88.8, 1], [0, 88.8, 88.8, 88.8], [1e4, 1e4, 1e4, 1e4],
                     [-1e4, -1e4, -1e4, -1e4]], np.float32)
    want_dy, want_values, _, gate, vgate, _ = E.loss_grad(yhat, heads, 2)
    got = launch(heads, 2, f, yhat, None, device)
    assert np.isfinite(got["dy"]).all() and np.isfinite(got["values"]).all() and np.isfinite(got["loss"])
    assert_within(got["dy"], want_dy, gate, "dY")
    assert_within(got["values"], want_values, vgate, "values")


def test_every_bad_argument_is_refused_without_a_launch(device):
    heads, levels, f, yhat, idx = build("local", 5, 3, 4, "none")
    m = yhat.shape[0]
    y = torch.from_numpy(yhat).to(device)
    ld = 64
    dy = torch.full((6 * levels, ld), SENTINEL, dtype=torch.float32, device=device)
    values = torch.full((40,), SENTINEL, dtype=torch.float64, device=device)
    loss = torch.full((1,), SENTINEL, dtype=torch.float64, device=device)
    ws = torch.zeros(ops.train_emulator_loss_workspace_doubles(), dtype=torch.float64, device=device)

    def refused(table, match, yhat_=y, n=5, raw=None):
        with pytest.raises(_lib.Fv3HipError, match=match):
            if raw is not None:
                raw()
            else:
                ops.train_emulator_loss_grad(yhat_, table, dy, values, loss, ws, n=n)
        torch.cuda.synchronize()
        assert np.all(dy.cpu().numpy() == SENTINEL) and np.all(values.cpu().numpy() == SENTINEL) and float(loss.cpu()[0]) == SENTINEL

    def table_with(change, levels_=levels):
        changed = [dataclasses.replace(h) for h in heads]
        change(changed)
        return device_table(changed, levels_, 0, device)

    good = device_table(heads, levels, 0, device)
    refused(good, "yhat is null", raw=lambda: _lib.call_on(device, "fv3hip_train_emulator_loss_grad", None, f, 5, levels, f, good.array,
                                                           len(heads), good.n_slots, good.rows, None, ops._ptr(dy), ld, ops._ptr(values),
                                                           ops._ptr(loss), None, ops._ptr(ws), ops._stream(device)))

    def one_channel(hs):
        hs[2].ncol, hs[3].col0 = 1, hs[2].col0 + 1
        hs[2].target = np.ascontiguousarray(hs[2].target[:, :, :1])
    refused(table_with(one_channel), "2 to 32 channels")

    def too_many_channels(hs):
        hs[2].ncol, hs[3].col0 = 33, hs[2].col0 + 33
        hs[2].target = np.zeros((5, levels, 33), np.float32)
    wide = torch.zeros((m, ld), dtype=torch.float32, device=device)
    refused(table_with(too_many_channels), "2 to 32 channels", yhat_=wide)

    def overlap(hs):
        hs[1].col0 = hs[0].col0
    refused(table_with(overlap), "overlaps")

    def gap(hs):
        hs[3].col0 += 1
    refused(table_with(gap), "belong to no head", yhat_=wide)

    refused(good, "does not hold", raw=lambda: _lib.call_on(device, "fv3hip_train_emulator_loss_grad", ops._ptr(y), f - 1, 5, levels, f,
                                                            good.array, len(heads), good.n_slots, good.rows, None, ops._ptr(dy), ld,
                                                            ops._ptr(values), ops._ptr(loss), None, ops._ptr(ws), ops._stream(device)))   # the last head past ldy
    with pytest.raises(ValueError, match="head features"):      # the wrapper refuses a view narrower than the heads, whatever its stride
        ops.train_emulator_loss_grad(wide[:, :f - 1], good, dy, values, loss, ws, n=5)
    with pytest.raises(ValueError, match="dy is"):
        ops.train_emulator_loss_grad(y, good, dy[:, :f - 1], values, loss, ws, n=5)

    def negative(hs):
        hs[0].weight = -1.0
    refused(table_with(negative), "finite and >= 0")

    def infinite(hs):
        hs[0].weight_after = float("inf")
    refused(table_with(infinite), "finite and >= 0")

    def dense_under_levels(hs):
        hs[3].kind = "mse"
    refused(table_with(dense_under_levels), "levels == 1")

    def slot_twice(hs):
        hs[1].slot = hs[0].slot
    refused(table_with(slot_twice), "used twice")

    rng = np.random.default_rng(1)
    many, f17 = C.make_heads(rng, 5, 1, [("mse", 1, dict(direct=("loss", 1.0)))] * (_lib.EMULATOR_MAX_HEADS + 1))
    refused(device_table(many, 1, 0, device), "at most 16", yhat_=wide)
    refused(good, "rows", yhat_=torch.zeros((6 * levels, f), dtype=torch.float32, device=device), n=6)     # rows < n without a table
