"""The two kernels of FMR training on their own: the weight gradient of a convolution with context channels
and the window loss.

``fv3hip_cyclegan_train_backward_weight_context`` against float64 autograd of ``conv2d`` on the halo-padded concatenation
``x || ctx_cell || ctx_uniform`` (the per-cell table repeated over the samples, the uniform values over all cells): padding the
concatenation gives the neighbouring face's cell context and the uniform value in the halo and zeros at its corners, or zeros
everywhere off the face, which is what the forward resolves.  Data: x, dy and both contexts are integers in [-3, 3], so every
element of dw is a sum of at most 3 * 384 = 1152 integer products of magnitude <= 9, far below 2**24: the float32 result does
not depend on the order of the sum and the device must equal the reference bit for bit.  n = 4 is 96 rows per sample (one short
chunk of the 512), n = 8 with S = 2 is 768 rows (a full and a short chunk), with S = 3 1152 (two full, one short).
c_in = 62 with five context channels crosses the 64-channel tile of the A operand; c_out = 33 and 64 are a short and a full
second 32-column half.

``fv3hip_fmr_loss_grad`` against a numpy float64 restatement: bit-equal on integer data where ``weight / N`` is a power of two
(every operation is then exact), and on random data ``dfake`` within one float32 ulp and the values within ``N 2**-53``
relative (N float64 additions in some order, each half an ulp of a partial sum no larger than the total: all terms are
non-negative)."""
import itertools

import numpy as np
import pytest
import torch

import cyclegan_cases as cc
import cyclegan_train_cases as tc

pytestmark = pytest.mark.gpu

CONTEXTS = [(3, 2), (3, 0), (0, 2), (0, 0)]


# -- backward-weight with context rows ---------------------------------------------------------------
def context_reference(k, halo, x, dy, ctx_cell, ctx_uni):
    """float64 autograd -> (dw ``[k, k, c_in, c_out]``, dw_ctx ``[k, k, c_cell + c_uni, c_out]``, db)."""
    S, _, n, _, c_in = x.shape
    parts = [torch.from_numpy(x).double()]
    if ctx_cell is not None:
        parts.append(torch.from_numpy(ctx_cell).double()[None].expand(S, -1, -1, -1, -1))
    if ctx_uni is not None:
        parts.append(torch.from_numpy(ctx_uni).double().expand(S, 6, n, n, -1))
    cat = torch.cat(parts, dim=-1)
    c_out = dy.shape[-1]
    w = torch.zeros((c_out, cat.shape[-1], k, k), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c_out, dtype=torch.float64, requires_grad=True)
    tc.torch_forward("regular", k, halo, cat, w, b).backward(torch.from_numpy(dy).double())
    dw = tc.kernel_weight("regular", w.grad.numpy())
    return dw[:, :, :c_in], dw[:, :, c_in:], b.grad.numpy()


def gapped_slice(device, a, off, width, gap):
    """``a`` at channel ``off`` of rows ``width`` wide with ``gap`` floats between the samples, everything else NaN."""
    from fv3net_amd.cube import _Slice

    buf, ld, stride = cc.gapped(a, off, width, gap=gap, fill=np.nan)
    t = torch.from_numpy(buf).to(device)
    return _Slice(t, ld, off, stride if gap else 0)


def device_context(device, k, halo, x, dy, ctx_cell, ctx_uni, kind="regular", x_off=0, x_width=None, x_gap=0, dy_off=0, dy_width=None,
                   dy_gap=0):
    from fv3net_amd import ops

    S, _, n, _, c_in = x.shape
    c_out = dy.shape[-1]
    c_cell, c_uni = 0 if ctx_cell is None else ctx_cell.shape[-1], 0 if ctx_uni is None else ctx_uni.shape[0]
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)   # noqa: E731
    xs, gs = gapped_slice(device, x, x_off, x_width, x_gap), gapped_slice(device, dy, dy_off, dy_width, dy_gap)
    dw = torch.full((k, k, c_in, c_out), cc.SENTINEL, device=device)
    dw_ctx = torch.full((k, k, c_cell + c_uni, c_out), cc.SENTINEL, device=device) if c_cell + c_uni else None
    db = torch.full((c_out,), cc.SENTINEL, device=device)
    floats = ops.cyclegan_train_backward_weight_context_workspace_floats(S, n, c_in, c_cell, c_uni, c_out, k)
    ws = torch.full((max(floats, 1),), np.nan, device=device)
    ops.cyclegan_train_backward_weight_context(xs, gs, up(ctx_cell), up(ctx_uni), dw, dw_ctx, db, S, n, c_in, c_out, k, halo, ws, kind=kind)
    torch.cuda.synchronize(device)
    return dw.cpu().numpy(), None if dw_ctx is None else dw_ctx.cpu().numpy(), db.cpu().numpy()


def integer_case(rng, n, S, c_in, c_out, c_cell, c_uni):
    draw = lambda *shape: rng.integers(-3, 4, shape).astype(np.float32)   # noqa: E731
    return (draw(S, 6, n, n, c_in), draw(S, 6, n, n, c_out), draw(6, n, n, c_cell) if c_cell else None, draw(c_uni) if c_uni else None)


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("halo", [True, False], ids=["cube", "zeros"])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_context_weight_gradient_of_integer_data_is_exact(device, k, halo, n):
    """Every (S, c_in, c_out) of {1, 2, 3} x {1, 16, 62} x {1, 33, 64} with the full context and one of the other three, which
    rotates so that every (c_in, context) and (c_out, context) pair occurs."""
    rng = np.random.default_rng(100 * n + 10 * k + halo)
    for i, (S, c_in, c_out) in enumerate(itertools.product((1, 2, 3), (1, 16, 62), (1, 33, 64))):
        for c_cell, c_uni in (CONTEXTS[0], CONTEXTS[1 + (i + i // 3 + i // 9) % 3]):
            x, dy, ctx_cell, ctx_uni = integer_case(rng, n, S, c_in, c_out, c_cell, c_uni)
            dw, dw_ctx, db = context_reference(k, halo, x, dy, ctx_cell, ctx_uni)
            got_dw, got_ctx, got_db = device_context(device, k, halo, x, dy, ctx_cell, ctx_uni)
            case = (k, halo, n, S, c_in, c_out, c_cell, c_uni)
            assert np.array_equal(got_dw, dw), (case, "dw", int(np.sum(got_dw != dw)))
            assert np.array_equal(got_db, db), (case, "db")
            if c_cell + c_uni:
                assert np.array_equal(got_ctx, dw_ctx), (case, "dw_ctx", int(np.sum(got_ctx != dw_ctx)))
            else:
                assert got_ctx is None and dw_ctx.shape[2] == 0


@pytest.mark.parametrize("k", [3, 5, 7])
def test_context_weight_gradient_on_strided_and_offset_slices(device, k):
    """x and dy at non-zero channel offsets of wider rows, with a gap between the samples."""
    rng = np.random.default_rng(k)
    x, dy, ctx_cell, ctx_uni = integer_case(rng, 8, 2, 6, 34, 3, 2)
    want = context_reference(k, True, x, dy, ctx_cell, ctx_uni)
    got = device_context(device, k, True, x, dy, ctx_cell, ctx_uni, x_off=2, x_width=11, x_gap=7, dy_off=3, dy_width=38, dy_gap=5)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("halo", [True, False], ids=["cube", "zeros"])
def test_without_a_context_it_is_the_existing_entry_point_bit_for_bit(device, halo):
    """On random normal data, where another order of the sum would show; and the source rows do not change a bit when a
    context is added (they share the kernel's tiles with it)."""
    rng = np.random.default_rng(5)
    for k, n, S, c_in, c_out in ((3, 8, 3, 62, 33), (5, 4, 2, 16, 64), (7, 8, 2, 1, 1)):
        x = rng.normal(0, 1, (S, 6, n, n, c_in)).astype(np.float32)
        dy = rng.normal(0, 1, (S, 6, n, n, c_out)).astype(np.float32)
        w = np.zeros((c_out, c_in, k, k), np.float32)
        _, dw, db = tc.device_backward(device, "regular", k, halo, x, w, dy)
        got_dw, got_ctx, got_db = device_context(device, k, halo, x, dy, None, None)
        assert got_ctx is None
        assert np.array_equal(tc.bits(got_dw), tc.bits(dw)) and np.array_equal(tc.bits(got_db), tc.bits(db)), (k, n, S)
        ctx_cell, ctx_uni = rng.normal(0, 1, (6, n, n, 3)).astype(np.float32), rng.normal(0, 1, 2).astype(np.float32)
        with_dw, with_ctx, with_db = device_context(device, k, halo, x, dy, ctx_cell, ctx_uni)
        assert np.array_equal(tc.bits(with_dw), tc.bits(dw)) and np.array_equal(tc.bits(with_db), tc.bits(db)), (k, n, S)
        again = device_context(device, k, halo, x, dy, ctx_cell, ctx_uni)[1]
        assert np.array_equal(tc.bits(with_ctx), tc.bits(again)), "two runs differ"


@pytest.mark.parametrize("kind,k", [("strided", 3), ("strided", 4), ("transposed", 4)])
def test_a_context_with_another_kind_is_unsupported(device, kind, k):
    from fv3net_amd import _lib

    rng = np.random.default_rng(0)
    n, n_out = 8, tc.out_edge(kind, 8)
    x, _, ctx_cell, ctx_uni = integer_case(rng, n, 1, 4, 5, 3, 2)
    dy = np.zeros((1, 6, n_out, n_out, 5), np.float32)
    from fv3net_amd import ops
    from fv3net_amd.cube import _Slice

    up = lambda a: torch.from_numpy(a).to(device)   # noqa: E731
    xt, dyt = up(x), up(dy)
    shape = (2, 2, 2, 2) if kind == "transposed" else (k, k)
    dw, dw_ctx = torch.zeros(shape + (4, 5), device=device), torch.zeros(shape[:2] + (5, 5), device=device)
    with pytest.raises(_lib.Fv3HipError, match="context channels are built for the regular convolution") as err:
        ops.cyclegan_train_backward_weight_context(_Slice(xt, 4), _Slice(dyt, 5), up(ctx_cell), up(ctx_uni), dw, dw_ctx, None, 1, n, 4, 5, k,
                                                   True, torch.zeros(1 << 16, device=device), kind=kind)
    assert err.value.code == _lib.EUNSUPPORTED


# -- the window loss ---------------------------------------------------------------------------------
def loss_reference(fake, real, dgan, kinds, weights):
    """The numpy float64 restatement on ``[window, time, ...]`` arrays -> (values ``[2]``, dfake float32)."""
    f, r = fake.astype(np.float64), real.astype(np.float64)
    d = f - r
    W, T = fake.shape[:2]
    E = int(np.prod(fake.shape[2:]))
    counts = (W * E, W * (T - 1) * E)
    parts = (d[:, :1], d[:, 1:])
    values, grads = [], []
    for part, kind, weight, count in zip(parts, kinds, weights, counts):
        coef = weight / count
        values.append(coef * float(np.sum(part * part if kind == "mse" else np.abs(part))))
        grads.append((2.0 * coef) * part if kind == "mse" else coef * np.sign(part))
    g = np.concatenate(grads, axis=1)
    if dgan is not None:
        g = dgan.astype(np.float64) + g
    return np.array(values), g.astype(np.float32)


def device_loss(device, fake, real, dgan, kinds, weights, time_major=False, want_grad=True):
    """``time_major``: fake, dgan and dfake live as ``[time, window, ...]`` and are handed over as permuted views; real stays
    window-major."""
    from fv3net_amd import ops

    def up(a):
        if a is None:
            return None
        if time_major:
            return torch.from_numpy(np.ascontiguousarray(np.swapaxes(a, 0, 1))).to(device).transpose(0, 1)
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    f, g = up(fake), up(dgan)
    r = torch.from_numpy(np.ascontiguousarray(real)).to(device)
    dfake = up(np.full(fake.shape, cc.SENTINEL, np.float32)) if want_grad else None
    values = ops.fmr_loss_grad(f, r, g, dfake, kinds[0], weights[0], kinds[1], weights[1])
    torch.cuda.synchronize(device)
    return values.cpu().numpy(), None if dfake is None else dfake.cpu().numpy()


LOSS_SHAPES = [(2, 4, 6, 4, 4, 3),      # 2304 elements: one full block of 2048 and a short one, a window ends inside the first
               (1, 2, 6, 3, 3, 5),      # 540 elements: one window, the fewest times, under one block
               (3, 3, 6, 8, 8, 1)]      # 3456 elements


@pytest.mark.parametrize("time_major", [False, True], ids=["window-major", "time-major"])
@pytest.mark.parametrize("kinds", [("mae", "mse"), ("mse", "mae")], ids=lambda k: "-".join(k))
def test_loss_of_integer_data_is_exact(device, kinds, time_major):
    """weight / N a power of two: N0 = W E, N1 = W (T - 1) E, so the weights are N0 / 8 and N1 / 4."""
    rng = np.random.default_rng(11)
    for shape in LOSS_SHAPES:
        W, T, E = shape[0], shape[1], int(np.prod(shape[2:]))
        weights = (W * E / 8.0, W * (T - 1) * E / 4.0)
        fake, real = (rng.integers(-4, 5, shape).astype(np.float32) for _ in range(2))
        for with_dgan in (True, False):
            dgan = rng.integers(-8, 9, shape).astype(np.float32) / 16 if with_dgan else None
            want_values, want_grad = loss_reference(fake, real, dgan, kinds, weights)
            values, grad = device_loss(device, fake, real, dgan, kinds, weights, time_major)
            assert np.array_equal(values, want_values), (shape, with_dgan, values, want_values)
            assert np.array_equal(tc.bits(grad), tc.bits(want_grad)), (shape, with_dgan)
        assert np.any(fake == real), "no zero difference drawn: sign(0) = 0 is not exercised"
        only, none = device_loss(device, fake, real, None, kinds, weights, time_major, want_grad=False)
        assert none is None and np.array_equal(only, loss_reference(fake, real, None, kinds, weights)[0])


@pytest.mark.parametrize("time_major", [False, True], ids=["window-major", "time-major"])
@pytest.mark.parametrize("kinds", [("mae", "mse"), ("mse", "mae")], ids=lambda k: "-".join(k))
def test_loss_of_random_data(device, kinds, time_major):
    rng = np.random.default_rng(12)
    for shape in LOSS_SHAPES:
        weights = (0.7, 13.0)
        fake, real, dgan = (rng.normal(0, 1, shape).astype(np.float32) for _ in range(3))
        want_values, _ = loss_reference(fake, real, dgan, kinds, weights)
        values, grad = device_loss(device, fake, real, dgan, kinds, weights, time_major)
        N = int(np.prod(shape))
        rel = np.abs(values - want_values) / want_values
        print(f"{kinds} {shape}: values off by {rel[0]:.1e}, {rel[1]:.1e} relative (gate {N * 2.0 ** -53:.1e})")
        assert np.all(rel <= N * 2.0 ** -53), (shape, rel)
        # dfake: the float64 expression rounded once; the restatement may differ in the last bit of that float64 value
        exact = loss_reference(fake, real, dgan, kinds, weights)[1].astype(np.float64)
        ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(grad.astype(np.float64) - exact) <= ulp), shape
        again_values, again = device_loss(device, fake, real, dgan, kinds, weights, time_major)
        assert np.array_equal(again_values, values) and np.array_equal(tc.bits(again), tc.bits(grad)), "two runs differ"


def test_loss_refusals(device):
    from fv3net_amd import _lib, ops

    f = torch.zeros((2, 1, 6, 4, 4, 3), device=device)
    with pytest.raises(_lib.Fv3HipError, match="n_times must be in \\[2"):
        ops.fmr_loss_grad(f, f.clone(), None, None, "mae", 1.0, "mse", 1.0)
    f = torch.zeros((2, 3, 6, 4, 4, 3), device=device)
    with pytest.raises(ValueError, match="unknown loss kind 'huber'"):
        ops.fmr_loss_grad(f, f.clone(), None, None, "huber", 1.0, "mse", 1.0)
    with pytest.raises(_lib.Fv3HipError, match="overlap"):
        ops.fmr_loss_grad(f, f.clone(), None, f, "mae", 1.0, "mse", 1.0)   # dfake is fake
    with pytest.raises(ValueError, match="fake's strides"):
        ops.fmr_loss_grad(f, f.clone(), None, torch.zeros((3, 2, 6, 4, 4, 3), device=device).transpose(0, 1), "mae", 1.0, "mse", 1.0)
    g = torch.ones_like(f)
    values = ops.fmr_loss_grad(f, f.clone(), g, g, "mae", 1.0, "mse", 1.0)   # in place on dgan
    torch.cuda.synchronize(device)
    assert float(values.sum()) == 0 and bool(torch.all(g == 1))
