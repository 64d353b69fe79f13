"""The CycleGAN training kernels on their own: training forward, backward-data, backward-weight / db, norm backward.

The reference of every convolution case is float64 autograd on the CPU through ``append_halos_tensor`` (or zero ``F.pad``), then
``F.conv2d`` / ``F.conv_transpose2d`` + crop (``cyclegan_train_cases``).

Exact data: inputs and dy are integers in [-3, 3], weights in [-2, 2], so every product and partial sum is an integer below
2**24 (the largest: 3 * 2 * 49 * 70), the float32 result does not depend on the order of the sum and the device must equal the
reference bit for bit.  Sizes: n = 4 (96 rows: under one 128-row block; with k = 7 the halo is 3 of 4 wide and a cell lies within
the halo width of both edges of an axis), n = 8 (384 rows: three blocks), n = 12 (864 rows).  The weight gradient's reduction
chunk is 512 rows: three samples of n = 8 and n = 12 cross it (1152 and 2592 rows; the strided kind's rows are the output
cells: 648 at n = 12), one sample of n = 12 does too, n = 4 stays within one chunk."""
import numpy as np
import pytest
import torch

import cyclegan_cases as cc
import cyclegan_train_cases as tc

pytestmark = pytest.mark.gpu

CHANNELS = [(1, 1), (3, 5), (16, 32), (20, 70)]   # the vector loader and not, one and several N tiles, N past 64
KIND_IDS = [f"{kind}{k}" for kind, k in tc.KIND_CASES]
U = 2.0 ** -24


def integers(rng, kind, k, n, S, c_in, c_out):
    n_out = tc.out_edge(kind, n)
    x = rng.integers(-3, 4, (S, 6, n, n, c_in)).astype(np.float32)
    dy = rng.integers(-3, 4, (S, 6, n_out, n_out, c_out)).astype(np.float32)
    w = rng.integers(-2, 3, tc.torch_weight_shape(kind, c_in, c_out, k)).astype(np.float32)
    return x, w, dy


@pytest.mark.parametrize("n", [4, 8, 12])
@pytest.mark.parametrize("halo", [True, False], ids=["cube", "zeros"])
@pytest.mark.parametrize("kind,k", tc.KIND_CASES, ids=KIND_IDS)
def test_gradients_of_integer_data_are_exact(device, kind, k, halo, n):
    rng = np.random.default_rng(1000 * n + 10 * k + len(kind))
    for c_in, c_out in CHANNELS:
        for S in (1, 3):
            x, w, dy = integers(rng, kind, k, n, S, c_in, c_out)
            _, dx, dw, db = tc.torch_backward(kind, k, halo, x, w, dy)
            got_dx, got_dw, got_db = tc.device_backward(device, kind, k, halo, x, w, dy)
            case = (kind, k, halo, n, c_in, c_out, S)
            assert np.array_equal(got_dx, dx), (case, "dx", int(np.sum(got_dx != dx)))
            assert np.array_equal(got_dw, dw), (case, "dw", int(np.sum(got_dw != dw)))
            assert np.array_equal(got_db, db), (case, "db", int(np.sum(got_db != db)))


@pytest.mark.parametrize("kind,k", tc.KIND_CASES, ids=KIND_IDS)
def test_gradients_on_slices_of_wider_buffers(device, kind, k):
    """x, dy and dx at non-zero channel offsets of rows wider than their channels; the neighbouring channels of dx stay."""
    rng = np.random.default_rng(k)
    n, S, c_in, c_out = 6, 2, 6, 34
    x, w, dy = integers(rng, kind, k, n, S, c_in, c_out)
    _, dx, dw, db = tc.torch_backward(kind, k, True, x, w, dy)
    got_dx, got_dw, got_db = tc.device_backward(device, kind, k, True, x, w, dy, x_off=2, x_width=c_in + 5, dy_off=3, dy_width=c_out + 4,
                                                dx_off=1, dx_width=c_in + 3)
    assert np.array_equal(got_dx[..., 1:1 + c_in], dx) and np.array_equal(got_dw, dw) and np.array_equal(got_db, db)
    assert cc.untouched(got_dx[..., :1]) and cc.untouched(got_dx[..., 1 + c_in:]), "the neighbouring channels were written"
    # the vector loader of dy (16 channels, aligned) from offset 4, and the scalar one from offset 2, give the same
    x, w, dy = integers(rng, kind, k, n, S, 5, 16)
    _, dx, _, _ = tc.torch_backward(kind, k, True, x, w, dy)
    for off in (4, 2):
        assert np.array_equal(tc.device_backward(device, kind, k, True, x, w, dy, dy_off=off, dy_width=24)[0], dx), off


def test_the_footprint_of_one_cell_across_each_of_the_24_edges(device):
    """dy = 1 on one output cell next to a face edge (off the edge's middle, so that a flipped edge shows), distinct weights: the
    gradient on the neighbouring face is the exact, rotated footprint."""
    n, kind, k = 4, "regular", 3
    w = np.arange(1, 10, dtype=np.float32).reshape(1, 1, 3, 3)
    x = np.zeros((1, 6, n, n, 1), np.float32)
    for tile in range(6):
        for side, (i, j) in enumerate([(0, 1), (n - 1, 1), (1, 0), (1, n - 1)]):
            dy = np.zeros((1, 6, n, n, 1), np.float32)
            dy[0, tile, i, j, 0] = 1.0
            _, dx, _, _ = tc.torch_backward(kind, k, True, x, w, dy)
            others = np.delete(dx[0], tile, axis=0)
            assert np.count_nonzero(others) == 3, (tile, side)   # three taps reach over the edge
            got = tc.device_backward(device, kind, k, True, x, w, dy)[0]
            assert np.array_equal(got, dx), (tile, side)


@pytest.mark.parametrize("halo", [True, False], ids=["cube", "zeros"])
@pytest.mark.parametrize("kind,k", tc.KIND_CASES, ids=KIND_IDS)
def test_training_forward(device, kind, k, halo):
    """Bit-identical to ``fv3hip_cyclegan_conv`` without a transform wherever both are built -- on random normal data, where a
    different order of the sum would show -- and to the reference on integer data (the 3 x 3 strided kind is built here only)."""
    rng = np.random.default_rng(k + 17)
    for n in (4, 8, 12):                      # the grid of test_gradients_of_integer_data_are_exact
        for c_in, c_out in CHANNELS:
            for S in (1, 3):
                x, w, _ = integers(rng, kind, k, n, S, c_in, c_out)
                b = rng.integers(-3, 4, c_out).astype(np.float32)
                want = tc.torch_forward(kind, k, halo, torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double())
                assert np.array_equal(tc.device_forward(device, kind, k, halo, x, w, b), want.numpy()), (kind, k, n, c_in, c_out, S)
                if (kind, k) != ("strided", 3):
                    xr = rng.normal(0, 1, x.shape).astype(np.float32)
                    wr, br = rng.normal(0, 1, w.shape).astype(np.float32), rng.normal(0, 1, c_out).astype(np.float32)
                    assert np.array_equal(tc.bits(tc.device_forward(device, kind, k, halo, xr, wr, br)),
                                          tc.bits(cc.device_layer(device, kind, k, halo, xr, wr, br))), (kind, k, n, c_in, c_out, S)
    x, w, _ = integers(rng, kind, k, 6, 2, 16, 3)   # the vector loader from a slice at offset 4, no bias
    want = tc.torch_forward(kind, k, halo, torch.from_numpy(x).double(), torch.from_numpy(w).double(), None)
    assert np.array_equal(tc.device_forward(device, kind, k, halo, x, w, None, src_off=4, src_width=24), want.numpy())


@pytest.mark.parametrize("halo", [True, False], ids=["cube", "zeros"])
@pytest.mark.parametrize("kind,k", tc.KIND_CASES, ids=KIND_IDS)
def test_gradients_of_random_data(device, kind, k, halo):
    """Per element |got - ref64| <= (N + 2) 2^-24 sum |a| |b| over the element's own N terms: the standard bound of a float32
    sum of separately rounded products (N - 1 additions and one product rounding each, first order; + 2 covers the second-order
    terms and the additions of the up to five positions of dx and of the chunk partials of dw, which are counted in N
    already; db is summed in float64 and only rounded at the end).  N and the sum of |a| |b| come from the same adjoint on ones
    and on absolute values.  n = 4, 8, 12 with 1 and 3 samples, as the integer test.  A sample's dx does not change a bit with
    the batch it is in; dw and db are bitwise equal between two runs."""
    rng = np.random.default_rng(k + 31)
    c_in, c_out = (20, 70) if kind == "regular" else (16, 32)
    for n, S in ((4, 1), (4, 3), (8, 1), (8, 3), (12, 1), (12, 3)):
        n_out = tc.out_edge(kind, n)
        x = rng.normal(0, 1, (S, 6, n, n, c_in)).astype(np.float32)
        dy = rng.normal(0, 1, (S, 6, n_out, n_out, c_out)).astype(np.float32)
        w = rng.normal(0, 1, tc.torch_weight_shape(kind, c_in, c_out, k)).astype(np.float32)
        ref = tc.torch_backward(kind, k, halo, x, w, dy)[1:]
        mag = tc.torch_abs_bound(kind, k, halo, x, w, dy)
        count = tc.torch_backward(kind, k, halo, np.ones_like(x), np.ones_like(w), np.ones_like(dy))[1:]
        got = tc.device_backward(device, kind, k, halo, x, w, dy)
        worst = []
        for name, g, r, m, cnt in zip(("dx", "dw", "db"), got, ref, mag, count):
            bound = (cnt + 2) * U * m
            err = np.abs(g.astype(np.float64) - r)
            worst.append(float(np.max(err / np.where(bound == 0, 1, bound))))
            assert np.all(err <= bound), (kind, k, halo, n, S, name, worst[-1])
        print(f"{kind}{k} halo={halo} n={n} S={S}: worst |err| / bound dx {worst[0]:.3f} dw {worst[1]:.3f} db {worst[2]:.3f}")
        if S > 1:
            alone = tc.device_backward(device, kind, k, halo, x[1:2], w, dy[1:2])[0]
            assert np.array_equal(tc.bits(alone[0]), tc.bits(got[0][1])), "a sample's dx depends on its batch"
        again = tc.device_backward(device, kind, k, halo, x, w, dy)
        assert all(np.array_equal(tc.bits(a), tc.bits(b)) for a, b in zip(got, again)), "two runs differ"


# -- instance norm + activation ---------------------------------------------------------------------
def norm_reference(x, bias, slope, dy, dtype):
    """torch's autograd of ``leaky_relu(instance_norm(x) + bias)`` on the CPU -> (pre-activation, dx, dbias), float64 arrays."""
    S, _, n, _, c = x.shape
    t = torch.from_numpy(x).to(dtype).requires_grad_()
    b = None if bias is None else torch.from_numpy(bias).to(dtype).requires_grad_()
    p = torch.nn.functional.instance_norm(t.permute(0, 1, 4, 2, 3).reshape(S * 6, c, n, n)).reshape(S, 6, c, n, n).permute(0, 1, 3, 4, 2)
    if b is not None:
        p = p + b
    y = p if slope == 1 else torch.nn.functional.leaky_relu(p, slope) if slope else torch.relu(p)
    y.backward(torch.from_numpy(dy).to(dtype))
    return p.detach().double().numpy(), t.grad.double().numpy(), None if b is None else b.grad.double().numpy()


def norm_inputs(rng, S, n, c, with_bias):
    """Inputs none of whose float64 pre-activations lies within 1e-4 of zero (offenders are nudged until none is left), so that
    no rounding can flip a mask."""
    x = rng.normal(0, 1, (S, 6, n, n, c)).astype(np.float32)
    bias = rng.normal(0, 0.3, (6, n, n, c)).astype(np.float32) if with_bias else None
    dy = rng.normal(0, 1, x.shape).astype(np.float32)
    for _ in range(100):
        p, _, _ = norm_reference(x, bias, 1, dy, torch.float64)
        close = np.abs(p) < 1e-3
        if not close.any():
            break
        x[close] += np.float32(0.05)
    return x, bias, dy


def device_norm_backward(device, x, bias, slope, dy, want_dbias):
    from fv3net_amd import _lib, ops
    from fv3net_amd.cube import _Slice

    S, _, n, _, c = x.shape
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    xt, dyt, bt = up(x), up(dy), up(bias)
    st = torch.empty((2, S, 6, c), dtype=torch.float32, device=device)
    _lib.call_on(device, "fv3hip_cyclegan_stats", xt.data_ptr(), c, 0, 0, st[0].data_ptr(), st[1].data_ptr(), S, n, c, 1e-5, ops._stream(device))
    dx = torch.full_like(xt, cc.SENTINEL)
    dbias = torch.full((6, n, n, c), cc.SENTINEL, device=device) if want_dbias else None
    ops.cyclegan_train_norm_backward(_Slice(dyt, c), _Slice(xt, c), st[0], st[1], bt, slope, _Slice(dx, c), dbias, S, n, c)
    torch.cuda.synchronize(device)
    return dx.cpu().numpy(), None if dbias is None else dbias.cpu().numpy()


@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("n", [2, 3, 12])
def test_norm_backward(device, n, slope):
    """Per (sample, tile, channel) face: |got - ref64|_inf <= 4 max(|torch32 - ref64|_inf, 2^-24 |ref64|_inf), torch32 being
    torch's float32 CPU autograd on the same inputs; 4 = a different order of the sums (2) x separately rounded products (2).
    The bias gradient is a sum of S terms g, each one rounding from exact: (S + 1) 2^-24 sum |g|."""
    rng = np.random.default_rng(100 * n + int(10 * slope))
    ratios = []
    for c in (1, 16, 20):
        with_bias = c != 16
        S = 2
        x, bias, dy = norm_inputs(rng, S, n, c, with_bias)
        p64, dx64, db64 = norm_reference(x, bias, slope, dy, torch.float64)
        assert np.min(np.abs(p64)) >= 1e-4, "a pre-activation lies within 1e-4 of zero"
        p32, dx32, _ = norm_reference(x, bias, slope, dy, torch.float32)
        assert np.array_equal(p32 > 0, p64 > 0)
        got, got_db = device_norm_backward(device, x, bias, slope, dy, with_bias)
        face = lambda a: np.max(np.abs(a), axis=(2, 3))   # noqa: E731
        gate = 4 * np.maximum(face(dx32 - dx64), U * face(dx64))
        err = face(got.astype(np.float64) - dx64)
        ratios.append(float(np.max(err / gate)))
        assert np.all(err <= gate), (n, slope, c, ratios[-1])
        if with_bias:
            g = np.where(p64 > 0, 1.0, slope) * dy.astype(np.float64)
            assert np.allclose(g.sum(axis=0), db64, rtol=0, atol=1e-12)
            assert np.all(np.abs(got_db - db64) <= (S + 1) * U * np.abs(g).sum(axis=0)), (n, slope, c)
    print(f"norm backward n={n} slope={slope}: worst face error / gate for c = 1, 16, 20: " + ", ".join(f"{r:.3f}" for r in ratios))


def test_norm_backward_of_a_constant_face_is_finite(device):
    x = np.full((1, 6, 3, 3, 4), 2.5, np.float32)
    dy = np.random.default_rng(0).normal(0, 1, x.shape).astype(np.float32)
    for slope in (0.0, 0.2, 1.0):
        got, _ = device_norm_backward(device, x, None, slope, dy, False)
        assert np.all(np.isfinite(got)), slope
