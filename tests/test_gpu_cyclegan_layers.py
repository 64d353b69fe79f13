"""Every ``fv3hip_cyclegan_*`` layer kernel on its own.

The convolutions run on exact data: inputs are integers in [-4, 4], weights in {-1, 0, 1}, biases integers, so every partial
sum is an integer below 2**24, the float32 result does not depend on the order of the sum, and the device must equal torch's
``conv2d`` / ``conv_transpose2d`` (+ crop by 3) on ``append_halos_tensor``-padded or zero-padded input bit for bit: taps,
parities, crop, seam orientation and flips with no tolerance.  Sizes: the smallest that cross one 128-cell block, one 32-channel
MFMA tile and one 16-row K chunk, with odd remainders.
"""
import numpy as np
import pytest
import torch

import cyclegan_cases as cc

pytestmark = pytest.mark.gpu

SHAPES = ([("regular", 3, n) for n in (2, 4, 16, 20)] + [("regular", 7, n) for n in (4, 16, 20)]
          + [("strided", 4, n) for n in (4, 20)] + [("transposed", 4, n) for n in (2, 10)])
C_IN, C_OUT = (1, 3, 8, 33), (1, 3, 32, 40)


def exact_layer(rng, kind, k, c_in, c_out):
    from fv3net_amd.cyclegan import weight_shape

    w = rng.integers(-1, 2, weight_shape(kind, c_in, c_out, k)).astype(np.float32)
    return w, rng.integers(-3, 4, c_out).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("halo", [True, False], ids=["cube", "zeros"])
@pytest.mark.parametrize("kind,k,n", SHAPES, ids=[f"{kind}{k}-n{n}" for kind, k, n in SHAPES])
def test_convolution_is_exact(device, kind, k, n, halo):
    """All 16 channel pairs; one sample where ``i + j`` is even, three where it is odd, so that every ``c_in`` and every
    ``c_out`` meets both."""
    rng = np.random.default_rng(n * 100 + k)
    for i, c_in in enumerate(C_IN):
        for j, c_out in enumerate(C_OUT):
            S = 3 if (i + j) % 2 else 1
            x = rng.integers(-4, 5, (S, 6, n, n, c_in)).astype(np.float32)
            w, b = exact_layer(rng, kind, k, c_in, c_out)
            want = cc.torch_layer(kind, k, halo, x, w, b)
            got = cc.device_layer(device, kind, k, halo, x, w, b)
            assert got.shape == want.shape, (c_in, c_out, got.shape, want.shape)
            assert np.array_equal(bits(got), bits(want)), (kind, k, n, c_in, c_out, S, int(np.sum(got != want)))


@pytest.mark.parametrize("halo", [True, False], ids=["cube", "zeros"])
@pytest.mark.parametrize("kind,k,n", [("regular", 3, 4), ("regular", 5, 6), ("regular", 7, 20), ("strided", 4, 20), ("transposed", 4, 10)])
def test_loader_transform_is_exact(device, kind, k, n, halo):
    """Integer mean, power-of-two rstd, integer per-cell bias and ReLU keep the data exact; halo cells take the statistics and
    the bias cell of the face they lie on, as the same transform applied in torch before padding gives them.  Also the per-cell
    output bias."""
    rng = np.random.default_rng(k + n)
    S, c_in, c_out = 3, 5, 35
    x = rng.integers(-4, 5, (S, 6, n, n, c_in)).astype(np.float32)
    w, b = exact_layer(rng, kind, k, c_in, c_out)
    mean = rng.integers(-3, 4, (S, 6, c_in)).astype(np.float32)
    rstd = (2.0 ** rng.integers(-1, 3, (S, 6, c_in))).astype(np.float32)
    cell_bias = rng.integers(-2, 3, (6, n, n, c_in)).astype(np.float32)
    for transform in ((mean, rstd, cell_bias, True), (mean, rstd, None, False), (None, None, cell_bias, True)):
        t = transform if transform[0] is not None else (np.zeros_like(mean), np.ones_like(rstd)) + transform[2:]
        want = cc.torch_layer(kind, k, halo, x, w, b, transform=t)
        got = cc.device_layer(device, kind, k, halo, x, w, b, transform=transform)
        assert np.array_equal(bits(got), bits(want)), (kind, transform[3], int(np.sum(got != want)))
    n_out = want.shape[2]
    out_bias = rng.integers(-5, 6, (6, n_out, n_out, c_out)).astype(np.float32)
    got = cc.device_layer(device, kind, k, halo, x, w, b, transform=(mean, rstd, cell_bias, True), out_bias=out_bias)
    assert np.array_equal(bits(got), bits(cc.torch_layer(kind, k, halo, x, w, b, transform=(mean, rstd, cell_bias, True)) + out_bias))


@pytest.mark.parametrize("halo", [True, False], ids=["cube", "zeros"])
@pytest.mark.parametrize("kind,k,n", [("regular", 3, 6), ("regular", 7, 5), ("strided", 4, 6), ("transposed", 4, 5)])
def test_vector_loader_is_exact(device, kind, k, n, halo):
    """``c_in`` a multiple of 16 on aligned slices takes the loader that reads four channels at once: with and without the
    transform, from a slice at channel offset 4 (vector loads) and at offset 2 (the scalar loader), the same exact answer."""
    rng = np.random.default_rng(k * n)
    for c_in, c_out in ((16, 3), (48, 40)):
        S = 2
        x = rng.integers(-4, 5, (S, 6, n, n, c_in)).astype(np.float32)
        w, b = exact_layer(rng, kind, k, c_in, c_out)
        mean = rng.integers(-3, 4, (S, 6, c_in)).astype(np.float32)
        rstd = (2.0 ** rng.integers(-1, 3, (S, 6, c_in))).astype(np.float32)
        cell_bias = rng.integers(-2, 3, (6, n, n, c_in)).astype(np.float32)
        for transform in (None, (mean, rstd, cell_bias, True)):
            want = cc.torch_layer(kind, k, halo, x, w, b, transform=transform)
            for src_off in (0, 4, 2):
                got = cc.device_layer(device, kind, k, halo, x, w, b, transform=transform, src_off=src_off, src_width=c_in + 8)
                assert np.array_equal(bits(got), bits(want)), (kind, c_in, c_out, transform is not None, src_off)


@pytest.mark.parametrize("kind,k,n", [("regular", 3, 5), ("strided", 4, 6), ("transposed", 4, 3)])
def test_slices_of_wider_buffers(device, kind, k, n):
    rng = np.random.default_rng(7)
    c_in, c_out = 6, 34
    x = rng.integers(-4, 5, (2, 6, n, n, c_in)).astype(np.float32)
    w, b = exact_layer(rng, kind, k, c_in, c_out)
    want = cc.torch_layer(kind, k, True, x, w, b)
    got = cc.device_layer(device, kind, k, True, x, w, b, src_off=2, src_width=c_in + 5, dst_off=3, dst_width=c_out + 4)
    assert np.array_equal(bits(got[..., 3:3 + c_out]), bits(want))
    assert np.all(got[..., :3] == -7.0) and np.all(got[..., 3 + c_out:] == -7.0), "the neighbouring channels were written"


def test_overlapping_slices_are_refused(device):
    from fv3net_amd import _lib
    from fv3net_amd.ops import _stream

    buf = torch.zeros((1, 6, 4, 4, 8), dtype=torch.float32, device=device)
    w = torch.zeros((3, 3, 4, 4), dtype=torch.float32, device=device)

    def conv(src_off, dst_off, dst=buf):
        _lib.call_on(device, "fv3hip_cyclegan_conv", buf.data_ptr(), 8, src_off, 0, None, None, None, 0, w.data_ptr(), None, None,
                     dst.data_ptr(), 8, dst_off, 0, 1, 4, 4, 4, _lib.CYCLEGAN_CONV_REGULAR, 3, _lib.CYCLEGAN_HALO_CUBE, _stream(device))

    conv(0, 4)                                          # the two halves of one buffer
    with pytest.raises(_lib.Fv3HipError, match="overlap"):
        conv(0, 3)
    with pytest.raises(_lib.Fv3HipError, match="overlap"):
        conv(0, 0, dst=buf.reshape(-1)[8:])             # another base inside the same memory
    with pytest.raises(_lib.Fv3HipError, match="k = 4"):
        _lib.call_on(device, "fv3hip_cyclegan_conv", buf.data_ptr(), 8, 0, 0, None, None, None, 0, w.data_ptr(), None, None,
                     buf.data_ptr(), 8, 4, 0, 1, 4, 4, 4, _lib.CYCLEGAN_CONV_STRIDED, 3, _lib.CYCLEGAN_HALO_CUBE, _stream(device))
    with pytest.raises(_lib.Fv3HipError, match="halo"):
        _lib.call_on(device, "fv3hip_cyclegan_conv", buf.data_ptr(), 8, 0, 0, None, None, None, 0, w.data_ptr(), None, None,
                     buf.data_ptr(), 8, 4, 0, 1, 2, 4, 4, _lib.CYCLEGAN_CONV_REGULAR, 7, _lib.CYCLEGAN_HALO_CUBE, _stream(device))
    torch.cuda.synchronize(device)


@pytest.mark.parametrize("center", [0.0, 1e3], ids=["n01", "mean1e3"])
@pytest.mark.parametrize("n", [2, 5, 16, 48])
def test_instance_norm(device, n, center):
    """The bound is torch's own float32 CPU ``instance_norm`` measured against its float64 evaluation: 4 x that + 1e-6."""
    rng = np.random.default_rng(n)
    x = rng.normal(center, 1, (2, 6, n, n, 19)).astype(np.float32)
    truth = cc.torch_instance_norm(x.astype(np.float64), torch.float64)
    err32 = float(np.max(np.abs(cc.torch_instance_norm(x) - truth)))
    got = cc.device_instance_norm(device, x)
    err = float(np.max(np.abs(got - truth)))
    print(f"n = {n}, centre {center}: torch float32 {err32:.2e}, device {err:.2e}")
    assert err <= 4 * err32 + 1e-6
    again = cc.device_instance_norm(device, x, in_place=True)
    assert np.array_equal(bits(got), bits(again)), "two runs (one of them in place) differ"
    mean, rstd = cc.device_stats(device, x)
    xd = x.astype(np.float64)
    assert np.allclose(mean, xd.mean(axis=(2, 3)), rtol=1e-6, atol=1e-7)
    assert np.allclose(rstd, 1 / np.sqrt(xd.var(axis=(2, 3)) + 1e-5), rtol=1e-6)


def test_instance_norm_of_a_constant_face_is_zero_and_apply_options(device):
    rng = np.random.default_rng(0)
    x = np.broadcast_to(rng.normal(0, 100, (2, 6, 1, 1, 19)).astype(np.float32), (2, 6, 5, 5, 19)).copy()
    assert np.all(cc.device_instance_norm(device, x) == 0.0)
    y = rng.normal(0, 1, (2, 6, 5, 5, 19)).astype(np.float32)
    res = rng.normal(0, 1, y.shape).astype(np.float32)
    plain = cc.device_instance_norm(device, y)
    assert np.array_equal(bits(cc.device_instance_norm(device, y, relu=True)), bits(np.maximum(plain, 0)))
    assert np.array_equal(bits(cc.device_instance_norm(device, y, residual=res)), bits(plain + res))


def test_a_nan_reaches_what_float64_says(device):
    """conv 3 x 3 -> instance norm + ReLU in the next loader -> conv 3 x 3 with a NaN in one cell at a seam of sample 1."""
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (3, 6, 8, 8, 3)).astype(np.float32)
    x[1, 2, 0, 3, 1] = np.nan
    w1, w2 = (rng.normal(0, 0.3, (4, 3, 3, 3)).astype(np.float32), rng.normal(0, 0.3, (5, 4, 3, 3)).astype(np.float32))
    b1, b2 = np.zeros(4, np.float32), np.zeros(5, np.float32)
    y1 = cc.device_layer(device, "regular", 3, True, x, w1, b1)
    t1 = cc.torch_layer("regular", 3, True, x.astype(np.float64), w1, b1, dtype=torch.float64)
    assert np.array_equal(np.isnan(y1), np.isnan(t1)) and 0 < np.isnan(t1).sum() < t1.size
    normed = cc.device_instance_norm(device, y1, relu=True)
    tn = np.maximum(cc.torch_instance_norm(t1, torch.float64), 0)
    tn[np.isnan(cc.torch_instance_norm(t1, torch.float64))] = np.nan
    assert np.array_equal(np.isnan(normed), np.isnan(tn))
    mean, rstd = cc.device_stats(device, y1)
    y2 = cc.device_layer(device, "regular", 3, True, y1, w2, b2, transform=(mean, rstd, None, True))
    t2 = cc.torch_layer("regular", 3, True, tn, w2, b2, dtype=torch.float64)
    assert np.array_equal(np.isnan(y2), np.isnan(t2))
    assert np.all(np.isfinite(y2[0])) and np.all(np.isfinite(y2[2])), "the NaN of sample 1 reached another sample"
    assert np.isnan(y2[1]).any()


def test_input_layer(device):
    from fv3net_amd import _lib
    from fv3net_amd.ops import _stream

    rng = np.random.default_rng(1)
    S, n, C = 3, 5, 2
    lon, xyz = cc.synthetic_grid(n)
    x = rng.normal(0, 1, (S, 6, n, n, C)).astype(np.float32)
    bias = rng.normal(0, 1, (6, n, n, C)).astype(np.float32)
    theta = rng.uniform(0, 6.28, S).astype(np.float32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
    src, db, dl, dx, dt = up(x), up(bias), up(lon), up(xyz.transpose(0, 2, 3, 1)), up(theta)
    dst = torch.full((S, 6, n, n, C + 5), -7.0, dtype=torch.float32, device=device)
    _lib.call_on(device, "fv3hip_cyclegan_input", src.data_ptr(), C, 0, 0, db.data_ptr(), dl.data_ptr(), dx.data_ptr(), dt.data_ptr(),
                 dst.data_ptr(), C + 5, 0, 0, S, n, C, _stream(device))
    got = dst.cpu().numpy()
    assert np.array_equal(bits(got[..., :C]), bits(x + bias))
    local = (lon[None] + theta[:, None, None, None]).astype(np.float32)
    assert np.allclose(got[..., C], np.sin(local.astype(np.float64)), atol=3e-7) and np.allclose(got[..., C + 1], np.cos(local.astype(np.float64)), atol=3e-7)
    assert np.array_equal(got[..., C + 2:], np.broadcast_to(xyz.transpose(0, 2, 3, 1), (S, 6, n, n, 3)))
    plain = torch.full((S, 6, n, n, C), -7.0, dtype=torch.float32, device=device)
    _lib.call_on(device, "fv3hip_cyclegan_input", src.data_ptr(), C, 0, 0, None, None, None, None, plain.data_ptr(), C, 0, 0, S, n, C,
                 _stream(device))
    assert np.array_equal(bits(plain.cpu().numpy()), bits(x))
