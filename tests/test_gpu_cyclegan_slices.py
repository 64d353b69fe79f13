"""``fv3hip_cyclegan_stats``, ``_apply`` and ``_input`` on slices: a row length, channel offset and sample stride of its own
for every operand, apply's per-cell bias and its residual in another buffer or in the destination itself, and the grid-stride
loop past the cap of 16 384 blocks (4 194 304 elements).

Data is exact as in ``test_gpu_cyclegan_geometry.py`` (integers in [-4, 4], integer means, biases and residuals, ``rstd`` a
power of two), so apply and the copied channels of input are compared bit for bit with ``cyclegan_cases.apply_np``, the kernel's
expression in numpy float32; ``test_apply_np_is_exact`` pins that expression against float64 on the host.  Sources lie in
NaN-filled buffers, destinations in sentinel-filled ones.
"""
import itertools

import numpy as np
import pytest
import torch

import cyclegan_cases as cc

gpu = pytest.mark.gpu
BLOCK_CAP = 16384 * 256   # grid_stride_blocks: elements that one pass of the capped grid covers


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def apply_case(rng, S, n, c):
    """x, mean, rstd, bias, res"""
    return (ints(rng, -4, 4, (S, 6, n, n, c)), ints(rng, -3, 3, (S, 6, c)), (2.0 ** rng.integers(-1, 3, (S, 6, c))).astype(np.float32),
            ints(rng, -2, 2, (6, n, n, c)), ints(rng, -4, 4, (S, 6, n, n, c)))


def exact_apply(x, mean, rstd, bias, relu, res):
    want, want64 = cc.apply_np(x, mean, rstd, bias, relu, res), cc.apply_np(x, mean, rstd, bias, relu, res, dtype=np.float64)
    assert want.dtype == np.float32 and want64.dtype == np.float64
    assert np.array_equal(want.astype(np.float64), want64) and np.max(np.abs(want64)) < 2 ** 24
    return want


def test_apply_np_is_exact():
    """On the host: the float32 expression equals its float64 evaluation on the tests' data for every option, every option
    changes the answer, and each step is what it says."""
    rng = np.random.default_rng(0)
    x, mean, rstd, bias, res = apply_case(rng, 2, 3, 5)
    seen = []
    for stats, with_bias, relu, with_res in itertools.product((False, True), repeat=4):
        seen.append(exact_apply(x, mean if stats else None, rstd if stats else None, bias if with_bias else None, relu, res if with_res else None))
    assert all(not np.array_equal(a, b) for a, b in itertools.combinations(seen, 2))
    m, r = mean[:, :, None, None].astype(np.float64), rstd[:, :, None, None].astype(np.float64)
    assert np.array_equal(seen[-1], np.maximum((x - m) * r + bias, 0) + res)
    assert np.array_equal(seen[0], x)
    v = cc.apply_np(np.array([np.nan, -1.0, 2.0], np.float32).reshape(1, 1, 1, 3, 1), relu=True).ravel()
    assert np.isnan(v[0]) and v[1] == 0 and v[2] == 2, "ReLU keeps a NaN"


# -- statistics ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", [1, 16, 17, 256])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_statistics_of_a_slice(device, n, C):
    """From channel 3 of a NaN-filled buffer ``C + 7`` wide, and with five NaNs between the two samples: the bits of the
    contiguous call.  ``C`` 17 and 256: a partial and a sixteenth block of channels."""
    rng = np.random.default_rng(100 * n + C)
    x = ints(rng, -4, 4, (2, 6, n, n, C))
    mean, rstd = cc.device_stats(device, x)
    xd = x.astype(np.float64)
    assert np.allclose(mean, xd.mean(axis=(2, 3)), rtol=1e-6, atol=1e-7)
    assert np.allclose(rstd, 1 / np.sqrt(xd.var(axis=(2, 3)) + 1e-5), rtol=1e-6)
    if n == 1:
        assert np.array_equal(bits(mean), bits(x[:, :, 0, 0])), "the mean of one cell is the cell"
        assert np.allclose(rstd, np.float32(1 / np.sqrt(1e-5)), rtol=1e-6)
    for layout in (dict(src_off=3, src_width=C + 7), dict(src_gap=5), dict(src_off=3, src_width=C + 7, src_gap=5)):
        m, r = cc.device_stats(device, x, **layout)
        assert np.array_equal(bits(m), bits(mean)) and np.array_equal(bits(r), bits(rstd)), layout


# -- apply -----------------------------------------------------------------------------------------
def check_apply(device, case, stats, with_bias, relu, res_mode, in_place, layout, what):
    x, mean, rstd, bias, res = case
    c = x.shape[-1]
    residual = None if res_mode == "none" else x if (in_place and res_mode == "dst") else res
    want = exact_apply(x, mean if stats else None, rstd if stats else None, bias if with_bias else None, relu, residual)
    cubes, rest = cc.device_apply(device, x, mean if stats else None, rstd if stats else None, bias if with_bias else None, relu,
                                  None if res_mode == "none" else res, in_place=in_place, res_is_dst=res_mode == "dst", **layout)
    off = layout.get("src_off" if in_place else "dst_off", 0)
    fill = np.nan if in_place else cc.SENTINEL
    assert np.array_equal(bits(cubes[..., off:off + c]), bits(want)), what + (int(np.sum(cubes[..., off:off + c] != want)),)
    assert cc.untouched(cubes[..., :off], fill) and cc.untouched(cubes[..., off + c:], fill), what + ("the neighbouring channels were written",)
    assert cc.untouched(rest, fill), what + ("the gap between two samples was written",)


@gpu
@pytest.mark.parametrize("in_place", [False, True], ids=["into-a-slice", "in-place"])
@pytest.mark.parametrize("res_mode", ["none", "own", "dst"])
def test_apply_options_on_slices(device, res_mode, in_place):
    """{statistics, none} x {per-cell bias, none} x ReLU, with no residual, a residual in a buffer with a row length and offset of
    its own, and the residual being the destination; into a slice of a wider sentinel buffer and in place."""
    rng = np.random.default_rng(3)
    layout = dict(src_off=2, src_width=5 + 3, res_off=1, res_width=5 + 4, dst_off=3, dst_width=5 + 5)
    for stats, with_bias, relu in itertools.product((True, False), repeat=3):
        check_apply(device, apply_case(rng, 2, 3, 5), stats, with_bias, relu, res_mode, in_place, layout, (stats, with_bias, relu))


@gpu
@pytest.mark.parametrize("in_place", [False, True], ids=["into-a-slice", "in-place"])
@pytest.mark.parametrize("res_mode", ["none", "own", "dst"])
def test_apply_with_sample_strides(device, res_mode, in_place):
    """Three samples; source, residual and destination each with a gap of its own, with and without channel slices."""
    rng = np.random.default_rng(4)
    gaps = dict(src_gap=3, res_gap=5, dst_gap=7)
    for layout in (gaps, dict(src_off=2, src_width=8, res_off=1, res_width=9, dst_off=3, dst_width=10, **gaps), dict(dst_gap=7), dict(src_gap=3)):
        for stats, with_bias, relu in ((True, True, True), (False, False, False)):
            check_apply(device, apply_case(rng, 3, 2, 5), stats, with_bias, relu, res_mode, in_place, layout, (sorted(layout), stats))


@gpu
def test_apply_past_the_block_cap(device):
    """n = 24 with 1 280 channels: 4 423 680 elements, so the threads of the first 896 blocks take a second element each."""
    rng = np.random.default_rng(5)
    case = apply_case(rng, 1, 24, 1280)
    assert BLOCK_CAP < case[0].size < 2 * BLOCK_CAP
    check_apply(device, case, True, True, True, "own", False, {}, ("past the cap",))


# -- input -----------------------------------------------------------------------------------------
def check_input(device, rng, S, n, C, layout):
    lon, xyz = cc.synthetic_grid(n)
    xyz = np.ascontiguousarray(xyz.transpose(0, 2, 3, 1))
    x, bias = ints(rng, -4, 4, (S, 6, n, n, C)), ints(rng, -2, 2, (6, n, n, C))
    theta = (0.5 + 1.75 * np.arange(S)).astype(np.float32)
    off = layout.get("dst_off", 0)
    cubes, rest = cc.device_input(device, x, bias, lon, xyz, theta, **layout)
    got = cubes[..., off:off + C + 5]
    assert np.array_equal(bits(got[..., :C]), bits(x + bias))
    local = (lon[None] + theta[:, None, None, None]).astype(np.float32).astype(np.float64)
    err = max(float(np.max(np.abs(got[..., C] - np.sin(local)))), float(np.max(np.abs(got[..., C + 1] - np.cos(local)))))
    assert err <= 3e-7, err
    assert np.array_equal(bits(got[..., C + 2:]), bits(np.broadcast_to(xyz, (S, 6, n, n, 3))))
    assert cc.untouched(cubes[..., :off]) and cc.untouched(cubes[..., off + C + 5:]) and cc.untouched(rest)
    return x, bias


@gpu
def test_input_on_slices_with_sample_strides(device):
    rng = np.random.default_rng(6)
    S, n, C = 3, 5, 2
    layout = dict(src_off=1, src_width=C + 3, src_gap=3, dst_off=2, dst_width=C + 5 + 4, dst_gap=5)
    x, bias = check_input(device, rng, S, n, C, layout)
    for b in (bias, None):     # without the geographic features: the state (+ bias) alone
        cubes, rest = cc.device_input(device, x, b, **layout)
        assert np.array_equal(bits(cubes[..., 2:2 + C]), bits(x if b is None else x + b))
        assert cc.untouched(cubes[..., :2]) and cc.untouched(cubes[..., 2 + C:]) and cc.untouched(rest)


@gpu
def test_input_past_the_block_cap(device):
    n, C = 24, 1275
    assert BLOCK_CAP < 6 * n * n * (C + 5) < 2 * BLOCK_CAP
    check_input(device, np.random.default_rng(7), 1, n, C, {})


# -- refusals --------------------------------------------------------------------------------------
@gpu
def test_refusals(device):
    from fv3net_amd import _lib
    from fv3net_amd.ops import _stream

    S, n, c = 2, 2, 4
    cube = 6 * n * n * c
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=device)
    a, b, r, st = z(S, cube), z(S, cube), z(S, cube), z(2, S, 6, c)
    wide, geo = z(S, 6, n, n, 3 * c), z(6, n, n, 3)
    stream = _stream(device)
    p = lambda t: None if t is None else t.data_ptr()

    def stats(ss):
        _lib.call_on(device, "fv3hip_cyclegan_stats", p(a), c, 0, ss, p(st[0]), p(st[1]), S, n, c, 1e-5, stream)

    def apply(src_ss=0, res_ss=0, dst_ss=0, src=a, src_ld=c, src_off=0, res=r, res_ld=c, res_off=0, dst=b, dst_ld=c, dst_off=0):
        _lib.call_on(device, "fv3hip_cyclegan_apply", p(src), src_ld, src_off, src_ss, None, None, None, 0, p(res), res_ld, res_off, res_ss,
                     p(dst), dst_ld, dst_off, dst_ss, S, n, c, stream)

    def inp(src_ss=0, dst_ss=0, lon=None, xyz=None, theta=None):
        _lib.call_on(device, "fv3hip_cyclegan_input", p(a), c, 0, src_ss, None, p(lon), p(xyz), p(theta), p(wide), 3 * c, 0, dst_ss, S, n, c,
                     stream)

    stats(0), stats(cube), apply(), apply(cube, cube, cube), inp(), inp(cube, 3 * cube), inp(lon=geo, xyz=geo, theta=geo)
    for short in (cube - 1, 1):
        for call in (lambda: stats(short), lambda: apply(src_ss=short), lambda: apply(res_ss=short), lambda: apply(dst_ss=short),
                     lambda: inp(src_ss=short), lambda: inp(dst_ss=3 * short)):
            with pytest.raises(_lib.Fv3HipError, match="sample stride"):
                call()
    apply(src=wide, src_ld=3 * c, dst=wide, dst_ld=3 * c, dst_off=c)                       # the two halves of one buffer
    apply(src=wide, src_ld=3 * c, dst=wide, dst_ld=3 * c, res=wide, res_ld=3 * c)          # all three the same slice
    with pytest.raises(_lib.Fv3HipError, match="overlap"):
        apply(src=wide, src_ld=3 * c, dst=wide, dst_ld=3 * c, dst_off=c - 1)
    with pytest.raises(_lib.Fv3HipError, match="overlap"):
        apply(res=wide, res_ld=3 * c, res_off=1, dst=wide, dst_ld=3 * c, dst_off=2)
    for kwargs in (dict(lon=geo), dict(xyz=geo), dict(lon=geo, theta=geo), dict(xyz=geo, theta=geo), dict(theta=geo)):
        with pytest.raises(_lib.Fv3HipError, match="come together"):
            inp(**kwargs)
    torch.cuda.synchronize(device)
