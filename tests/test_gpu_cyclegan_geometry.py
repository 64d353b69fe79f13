"""The index expressions of ``cyclegan_conv_kernel`` that no whole-model test pins: sample strides on either side, faces as
narrow as the halo, the production channel counts (further channel groups on ``blockIdx.y``, the parity's weight block on top
of them) and where a non-finite value may reach.

As in ``test_gpu_cyclegan_layers.py`` the data is exact -- inputs, means, biases and context values small integers, weights in
{-1, 0, 1}, ``rstd`` a power of two -- so the float32 result does not depend on the order of the sum and the device must equal
torch bit for bit.  Every reference is checked on the CPU before it is used: torch's float32 and float64 evaluations agree and
``max |want| < 2**24`` (``exact_reference``).  Sources lie in NaN-filled buffers and destinations in sentinel-filled ones, so a
read or a write one element off its slice, its cube or its sample shows.
"""
import numpy as np
import pytest
import torch

import cyclegan_cases as cc
import fmr_cases as fc

pytestmark = pytest.mark.gpu

HALOS = pytest.mark.parametrize("halo", [True, False], ids=["cube", "zeros"])
KINDS3 = [("regular", 3, 4), ("strided", 4, 4), ("transposed", 4, 2)]     # the smallest faces with h < n
OUT_EDGE = {"regular": lambda n: n, "strided": lambda n: n // 2, "transposed": lambda n: 2 * n}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def exact_transform(rng, S, n, c_in, stats=True, cell_bias=True, relu=True):
    mean = ints(rng, -3, 3, (S, 6, c_in)) if stats else None
    rstd = (2.0 ** rng.integers(-1, 3, (S, 6, c_in))).astype(np.float32) if stats else None
    return mean, rstd, ints(rng, -2, 2, (6, n, n, c_in)) if cell_bias else None, relu


def with_statistics(transform, S, c_in):
    """The same transform with a zero mean and a unit ``rstd`` where it has none (the CPU references want arrays)."""
    if transform is None or transform[0] is not None:
        return transform
    return (np.zeros((S, 6, c_in), np.float32), np.ones((S, 6, c_in), np.float32)) + tuple(transform[2:])


def exact_case(rng, kind, k, S, n, c_in, c_out):
    from fv3net_amd.cyclegan import weight_shape

    return ints(rng, -4, 4, (S, 6, n, n, c_in)), ints(rng, -1, 1, weight_shape(kind, c_in, c_out, k)), ints(rng, -3, 3, c_out)


def exact_reference(kind, k, halo, x, w, b, transform=None, out_bias=None):
    t = with_statistics(transform, x.shape[0], x.shape[-1])
    want = cc.torch_layer(kind, k, halo, x, w, b, transform=t)
    want64 = cc.torch_layer(kind, k, halo, x, w, b, transform=t, dtype=torch.float64)
    if out_bias is not None:
        want, want64 = want + out_bias, want64 + out_bias.astype(np.float64)
    assert want.dtype == np.float32 and want64.dtype == np.float64
    assert np.array_equal(want.astype(np.float64), want64), "the case is not exact: torch's float32 and float64 differ"
    assert np.max(np.abs(want64)) < 2 ** 24
    return want


def exact_context(rng, S, n, k, c_in, c_cell, c_uni, c_out):
    x, w, b = exact_case(rng, "regular", k, S, n, c_in, c_out)
    w_ctx = ints(rng, -1, 1, (c_out, c_cell + c_uni, k, k))
    return x, w, w_ctx, b, ints(rng, -4, 4, (6, n, n, c_cell)) if c_cell else None, ints(rng, -4, 4, c_uni) if c_uni else None


def context_reference(k, halo, x, w, w_ctx, b, cell, uni, transform=None, out_bias=None):
    t = with_statistics(transform, x.shape[0], x.shape[-1])
    f64 = lambda a: a if a is None or isinstance(a, (bool, np.bool_)) else np.asarray(a, np.float64)
    want = fc.torch_context_layer(k, halo, x, w, w_ctx, b, cell, uni, transform=t)
    want64 = fc.torch_context_layer(k, halo, f64(x), f64(w), f64(w_ctx), f64(b), f64(cell), f64(uni), transform=t and tuple(f64(a) for a in t))
    if out_bias is not None:
        want, want64 = want + out_bias, want64 + out_bias.astype(np.float64)
    assert want.dtype == np.float32 and want64.dtype == np.float64
    assert np.array_equal(want.astype(np.float64), want64), "the case is not exact: torch's float32 and float64 differ"
    assert np.max(np.abs(want64)) < 2 ** 24
    return want


# -- 1. sample strides -----------------------------------------------------------------------------
# (c_in, src_gap, dst_gap, slices and transform): 16 channels with a gap of 4 keep the vector loader, a gap of 6 turns it off
GAPS = [(16, 4, 0, False), (16, 6, 0, False), (5, 3, 0, False), (16, 0, 5, False), (5, 3, 5, False), (16, 4, 5, True), (16, 6, 5, True),
        (5, 3, 5, True)]


def check_gapped(got, want, plain, S, n_out, c_out, dst_off, dst_ld, dst_gap, what):
    cubes, rest = cc.split(got, S, n_out, dst_ld, dst_gap)
    here = slice(dst_off, dst_off + c_out)
    assert np.array_equal(bits(cubes[..., here]), bits(want)), what + (int(np.sum(cubes[..., here] != want)),)
    assert np.array_equal(bits(cubes[..., here]), bits(plain[..., here])), what
    assert cc.untouched(rest), what + ("the gap between two samples was written",)
    assert cc.untouched(cubes[..., :dst_off]) and cc.untouched(cubes[..., dst_off + c_out:]), what + ("the neighbouring channels were written",)


@HALOS
@pytest.mark.parametrize("kind,k,n", KINDS3, ids=[f"{kind}{k}-n{n}" for kind, k, n in KINDS3])
def test_convolution_with_sample_strides(device, kind, k, n, halo):
    """Three samples whose cubes are ``gap`` floats apart, NaN between the source's and the sentinel between the destination's:
    torch's answer, the bits of the launch without gaps, and nothing written outside the cubes."""
    rng = np.random.default_rng(11 * n + k)
    S, c_out, n_out = 3, 35, OUT_EDGE[kind](n)
    for c_in, src_gap, dst_gap, sliced in GAPS:
        x, w, b = exact_case(rng, kind, k, S, n, c_in, c_out)
        transform = exact_transform(rng, S, n, c_in) if sliced else None
        layout = dict(src_off=4 if c_in == 16 else 2, src_width=c_in + 8, dst_off=3, dst_width=c_out + 4) if sliced else {}
        want = exact_reference(kind, k, halo, x, w, b, transform)
        plain = cc.device_layer(device, kind, k, halo, x, w, b, transform=transform, **layout)
        got = cc.device_layer(device, kind, k, halo, x, w, b, transform=transform, src_gap=src_gap, dst_gap=dst_gap, **layout)
        check_gapped(got, want, plain, S, n_out, c_out, layout.get("dst_off", 0), plain.shape[-1], dst_gap, (kind, c_in, src_gap, dst_gap, sliced))


@HALOS
def test_context_convolution_with_sample_strides(device, halo):
    rng = np.random.default_rng(12)
    S, n, k, c_out = 3, 4, 3, 35
    for c_in, src_gap, dst_gap, sliced in GAPS:
        x, w, w_ctx, b, cell, uni = exact_context(rng, S, n, k, c_in, 3, 2, c_out)
        transform = exact_transform(rng, S, n, c_in) if sliced else None
        layout = dict(src_off=4 if c_in == 16 else 2, src_width=c_in + 8, dst_off=3, dst_width=c_out + 4) if sliced else {}
        want = context_reference(k, halo, x, w, w_ctx, b, cell, uni, transform)
        plain = fc.device_context_layer(device, k, halo, x, w, w_ctx, b, cell, uni, transform=transform, **layout)
        got = fc.device_context_layer(device, k, halo, x, w, w_ctx, b, cell, uni, transform=transform, src_gap=src_gap, dst_gap=dst_gap, **layout)
        check_gapped(got, want, plain, S, n, c_out, layout.get("dst_off", 0), plain.shape[-1], dst_gap, (c_in, src_gap, dst_gap, sliced))


@HALOS
@pytest.mark.parametrize("kind,k,n", KINDS3 + [("regular", 7, 4)], ids=[f"{kind}{k}-n{n}" for kind, k, n in KINDS3 + [("regular", 7, 4)]])
def test_one_time_of_a_rollout_array(device, kind, k, n, halo):
    """The recurrent generator's layout: the destination is time ``t`` of ``[S, 2, 6, n, n, C]``, so the sample stride is two
    cubes and the base is ``t`` cubes in.  Two launches fill the two times; each leaves the other's cubes as they were.  Then
    the same with the source being one time of such an array."""
    rng = np.random.default_rng(13 * n + k)
    S, c_in, C, n_out = 3, 16, 5, OUT_EDGE[kind](n)
    cube = 6 * n_out * n_out * C
    cases = [exact_case(rng, kind, k, S, n, c_in, C) for _ in range(2)]
    wants = [exact_reference(kind, k, halo, x, w, b) for x, w, b in cases]
    assert not np.array_equal(wants[0], wants[1])
    out = torch.full((S * 2 * cube,), cc.SENTINEL, dtype=torch.float32, device=device)
    for t, (x, w, b) in enumerate(cases):
        got = cc.device_layer(device, kind, k, halo, x, w, b, dst_gap=cube, dst_lead=t * cube, into=out).reshape(S, 2, 6, n_out, n_out, C)
        assert np.array_equal(bits(got[:, 0]), bits(wants[0])), (t, "time 0")
        assert np.array_equal(bits(got[:, 1]), bits(wants[1])) if t else cc.untouched(got[:, 1]), (t, "time 1")
    x, w, b = cases[0]
    for t in range(2):
        got = cc.device_layer(device, kind, k, halo, x, w, b, src_gap=6 * n * n * c_in, src_lead=t * 6 * n * n * c_in)
        cubes, rest = cc.split(got, S, n_out, C)
        assert np.array_equal(bits(cubes), bits(wants[0])) and rest.size == 0, t


def test_short_strides_and_interleaved_cubes_are_refused(device):
    """A stride below one cube on either side of both entry points; and source and destination cubes taking turns in one
    allocation (``[S, 2, cube]`` with a common stride of two cubes), which this family refuses as an overlap of the buffers."""
    from fv3net_amd import _lib
    from fv3net_amd.ops import _stream

    S, n, c = 2, 4, 4
    cube = 6 * n * n * c
    buf = torch.zeros((S, 2, cube), dtype=torch.float32, device=device)
    other = torch.zeros((S, 2, cube), dtype=torch.float32, device=device)
    w = torch.zeros((3, 3, c, c), dtype=torch.float32, device=device)

    def conv(name, src, src_ss, dst, dst_ss):
        tail = (None, 0, None, 0, None) if name.endswith("context") else ()
        _lib.call_on(device, name, src, c, 0, src_ss, None, None, None, 0, w.data_ptr(), None, None, dst, c, 0, dst_ss, S, n, c, c,
                     _lib.CYCLEGAN_CONV_REGULAR, 3, _lib.CYCLEGAN_HALO_CUBE, *tail, _stream(device))

    for name in ("fv3hip_cyclegan_conv", "fv3hip_cyclegan_conv_context"):
        conv(name, buf.data_ptr(), 2 * cube, other.data_ptr(), 2 * cube)
        conv(name, buf.data_ptr(), cube, other.data_ptr(), cube)
        for src_ss, dst_ss in ((cube - 1, 0), (0, cube - 1), (1, 0), (0, 1)):
            with pytest.raises(_lib.Fv3HipError, match="sample stride"):
                conv(name, buf.data_ptr(), src_ss, other.data_ptr(), dst_ss)
        with pytest.raises(_lib.Fv3HipError, match="overlap"):
            conv(name, buf.data_ptr(), 2 * cube, buf.data_ptr() + 4 * cube, 2 * cube)
    torch.cuda.synchronize(device)
    assert torch.all(buf == 0) and torch.all(other == 0)


# -- 3. faces as narrow as the halo ----------------------------------------------------------------
NARROW = [("regular", 3, 1), ("regular", 5, 2), ("regular", 7, 3), ("strided", 4, 2), ("transposed", 4, 1)]


@HALOS
@pytest.mark.parametrize("kind,k,n", NARROW, ids=[f"{kind}{k}-n{n}" for kind, k, n in NARROW])
def test_faces_as_narrow_as_the_halo(device, kind, k, n, halo):
    """``h == n``: the outermost halo line is the far edge of the neighbouring face, and at ``n == 1`` every face is one cell."""
    rng = np.random.default_rng(17 * n + k)
    for S in (1, 3):
        for c_in in (3, 16):
            for c_out in (5, 40):
                x, w, b = exact_case(rng, kind, k, S, n, c_in, c_out)
                for transform in (None, exact_transform(rng, S, n, c_in)):
                    want = exact_reference(kind, k, halo, x, w, b, transform)
                    got = cc.device_layer(device, kind, k, halo, x, w, b, transform=transform)
                    assert got.shape == want.shape
                    assert np.array_equal(bits(got), bits(want)), (kind, k, n, S, c_in, c_out, transform is not None, int(np.sum(got != want)))


@HALOS
@pytest.mark.parametrize("k,n", [(3, 1), (7, 3)], ids=["k3-n1", "k7-n3"])
def test_context_on_faces_as_narrow_as_the_halo(device, k, n, halo):
    rng = np.random.default_rng(19 * n + k)
    for S in (1, 3):
        for c_in in (3, 16):
            for c_out in (5, 40):
                x, w, w_ctx, b, cell, uni = exact_context(rng, S, n, k, c_in, 3, 2, c_out)
                for transform in (None, exact_transform(rng, S, n, c_in)):
                    want = context_reference(k, halo, x, w, w_ctx, b, cell, uni, transform)
                    got = fc.device_context_layer(device, k, halo, x, w, w_ctx, b, cell, uni, transform=transform)
                    assert got.shape == want.shape
                    assert np.array_equal(bits(got), bits(want)), (k, n, S, c_in, c_out, transform is not None, int(np.sum(got != want)))


# -- 4. production channel counts at the smallest faces -----------------------------------------
WIDE = ([("regular", 3, 2, 256, 256), ("regular", 7, 4, 8, 64), ("regular", 7, 4, 64, 3), ("strided", 4, 4, 64, 128),
         ("strided", 4, 4, 128, 256), ("transposed", 4, 2, 256, 128), ("transposed", 4, 2, 128, 64)]
        + [(kind, k, n, 33, c_out) for kind, k, n in (("regular", 3, 2), ("strided", 4, 4), ("transposed", 4, 2)) for c_out in (65, 129)])
# (samples, cube halos, loader transform and per-cell output bias)
VARIANTS = [(1, True, False), (1, False, False), (3, True, False), (1, True, True)]


@pytest.mark.parametrize("kind,k,n,c_in,c_out", WIDE, ids=[f"{kind}{k}-n{n}-{ci}to{co}" for kind, k, n, ci, co in WIDE])
def test_wide_channels(device, kind, k, n, c_in, c_out):
    """Up to 144 K chunks and four channel groups (``blockIdx.y``), for the transposed kind under four parities (``blockIdx.z``)
    whose weight blocks lie ``K * N`` apart; 33 -> 65 and 129: a partial last group on the scalar loader."""
    rng = np.random.default_rng(c_in + c_out + k)
    n_out = OUT_EDGE[kind](n)
    for S, halo, extras in VARIANTS:
        x, w, b = exact_case(rng, kind, k, S, n, c_in, c_out)
        transform = exact_transform(rng, S, n, c_in) if extras else None
        out_bias = ints(rng, -5, 5, (6, n_out, n_out, c_out)) if extras else None
        want = exact_reference(kind, k, halo, x, w, b, transform, out_bias)
        got = cc.device_layer(device, kind, k, halo, x, w, b, transform=transform, out_bias=out_bias)
        assert got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), (kind, c_in, c_out, S, halo, extras, int(np.sum(got != want)))


def test_wide_context_layers(device):
    """The production step layer (256 + 3 + 2 -> 256 at k = 3) and the argument pattern of the recurrent generator's first layer:
    k = 7 on two state channels with a pending per-cell bias and no statistics, x, y, z as the per-cell context."""
    rng = np.random.default_rng(23)
    for S, halo, extras in VARIANTS:
        n, k = 2, 3
        x, w, w_ctx, b, cell, uni = exact_context(rng, S, n, k, 256, 3, 2, 256)
        transform = exact_transform(rng, S, n, 256) if extras else None
        out_bias = ints(rng, -5, 5, (6, n, n, 256)) if extras else None
        want = context_reference(k, halo, x, w, w_ctx, b, cell, uni, transform, out_bias)
        got = fc.device_context_layer(device, k, halo, x, w, w_ctx, b, cell, uni, transform=transform, out_bias=out_bias)
        assert np.array_equal(bits(got), bits(want)), ("step", S, halo, extras, int(np.sum(got != want)))
        n, k = 8, 7
        x, w, w_ctx, b, cell, uni = exact_context(rng, S, n, k, 2, 3, 0, 64)
        transform = exact_transform(rng, S, n, 2, stats=extras, relu=extras)
        out_bias = ints(rng, -5, 5, (6, n, n, 64)) if extras else None
        want = context_reference(k, halo, x, w, w_ctx, b, cell, uni, transform, out_bias)
        got = fc.device_context_layer(device, k, halo, x, w, w_ctx, b, cell, uni, transform=transform, out_bias=out_bias)
        assert np.array_equal(bits(got), bits(want)), ("first", S, halo, extras, int(np.sum(got != want)))


# -- 5. where a non-finite value reaches -----------------------------------------------------------
def classes(a):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 0)))


@HALOS
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("kind,n", [("strided", 8), ("transposed", 4)])
def test_a_non_finite_cell_reaches_what_float64_says(device, kind, n, value, halo):
    """One value in a seam cell of sample 1 of 3.  Real-valued weights: no zero weight meets an infinity."""
    from fv3net_amd.cyclegan import weight_shape

    rng = np.random.default_rng(29 + n)
    c_in, c_out = 3, 5
    clean = rng.normal(0, 1, (3, 6, n, n, c_in)).astype(np.float32)
    w = rng.normal(0, 0.3, weight_shape(kind, c_in, c_out, 4)).astype(np.float32)
    assert np.all(w != 0)
    b = rng.normal(0, 1, c_out).astype(np.float32)
    x = clean.copy()
    x[1, 2, 0, n // 2 - 1, 1] = value
    truth = cc.torch_layer(kind, 4, halo, x, w, b, dtype=torch.float64)
    hit = classes(truth) != 0
    assert hit[1].any() and not hit[1].all() and not hit[0].any() and not hit[2].any()
    assert np.any(hit[1, [t for t in range(6) if t != 2]]) == halo, "the value should cross the seam with cube halos and only then"
    got, base = cc.device_layer(device, kind, 4, halo, x, w, b), cc.device_layer(device, kind, 4, halo, clean, w, b)
    assert np.array_equal(classes(got), classes(truth))
    assert np.array_equal(bits(got[[0, 2]]), bits(base[[0, 2]])), "the value of sample 1 reached another sample"
    assert np.array_equal(bits(got[1][~hit[1]]), bits(base[1][~hit[1]]))


@HALOS
def test_a_nan_in_the_cell_context_reaches_what_float64_says(device, halo):
    rng = np.random.default_rng(31)
    S, n, k, c_in, c_out = 3, 8, 3, 3, 5
    x = rng.normal(0, 1, (S, 6, n, n, c_in)).astype(np.float32)
    w, w_ctx = rng.normal(0, 0.3, (c_out, c_in, k, k)).astype(np.float32), rng.normal(0, 0.3, (c_out, 5, k, k)).astype(np.float32)
    b, uni = rng.normal(0, 1, c_out).astype(np.float32), rng.normal(0, 1, 2).astype(np.float32)
    clean = rng.normal(0, 1, (6, n, n, 3)).astype(np.float32)
    cell = clean.copy()
    cell[2, 0, 3, 1] = np.nan
    f64 = lambda a: np.asarray(a, np.float64)
    truth = fc.torch_context_layer(k, halo, f64(x), f64(w), f64(w_ctx), f64(b), f64(cell), f64(uni))
    hit = np.isnan(truth)
    assert np.all(np.isfinite(truth[~hit])) and np.array_equal(hit, np.broadcast_to(hit[:1], hit.shape)), "the context is every sample's"
    on_face, elsewhere = int(hit[0, 2].sum()), int(hit[0].sum() - hit[0, 2].sum())
    assert on_face == 2 * 3 * c_out and elsewhere == (3 * c_out if halo else 0), (on_face, elsewhere)
    got = fc.device_context_layer(device, k, halo, x, w, w_ctx, b, cell, uni)
    base = fc.device_context_layer(device, k, halo, x, w, w_ctx, b, clean, uni)
    assert np.array_equal(classes(got), classes(truth))
    assert np.array_equal(bits(got[~hit]), bits(base[~hit]))
