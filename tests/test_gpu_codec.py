"""The column codec kernels (fv3net_amd/csrc/codec.hip) on the MI355X against the restatement (tests/codec_np.py).

Gates: the scale-only form -- the normalisation alone -- is bit-identical to numpy float32; dense chains go through the
project's MLP gate (tests/tolerances.py, 1e-5 of each level's scale and no worse than 8x the float32 CPU evaluation); the
affine float64 codec stays within 1e-12 x max|want| per latent unit / output level, compared class first
(reservoir_cases.check).  Each shape case runs once over 257 columns through its gate; the smaller column counts (1, 63 as a
7 x 9 extent, 64, 65) and every kind of source and output view must then reproduce the bits of its leading columns, which
holds them to the same gate.
"""
import ctypes

import numpy as np
import pytest
import torch

from fv3net_amd import _lib
from fv3net_amd.reservoir import DenseAutoencoder, SkTransformer

import codec_cases as C
import codec_np as N
import reservoir_cases as RC
import tolerances

pytestmark = pytest.mark.gpu


def _view(a, view):
    """A device (x, y, z) tensor of ``a`` that is plain, an (x, y, z) view of a (z, y, x) array, or every second y and all
    but the last z of a larger array."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if view == "transposed":
        t = t.permute(2, 1, 0).contiguous().permute(2, 1, 0)
    elif view == "strided":
        big = torch.zeros((a.shape[0], 2 * a.shape[1], a.shape[2] + 1), dtype=t.dtype, device="cuda")
        big[:, ::2, :a.shape[2]] = t
        t = big[:, ::2, :a.shape[2]]
    return t


def _sources(arrays, count, kind, views):
    n = len(arrays)
    views = [views] * n if isinstance(views, str) else [views[v % len(views)] for v in range(n)]
    return [_view(a.astype(dt), view) for a, dt, view in zip(C.as_extent(arrays, count), C.source_dtypes(kind, n), views)]


def _strided_outputs(codec, nx, ny):
    """(views to decode into, the arrays behind them): every second y and all but the last z, filled with a sentinel."""
    bigs = [torch.full((nx, 2 * ny, nz + 1), -7.0, dtype=codec.output_dtype, device="cuda")
            for nz in codec.original_feature_sizes]
    return [b[:, ::2, :nz] for b, nz in zip(bigs, codec.original_feature_sizes)], bigs


def _assert_untouched(bigs, sizes):
    for b, nz in zip(bigs, sizes):
        assert torch.all(b[:, 1::2, :] == -7.0) and torch.all(b[:, :, nz:] == -7.0), "a store landed outside its view"


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _variable_gate(want):
    """1e-12 x max|want| over one decoded variable."""
    return C.AFFINE_GATE * np.abs(np.where(np.isfinite(want), want, 0.0)).max()


def _encode_all_views(codec, x, full, name):
    """Every column count, source dtype and kind of view reproduces the leading columns of the 257-column result."""
    for count, (nx, ny) in C.COLUMN_COUNTS.items():
        for kind in C.SOURCES:
            for views in C.VIEWS:
                got = codec.encode_device(_sources(x, count, kind, views)).cpu().numpy()
                assert _bits_equal(got.reshape(count, -1), full[:count]), (name, count, kind, views)


def _decode_all_views(codec, latent, full, name):
    for count, (nx, ny) in C.COLUMN_COUNTS.items():
        for dtype in (np.float32, np.float64):
            z = torch.from_numpy(np.ascontiguousarray(latent[:count]).astype(dtype).reshape(nx, ny, -1)).cuda()
            outs, bigs = _strided_outputs(codec, nx, ny)
            for o, want in zip(codec.decode_device(z, outs), full):
                assert _bits_equal(o.cpu().numpy().reshape(count, -1), want[:count]), (name, count, dtype)
            _assert_untouched(bigs, codec.original_feature_sizes)
            for o, want in zip(codec.decode_device(z), full):
                assert _bits_equal(o.cpu().numpy().reshape(count, -1), want[:count]), (name, count, dtype, "plain")


# ---------------------------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(C.SCALE_ONLY))
def test_scale_only_is_bit_identical_to_numpy_float32(name):
    spec, x, latent = C.cached(C.scale_only_case, name)
    codec = C.dense_codec(spec)
    assert codec.n_latent_dims == sum(spec["sizes"])
    want = N.normalise32(spec, x)
    got = codec.encode_device(_sources(x, 257, "f64", "plain")).cpu().numpy().reshape(257, -1)
    assert _bits_equal(got, want), "the normalisation differs from numpy float32"
    _encode_all_views(codec, x, want, name)
    want_dec = N.dense_decode(spec, latent, np.float32)
    _decode_all_views(codec, latent, want_dec, name)


@pytest.mark.parametrize("name", list(C.DENSE))
def test_dense_encode(name):
    spec, x, _ = C.cached(C.dense_case, name)
    codec = C.dense_codec(spec)
    got = codec.encode_device(_sources(x, 257, "f64", "plain"))
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 257, codec.n_latent_dims)
    got = got.cpu().numpy().reshape(257, -1)
    ratio = tolerances.assert_close_per_level(got, N.dense_encode(spec, x, np.float64), cpu32=N.dense_encode(spec, x, np.float32),
                                              name=f"encode {name}", rel=1e-5)
    print(f"gate fraction [dense encode] {name}: {ratio / 1e-5:.3g}")
    _encode_all_views(codec, x, got, name)


@pytest.mark.parametrize("name", list(C.DENSE))
def test_dense_decode(name):
    spec, _, latent = C.cached(C.dense_case, name)
    codec = C.dense_codec(spec)
    outs = [o.cpu().numpy().reshape(257, -1) for o in codec.decode_device(torch.from_numpy(latent.reshape(1, 257, -1)).cuda())]
    truth, cpu32 = N.dense_decode(spec, latent, np.float64), N.dense_decode(spec, latent, np.float32)
    for v, (g, t, c) in enumerate(zip(outs, truth, cpu32)):
        assert g.dtype == np.float32
        ratio = tolerances.assert_close_per_level(g, t, cpu32=c, name=f"decode {name} variable {v}", rel=1e-5)
        print(f"gate fraction [dense decode] {name} variable {v}: {ratio / 1e-5:.3g}")
    lo, hi = spec["min"][0], spec["max"][-1]
    assert (outs[0] == np.float32(lo)).any() and (outs[-1] == np.float32(hi)).any(), "the limits were never reached"
    assert outs[0].min() >= np.float32(lo) and outs[-1].max() <= np.float32(hi)
    _decode_all_views(codec, latent, outs, name)


# ---------------------------------------------------------------------------------------------
# affine
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(C.AFFINE))
def test_affine_encode(name):
    spec, x, _, want, _ = C.cached(C.affine_case, name)
    codec = C.affine_codec(spec)
    got = codec.encode_device(_sources(x, 257, "f64", "plain"))
    assert got.dtype == torch.float64
    got = got.cpu().numpy().reshape(257, -1)
    print(f"gate fraction [affine encode] {name}: {RC.check(got, want, C.affine_gate(want), name):.3g}")
    for count, (nx, ny) in C.COLUMN_COUNTS.items():
        for views in C.VIEWS + (C.VIEWS,):
            again = codec.encode_device(_sources(x, count, "f64", views)).cpu().numpy()
            assert _bits_equal(again.reshape(count, -1), got[:count]), (name, count, views)
    for kind in ("f32", "mixed"):  # a float32 source is widened first: its own expectation, through the same gate
        src = _sources(x, 257, kind, C.VIEWS)
        w = N.affine_encode(spec, [s.cpu().numpy().astype(np.float64).reshape(257, -1) for s in src])
        full = codec.encode_device(src).cpu().numpy().reshape(257, -1)
        RC.check(full, w, C.affine_gate(w), f"{name} {kind}")
        for count in C.COLUMN_COUNTS:
            again = codec.encode_device(_sources(x, count, kind, "strided")).cpu().numpy()
            assert _bits_equal(again.reshape(count, -1), full[:count]), (name, count, kind)


@pytest.mark.parametrize("name", list(C.AFFINE))
def test_affine_decode(name):
    spec, _, latent, _, want = C.cached(C.affine_case, name)
    codec = C.affine_codec(spec)
    outs = [o.cpu().numpy().reshape(257, -1) for o in codec.decode_device(torch.from_numpy(latent.reshape(1, 257, -1)).cuda())]
    for v, (g, w) in enumerate(zip(outs, want)):
        assert g.dtype == np.float64
        print(f"gate fraction [affine decode] {name} variable {v}: {RC.check(g, w, _variable_gate(w), f'{name} {v}'):.3g}")
    if spec["positive"]:
        assert all((g >= 0).all() for g in outs) and any((g == 0).any() for g in outs)
    for count, (nx, ny) in C.COLUMN_COUNTS.items():
        z = torch.from_numpy(np.ascontiguousarray(latent[:count]).reshape(nx, ny, -1)).cuda()
        views, bigs = _strided_outputs(codec, nx, ny)
        for o, full in zip(codec.decode_device(z, views), outs):
            assert _bits_equal(o.cpu().numpy().reshape(count, -1), full[:count]), (name, count)
        _assert_untouched(bigs, codec.original_feature_sizes)
    # a float32 latent is widened first
    z32 = torch.from_numpy(latent.astype(np.float32).reshape(1, 257, -1)).cuda()
    w = N.affine_decode(spec, latent.astype(np.float32).astype(np.float64))
    full = [o.cpu().numpy().reshape(257, -1) for o in codec.decode_device(z32)]
    for v, (o, wv) in enumerate(zip(full, w)):
        RC.check(o, wv, _variable_gate(wv), f"{name} f32 latent {v}")
    for count, (nx, ny) in C.COLUMN_COUNTS.items():
        for o, f in zip(codec.decode_device(z32.reshape(257, -1)[:count].reshape(nx, ny, -1)), full):
            assert _bits_equal(o.cpu().numpy().reshape(count, -1), f[:count]), (name, count, "f32 latent")


# ---------------------------------------------------------------------------------------------
# non-finite values
# ---------------------------------------------------------------------------------------------


def _planted(x, column, values):
    out = [a.copy() for a in x]
    for (v, z), value in values.items():
        out[v][column, z] = value
    return out


@pytest.mark.parametrize("value", list(RC.NON_FINITE))
@pytest.mark.parametrize("kind", ["dense", "affine"])
def test_non_finite_input_stays_in_its_column(kind, value):
    """NaN or +-Inf in one column (in the middle of a tile): that column follows the restatement's classes, every other
    column keeps the bits of the clean run."""
    if kind == "dense":
        spec, x, _ = C.cached(C.dense_case, "default")
        codec = C.dense_codec(spec)
    else:
        spec, x, _, _, _ = C.cached(C.affine_case, "default")
        codec = C.affine_codec(spec)
    clean = codec.encode_device(_sources(x, 257, "f64", "plain")).cpu().numpy().reshape(257, -1)
    bad = _planted(x, 70, {(1, 3): RC.NON_FINITE[value]})
    got = codec.encode_device(_sources(bad, 257, "f64", "plain")).cpu().numpy().reshape(257, -1)
    others = np.arange(257) != 70
    assert _bits_equal(got[others], clean[others]), "a non-finite value reached another column"
    if kind == "dense":
        want = N.dense_encode(spec, bad, np.float64)[70]
        RC.check(got[70], want, 1e-4 * np.abs(np.where(np.isfinite(want), want, 0)).max() + 1e-30, f"dense {value}")
    else:
        want = N.affine_encode(spec, bad)[70]
        RC.check(got[70], want, C.affine_gate(clean), f"affine {value}")
    # the same through the decoder
    lat_clean = clean.copy()
    lat_bad = clean.copy()
    lat_bad[70, 0] = RC.NON_FINITE[value]
    dec = lambda z: [o.cpu().numpy().reshape(257, -1)  # noqa: E731
                     for o in codec.decode_device(torch.from_numpy(z.reshape(1, 257, -1)).cuda())]
    for v, (g, c) in enumerate(zip(dec(lat_bad), dec(lat_clean))):
        assert _bits_equal(g[others], c[others]), f"decode: a non-finite latent reached another column (variable {v})"
    want = (N.dense_decode(spec, lat_bad[70:71], np.float64) if kind == "dense" else N.affine_decode(spec, lat_bad[70:71]))
    for v, (g, w) in enumerate(zip(dec(lat_bad), want)):
        assert np.array_equal(RC.classes(g[70]), RC.classes(w[0].astype(g.dtype))), f"decode classes, variable {v}"


def test_dense_zero_denominator_and_float32_range():
    """A scale of exactly -1e-7f makes the denominator 0 (+-Inf, and NaN where the source is the center); a float64 source
    beyond float32's range is +-Inf after the cast.  Scale-only, so bit for bit."""
    spec, x, _ = C.cached(C.scale_only_case, "s7")
    spec = dict(spec, scale=spec["scale"].copy())
    spec["scale"][2] = np.float32(-1.0e-7)
    x = [a.copy() for a in x]
    x[0][5, 2] = np.float64(spec["center"][2])  # 0 / 0
    x[0][6, 0] = 1.0e39
    x[1][7, 0] = -1.0e39
    want = N.normalise32(spec, x)
    assert np.isnan(want[5, 2]) and np.isinf(want[:, 2]).sum() == 256 and want[6, 0] == np.inf and want[7, 5] == -np.inf
    got = C.dense_codec(spec).encode_device(_sources(x, 257, "f64", C.VIEWS)).cpu().numpy().reshape(257, -1)
    RC.check(got, want, 0.0, "zero denominator / float32 range")
    assert _bits_equal(got[np.isfinite(want)], want[np.isfinite(want)])


def test_dense_limits_pass_nan():
    spec, _, latent = C.cached(C.scale_only_case, "s7")
    spec = dict(spec, min=[-0.25, None, 0.5], max=[0.25, 0.125, None])
    latent = latent.copy()
    latent[3, :] = np.nan
    latent[4, :] = np.inf
    latent[5, :] = -np.inf
    want = N.dense_decode(spec, latent, np.float32)
    assert all(np.isnan(w[3]).all() for w in want)
    outs = C.dense_codec(spec).decode_device(torch.from_numpy(latent.reshape(1, 257, -1)).cuda())
    for v, (o, w) in enumerate(zip(outs, want)):
        got = o.cpu().numpy().reshape(257, -1)
        RC.check(got, w, 0.0, f"limits, variable {v}")
        assert _bits_equal(got[~np.isnan(w)], w[~np.isnan(w)])


def test_affine_enforce_positive_on_nan_zero_and_negatives():
    spec, _, latent, _, _ = C.cached(C.affine_case, "k7")
    assert spec["positive"]
    latent = latent.copy()
    latent[3, 0] = np.nan
    latent[4, 0] = np.inf
    latent[5, 0] = -np.inf
    want = N.affine_decode(spec, latent)
    assert all((w[3] == 0).all() for w in want), "np.where turns a NaN into 0.0"
    outs = C.affine_codec(spec).decode_device(torch.from_numpy(latent.reshape(1, 257, -1)).cuda())
    for v, (o, w) in enumerate(zip(outs, want)):
        got = o.cpu().numpy().reshape(257, -1)
        RC.check(got, w, _variable_gate(w), f"enforce positive, variable {v}")
        assert (got >= 0).all()
    # -0.0 compares >= 0 and passes, a negative becomes 0.0: an identity codec, against the restatement
    ident = {"sizes": [3], "mean": None, "std": None, "pca_mean": np.zeros(3), "components": np.eye(3), "ev": None,
             "positive": True}
    z = np.array([[[-0.0, -1.5, 2.0]]])
    got = C.affine_codec(ident).decode_device(torch.from_numpy(z).cuda())[0].cpu().numpy()
    RC.check(got, N.affine_decode(ident, z)[0], 0.0, "identity")
    assert got.reshape(-1).tolist() == [0.0, 0.0, 2.0]


# ---------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------


def _einval(codec, match):
    with pytest.raises(_lib.Fv3HipError, match=match) as err:
        codec._handle_on(torch.device("cuda"))
    assert err.value.code == _lib.EINVAL


def test_caps_come_back_as_einval():
    rng = np.random.RandomState(0)
    layer = lambda a, b: (rng.randn(a, b).astype(np.float32), np.zeros(b, np.float32))  # noqa: E731

    def dense(sizes, widths, n_latent, dec_widths=None):
        k = sum(sizes)
        enc = [layer(a, b) for a, b in zip([k, *widths], [*widths, n_latent])]
        dw = widths if dec_widths is None else dec_widths
        dec = [layer(a, b) for a, b in zip([n_latent, *dw], dw)]
        last = dw[-1] if dw else n_latent
        heads = [layer(last, nz) for nz in sizes]
        u = lambda ls, i: [x[i] for x in ls]  # noqa: E731
        return DenseAutoencoder(np.zeros(k), np.ones(k), sizes, u(enc, 0), u(enc, 1), u(dec, 0), u(dec, 1), u(heads, 0),
                                u(heads, 1))

    _einval(dense([1] * 17, [4], 2), r"n_variables must be in \[1, 16\]")
    _einval(dense([1025], [4], 2), "exceeds the cap of 1024 features")
    _einval(dense([4, 4], [257], 2), r"width 257 is outside \[1, 256\]")
    _einval(dense([300], [4], 257), r"outside \[1, 256\]")
    _einval(dense([4], [4] * 8, 2), "exceed the cap of 8 layers per side")
    _einval(dense([4], [4], 2, dec_widths=[4] * 9), "exceed the cap of 8 layers per side")
    _einval(SkTransformer(np.zeros((257, 300)), np.zeros(300), [300]), r"n_latent 257 is outside \[1, 256\]")
    _einval(SkTransformer(np.zeros((2, 1025)), np.zeros(1025), [1025]), "exceeds the cap of 1024 features")
    # at the caps it is accepted
    dense([64] * 16, [256] * 7, 256)._handle_on(torch.device("cuda"))


def test_call_errors():
    spec, x, _ = C.cached(C.scale_only_case, "s7")
    codec = C.dense_codec(spec)
    h = codec._handle_on(torch.device("cuda"))
    lat = torch.empty((1, 257, 7), device="cuda")
    with pytest.raises(_lib.Fv3HipError, match="bad extent") as err:
        _lib.call("fv3hip_codec_decode", h, lat.data_ptr(), _lib.F32, 0, 257, (ctypes.c_void_p * 3)(),
                  (ctypes.c_int64 * 9)(), None)
    assert err.value.code == _lib.EINVAL
    with pytest.raises(_lib.Fv3HipError, match="latent dtype") as err:
        _lib.call("fv3hip_codec_decode", h, lat.data_ptr(), _lib.I32, 1, 257, (ctypes.c_void_p * 3)(),
                  (ctypes.c_int64 * 9)(), None)
    assert err.value.code == _lib.EINVAL
    with pytest.raises(ValueError, match="Expected 3 input arrays"):
        codec.encode_device(_sources(x[:2], 64, "f32", "plain"))
    with pytest.raises(ValueError, match="feature dimension must be 5"):
        codec.encode_device(_sources([x[1], x[1], x[2]], 64, "f32", "plain"))
