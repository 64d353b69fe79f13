"""tests/glue_np.py -- the numpy references tests/test_gpu_glue_edges.py holds the glue kernels to -- pinned on the host against
numpy and sklearn themselves, on the inputs the GPU tests use (tests/glue_cases.py)."""
import warnings

import numpy as np
import pytest

import glue_cases as cases
import glue_np as G
from oracle import data_transform_np as D

nan, inf = np.nan, np.inf


same_bits = G.assert_same_bits


def test_ew_reference_covers_the_op_table():
    from fv3net_amd import ops

    assert set(G._EW) == set(ops.EW_OPS) and len(ops.EW_OPS) == 36
    assert G.EW_NEEDS_C <= G.EW_NEEDS_B and set(G.EW_TRANSCENDENTAL) <= set(G._EW)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ew_reference_known_answers(dtype):
    """What the kernel's comments state about NaN, +-0, +-inf and ``== scalar``, as tables written out by hand."""
    T = np.dtype(dtype).type
    x = np.array([nan, -inf, inf, -0.0, 0.0, -2, 0.25, 1, 2], dtype)
    ones = np.ones_like(x)

    def check(op, want, b=None, c=None, s=0.0, a=x):
        same_bits(G.ew(op, a, b, c, s), np.array(want, dtype))

    check("sign", [nan, -1, 1, 0, 0, -1, 1, 1, 1])                       # np.sign: NaN stays, +-0 -> +0
    check("abs", [nan, inf, inf, 0, 0, 2, 0.25, 1, 2])                   # np.abs: -0 -> +0
    check("clip01", [nan, 0, 1, -0.0, 0, 0, 0.25, 1, 1])                 # np.clip(a, 0, 1): NaN stays
    check("minimum_s", [nan, -inf, 1, -0.0, 0, -2, 0.25, 1, 1], s=1.0)   # np.minimum: NaN stays, == scalar gives the scalar
    check("min_s", [1, -inf, 1, -0.0, 0, -2, 0.25, 1, 1], s=1.0)         # a.where(a < s, other=s): a NaN becomes s
    check("where_gt_s", [1, 1, inf, 1, 1, 1, 1, 1, 2], s=1.0)            # a.where(a > s, s): a NaN becomes s
    check("gt_s", [0, 0, 1, 0, 0, 0, 0, 0, 1], s=1.0)
    check("lt_s", [0, 1, 0, 1, 1, 1, 1, 0, 0], s=1.0)
    check("le_s", [0, 1, 0, 1, 1, 1, 1, 1, 0], s=1.0)
    check("fillna_s", [7, -inf, inf, -0.0, 0, -2, 0.25, 1, 2], s=7.0)
    check("isclose_s", [0, 0, 0, 0, 0, 0, 0, 1, 0], s=1.0)
    check("isclose_s", [0, 0, 1, 0, 0, 0, 0, 0, 0], s=inf)               # only an equal infinity is close to an infinity
    check("isclose", [0, 0, 1, 0, 0, 0, 0, 0, 0], b=inf * ones)
    check("isclose", [0, 0, 0, 1, 1, 0, 0, 0, 0], b=0 * ones)
    check("isclose", [0, 0, 0, 0, 0, 0, 0, 0, 0], b=nan * ones)
    check("relu_threshold_s", [nan, 0, inf, 0, 0, 0, 0, 0, 2], s=1.0)    # strict, NaN stays (oracle/mlp_np.py:limit_value_backward)
    check("below_s", [nan, -inf, nan, -0.0, 0, -2, 0.25, 0, 0], s=1.0)   # 0 * x where x >= s: NaN for NaN and +inf
    check("where_nan", [nan, -inf, nan, -0.0, nan, -2, 0.25, 1, 2], b=np.array([1, 1, 0, 1, -0.0, nan, 2, -1, inf], dtype))  # a NaN mask is "true"
    check("and", [1, 1, 0, 0, 0, 1, 0, 1, 1], b=np.array([1, nan, 0, 1, 1, -1, -0.0, inf, 2], dtype))  # a NaN is "true" (!= 0)
    # incloud_to_gridcell at its two thresholds: <= 1e-3 keeps the in-cloud value, (1e-3, 5e-2] multiplies by 5e-2
    lim1, lim2 = T(1e-3), T(5e-2)
    frac = np.array([nan, 0, lim1, np.nextafter(lim1, T(1)), lim2, np.nextafter(lim2, T(1)), 1, -inf, inf], dtype)
    q = T(3) * ones
    # (a NaN fraction fails both comparisons of clouds.py:40-66 and is treated as the upper threshold)
    check("incloud_to_gridcell", [T(3) * lim2, 3, 3, T(3) * lim2, T(3) * lim2, T(3) * np.nextafter(lim2, T(1)), 3, 3, inf], b=q, a=frac)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("s", cases.SCALARS)
def test_ew_reference_against_the_numpy_calls(dtype, s):
    """On the operands the GPU test uses: each op whose semantics the kernel takes from a numpy call gives what that call
    gives, for the scalar cast to the array's dtype."""
    a, b, c = cases.ew_operands(dtype, s)
    st = np.dtype(dtype).type(s)
    with np.errstate(all="ignore"):
        same_bits(G.ew("isclose", a, b), np.isclose(a, b).astype(dtype))
        same_bits(G.ew("isclose_s", a, s=s), np.isclose(a, st).astype(dtype))
        same_bits(G.ew("sign", a), np.sign(a))
        same_bits(G.ew("abs", a), np.abs(a))
        same_bits(G.ew("clip01", a), np.clip(a, 0, 1))
        same_bits(G.ew("minimum_s", a, s=s), np.minimum(a, st))
        same_bits(G.ew("where_gt_s", a, s=s), np.where(a > st, a, st))
        same_bits(G.ew("min_s", a, s=s), np.where(a < st, a, st))
        same_bits(G.ew("incloud_to_gridcell", a, b), D.incloud_to_gridcell_condensate(a, b))
    for op in G._EW:  # every op evaluates on these operands, in the operands' dtype
        out = G.ew(op, a, b if op in G.EW_NEEDS_B else None, c if op in G.EW_NEEDS_C else None, s)
        assert out.dtype == dtype and out.shape == a.shape, op
    # the operands really hold what the kernel's branches turn on
    assert np.isnan(a).any() and np.isinf(a).any() and (a == st).any() and (np.signbit(a) & (a == 0)).any()
    tiny = np.finfo(dtype).smallest_subnormal
    assert (a == tiny).any() and (a == -tiny).any()
    close = np.isclose(a, b)
    assert close.any() and (~close).any()


def test_ew_reference_shared_operands():
    rng = np.random.default_rng(0)
    a, b, c = rng.normal(size=(2, 3, 5, 7)), rng.normal(size=(2, 5, 7)), rng.normal(size=(2, 3, 5, 7))
    np.testing.assert_array_equal(G.ew("select", a, b, c > 0), np.where(c > 0, a, b[:, None]))
    np.testing.assert_array_equal(G.ew("blend", a, c, b), a * c + (1 - a) * b[:, None])


@pytest.mark.parametrize("kind", cases.MEMBER_DTYPES)
@pytest.mark.parametrize("count", cases.MEMBER_COUNTS)
def test_member_references_against_nanmean_and_nanmedian(kind, count):
    for n in cases.SIZES:
        _check_members(cases.members(kind, count, n))


def test_member_references_past_the_grid_cap():
    _check_members(cases.members("float32", 3, cases.PAST_THE_CAP))


def _check_members(ms):
    stack, dt = G._members(ms)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)  # (all-NaN cells, inf - inf)
        want_mean, want_median = np.nanmean(stack, axis=0), np.nanmedian(stack, axis=0)
    assert want_mean.dtype == dt and want_median.dtype == dt
    same_bits(G.member_mean(ms), want_mean, ignore_zero_sign=True)
    same_bits(G.member_median(ms), want_median, ignore_zero_sign=True)
    if stack.shape[1] >= 15:  # the patterns are all there
        got = G.member_mean(ms)
        assert np.isnan(got[1]) and got[2] == 2.5 and got[6] == 1.75 and got[9] == 0 and np.signbit(got[9])
        if stack.shape[0] >= 2:
            assert np.isnan(got[10]) and np.isinf(got[13]) and np.isinf(got[14])


@pytest.mark.parametrize("kind", ["float32", "float64"])
@pytest.mark.parametrize("nz", [1, 2, 79])
def test_flux_references_against_the_oracle(kind, nz):
    """[z, y, x] input: the same values as oracle/data_transform_np.py (numpy adds along a leading axis level by level)."""
    tend, delp, toa, up, flux, down = cases.columns(kind, (nz, 5, 7), 0)
    with np.errstate(all="ignore"):
        for rectify in (True, False):
            got_flux, got_down = G.tendency_to_flux(tend, delp, toa, up, 0, rectify)
            want_flux, want_down = D.tendency_to_flux(tend, toa, up, delp, rectify)
            same_bits(got_flux, want_flux)
            same_bits(got_down, want_down)
            same_bits(G.implied_surface_downward_flux(tend, delp, toa, up, 0, rectify),
                      D.tendency_to_implied_surface_downward_flux(tend, toa, up, delp, rectify))
            zero = np.zeros_like(toa)
            same_bits(G.tendency_to_flux(tend, delp, None, up, 0, rectify)[1], D.tendency_to_flux(tend, zero, up, delp, rectify)[1])
        same_bits(G.flux_to_tendency(flux, down, up, delp, 0), D.flux_to_tendency(flux, down, up, delp))
    assert got_flux.dtype == np.dtype(kind) and np.isnan(got_down).any() and np.isinf(got_down).any()  # (the unrectified ones)


def test_flux_references_other_axes_and_promotion():
    tend, delp, toa, up, flux, down = cases.columns("mixed", (3, 4, 5, 7), 1)
    assert tend.dtype == np.float32 and delp.dtype == np.float64
    got_flux, got_down = G.tendency_to_flux(tend, delp, toa, up, 1)
    assert got_flux.dtype == np.float64 and got_flux.shape == tend.shape and got_down.shape == (3, 5, 7)
    for o in range(3):
        with np.errstate(all="ignore"):
            want_flux, want_down = D.tendency_to_flux(tend[o].astype(np.float64), toa[o].astype(np.float64), up[o].astype(np.float64), delp[o])
        same_bits(got_flux[o], want_flux)
        same_bits(got_down[o], want_down)
    # the round trip of finite data (vcm/tests/test_flux_form.py)
    tend, delp, toa, up, _, _ = cases.columns("float64", (3, 79, 5, 7), 1, finite=True)
    f, d = G.tendency_to_flux(tend, delp, toa, up, 1, rectify=False)
    np.testing.assert_allclose(G.flux_to_tendency(f, d, up, delp, 1), tend, rtol=1e-9)


@pytest.mark.parametrize("n_vars,n_feat", [(1, 1), (2, 7), (5, 79)])
def test_minmax_reference_against_sklearn(n_vars, n_feat):
    from sklearn.preprocessing import MinMaxScaler

    for plant in (None, ("first", nan), ("middle", inf), ("last", -inf)):
        variables, _, _ = cases.minmax_case(n_vars, n_feat, 257, np.float64, plant)
        train, _, _ = cases.minmax_case(n_vars, n_feat, 300, np.float64, None, seed=1)
        scaler = MinMaxScaler().fit(np.concatenate(train, axis=0).T)
        X = np.concatenate(variables, axis=0).T  # [sample, feature]
        bounds = np.cumsum([0] + [v.shape[0] for v in variables])
        scales = [scaler.scale_[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
        offsets = [scaler.min_[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
        with np.errstate(all="ignore"):
            scaled = X * scaler.scale_ + scaler.min_
            if plant is None or np.isnan(plant[1]):  # (MinMaxScaler.transform lets a NaN through and refuses an infinity)
                np.testing.assert_array_equal(scaled, scaler.transform(X))
            want = D.minmax_score(scaled)
        got = G.minmax_score(variables, scales, offsets)
        same_bits(got, want)
        assert (got == 0).any() and (n_feat == 1 or (got[np.isfinite(got)] > 0).any())
        assert plant is None or not np.isfinite(got[257 // 2])


def test_minmax_reference_float32_pack_differs_from_sklearn_by_two_float32_roundings():
    """The documented divergence: sklearn keeps an all-float32 pack in float32 (``X * scale_`` rounded, ``+ min_`` rounded
    again), the project evaluates it in float64.  Each float32 rounding moves a value by at most half its float32 spacing."""
    from sklearn.preprocessing import MinMaxScaler

    (ps,), _, _ = cases.minmax_case(1, 7, 1000, np.float32, None)
    scaler = MinMaxScaler().fit(ps.T)
    in_float32 = scaler.transform(ps.T).T
    assert in_float32.dtype == np.float32
    scale, offset = scaler.scale_.astype(np.float64), scaler.min_.astype(np.float64)
    product = ps.astype(np.float64) * scale[:, None]
    in_float64 = product + offset[:, None]
    diff = np.abs(in_float32.astype(np.float64) - in_float64)
    bound = 0.5 * np.spacing(np.abs(product).astype(np.float32)).astype(np.float64) + 0.5 * np.spacing(np.abs(in_float32)).astype(np.float64)
    assert (diff <= bound).all(), (diff - bound).max()
    assert diff.max() > 0  # (they do differ: about 1e-6 on surface-pressure-sized values)
    same_bits(G.minmax_score([ps], [scale], [offset]), D.minmax_score(in_float64.T))


def test_ocsvm_reference_against_sklearn_at_158_features():
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import StandardScaler
    from sklearn.svm import OneClassSVM

    rng = np.random.default_rng(8)
    nf = 158
    train, test = rng.normal(0, 1, (400, nf)) * rng.uniform(0.5, 20, nf), rng.normal(0, 1.3, (200, nf)) * rng.uniform(0.5, 20, nf)
    pipeline = make_pipeline(StandardScaler(), OneClassSVM(kernel="rbf", gamma=1.0 / (4 * nf), nu=0.1)).fit(train)
    scaler, svm = pipeline.steps[0][1], pipeline.steps[1][1]
    assert svm.support_vectors_.shape[0] > 20
    got = G.ocsvm_score(test.T, scaler.mean_, scaler.scale_, svm.support_vectors_, svm.dual_coef_[0], svm._gamma)
    np.testing.assert_allclose(got, -1 * pipeline.score_samples(test), rtol=1e-12)
    # a NaN feature gives a NaN score, an infinite one is infinitely far from every support vector (every term is 0)
    x, mean, scale, sv, coef, gamma = cases.ocsvm_case(7, 65, 5)
    score = G.ocsvm_score(x, mean, scale, sv, coef, gamma)
    assert np.isnan(score[1]) and score[65 - 2] == 0 and np.isfinite(np.delete(score, 1)).all()
    assert (G.ocsvm_score(x, mean, scale, sv[:0], coef[:0], gamma) == 0).all()
