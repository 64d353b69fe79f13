"""The small kernels every composite model runs after the network, each compared directly with a plain numpy reference
(tests/glue_np.py, pinned on the host by tests/test_host_glue.py) on the inputs of tests/glue_cases.py: the six kernels of
csrc/fit.hip, the 36-op ``ew_kernel`` table of csrc/coarsen.hip and ``limit_value`` of csrc/local.hip -- at non-finite inputs,
+-0, values on a threshold and next to it, sizes around one 256-thread block and past the 16384-block cap of the grid-stride
loops, every layout with its own index arithmetic.  Bit for bit unless a tolerance is stated."""
import numpy as np
import pytest
import torch

import glue_cases as cases
import glue_np as G
import local_cases
from oracle import mlp_np

pytestmark = pytest.mark.gpu

same_bits = G.assert_same_bits
F32, F64 = np.float32, np.float64


def _to(device, x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------
# LimitValueTransform.backward: one truth table (oracle/mlp_np.py:limit_value_backward) on both device paths
# ------------------------------------------------------------------------------------------------
LIMITS = [(-1.5, None), (None, 2.5), (-1.5, 2.5), (0.0, None), (0.1, 0.7), (1.0, 1.0)]


def _limit_inputs(dtype, lower, upper):
    T = np.dtype(dtype).type
    vals = [np.nan, np.inf, -np.inf, 0.0, -0.0, -3, -1, 0.5, 1, 2, 3, 1e30, -1e30]
    for lim in (lower, upper):
        if lim is not None:
            vals += [T(lim), np.nextafter(T(lim), T(np.inf)), np.nextafter(T(lim), T(-np.inf))]
    return np.array(vals, dtype)


@pytest.mark.parametrize("layout", ["contiguous", "transposed"])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_limit_value_transform_on_device_tensors(device, dtype, layout):
    """The ew path (relu_threshold_s, below_s): [sample, feature] tensors as the hook hands them over, contiguous and as the
    transposed view of a [feature, sample] buffer."""
    from fv3net_amd.emulation.transforms import LimitValueTransform

    for lower, upper in LIMITS:
        v = _limit_inputs(dtype, lower, upper)
        x = np.ascontiguousarray(np.stack([np.roll(v, k) for k in range(5)], axis=1))  # [sample, 5 features]
        t = _to(device, x) if layout == "contiguous" else _to(device, x.T).t()
        assert tuple(t.shape) == x.shape and t.is_contiguous() == (layout == "contiguous")
        got = LimitValueTransform(lower=lower, upper=upper).backward(t)
        assert tuple(got.shape) == x.shape
        same_bits(_np(got), mlp_np.limit_value_backward(x, lower, upper), err_msg=f"lower={lower}, upper={upper}")
        assert LimitValueTransform(lower=lower, upper=upper).forward(t) is t


def test_limit_value_in_local_unpack(device):
    """The ``local_unpack_kernel`` path: a dense-local model whose last layer is zero, so that the value is exactly
    ``center[z]`` -- on ``value_lo != 0``, one float above and one below it, the same at ``value_hi``, NaN and both
    infinities -- with and without conditional scaling (its two call sites), and a Difference whose ``before + value`` lands on
    ``after_lo`` and on ``after_hi``, next to them, and on NaN / infinite ``before`` values."""
    from fv3net_amd.local_mlp import LocalMlpModel

    f = np.float32
    lo, hi, alo, ahi = f(-1.5), f(2.5), f(1.0), f(3.0)
    up, dn = (lambda x: np.nextafter(f(x), f(np.inf))), (lambda x: np.nextafter(f(x), f(-np.inf)))
    center = np.array([lo, up(lo), dn(lo), hi, up(hi), dn(hi), 0.5, np.nan, np.inf, -np.inf], f)
    # before + 0.5 (each sum is exact): on after_lo, one float above and below it, the same at after_hi, then the rest
    row = np.array([alo - f(0.5), up(alo) - f(0.5), dn(alo) - f(0.5), ahi - f(0.5), up(ahi) - f(0.5), dn(ahi) - f(0.5),
                    np.nan, np.inf, -np.inf, 0.0, -0.5, 4.5], f)
    assert row[1] + f(0.5) == up(alo) and row[2] + f(0.5) == dn(alo) and row[4] + f(0.5) == up(ahi) and row[5] + f(0.5) == dn(ahi)
    nz, ncol = center.size, row.size
    rng = np.random.default_rng(3)
    st = local_cases.state(rng, nz, ncol, np.float32)
    spec = local_cases.regressor(rng, st, nz, width=32, depth=1, make=local_cases.product_makers())
    spec.out_kernel = np.zeros_like(spec.out_kernel)
    spec.out_bias = np.zeros_like(spec.out_bias)
    for o, before in zip(spec.outputs, ("before_a", "before_b")):
        o.scale, o.center, o.before = np.ones(nz, f), center.copy(), before
        o.value_limit, o.after_limit = (float(lo), float(hi)), (float(alo), float(ahi))
        st[before] = np.ascontiguousarray(np.broadcast_to(row, (nz, ncol)))
    cond = spec.outputs[0].conditional  # (scale 1, center 0: the un-scaled value is the value)
    cond.scale, cond.center, cond.min_scale = np.ones_like(cond.scale), np.zeros_like(cond.center), 0.0
    spec.outputs[1].conditional = None
    got = LocalMlpModel(spec, device=device).predict({k: _to(device, v) for k, v in st.items()})
    want = mlp_np.forward_local(spec, {k: v.T for k, v in st.items()}, dtype=np.float32)
    assert list(got) == spec.output_names and len(got) == 5
    for name in spec.output_names:
        same_bits(_np(got[name]), np.ascontiguousarray(want[name].T), err_msg=name)
    limited = _np(got[spec.outputs[1].name])[:, 0]
    same_bits(limited, np.array([0, up(lo), 0, 0, 0, dn(hi), 0.5, np.nan, np.nan, 0], f))  # the table, spelled out once
    after = _np(got[spec.outputs[1].after])[6]  # value 0.5
    same_bits(after, np.array([0, up(alo), 0, 0, 0, dn(ahi), np.nan, np.nan, 0, 0, 0, 0], f))


# ------------------------------------------------------------------------------------------------
# ew
# ------------------------------------------------------------------------------------------------
# Worst error, in ulps of the dtype against an np.longdouble evaluation, of the finite results of the five ops that go
# through the device math library.  No document at hand states the library's bounds, so each gate is the worst case
# measured on an MI355X over this test's inputs (the first figure) plus one ulp.
ULP_GATE = {
    ("exp", "float32"): 0.6856 + 1, ("exp", "float64"): 0.7217 + 1,
    ("log_floor_s", "float32"): 1.7853 + 1, ("log_floor_s", "float64"): 0.5796 + 1,
    ("sin", "float32"): 0.8925 + 1, ("sin", "float64"): 0.7012 + 1,
    ("cos", "float32"): 1.0162 + 1, ("cos", "float64"): 0.6367 + 1,
    ("pow_base_s", "float32"): 0.4948 + 1, ("pow_base_s", "float64"): 1.0244 + 1,  # (float32: pow in float64, rounded once)
}


def ulp_errors(op, got, a, s):
    """(exact, ulps): where the result must equal numpy's bit for bit -- a non-finite result (exp(inf), log at a floor <= 0,
    sin(inf), s ** nan), a result that no rounding enters (exp(-inf) = 0, s ** +-inf = 0, 1 or inf, f(+-0) of exp / sin /
    cos / pow, 0 ** x, 1 ** x) -- and the error of every other result against the long double evaluation, in units of
    the spacing of the dtype at the true value.  Every cell outside ``exact`` has a finite reference, a non-finite input
    included where the library computes its result (log(max(-inf, s)) = log(s)); a NaN or infinite result there gives a
    NaN or infinite error, which the caller's gate refuses."""
    T = a.dtype.type
    ref = G.ew_longdouble(op, a, s)
    with np.errstate(all="ignore"):
        rounded = ref.astype(a.dtype)
        exact = ~np.isfinite(rounded)
        if op != "log_floor_s":
            exact |= (a == 0) | np.isinf(a)
        if op == "pow_base_s" and T(s) in (T(0), T(1)):
            exact[:] = True  # 0 ** x is 0, 1 or inf; 1 ** x is 1
        ulps = np.abs(got.astype(np.longdouble) - ref) / np.spacing(np.abs(rounded)).astype(np.longdouble)
    return exact, np.where(exact, 0, ulps).astype(np.float64)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("op", sorted(G._EW))
def test_ew_values(device, op, dtype):
    """Every op on specials crossed with specials (tests/glue_cases.py:ew_operands) and a few hundred random values, for
    several scalars.  Exact, except the finite results of exp, log_floor_s, sin, cos and pow_base_s, which are gated in ulps.
    Measured worst cases on an MI355X, in ulps (float32 / float64): exp 0.6856 / 0.7217, log_floor_s 1.7853 / 0.5796,
    sin 0.8925 / 0.7012, cos 1.0162 / 0.6367, pow_base_s 0.4948 / 1.0244; each gate in ULP_GATE is that figure plus one."""
    from fv3net_amd import ops

    gate = ULP_GATE.get((op, np.dtype(dtype).name))
    for s in cases.SCALARS:
        a, b, c = cases.ew_operands(dtype, s)
        b, c = (b if op in G.EW_NEEDS_B else None), (c if op in G.EW_NEEDS_C else None)
        got = _np(ops.ew(op, _to(device, a), _to(device, b), _to(device, c), scalar=s))
        want = G.ew(op, a, b, c, s)
        if op not in G.EW_TRANSCENDENTAL:
            same_bits(got, want, err_msg=f"{op}, scalar {s}")
            continue
        exact, ulps = ulp_errors(op, got, a, s)
        same_bits(got[exact], want[exact], err_msg=f"{op}, scalar {s}: special values")
        assert exact.any() and (~exact).any() or op == "pow_base_s"
        assert np.isfinite(got[~exact]).all(), f"{op}, scalar {s}: a non-finite result where the reference is finite"
        assert np.all(ulps <= gate), (op, s, float(np.nanmax(ulps)), gate)  # (NaN <= gate is False: a NaN error fails)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_ew_shared_operands(device, dtype):
    """b and c of a's shape or [.., y, x] fields shared over a's level axis (b_rep, c_rep), in every combination; a 1-D a."""
    from fv3net_amd import ops

    rng = np.random.default_rng(5)
    exact_ops = [op for op in sorted(G._EW) if op not in G.EW_TRANSCENDENTAL]
    for sa, sb, sc in cases.EW_SHAPES:
        a, b, c = cases.field(rng, sa, dtype), cases.field(rng, sb, dtype, 0.3), cases.field(rng, sc, dtype, 0.3)
        da, db, dc = _to(device, a), _to(device, b), _to(device, c)
        for op in exact_ops:
            bb, cc = (op in G.EW_NEEDS_B), (op in G.EW_NEEDS_C)
            got = ops.ew(op, da, db if bb else None, dc if cc else None, scalar=0.5)
            same_bits(_np(got), G.ew(op, a, b if bb else None, c if cc else None, 0.5), err_msg=f"{op} {sa} {sb} {sc}")
    # (operands the table does not read may be absent; one it reads may not)
    from fv3net_amd._lib import Fv3HipError

    with pytest.raises(Fv3HipError, match="operand c"):
        ops.ew("select", da, db)
    with pytest.raises(ValueError, match="does not match"):
        ops.ew("mul", _to(device, np.zeros((2, 3, 5, 7), dtype)), _to(device, np.zeros((3, 5, 7), dtype)))


@pytest.mark.parametrize("n", cases.SIZES)
def test_ew_sizes_around_one_block(device, n):
    from fv3net_amd import ops

    rng = np.random.default_rng(n)
    for dtype in (F32, F64):
        a, b = cases.field(rng, (n,), dtype), cases.field(rng, (n,), dtype)
        same_bits(_np(ops.ew("mul", _to(device, a), _to(device, b))), G.ew("mul", a, b))
        same_bits(_np(ops.ew("relu_threshold_s", _to(device, a), scalar=-0.25)), G.ew("relu_threshold_s", a, s=-0.25))


def test_ew_past_the_grid_stride_cap(device):
    """More elements than the 16384 blocks hold: the second trip of the grid-stride loop, with a shared operand."""
    from fv3net_amd import ops

    rng = np.random.default_rng(1)
    a = cases.field(rng, cases.PAST_THE_CAP_SHAPE, F32, 0.01)
    b = cases.field(rng, cases.PAST_THE_CAP_SHAPE[1:], F32, 0.01)
    assert a.size == cases.PAST_THE_CAP
    da = _to(device, a)
    same_bits(_np(ops.ew("mul", da, _to(device, b))), G.ew("mul", a, b))
    same_bits(_np(ops.ew("below_s", da.reshape(-1), scalar=0.5)), G.ew("below_s", a.reshape(-1), s=0.5))


# ------------------------------------------------------------------------------------------------
# level_scale
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_level_scale_layouts_and_special_values(device, dtype):
    """[outer, z, y, x], z first, z last, one level; float32 input promoted to float64; a scale holding 0, NaN and inf
    against inf / NaN data (0 * inf and inf * 0 are NaN)."""
    from fv3net_amd import ops

    rng = np.random.default_rng(2)
    for shape, z_axis in [((2, 5, 3, 7), 1), ((5, 2, 3, 7), 0), ((2, 3, 7, 5), 3), ((2, 3, 7, 5), -1), ((4, 1, 6), 1), ((1,), 0)]:
        x = cases.field(rng, shape, dtype, 0.3)
        nz = shape[z_axis]
        scale = np.array([0.0, np.nan, np.inf, -2.5, 0.1][:nz] if nz > 1 else [0.1])
        if x.ndim > 1:  # an infinity and a NaN under every scale factor
            by_level = np.moveaxis(x, z_axis, 0)  # (a view)
            by_level[(slice(None),) + (0,) * (x.ndim - 1)] = np.inf
            by_level[(slice(None),) + (-1,) * (x.ndim - 1)] = np.nan
        got = ops.level_scale(_to(device, x), _to(device, scale), z_axis)
        assert got.dtype == torch.float64
        same_bits(_np(got), G.level_scale(x, scale, z_axis), err_msg=f"{shape} z_axis={z_axis}")
    with pytest.raises(ValueError, match="scale must have shape"):
        ops.level_scale(_to(device, np.zeros((2, 5), dtype)), _to(device, np.zeros(2)), 1)


@pytest.mark.parametrize("n", cases.SIZES + (cases.PAST_THE_CAP,))
def test_level_scale_sizes(device, n):
    from fv3net_amd import ops

    rng = np.random.default_rng(n)
    shape, z_axis = (cases.PAST_THE_CAP_SHAPE, 1) if n == cases.PAST_THE_CAP else ((n,), 0)
    x = cases.field(rng, shape, F32, 0.01)
    scale = rng.normal(0, 1, shape[z_axis])
    same_bits(_np(ops.level_scale(_to(device, x), _to(device, scale), z_axis)), G.level_scale(x, scale, z_axis))
    if n != cases.PAST_THE_CAP:  # one level, n points in it
        same_bits(_np(ops.level_scale(_to(device, x[None]), _to(device, scale[:1]), 0)), G.level_scale(x[None], scale[:1], 0))


# ------------------------------------------------------------------------------------------------
# member_reduce
# ------------------------------------------------------------------------------------------------
def _check_member_reduce(device, ms):
    from fv3net_amd import ops

    dms = [_to(device, m) for m in ms]
    same_bits(_np(ops.member_reduce(dms, "mean")), G.member_mean(ms), err_msg="mean")
    same_bits(_np(ops.member_reduce(dms, "median")), G.member_median(ms), err_msg="median")


@pytest.mark.parametrize("kind", cases.MEMBER_DTYPES)
@pytest.mark.parametrize("count", cases.MEMBER_COUNTS)
def test_member_reduce_patterns(device, kind, count):
    """1 .. 32 members (32 fills the array the insertion sort works in): no NaN, all NaN, all but one, alternating; inf and
    -inf in one cell with odd and even kept counts; ties, +-0, ascending, descending, all equal; two values whose sum
    overflows.  float32, float64, and mixed members (promoted to float64)."""
    for n in cases.SIZES:
        _check_member_reduce(device, cases.members(kind, count, n))


def test_member_reduce_past_the_grid_stride_cap(device):
    _check_member_reduce(device, cases.members("float32", 3, cases.PAST_THE_CAP))


def test_member_reduce_refuses_33_members(device):
    from fv3net_amd import ops
    from fv3net_amd._lib import Fv3HipError

    ms = [_to(device, m) for m in cases.members("float32", 33, 7)]
    with pytest.raises(Fv3HipError, match="between 1 and 32 members"):
        ops.member_reduce(ms, "median")
    with pytest.raises(ValueError, match="differ in shape"):
        ops.member_reduce([ms[0], ms[1][:3]], "mean")


# ------------------------------------------------------------------------------------------------
# tendency_to_flux, flux_to_tendency
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["float32", "float64", "mixed"])
@pytest.mark.parametrize("nz", [1, 2, 79])
def test_flux_kernels_layouts_options_and_non_finite_columns(device, nz, kind):
    """[tile, z, y, x] (outer and inner extents both > 1: the only layout where ``(o * nz + k) * inner + i`` can be wrong),
    [z, columns] and [columns, z] with 1, 255, 256, 257 and 1000 columns; toa given or not, rectified or not, the closure
    form; NaN / inf at the top, a middle and the bottom level, delp = 0 under flux_to_tendency."""
    from fv3net_amd import ops

    for shape, z_axis in cases.column_layouts(nz):
        tend, delp, toa, up, flux, down = cases.columns(kind, shape, z_axis)
        d_tend, d_delp, d_toa, d_up, d_flux, d_down = (_to(device, x) for x in (tend, delp, toa, up, flux, down))
        where = f"{shape} z_axis={z_axis}"
        for with_toa in (True, False):
            for rectify in (True, False):
                got_flux, got_down = ops.tendency_to_flux(d_tend, d_delp, d_toa if with_toa else None, d_up, z_axis, rectify=rectify)
                want_flux, want_down = G.tendency_to_flux(tend, delp, toa if with_toa else None, up, z_axis, rectify)
                same_bits(_np(got_flux), want_flux, err_msg=f"flux {where} toa={with_toa} rectify={rectify}")
                same_bits(_np(got_down), want_down, err_msg=f"down {where} toa={with_toa} rectify={rectify}")
                none, closed = ops.tendency_to_flux(d_tend, d_delp, d_toa if with_toa else None, d_up, z_axis, rectify=rectify, closure_only=True)
                assert none is None
                same_bits(_np(closed), G.implied_surface_downward_flux(tend, delp, toa if with_toa else None, up, z_axis, rectify),
                          err_msg=f"closure {where} toa={with_toa} rectify={rectify}")
        same_bits(_np(ops.flux_to_tendency(d_flux, d_down, d_up, d_delp, z_axis)), G.flux_to_tendency(flux, down, up, delp, z_axis),
                  err_msg=f"flux_to_tendency {where}")


def test_flux_round_trip(device):
    """vcm/tests/test_flux_form.py: finite tendencies come back from their fluxes."""
    from fv3net_amd import ops

    for shape, z_axis in [((3, 79, 5, 7), 1), ((79, 257), 0), ((257, 79), 1)]:
        tend, delp, toa, up, _, _ = cases.columns("float64", shape, z_axis, finite=True)
        d_delp, d_up = _to(device, delp), _to(device, up)
        flux, down = ops.tendency_to_flux(_to(device, tend), d_delp, _to(device, toa), d_up, z_axis, rectify=False)
        np.testing.assert_allclose(_np(ops.flux_to_tendency(flux, down, d_up, d_delp, z_axis)), tend, rtol=1e-9)


# ------------------------------------------------------------------------------------------------
# minmax_score
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n_vars,n_feat", [(1, 1), (2, 7), (5, 79), (1, 79), (5, 1)])
def test_minmax_score_bit_equal_to_numpy(device, n_vars, n_feat, dtype):
    """The library is built without contraction, so ``x * scale + offset`` is two rounded steps as in sklearn and the score
    equals numpy's bit for bit.  A NaN (then +inf, -inf) planted in the first, a middle and the last variable's launch;
    1 .. 1000 samples (several blocks); float32 variables are evaluated in float64."""
    from fv3net_amd import ops

    for n in (1, 257, 1000):
        for plant in (None, ("first", np.nan), ("middle", np.nan), ("last", np.nan), ("first", np.inf), ("middle", -np.inf), ("last", np.inf)):
            variables, scales, offsets = cases.minmax_case(n_vars, n_feat, n, dtype, plant)
            got = ops.minmax_score([_to(device, v) for v in variables], [_to(device, s) for s in scales], [_to(device, o) for o in offsets])
            assert got.dtype == torch.float64
            want = G.minmax_score(variables, scales, offsets)
            same_bits(_np(got), want, err_msg=f"n={n} plant={plant}")
            assert plant is None or not np.isfinite(want[n // 2])


@pytest.mark.parametrize("dtype", [F32, F64])
def test_minmax_score_strided_views(device, dtype):
    """A level clip with ``step=2`` (every other feature row of a larger buffer) and a [sample, feature] buffer passed
    transposed: the kernel reads through the strides."""
    from fv3net_amd import ops

    n = 300
    (wide, full, other), (s_wide, s_full, s_other), (o_wide, o_full, o_other) = cases.minmax_case(3, 14, n, dtype, ("middle", np.nan))
    clipped, s_clip, o_clip = wide[1:13:2], s_wide[1:13:2], o_wide[1:13:2]
    d_clip = _to(device, wide)[1:13:2]
    d_t = _to(device, np.ascontiguousarray(full.T)).t()  # [feature, sample] view of a [sample, feature] buffer
    assert d_clip.stride() == (2 * n, 1) and d_t.stride() == (1, 14)
    got = ops.minmax_score([d_clip, d_t, _to(device, other)], [_to(device, x) for x in (s_clip, s_full, s_other)],
                           [_to(device, x) for x in (o_clip, o_full, o_other)])
    want = G.minmax_score([clipped, full, other], [s_clip, s_full, s_other], [o_clip, o_full, o_other])
    same_bits(_np(got), want)
    assert np.isnan(want).sum() == 2 and np.isfinite(want).sum() == n - 2


def test_minmax_score_refuses_an_empty_variable_list(device):
    from fv3net_amd import ops

    with pytest.raises(ValueError, match="at least one variable"):
        ops.minmax_score([], [], [])
    v = _to(device, np.zeros((3, 4)))
    with pytest.raises(ValueError, match="one scale and one offset"):
        ops.minmax_score([v, v], [_to(device, np.ones(3))], [_to(device, np.zeros(3))])


# ------------------------------------------------------------------------------------------------
# ocsvm_score
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_feat", [1, 128, 129, 158, 320])
def test_ocsvm_score_feature_counts_up_to_the_lds_ceiling(device, n_feat):
    """128 features fill the default 64 KiB of dynamic LDS, 129 is the first count that needs the raised limit, 158 is a
    detector on two 79-level variables, 320 features fill the 160 KiB of a workgroup.  1 .. 200 samples (a partial, a full
    and several workgroups), 0 / 1 / 300 support vectors; a NaN feature and an infinite one in single samples.  Finite
    scores at the kernel's existing gate, rtol=1e-12; non-finite ones exact."""
    from fv3net_amd import ops

    for n in (1, 63, 64, 65, 200):
        for n_sv in (0, 1, 300):
            x, mean, scale, sv, coef, gamma = cases.ocsvm_case(n_feat, n, n_sv)
            got = _np(ops.ocsvm_score(*(_to(device, t) for t in (x, mean, scale, sv, coef)), gamma))
            want = G.ocsvm_score(x, mean, scale, sv, coef, gamma)
            where = f"n_feat={n_feat} n={n} n_sv={n_sv}"
            finite = np.isfinite(want)
            np.testing.assert_array_equal(np.isfinite(got), finite, err_msg=where)
            same_bits(got[~finite], want[~finite], err_msg=where)
            np.testing.assert_allclose(got[finite], want[finite], rtol=1e-12, atol=0, err_msg=where)
            if n >= 3 and n_sv:  # the NaN sample, the infinitely distant one, and nobody else
                assert np.isnan(want[1]) and finite.sum() == n - 1 and want[n - 2] == 0 and (np.delete(want, [1, n - 2]) < 0).all()


def test_ocsvm_score_refuses_more_features_than_lds_holds(device):
    from fv3net_amd import ops
    from fv3net_amd._lib import Fv3HipError

    x, mean, scale, sv, coef, gamma = cases.ocsvm_case(321, 5, 2)
    with pytest.raises(Fv3HipError, match="LDS"):
        ops.ocsvm_score(*(_to(device, t) for t in (x, mean, scale, sv, coef)), gamma)
