"""TEST INFRASTRUCTURE ONLY: plain numpy references of the small "glue" kernels that every composite model runs after the
network -- the 36-op ``ew_kernel`` table of csrc/coarsen.hip and the six kernels of csrc/fit.hip -- each a few lines in the
precision of the operation.  tests/test_host_glue.py pins them against numpy and sklearn themselves; tests/test_gpu_glue_edges.py
compares the kernels with them, bit for bit where nothing else is said."""
import numpy as np

from oracle.mlp_np import limit_value_backward

GRAVITY = 9.80665            # vcm/calc/thermo/constants.py:2
CLIMIT1, CLIMIT2 = 1.0e-3, 5.0e-2  # vcm/calc/clouds.py:40-66


def assert_same_bits(got, want, ignore_zero_sign=False, err_msg=""):
    """Equal dtype, shape and values, NaNs in the same places and (unless told otherwise) zeros of the same sign."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (err_msg, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=err_msg)
    if not ignore_zero_sign:
        np.testing.assert_array_equal(np.signbit(got) & ~np.isnan(got), np.signbit(want) & ~np.isnan(want), err_msg=f"{err_msg} (sign of zero)")


# ------------------------------------------------------------------------------------------------
# ew: every op of fv3net_amd.ops.EW_OPS as the numpy / xarray expression the kernel's comment names
# ------------------------------------------------------------------------------------------------
_EW = {
    "mul": lambda a, b, c, s: a * b,
    "isclose": lambda a, b, c, s: np.isclose(a, b).astype(a.dtype),
    "isclose_s": lambda a, b, c, s: np.isclose(a, s).astype(a.dtype),
    "where_nan": lambda a, b, c, s: np.where(b != 0, a, a.dtype.type(np.nan)),        # a.where(mask b)
    "select": lambda a, b, c, s: np.where(c != 0, a, b),                              # xr.where(mask c, a, b)
    "select_s": lambda a, b, c, s: np.where(b != 0, s, a),                            # xr.where(mask b, s, a)
    "gt_s": lambda a, b, c, s: (a > s).astype(a.dtype),
    "lt_s": lambda a, b, c, s: (a < s).astype(a.dtype),
    "fillna_s": lambda a, b, c, s: np.where(np.isnan(a), s, a),                       # a.fillna(s)
    "and": lambda a, b, c, s: ((a != 0) & (b != 0)).astype(a.dtype),
    "min_s": lambda a, b, c, s: np.where(a < s, a, s),                                # a.where(a < s, other=s): a NaN becomes s
    "blend": lambda a, b, c, s: a * b + (a.dtype.type(1) - a) * c,
    "mul_s": lambda a, b, c, s: s * a,
    "where_s": lambda a, b, c, s: np.where(b != 0, a, s),                             # a.where(mask b, other=s)
    "add": lambda a, b, c, s: a + b,
    "add_s": lambda a, b, c, s: a + s,
    "sub": lambda a, b, c, s: a - b,
    "log_floor_s": lambda a, b, c, s: np.log(np.maximum(a, s)),                       # tf.math.log(tf.maximum(a, s))
    "exp": lambda a, b, c, s: np.exp(a),
    "relu_threshold_s": lambda a, b, c, s: limit_value_backward(a, lower=s),          # LimitValueTransform, lower limit
    "below_s": lambda a, b, c, s: limit_value_backward(a, upper=s),                   # LimitValueTransform, upper limit
    "div_s": lambda a, b, c, s: a / s,
    "incloud_to_gridcell": lambda a, b, c, s: np.where(                               # a = cloud fraction, b = in-cloud condensate
        a <= a.dtype.type(CLIMIT1), b, b * np.where(a > a.dtype.type(CLIMIT2), a, a.dtype.type(CLIMIT2))),
    "clip01": lambda a, b, c, s: np.clip(a, 0, 1),
    "pow_base_s": lambda a, b, c, s: s ** a,
    "minimum_s": lambda a, b, c, s: np.minimum(a, s),
    "div": lambda a, b, c, s: a / b,
    "where_pos_s": lambda a, b, c, s: np.where(b > 0, a, s),                          # xr.where(b > 0, a, s)
    "sign": lambda a, b, c, s: np.sign(a),
    "abs": lambda a, b, c, s: np.abs(a),
    "rsub_s": lambda a, b, c, s: s - a,
    "rdiv_s": lambda a, b, c, s: s / a,
    "where_gt_s": lambda a, b, c, s: np.where(a > s, a, s),                           # a.where(a > s, s): a NaN becomes s
    "le_s": lambda a, b, c, s: (a <= s).astype(a.dtype),
    "sin": lambda a, b, c, s: np.sin(a),
    "cos": lambda a, b, c, s: np.cos(a),
}
EW_NEEDS_B = {"mul", "isclose", "where_nan", "select", "select_s", "and", "blend", "where_s", "add", "sub", "incloud_to_gridcell",
              "div", "where_pos_s"}
EW_NEEDS_C = {"select", "blend"}
# the ops whose finite results depend on the math library: gated in ulps against ew_longdouble, everything else is exact
EW_TRANSCENDENTAL = ("exp", "log_floor_s", "sin", "cos", "pow_base_s")


def _shared(t, a):
    """An operand of ``a``'s shape, or a [.., y, x] field shared by the level axis of ``a`` [.., level, y, x]."""
    if t is None:
        return None
    t = np.asarray(t).astype(a.dtype)
    if t.shape != a.shape:
        assert a.ndim >= 3 and t.shape == a.shape[:-3] + a.shape[-2:], (t.shape, a.shape)
        t = np.broadcast_to(np.expand_dims(t, -3), a.shape)
    return t


def ew(op, a, b=None, c=None, s=0.0):
    """``fv3net_amd.ops.ew`` in ``a``'s dtype, the scalar cast to that dtype first."""
    a = np.asarray(a)
    with np.errstate(all="ignore"):
        out = _EW[op](a, _shared(b, a), _shared(c, a), a.dtype.type(s))
    assert out.dtype == a.dtype and out.shape == a.shape, (op, out.dtype, out.shape)
    return out


def ew_longdouble(op, a, s=0.0):
    """The transcendental ops evaluated in ``np.longdouble`` from the same (already rounded) inputs."""
    x, s = np.asarray(a).astype(np.longdouble), np.longdouble(np.asarray(a).dtype.type(s))
    with np.errstate(all="ignore"):
        if op == "log_floor_s":
            return np.log(np.maximum(x, s))
        if op == "pow_base_s":
            return s ** x
        return {"exp": np.exp, "sin": np.sin, "cos": np.cos}[op](x)


# ------------------------------------------------------------------------------------------------
# fit.hip
# ------------------------------------------------------------------------------------------------
def level_scale(x, scale, z_axis):
    """TaperConfig.apply: ``scale[z] * x`` along ``z_axis`` in float64."""
    x = np.asarray(x)
    shape = [1] * x.ndim
    shape[z_axis] = -1
    with np.errstate(all="ignore"):
        return np.asarray(scale, np.float64).reshape(shape) * x.astype(np.float64)


def _members(members):
    dt = np.float64 if any(np.asarray(m).dtype == np.float64 for m in members) else np.float32
    return np.stack([np.asarray(m).astype(dt) for m in members]), dt


def member_mean(members):
    """NaN-skipping mean over the members: the kept values added in member order starting from the first kept one, divided
    once by their count, in the members' (promoted) dtype; NaN where every member is NaN."""
    m, dt = _members(members)
    total, started, count = np.zeros(m.shape[1:], dt), np.zeros(m.shape[1:], bool), np.zeros(m.shape[1:], np.int64)
    with np.errstate(all="ignore"):
        for x in m:
            keep = ~np.isnan(x)
            total = np.where(keep, np.where(started, total + x, x), total)
            started |= keep
            count += keep
        return np.where(count > 0, total / count.astype(dt), dt(np.nan))


def member_median(members):
    """NaN-skipping median: the middle kept value, or half the sum of the two middle ones; equal values (+0 and -0) keep
    their member order."""
    m, dt = _members(members)
    count = (~np.isnan(m)).sum(axis=0)
    srt = np.sort(m, axis=0, kind="stable")  # (NaNs last)
    lo = np.take_along_axis(srt, np.maximum((count - 1) // 2, 0)[None], axis=0)[0]
    hi = np.take_along_axis(srt, np.minimum(count // 2, m.shape[0] - 1)[None], axis=0)[0]
    with np.errstate(all="ignore"):
        return np.where(count == 0, dt(np.nan), np.where(count % 2 == 1, hi, dt(0.5) * (lo + hi)))


def _column_dtype(*arrays):
    return np.float64 if any(a is not None and np.asarray(a).dtype == np.float64 for a in arrays) else np.float32


def _mass_cumsum(tendency, delp, z_axis, dt):
    t, dp = (np.moveaxis(np.asarray(x).astype(dt), z_axis, 0) for x in (tendency, delp))
    return np.cumsum(t * dp / dt(GRAVITY), axis=0)  # vcm.mass_cumsum (vertically_dependent.py:25-27)


def _rectified(down, rectify):
    return np.where(down >= 0, down, down.dtype.type(0)) if rectify else down  # x.where(x >= 0, 0): a NaN becomes 0


def tendency_to_flux(tendency, delp, toa_net_flux, surface_upward_flux, z_axis, rectify=True):
    """vcm/calc/flux_form.py:7-42 with ``np.cumsum`` (a running sum from the model top, NaNs propagate) in the arrays'
    promoted dtype: (net flux at the interface above each cell, surface downward flux).

    Not modelled, here or in the kernels or in oracle/data_transform_np.py: xarray's ``cumsum`` / ``sum`` skip NaNs by default
    for floats, so the reference may carry a column past a NaN tendency where this propagates it (unverified: xarray was not
    available to check)."""
    dt = _column_dtype(tendency, delp, toa_net_flux, surface_upward_flux)
    with np.errstate(all="ignore"):
        flux = -_mass_cumsum(tendency, delp, z_axis, dt)
        flux = np.concatenate([np.zeros_like(flux[:1]), flux], axis=0)  # flux.pad({dim: (1, 0)}, constant_values=0.0)
        flux = flux + (dt(0) if toa_net_flux is None else np.asarray(toa_net_flux).astype(dt))
        down = _rectified(flux[-1] + np.asarray(surface_upward_flux).astype(dt), rectify)
    return np.moveaxis(flux[:-1], 0, z_axis), down


def implied_surface_downward_flux(tendency, delp, toa_net_flux, surface_upward_flux, z_axis, rectify=True):
    """flux_form.py:45-73 (the closure form): toa + upward - the column integral, the integral taken level by level from
    the model top (the last entry of the cumulative sum)."""
    dt = _column_dtype(tendency, delp, toa_net_flux, surface_upward_flux)
    with np.errstate(all="ignore"):
        integral = _mass_cumsum(tendency, delp, z_axis, dt)[-1]
        toa = np.zeros_like(integral) if toa_net_flux is None else np.asarray(toa_net_flux).astype(dt)
        return _rectified(toa + np.asarray(surface_upward_flux).astype(dt) - integral, rectify)


def flux_to_tendency(net_flux, surface_downward_flux, surface_upward_flux, delp, z_axis):
    """flux_form.py:76-100: ``-(g * diff(concat(net_flux, down - up)) / delp)``."""
    dt = _column_dtype(net_flux, surface_downward_flux, surface_upward_flux, delp)
    f, dp = (np.moveaxis(np.asarray(x).astype(dt), z_axis, 0) for x in (net_flux, delp))
    with np.errstate(all="ignore"):
        surface_net = np.asarray(surface_downward_flux).astype(dt) - np.asarray(surface_upward_flux).astype(dt)
        tend = -(dt(GRAVITY) * np.diff(np.concatenate([f, surface_net[None]], axis=0), axis=0) / dp)
    return np.moveaxis(tend, 0, z_axis)


def minmax_score(variables, scales, offsets):
    """MinMaxNoveltyDetector's score of ``[feature, sample]`` arrays: ``X.astype(float64) * scale_ + min_`` (two rounded steps,
    as ``MinMaxScaler.transform`` computes them), numpy's NaN-propagating max / min over all features, then
    ``max(max - 1, 0) + max(-min, 0)``.

    Documented divergence: for an all-float32 pack sklearn 1.7 keeps float32 in ``MinMaxScaler.transform``, so its scaled
    values carry two float32 roundings (about 1e-6 absolute on surface-pressure-sized data); the project evaluates float32
    inputs in float64 on purpose.  tests/test_host_glue.py bounds the difference by those two roundings."""
    with np.errstate(all="ignore"):
        scaled = np.concatenate([np.asarray(v).astype(np.float64) * np.asarray(sc, np.float64)[:, None] + np.asarray(off, np.float64)[:, None]
                                 for v, sc, off in zip(variables, scales, offsets)], axis=0)
        return np.maximum(scaled.max(axis=0) - 1, 0) + np.maximum(-1 * scaled.min(axis=0), 0)


def ocsvm_score(x, mean, scale, support_vectors, dual_coef, gamma):
    """``-Pipeline(StandardScaler, OneClassSVM(rbf)).score_samples`` of ``x`` [feature, sample] in float64:
    ``-(coef * exp(-gamma * |z - sv|^2)).sum()`` with ``z = (x - mean) / scale``."""
    with np.errstate(all="ignore"):
        z = (np.asarray(x, np.float64).T - np.asarray(mean, np.float64)) / np.asarray(scale, np.float64)  # [sample, feature]
        total = np.zeros(z.shape[0])
        for sv, coef in zip(np.asarray(support_vectors, np.float64), np.asarray(dual_coef, np.float64)):
            total = total + coef * np.exp(-gamma * ((z - sv) ** 2).sum(axis=1))
        return -total
