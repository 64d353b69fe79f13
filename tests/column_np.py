"""TEST INFRASTRUCTURE ONLY: plain numpy references of the nine small column kernels of csrc/vertical.hip that both restart
pipelines run around the remap -- interface and midpoint pressures, the four weight masks, the column sum, the blending weights
and the hydrostatic balance -- each a few lines in the order of operations the kernel's comment names.
tests/test_host_columns.py pins them against oracle/coarsen_np.py and oracle/coarsen_restarts_np.py; tests/test_gpu_column_edges.py
compares the kernels with them, bit for bit except for the two kernels that call ``log``."""
import numpy as np

from oracle.coarsen_np import block_upsample

GRAVITY, RDGAS, RVGAS = 9.80665, 287.05, 461.5   # vcm/calc/thermo/constants.py:2-4
VIRTUAL_COEFFICIENT = RVGAS / RDGAS - 1          # a Python float: numpy rounds it ONCE to the array's dtype (vertically_dependent.py:233)
LOG_ULPS = 3        # the ulp bound of log in the OpenCL full profile, which the device math library is written to
MIDPOINT_ROUNDINGS = 2   # pressure_at_midpoint_log_kernel besides its logs: the difference and the quotient
DZ_ROUNDINGS = 4         # hydrostatic_kernel besides its logs: the difference, two products and the quotient
SKIP_BOUND = 0.5    # a level whose bound exceeds this is ill conditioned (a layer thinner than the spacing of its logs)


def _z_first(x, z_axis):
    return np.moveaxis(np.asarray(x), z_axis, 0)


def _z_back(x, z_axis):
    return np.ascontiguousarray(np.moveaxis(x, 0, z_axis))


def _interfaces(delp, toa_pressure):
    """[nz + 1, ...] from delp [nz, ...]: p = toa; p = p + delp[k], in delp's dtype."""
    T = delp.dtype.type
    out = np.empty((delp.shape[0] + 1,) + delp.shape[1:], delp.dtype)
    p = np.full(delp.shape[1:], T(toa_pressure), delp.dtype)
    out[0] = p
    with np.errstate(all="ignore"):
        for k in range(delp.shape[0]):
            p = p + delp[k]
            out[k + 1] = p
    return out


def pressure_at_interface(delp, toa_pressure, z_axis):
    """``p[0] = toa; p[k + 1] = p[k] + delp[k]`` down each column in delp's dtype."""
    return _z_back(_interfaces(_z_first(delp, z_axis), toa_pressure), z_axis)


def column_sum(x, z_axis, addend=0.0):
    """``acc = 0; acc = acc + x[k]`` from the first level to the last, then ``acc + addend``, in x's dtype."""
    x = _z_first(x, z_axis)
    acc = np.zeros(x.shape[1:], x.dtype)
    with np.errstate(all="ignore"):
        for k in range(x.shape[0]):
            acc = acc + x[k]
        return np.ascontiguousarray(acc + x.dtype.type(addend))


def mask_weights(weights, p_cmp, p_fine, cmp_offset, w_repeat=1):
    """``weights where p_cmp[k + cmp_offset] < p_fine[surface] else +0`` (regridz.py:200-220) on the arrays of the C entry
    point: ``p_cmp`` [n_batch, cmp_levels, ...], ``p_fine`` [n_batch, nz + 1, ...], ``weights`` [n_batch / w_repeat, ...]
    (weight slice ``b // w_repeat`` serves batch ``b``).  Result [n_batch, nz, ...] in the weights' dtype."""
    weights, p_cmp, p_fine = np.asarray(weights), np.asarray(p_cmp), np.asarray(p_fine)
    nz = p_fine.shape[1] - 1
    level, ps = p_cmp[:, cmp_offset:cmp_offset + nz], p_fine[:, nz:nz + 1]
    w = np.repeat(weights, w_repeat, axis=0)[:, None]
    return np.ascontiguousarray(np.where(level < ps, w, weights.dtype.type(0)))


def upsample_onto(p_coarse, ny, nx, factor):
    """``oracle.coarsen_np.block_upsample`` onto a fine grid of known extents.  block_upsample takes an odd COARSE extent for
    a staggered dim; the entry point is told the FINE extents and takes an odd one of those for staggered (include/fv3hip.h).
    The two agree except where an unstaggered fine extent has an odd number of blocks (12 columns by 4), which the reference's
    rule cannot express: there every coarse point is repeated.  (``ops.mask_weights`` upsamples with block_upsample's rule where
    it falls back to the fine route, and refuses such a shape with a ValueError.)"""
    p_coarse = np.asarray(p_coarse)
    up = block_upsample(p_coarse, factor)
    if up.shape[-2:] == (ny, nx):
        return up
    for axis, n in ((-1, nx), (-2, ny)):
        p_coarse = np.take(p_coarse, np.arange(n) // factor, axis=axis)  # (a staggered dim: (n - 1) // factor is its last point)
    assert p_coarse.shape[-2:] == (ny, nx), (p_coarse.shape, ny, nx)
    return p_coarse


def mask_weights_coarse(weights, p_cmp_coarse, p_fine, cmp_offset, factor, w_repeat=1):
    """The same with ``p_cmp_coarse`` [n_batch, cmp_levels, ny / factor, nx / factor] upsampled first (regridz.py:119-121)."""
    ny, nx = np.asarray(p_fine).shape[-2:]
    return mask_weights(weights, upsample_onto(p_cmp_coarse, ny, nx, factor), p_fine, cmp_offset, w_repeat)


def blend_weights(blending_pressure, ps_coarse, pfull_coarse, z_axis):
    """``(ps - p) / (ps - pb)`` where ``p > pb``, else 1 (coarsen_restarts.py:559-576), in the dtype of ``pfull_coarse``."""
    p = np.asarray(pfull_coarse)
    ps, pb = (np.expand_dims(np.asarray(a).astype(p.dtype), z_axis % p.ndim) for a in (ps_coarse, blending_pressure))
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(np.where(p > pb, (ps - p) / (ps - pb), p.dtype.type(1)))


def _log_difference(delp, toa_pressure, roundings):
    """(d, bound) [nz, ...] in float64: the differences of the float64 logs of the interfaces accumulated in delp's dtype,
    and the relative error bound of a result that divides by, or multiplies, the dtype's own ``log`` difference:
    ``eps * (LOG_ULPS * (|lp[k]| + |lp[k + 1]|) / |d| + roundings)``."""
    eps = float(np.finfo(delp.dtype).eps)
    with np.errstate(all="ignore"):
        lp = np.log(_interfaces(delp, toa_pressure).astype(np.float64))
        d = lp[1:] - lp[:-1]
        return d, eps * (LOG_ULPS * (np.abs(lp[:-1]) + np.abs(lp[1:])) / np.abs(d) + roundings)


def pressure_at_midpoint_log_f64(delp, toa_pressure, z_axis):
    """(``delp / diff(log(p_interface))`` in float64 from the interfaces accumulated in delp's dtype, its bound)."""
    delp = _z_first(delp, z_axis)
    d, bound = _log_difference(delp, toa_pressure, MIDPOINT_ROUNDINGS)
    with np.errstate(all="ignore"):
        return _z_back(delp.astype(np.float64) / d, z_axis), _z_back(bound, z_axis)


def virtual_temperature(t, q):
    """``T * (1 + (Rv / Rd - 1) * q)`` in the arrays' dtype, the constant rounded once from float64."""
    t, q = np.asarray(t), np.asarray(q)
    T = t.dtype.type
    with np.errstate(all="ignore"):
        return t * (T(1) + T(VIRTUAL_COEFFICIENT) * q)


def hydrostatic_dz_f64(t, q, delp, toa_pressure, z_axis):
    """(``-diff(log(p_interface)) * Rd * Tv / g`` in float64, its bound): the interfaces and Tv in the arrays' dtype, Rd and g
    as that dtype holds them, everything after the logs in float64."""
    delp = _z_first(delp, z_axis)
    T = delp.dtype.type
    d, bound = _log_difference(delp, toa_pressure, DZ_ROUNDINGS)
    tv = _z_first(virtual_temperature(t, q), z_axis).astype(np.float64)
    with np.errstate(all="ignore"):
        return _z_back(-d * float(T(RDGAS)) * tv / float(T(GRAVITY)), z_axis), _z_back(bound, z_axis)


def hydrostatic_phis(dz_in, phis, dz_out, T, z_axis):
    """The kernel's two sequential sums in ``T``: ``top = phis / g`` then ``top + (-dz_in[k])`` from the bottom level up,
    ``sum`` of ``dz_out`` from the top level down, ``g * (top + sum)``."""
    dz_in, dz_out = (_z_first(np.asarray(a).astype(T), z_axis) for a in (dz_in, dz_out))
    T = np.dtype(T).type
    with np.errstate(all="ignore"):
        top = np.asarray(phis).astype(T) / T(GRAVITY)
        for k in range(dz_in.shape[0] - 1, -1, -1):
            top = top + (-dz_in[k])
        total = np.zeros(top.shape, T)
        for k in range(dz_out.shape[0]):
            total = total + dz_out[k]
        return np.ascontiguousarray(T(GRAVITY) * (top + total))


def error_over_bound(got, want, bound):
    """(worst |got - want| / (|want| * bound) over the cells with a finite, non-zero reference and a bound <= SKIP_BOUND,
    number of cells skipped for their bound, number of cells with a finite reference); asserts that ``got`` has the
    reference's NaNs and infinities."""
    got, want, bound = np.asarray(got).astype(np.float64), np.asarray(want), np.asarray(bound)
    finite = np.isfinite(want)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg="NaN pattern")
    np.testing.assert_array_equal(got[~finite & ~np.isnan(want)], want[~finite & ~np.isnan(want)], err_msg="infinities")
    use = finite & (want != 0) & (bound <= SKIP_BOUND)
    n_skipped, n_finite = int(np.count_nonzero(finite & ~use)), int(np.count_nonzero(finite))
    if not use.any():
        return 0.0, n_skipped, n_finite
    return float(np.max(np.abs(got[use] - want[use]) / (np.abs(want[use]) * bound[use]))), n_skipped, n_finite


class Tally:
    """Worst error / bound and the skipped share per key (a dtype, the thin-layer case apart) over the inputs of a test."""

    def __init__(self):
        self.worst, self.skipped, self.cells = {}, {}, {}

    def add(self, key, got, want, bound):
        ratio, n_skipped, n_finite = error_over_bound(got, want, bound)
        self.worst[key] = max(self.worst.get(key, 0.0), ratio)
        self.skipped[key] = self.skipped.get(key, 0) + n_skipped
        self.cells[key] = self.cells.get(key, 0) + n_finite
        return ratio

    def check(self, what):
        """A ratio above 1 is a failure; no level is skipped outside the thin-layer case, under 1 % of them in it."""
        print(what, "worst error / bound:", ", ".join(f"{k}: {v:.4f}" for k, v in sorted(self.worst.items())),
              "| skipped share:", ", ".join(f"{k}: {self.skipped[k] / max(self.cells[k], 1):.5f}" for k in sorted(self.skipped)))
        for key, ratio in self.worst.items():
            assert ratio <= 1, (what, key, ratio)
            share = self.skipped[key] / max(self.cells[key], 1)
            assert share < 0.01 if "thin" in key else share == 0, (what, key, share)
