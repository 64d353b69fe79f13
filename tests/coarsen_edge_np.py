"""Plain numpy restatements of the kernels of csrc/coarsen.hip that oracle/coarsen_np.py does not already have: the boundary
vectors of the cube faces and the pick that turns them into halos, the centre-to-edge lines with explicit halos, weighted
means and reductions over strided windows, and the repeat.  tests/test_host_coarsen_edges.py pins them against the oracle
on the inputs of tests/coarsen_edge_cases.py; tests/test_gpu_coarsen_edges.py runs the kernels against them."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from oracle import coarsen_np
from oracle.coarsen_np import FV3_FACE_CONNECTIONS

# index of a tile's boundary vector in edge_rows_np: (axis the vector bounds, first / last line along it)
_ROW = {("x", "first"): 0, ("x", "last"): 1, ("y", "first"): 2, ("y", "last"): 3}


def int_view(a):
    """The words of ``a`` as integers of the same width: what a word copy must preserve (NaN payloads, the sign of a zero)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def assert_same_words(got, want, err_msg=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (err_msg, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(int_view(got), int_view(want), err_msg=err_msg)


def assert_same_outside_nan(got, want, err_msg=""):
    """Equal dtype and shape, NaNs in the same places, every other word equal (so a zero keeps its sign)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (err_msg, got.dtype, want.dtype, got.shape, want.shape)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{err_msg} (NaN pattern)")
    np.testing.assert_array_equal(np.where(nan, 0, int_view(got)), np.where(nan, 0, int_view(want)), err_msg=err_msg)


def cast_np(x, dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(dtype)


def edge_rows_np(a):
    """[tile, ..., n, n] -> [tile, 4, ..., n]: 0: x = 0, 1: x = n - 1 (indexed by y), 2: y = 0, 3: y = n - 1 (indexed by x)."""
    a = np.asarray(a)
    return np.stack([a[..., :, 0], a[..., :, -1], a[..., 0, :], a[..., -1, :]], axis=1)


def halo_pick_np(rows, tiles, axis):
    """(lo, hi) [len(tiles), ..., n] for ``axis`` from the boundary vectors of all six tiles: the left neighbour's last line
    along its connecting axis, the right neighbour's first; a neighbour joined through its other axis is read reversed."""
    lo, hi = [], []
    for t in tiles:
        (ln, la), (rn, ra) = FV3_FACE_CONNECTIONS[int(t)][axis]
        left, right = rows[ln, _ROW[(la, "last")]], rows[rn, _ROW[(ra, "first")]]
        lo.append(left if la == axis else left[..., ::-1])
        hi.append(right if ra == axis else right[..., ::-1])
    return np.stack(lo), np.stack(hi)


def interp_lines_np(x, lo, hi, axis, step=1):
    """``0.5 * (left + right)`` in ``x``'s dtype on every ``step``-th of the n + 1 edges along the last (``axis`` = 0) or
    second-to-last (``axis`` = 1) dim of a rectangular field; ``lo`` / ``hi`` [..., n_along_the_edge] lie beyond the two ends."""
    x = np.asarray(x)
    lo, hi = np.asarray(lo, x.dtype), np.asarray(hi, x.dtype)
    half = x.dtype.type(0.5)
    with np.errstate(over="ignore", invalid="ignore"):
        if axis == 0:
            ext = np.concatenate([lo[..., :, None], x, hi[..., :, None]], axis=-1)
            return (half * (ext[..., :, :-1] + ext[..., :, 1:]))[..., :, ::step].astype(x.dtype)
        ext = np.concatenate([lo[..., None, :], x, hi[..., None, :]], axis=-2)
        return (half * (ext[..., :-1, :] + ext[..., 1:, :]))[..., ::step, :].astype(x.dtype)


def _windows(a, window, stride):
    """[..., ny, nx] -> [..., nyo, nxo, by, bx]: the windows (by, bx) that start every (sy, sx) cells and fit the field."""
    (by, bx), (sy, sx) = window, stride
    return sliding_window_view(np.asarray(a), (by, bx), axis=(-2, -1))[..., ::sy, ::sx, :, :]


def window_average_np(obj, w, window, stride):
    """(mean, sum|obj * w|, sum(w), n) over strided windows, in float64 from the inputs as stored: a NaN product is left out
    of the numerator, a NaN weight out of the denominator; a NaN ``obj`` with a finite weight still counts in the denominator
    (``weights.coarsen(...).sum()``).  ``w`` broadcasts against ``obj`` with numpy's rules."""
    obj = np.asarray(obj, np.float64)
    w = np.broadcast_to(np.asarray(w, np.float64), obj.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        p = obj * w
    pw, ww = _windows(p, window, stride), _windows(w, window, stride)
    with np.errstate(invalid="ignore", divide="ignore"):
        num = np.where(np.isnan(pw), 0.0, pw).sum(axis=(-2, -1))
        mag = np.where(np.isnan(pw), 0.0, np.abs(pw)).sum(axis=(-2, -1))
        den = np.where(np.isnan(ww), 0.0, ww).sum(axis=(-2, -1))
        return num / den, mag, den, window[0] * window[1]


def window_reduce_np(a, window, stride, op, nan_policy="skip"):
    """sum / mean / min / max ('skip': xarray's NaN-skipping coarsen; 'propagate': numpy's plain reductions), median
    (numpy.median) and mode (scipy.stats.mode 1.7.3 as oracle.coarsen_np._mode_1d, 'propagate' or 'omit') over strided
    windows, in ``a``'s dtype."""
    a = np.asarray(a)
    v = _windows(a, window, stride)
    v = v.reshape(v.shape[:-2] + (-1,))
    isfloat = np.issubdtype(a.dtype, np.floating)
    skip = isfloat and nan_policy == "skip"
    with np.errstate(invalid="ignore"), np.testing.suppress_warnings() as sup:
        sup.filter(RuntimeWarning)
        if op == "sum":
            out = (np.where(np.isnan(v), 0, v) if skip else v).sum(axis=-1)
        elif op == "mean":
            out = np.nanmean(v, axis=-1) if skip else v.mean(axis=-1)
        elif op == "min":
            out = np.nanmin(v, axis=-1) if skip else v.min(axis=-1)
        elif op == "max":
            out = np.nanmax(v, axis=-1) if skip else v.max(axis=-1)
        elif op == "median":
            out = np.median(v, axis=-1)
        elif op == "mode":
            out = np.empty(v.shape[:-1], a.dtype)
            for idx in np.ndindex(out.shape):
                out[idx] = coarsen_np._mode_1d(v[idx], nan_policy)
        else:
            raise ValueError(f"unknown reduction {op!r}")
    return out.astype(a.dtype)


def repeat_np(a, fy, fx):
    return np.repeat(np.repeat(np.asarray(a), fy, axis=-2), fx, axis=-1)
