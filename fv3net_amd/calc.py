"""``vcm.calc.calc``'s ``local_time`` and ``weighted_average`` (external/vcm/vcm/calc/calc.py:25-49)."""
from typing import Hashable, Sequence

import numpy as np
import torch

from . import ops
from .select import cell_weights, cells_last, ratio_like
from .xr_compat import DataArray, Dataset, from_compat, to_compat

HOUR_PER_DEG_LONGITUDE = 1.0 / 15


def fractional_hour(times) -> np.ndarray:
    """``hour + minute / 60 + second / 3600`` of every time (datetime, cftime or numpy datetime64 values)."""
    times = np.atleast_1d(np.asarray(times))
    if np.issubdtype(times.dtype, np.datetime64):
        seconds = (times.astype("datetime64[s]") - times.astype("datetime64[D]")).astype(np.int64)
        hour, minute, second = seconds // 3600, seconds % 3600 // 60, seconds % 60
    else:
        hour, minute, second = (np.array([getattr(t, k) for t in times.ravel()]).reshape(times.shape) for k in ("hour", "minute", "second"))
    return hour + (minute / 60.0) + (second / 3600.0)


def local_time(ds, time: Hashable = "initial_time", lon_var: Hashable = "lon"):
    """Local solar time in hours, [time, *dims of the longitude]: ``(fractional hour + lon / 15) % 24``.  A table of the
    grid's size per time, computed where the longitudes are read: on the host."""
    d = to_compat(ds)
    lon = d[lon_var]
    times = np.asarray(d.coords[time])
    hours = fractional_hour(times)
    scaled = lon.values * HOUR_PER_DEG_LONGITUDE
    if times.ndim == 0:
        return from_compat(DataArray((hours[0] + scaled) % 24, dims=lon.dims, coords=lon.coords), ds)
    value = (hours.reshape((-1,) + (1,) * scaled.ndim) + scaled) % 24
    return from_compat(DataArray(value, dims=(time,) + tuple(lon.dims), coords={**lon.coords, time: times}), ds)


def weighted_average(array, weights, dims: Sequence[Hashable] = ("tile", "y", "x")):
    """``array.weighted(weights.fillna(0.0)).mean(dims)``: ``sum(w x) / sum(w where x is not NaN)`` over ``dims``, for a
    DataArray or every variable of a Dataset, summed on the device by ``ops.group_sums`` with one group of all cells."""
    dims = [dims] if isinstance(dims, str) else list(dims)
    sizes = dict(to_compat(weights).sizes)
    plan = w = None

    def one(da: DataArray) -> DataArray:
        nonlocal plan, w
        if not set(dims) <= set(da.dims):
            raise ValueError(f"{da.name!r} lacks some of the dimensions {dims}")
        t, other = cells_last(da, dims)
        if plan is None:
            sizes.update({k: da.sizes[k] for k in dims})
            w = cell_weights(weights, dims, sizes)
            plan = ops.group_plan(torch.zeros((1, t.shape[-1]), dtype=torch.int32, device=t.device), 1)
        sums = ops.group_sums(t, None, w, plan, z_axis=1).cpu().numpy()
        mean = ratio_like(sums[2, 0], sums[1, 0], da, t).reshape([da.sizes[k] for k in other])
        return DataArray(mean, dims=tuple(other), coords={k: v for k, v in da.coords.items() if k in other}, name=da.name,
                         attrs=da.attrs)

    d = to_compat(array)
    if isinstance(d, Dataset):
        out = Dataset(attrs=d.attrs)
        for v in d:
            out[v] = one(d[v])
        return from_compat(out, array)
    return from_compat(one(d), array)
