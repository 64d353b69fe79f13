"""``vcm.select``'s approximate zonal and meridional means (external/vcm/vcm/select.py:18-77) on the device: the cells of
every latitude / longitude bin are summed by ``ops.group_sums``; the bin of a cell is found on the host (the grid is
read once), the fields stay where they are."""
from typing import Hashable, Optional, Sequence

import numpy as np
import torch

from . import ops
from .cubedsphere._device import on_device
from .xr_compat import DataArray, Dataset, from_compat, to_compat


def bin_index(values, bins) -> np.ndarray:
    """The bin ``(bins[i], bins[i + 1]]`` each value falls in, as ``pandas.cut(values, bins)`` (what xarray's
    ``groupby_bins`` uses); -1: in no bin (at or below the first edge, above the last, NaN)."""
    values = np.asarray(values, dtype=np.float64)
    bins = np.asarray(bins, dtype=np.float64)
    idx = np.digitize(values, bins, right=True) - 1
    return np.where((idx < 0) | (idx >= len(bins) - 1) | np.isnan(values), -1, idx).astype(np.int32)


def as_float(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype in (torch.float32, torch.float64) else ops.cast(t, torch.float64) if t.dtype in (torch.int32, torch.int64) \
        else t.to(torch.float64)


def cells_last(da: DataArray, cell_dims: Sequence[Hashable]):
    """``da`` as a device tensor [1, n_other, n_cells] with ``cell_dims`` flattened last; also the other dims."""
    other = [d for d in da.dims if d not in cell_dims]
    t = as_float(on_device(da.transpose(*other, *cell_dims).data)).contiguous()
    n_cells = int(np.prod([da.sizes[d] for d in cell_dims], dtype=np.int64))
    return t.reshape(1, -1, n_cells), other


def cell_weights(weights, cell_dims: Sequence[Hashable], sizes) -> Optional[torch.Tensor]:
    """Weights broadcast over ``cell_dims`` as a device tensor [1, n_cells] (None stays None)."""
    if weights is None:
        return None
    w = to_compat(weights)
    if not set(w.dims) <= set(cell_dims):
        raise ValueError(f"weights may only have the dimensions that are averaged over {tuple(cell_dims)}, got {w.dims}")
    t = as_float(on_device(w.transpose(*[d for d in cell_dims if d in w.dims]).data))
    t = t.reshape([sizes[d] if d in w.dims else 1 for d in cell_dims]).expand(*[sizes[d] for d in cell_dims])
    return t.contiguous().reshape(1, -1)


def ratio_like(num: np.ndarray, den: np.ndarray, da: DataArray, like: torch.Tensor):
    """``num / den`` (host tables, float64) in the field's float dtype, on the device if the field was."""
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (num / den).astype(np.float32 if like.dtype == torch.float32 else np.float64)
    return torch.from_numpy(out).to(da.data.device) if isinstance(da.data, torch.Tensor) else out


def _groupby_bins(data, group, group_name, bins, weights=None):
    g = to_compat(group)
    bins = np.asarray(bins, dtype=np.float64)
    n_bins = len(bins) - 1
    ids = torch.from_numpy(bin_index(g.values, bins).reshape(1, -1))
    plan = ops.group_plan(on_device(ids), n_bins)
    w = cell_weights(weights, g.dims, g.sizes)
    midpoints = 0.5 * (bins[:-1] + bins[1:])

    def one(da: DataArray) -> DataArray:
        if not set(g.dims) <= set(da.dims):
            return da
        t, other = cells_last(da, g.dims)
        sums = ops.group_sums(t, None, w, plan, z_axis=1).cpu().numpy()
        # unweighted: sum x / count of non-NaN x; weighted: sum w x / sum w over non-NaN x (xarray_utils.py:107-140)
        mean = ratio_like(sums[2].T, sums[1].T, da, t).reshape([da.sizes[d] for d in other] + [n_bins])
        coords = {k: v for k, v in da.coords.items() if k in other}
        coords[group_name] = midpoints
        return DataArray(mean, dims=tuple(other) + (group_name,), coords=coords, name=da.name, attrs=da.attrs)

    d = to_compat(data)
    if isinstance(d, Dataset):
        out = Dataset(attrs=d.attrs)
        for v in d:
            out[v] = one(d[v])
        return from_compat(out, data)
    return from_compat(one(d), data)


def zonal_average_approximate(lat, data, bins: Optional[Sequence[float]] = None, lat_name: str = "lat", weights=None):
    """Zonal mean of a DataArray or Dataset over latitude bins ``(lo, hi]`` (default ``np.arange(-90, 91, 2)``); the output
    coordinate ``lat_name`` holds the bin midpoints, empty bins are NaN."""
    if bins is None:
        bins = np.arange(-90, 91, 2)
    return _groupby_bins(data, lat, lat_name, bins, weights)


def meridional_average_approximate(lon, data, bins: Optional[Sequence[float]] = None, lon_name: str = "lon", weights=None):
    """Meridional mean over longitude bins ``(lo, hi]`` (default ``np.arange(0, 361, 2)``)."""
    if bins is None:
        bins = np.arange(0, 361, 2)
    return _groupby_bins(data, lon, lon_name, bins, weights)
