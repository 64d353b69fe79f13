"""``vcm.histogram`` and ``vcm.histogram2d`` (external/vcm/vcm/calc/histogram.py) with the counting on the device
(``ops.histogram_counts`` / ``ops.histogram2d_counts``).  Only explicit bin edges are accepted: an integer ``bins`` or a
``range=`` would have numpy derive the edges from the data's extremes."""
from typing import Tuple

import numpy as np

from . import ops
from .cubedsphere._device import on_device
from .xr_compat import DataArray, from_compat, to_compat


def _explicit_edges(bins, what: str = "bins") -> np.ndarray:
    if bins is None or np.ndim(bins) != 1:
        raise ValueError(f"{what} must be an explicit 1-D array of bin edges (an integer number of bins is not supported)")
    edges = np.asarray(bins)
    if len(edges) < 2:
        raise ValueError(f"{what} must hold at least two edges")
    if np.any(edges[:-1] > edges[1:]):
        raise ValueError("`bins` must increase monotonically, when an array")
    return edges


def density_of(count: np.ndarray, edges: np.ndarray) -> np.ndarray:
    """``np.histogram(..., density=True)``: ``n / diff(bins) / n.sum()`` in float64, in that order."""
    db = np.array(np.diff(edges), float)
    return count / db / count.sum()


def histogram(da, bins=None, density: bool = False, **kwargs) -> Tuple[DataArray, DataArray]:
    """Counts (or the density) and bin widths of ``da`` over the explicit edges ``bins``; both carry the left edges as the
    coordinate ``f"{da.name}_bins"`` (``"bins"`` for an unnamed array)."""
    if kwargs:
        raise ValueError(f"only bins= (explicit edges) and density= are supported, got {sorted(kwargs)}")
    edges = _explicit_edges(bins)
    d = to_compat(da)
    coord_name = f"{d.name}_bins" if d.name is not None else "bins"
    x = on_device(d.data)
    count = ops.histogram_counts(x.reshape(-1), on_device(edges.astype(np.float64))).cpu().numpy()
    if density:
        count = density_of(count, edges)
    coords = {coord_name: edges[:-1]}
    width_da = DataArray(edges[1:] - edges[:-1], dims=[coord_name], coords=coords)
    count_da = DataArray(count, dims=[coord_name], coords=coords)
    if "units" in d.attrs:
        width_da.attrs["units"] = d.attrs["units"]
    return from_compat(count_da, da), from_compat(width_da, da)


def histogram2d(x, y, bins=None, **kwargs) -> Tuple[DataArray, DataArray, DataArray]:
    """Joint counts of ``x`` and ``y`` (any dim order; ``y`` is transposed to ``x``'s) over ``bins = [xedges, yedges]``, and
    the two bin widths; the coordinates are the left edges, ``f"{name}_bins"`` (``"xbins"`` / ``"ybins"`` when unnamed).
    Counts are float64, as ``np.histogram2d`` returns them."""
    if kwargs:
        raise ValueError(f"only bins=[xedges, yedges] is supported, got {sorted(kwargs)}")
    if not isinstance(bins, (list, tuple)) or len(bins) != 2 or np.ndim(bins[0]) != 1 or np.ndim(bins[1]) != 1:
        raise ValueError("bins must be [xedges, yedges], two explicit 1-D arrays of bin edges")
    xedges, yedges = _explicit_edges(bins[0], "bins[0]"), _explicit_edges(bins[1], "bins[1]")
    dx, dy = to_compat(x), to_compat(y)
    xname = f"{dx.name}_bins" if dx.name is not None else "xbins"
    yname = f"{dy.name}_bins" if dy.name is not None else "ybins"
    tx = on_device(dx.data).contiguous().reshape(-1)
    ty = on_device(dy.transpose(*dx.dims).data).contiguous().reshape(-1)
    count = ops.histogram2d_counts(tx, ty, on_device(xedges.astype(np.float64)), on_device(yedges.astype(np.float64)))
    count = count.cpu().numpy().astype(np.float64)
    xcoord, ycoord = {xname: xedges[:-1]}, {yname: yedges[:-1]}
    xwidth_da = DataArray(xedges[1:] - xedges[:-1], dims=[xname], coords=xcoord)
    ywidth_da = DataArray(yedges[1:] - yedges[:-1], dims=[yname], coords=ycoord)
    count_da = DataArray(count, dims=[xname, yname], coords={**xcoord, **ycoord})
    if "units" in dx.attrs:
        xwidth_da.attrs["units"] = dx.attrs["units"]
    if "units" in dy.attrs:
        ywidth_da.attrs["units"] = dy.attrs["units"]
    return from_compat(count_da, x), from_compat(xwidth_da, x), from_compat(ywidth_da, x)
