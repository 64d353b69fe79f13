"""The streaming form of the offline report's ``compute_diagnostics``
(workflows/diagnostics/fv3net/diagnostics/offline/compute_diagnostics.py with _shared/transform.py): predictions and targets
stay on the device, every ``update`` reduces its time steps to small tables (``ops.group_sums``, ``ops.histogram_counts``,
``ops.histogram2d_counts``), and ``compute`` turns the accumulated tables into the reference's Dataset.

The reference masks its inputs and then reduces; here every cell gets one class and the reductions are per class:

* area-weighted domains -- a per-time class from the surface type (``land_sea_mask`` 0, 1, 2, anything else) and the sign of
  the net precipitation of the target (``> 0``, ``<= 0``, unknown): 12 disjoint classes, of which ``global``, ``land``,
  ``sea``, ``positive_net_precipitation`` and ``negative_net_precipitation`` are unions (``DOMAIN_CLASSES``, the cells
  ``_mask_array`` leaves unmasked, transform.py:288-318).  Per time step the tables hold ``stat / stat0``: the denominator is
  the domain's area whatever the data's NaNs, as ``(ds * w).sum() / w.sum()`` has it; ``compute`` takes the NaN-skipping mean
  over time.
* zonal means -- groups are (latitude bin x surface type), unweighted, a ratio per time step and the mean over time.
* the diurnal cycle -- groups are (hour of local time x surface type), pooled over all time steps as the reference's
  ``groupby("local_time").mean()`` pools them; one plan per distinct time of day.
* histograms -- counts pooled over time; the density is formed in ``compute``.

Variances are linear in the per-time ratios once the time-mean ``m`` is known:
``mean_t wm((m - x)^2) = m^2 mean_t(S4 / S0) - 2 m mean_t(S5 / S0) + mean_t(S6 / S0)``.

Left out: ``time_mean_global`` (a running mean per cell: nothing is reduced in space), and the grouping variable
``local_time`` itself, which the reference's diurnal cycle carries along as a data variable.
"""
from typing import Dict, Hashable, List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..calc import HOUR_PER_DEG_LONGITUDE, fractional_hour
from ..cubedsphere._device import download_all, on_device
from ..histogram import density_of
from ..interpolate import PRESSURE_GRID
from ..select import as_float, bin_index
from ..xr_compat import DataArray, Dataset, to_compat

DOMAINS = ("land", "sea", "global", "positive_net_precipitation", "negative_net_precipitation")
SURFACE_DOMAINS = ("global", "sea", "land")
SURFACE_TYPE_CODES = {"sea": (0, 2), "land": (1,), "seaice": (2,)}
DERIVATION_DIM = "derivation"
WVP = "water_vapor_path"
COL_MOISTENING = "column_integrated_Q2"
COL_DRYING = "minus_column_integrated_q2"
# _shared/constants.py:15-20
HISTOGRAM_BINS = {
    "total_precip_to_surface": np.logspace(-1, np.log10(500), 101),
    WVP: np.linspace(-10, 90, 101),
    COL_DRYING: np.linspace(-50, 150, 101),
    "column_integrated_q2": np.linspace(-150, 50, 101),
}
ZONAL_BINS = np.arange(-90, 91, 2)
_GRAVITY = 9.80665
_TOA_PRESSURE = 300.0

# surface index: the three codes of land_sea_mask, then "none of them"; precipitation index: > 0, <= 0, unknown (NaN)
N_SURFACE, N_PRECIP = 4, 3
N_CLASSES = N_SURFACE * N_PRECIP
_SURFACE_OF_DOMAIN = {"global": (0, 1, 2, 3), "sea": (0, 2), "land": (1,), "seaice": (2,)}
DOMAIN_CLASSES = {
    "global": tuple(range(N_CLASSES)),
    "land": tuple(s * N_PRECIP + p for s in _SURFACE_OF_DOMAIN["land"] for p in range(N_PRECIP)),
    "sea": tuple(s * N_PRECIP + p for s in _SURFACE_OF_DOMAIN["sea"] for p in range(N_PRECIP)),
    "seaice": tuple(s * N_PRECIP + p for s in _SURFACE_OF_DOMAIN["seaice"] for p in range(N_PRECIP)),
    "positive_net_precipitation": tuple(s * N_PRECIP + 0 for s in range(N_SURFACE)),
    "negative_net_precipitation": tuple(s * N_PRECIP + 1 for s in range(N_SURFACE)),
}

# the names registered in compute_diagnostics.py, in its order; "time_mean_global" is left out (see the module docstring)
DIAGNOSTIC_NAMES = tuple(
    [f"{family}_{d}" for family in ("mse_2d", "mse_pressure_level", "mse_model_level", "variance_2d", "variance_pressure_level",
                                    "variance_model_level", "bias_2d", "bias_pressure_level", "bias_2d_zonal_avg",
                                    "bias_pressure_level_zonal_avg", "mse_pressure_level_zonal_avg",
                                    "variance_pressure_level_zonal_avg") for d in ("global", "sea", "land")]
    + [f"{family}_{d}" for family in ("diurnal_cycle", "time_domain_mean_2d", "time_domain_mean_pressure_level")
       for d in ("global", "land", "sea")]
    + [f"time_domain_mean_model_level_{d}" for d in ("global", "land", "sea", "positive_net_precipitation",
                                                     "negative_net_precipitation")]
    + [f"time_domain_mean_pressure_level_zonal_avg_{d}" for d in ("global", "land", "sea")]
    + ["hist_2d", "histogram"])


def output_name(variable: Hashable, diagnostic_name: str) -> str:
    """``merge_diagnostics`` (compute_diagnostics.py:32-52): the lower-cased variable, then the diagnostic's name."""
    return f"{str(variable).lower()}_{diagnostic_name}"


def surface_index(land_sea_mask: np.ndarray) -> np.ndarray:
    m = np.asarray(land_sea_mask)
    return np.where(m == 0, 0, np.where(m == 1, 1, np.where(m == 2, 2, 3))).astype(np.int32)


def precipitation_index(net_precipitation: Optional[np.ndarray], shape=None) -> np.ndarray:
    if net_precipitation is None:
        return np.full(shape, 2, dtype=np.int32)
    p = np.asarray(net_precipitation)
    with np.errstate(invalid="ignore"):
        return np.where(p > 0.0, 0, np.where(p <= 0.0, 1, 2)).astype(np.int32)


def cell_class(land_sea_mask, net_precipitation=None) -> np.ndarray:
    """The class of every cell (host restatement of what ``update`` does on the device)."""
    s = surface_index(land_sea_mask)
    return s * N_PRECIP + precipitation_index(net_precipitation, s.shape)


def region_mask(region: str, latitude, land_sea_mask, net_precipitation=None) -> np.ndarray:
    """The cells ``_mask_array(region, ...)`` leaves unmasked (transform.py:288-318): by class for the surface types and the
    two net-precipitation regions, by latitude for the tropics."""
    lat = np.asarray(latitude)
    if region in ("tropics", "tropics15", "tropics20"):
        return np.abs(lat) <= {"tropics": 10.0, "tropics15": 15.0, "tropics20": 20.0}[region]
    if region not in DOMAIN_CLASSES:
        raise ValueError(f"Masking procedure for region '{region}' is not defined.")
    return np.isin(cell_class(land_sea_mask, net_precipitation), DOMAIN_CLASSES[region])


class _TimeMean:
    """NaN-skipping mean over time of per-time tables (xarray's ``mean("time")``)."""

    def __init__(self):
        self.total = None
        self.count = None

    def add(self, table: np.ndarray):
        ok = ~np.isnan(table)
        if self.total is None:
            self.total, self.count = np.zeros(table.shape), np.zeros(table.shape, dtype=np.int64)
        self.total += np.where(ok, table, 0.0)
        self.count += ok

    def mean(self) -> np.ndarray:
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.total / self.count


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return num / den


class OfflineDiagnostics:
    """``grid`` holds ``lat``, ``lon``, ``area`` and ``land_sea_mask`` over ``horizontal_dims``.  ``update(prediction, target,
    delp)`` takes Datasets (this package's or xarray's) whose variables carry the horizontal dims, optionally
    ``vertical_dim`` and ``time_dim``; variables of the prediction are looked up in the target.  The time coordinate, when
    there is one, drives the diurnal cycle (without it that diagnostic is skipped)."""

    def __init__(self, grid, horizontal_dims: Sequence[Hashable] = ("x", "y", "tile"), vertical_dim: Hashable = "z",
                 time_dim: Hashable = "time", pressure_levels=PRESSURE_GRID):
        g = to_compat(grid)
        self.horizontal_dims = tuple(horizontal_dims)
        self.vertical_dim, self.time_dim = vertical_dim, time_dim
        lat = g["lat"]
        if set(lat.dims) != set(self.horizontal_dims):
            raise ValueError(f"the grid's lat has dims {lat.dims}, expected {self.horizontal_dims}")
        self.cell_dims = tuple(lat.dims)
        host = lambda name: np.asarray(g[name].transpose(*self.cell_dims).values).reshape(-1)  # noqa: E731
        self._lat, self._lon, self._mask = host("lat"), host("lon"), host("land_sea_mask")
        self.n_cells = self._lat.size
        self._area = as_float(on_device(g["area"].transpose(*self.cell_dims).data)).contiguous().reshape(1, -1)
        self.device = self._area.device
        self._surface = surface_index(self._mask)
        self._surface_dev = on_device(self._surface.astype(np.int64))
        self.pressure = np.asarray(to_compat(pressure_levels).values, dtype=np.float64)
        self._levels = None
        self.latitude = 0.5 * (ZONAL_BINS[:-1] + ZONAL_BINS[1:])
        lat_bin = bin_index(self._lat, ZONAL_BINS).astype(np.int64)
        zonal_id = np.where(lat_bin < 0, -1, lat_bin * N_SURFACE + self._surface)
        self._zonal_plan = ops.group_plan(on_device(zonal_id.reshape(1, -1)), len(self.latitude) * N_SURFACE)
        tropical_sea = region_mask("tropics20", self._lat, self._mask) & region_mask("sea", self._lat, self._mask)
        self._hist2d_mask = on_device(tropical_sea.astype(np.float64).reshape(1, -1))
        self._edges = {k: on_device(v.astype(np.float64)) for k, v in HISTOGRAM_BINS.items()}
        self._domain_plan_no_precip = None
        self._diurnal_plans: Dict[float, ops.GroupPlan] = {}
        self._means: Dict[tuple, _TimeMean] = {}
        self._diurnal: Dict[Hashable, np.ndarray] = {}
        self._counts: Dict[str, np.ndarray] = {}
        self._is_3d: Dict[Hashable, bool] = {}
        self._attrs: Dict[Hashable, dict] = {}
        self.n_times = 0

    # -- plans --------------------------------------------------------------------------------------------------------
    def _domain_plan(self, q2: Optional[torch.Tensor], delp: Optional[torch.Tensor]) -> ops.GroupPlan:
        """Classes of one time step.  The net precipitation is ``minus_column_integrated_moistening(Q2, delp)``
        (vertically_dependent.py:18-22, 310-327): only its sign is used, so its positive unit factor is left out."""
        if q2 is None or delp is None:
            if self._domain_plan_no_precip is None:
                ids = self._surface_dev * N_PRECIP + 2
                self._domain_plan_no_precip = ops.group_plan(ids.reshape(1, -1), N_CLASSES)
            return self._domain_plan_no_precip
        dt = torch.float64 if torch.float64 in (q2.dtype, delp.dtype) else torch.float32
        x = ops.ew("mul", ops.ew("mul_s", ops.cast(q2, dt), scalar=-1.0), ops.cast(delp, dt))
        x = ops.ew("fillna_s", ops.ew("div_s", x, scalar=_GRAVITY), scalar=0.0)  # (xarray's sum skips NaN)
        net = ops.column_sum(x.reshape(1, x.shape[0], -1), 1).reshape(-1)
        precip = torch.where(net > 0, 0, torch.where(net <= 0, 1, 2))
        return ops.group_plan((self._surface_dev * N_PRECIP + precip).reshape(1, -1), N_CLASSES)

    def _diurnal_plan(self, hour: float) -> ops.GroupPlan:
        plan = self._diurnal_plans.get(hour)
        if plan is None:
            local = np.floor((hour + self._lon * HOUR_PER_DEG_LONGITUDE) % 24)  # calc.py:25-30, compute_diagnostics.py:75-77
            ids = np.where(np.isnan(local), -1, local.astype(np.int64) * N_SURFACE + self._surface)
            plan = self._diurnal_plans[hour] = ops.group_plan(on_device(ids.reshape(1, -1)), 24 * N_SURFACE)
        return plan

    # -- input --------------------------------------------------------------------------------------------------------
    def _arranged(self, da: DataArray, n_times: Optional[int] = None) -> torch.Tensor:
        """[time, level, cell] (level = 1 without the vertical dim) on the device, float."""
        lead = [d for d in (self.time_dim, self.vertical_dim) if d in da.dims]
        extra = set(da.dims) - set(lead) - set(self.cell_dims)
        if extra or not set(self.cell_dims) <= set(da.dims):
            raise ValueError(f"{da.name!r} has dims {da.dims}: expected {self.cell_dims}, optionally {self.time_dim!r} and "
                             f"{self.vertical_dim!r}")
        t = as_float(on_device(da.transpose(*lead, *self.cell_dims).data)).contiguous()
        nt = da.sizes.get(self.time_dim, 1)
        t = t.reshape(nt, da.sizes.get(self.vertical_dim, 1), self.n_cells)
        if n_times is not None and nt != n_times:
            if nt != 1:
                raise ValueError(f"{da.name!r} has {nt} time steps, expected {n_times}")
            t = t.expand(n_times, -1, -1)
        return t

    def _pressure_levels(self, dtype) -> torch.Tensor:
        if self._levels is None or self._levels.dtype != dtype:
            levels = on_device(self.pressure).to(dtype)
            self._levels = levels.reshape(-1, 1).expand(-1, self.n_cells).contiguous()  # (the kernel reads levels per column)
        return self._levels

    # -- update -------------------------------------------------------------------------------------------------------
    def update(self, prediction, target, delp=None) -> None:
        pred, targ = to_compat(prediction), to_compat(target)
        names = [v for v in pred if set(self.cell_dims) <= set(pred[v].dims)]
        if not names:
            return
        missing = [v for v in names if v not in targ.data_vars]
        if missing:
            raise KeyError(f"the target lacks {missing}")
        n_times = max(pred[v].sizes.get(self.time_dim, 1) for v in names)
        times = pred.coords.get(self.time_dim)
        hours = None if times is None else fractional_hour(times)
        if hours is not None and len(hours) != n_times:
            raise ValueError(f"{len(hours)} time coordinates for {n_times} time steps")
        a = {v: self._arranged(pred[v], n_times) for v in names}
        b = {v: self._arranged(targ[v], n_times) for v in names}
        for v in names:
            is_3d = self.vertical_dim in pred[v].dims
            if self._is_3d.setdefault(v, is_3d) != is_3d:
                raise ValueError(f"{v!r} changed its dimensionality between updates")
            self._attrs.setdefault(v, dict(pred[v].attrs))
        dp = None if delp is None else self._arranged(to_compat(delp), n_times)
        q2 = self._arranged(targ["Q2"], n_times) if dp is not None and "Q2" in targ.data_vars else None
        if q2 is not None and q2.shape[1] != dp.shape[1]:
            raise ValueError("Q2 and delp differ in their number of levels")
        if dp is None and any(self._is_3d[v] for v in names):
            raise ValueError("delp is needed to bring 3-D variables to pressure levels")

        for t in range(n_times):
            tables = {}
            domain_plan = self._domain_plan(None if q2 is None else q2[t], None if dp is None else dp[t])
            diurnal_plan = None if hours is None else self._diurnal_plan(float(hours[t]))
            p_mid = None
            for v in names:
                at, bt = a[v][t:t + 1], b[v][t:t + 1]
                if self._is_3d[v]:
                    tables[(v, "model_level")] = ops.group_sums(at, bt, self._area, domain_plan, z_axis=1)
                    if p_mid is None:
                        p_mid = ops.pressure_at_midpoint_log(dp[t], _TOA_PRESSURE, z_axis=0).to(torch.float64)
                        levels = self._pressure_levels(p_mid.dtype)
                    # interpolate_to_pressure_levels (interpolate.py): linear in the midpoint pressure, NaN outside the column
                    ap = ops.interpolate_2d(levels, p_mid, at[0], z_axis=0).unsqueeze(0)
                    bp = ops.interpolate_2d(levels, p_mid, bt[0], z_axis=0).unsqueeze(0)
                    tables[(v, "pressure_level")] = ops.group_sums(ap, bp, self._area, domain_plan, z_axis=1)
                    tables[(v, "pressure_level_zonal")] = ops.group_sums(ap, bp, None, self._zonal_plan, z_axis=1)
                else:
                    tables[(v, "2d")] = ops.group_sums(at, bt, self._area, domain_plan, z_axis=1)
                    tables[(v, "2d_zonal")] = ops.group_sums(at, bt, None, self._zonal_plan, z_axis=1)
                    if diurnal_plan is not None:
                        tables[(v, "diurnal")] = ops.group_sums(at, bt, None, diurnal_plan, z_axis=1)
            self._accumulate(download_all(tables))
        self.n_times += n_times

        if COL_MOISTENING in names and WVP in names and not self._is_3d[COL_MOISTENING] and not self._is_3d[WVP]:
            counts = {}
            for derivation, src in (("predict", a), ("target", b)):
                wvp, moistening = src[WVP], src[COL_MOISTENING]  # [time, 1, cell]
                drying = ops.ew("mul_s", moistening, scalar=-1.0)
                nan = float("nan")
                counts[("hist_2d", derivation)] = ops.histogram2d_counts(
                    ops.ew("where_s", wvp, self._hist2d_mask, scalar=nan), ops.ew("where_s", drying, self._hist2d_mask, scalar=nan),
                    self._edges[WVP], self._edges[COL_DRYING])
                for name, x in ((WVP, wvp), (COL_MOISTENING, moistening), (COL_DRYING, drying)):
                    counts[(name, derivation)] = ops.histogram_counts(x, self._edges[name.lower()])
            for key, c in download_all(counts).items():
                self._counts[key] = self._counts.get(key, 0) + c

    def _accumulate(self, tables: Dict[tuple, np.ndarray]) -> None:
        for (v, kind), s in tables.items():
            nz = s.shape[-1]
            if kind in ("2d", "model_level", "pressure_level"):
                domains = DOMAINS if kind == "model_level" else SURFACE_DOMAINS
                for d in domains:
                    sd = s[:, list(DOMAIN_CLASSES[d])].sum(axis=1)  # [10, nz], classes added in class order
                    self._means.setdefault((v, kind, d), _TimeMean()).add(_ratio(sd, sd[0]))
            elif kind.endswith("zonal"):
                by_surface = s.reshape(10, -1, N_SURFACE, nz)
                for d in SURFACE_DOMAINS:
                    sd = by_surface[:, :, list(_SURFACE_OF_DOMAIN[d])].sum(axis=2)  # [10, latitude, nz]
                    # pred mean, target mean, target mean square, bias, mse: each over the cells where its term is not NaN
                    ratios = np.stack([_ratio(sd[2], sd[1]), _ratio(sd[5], sd[4]), _ratio(sd[6], sd[4]), _ratio(sd[8], sd[7]),
                                       _ratio(sd[9], sd[7])])
                    self._means.setdefault((v, kind, d), _TimeMean()).add(ratios)
            else:  # the diurnal cycle pools the sums themselves
                self._diurnal[v] = self._diurnal.get(v, 0.0) + s.reshape(10, 24, N_SURFACE)

    # -- compute ------------------------------------------------------------------------------------------------------
    def compute(self) -> Dataset:
        out: Dict[str, DataArray] = {}
        derivation = {DERIVATION_DIM: np.array(["predict", "target"])}

        def put(v, name, values, dims, coords=None):
            out[output_name(v, name)] = DataArray(np.asarray(values), dims=dims, coords=coords, attrs=self._attrs.get(v))

        z, p, lat = self.vertical_dim, "pressure", "latitude"
        p_coord, lat_coord = {p: self.pressure}, {lat: self.latitude}
        for v, is_3d in self._is_3d.items():
            kinds = (("model_level", "model_level", (z,), {}), ("pressure_level", "pressure_level", (p,), p_coord)) if is_3d \
                else (("2d", "2d", (), {}),)
            for kind, label, dims, coords in kinds:
                for d in (DOMAINS if kind == "model_level" else SURFACE_DOMAINS):
                    r = self._means[(v, kind, d)].mean()  # [10, nz]: mean over time of stat / stat0
                    r = r if dims else r[:, 0]
                    if d in SURFACE_DOMAINS:
                        put(v, f"mse_{label}_{d}", r[9], dims, coords)
                        m = r[5]
                        put(v, f"variance_{label}_{d}", m * m * r[4] - 2.0 * m * r[5] + r[6], dims, coords)
                        if kind != "model_level":
                            put(v, f"bias_{label}_{d}", r[8], dims, coords)
                    put(v, f"time_domain_mean_{label}_{d}", np.stack([r[2], r[5]]), (DERIVATION_DIM,) + dims, {**derivation, **coords})
            zonal = "pressure_level_zonal" if is_3d else "2d_zonal"
            label = "pressure_level" if is_3d else "2d"
            zdims, zcoords = ((p, lat), {**p_coord, **lat_coord}) if is_3d else ((lat,), lat_coord)
            for d in SURFACE_DOMAINS:
                r = self._means[(v, zonal, d)].mean()  # [5, latitude, nz]
                r = np.swapaxes(r, 1, 2) if is_3d else r[:, :, 0]
                put(v, f"bias_{label}_zonal_avg_{d}", r[3], zdims, zcoords)
                if is_3d:
                    put(v, f"mse_{label}_zonal_avg_{d}", r[4], zdims, zcoords)
                    put(v, f"variance_{label}_zonal_avg_{d}", r[2] - r[1] ** 2, zdims, zcoords)
                    # (the reference masks the area here, which an unweighted zonal mean does not read: the data are whole)
                    g = self._means[(v, zonal, "global")].mean()
                    g = np.swapaxes(g, 1, 2)
                    put(v, f"time_domain_mean_{label}_zonal_avg_{d}", np.stack([g[0], g[1]]), (DERIVATION_DIM,) + zdims,
                        {**derivation, **zcoords})
            if not is_3d and v in self._diurnal:
                s = self._diurnal[v]  # [10, hour, surface]
                present = s[0].sum(axis=1) > 0  # the hours some cell fell in, whatever its data
                hours = np.arange(24.0)[present]
                for d in SURFACE_DOMAINS:
                    sd = s[:, :, list(_SURFACE_OF_DOMAIN[d])].sum(axis=2)[:, present]
                    put(v, f"diurnal_cycle_{d}", np.stack([_ratio(sd[2], sd[1]), _ratio(sd[5], sd[4])]),
                        (DERIVATION_DIM, "local_time"), {**derivation, "local_time": hours})
        if self._counts:
            stack = lambda key: np.stack([self._counts[(key, "predict")], self._counts[(key, "target")]])  # noqa: E731
            x_bins, y_bins = f"{WVP}_bins", f"{COL_DRYING}_bins"
            xe, ye = HISTOGRAM_BINS[WVP], HISTOGRAM_BINS[COL_DRYING]
            out[output_name(f"{WVP}_versus_{COL_DRYING}", "hist_2d")] = DataArray(
                stack("hist_2d").astype(np.float64), dims=(DERIVATION_DIM, x_bins, y_bins),
                coords={**derivation, x_bins: xe[:-1], y_bins: ye[:-1]})
            out[output_name(f"{WVP}_bin_width", "hist_2d")] = DataArray(np.stack([np.diff(xe)] * 2), dims=(DERIVATION_DIM, x_bins),
                                                                        coords={**derivation, x_bins: xe[:-1]})
            out[output_name(f"{COL_DRYING}_bin_width", "hist_2d")] = DataArray(np.stack([np.diff(ye)] * 2), dims=(DERIVATION_DIM, y_bins),
                                                                               coords={**derivation, y_bins: ye[:-1]})
            for name in (WVP, COL_MOISTENING, COL_DRYING):
                edges = HISTOGRAM_BINS[name.lower()]
                bins = f"{name}_bins"
                coords = {**derivation, bins: edges[:-1]}
                density = np.stack([density_of(c, edges) for c in stack(name)])
                out[output_name(name, "histogram")] = DataArray(density, dims=(DERIVATION_DIM, bins), coords=coords,
                                                                attrs=self._attrs.get(name))
                out[output_name(f"{name}_bin_width", "histogram")] = DataArray(np.stack([np.diff(edges)] * 2),
                                                                               dims=(DERIVATION_DIM, bins), coords=coords)
        return Dataset(out)
