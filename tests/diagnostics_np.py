"""The checker of the device diagnostics: a float64 numpy restatement that follows the reference line by line
(workflows/diagnostics/fv3net/diagnostics/offline/compute_diagnostics.py, _shared/transform.py, vcm/select.py,
vcm/calc/histogram.py, vcm/calc/calc.py, vcm/interpolate.py) -- masks first, then ``nansum`` / ``nanmean`` reductions,
``np.digitize(right=True)`` for the ``(lo, hi]`` bins of ``groupby_bins``, ``np.histogram`` / ``np.histogram2d`` and the
two-pass variance.  Arrays are [time, (level,) cell] with the horizontal dims flattened."""
import warnings

import numpy as np

GRAVITY = 9.80665
KG_M2S_TO_MM_DAY = (1e3 * 86400) / 997.0
TOA_PRESSURE = 300.0
PRESSURE_GRID = np.array([
    300.0, 500.0, 700.0, 1000.0, 2000.0, 3000.0, 5000.0, 7000.0, 10000.0, 12500.0, 15000.0, 17500.0, 20000.0, 22500.0, 25000.0,
    30000.0, 35000.0, 40000.0, 45000.0, 50000.0, 55000.0, 60000.0, 65000.0, 70000.0, 75000.0, 77500.0, 80000.0, 82500.0, 85000.0,
    87500.0, 90000.0, 92500.0, 95000.0, 97500.0, 100000.0])
SURFACE_TYPE_CODES = {"sea": (0, 2), "land": (1,), "seaice": (2,)}
WVP, COL_MOISTENING, COL_DRYING = "water_vapor_path", "column_integrated_Q2", "minus_column_integrated_q2"
HISTOGRAM_BINS = {
    WVP: np.linspace(-10, 90, 101),
    COL_DRYING: np.linspace(-50, 150, 101),
    "column_integrated_q2": np.linspace(-150, 50, 101),
    "total_precip_to_surface": np.logspace(-1, np.log10(500), 101),
}
ZONAL_BINS = np.arange(-90, 91, 2)


# ---------------------------------------------------------------------------------------------------------------------
# ops.group_sums
# ---------------------------------------------------------------------------------------------------------------------
def group_sums(a, b, w, group_id, n_groups):
    """(sums, abs_sums, n): float64 [10, n_groups, nz] sums of the ten statistics and of their terms' magnitudes, and the
    cells per group [n_groups].  a, b: [n_batch, nz, n_inner] (b may be None); w: [n_batch, n_inner] or None; group_id:
    [n_batch, n_inner].  Terms are formed in float64 exactly as the kernel forms them; ``np.nansum`` adds them."""
    a = np.asarray(a, dtype=np.float64)
    n_batch, nz, n_inner = a.shape
    cells = lambda x: np.asarray(x, dtype=np.float64).transpose(0, 2, 1).reshape(-1, nz)  # noqa: E731  [cell, level]
    av = cells(a)
    wv = (np.ones(n_batch * n_inner) if w is None else np.asarray(w, dtype=np.float64).reshape(-1))[:, None] * np.ones((1, nz))
    nan = np.full_like(av, np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = [wv, np.where(np.isnan(av), nan, wv), wv * av, (wv * av) * av]
        if b is not None:
            bv = cells(b)
            d = av - bv
            terms += [np.where(np.isnan(bv), nan, wv), wv * bv, (wv * bv) * bv, np.where(np.isnan(d), nan, wv), wv * d, (wv * d) * d]
    gid = np.asarray(group_id).reshape(-1)
    sums, abs_sums = np.zeros((10, n_groups, nz)), np.zeros((10, n_groups, nz))
    n = np.zeros(n_groups, dtype=np.int64)
    for g in range(n_groups):
        sel = gid == g
        n[g] = sel.sum()
        for s, t in enumerate(terms):
            with np.errstate(invalid="ignore"):
                sums[s, g] = np.nansum(t[sel], axis=0)
                abs_sums[s, g] = np.nansum(np.abs(t[sel]), axis=0)
    return sums, abs_sums, n


# ---------------------------------------------------------------------------------------------------------------------
# the offline diagnostics
# ---------------------------------------------------------------------------------------------------------------------
def mask_array(region, arr, latitude, land_sea_mask, net_precipitation=None):
    """transform.py:288-318 (``arr.where(...)``: NaN outside the region)."""
    arr = np.asarray(arr, dtype=np.float64)
    if net_precipitation is None:
        net_precipitation = np.full_like(arr, np.nan)
    with np.errstate(invalid="ignore"):
        if region == "tropics":
            keep = np.abs(latitude) <= 10.0
        elif region == "tropics15":
            keep = np.abs(latitude) <= 15.0
        elif region == "tropics20":
            keep = np.abs(latitude) <= 20.0
        elif region == "global":
            return arr.copy()
        elif region == "positive_net_precipitation":
            keep = net_precipitation > 0.0
        elif region == "negative_net_precipitation":
            keep = net_precipitation <= 0.0
        elif region in SURFACE_TYPE_CODES:
            keep = np.zeros(np.shape(land_sea_mask), dtype=bool)
            for code in SURFACE_TYPE_CODES[region]:
                keep = np.logical_or(keep, land_sea_mask == code)
        else:
            raise ValueError(f"Masking procedure for region '{region}' is not defined.")
    return np.where(keep, arr, np.nan)


def net_precipitation(q2, delp):
    """minus_column_integrated_moistening (vertically_dependent.py:18-22, 310-327); [time, level, cell] -> [time, cell]."""
    return KG_M2S_TO_MM_DAY * np.nansum(q2 * -1 * delp / GRAVITY, axis=1)


def pressure_at_midpoint_log(delp):
    pi = np.cumsum(np.concatenate([np.full_like(delp[:, :1], TOA_PRESSURE), delp], axis=1), axis=1)
    return delp / np.diff(np.log(pi), axis=1)


def interpolate_to_pressure_levels(field, delp, levels=PRESSURE_GRID):
    """Linear in the midpoint pressure of each column, NaN outside the column; [time, level, cell] -> [time, pressure, cell]."""
    x, y = pressure_at_midpoint_log(delp), np.asarray(field, dtype=np.float64)
    out = np.full((x.shape[0], len(levels), x.shape[2]), np.nan)
    for j, xp in enumerate(levels):
        for k in range(x.shape[1] - 1):
            hit = (x[:, k] <= xp) & (xp < x[:, k + 1])
            weight = (xp - x[:, k]) / (x[:, k + 1] - x[:, k])
            out[:, j] = np.where(hit, y[:, k] * (1 - weight) + y[:, k + 1] * weight, out[:, j])
        out[:, j] = np.where(x[:, -1] == xp, y[:, -1], out[:, j])
    return out


def weighted_mean(x, w):
    """compute_diagnostics.py:93-95 over the cells: ``(ds * weights).sum(dims) / weights.sum(dims)``, both skipping NaN."""
    w = w if x.ndim == w.ndim else w[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.nansum(x * w, axis=-1) / np.nansum(w * np.ones_like(x), axis=-1)


def time_mean(x):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(x, axis=0)


def bin_index(values, bins):
    idx = np.digitize(values, bins, right=True) - 1
    return np.where((idx < 0) | (idx >= len(bins) - 1), -1, idx)


def zonal_average(lat, x, bins=ZONAL_BINS):
    """vcm.zonal_average_approximate, unweighted: the NaN-skipping mean over the cells of each bin; [..., cell] -> [..., bin]."""
    idx = bin_index(lat, bins)
    out = np.full(x.shape[:-1] + (len(bins) - 1,), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for i in range(len(bins) - 1):
            if np.any(idx == i):
                out[..., i] = np.nanmean(x[..., idx == i], axis=-1)
    return out


def variance_two_pass(target, w):
    mean = time_mean(weighted_mean(target, w))
    return time_mean(weighted_mean((mean[..., None] - target) ** 2, w))


def variance_moments(target, w):
    """The form the streaming implementation uses: m^2 mean_t(S4 / S0) - 2 m mean_t(S5 / S0) + mean_t(S6 / S0)."""
    wb = w if target.ndim == w.ndim else w[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        s0 = np.nansum(wb * np.ones_like(target), axis=-1)
        r4 = time_mean(np.nansum(np.where(np.isnan(target), np.nan, wb), axis=-1) / s0)
        r5 = time_mean(np.nansum(wb * target, axis=-1) / s0)
        r6 = time_mean(np.nansum(wb * target * target, axis=-1) / s0)
    return r5 * r5 * r4 - 2.0 * r5 * r5 + r6


def offline_diagnostics(prediction, target, delp, lat, lon, area, land_sea_mask, hours):
    """Every output of ``OfflineDiagnostics.compute`` for the whole stack of time steps at once.  prediction / target: dicts
    of [time, cell] (2-D) or [time, level, cell] (3-D) arrays; delp [time, level, cell]; hours: the fractional hour of
    every time step."""
    out = {}
    p64 = {k: np.asarray(v, dtype=np.float64) for k, v in prediction.items()}
    t64 = {k: np.asarray(target[k], dtype=np.float64) for k in prediction}
    delp = np.asarray(delp, dtype=np.float64)
    precip = net_precipitation(np.asarray(target["Q2"], dtype=np.float64), delp) if "Q2" in target else None
    area_t = np.broadcast_to(np.asarray(area, dtype=np.float64), (delp.shape[0], len(lat)))
    masked_area = {d: mask_array(d, area_t, lat, land_sea_mask, precip if "precipitation" in d else None)
                   for d in ("global", "land", "sea", "positive_net_precipitation", "negative_net_precipitation")}
    both = lambda f: np.stack([f("predict"), f("target")])  # noqa: E731
    for v in prediction:
        name = v.lower()
        is_3d = p64[v].ndim == 3
        pairs = [("model_level", p64[v], t64[v]), ("pressure_level", interpolate_to_pressure_levels(p64[v], delp),
                                                   interpolate_to_pressure_levels(t64[v], delp))] if is_3d else [("2d", p64[v], t64[v])]
        for label, p, t in pairs:
            for d in ("global", "sea", "land"):
                w = masked_area[d]
                out[f"{name}_mse_{label}_{d}"] = time_mean(weighted_mean((p - t) ** 2, w))
                out[f"{name}_variance_{label}_{d}"] = variance_two_pass(t, w)
                if label != "model_level":
                    out[f"{name}_bias_{label}_{d}"] = time_mean(weighted_mean(p - t, w))
            for d in masked_area if label == "model_level" else ("global", "land", "sea"):
                w = masked_area[d]
                out[f"{name}_time_domain_mean_{label}_{d}"] = np.stack([time_mean(weighted_mean(p, w)), time_mean(weighted_mean(t, w))])
            if label == "model_level":
                continue
            for d in ("global", "sea", "land"):
                pm, tm = mask_array(d, p, lat, land_sea_mask), mask_array(d, t, lat, land_sea_mask)
                out[f"{name}_bias_{label}_zonal_avg_{d}"] = time_mean(zonal_average(lat, pm - tm))
                if is_3d:
                    out[f"{name}_mse_{label}_zonal_avg_{d}"] = time_mean(zonal_average(lat, (pm - tm) ** 2))
                    out[f"{name}_variance_{label}_zonal_avg_{d}"] = (time_mean(zonal_average(lat, tm ** 2))
                                                                    - time_mean(zonal_average(lat, tm)) ** 2)
                    # mask_area only: the unweighted zonal mean does not read the area
                    out[f"{name}_time_domain_mean_{label}_zonal_avg_{d}"] = np.stack(
                        [time_mean(zonal_average(lat, p)), time_mean(zonal_average(lat, t))])
        if not is_3d:
            local = np.floor((np.asarray(hours)[:, None] + lon * (1.0 / 15)) % 24)
            present = np.unique(local[~np.isnan(local)])
            for d in ("global", "land", "sea"):
                pm, tm = mask_array(d, p64[v], lat, land_sea_mask), mask_array(d, t64[v], lat, land_sea_mask)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    out[f"{name}_diurnal_cycle_{d}"] = np.stack([[np.nanmean(x[local == h]) for h in present] for x in (pm, tm)])
            out["local_time"] = present
    if COL_MOISTENING in prediction and WVP in prediction:
        tropical_sea = lambda x: mask_array("sea", mask_array("tropics20", x, lat, land_sea_mask), lat, land_sea_mask)  # noqa: E731
        src = {"predict": p64, "target": t64}
        bins = [HISTOGRAM_BINS[WVP], HISTOGRAM_BINS[COL_DRYING]]
        out[f"{WVP}_versus_{COL_DRYING}_hist_2d"] = both(lambda k: np.histogram2d(
            tropical_sea(src[k][WVP]).ravel(), tropical_sea(-src[k][COL_MOISTENING]).ravel(), bins=bins)[0])
        out[f"{WVP}_bin_width_hist_2d"] = both(lambda k: np.diff(bins[0]))
        out[f"{COL_DRYING}_bin_width_hist_2d"] = both(lambda k: np.diff(bins[1]))
        for var in (WVP, COL_MOISTENING, COL_DRYING):
            edges = HISTOGRAM_BINS[var.lower()]
            data = lambda k: -src[k][COL_MOISTENING] if var == COL_DRYING else src[k][var]  # noqa: E731
            out[f"{var.lower()}_histogram"] = both(lambda k: np.histogram(data(k), bins=edges, density=True)[0])
            out[f"{var.lower()}_bin_width_histogram"] = both(lambda k: np.diff(edges))
    return out


def e2e_inputs(seed=0, n_tile=6, n=12, nz=5, nt=3, mixed_sign_q2=False):
    """The end-to-end case of the host and GPU tests: C12, 5 levels, 3 time steps, targets drawn from U(0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    nc = n_tile * n * n
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, nc)))
    lon = rng.uniform(0, 360, nc)
    area = rng.uniform(0.5, 1.5, nc).astype(np.float32)
    mask = rng.choice([0.0, 1.0, 2.0], size=nc, p=[0.55, 0.3, 0.15])
    delp = rng.uniform(12000, 26000, (nt, nz, nc))
    target, prediction = {}, {}
    for name, levels, scale in (("dQ1", nz, 1.0), ("Q2", nz, 1.0), ("water_vapor_path", 0, 40.0), ("column_integrated_Q2", 0, 20.0),
                                ("net_heating", 0, 1.0)):
        shape = (nt, levels, nc) if levels else (nt, nc)
        target[name] = (scale * rng.uniform(0.5, 1.5, shape)).astype(np.float32)
        prediction[name] = (target[name] + scale * rng.normal(0, 0.2, shape)).astype(np.float32)
    if mixed_sign_q2:
        target["Q2"] = (target["Q2"] * rng.choice([-1.0, 1.0], size=(nt, 1, nc))).astype(np.float32)
    hours = np.array([0.0, 3.0, 7.5])[:nt]
    return dict(prediction=prediction, target=target, delp=delp, lat=lat, lon=lon, area=area, land_sea_mask=mask, hours=hours)
