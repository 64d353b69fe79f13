"""The device reductions of the offline diagnostics against the reference's known answers, the numpy checker
(tests/diagnostics_np.py) and numpy's histograms.

group_sums gate: the terms are bit-identical to the checker's by construction (float64, every product rounded once), so
only the order of summation differs; any order of n terms errs by at most (n - 1) 2^-53 sum|terms|, the checker's own
(pairwise) order by less: |got - want| <= 2 n 2^-53 sum|terms|.  Where the wanted sum is not finite (an infinity among the
terms) it must be met exactly."""
import numpy as np
import pytest
import torch

import diagnostics_np as ref
from fv3net_amd import calc, ops, select
from fv3net_amd import histogram as hist
from fv3net_amd.diagnostics import OfflineDiagnostics
from fv3net_amd.xr_compat import DataArray, Dataset

pytestmark = pytest.mark.gpu

NP_DTYPE = {"f32": np.float32, "f64": np.float64}


def dev(x, device):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(device)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's known answers, restated as literals
# ---------------------------------------------------------------------------------------------------------------------
def test_histogram():
    # external/vcm/tests/test_histogram.py:6-15
    data = DataArray(np.reshape(np.arange(0, 40, 2), (5, 4)), dims=["x", "y"], name="temperature")
    count, width = hist.histogram(data, bins=[0, 30, 40])
    assert count.dims == width.dims == ("temperature_bins",)
    np.testing.assert_array_equal(count.values, [15, 5])
    np.testing.assert_array_equal(width.values, [30, 10])
    np.testing.assert_array_equal(count.coords["temperature_bins"], [0, 30])
    np.testing.assert_array_equal(width.coords["temperature_bins"], [0, 30])


def test_histogram2d():
    # external/vcm/tests/test_histogram.py:18-37
    data_x, data_y = np.arange(0, 40, 2), np.arange(0, 20, 1)
    bins = [np.array([0, 20, 40]), np.array([0, 10, 20])]
    var1 = DataArray(np.reshape(data_x, (5, 4)), dims=["x", "y"], name="temp")
    var2 = DataArray(np.reshape(data_y, (5, 4)), dims=["x", "y"], name="humidity").transpose("y", "x")
    count, xwidth, ywidth = hist.histogram2d(var1, var2, bins=bins)
    assert count.dims == ("temp_bins", "humidity_bins")
    np.testing.assert_array_equal(count.values, [[10.0, 0.0], [0.0, 10.0]])
    np.testing.assert_array_equal(count.values, np.histogram2d(data_x, data_y, bins)[0])
    np.testing.assert_array_equal(xwidth.values, [20, 20])
    np.testing.assert_array_equal(ywidth.values, [10, 10])
    np.testing.assert_array_equal(count.coords["temp_bins"], [0, 20])
    np.testing.assert_array_equal(count.coords["humidity_bins"], [0, 10])


def test_weighted_mean_via_groupby_bins():
    # external/vcm/tests/test_xarray_utils.py:116-130, through select._groupby_bins as vcm.select calls it
    a = DataArray(np.arange(10), dims=["x"], name="foo")
    group = DataArray(np.arange(10), dims=["x"], name="bar")
    weights = DataArray((np.arange(10) % 2) == 1, dims=["x"])
    result = select.zonal_average_approximate(group, a, bins=np.arange(0, 11, 2), lat_name="bar", weights=weights)
    assert result.dims == ("bar",) and result.name == "foo" and result.values.dtype == np.float64
    np.testing.assert_array_equal(result.values, [1.0, 3.0, 5.0, 7.0, 9.0])
    np.testing.assert_array_equal(result.coords["bar"], [1.0, 3.0, 5.0, 7.0, 9.0])   # (the bins' midpoints)


def test_weighted_mean_via_groupby_bins_with_nans():
    # external/vcm/tests/test_xarray_utils.py:133-148
    values = np.arange(10, dtype=float)
    a = DataArray(np.where((values % 5) > 2, values, np.nan), dims=["x"], name="foo")
    group = DataArray(np.arange(10), dims=["x"], name="bar")
    weights = DataArray(np.ones(10, dtype=np.int64), dims=["x"])
    result = select.zonal_average_approximate(group, a, bins=np.arange(0, 11, 5), lat_name="bar", weights=weights)
    np.testing.assert_array_equal(result.values, [3.5, 8.5])
    unweighted = select.meridional_average_approximate(group, a.to_dataset(), bins=np.arange(0, 11, 5), lon_name="bar")
    np.testing.assert_array_equal(unweighted["foo"].values, [3.5, 8.5])


def test_weighted_average_and_local_time(device):
    rng = np.random.default_rng(3)
    x = rng.normal(size=(2, 6, 4, 4))
    x[0, 1, 2, 3] = np.nan
    w = rng.uniform(0.5, 1, (6, 4, 4))
    w[3, 0, 0] = np.nan   # fillna(0.0)
    got = calc.weighted_average(DataArray(x, dims=["time", "tile", "y", "x"], name="a"), DataArray(w, dims=["tile", "y", "x"]))
    w0 = np.where(np.isnan(w), 0.0, w)
    want = np.nansum(x * w0, axis=(1, 2, 3)) / np.sum(np.where(np.isnan(x), 0.0, w0), axis=(1, 2, 3))
    assert got.dims == ("time",)
    np.testing.assert_allclose(got.values, want, rtol=1e-13)
    import datetime
    ds = Dataset({"lon": DataArray(np.array([0.0, 90.0, 359.0], dtype=np.float32), dims=["x"])},
                 coords={"time": [datetime.datetime(2016, 8, 1, 3, 30), datetime.datetime(2016, 8, 1, 23, 0, 36)]})
    lt = calc.local_time(ds, time="time", lon_var="lon")
    assert lt.dims == ("time", "x")
    lon = np.array([0.0, 90.0, 359.0], dtype=np.float32)
    np.testing.assert_array_equal(lt.values, (np.array([3 + 30 / 60.0 + 0 / 3600.0, 23 + 0 / 60.0 + 36 / 3600.0])[:, None] + lon * (1.0 / 15)) % 24)


# ---------------------------------------------------------------------------------------------------------------------
# group_sums against the checker
# ---------------------------------------------------------------------------------------------------------------------
def check_group_sums(device, a, b, w, group_id, n_groups, z_axis=1):
    plan = ops.group_plan(dev(group_id, device), n_groups)
    got_t = ops.group_sums(dev(a, device), dev(b, device), dev(w, device), plan, z_axis=z_axis)
    again = ops.group_sums(dev(a, device), dev(b, device), dev(w, device), plan, z_axis=z_axis)
    assert torch.equal(got_t, again), "two runs of the same call differ"
    got = got_t.cpu().numpy()
    a3 = a if a.ndim == 3 else a.reshape(group_id.shape[0], 1, group_id.shape[1])
    b3 = None if b is None else b.reshape(a3.shape)
    want, abs_sums, n = ref.group_sums(a3, b3, w, group_id, n_groups)
    assert got.shape == want.shape == (10, n_groups, a3.shape[1])
    np.testing.assert_array_equal(plan.counts, n)
    finite = np.isfinite(want)
    np.testing.assert_array_equal(got[~finite], want[~finite])
    bound = 2.0 * n[None, :, None] * 2.0 ** -53 * abs_sums
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)   # (inf - inf where an infinity is wanted: checked exactly above)
    worst = np.max(np.where(finite, err / np.maximum(bound, 1e-300), 0.0))
    print(f"group_sums: worst error / bound = {worst:.3g} over {finite.sum()} sums")
    assert np.all(err[finite] <= bound[finite]), (np.argwhere(finite & ~(err <= bound))[:5], worst)
    if b is None:
        assert not got[4:].any()
    return got


def fields(rng, shape, dtype, w_dtype, with_b=True, with_w=True):
    a = rng.normal(1.0, 2.0, shape).astype(dtype)
    b = rng.normal(1.0, 2.0, shape).astype(dtype) if with_b else None
    w = rng.uniform(0.5, 1.5, (shape[0], shape[2])).astype(w_dtype) if with_w else None
    return a, b, w


def latitude_groups(rng, n_batch, n_inner):
    """2-degree bins with about 38 cells each at 6 x 24 x 24; bin 40 is empty, and a few cells are in no bin."""
    lat = rng.uniform(-90, 90, (n_batch, n_inner))
    lat[(lat > -10) & (lat <= -8)] += 2.0   # empties bin 40, in the middle
    lat[0, :3] = [-90.0, np.nan, 91.0]       # in no group
    return select.bin_index(lat, np.arange(-90, 91, 2)).astype(np.int32)


@pytest.mark.parametrize("nz", [1, 5])
@pytest.mark.parametrize("dtypes", [("f32", "f64"), ("f64", "f32")])
def test_group_sums_latitude_bins(device, nz, dtypes):
    rng = np.random.default_rng(nz)
    gid = latitude_groups(rng, 6, 24 * 24)
    assert (gid == 40).sum() == 0 and (gid < 0).sum() >= 3
    a, b, w = fields(rng, (6, nz, 24 * 24), NP_DTYPE[dtypes[0]], NP_DTYPE[dtypes[1]])
    got = check_group_sums(device, a, b, w, gid, 90)
    assert not got[:, 40].any()


@pytest.mark.parametrize("dtypes", [("f32", "f64"), ("f64", "f32")])
def test_group_sums_one_group_of_all_cells(device, dtypes):
    rng = np.random.default_rng(7)
    n = 6 * 48 * 48
    a, b, w = fields(rng, (1, 2, n), NP_DTYPE[dtypes[0]], NP_DTYPE[dtypes[1]])
    check_group_sums(device, a, b, w, np.zeros((1, n), dtype=np.int64), 1)
    # no level axis, no weights, no b
    check_group_sums(device, a[:, 0], None, None, np.zeros((1, n), dtype=np.int32), 1, z_axis=None)


@pytest.mark.parametrize("dtypes", [("f32", "f64"), ("f64", "f32")])
def test_group_sums_group_sizes_around_the_chunk(device, dtypes):
    chunk = ops.group_sums_chunk()
    sizes = [1, chunk - 1, chunk, 0, chunk + 1, 2 * chunk + 1]   # an empty group in the middle
    n = 6 * 48 * 48
    assert sum(sizes) < n
    rng = np.random.default_rng(11)
    gid = np.concatenate([np.full(s, g) for g, s in enumerate(sizes)] + [np.full(n - sum(sizes), -1)])
    gid[-5:] = len(sizes)   # an id past the last group: in no group either
    gid = rng.permutation(gid).reshape(6, -1).astype(np.int32)
    a, b, w = fields(rng, (6, 3, n // 6), NP_DTYPE[dtypes[0]], NP_DTYPE[dtypes[1]])
    plan = ops.group_plan(dev(gid, device), len(sizes))
    assert plan.counts.tolist() == sizes and plan.n_items == 1 + 1 + 1 + 0 + 2 + 3
    got = check_group_sums(device, a, b, w, gid, len(sizes))
    assert not got[:, 3].any()
    check_group_sums(device, a, None, w, gid, len(sizes))
    check_group_sums(device, a, b, None, gid, len(sizes))


@pytest.mark.parametrize("case", ["nan_in_a", "nan_in_b", "nan_in_w", "group_all_nan", "one_inf"])
def test_group_sums_non_finite_data(device, case):
    rng = np.random.default_rng(5)
    gid = latitude_groups(rng, 6, 24 * 24)
    a, b, w = fields(rng, (6, 5, 24 * 24), np.float32, np.float64)
    hit = rng.uniform(size=a.shape) < 0.1
    if case == "nan_in_a":
        a[hit] = np.nan
    elif case == "nan_in_b":
        b[hit] = np.nan
    elif case == "nan_in_w":
        w[hit[:, 0]] = np.nan
    elif case == "group_all_nan":
        a[np.broadcast_to((gid == 17)[:, None, :], a.shape)] = np.nan
    else:
        cell = np.argwhere(gid == 23)[0]
        a[cell[0], 2, cell[1]] = np.inf
    got = check_group_sums(device, a, b, w, gid, 90)
    if case == "group_all_nan":
        assert (got[0, 17] > 0).all() and not got[1:4, 17].any() and not got[7:, 17].any()
        with np.errstate(invalid="ignore"):
            assert np.isnan(got[2, 17] / got[1, 17]).all()   # the mean of an all-NaN group is NaN, its sums are 0
        assert got[5, 17].all()   # (b is whole)
    if case == "one_inf":
        assert got[2, 23, 2] == np.inf and got[3, 23, 2] == np.inf and got[8, 23, 2] == np.inf and np.isfinite(got[5, 23, 2])
        assert np.isfinite(got[:, 23, 1]).all()


# ---------------------------------------------------------------------------------------------------------------------
# histograms: np.array_equal to numpy
# ---------------------------------------------------------------------------------------------------------------------
def histogram_data(rng, n, edges, dtype=np.float32):
    lo, hi = edges[0], edges[-1]
    x = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), n).astype(dtype)
    special = np.concatenate([edges.astype(dtype), [np.nan, np.inf, -np.inf, lo, hi, np.nextafter(dtype(hi), dtype(np.inf)),
                                                    np.nextafter(dtype(lo), dtype(-np.inf))]]).astype(dtype)
    k = min(n, len(special))
    where = rng.choice(n, size=k, replace=False)
    x[where] = rng.permutation(special)[:k]
    return x


@pytest.mark.parametrize("n", [1, 63, 64, 100003])
@pytest.mark.parametrize("bins", ["total_precip_to_surface", "water_vapor_path", "column_integrated_q2"])
def test_histogram_equals_numpy(device, n, bins):
    edges = ref.HISTOGRAM_BINS[bins]   # one log-spaced, two linear
    rng = np.random.default_rng(n)
    for dtype in (np.float32, np.float64):
        x = histogram_data(rng, n, edges, dtype)
        got = ops.histogram_counts(dev(x, device), dev(edges, device)).cpu().numpy()
        assert got.dtype == np.int64
        assert np.array_equal(got, np.histogram(x, bins=edges)[0])
    x = histogram_data(rng, n, edges)
    for value in (edges[0], edges[-1], edges[3], np.nan, np.inf):   # n = 1: each kind of value on its own
        x[0] = value
        got = ops.histogram_counts(dev(x, device), dev(edges, device)).cpu().numpy()
        assert np.array_equal(got, np.histogram(x, bins=edges)[0])
    count, width = hist.histogram(DataArray(dev(x, device), dims=["sample"], name=bins, attrs={"units": "mm"}), bins=edges, density=True)
    if np.histogram(x, bins=edges)[0].sum() > 0:
        assert np.array_equal(count.values, np.histogram(x, bins=edges, density=True)[0])   # bit-equal
    assert np.array_equal(width.values, np.diff(edges)) and width.attrs == {"units": "mm"}


@pytest.mark.parametrize("n", [1, 63, 64, 100003])
def test_histogram2d_equals_numpy(device, n):
    xe, ye = ref.HISTOGRAM_BINS["water_vapor_path"], ref.HISTOGRAM_BINS["minus_column_integrated_q2"]   # 100 x 100 bins
    rng = np.random.default_rng(n)
    x, y = histogram_data(rng, n, xe), histogram_data(rng, n, ye)
    got = ops.histogram2d_counts(dev(x, device), dev(y, device), dev(xe, device), dev(ye, device)).cpu().numpy()
    assert got.shape == (100, 100) and got.dtype == np.int64
    assert np.array_equal(got, np.histogram2d(x, y, bins=[xe, ye])[0])
    # log-spaced against linear, float64 against float32 data
    le = ref.HISTOGRAM_BINS["total_precip_to_surface"]
    z = histogram_data(rng, n, le, np.float64)
    got = ops.histogram2d_counts(dev(z, device), dev(y, device), dev(le, device), dev(ye, device)).cpu().numpy()
    assert np.array_equal(got, np.histogram2d(z, y.astype(np.float64), bins=[le, ye])[0])


def test_histogram_limits(device):
    x = torch.zeros(8, device=device)
    assert ops.histogram_counts(x, torch.linspace(-1, 1, 4097, dtype=torch.float64, device=device)).sum().item() == 8
    with pytest.raises(ValueError, match="4096"):
        ops.histogram_counts(x, torch.linspace(-1, 1, 4098, dtype=torch.float64, device=device))
    e128, e129 = (torch.linspace(-1, 1, k + 1, dtype=torch.float64, device=device) for k in (128, 129))
    assert ops.histogram2d_counts(x, x, e128, e128).sum().item() == 8
    with pytest.raises(ValueError, match="128"):
        ops.histogram2d_counts(x, x, e128, e129)


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def run_offline(device, inp, n_tile=6, n=12, splits=((0, 2), (2, 3))):
    import datetime

    horizontal = ["tile", "y", "x"]
    cube = lambda v: np.asarray(v).reshape(v.shape[:-1] + (n_tile, n, n))  # noqa: E731
    grid = Dataset({k: DataArray(cube(inp[k]), dims=horizontal) for k in ("lat", "lon", "area", "land_sea_mask")})
    diags = OfflineDiagnostics(grid, horizontal_dims=("x", "y", "tile"), vertical_dim="z")
    times = [datetime.datetime(2016, 8, 1) + datetime.timedelta(hours=float(h)) for h in inp["hours"]]

    def dataset(arrays, lo, hi):
        return Dataset({k: DataArray(dev(cube(v[lo:hi]), device), dims=["time"] + (["z"] if v.ndim == 3 else []) + horizontal)
                        for k, v in arrays.items()}, coords={"time": times[lo:hi]})

    for lo, hi in splits:
        delp = DataArray(dev(cube(inp["delp"][lo:hi]), device), dims=["time", "z"] + horizontal)
        diags.update(dataset(inp["prediction"], lo, hi), dataset(inp["target"], lo, hi), delp)
    return diags.compute()


def compare_with_checker(out, want):
    local_time = want.pop("local_time")
    assert set(out) == set(want), set(out) ^ set(want)
    worst = 0.0
    for name, w in want.items():
        g = out[name].values
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"{name}: NaN patterns differ"
        ok = ~np.isnan(w)
        if "hist" in name:
            assert np.array_equal(g, w), name
            continue
        diff = np.abs(g[ok] - w[ok])
        rel = (diff / np.maximum(np.abs(w[ok]), 1e-300)).max(initial=0.0)
        worst = max(worst, rel)
        assert np.all(diff <= 1e-9 * np.abs(w[ok])), (name, rel)
        if "diurnal_cycle" in name:
            np.testing.assert_array_equal(out[name].coords["local_time"], local_time)
    print(f"end to end: worst relative error {worst:.3g} over {len(want)} outputs")


@pytest.mark.parametrize("mixed_sign_q2", [False, True])
def test_offline_diagnostics_end_to_end(device, mixed_sign_q2):
    """C12, 5 levels, 3 time steps fed in two updates, a land / sea / ice mask, delp given: every output against the checker
    run on the whole stack at once, at 1e-9 relative, with identical NaN patterns.  Targets are drawn from U(0.5, 1.5) (mean
    square / variance about 13: tests/test_host_diagnostics.py checks that the moment form of the variance then stays
    within the gate; one cell of the 864 carries about 1e-3 of a mean, so a dropped cell moves a result by 1e-4 or more); with
    ``mixed_sign_q2`` the target Q2 changes sign from column to column, which populates both
    net-precipitation domains (mean square / variance about 1)."""
    inp = ref.e2e_inputs(mixed_sign_q2=mixed_sign_q2)
    out = run_offline(device, inp)
    want = ref.offline_diagnostics(**inp)
    compare_with_checker({k: out[k] for k in out}, want)
    assert out["dq1_time_domain_mean_pressure_level_zonal_avg_land"].dims == ("derivation", "pressure", "latitude")
    assert out["dq1_mse_model_level_sea"].dims == ("z",) and out["net_heating_mse_2d_global"].dims == ()
    positive = out["dq1_time_domain_mean_model_level_positive_net_precipitation"].values
    assert np.isnan(positive).all() != mixed_sign_q2
