"""Host-side logic of the offline diagnostics that needs no GPU: the ``(lo, hi]`` bin rule, the class-to-domain table against
the reference's known answers, the output names, the refusals, and that the checker's two variance formulations agree."""
import numpy as np
import pytest

import diagnostics_np as ref
from fv3net_amd import histogram as hist
from fv3net_amd.diagnostics import offline
from fv3net_amd.select import bin_index
from fv3net_amd.xr_compat import DataArray


def test_bin_edges_are_open_on_the_left_like_pandas_cut():
    values = np.array([-90.0, -89.9, -88.0, -87.99, 90.0, 91.0, np.nan])
    want = [-1, 0, 0, 1, 89, -1, -1]
    assert bin_index(values, np.arange(-90, 91, 2)).tolist() == want
    assert ref.bin_index(values, np.arange(-90, 91, 2)).tolist() == want
    assert bin_index(np.float32(values), np.arange(-90, 91, 2)).tolist() == want


# workflows/diagnostics/tests/prognostic/test_transform.py:37-120 (input_args, test_mask_area), restated as literals
MASK = np.array([[[0, 1], [0, 2]]])
AREA = np.array([[[1.0, 2.0], [3.0, 4.0]]])
LATITUDE = np.array([[[0, 0], [15, 15]]])
Q2 = np.array([[[[-0.1, 0.1], [0.1, 0.1]]], [[[-0.1, 0.1], [0.1, 0.1]]]])   # [z, tile, x, y]
DELP = np.array([[[[10000, 10000], [10000, 10000]]], [[[20000, 20000], [20000, 20000]]]])
nan = np.nan


@pytest.mark.parametrize("region, expected", [
    ("global", [[[1, 2], [3, 4]]]),
    ("land", [[[nan, 2], [nan, nan]]]),
    ("sea", [[[1, nan], [3, 4]]]),
    ("tropics", [[[1, 2], [nan, nan]]]),
    ("positive_net_precipitation", [[[1, nan], [nan, nan]]]),
    ("negative_net_precipitation", [[[nan, 2], [3, 4]]]),
])
def test_class_to_domain_table_reproduces_mask_area(region, expected):
    net = ref.net_precipitation(Q2.reshape(1, 2, 4), DELP.reshape(1, 2, 4).astype(float)).reshape(MASK.shape)
    keep = offline.region_mask(region, LATITUDE, MASK, net)
    np.testing.assert_array_equal(np.where(keep, AREA, nan), np.array(expected, dtype=float))
    np.testing.assert_array_equal(ref.mask_array(region, AREA, LATITUDE, MASK, net), np.array(expected, dtype=float))


def test_precipitation_domains_are_empty_without_q2():
    # test_transform.py:123-134
    assert not offline.region_mask("positive_net_precipitation", LATITUDE, MASK, None).any()
    assert not offline.region_mask("negative_net_precipitation", LATITUDE, MASK, None).any()
    with pytest.raises(ValueError, match="not defined"):
        offline.region_mask("mars", LATITUDE, MASK)


def test_classes_are_disjoint_and_the_domains_are_their_unions():
    masks = np.array([0, 1, 2, 7, np.nan])
    precip = np.array([1.0, -1.0, np.nan])
    cls = offline.cell_class(masks[:, None] * np.ones(3), precip[None, :] * np.ones((5, 1)))
    assert sorted(cls.ravel().tolist()) == sorted(list(range(offline.N_CLASSES)) + [9, 10, 11])  # (NaN and 7: no surface type)
    assert offline.cell_class(np.array([1.0]), np.array([0.0])).tolist() == [1 * offline.N_PRECIP + 1]  # (0 is "<= 0")
    assert set(offline.DOMAIN_CLASSES["land"]).isdisjoint(offline.DOMAIN_CLASSES["sea"])
    assert set(offline.DOMAIN_CLASSES["positive_net_precipitation"]).isdisjoint(offline.DOMAIN_CLASSES["negative_net_precipitation"])
    assert set(offline.DOMAIN_CLASSES["seaice"]) < set(offline.DOMAIN_CLASSES["sea"])
    assert set(offline.DOMAIN_CLASSES["global"]) == set(range(offline.N_CLASSES))


def test_output_names_are_the_reference_s():
    assert offline.output_name("dQ1", "mse_pressure_level_global") == "dq1_mse_pressure_level_global"
    assert offline.output_name("column_integrated_Q2", "histogram") == "column_integrated_q2_histogram"
    names = offline.DIAGNOSTIC_NAMES
    assert len(names) == len(set(names)) == 55
    assert "time_mean_global" not in names   # a per-cell running mean: left out on purpose
    for expected in ("mse_2d_sea", "variance_model_level_land", "bias_2d_zonal_avg_global", "variance_pressure_level_zonal_avg_sea",
                     "diurnal_cycle_land", "time_domain_mean_model_level_positive_net_precipitation",
                     "time_domain_mean_pressure_level_zonal_avg_global", "hist_2d", "histogram"):
        assert expected in names
    assert "bias_model_level_global" not in names and "mse_2d_positive_net_precipitation" not in names
    np.testing.assert_array_equal(offline.HISTOGRAM_BINS["water_vapor_path"], np.linspace(-10, 90, 101))
    np.testing.assert_array_equal(offline.HISTOGRAM_BINS["minus_column_integrated_q2"], np.linspace(-50, 150, 101))
    np.testing.assert_array_equal(offline.HISTOGRAM_BINS["column_integrated_q2"], np.linspace(-150, 50, 101))
    np.testing.assert_array_equal(offline.HISTOGRAM_BINS["total_precip_to_surface"], np.logspace(-1, np.log10(500), 101))


def test_histograms_take_explicit_edges_only():
    da = DataArray(np.arange(6.0), dims=["x"], name="t")
    with pytest.raises(ValueError, match="explicit"):
        hist.histogram(da, bins=10)
    with pytest.raises(ValueError, match="explicit"):
        hist.histogram(da)
    with pytest.raises(ValueError, match="range"):
        hist.histogram(da, bins=[0, 1, 2], range=(0, 2))
    with pytest.raises(ValueError, match="monotonically"):
        hist.histogram(da, bins=[0, 2, 1])
    with pytest.raises(ValueError, match="explicit"):
        hist.histogram2d(da, da, bins=10)
    with pytest.raises(ValueError, match="explicit"):
        hist.histogram2d(da, da, bins=[5, np.array([0.0, 1.0])])
    with pytest.raises(ValueError, match="range"):
        hist.histogram2d(da, da, bins=[np.array([0.0, 1.0]), np.array([0.0, 1.0])], range=[[0, 1], [0, 1]])


def test_density_is_numpy_s_expression():
    edges = np.logspace(-1, np.log10(500), 101)
    count = np.random.default_rng(0).integers(0, 1000, 100)
    np.testing.assert_array_equal(hist.density_of(count, edges), count / np.diff(edges) / count.sum())


@pytest.mark.parametrize("mixed_sign_q2", [False, True])
def test_checker_s_two_variance_formulations_agree(mixed_sign_q2):
    """The streaming code forms variances from moments; the reference from a second pass.  On the end-to-end inputs
    (mean square / variance about 13 for U(0.5, 1.5), below the cap of 20 the bound assumes; about 1 with signs mixed)
    the moment form errs by at most n 2^-53 20 = 2e-11 for n <= 1e4 cells, within the end-to-end gate of 1e-9."""
    inp = ref.e2e_inputs(mixed_sign_q2=mixed_sign_q2)
    lat, mask, area, delp = inp["lat"], inp["land_sea_mask"], inp["area"], inp["delp"]
    area_t = np.broadcast_to(area.astype(np.float64), (delp.shape[0], len(lat)))
    precip = ref.net_precipitation(inp["target"]["Q2"].astype(np.float64), delp)
    checked = 0
    for name, t in inp["target"].items():
        t = t.astype(np.float64)
        ms_over_var = np.mean(t ** 2) / np.var(t)
        assert ms_over_var < 20, (name, ms_over_var)
        fields = [t] + ([ref.interpolate_to_pressure_levels(t, delp)] if t.ndim == 3 else [])
        for field in fields:
            for d in ("global", "land", "sea"):
                w = ref.mask_array(d, area_t, lat, mask, precip)
                two_pass, moments = ref.variance_two_pass(field, w), ref.variance_moments(field, w)
                assert np.array_equal(np.isnan(two_pass), np.isnan(moments))
                ok = ~np.isnan(two_pass)
                assert np.all(np.abs(moments[ok] - two_pass[ok]) <= 1e-9 * np.abs(two_pass[ok]))
                checked += int(ok.sum())
    assert checked > 100
