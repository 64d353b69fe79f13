"""Reservoir computing on the MI355X against the float64 numpy/scipy restatement (tests/reservoir_np.py)."""
import json
import os

import numpy as np
import pytest
import torch

from fv3net_amd import fit
from fv3net_amd.fit.reservoir import (HybridReservoirComputingModel, Reservoir, ReservoirComputingModel,
                                      ReservoirComputingReadout, TransformerGroup)
from fv3net_amd.reservoir import (WIN_CSR, WIN_DENSE, DoNothingTransformer, RankXYDivider,
                                  ScaleSpatialConcatZTransformer, SparseMatrix)
from fv3net_amd.xr_compat import DataArray, Dataset

import reservoir_np as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reservoir")


def _tf(t):
    if t["kind"] == "do-nothing":
        return DoNothingTransformer(t["sizes"])
    return ScaleSpatialConcatZTransformer(t["center"], t["scale"], t["spatial_features"], t["num_variables"], t.get("mask"))


def package_model(m, state=None, storage=0):
    """The package's model of a restatement model (no files)."""
    nz_in = _tf(m["input"]).n_latent_dims
    divider = RankXYDivider(tuple(m["layout"]), m["overlap"], rank_extent=tuple(m["rank"]), z_feature_size=nz_in)
    S = m["w_res"][3][0]
    res = Reservoir({"state_size": S}, m["w_in"][3][1], SparseMatrix.from_csr(*m["w_in"]),
                    SparseMatrix.from_csr(*m["w_res"]), input_mask_array=m.get("input_mask"), state=state)
    readout = ReservoirComputingReadout(m["coefficients"], m["intercepts"])
    hyb = m["hybrid"] if m["hybrid"] is not None else m["input"]
    tfs = TransformerGroup(_tf(m["input"]), _tf(m["output"]), _tf(hyb))
    if m["hybrid"] is not None:
        return HybridReservoirComputingModel(["a", "b"], ["a", "b"], ["a", "b"], res, readout, divider, tfs,
                                             square_half_hidden_state=m["square"], hybrid_input_mask=m.get("hybrid_mask"),
                                             w_in_storage=storage)
    return ReservoirComputingModel(["a", "b"], ["a", "b"], res, readout, divider, tfs,
                                   square_half_hidden_state=m["square"], w_in_storage=storage)


def _inputs(rng, m, extent, dtype=np.float64, layout="plain"):
    n_var = m["n_var"] if "n_var" in m else 2
    nz = m.get("nz", 1)
    out = []
    for _ in range(n_var):
        a = rng.randn(extent[0], extent[1], nz).astype(dtype)
        if layout == "transposed":  # a (x, y, z) view of a (z, y, x) array
            a = np.ascontiguousarray(a.transpose(2, 1, 0)).transpose(2, 1, 0)
        elif layout == "strided":
            big = np.zeros((extent[0], 2 * extent[1], nz + 1), dtype)
            big[:, ::2, :nz] = a
            a = big[:, ::2, :nz]
        out.append(a)
    return out


def _ovext(m):
    return (m["rank"][0] + 2 * m["overlap"], m["rank"][1] + 2 * m["overlap"])


INCREMENT_CASES = [
    dict(in_kind="do-nothing", overlap=0, nz=1, dtype=np.float64, layout="plain", input_mask=False, storage=WIN_DENSE),
    dict(in_kind="do-nothing", overlap=2, nz=3, dtype=np.float32, layout="transposed", input_mask=True, storage=WIN_CSR),
    dict(in_kind="scale-spatial", overlap=0, nz=3, dtype=np.float64, layout="strided", input_mask=True, storage=WIN_DENSE),
    dict(in_kind="scale-spatial", overlap=2, nz=1, dtype=np.float32, layout="plain", input_mask=False, storage=WIN_CSR),
    dict(in_kind="scale-spatial", overlap=2, nz=3, dtype=np.float32, layout="transposed", input_mask=True,
         storage=WIN_DENSE),
    dict(in_kind="do-nothing", overlap=2, nz=1, dtype=np.float64, layout="strided", input_mask=False, storage=WIN_DENSE),
]


@pytest.mark.parametrize("case", INCREMENT_CASES, ids=lambda c: "-".join(str(v) for v in c.values()))
def test_increment_matches_restatement(case):
    rng = np.random.RandomState(7)
    m = R.make_model(rng, overlap=case["overlap"], nz=case["nz"], in_kind=case["in_kind"], input_mask=case["input_mask"],
                     w_in_density=0.9 if case["storage"] == WIN_CSR else 1.0, state_size=41)
    state0 = rng.uniform(-1, 1, (4, 41))
    model = package_model(m, state=state0, storage=case["storage"])
    x = _inputs(rng, m, _ovext(m), case["dtype"], case["layout"])
    before = [a.copy() for a in x]
    model.increment_state(x)
    want = R.increment(m, state0, x)
    np.testing.assert_allclose(model.get_state(), want, rtol=0, atol=1e-13)
    for a, b in zip(x, before):
        np.testing.assert_array_equal(a, b)
    # device inputs too
    model.set_state(state0)
    model.increment_state([torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in x])
    np.testing.assert_allclose(model.get_state(), want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("storage", [WIN_DENSE, WIN_CSR])
def test_chained_increments_and_synchronize(storage):
    rng = np.random.RandomState(11)
    m = R.make_model(rng, overlap=1, nz=2, state_size=64, radius=0.99, coupling=0.3)
    model = package_model(m, storage=storage)
    model.reset_state()
    state = np.zeros((4, 64))
    series = [rng.randn(100, 10, 10, 2) for _ in range(2)]
    for t in range(100):
        model.increment_state([s[t] for s in series])
        state = R.increment(m, state, [s[t] for s in series])
    np.testing.assert_allclose(model.get_state(), state, rtol=0, atol=1e-12)
    steps = [model.get_state()]
    model.synchronize([s[:5] for s in series])
    synced = model.get_state()
    model.reset_state()
    for t in range(5):
        model.increment_state([s[t] for s in series])
    np.testing.assert_array_equal(model.get_state(), synced)
    assert not np.array_equal(steps[0], synced)


PREDICT_CASES = [(h, sq, lay, hm, out) for h in (False, True) for sq in (False, True) for lay in ((1, 1), (2, 2))
                 for hm in ((False, True) if h else (False,)) for out in ("do-nothing", "scale-spatial")]


@pytest.mark.parametrize("hybrid, square, layout, hybrid_mask, out_kind", PREDICT_CASES)
def test_predict_matches_restatement(hybrid, square, layout, hybrid_mask, out_kind):
    rng = np.random.RandomState(5)
    m = R.make_model(rng, layout=layout, rank=(6, 8), overlap=1, nz=2, state_size=33, out_kind=out_kind, n_out_var=2,
                     hybrid_kind="scale-spatial" if hybrid else None, hybrid_mask=hybrid_mask, square=square)
    ns = layout[0] * layout[1]
    state = rng.uniform(-1, 1, (ns, 33))
    model = package_model(m, state=state)
    h = _inputs(rng, m, m["rank"], np.float32) if hybrid else None
    got = model.predict(h) if hybrid else model.predict()
    want = R.predict(m, state, h)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        if w.dtype == np.float64:
            np.testing.assert_allclose(g, w, rtol=0, atol=1e-12 * np.abs(w).max())
        else:
            ulp = np.spacing(np.abs(w).astype(np.float32))
            assert np.all(np.abs(g.astype(np.float64) - w) <= ulp), np.max(np.abs(g.astype(np.float64) - w) / ulp)


def test_pure_model_squares_even_subdomains():
    """square_even_terms(state, axis=0): with one subdomain every element is squared; with four, subdomains 0 and 2."""
    for layout in ((1, 1), (2, 2)):
        rng = np.random.RandomState(2)
        m = R.make_model(rng, layout=layout, state_size=8, square=True)
        state = rng.uniform(-1, 1, (layout[0] * layout[1], 8))
        sq = state.copy()
        sq[0::2] = sq[0::2] ** 2
        got = package_model(m, state=state).predict()[0]
        plain = package_model(dict(m, square=False), state=sq).predict()[0]
        np.testing.assert_array_equal(got, plain)


def _regtest_check(result, golden, names="ab"):
    for name in names:
        flat = np.asarray(result[name].values).reshape(-1)
        for got, want in zip(np.concatenate([flat[:3], flat[-3:]]), golden[name]["first"] + golden[name]["last"]):
            assert float(f"{got:.4g}") == want


@pytest.mark.parametrize("hybrid", [True, False])
def test_adapters_reproduce_regtests(tmp_path, hybrid):
    with open(os.path.join(GOLDEN, "regtest_adapter_predict.json")) as f:
        g = json.load(f)["test_adapter_predict" if hybrid else "test_nonhybrid_adapter_predict"]
    m = R.regtest_model(hybrid)
    path = R.write_reference_layout(m, str(tmp_path / "m"), name="hybrid-reservoir-adapter" if hybrid else
                                    "reservoir-adapter", fmt="csc")
    adapter = fit.load(path)
    assert adapter.is_hybrid == hybrid and adapter.input_overlap == 2
    a, b = R.regtest_data(True)
    if not hybrid:
        a, b = R.regtest_data(False)
    ds = Dataset({"a": DataArray(a, dims=["x", "y", "z"]), "b": DataArray(b, dims=["x", "y", "z"])})
    nh = 2
    inputs = ds.isel(x=slice(nh, -nh), y=slice(nh, -nh))
    adapter.reset_state()
    result = adapter.predict(inputs)
    _regtest_check(result, g)
    want = R.predict(m, np.zeros((4, 25)), [inputs["a"].values, inputs["b"].values] if hybrid else None)
    for name, w in zip("ab", want):
        assert result[name].dims == ("x", "y", "z")
        np.testing.assert_allclose(result[name].values, w, rtol=0, atol=1e-12 * np.abs(w).max())
    # dims follow the input's order; the input is not modified
    a0 = inputs["a"].values.copy()
    swapped = inputs.transpose("z", "y", "x")
    r2 = adapter.predict(swapped)
    assert r2["a"].dims == ("z", "y", "x")
    np.testing.assert_array_equal(r2["a"].values, np.transpose(result["a"].values, (2, 1, 0)))
    np.testing.assert_array_equal(inputs["a"].values, a0)
    assert swapped["a"].dims == ("z", "y", "x")


def test_adapter_squeezes_single_level_and_increments(tmp_path):
    rng = np.random.RandomState(4)
    m = R.make_model(rng, overlap=1, nz=1, in_kind="do-nothing", state_size=20)
    path = R.write_reference_layout(m, str(tmp_path / "m"), name="reservoir-adapter")
    adapter = fit.load(path)
    adapter.reset_state()
    a, b = rng.randn(10, 10), rng.randn(10, 10)
    ds = Dataset({"a": DataArray(a.T.copy(), dims=["y", "x"]), "b": DataArray(b, dims=["x", "y"])})
    adapter.increment_state(ds)
    state = R.increment(m, np.zeros((4, 20)), [a[..., None], b[..., None]])
    np.testing.assert_allclose(adapter.model.get_state(), state, rtol=0, atol=1e-13)
    out = adapter.predict(ds)
    assert out["a"].dims == ("y", "x")
    want = R.predict(m, state)[0][..., 0]
    np.testing.assert_allclose(out["a"].values, want.T, rtol=0, atol=1e-12 * np.abs(want).max())
    dev = Dataset({k: DataArray(torch.from_numpy(v.values).cuda(), dims=v.dims) for k, v in ds.items()})
    out_dev = adapter.predict(dev)
    assert isinstance(out_dev["a"].data, torch.Tensor) and out_dev["a"].data.is_cuda


def test_scale_spatial_rejects_other_extents():
    rng = np.random.RandomState(0)
    m = R.make_model(rng, overlap=0, in_kind="scale-spatial")
    model = package_model(m)
    with pytest.raises(ValueError, match="All arrays must have the same x,y,z features"):
        model.increment_state([rng.randn(12, 12, 1), rng.randn(12, 12, 1)])


@pytest.mark.parametrize("hybrid", [False, True])
def test_subdomain_models_match_full_model(hybrid):
    rng = np.random.RandomState(9)
    m = R.make_model(rng, overlap=2, nz=1, state_size=30, hybrid_kind="do-nothing" if hybrid else None, hybrid_mask=hybrid)
    model = package_model(m)
    model.reset_state()
    x = _inputs(rng, m, _ovext(m))
    model.increment_state(x)
    h = _inputs(rng, m, m["rank"]) if hybrid else None
    full = model.predict(h) if hybrid else model.predict()
    nod = RankXYDivider((2, 2), 0, rank_extent=(8, 8), z_feature_size=1)
    sub_h = RankXYDivider((2, 2), 0, rank_extent=(8, 8), z_feature_size=1)
    for i, sub in enumerate(fit.split_multi_subdomain_model(model)):
        got = sub.predict([sub_h.get_subdomain(a, i) for a in h]) if hybrid else sub.predict()
        np.testing.assert_array_equal(got[0], nod.get_subdomain(full[0], i))
        # as the reference's test drives it: reset, increment with the subdomain's own inputs
        ov = RankXYDivider((2, 2), 2, rank_extent=(8, 8), z_feature_size=1)
        sub.reset_state()
        sub.increment_state([ov.get_subdomain(a, i) for a in x])
        np.testing.assert_allclose(sub.get_state()[0], model.get_state()[i], rtol=0, atol=1e-14)


@pytest.mark.parametrize("rank, layout, state_size, n_var, hybrid", [
    ((192, 192), (4, 4), 2000, 1, False),   # a C192-sized tile at 4x4: 2304 inputs and outputs per subdomain
    ((96, 96), (8, 8), 2001, 2, True),      # 64 subdomains: two subdomain groups, odd state size
    ((14, 14), (2, 2), 1001, 3, True),      # odd output length (7 x 7 x 3)
])
def test_large_shapes_match_restatement(rank, layout, state_size, n_var, hybrid):
    rng = np.random.RandomState(13)
    m = R.make_model(rng, layout=layout, rank=rank, n_var=n_var, state_size=state_size, in_kind="scale-spatial",
                     w_res_density=0.002, hybrid_kind="do-nothing" if hybrid else None, coupling=0.05)
    m["n_var"] = n_var
    ns = layout[0] * layout[1]
    state0 = rng.uniform(-1, 1, (ns, state_size))
    model = package_model(m, state=state0)
    x = _inputs(rng, m, _ovext(m), np.float32)
    model.increment_state(x)
    state = R.increment(m, state0, x)
    np.testing.assert_allclose(model.get_state(), state, rtol=0, atol=1e-13)
    h = _inputs(rng, m, m["rank"]) if hybrid else None
    got = model.predict(h) if hybrid else model.predict()
    want = R.predict(m, state, h)
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=0, atol=1e-12 * np.abs(w).max())
