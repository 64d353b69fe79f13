"""Random forest on the MI355X: ``fv3hip_forest_apply`` equals sklearn's ``forest.apply`` and ``RandomForest.predict``
equals the reference's ``denormalize(forest.predict(pack(X)))`` bit for bit, through every layer (``ForestModel``,
``fit.RandomForest``, ``fit.load`` of the reference's own layout, the composites)."""
import io
import os

import numpy as np
import pytest
import torch
import yaml

sklearn_ensemble = pytest.importorskip("sklearn.ensemble")
joblib = pytest.importorskip("joblib")

from fv3net_amd import fit  # noqa: E402
from fv3net_amd.forest import ForestInput, ForestModel, ForestOutput, ForestSpec, tree_arrays  # noqa: E402
from fv3net_amd.xr_compat import DataArray, Dataset  # noqa: E402

pytestmark = pytest.mark.gpu
NZ = 12


def _train(X, n_out, n_trees, max_depth, seed=0):
    rng = np.random.default_rng(seed)
    w = rng.normal(size=(X.shape[1], n_out))
    y = np.tanh(X.astype(np.float64) @ w / np.sqrt(X.shape[1])) + 0.05 * rng.normal(size=(X.shape[0], n_out))
    forest = sklearn_ensemble.RandomForestRegressor(n_estimators=n_trees, max_depth=max_depth, random_state=seed,
                                                    n_jobs=16).fit(X, y if n_out > 1 else y[:, 0])
    forest.set_params(n_jobs=None)  # predict as the reference does: threads would add the trees in any order
    return forest


def _apply_on_device(forest, X, device):
    spec = ForestSpec([ForestInput("x", X.shape[1])], [ForestOutput("y", forest.n_outputs_)], tree_arrays(forest),
                      np.zeros(forest.n_outputs_), np.ones(forest.n_outputs_))
    model = ForestModel(spec, device=device)
    xt = torch.from_numpy(np.ascontiguousarray(X.T)).to(device)
    return model, model.apply({"x": xt}).cpu().numpy(), xt


@pytest.mark.parametrize("n_trees, max_depth", [(1, 13), (3, 13), (100, 13), (1, None), (3, None), (100, None)])
def test_apply_matches_sklearn(device, n_trees, max_depth):
    rng = np.random.default_rng(n_trees)
    X = rng.normal(size=(3000, 17)).astype(np.float32)
    forest = _train(X, 4, n_trees, max_depth)
    Xq = np.concatenate([X, rng.normal(0, 1.5, (1000, 17)).astype(np.float32)])
    Xq[rng.uniform(size=Xq.shape) < 0.05] = np.nan
    _, leaves, _ = _apply_on_device(forest, Xq, device)
    np.testing.assert_array_equal(leaves.T, forest.apply(Xq))


def test_many_trees_cross_the_sample_slab(device):
    """Enough trees that the [tree][sample] leaf scratch holds fewer samples than the call: predict runs in slabs."""
    rng = np.random.default_rng(5)
    X = rng.normal(size=(400, 9)).astype(np.float32)
    forest = _train(X, 3, 3000, 3)
    Xq = rng.normal(size=(13824, 9)).astype(np.float32)
    model, leaves, xt = _apply_on_device(forest, Xq, device)
    np.testing.assert_array_equal(leaves.T, forest.apply(Xq))
    got = model.predict({"x": xt})["y"].cpu().numpy().T
    np.testing.assert_array_equal(got, forest.predict(Xq))  # (mean 0, std 1)


# ---- the predictor over datasets ---------------------------------------------------------------------------------
def _dataset(ny, nx, rng, order=("z", "y", "x"), dtype=np.float32, nan_fraction=0.0):
    def field(dims):
        sizes = {"z": NZ, "y": ny, "x": nx}
        a = rng.normal(size=[sizes[d] for d in dims]).astype(dtype)
        if nan_fraction:
            a[rng.uniform(size=a.shape) < nan_fraction] = np.nan
        return DataArray(a, dims=dims)

    return Dataset({"T": field(order), "q": field(order), "cos_zenith": field(tuple(d for d in order if d != "z"))})


def _sample_dims(ds, names, predict_columns):
    return ("y", "x") if predict_columns else tuple(d for d in ("z", "y", "x") if d in ds[names[0]].dims)


def _pack(ds, names, clip, predict_columns):
    """The reference's pack: [sample, feature], variables in order, clipped levels; with predict_columns false every
    dim is a sample dim and each variable one feature."""
    sdims = _sample_dims(ds, names, predict_columns)
    cols = []
    for name in names:
        da = ds[name]
        if predict_columns and "z" in da.dims:
            a = np.asarray(da.transpose(*sdims, "z").data)
            a = a.reshape(-1, a.shape[-1])[:, fit.novelty._slice(clip, name)]
        else:
            a = np.asarray(da.transpose(*sdims).data).reshape(-1, 1)
        cols.append(a)
    return np.concatenate(cols, axis=1)


def _expected(forest, ds, model):
    """{name: (dims, denormalize(forest.predict(pack(X))))}"""
    sdims = _sample_dims(ds, model.input_variables, model.predict_columns)
    shape = [ds[model.input_variables[0]].sizes[d] for d in sdims]
    X = _pack(ds, model.input_variables, model.clip, model.predict_columns)
    y = forest.predict(X).reshape(X.shape[0], -1)
    y = y * model.std
    y = y + model.mean
    out, col = {}, 0
    for name, nf in zip(model.output_variables, model.output_features):
        part = y[:, col:col + nf]
        out[name] = (sdims, part.reshape(shape)) if nf == 1 else (("z",) + sdims, part.T.reshape([nf] + shape))
        col += nf
    return out


def _model(rng, clip=None, predict_columns=True, n_trees=10, max_depth=13, outputs=(("dQ1", NZ), ("dQ2", NZ)),
           inputs=("T", "q", "cos_zenith")):
    train = _dataset(30, 40, rng, dtype=np.float64)
    X = _pack(train, list(inputs), clip or {}, predict_columns)
    n_out = sum(n for _, n in outputs)
    forest = _train(X.astype(np.float32), n_out, n_trees, max_depth)
    mean, std = rng.normal(size=n_out), rng.uniform(0.5, 2.0, n_out)
    model = fit.RandomForest.from_sklearn(forest, list(inputs), [o for o, _ in outputs], [n for _, n in outputs],
                                          mean, std, clip=clip, predict_columns=predict_columns)
    return forest, model


def _check(model, forest, ds):
    before = {k: np.array(ds[k].data, copy=True) for k in ds}
    got = model.predict(ds)
    for k in ds:
        np.testing.assert_array_equal(np.asarray(ds[k].data), before[k])  # X not mutated
    for name, (dims, want) in _expected(forest, ds, model).items():
        da = got[name]
        assert isinstance(da.data, np.ndarray) and da.dtype == np.float64
        assert set(da.dims) == set(dims)
        np.testing.assert_array_equal(np.asarray(da.transpose(*dims).data), want)
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("order", [("z", "y", "x"), ("y", "x", "z")])
def test_predict_matches_sklearn(dtype, order):
    rng = np.random.default_rng(0)
    forest, model = _model(rng)
    ds = _dataset(20, 30, rng, order=order, dtype=dtype)
    got = _check(model, forest, ds)
    assert got["dQ1"].dims == order
    assert got["dQ1"].sizes == {"z": NZ, "y": 20, "x": 30}


def test_predict_clipped_scalar_output_and_nans():
    rng = np.random.default_rng(1)
    forest, model = _model(rng, clip={"T": {"start": 3, "stop": 10}, "q": {"start": 2}},
                           outputs=(("dQ1", NZ), ("total_precipitation", 1)))
    _check(model, forest, _dataset(16, 17, rng, nan_fraction=0.05))


def test_predict_columns_false():
    """Every dim a sample dim (the reference's gridcell models); a single-feature output keeps the input's dims, and the
    model's packed feature count is checked (test_sklearn_wrapper.py:185-193)."""
    rng = np.random.default_rng(2)
    forest, model = _model(rng, predict_columns=False, outputs=(("dQ1", 1), ("dQ2", 1)), inputs=("T", "q"))
    ds = _dataset(18, 19, rng, order=("y", "z", "x"))
    got = _check(model, forest, Dataset({"T": ds["T"], "q": ds["q"]}))
    assert got["dQ1"].dims == ("y", "z", "x")
    model.predict_columns = True
    with pytest.raises(ValueError, match="features"):
        model.predict(Dataset({"T": ds["T"], "q": ds["q"]}))


@pytest.mark.parametrize("n", [1, 63, 65, 13824])
def test_predict_sample_counts_and_repeat(n):
    rng = np.random.default_rng(n)
    forest, model = _model(rng)
    ds = _dataset(1, n, rng)
    first = _check(model, forest, ds)
    second = model.predict(ds)
    for name in model.output_variables:
        np.testing.assert_array_equal(np.asarray(first[name].data), np.asarray(second[name].data))


def test_device_in_device_out_and_coords(device):
    rng = np.random.default_rng(4)
    forest, model = _model(rng)
    host = _dataset(6, 7, rng)
    host = Dataset({k: DataArray(host[k].data, dims=host[k].dims, coords={"x": np.arange(7.0) * 2}) for k in host})
    dev = Dataset({k: DataArray(torch.from_numpy(np.asarray(host[k].data)).to(device), dims=host[k].dims,
                                coords={"x": np.arange(7.0) * 2}) for k in host})
    got_h, got_d = model.predict(host), model.predict(dev)
    for name in model.output_variables:
        assert isinstance(got_h[name].data, np.ndarray)
        assert isinstance(got_d[name].data, torch.Tensor) and got_d[name].data.is_cuda
        np.testing.assert_array_equal(got_d[name].data.cpu().numpy(), got_h[name].data)
        np.testing.assert_array_equal(np.asarray(got_h[name].coords["x"].data), np.arange(7.0) * 2)


def test_c384_tile(device):
    """One full C384 tile (147 456 columns), 13 trees of depth 13, against sklearn."""
    rng = np.random.default_rng(6)
    forest, model = _model(rng, n_trees=13, max_depth=13)
    _check(model, forest, _dataset(384, 384, rng))


def _reference_dir(path, forest, model):
    os.makedirs(path)
    with open(os.path.join(path, "name"), "w") as f:
        f.write("sklearn")
    buf = io.BytesIO()
    joblib.dump({"regressors": forest, "n_jobs": 1}, buf)
    with open(os.path.join(path, "sklearn.pkl"), "wb") as f:
        f.write(buf.getvalue())
    npz = io.BytesIO()
    np.savez(npz, mean=model.mean, std=model.std)
    with open(os.path.join(path, "scaler.bin"), "wb") as f:
        f.write(yaml.safe_dump(("standard", npz.getvalue())).encode("UTF-8"))
    meta = {"input_variables": list(model.input_variables), "output_variables": list(model.output_variables),
            "output_features": {"names": list(model.output_variables), "features": model.output_features},
            "packer_config": {"clip": model.clip}, "predict_columns": model.predict_columns}
    with open(os.path.join(path, "metadata.bin"), "wb") as f:
        f.write(yaml.safe_dump(meta).encode("UTF-8"))


def test_load_reference_layout_predicts_like_sklearn(tmp_path):
    rng = np.random.default_rng(7)
    forest, model = _model(rng, clip={"T": {"start": 1, "stop": None, "step": None}})
    _reference_dir(str(tmp_path / "ref"), forest, model)
    loaded = fit.load(str(tmp_path / "ref"))
    assert isinstance(loaded, fit.RandomForest)
    _check(loaded, forest, _dataset(10, 11, rng))


def test_out_of_sample_and_derived_over_a_forest(tmp_path):
    rng = np.random.default_rng(8)
    forest, model = _model(rng)
    fit.dump(model, str(tmp_path / "forest"))
    train = _dataset(30, 40, rng)
    detector = fit.MinMaxNoveltyDetector.fit(["T", "q"], train)
    fit.dump(detector, str(tmp_path / "minmax"))
    os.makedirs(tmp_path / "oos")
    with open(tmp_path / "oos" / "name", "w") as f:
        f.write("out_of_sample")
    with open(tmp_path / "oos" / "out_of_sample_model.yaml", "w") as f:
        yaml.safe_dump({"base_model_path": str(tmp_path / "forest"), "novelty_detector_path": str(tmp_path / "minmax"),
                        "cutoff": 0.0}, f)
    oos = fit.load(str(tmp_path / "oos"))
    ds = _dataset(8, 9, rng)
    ds["T"] = DataArray(np.asarray(ds["T"].data) * 3.0, dims=ds["T"].dims)  # some columns out of the training range
    want = {k: v for k, (_, v) in _expected(forest, ds, model).items()}
    got = oos.predict(ds)
    score = np.asarray(got["novelty_score"].transpose("y", "x").data)
    keep = (score <= 0.0).astype(np.float64)
    assert 0 < keep.sum() < keep.size
    np.testing.assert_array_equal(np.asarray(got["dQ1"].transpose("z", "y", "x").data), want["dQ1"] * keep)

    derived = fit.DerivedModel(fit.load(str(tmp_path / "forest")), ["Q1"])
    fit.dump(derived, str(tmp_path / "derived"))
    ds["pQ1"] = DataArray(np.full((NZ, 8, 9), 0.5), dims=("z", "y", "x"))
    ds["pressure_thickness_of_atmospheric_layer"] = DataArray(np.ones((NZ, 8, 9)), dims=("z", "y", "x"))
    got = fit.load(str(tmp_path / "derived")).predict(ds)
    np.testing.assert_array_equal(np.asarray(got["Q1"].transpose("z", "y", "x").data), want["dQ1"] + 0.5)
    np.testing.assert_array_equal(np.asarray(got["dQ2"].transpose("z", "y", "x").data), want["dQ2"])
