"""Random forest, host side: the exported arrays, walked by a numpy restatement of the device kernels, reproduce sklearn's
``apply`` and ``predict`` bit for bit; ``fv3hip_forest_create`` refuses malformed forests before touching the GPU; the
artifact round-trips, and a directory in the reference's own layout converts to the same arrays."""
import io
import os

import numpy as np
import pytest
import yaml

sklearn_ensemble = pytest.importorskip("sklearn.ensemble")
joblib = pytest.importorskip("joblib")

from fv3net_amd import _lib  # noqa: E402
from fv3net_amd.fit import RandomForest, load  # noqa: E402
from fv3net_amd.forest import ForestInput, ForestOutput, ForestSpec, create_handle, float32_floor, tree_arrays  # noqa: E402


def walk(trees, X32, threshold=None):
    """The device walk restated: leaf node id [tree, sample] (tree-local) for float32 inputs [sample, feature]."""
    off = trees["node_offset"]
    thr = trees["threshold"] if threshold is None else threshold
    n = X32.shape[0]
    leaves = np.empty((off.shape[0] - 1, n), np.int64)
    rows = np.arange(n)
    for t in range(off.shape[0] - 1):
        o = off[t]
        node = np.zeros(n, np.int64)
        while True:
            internal = trees["children_left"][o + node] != -1
            if not internal.any():
                break
            g = o + node[internal]
            x = X32[rows[internal], trees["feature"][g]]
            left = np.where(np.isnan(x), trees["missing_go_to_left"][g] == 1, x <= thr[g])
            node[internal] = np.where(left, trees["children_left"][g], trees["children_right"][g])
        leaves[t] = node
    return leaves


def forest_sum(trees, leaves):
    """y = 0; y += value_t[leaf_t] in tree order; y /= T (float64)."""
    off = trees["node_offset"]
    y = np.zeros((leaves.shape[1], trees["leaf_values"].shape[1]))
    for t in range(leaves.shape[0]):
        y += trees["leaf_values"][trees["leaf_row"][off[t] + leaves[t]]]
    return y / leaves.shape[0]


def probe_inputs(forest, X_train, rng):
    """Training values, the float32 neighbours on both sides of every threshold (in rows otherwise from the training
    set), random values, and NaNs."""
    X = [X_train.astype(np.float32)]
    for est in forest.estimators_:
        t = est.tree_
        internal = np.flatnonzero(t.children_left != -1)
        base = X_train[rng.integers(0, X_train.shape[0], internal.shape[0])].astype(np.float32)
        lo = float32_floor(t.threshold[internal])
        hi = np.nextafter(lo, np.float32(np.inf))
        for v in (lo, hi, t.threshold[internal].astype(np.float32)):
            b = base.copy()
            b[np.arange(internal.shape[0]), t.feature[internal]] = v
            X.append(b)
    r = rng.normal(0, 2, (200, X_train.shape[1])).astype(np.float32)
    r[rng.uniform(size=r.shape) < 0.2] = np.nan
    X.append(r)
    return np.concatenate(X)


def _train(n_out, max_depth, n_trees=5, seed=0, n=300, k=6, cls=None):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, k)).astype(np.float32)
    y = np.stack([np.sin(X[:, i % k] * (1 + i % 5)) + 0.1 * rng.normal(size=n) for i in range(n_out)], axis=1)
    cls = cls or sklearn_ensemble.RandomForestRegressor
    forest = cls(n_estimators=n_trees, max_depth=max_depth, random_state=seed, n_jobs=1).fit(X, y if n_out > 1 else y[:, 0])
    return forest, X


@pytest.mark.parametrize("n_out, max_depth", [(1, 13), (158, 13), (1, None), (158, None)])
def test_exported_arrays_reproduce_apply_and_predict(n_out, max_depth):
    forest, X_train = _train(n_out, max_depth)
    rng = np.random.default_rng(1)
    X = probe_inputs(forest, X_train, rng)
    trees = tree_arrays(forest)
    leaves = walk(trees, X)
    np.testing.assert_array_equal(leaves.T, forest.apply(X))
    want = forest.predict(X)
    got = forest_sum(trees, leaves)
    np.testing.assert_array_equal(got, want.reshape(got.shape))


def test_extra_trees_export():
    forest, X_train = _train(3, 8, cls=sklearn_ensemble.ExtraTreesRegressor)
    X = probe_inputs(forest, X_train, np.random.default_rng(2))
    trees = tree_arrays(forest)
    leaves = walk(trees, X)
    np.testing.assert_array_equal(leaves.T, forest.apply(X))
    np.testing.assert_array_equal(forest_sum(trees, leaves), forest.predict(X))


def test_naive_rounding_misroutes():
    forest, X_train = _train(158, 13)
    X = probe_inputs(forest, X_train, np.random.default_rng(1))
    trees = tree_arrays(forest)
    naive = np.concatenate([est.tree_.threshold.astype(np.float32) for est in forest.estimators_])
    assert not np.array_equal(naive, trees["threshold"])
    assert (walk(trees, X, threshold=naive).T != forest.apply(X)).any()
    assert (walk(trees, X).T == forest.apply(X)).all()


def test_float32_floor():
    t = np.array([0.1, -0.1, 1.0, 1e-40, np.float64(np.float32(0.3)), 3.4e38])
    r = float32_floor(t)
    assert r.dtype == np.float32
    assert (r.astype(np.float64) <= t).all()
    assert (np.nextafter(r, np.float32(np.inf)).astype(np.float64) > t).all()


def _spec(trees, k=6, n_out=1):
    return ForestSpec([ForestInput("x", k)], [ForestOutput("y", n_out)], trees, np.zeros(n_out), np.ones(n_out))


def _small_trees():
    forest, _ = _train(1, 3, n_trees=2)
    return tree_arrays(forest)


@pytest.mark.parametrize("breakage, message", [
    ("child", b"children"),
    ("feature", b"feature"),
    ("leaf_row", b"leaf row"),
    ("no_trees", b"at least one tree"),
])
def test_create_refuses_malformed_forests_without_the_gpu(breakage, message):
    trees = {k: v.copy() for k, v in _small_trees().items()}
    internal = np.flatnonzero(trees["children_left"] != -1)
    leaf = np.flatnonzero(trees["children_left"] == -1)
    if breakage == "child":
        node = internal[internal < trees["node_offset"][1]][1]  # an internal node of tree 0 below the root
        trees["children_right"][node] = node  # a child id equal to its parent's
    elif breakage == "feature":
        trees["feature"][internal[-1]] = 6
    elif breakage == "leaf_row":
        trees["leaf_row"][leaf[-1]] = trees["leaf_values"].shape[0]
    else:
        for k in ("children_left", "children_right", "feature", "threshold", "missing_go_to_left", "leaf_row"):
            trees[k] = trees[k][:0]
        trees["node_offset"] = np.zeros(1, np.int64)
    with pytest.raises(_lib.Fv3HipError) as err:
        create_handle(_spec(trees))
    assert err.value.code == _lib.EINVAL
    assert message in _lib.load().fv3hip_last_error()


def test_create_refuses_a_child_below_its_parent():
    trees = {k: v.copy() for k, v in _small_trees().items()}
    node = np.flatnonzero(trees["children_left"][:trees["node_offset"][1]] != -1)[1]
    trees["children_left"][node] = 0  # points back at the root: the walk would cycle
    with pytest.raises(_lib.Fv3HipError) as err:
        create_handle(_spec(trees))
    assert err.value.code == _lib.EINVAL


def _model(predict_columns=True, clip=None):
    forest, _ = _train(5, 6, n_trees=4, k=7)
    mean, std = np.linspace(-1, 1, 5), np.linspace(0.5, 2, 5)
    return forest, RandomForest.from_sklearn(forest, ["T", "cos_zenith"], ["dQ1", "dQ2"], [3, 2], mean, std, clip=clip,
                                             predict_columns=predict_columns)


def _assert_same(a: RandomForest, b: RandomForest):
    assert list(a.input_variables) == list(b.input_variables)
    assert list(a.output_variables) == list(b.output_variables)
    assert a.output_features == b.output_features and a.n_features_in == b.n_features_in
    assert a.clip == b.clip and a.predict_columns == b.predict_columns
    for k in a.trees:
        np.testing.assert_array_equal(a.trees[k], b.trees[k])
        assert a.trees[k].dtype == b.trees[k].dtype, k
    np.testing.assert_array_equal(a.mean, b.mean)
    np.testing.assert_array_equal(a.std, b.std)


def test_dump_load_round_trip(tmp_path):
    from fv3net_amd.fit import dump

    _, model = _model(clip={"T": {"start": 2, "stop": None}})
    dump(model, str(tmp_path / "m"))
    assert open(tmp_path / "m" / "name").read() == "sklearn"
    assert sorted(os.listdir(tmp_path / "m")) == ["forest.npz", "metadata.yaml", "name"]
    _assert_same(model, load(str(tmp_path / "m")))


def _write_reference_layout(path, forest, regressors=None, scaler=True, clip=None, predict_columns=True):
    os.makedirs(path)
    with open(os.path.join(path, "name"), "w") as f:
        f.write("sklearn")
    buf = io.BytesIO()
    joblib.dump({"regressors": forest if regressors is None else regressors, "n_jobs": 1}, buf)
    with open(os.path.join(path, "sklearn.pkl"), "wb") as f:
        f.write(buf.getvalue())
    if scaler:
        npz = io.BytesIO()
        np.savez(npz, mean=np.linspace(-1, 1, 5), std=np.linspace(0.5, 2, 5))
        with open(os.path.join(path, "scaler.bin"), "wb") as f:
            f.write(yaml.safe_dump(("standard", npz.getvalue())).encode("UTF-8"))
    meta = {"input_variables": ["T", "cos_zenith"], "output_variables": ["dQ1", "dQ2"],
            "output_features": {"names": ["dQ1", "dQ2"], "features": [3, 2]},
            "packer_config": {"clip": clip or {}}, "predict_columns": predict_columns}
    with open(os.path.join(path, "metadata.bin"), "wb") as f:
        f.write(yaml.safe_dump(meta).encode("UTF-8"))


def test_reference_layout_loads_to_the_same_arrays(tmp_path):
    clip = {"T": {"start": 2, "stop": None, "step": None}}
    forest, model = _model(clip=clip)
    _write_reference_layout(str(tmp_path / "ref"), forest, clip=clip)
    _assert_same(model, load(str(tmp_path / "ref")))
    # the legacy one-element list of batch regressors
    _write_reference_layout(str(tmp_path / "legacy"), forest, regressors=[forest], clip=clip)
    _assert_same(model, load(str(tmp_path / "legacy")))


def test_reference_layout_refusals(tmp_path, monkeypatch):
    forest, _ = _model()
    _write_reference_layout(str(tmp_path / "two"), forest, regressors=[forest, forest])
    with pytest.raises(ValueError, match="multiple batch regressors"):
        load(str(tmp_path / "two"))
    _write_reference_layout(str(tmp_path / "noscaler"), forest, scaler=False)
    with pytest.raises(ValueError, match="Target scaler not present"):
        load(str(tmp_path / "noscaler"))
    _write_reference_layout(str(tmp_path / "ok"), forest)
    monkeypatch.setitem(__import__("sys").modules, "joblib", None)  # as where sklearn / joblib are not installed
    with pytest.raises(ValueError, match="export"):
        load(str(tmp_path / "ok"))


def test_non_forest_estimators_are_refused():
    from sklearn.linear_model import LinearRegression
    from sklearn.tree import DecisionTreeRegressor

    X, y = np.random.default_rng(0).normal(size=(20, 3)), np.arange(20.0)
    for est in (LinearRegression().fit(X, y), DecisionTreeRegressor().fit(X, y)):
        with pytest.raises(NotImplementedError, match=type(est).__name__):
            RandomForest.from_sklearn(est, ["x"], ["y"], [1], np.zeros(1), np.ones(1))
