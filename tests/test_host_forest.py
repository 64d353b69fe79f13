"""Random forest, host side: the exported arrays, walked by a numpy restatement of the device kernels, reproduce sklearn's
``apply`` and ``predict`` bit for bit; ``fv3hip_forest_create`` refuses malformed forests before touching the GPU; the
artifact round-trips, and a directory in the reference's own layout converts to the same arrays."""
import io
import os
from fractions import Fraction

import numpy as np
import pytest
import yaml

sklearn_ensemble = pytest.importorskip("sklearn.ensemble")
joblib = pytest.importorskip("joblib")

from fv3net_amd import _lib  # noqa: E402
from fv3net_amd.fit import RandomForest, load  # noqa: E402
from fv3net_amd.forest import ForestInput, ForestOutput, ForestSpec, create_handle, float32_floor, tree_arrays  # noqa: E402

import forest_np  # noqa: E402
from forest_np import forest_sum, probe_inputs, walk  # noqa: E402


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


# ---- the reference and the inputs of tests/test_gpu_forest_edges.py, proved here before any kernel is involved -----
def _apply_and_predict_equal_sklearn(forest, X):
    trees = tree_arrays(forest)
    leaves = walk(trees, X)
    np.testing.assert_array_equal(leaves.T, forest.apply(X))
    forest_np.assert_same_bits(forest_sum(trees, leaves), forest_np.sklearn_predict(forest, X))
    return trees, leaves


@pytest.mark.parametrize("kind", forest_np.SKLEARN_KINDS)
def test_reference_equals_sklearn_on_every_kind_of_forest(kind):
    forest, X_train = forest_np.sklearn_forest(kind)
    thresholds = np.concatenate([e.tree_.threshold[e.tree_.children_left != -1] for e in forest.estimators_])
    counts = [e.tree_.node_count for e in forest.estimators_]
    if kind == "rf_nan_depth8":
        assert np.isposinf(thresholds).any()  # what sklearn gives a node that only splits off the missing values
    if kind == "constant_target":
        assert counts == [1] * 7
    if kind == "rf_nan_best_first":
        assert max(e.tree_.n_leaves for e in forest.estimators_) == 40 and forest.n_outputs_ == 1
    X = probe_inputs(forest, X_train, np.random.default_rng(1))
    assert np.isnan(X).any() and not np.isinf(X).any()
    trees, _ = _apply_and_predict_equal_sklearn(forest, X)
    assert trees["node_offset"].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()


@pytest.mark.parametrize("kind", forest_np.SKLEARN_KINDS)
def test_float64_probes_equal_sklearn_when_cast(kind):
    forest, X_train = forest_np.sklearn_forest(kind)
    X = forest_np.float64_probes(forest, np.nan_to_num(X_train), np.random.default_rng(2))
    assert X.dtype == np.float64
    if kind == "constant_target":
        assert X.shape[0] == 0
        return
    trees = tree_arrays(forest)
    leaves = walk(trees, X)  # rounds to float32 itself, like the kernel
    np.testing.assert_array_equal(leaves.T, forest.apply(X))  # sklearn casts float64 to float32 too
    np.testing.assert_array_equal(leaves, walk(trees, X.astype(np.float32)))
    forest_np.assert_same_bits(forest_sum(trees, leaves), forest_np.sklearn_predict(forest, X))


def test_probes_tell_each_walk_mutation_from_the_contract():
    """Every switch of ``forest_np.walk`` changes a leaf id on the inputs the GPU tests feed the kernel."""
    forest, X_train = forest_np.sklearn_forest("rf_nan_depth8")
    trees = tree_arrays(forest)
    X32 = probe_inputs(forest, X_train, np.random.default_rng(1))
    right = walk(trees, X32)
    assert (walk(trees, X32, strict=True) != right).any()
    assert (walk(trees, X32, nan_left=True) != right).any()
    assert (walk(trees, X32, nan_left=False) != right).any()
    naive = np.concatenate([est.tree_.threshold.astype(np.float32) for est in forest.estimators_])
    assert (walk(trees, X32, threshold=naive) != right).any()
    X64 = forest_np.float64_probes(forest, np.nan_to_num(X_train), np.random.default_rng(2))
    assert (walk(trees, X64, cast=False) != walk(trees, X64)).any()
    np.testing.assert_array_equal(walk(trees, X32, cast=False), right)  # (nothing to round in a float32)
    # the inputs sklearn refuses, so that forest_np is the only reference there
    for dtype in (np.float32, np.float64):
        Xu = forest_np.unrepresentable_inputs(forest, X_train, np.random.default_rng(3), dtype)
        with pytest.raises(ValueError), np.errstate(over="ignore", invalid="ignore"):
            forest.apply(Xu)
        right = walk(trees, Xu)
        assert (walk(trees, Xu, strict=True) != right).any()
        assert (walk(trees, Xu, nan_left=True) != right).any() and (walk(trees, Xu, nan_left=False) != right).any()


def test_hand_made_cases_tell_each_mutation_from_the_contract():
    # special values: <= against <, and the rounding of a float64, at zero, the subnormals and the largest float32
    assert F32_TINY_IS_KEPT
    for dtype in (np.float32, np.float64):
        trees, X = forest_np.special_value_case(dtype)
        right = walk(trees, X)
        np.testing.assert_array_equal(forest_np.walk_stumps(trees, X), right)
        assert (walk(trees, X, strict=True) != right).any()
        assert (walk(trees, X, nan_left=True) != right).any() and (walk(trees, X, nan_left=False) != right).any()
        # restated once more in Python's own floats (every float32 is one exactly)
        with np.errstate(over="ignore"):
            x32 = X.astype(np.float32)
        for t in range(right.shape[0]):
            thr, k, mgl = float(trees["threshold"][3 * t]), trees["feature"][3 * t], trees["missing_go_to_left"][3 * t]
            want = [1 if (mgl if x != x else x <= thr) else 2 for x in map(float, x32[:, k])]
            assert right[t].tolist() == want
    trees, X = forest_np.special_value_case(np.float64)
    changed = walk(trees, X, cast=False) != walk(trees, X)
    assert changed.any()
    # code packing: the missing-left bit of sources 0 and 31
    trees, X, _ = forest_np.packing_case()
    right = walk(trees, X)
    for t in range(4):
        assert (walk(trees, X, nan_left=not trees["missing_go_to_left"][3 * t])[t] != right[t]).any()
    assert not np.isnan(X[:, 1:31]).any()
    # the order of the sum
    for T in forest_np.SUM_T:
        for n_out in forest_np.SUM_N_OUT:
            trees, X, mean, std = forest_np.sum_case(T, n_out)
            leaves = forest_np.walk_stumps(trees, X)
            np.testing.assert_array_equal(leaves, walk(trees, X))
            a, b = forest_sum(trees, leaves), forest_sum(trees, leaves, reverse=True)
            assert np.isfinite(a).all()
            if T >= 7:
                assert (a != b).any(), (T, n_out)
    # y * std + mean in two roundings, not one: a contracted multiply-add would show on these values
    trees, X, mean, std = forest_np.sum_case(8, 3)
    y = forest_sum(trees, forest_np.walk_stumps(trees, X))
    fused = [[float(Fraction(v) * Fraction(s_) + Fraction(m)) for v, s_, m in zip(row, std, mean)] for row in y]
    assert (forest_np.denormalize(y, mean, std) != np.asarray(fused)).any()


F32_TINY_IS_KEPT = bool(np.float32(1e-45) > 0 and np.float32(1e-45) / np.float32(2) == 0)  # numpy does not flush subnormals


@pytest.mark.parametrize("side", ["left", "right"])
def test_chain_stops_at_every_depth(side):
    depth = 200
    rng = np.random.default_rng(4)
    trees = forest_np.chain(depth, side, 3, 2, rng)
    assert trees["node_offset"].tolist() == [0, 2 * depth + 1]
    X = forest_np.chain_inputs(depth, 3, rng)
    leaves = walk(trees, X)
    assert set(leaves[0].tolist()) == set(np.flatnonzero(trees["children_left"] == -1).tolist())  # every leaf, the deepest two too
    assert {2 * depth - 1, 2 * depth} <= set(leaves[0, :X.shape[0] // 2].tolist())


def test_concat_forests_renumbers():
    rng = np.random.default_rng(5)
    a = forest_np.stumps(3, 4, 2, rng)
    b = forest_np.single_leaf(2)
    c = forest_np.chain(5, "right", 4, 2, rng)
    f = forest_np.concat_forests(a, b, c, b)
    assert f["node_offset"].tolist() == [0, 3, 6, 9, 10, 21, 22]
    rows = f["leaf_row"][f["children_left"] == -1]
    assert rows.tolist() == list(range(f["leaf_values"].shape[0]))  # one row per leaf, in node order
    X = rng.normal(size=(50, 4)).astype(np.float32) * 3
    leaves = walk(f, X)
    parts = [walk(p, X) for p in (a, b, c, b)]
    np.testing.assert_array_equal(leaves, np.concatenate(parts))
    want = sum(forest_sum(p, l) * l.shape[0] for p, l in zip((a, b, c, b), parts))
    np.testing.assert_allclose(forest_sum(f, leaves) * 6, want, rtol=1e-12)


def test_stump_reference_equals_the_generic_walk():
    rng = np.random.default_rng(6)
    trees = forest_np.stumps(50, 4, 3, rng)
    X = rng.normal(size=(80, 4))
    X[rng.uniform(size=X.shape) < 0.2] = np.nan
    for dtype in (np.float32, np.float64):
        np.testing.assert_array_equal(forest_np.walk_stumps(trees, X.astype(dtype)), walk(trees, X.astype(dtype)))
    assert not forest_np.is_stumps(forest_np.concat_forests(trees, forest_np.single_leaf(3)))
