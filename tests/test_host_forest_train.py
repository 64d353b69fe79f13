"""The random-forest trainer without a GPU: the numpy restatement (``forest_train_np``) pinned to sklearn -- seeds, bootstrap
counts, node counts, the partition of the in-bag samples into leaves, leaf values -- importances from exported arrays, and the
host layer's validation.  Node-for-node equality with sklearn is not asked for: where two features induce the same partition of
a node, sklearn keeps the one its private random stream visits first, the restatement the lowest index."""
import numpy as np
import pytest
import torch

import forest_train_cases as C
import forest_train_np as T
from fv3net_amd import fit, forest_train
from fv3net_amd.forest import TREE_ARRAYS, TREE_STATS, tree_arrays
from fv3net_amd.xr_compat import DataArray, Dataset

sklearn_ensemble = pytest.importorskip("sklearn.ensemble")

# (n, F, O, max_depth, min_samples_leaf, feature grid, random_state); three trees each
CONFIGS = [
    (33, 4, 1, None, 1, None, 11),
    (300, 6, 3, 5, 1, None, 12),
    (500, 5, 8, 6, 3, None, 13),
    (1000, 7, 2, 13, 1, 0.125, 14),
    (2000, 5, 4, None, 3, None, 15),
]
N_TREES = 3


def _data(n, F, O, grid, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)).astype(np.float32)
    if grid:
        X = (np.round(X / grid) * grid).astype(np.float32)
    w = rng.normal(size=(F, O))
    y = np.tanh(X.astype(np.float64) @ w / np.sqrt(F)) + 0.1 * rng.normal(size=(n, O))
    return X, y


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: f"n{c[0]}")
def fitted(request):
    n, F, O, depth, leaf, grid, seed = request.param
    X, y = _data(n, F, O, grid, seed)
    forest = sklearn_ensemble.RandomForestRegressor(n_estimators=N_TREES, max_depth=depth, min_samples_leaf=leaf,
                                                    random_state=seed).fit(X, y if O > 1 else y[:, 0])
    ours = T.grow_forest(X, y, N_TREES, random_state=seed, max_depth=depth, min_samples_leaf=leaf)
    return X, y, forest, ours


def test_seeds_and_bootstrap_counts_are_sklearns(fitted):
    X, y, forest, ours = fitted
    n = X.shape[0]
    seeds = T.tree_seeds(forest.random_state, N_TREES)
    assert seeds == [est.random_state for est in forest.estimators_] == forest_train.tree_seeds(forest.random_state, N_TREES)
    for seed, samples, (w, _) in zip(seeds, forest.estimators_samples_, ours):
        np.testing.assert_array_equal(w, np.bincount(samples, minlength=n))
        np.testing.assert_array_equal(w, forest_train.bootstrap_counts(seed, n, n))


def test_restatement_partitions_like_sklearn(fitted):
    X, y, forest, ours = fitted
    n = X.shape[0]
    bound = 4 * n * 2.0 ** -53 * np.abs(y).max()
    for est, (w, tree) in zip(forest.estimators_, ours):
        inbag = np.flatnonzero(w > 0)
        assert tree["feature"].shape[0] == est.tree_.node_count
        want_leaf = est.apply(X[inbag])
        got_leaf = tree["leaf_of_sample"][inbag]
        assert (got_leaf >= 0).all()
        assert T.leaf_partition(got_leaf) == T.leaf_partition(want_leaf)
        np.testing.assert_array_equal(np.sort(tree["n_node_samples"]), np.sort(est.tree_.n_node_samples))
        err = np.abs(tree["value"][got_leaf] - est.tree_.value[want_leaf, :, 0]).max()
        print(f"n = {n}: leaf value error {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def test_pairwise_twin_partitions_alike(fitted):
    """No decision of these configurations hangs on the order of a sum."""
    X, y, forest, ours = fitted
    n, F, O, depth, leaf, grid, seed = next(c for c in CONFIGS if c[0] == X.shape[0])
    twin = T.grow_forest(X, y, N_TREES, random_state=seed, max_depth=depth, min_samples_leaf=leaf, pairwise=True)
    for (w, a), (_, b) in zip(ours, twin):
        inbag = np.flatnonzero(w > 0)
        assert T.leaf_partition(a["leaf_of_sample"][inbag]) == T.leaf_partition(b["leaf_of_sample"][inbag])


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_gpu_cases_do_not_hang_on_rounding(case):
    """The configurations of the GPU tests: the restatement, its pairwise twin and sklearn put the in-bag samples into the same
    leaves, so a GPU tree that partitions otherwise is wrong, not unlucky."""
    X, y = C.data(case)
    forest = sklearn_ensemble.RandomForestRegressor(n_estimators=case.n_trees, random_state=case.seed, **case.params())
    forest.fit(X, y if case.O > 1 else y[:, 0])
    seq = T.grow_forest(X, y, case.n_trees, random_state=case.seed, **case.params())
    twin = T.grow_forest(X, y, case.n_trees, random_state=case.seed, pairwise=True, **case.params())
    for est, (w, a), (_, b) in zip(forest.estimators_, seq, twin):
        inbag = np.flatnonzero(w > 0)
        assert a["feature"].shape[0] == b["feature"].shape[0] == est.tree_.node_count
        want = T.leaf_partition(est.apply(X[inbag]))
        assert T.leaf_partition(a["leaf_of_sample"][inbag]) == want
        assert T.leaf_partition(b["leaf_of_sample"][inbag]) == want


def test_importances_from_exported_arrays(fitted):
    X, y, forest, ours = fitted
    arrays = tree_arrays(forest)
    assert set(arrays) == set(TREE_ARRAYS) | set(TREE_STATS)
    got = forest_train.feature_importances(arrays, X.shape[1])
    want = np.stack([est.feature_importances_ for est in forest.estimators_])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got.mean(axis=0), forest.feature_importances_, rtol=0, atol=1e-12)
    for est, row in zip(forest.estimators_, got):
        t = est.tree_
        ref = T.importances({"children_left": t.children_left, "children_right": t.children_right, "feature": t.feature,
                             "weighted_n_node_samples": t.weighted_n_node_samples, "impurity": t.impurity}, X.shape[1])
        np.testing.assert_allclose(row, ref, rtol=0, atol=1e-12)


def test_depth_first_renumbering_and_forest_arrays():
    # level order: 0 -> (1, 2); 1 -> (3, 4); 2 leaf; 3 leaf; 4 -> (5, 6)
    tree = {"children_left": np.array([1, 3, -1, -1, 5, -1, -1], np.int32), "children_right": np.array([2, 4, -1, -1, 6, -1, -1], np.int32),
            "feature": np.array([0, 1, -2, -2, 0, -2, -2], np.int32), "threshold": np.array([0.5, 0.1, -2, -2, 0.3, -2, -2]),
            "missing_go_to_left": np.zeros(7, np.uint8), "value": np.arange(14.0).reshape(7, 2), "impurity": np.arange(7.0),
            "n_node_samples": np.array([8, 5, 3, 2, 3, 1, 2], np.int32), "weighted_n_node_samples": np.array([8.0, 5, 3, 2, 3, 1, 2])}
    out = forest_train.depth_first(tree)
    np.testing.assert_array_equal(out["children_left"], [1, 2, -1, 4, -1, -1, -1])
    np.testing.assert_array_equal(out["children_right"], [6, 3, -1, 5, -1, -1, -1])
    np.testing.assert_array_equal(out["impurity"], [0, 1, 3, 4, 5, 6, 2])
    arrays = forest_train.forest_arrays([out, out])
    assert set(arrays) == set(TREE_ARRAYS) | set(TREE_STATS)
    np.testing.assert_array_equal(arrays["node_offset"], [0, 7, 14])
    assert arrays["threshold"].dtype == np.float32 and arrays["leaf_values"].shape == (8, 2)
    np.testing.assert_array_equal(arrays["leaf_row"][:7], [-1, -1, 0, -1, 1, 2, 3])
    np.testing.assert_array_equal(arrays["leaf_values"][:4], out["value"][[2, 4, 5, 6]])


def test_bootstrap_sizes_and_min_samples():
    assert forest_train.n_bootstrap_samples(300, None) == 300
    assert forest_train.n_bootstrap_samples(300, 0.5) == 150
    assert forest_train.n_bootstrap_samples(300, 17) == 17
    assert forest_train.n_bootstrap_samples(3, 0.01) == 1
    with pytest.raises(ValueError):
        forest_train.n_bootstrap_samples(300, 301)
    with pytest.raises(ValueError):
        forest_train.n_bootstrap_samples(300, 1.5)
    assert forest_train.resolve_min_samples(100, 2, 1) == (2, 1)
    assert forest_train.resolve_min_samples(100, 2, 17) == (34, 17)
    assert forest_train.resolve_min_samples(100, 0.1, 0.02) == (10, 2)
    with pytest.raises(ValueError):
        forest_train.resolve_min_samples(100, 1, 1)
    for all_features in ("auto", None, 1.0, 5):
        forest_train.check_max_features(all_features, 5)
    forest_train.check_max_features(1, 1)   # one feature: the integer 1 is all of them
    for subset in ("sqrt", "log2", 0.5, 3, 1, True, np.int64(1), 5.0, False):   # (1 == True == 1.0, but only the float means all)
        with pytest.raises(NotImplementedError, match="feature-sampling stream"):
            forest_train.check_max_features(subset, 5)


def test_hyperparameter_defaults_are_the_references():
    hp = fit.RandomForestHyperparameters(["a"], ["b"])
    assert (hp.scaler_type, hp.scaler_kwargs, hp.n_jobs, hp.random_state, hp.n_estimators, hp.max_depth) == ("standard", None, 8, 0, 100, None)
    assert (hp.min_samples_split, hp.min_samples_leaf, hp.max_features, hp.max_samples, hp.bootstrap) == (2, 1, "auto", None, True)
    assert hp.clip == {} and hp.predict_columns is True
    hp = fit.RandomForestHyperparameters(["a"], ["b"], packer_config={"clip": {"a": {"start": 2, "stop": None, "step": None}}})
    assert hp.clip == {"a": {"start": 2, "stop": None, "step": None}}


def _batches(bad=None):
    rng = np.random.default_rng(0)
    out = []
    for _ in range(2):
        a, b = rng.normal(size=(20, 4)), rng.normal(size=(20, 3))
        if bad == "x":
            a[3, 1] = np.nan
        if bad == "y":
            b[5, 0] = np.inf
        out.append(Dataset({"a": DataArray(a, dims=("sample", "z")), "s": DataArray(rng.normal(size=20), dims=("sample",)),
                            "b": DataArray(b, dims=("sample", "z"))}))
    return out


def test_training_refuses_what_it_cannot_do():
    hp = fit.RandomForestHyperparameters(["a", "s"], ["b"], n_estimators=2)
    with pytest.raises(NotImplementedError, match="standard"):
        fit.train_random_forest(fit.RandomForestHyperparameters(["a"], ["b"], scaler_type="mass"), _batches())
    with pytest.raises(NotImplementedError, match="feature-sampling stream"):
        fit.train_random_forest(fit.RandomForestHyperparameters(["a"], ["b"], max_features="sqrt"), _batches())
    with pytest.raises(NotImplementedError, match="Clipping for ML outputs"):
        fit.train_random_forest(fit.RandomForestHyperparameters(["a"], ["b"], packer_config={"clip": {"b": {"start": 1}}}), _batches())
    with pytest.raises(NotImplementedError, match="feature-sampling stream"):
        fit.train_random_forest(fit.RandomForestHyperparameters(["a"], ["b"], max_features=1), _batches())
    with pytest.raises(NotImplementedError, match="has a step"):
        fit.train_random_forest(fit.RandomForestHyperparameters(["a"], ["b"], packer_config={"clip": {"a": {"start": 0, "stop": 4, "step": 2}}}),
                                _batches())
    for bad in ("x", "y"):
        with pytest.raises(ValueError, match="finite"):
            fit.train_random_forest(hp, _batches(bad))
    with pytest.raises(ValueError, match="finite"):
        forest_train.ForestTrainer(np.full((3, 2), np.nan, np.float32), np.zeros((3, 1)), device="cpu")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_training_needs_a_gpu():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit.train_random_forest(fit.RandomForestHyperparameters(["a", "s"], ["b"], n_estimators=2), _batches())


def test_input_sensitivity_of_exported_forest(tmp_path):
    rng = np.random.default_rng(3)
    X = rng.normal(size=(200, 5)).astype(np.float32)
    y = X[:, :2].astype(np.float64) * [1.0, 3.0] + 0.1 * rng.normal(size=(200, 2))
    forest = sklearn_ensemble.RandomForestRegressor(n_estimators=4, max_depth=4, random_state=0).fit(X, y)
    model = fit.RandomForest.from_sklearn(forest, ["a", "s"], ["b"], [2], np.zeros(2), np.ones(2), clip={"a": {"start": 1, "stop": 5}})
    sample = Dataset({"a": DataArray(np.zeros((3, 6)), dims=("sample", "z")), "s": DataArray(np.zeros(3), dims=("sample",))})
    sens = model.input_sensitivity(sample).rf_feature_importances
    per_tree = np.stack([est.feature_importances_ for est in forest.estimators_])
    assert list(sens) == ["a", "s"] and sens["a"].indices == [0, 1, 2, 3] and np.isnan(sens["s"].indices[0])
    np.testing.assert_allclose(sens["a"].mean_importances, per_tree.mean(axis=0)[:4], rtol=0, atol=1e-12)
    np.testing.assert_allclose(sens["s"].std_importances, per_tree.std(axis=0)[4:], rtol=0, atol=1e-12)
    # dump / load keeps the statistics; a forest without them says what is missing
    model.dump(str(tmp_path / "m"))
    again = fit.load(str(tmp_path / "m")).input_sensitivity(sample).rf_feature_importances
    assert again["a"].mean_importances == sens["a"].mean_importances
    old = fit.RandomForest(["a", "s"], ["b"], [2], {k: model.trees[k] for k in TREE_ARRAYS}, 5, np.zeros(2), np.ones(2),
                           clip=model.clip)
    with pytest.raises(NotImplementedError, match="impurity statistics"):
        old.input_sensitivity(sample)
    with pytest.raises(ValueError, match="input features"):
        model.input_sensitivity(Dataset({"a": DataArray(np.zeros((3, 4)), dims=("sample", "z")),
                                         "s": DataArray(np.zeros(3), dims=("sample",))}))
