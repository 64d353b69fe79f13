"""Random-forest training on the MI355X (csrc/forest_train.hip through ``forest_train.ForestTrainer`` and
``fit.train_random_forest``) against sklearn's ``RandomForestRegressor`` with the same hyperparameters and ``random_state`` and
against the numpy restatement ``forest_train_np``: tree by tree the same node count, the same partition of the in-bag samples
into leaves (the leaf ids from the device predictor's ``ForestModel.apply``), the same multiset of node sizes, leaf values and
impurities within ``4 n 2^-53 max|y|``.  Node-for-node equality is asked only where nothing can tie (one feature) or the tie rule
decides (two identical columns: the lower index)."""
import numpy as np
import pytest
import torch

sklearn_ensemble = pytest.importorskip("sklearn.ensemble")

import forest_train_cases as C  # noqa: E402
import forest_train_np as T  # noqa: E402
from fv3net_amd import fit, forest_train  # noqa: E402
from fv3net_amd.forest import TREE_STATS, ForestInput, ForestModel, ForestOutput, ForestSpec  # noqa: E402
from fv3net_amd.xr_compat import DataArray, Dataset  # noqa: E402

pytestmark = pytest.mark.gpu


def _bound(n, y):
    return 4 * n * 2.0 ** -53 * np.abs(y).max()


def _leaves_on_device(arrays, X, n_out, device):
    spec = ForestSpec([ForestInput("x", X.shape[1])], [ForestOutput("y", n_out)], arrays, np.zeros(n_out), np.ones(n_out))
    xt = torch.from_numpy(np.ascontiguousarray(X.T)).to(device)
    return ForestModel(spec, device=device).apply({"x": xt}).cpu().numpy()   # [tree, sample]


def _compare(X, y, n_trees, seed, params, device, against_sklearn=True):
    """Grow on the device; check every tree against sklearn's and the restatement's."""
    n, O = X.shape[0], y.shape[1]
    forest = sklearn_ensemble.RandomForestRegressor(n_estimators=n_trees, random_state=seed, **params)
    forest.fit(X, y if O > 1 else y[:, 0])
    restated = T.grow_forest(X, y, n_trees, random_state=seed, **params)
    grown = forest_train.grow_forest(X, y, n_estimators=n_trees, random_state=seed, device=device, **params)
    arrays = forest_train.forest_arrays(grown)
    leaves = _leaves_on_device(arrays, X, O, device)
    bound = _bound(n, y)
    for t, (est, (w, ref), got) in enumerate(zip(forest.estimators_, restated, grown)):
        inbag = np.flatnonzero(w > 0)
        np.testing.assert_array_equal(w, np.bincount(forest.estimators_samples_[t], minlength=n))
        mine = leaves[t]
        assert (got["children_left"][mine] == -1).all()
        references = [("restatement", ref["feature"].shape[0], ref["leaf_of_sample"][inbag], ref["value"], ref["impurity"],
                       ref["n_node_samples"], ref["weighted_n_node_samples"])]
        if against_sklearn:
            sk = est.tree_
            references.append(("sklearn", sk.node_count, est.apply(X[inbag]), sk.value[:, :, 0], sk.impurity, sk.n_node_samples,
                               sk.weighted_n_node_samples))
        for name, node_count, leaf, value, impurity, n_node, weighted_n in references:
            assert got["feature"].shape[0] == node_count, f"tree {t}: node count, {name}"
            assert T.leaf_partition(mine[inbag]) == T.leaf_partition(leaf), f"tree {t}: the leaf partition differs from {name}'s"
            np.testing.assert_array_equal(np.sort(got["n_node_samples"]), np.sort(n_node))
            np.testing.assert_array_equal(np.sort(got["weighted_n_node_samples"]), np.sort(weighted_n))
            err_v = np.abs(got["value"][mine[inbag]] - value[leaf]).max()
            err_i = np.abs(got["impurity"][mine[inbag]] - impurity[leaf]).max()
            print(f"tree {t} against {name}: {node_count} nodes, leaf value error {err_v:.2e}, impurity error {err_i:.2e}, bound {bound:.2e}")
            assert max(err_v, err_i) <= bound
    return forest, restated, grown, arrays


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_trees_match_sklearn_and_the_restatement(device, case):
    X, y = C.data(case)
    _compare(X, y, case.n_trees, case.seed, case.params(), device)


# ---- edges ---------------------------------------------------------------------------------------------------------
def _edge_data(n, F, O, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)).astype(np.float32)
    y = np.tanh(X.astype(np.float64) @ rng.normal(size=(F, O))) + 0.1 * rng.normal(size=(n, O))
    return X, y


def test_a_constant_feature_is_never_split_on(device):
    X, y = _edge_data(200, 4, 2, 20)
    X[:, 1] = 1.5
    _, _, grown, _ = _compare(X, y, 2, 20, dict(max_depth=5), device)
    for tree in grown:
        assert (tree["feature"] != 1).all()


def test_all_features_constant_makes_the_root_a_leaf(device):
    X, y = _edge_data(100, 3, 2, 21)
    X[:] = np.float32(0.25)
    _, _, grown, _ = _compare(X, y, 2, 21, {}, device)
    for tree in grown:
        assert tree["feature"].tolist() == [-2] and tree["children_left"].tolist() == [-1]


def test_negative_and_positive_zero_are_one_value(device):
    """A column of -0.0, +0.0 and a few other values: the zeros of either sign sort together (ties by sample index), no cut
    falls between them, and the partition is sklearn's."""
    X, y = _edge_data(200, 3, 2, 25)
    rng = np.random.default_rng(25)
    X[:, 1] = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), size=200)
    y[:, 0] += np.where(X[:, 1] == 0, 0.0, 2.0 * X[:, 1])
    zeros = X[:, 1] == 0
    assert np.signbit(X[zeros, 1]).sum() >= 20 and (~np.signbit(X[zeros, 1])).sum() >= 20
    _, _, grown, arrays = _compare(X, y, 2, 25, dict(max_depth=5), device)
    leaves = _leaves_on_device(arrays, X, 2, device)
    for t, tree in enumerate(grown):
        on_zeros = tree["feature"] == 1
        assert on_zeros.any() and (np.abs(tree["threshold"][on_zeros]) == 0.5).all()
        # a sample reaches the same leaf whichever sign its zero has
        flipped = X.copy()
        flipped[zeros, 1] = -flipped[zeros, 1]
        np.testing.assert_array_equal(_leaves_on_device(arrays, flipped, 2, device)[t], leaves[t])


def test_a_node_with_a_constant_target_is_a_leaf(device):
    """Integer targets: the sums are exact, so a pure node has impurity exactly 0 <= DBL_EPSILON here and in sklearn."""
    X, _ = _edge_data(300, 3, 1, 22)
    y = np.stack([(X[:, 0] > 0.1).astype(np.float64), 2.0 * (X[:, 0] > 0.1)], axis=1)
    _, _, grown, _ = _compare(X, y, 2, 22, {}, device)
    for tree in grown:
        assert tree["feature"].tolist() == [0, -2, -2]
        assert (tree["impurity"][1:] == 0.0).all()


def test_values_5e_8_apart_are_not_split(device):
    """0.1 and 0.1 + 5e-8 are distinct float32 values within the splitter's 1e-7: the best cut, between them, is not admissible
    and the next best is taken.  The reference here is the restatement alone: sklearn's source states the rule
    (``FEATURE_THRESHOLD = 1e-7``, tree/_partitioner.pxd), but the compiled sklearn 1.7.2 splitter behaves as if the constant
    were 0 and cuts between values 7e-9 apart (``DecisionTreeRegressor(max_depth=1)`` on these five points gives the threshold
    0.10000002756714821)."""
    x = np.array([0.1, 0.1 + 5e-8, 0.5, 0.9, 1.3], np.float32)
    assert x[1] > x[0] and x[1] <= x[0] + np.float32(1e-7)
    X = x[:, None]
    y = np.array([[0.0], [1.0], [1.0], [1.0], [1.0]])
    _, _, grown, _ = _compare(X, y, 1, 0, dict(bootstrap=False, max_depth=1), device, against_sklearn=False)
    assert grown[0]["threshold"][0] == np.float64(x[1]) / 2 + np.float64(x[2]) / 2
    assert grown[0]["n_node_samples"].tolist() == [5, 2, 3]


def test_identical_columns_choose_the_lower_index(device):
    """Columns 2 and 3 repeat 0 and 1: their lists, sums and proxies are the same bits, and the tie goes to the lower index."""
    X, y = _edge_data(300, 4, 2, 23)
    X[:, 3] = X[:, 1]
    X[:, 2] = X[:, 0]
    _, _, grown, _ = _compare(X, y, 2, 23, dict(max_depth=6), device)
    for tree in grown:
        assert (tree["children_left"] != -1).sum() >= 10
        assert not np.isin(tree["feature"], (2, 3)).any()


def test_one_feature_trees_equal_sklearns_node_for_node(device):
    """With one feature nothing can tie: feature, children and threshold bits are sklearn's."""
    X, y = _edge_data(300, 1, 1, 24)
    forest, restated, grown, arrays = _compare(X, y, 3, 24, dict(max_depth=4), device)
    for est, tree in zip(forest.estimators_, grown):
        sk = est.tree_
        np.testing.assert_array_equal(tree["children_left"], sk.children_left)
        np.testing.assert_array_equal(tree["children_right"], sk.children_right)
        np.testing.assert_array_equal(tree["feature"], sk.feature)
        assert tree["threshold"].dtype == np.float64
        np.testing.assert_array_equal(tree["threshold"].view(np.int64), sk.threshold.view(np.int64))
        np.testing.assert_array_equal(tree["n_node_samples"], sk.n_node_samples)
        internal = sk.children_left != -1
        np.testing.assert_array_equal(tree["missing_go_to_left"][internal], sk.missing_go_to_left[internal])


def test_growing_twice_gives_the_same_bits(device):
    case = C.CASES[8]
    X, y = C.data(case)
    trainer = forest_train.ForestTrainer(X, y, device=device)
    first = forest_train.grow_forest(X, y, n_estimators=2, random_state=3, trainer=trainer, **case.params())
    second = forest_train.grow_forest(X, y, n_estimators=2, random_state=3, trainer=trainer, **case.params())
    fresh = forest_train.grow_forest(X, y, n_estimators=2, random_state=3, device=device, **case.params())
    for a, b, c in zip(first, second, fresh):
        for k in forest_train.GROWN_ARRAYS:
            np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8))
            np.testing.assert_array_equal(a[k].view(np.uint8), c[k].view(np.uint8))


# ---- the training function ---------------------------------------------------------------------------------------------
def _batches(rng, n_batches=3, per_batch=100, nz=6):
    out = []
    for _ in range(n_batches):
        T_ = rng.normal(size=(per_batch, nz))
        q = rng.normal(size=(per_batch, nz))
        cz = rng.uniform(size=per_batch)
        dq1 = 280.0 + 5.0 * np.tanh(T_ + q[:, ::-1]) + 0.2 * rng.normal(size=(per_batch, nz))
        precip = 1e-4 * (cz + T_[:, 0] ** 2) + 1e-5 * rng.normal(size=per_batch)
        out.append(Dataset({"T": DataArray(T_, dims=("sample", "z")), "q": DataArray(q, dims=("sample", "z")),
                            "cos_zenith": DataArray(cz, dims=("sample",)), "dQ1": DataArray(dq1, dims=("sample", "z")),
                            "precip": DataArray(precip, dims=("sample",))}))
    return out


_TRAINED = dict(n_estimators=4, max_depth=7, random_state=5, min_samples_leaf=2)


def _train(bootstrap):
    rng = np.random.default_rng(30)
    batches = _batches(rng)
    hp = fit.RandomForestHyperparameters(["T", "q", "cos_zenith"], ["dQ1", "precip"], bootstrap=bootstrap,
                                         packer_config={"clip": {"q": {"start": 2, "stop": None, "step": None}}}, **_TRAINED)
    model = fit.train_random_forest(hp, batches)
    # the reference's pipeline around sklearn (SklearnWrapper.fit, _random_forest.py:232-257)
    f32 = {k: np.concatenate([np.asarray(b[k].values) for b in batches]).astype(np.float32) for k in batches[0]}
    X = np.concatenate([f32["T"], f32["q"][:, 2:], f32["cos_zenith"][:, None]], axis=1)
    y = np.concatenate([f32["dQ1"], f32["precip"][:, None]], axis=1)
    mean, std = np.mean(y, axis=0).astype(np.float64), np.std(y, axis=0).astype(np.float64) + 1e-12
    y_norm = (y - mean) / std
    forest = sklearn_ensemble.RandomForestRegressor(n_jobs=None, min_samples_split=2, max_features=1.0, bootstrap=bootstrap,
                                                    **_TRAINED).fit(X, y_norm)
    return hp, batches, model, forest, X, y_norm, mean, std


@pytest.fixture(scope="module")
def trained():
    return _train(True)


@pytest.mark.parametrize("bootstrap", [True, False])
def test_train_random_forest_predicts_like_the_reference(trained, bootstrap):
    """``predict`` on the training inputs against ``denormalize(forest.predict(X))`` of sklearn's forest.  The two forests put
    every tree's in-bag samples into the same leaves; a sample out of a tree's bag may fall elsewhere where the two trees split
    on different features of equal proxy.  So with the bootstrap the samples that are in every tree's bag are compared (and there
    must be some), without it all of them."""
    hp, batches, model, forest, X, y_norm, mean, std = trained if bootstrap else _train(False)
    assert isinstance(model, fit.RandomForest) and model.n_trees == 4 and model.n_features_in == X.shape[1]
    assert model.output_features == [6, 1]
    np.testing.assert_array_equal(model.mean, mean)
    np.testing.assert_array_equal(model.std, std)
    nz = 6
    n = X.shape[0]
    in_every_bag = np.ones(n, bool)
    for samples in forest.estimators_samples_:
        in_every_bag &= np.bincount(samples, minlength=n) > 0
    assert in_every_bag.sum() >= 20 and (bootstrap or in_every_bag.all())
    ds = Dataset({k: DataArray(np.concatenate([np.asarray(b[k].values) for b in batches]).T.reshape((nz, 1, n) if k in ("T", "q") else (1, n)),
                               dims=("z", "y", "x") if k in ("T", "q") else ("y", "x")) for k in ("T", "q", "cos_zenith")})
    got = model.predict(ds)
    want = forest.predict(X) * std + mean
    bound = _bound(n, y_norm)
    err = (np.abs(np.asarray(got["dQ1"].transpose("z", "y", "x").data).reshape(nz, n).T - want[:, :nz]) / std[:nz])[in_every_bag]
    err_p = (np.abs(np.asarray(got["precip"].data).reshape(n) - want[:, nz]) / std[nz])[in_every_bag]
    print(f"predict error over std on {in_every_bag.sum()} samples: {err.max():.2e}, {err_p.max():.2e}; bound {bound:.2e}")
    assert max(err.max(), err_p.max()) <= bound


def test_dump_load_predict_and_sensitivity(trained, tmp_path):
    hp, batches, model, forest, X, y_norm, mean, std = trained
    fit.dump(model, str(tmp_path / "rf"))
    loaded = fit.load(str(tmp_path / "rf"))
    assert isinstance(loaded, fit.RandomForest)
    for k in model.trees:
        np.testing.assert_array_equal(loaded.trees[k], model.trees[k])
    assert set(TREE_STATS) <= set(loaded.trees)
    rng = np.random.default_rng(31)
    ds = Dataset({"T": DataArray(rng.normal(size=(6, 5, 7)), dims=("z", "y", "x")), "q": DataArray(rng.normal(size=(6, 5, 7)), dims=("z", "y", "x")),
                  "cos_zenith": DataArray(rng.uniform(size=(5, 7)), dims=("y", "x"))})
    a, b = model.predict(ds), loaded.predict(ds)
    for name in ("dQ1", "precip"):
        np.testing.assert_array_equal(np.asarray(a[name].data), np.asarray(b[name].data))
    # importances of the device-grown arrays: the restatement's formula, and sklearn's numbers to the accuracy of the impurities
    sample = batches[0]
    sens = loaded.input_sensitivity(sample).rf_feature_importances
    offsets = model.trees["node_offset"]
    rows = []
    for t in range(model.n_trees):
        sl = slice(int(offsets[t]), int(offsets[t + 1]))
        rows.append(T.importances({k: model.trees[k][sl] for k in ("children_left", "children_right", "feature", "impurity",
                                                                   "weighted_n_node_samples")}, X.shape[1]))
    rows = np.stack(rows)
    flat_mean = np.concatenate([sens[k].mean_importances for k in ("T", "q", "cos_zenith")])
    flat_std = np.concatenate([sens[k].std_importances for k in ("T", "q", "cos_zenith")])
    np.testing.assert_allclose(flat_mean, rows.mean(axis=0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(flat_std, rows.std(axis=0), rtol=0, atol=1e-12)
    assert sens["T"].indices == list(range(6)) and sens["q"].indices == list(range(4)) and np.isnan(sens["cos_zenith"].indices[0])
    assert abs(flat_mean.sum() - 1.0) < 1e-12
