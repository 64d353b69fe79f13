"""The single-level reference of the random-forest trainer (``forest_level_np``) without a GPU: chained from ``begin`` to the end
of a tree it is ``forest_train_np.grow`` node for node and, on one feature with ``sample_weight``, sklearn's
``DecisionTreeRegressor``; and every case of ``test_gpu_forest_train_levels.py`` meets the conditions it is there for -- sums
below 2^53, ties that really tie, the segments its name claims, the gap of the real-valued case."""
import numpy as np
import pytest

import forest_level_cases as LC
import forest_level_np as L
import forest_train_cases as C
import forest_train_np as T
from fv3net_amd import forest_train

sklearn_tree = pytest.importorskip("sklearn.tree")


def _data(n, F, O, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)).astype(np.float32)
    y = np.rint(4.0 * np.tanh(X[:, :1].astype(np.float64) + 0.5 * X[:, -1:]) + rng.normal(size=(n, O))) + 0.0   # whole numbers in [-8, 8], no -0.0
    w = rng.integers(0, 4, size=n)
    w[0] = 2
    return X, y, w


@pytest.mark.parametrize("n, F, O, params", [
    (33, 3, 2, dict()),
    (300, 3, 2, dict(max_depth=6, min_samples_leaf=3, min_samples_split=8)),
    (1000, 2, 1, dict()),
], ids=["n33", "n300", "n1000"])
def test_chained_levels_are_the_restatement_node_for_node(n, F, O, params):
    X, y, w = _data(n, F, O, 40 + n)
    assert np.abs(y).max() <= 8 and L.is_whole(y)
    tree, levels = L.chain(X, y, w, **params)
    assert max(r["max_int"] for r in levels) < L.EXACT_LIMIT
    got = forest_train.depth_first(tree)
    want = T.grow(X, y, w, **params)
    assert got["feature"].shape[0] == want["feature"].shape[0] > (1 if n == 33 else 30)
    for key in ("children_left", "children_right", "feature", "n_node_samples", "missing_go_to_left"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    for key in ("threshold", "value", "impurity", "weighted_n_node_samples"):
        np.testing.assert_array_equal(got[key].view(np.int64), want[key].view(np.int64), err_msg=key)
    # the widths the levels report are the tree's
    assert sum(r["n_samples"].shape[0] for r in levels) == want["feature"].shape[0]


@pytest.mark.parametrize("n", [33, 300, 1000])
def test_chained_levels_on_one_feature_are_sklearns_tree(n):
    X, y, w = _data(n, 1, 1, 50 + n)
    tree, _ = L.chain(X, y, w)
    got = forest_train.depth_first(tree)
    inbag = w > 0
    sk = sklearn_tree.DecisionTreeRegressor(random_state=0).fit(X[inbag], y[inbag, 0], sample_weight=w[inbag].astype(np.float64)).tree_
    np.testing.assert_array_equal(got["children_left"], sk.children_left)
    np.testing.assert_array_equal(got["children_right"], sk.children_right)
    np.testing.assert_array_equal(got["threshold"].view(np.int64), sk.threshold.view(np.int64))
    np.testing.assert_array_equal(got["n_node_samples"], sk.n_node_samples)
    np.testing.assert_array_equal(got["weighted_n_node_samples"], sk.weighted_n_node_samples)


def test_layout_deals_sorted_segments():
    X, y, w = LC.int_data(50, 3, 1, 7)
    X[::5, 1] = 0.25   # ties: by sample index
    w[3] = 0
    lst, seg, node = L.layout(X, w, [7, 1, 20], first_node=4, seed=1)
    assert seg.tolist() == [0, 7, 8, 28] and sorted(node.tolist()) == [4, 5, 6] and lst.shape == (3, 28)
    assert 3 not in lst
    for k in range(3):
        members = set(lst[0, seg[k]:seg[k + 1]].tolist())
        for f in range(3):
            ids = lst[f, seg[k]:seg[k + 1]]
            assert set(ids.tolist()) == members and len(members) == seg[k + 1] - seg[k]
            keys = list(zip(X[ids, f].tolist(), ids.tolist()))
            assert keys == sorted(keys)
    assert len(set(lst[0].tolist())) == 28


@pytest.mark.parametrize("case", LC.CASES, ids=repr)
def test_level_cases_meet_their_conditions(case):
    ref = LC.reference(case.name)
    steps = ref["steps"]
    n, F = case.X.shape
    assert case.X.dtype == np.float32 and case.y.shape[0] == n and case.weight.shape == (n,)
    assert (case.weight >= (0 if case.lengths is None else 1)).all() and case.weight.max() <= 7
    assert 1 <= len(steps) <= 3
    if case.exact:
        assert L.is_whole(case.y) and np.abs(case.y).max() <= 8
        assert max(s["result"]["max_int"] for s in steps) < L.EXACT_LIMIT
    else:
        assert not L.is_whole(case.y)
    if case.lengths is not None:
        assert steps[0]["seg"].tolist() == np.concatenate([[0], np.cumsum(case.lengths)]).tolist()
        assert sorted(steps[0]["node"].tolist()) == list(range(case.first_node, case.first_node + len(case.lengths)))
    else:
        m = int(np.count_nonzero(case.weight))
        assert ref["begin"]["list"].shape == (F, m) and m >= 1
        for f in range(F):
            ids = ref["begin"]["list"][f]
            assert (case.weight[ids] > 0).all() and len(set(ids.tolist())) == m
            keys = list(zip(case.X[ids, f].tolist(), ids.tolist()))
            assert keys == sorted(keys)
    k_cap, node_cap = LC.caps(case.name)
    for s in steps:
        assert len(s["node"]) <= k_cap and s["result"]["level"][0] <= k_cap and s["result"]["level"][2] <= node_cap
    if case.check is not None:
        case.check(case, steps)


def test_the_wide_whole_tree_case_opens_more_than_1024_nodes():
    """``n4096_over_1024_open_nodes`` is there for ``ft_children_kernel``'s carry across its rounds of 1024 nodes."""
    case = next(c for c in C.CASES if c.name == "n4096_over_1024_open_nodes")
    X, y = C.data(case)
    tree = T.grow(X, y, np.ones(case.n, np.int64), **{k: v for k, v in case.params().items() if k not in ("bootstrap", "max_samples")})
    depth = np.zeros(tree["feature"].shape[0], np.int64)
    for node in range(depth.shape[0]):   # parents come before their children
        for child in (tree["children_left"][node], tree["children_right"][node]):
            if child >= 0:
                depth[child] = depth[node] + 1
    widest = int(np.bincount(depth).max())
    print(f"widest level: {widest} nodes of {depth.shape[0]}")
    assert widest > 1024
