"""The random forest's device kernels restated in numpy, the inputs that tell a right kernel from a nearly right one, and
hand-made forests (``TREE_ARRAYS`` dicts) that need no sklearn.  Shared by ``test_host_forest.py`` (which proves the
restatement against sklearn and that every input set discriminates) and the GPU tests (which hold the kernels to it).

``walk`` and ``forest_sum`` carry switches that restate plausible kernel errors; their defaults are the contract."""
import functools

import numpy as np

from fv3net_amd.forest import float32_floor, tree_arrays

F32_MAX = np.finfo(np.float32).max
F32_TINY = np.float32(1e-45)  # the smallest float32 subnormal


# ---- the kernels restated ----------------------------------------------------------------------------------------
def walk(trees, X, threshold=None, *, strict=False, cast=True, nan_left=None):
    """The device walk restated: leaf node id [tree, sample] (tree-local) for inputs [sample, feature], float32 or
    float64 (rounded to float32 like numpy's ``astype``, as the kernel does).

    Mutations: ``threshold`` other thresholds; ``strict`` compares ``<``; ``cast=False`` compares a float64 input as it
    is; ``nan_left`` sends every NaN left (True) or right (False) whatever ``missing_go_to_left`` says."""
    off = trees["node_offset"]
    thr = trees["threshold"] if threshold is None else threshold
    if cast:
        with np.errstate(over="ignore"):
            X = X.astype(np.float32)
    else:
        thr = thr.astype(X.dtype)
    n = X.shape[0]
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
            x = X[rows[internal], trees["feature"][g]]
            missing = trees["missing_go_to_left"][g] == 1 if nan_left is None else np.full(g.shape, nan_left)
            left = np.where(np.isnan(x), missing, x < thr[g] if strict else x <= thr[g])
            node[internal] = np.where(left, trees["children_left"][g], trees["children_right"][g])
        leaves[t] = node
    return leaves


def is_stumps(trees):
    off = trees["node_offset"]
    n = off.shape[0] - 1
    return (np.array_equal(off, 3 * np.arange(n + 1)) and (trees["children_left"].reshape(n, 3) == [1, -1, -1]).all()
            and (trees["children_right"].reshape(n, 3) == [2, -1, -1]).all())


def walk_stumps(trees, X):
    """``walk`` for a forest of ``stumps`` in one vectorised step: int32 [tree, sample]."""
    assert is_stumps(trees)
    with np.errstate(over="ignore"):
        x = X.astype(np.float32)[:, trees["feature"][0::3]].T
    left = np.where(np.isnan(x), trees["missing_go_to_left"][0::3, None] == 1, x <= trees["threshold"][0::3, None])
    return np.where(left, np.int32(1), np.int32(2))


def forest_sum(trees, leaves, *, reverse=False):
    """y = 0; y += value_t[leaf_t] in tree order; y /= T (float64).  Mutation: ``reverse`` adds the last tree first."""
    rows = trees["leaf_row"][trees["node_offset"][:-1, None] + leaves]
    values = trees["leaf_values"]
    y = np.zeros((leaves.shape[1], values.shape[1]))
    order = range(leaves.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for t in reversed(order) if reverse else order:
            y += values[rows[t]]
        return y / leaves.shape[0]


def denormalize(y, mean, std):
    """The target scaler: y * std, rounded, then + mean."""
    with np.errstate(invalid="ignore", over="ignore"):
        y = y * std
        return y + mean


def predict(trees, X, mean, std):
    leaves = walk_stumps(trees, X) if is_stumps(trees) else walk(trees, X)
    return denormalize(forest_sum(trees, leaves), mean, std)


def assert_same_bits(got, want, name=""):
    """Equal bit for bit; where ``want`` is NaN only a NaN is asked for (sign and payload of a generated NaN differ
    between processors)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and want.dtype == np.float64 and got.shape == want.shape, (name, got.shape, want.shape)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{name}: NaNs")
    np.testing.assert_array_equal(np.where(nan, 0.0, got).view(np.int64), np.where(nan, 0.0, want).view(np.int64),
                                  err_msg=f"{name}: bits")


# ---- inputs next to the thresholds of a fitted sklearn forest ------------------------------------------------------
def _finite_internal(tree):
    internal = np.flatnonzero(tree.children_left != -1)
    return internal[np.isfinite(tree.threshold[internal])]  # (a forest trained on NaNs has thresholds of +inf)


def probe_inputs(forest, X_train, rng):
    """float32: training values, the float32 neighbours on both sides of every finite threshold and the threshold
    rounded naively (in rows otherwise from the training set), random values, and NaNs."""
    X = [X_train.astype(np.float32)]
    for est in forest.estimators_:
        t = est.tree_
        nodes = _finite_internal(t)
        base = X_train[rng.integers(0, X_train.shape[0], nodes.shape[0])].astype(np.float32)
        lo = float32_floor(t.threshold[nodes])
        hi = np.nextafter(lo, np.float32(np.inf))
        for v in (lo, hi, t.threshold[nodes].astype(np.float32)):
            b = base.copy()
            b[np.arange(nodes.shape[0]), t.feature[nodes]] = v
            X.append(b)
    r = rng.normal(0, 2, (200, X_train.shape[1])).astype(np.float32)
    r[rng.uniform(size=r.shape) < 0.2] = np.nan
    X.append(r)
    return np.concatenate(X)


def float64_probes(forest, X_train, rng):
    """float64 inputs whose rounding to float32 decides the route.  With ``lo = float32_floor(t)`` and ``hi`` the next
    float32, for every finite threshold ``t``: ``t`` itself, the midpoint of ``lo`` and ``hi`` (a tie), the midpoint's two
    float64 neighbours, and the float64 just below ``hi``; in rows otherwise from the training set."""
    X = []
    for est in forest.estimators_:
        t = est.tree_
        nodes = _finite_internal(t)
        base = X_train[rng.integers(0, X_train.shape[0], nodes.shape[0])].astype(np.float64)
        thr = t.threshold[nodes]
        lo = float32_floor(thr)
        hi = np.nextafter(lo, np.float32(np.inf)).astype(np.float64)
        mid = (lo.astype(np.float64) + hi) / 2  # exact: one more bit than a float32 holds
        for v in (thr, mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf), np.nextafter(hi, -np.inf)):
            b = base.copy()
            b[np.arange(nodes.shape[0]), t.feature[nodes]] = v
            X.append(b)
    return np.concatenate(X)


SKLEARN_KINDS = ("rf_nan_depth8", "rf_nan_unbounded", "rf_nan_best_first", "extra_trees_nan", "constant_target", "rf_depth13")


@functools.lru_cache(maxsize=None)
def sklearn_forest(kind):
    """(fitted forest, X_train): 7 trees on 300 x 6 inputs; the ``*_nan`` kinds are trained on 10 % NaN."""
    from sklearn.ensemble import ExtraTreesRegressor, RandomForestRegressor

    cls, n_out, kw = {
        "rf_nan_depth8": (RandomForestRegressor, 3, dict(max_depth=8)),
        "rf_nan_unbounded": (RandomForestRegressor, 2, dict(max_depth=None)),
        "rf_nan_best_first": (RandomForestRegressor, 1, dict(max_leaf_nodes=40)),
        "extra_trees_nan": (ExtraTreesRegressor, 3, dict(max_depth=8)),
        "constant_target": (RandomForestRegressor, 2, dict(max_depth=8)),
        "rf_depth13": (RandomForestRegressor, 4, dict(max_depth=13)),
    }[kind]
    rng = np.random.default_rng(SKLEARN_KINDS.index(kind))
    X = rng.normal(size=(300, 6)).astype(np.float32)
    y = np.stack([np.sin(X[:, i % 6] * (1 + i % 5)) + 0.1 * rng.normal(size=300) for i in range(n_out)], axis=1)
    if kind == "constant_target":
        y = np.broadcast_to(np.linspace(-1.5, 2.5, n_out), y.shape).copy()
    if "_nan" in kind:
        X[rng.uniform(size=X.shape) < 0.1] = np.nan
    forest = cls(n_estimators=7, random_state=0, n_jobs=1, **kw).fit(X, y if n_out > 1 else y[:, 0])
    return forest, X


def sklearn_predict(forest, X, mean=None, std=None):
    """``forest.predict`` as [sample, n_out] float64, denormalised if a scaler is given."""
    with np.errstate(invalid="ignore"):
        y = forest.predict(X).reshape(X.shape[0], -1)
    return y if mean is None else denormalize(y, mean, std)


def unrepresentable_inputs(forest, X_train, rng, dtype):
    """Inputs sklearn refuses: rows of the training set with +-inf planted (float32), or with +-1e39 (infinite as
    float32), 1e-40 (a float32 subnormal) and 1e-46 (zero as float32) planted (float64)."""
    base = X_train[rng.integers(0, X_train.shape[0], 600)].astype(dtype)
    planted = [np.inf, -np.inf] if dtype == np.float32 else [1e39, -1e39, 1e-40, -1e-40, 1e-46, -1e-46]
    where = rng.uniform(size=base.shape) < 0.3
    base[where] = rng.choice(np.asarray(planted, dtype), size=int(where.sum()))
    return base


# ---- hand-made forests ---------------------------------------------------------------------------------------------
def wide_values(shape, rng):
    """Leaf values of both signs from 1e-300 to 1e300: sums that cancel and absorb, so the order of the trees shows."""
    exponent = rng.choice([-300.0, -100.0, 0.0, 100.0, 300.0], size=shape)
    return rng.choice([-1.0, 1.0], size=shape) * rng.uniform(1.0, 2.0, size=shape) * 10.0 ** exponent


def _forest(trees_nodes, leaf_values):
    """TREE_ARRAYS from per-tree (children_left, children_right, feature, threshold, missing_go_to_left); the leaves'
    rows are numbered in node order, tree after tree."""
    out = {k: [] for k in ("children_left", "children_right", "feature", "threshold", "missing_go_to_left", "leaf_row")}
    offsets, n_rows = [0], 0
    for cl, cr, feat, thr, mgl in trees_nodes:
        cl = np.asarray(cl, np.int32)
        leaf = cl == -1
        rows = np.full(cl.shape, -1, np.int32)
        rows[leaf] = n_rows + np.arange(int(leaf.sum()), dtype=np.int32)
        n_rows += int(leaf.sum())
        offsets.append(offsets[-1] + cl.shape[0])
        for k, v, dt in (("children_left", cl, np.int32), ("children_right", cr, np.int32), ("feature", feat, np.int32),
                         ("threshold", thr, np.float32), ("missing_go_to_left", mgl, np.uint8), ("leaf_row", rows, np.int32)):
            out[k].append(np.asarray(v, dt))
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["node_offset"] = np.asarray(offsets, np.int64)
    leaf_values = np.ascontiguousarray(leaf_values, np.float64)
    assert leaf_values.shape[0] == n_rows
    out["leaf_values"] = leaf_values
    return out


def stumps(T, n_features, n_out, rng, values=None, feature=None, threshold=None, missing=None):
    """``T`` trees of one split and two leaves (local ids 1 and 2); random unless given."""
    feature = rng.integers(0, n_features, T) if feature is None else np.asarray(feature)
    threshold = rng.normal(size=T).astype(np.float32) if threshold is None else np.asarray(threshold, np.float32)
    missing = rng.integers(0, 2, T) if missing is None else np.asarray(missing)
    z = np.zeros(T)
    return {
        "node_offset": 3 * np.arange(T + 1, dtype=np.int64),
        "children_left": np.tile(np.asarray([1, -1, -1], np.int32), T),
        "children_right": np.tile(np.asarray([2, -1, -1], np.int32), T),
        "feature": np.stack([feature, z - 2, z - 2], 1).astype(np.int32).ravel(),
        "threshold": np.stack([threshold, z - 2, z - 2], 1).astype(np.float32).ravel(),
        "missing_go_to_left": np.stack([missing, z, z], 1).astype(np.uint8).ravel(),
        "leaf_row": np.stack([z - 1, 2 * np.arange(T), 2 * np.arange(T) + 1], 1).astype(np.int32).ravel(),
        "leaf_values": np.ascontiguousarray(rng.normal(size=(2 * T, n_out)) if values is None else values, np.float64),
    }


def chain(depth, side, n_features, n_out, rng, values=None):
    """One tree of ``2 * depth + 1`` nodes: internal node ``2d`` (level ``d``) has the leaf ``2d + 1`` and, on its
    ``side``, the next internal node ``2d + 2``; the last one has two leaves, at exactly ``depth``.  Level ``d`` splits
    feature ``d % n_features`` at ``depth - d`` ("left": smaller inputs walk on) or at ``d`` ("right")."""
    n = 2 * depth + 1
    cl, cr = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    d = np.arange(depth)
    (cl if side == "left" else cr)[2 * d] = 2 * d + 2
    (cr if side == "left" else cl)[2 * d] = 2 * d + 1
    feat, thr = np.full(n, -2, np.int32), np.full(n, -2, np.float32)
    feat[2 * d] = d % n_features
    thr[2 * d] = depth - d if side == "left" else d
    mgl = np.zeros(n, np.uint8)
    mgl[2 * d] = rng.integers(0, 2, depth)
    return _forest([(cl, cr, feat, thr, mgl)], rng.normal(size=(depth + 1, n_out)) if values is None else values)


def chain_inputs(depth, n_features, rng):
    """float32 rows, all features equal, that leave a ``chain`` at every level (whole and half numbers from -1 to
    depth + 1), then the same rows with NaNs."""
    x = np.arange(-2, 2 * depth + 3, dtype=np.float32) / 2
    X = np.repeat(x[:, None], n_features, 1)
    Xn = X.copy()
    Xn[rng.uniform(size=X.shape) < 0.3] = np.nan
    return np.concatenate([X, Xn])


def single_leaf(n_out, value=None):
    """One tree that is one leaf (sklearn's ``node_count == 1`` for a constant target)."""
    value = np.linspace(-1.0, 1.0, n_out) if value is None else value
    return _forest([([-1], [-1], [-2], [-2.0], [0])], np.asarray(value, np.float64).reshape(1, n_out))


def concat_forests(*forests):
    """The trees of several forests as one: ``node_offset`` and ``leaf_row`` renumbered."""
    out = {k: np.concatenate([f[k] for f in forests]) for k in
           ("children_left", "children_right", "feature", "threshold", "missing_go_to_left", "leaf_values")}
    offsets, rows, n_nodes, n_rows = [np.zeros(1, np.int64)], [], 0, 0
    for f in forests:
        offsets.append(f["node_offset"][1:] + n_nodes)
        rows.append(np.where(f["leaf_row"] >= 0, f["leaf_row"] + n_rows, -1).astype(np.int32))
        n_nodes += int(f["node_offset"][-1])
        n_rows += f["leaf_values"].shape[0]
    out["node_offset"] = np.concatenate(offsets)
    out["leaf_row"] = np.concatenate(rows)
    return out


# ---- the hand-made cases of the GPU tests (built here so the host tests can show that they discriminate) ------------
SUM_T = (1, 7, 8, 9, 16, 17)
SUM_N_OUT = (1, 2, 3)


def sum_case(T, n_out):
    """(trees, X float32 [300, 4], mean, std): stumps with ``wide_values`` and a scaler that rounds twice."""
    rng = np.random.default_rng(100 * T + n_out)
    values = wide_values((2 * T, n_out), rng)
    if T >= 3:  # small + big - big: the small one survives only if it is added last
        values[0:2] = rng.normal(size=(2, n_out))
        values[2:4] = 1e300 * rng.uniform(1.0, 2.0, n_out)
        values[4:6] = -values[2:4]
    trees = stumps(T, 4, n_out, rng, values=values)
    X = rng.normal(size=(300, 4)).astype(np.float32)
    X[rng.uniform(size=X.shape) < 0.1] = np.nan
    return trees, X, rng.normal(size=n_out), rng.uniform(0.5, 2.0, n_out)


SPECIAL_THRESHOLDS = np.asarray([np.inf, 0.0, -0.0, F32_TINY, 1e-40, F32_MAX, -F32_MAX], np.float32)


def special_value_case(dtype):
    """(trees, X [sample, 2]): one stump per special threshold, per feature and per ``missing_go_to_left``; inputs are each
    threshold and its two float32 neighbours, +-0, NaN and +-inf, in every pair; as float64 also values that only become
    those when rounded to float32."""
    thr = np.tile(SPECIAL_THRESHOLDS, 4)
    n = SPECIAL_THRESHOLDS.shape[0]
    feature = np.repeat([0, 1, 0, 1], n)
    missing = np.repeat([0, 0, 1, 1], n)
    rng = np.random.default_rng(7)
    trees = stumps(thr.shape[0], 2, 2, rng, feature=feature, threshold=thr, missing=missing)
    t = SPECIAL_THRESHOLDS
    with np.errstate(over="ignore"):
        x = np.concatenate([t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf)),
                            np.asarray([0.0, -0.0, np.nan, np.inf, -np.inf], np.float32)]).astype(dtype)
    if dtype == np.float64:
        x = np.concatenate([x, [1e39, -1e39, 1e-40, -1e-40, 1e-46, -1e-46, 7e-46, 2.1e-45, float(F32_MAX) * (1 + 2.0 ** -26),
                                float(F32_MAX) * (1 + 2.0 ** -24)]])
    a, b = np.meshgrid(x, x, indexing="ij")
    return trees, np.stack([a.ravel(), b.ravel()], 1)


PACK_N = 32


def packing_case():
    """(trees, X float32 [200, 32], starts): stumps over 32 single-feature sources, the first four on sources 31 and 0
    with ``missing_go_to_left`` 0 and 1; NaNs in exactly those two sources.  Source ``i`` is clipped to ``starts[i]``."""
    rng = np.random.default_rng(31)
    T = 48
    feature = rng.permutation(np.arange(T) % PACK_N)
    missing = rng.integers(0, 2, T)
    feature[:4], missing[:4] = [31, 31, 0, 0], [0, 1, 0, 1]
    trees = stumps(T, PACK_N, 3, rng, feature=feature, missing=missing)
    X = rng.normal(size=(200, PACK_N)).astype(np.float32)
    for k in (0, 31):
        X[rng.uniform(size=200) < 0.4, k] = np.nan
    return trees, X, 1 + np.arange(PACK_N) % 3


NON_FINITE = (np.inf, -np.inf, np.nan, 0.0, -0.0)


def non_finite_model_case():
    """(trees, X): 9 stumps with 5 outputs whose leaf values hold inf, -inf, NaN, 0.0 and -0.0 among ordinary numbers."""
    rng = np.random.default_rng(11)
    T, n_out = 9, 5
    values = rng.normal(size=(2 * T, n_out))
    put = rng.uniform(size=values.shape) < 0.15
    values[put] = rng.choice(NON_FINITE, size=int(put.sum()))
    values[:5, 0] = NON_FINITE
    trees = stumps(T, 3, n_out, rng, values=values)
    return trees, rng.normal(size=(400, 3)).astype(np.float32)


def non_finite_scalers():
    """(mean, std) pairs for 5 outputs: every non-finite value in every slot once, the other vector ordinary."""
    v = np.asarray(NON_FINITE)
    o = np.asarray([0.5, -1.5, 2.0, 1.0, -0.25])
    return [(v, o), (o, v), (v, v[::-1].copy()), (np.roll(v, 1), np.roll(v, 3))]
