"""Float64 numpy restatement of the random-forest trainer (``fv3net_amd.forest_train``; sklearn's
``RandomForestRegressor.fit`` with the squared-error criterion, the exact splitter and every feature considered).

What it restates, rule for rule:
  seeds     ``RandomState(random_state).randint(np.iinfo(np.int32).max)`` per tree, then
            ``RandomState(seed).randint(0, n, n_bootstrap)``; the tree is fitted with ``sample_weight = bincount(indices)`` and
            the zero-weight samples dropped; ``min_samples_*`` count the in-bag samples unweighted.
  split     per feature, in the stable order of its float32 values (ties by sample index): position p | p + 1 is admissible
            where ``x[p + 1] > float32(x[p] + float32(1e-7))`` and both sides hold ``min_samples_leaf`` samples; the proxy is
            ``sum_k SL_k^2 / WL + sum_k (S_k - SL_k)^2 / WR``; the greatest wins, then the lowest feature, then the lowest
            position (sklearn visits the features in the order of a private random stream and keeps the first: node-for-node
            equality is not claimed, the partition of the samples into leaves is).  Threshold: ``x[p] / 2 + x[p + 1] / 2`` in
            float64, ``x[p]`` where that equals ``x[p + 1]`` or is infinite.
  leaf      depth >= max_depth, n < min_samples_split, n < 2 min_samples_leaf, impurity <= DBL_EPSILON, no admissible position.
  impurity  ``(sum w y^2 / W - sum_k (S_k / W)^2) / O``; value ``S_k / W``.
Sums run sequentially (``np.cumsum``); ``pairwise=True`` takes the node totals and the sums over the outputs with ``np.sum``
(pairwise) and the running sums in extended precision, rounded: a differently rounded twin, for choosing test seeds on which no
decision hangs on the last bit.  Nodes are numbered as sklearn numbers them: depth first, left subtree first.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
_MAX_BLOCK = 1 << 21  # elements of one [position, feature, output] block


def tree_seeds(random_state, n_estimators):
    rs = np.random.RandomState(random_state)
    return [int(rs.randint(np.iinfo(np.int32).max)) for _ in range(n_estimators)]


def n_bootstrap(n, max_samples):
    if max_samples is None:
        return n
    if isinstance(max_samples, (int, np.integer)):
        return int(max_samples)
    return max(round(n * max_samples), 1)


def bootstrap_counts(seed, n, n_draws):
    return np.bincount(np.random.RandomState(seed).randint(0, n, n_draws), minlength=n)


def _seq(a, axis):
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def _best_split(Xn, yn, wn, min_samples_leaf, pairwise):
    """(proxy, feature, position) of the best admissible split of one node, or None."""
    m, F = Xn.shape
    O = yn.shape[1]
    total = np.sum(wn[:, None] * yn, axis=0) if pairwise else _seq(wn[:, None] * yn, 0)
    w_total = wn.sum()
    n_left = np.arange(1, m)
    counts_ok = (n_left >= min_samples_leaf) & (m - n_left >= min_samples_leaf)
    best = (-np.inf, -1, -1)
    block = max(1, _MAX_BLOCK // max(1, m * O))
    for f0 in range(0, F, block):
        xb = Xn[:, f0:f0 + block]
        order = np.argsort(xb, axis=0, kind="stable")
        xs = np.take_along_axis(xb, order, axis=0)
        wy = wn[order][:, :, None] * yn[order]                       # [m, f, O]
        if pairwise:
            sl = np.cumsum(wy.astype(np.longdouble), axis=0).astype(np.float64)[:-1]
        else:
            sl = np.cumsum(wy, axis=0)[:-1]
        sr = total - sl
        wl = np.cumsum(wn[order], axis=0)[:-1]
        wr = w_total - wl
        pl, pr = (np.sum(sl * sl, axis=2), np.sum(sr * sr, axis=2)) if pairwise else (_seq(sl * sl, 2), _seq(sr * sr, 2))
        ok = counts_ok[:, None] & ~(xs[1:] <= xs[:-1] + np.float32(1e-7)) & (wl > 0) & (wr > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            proxy = np.where(ok, pl / wl + pr / wr, -np.inf)
        pos = np.argmax(proxy, axis=0)                               # the first (lowest) position of the greatest
        val = proxy[pos, np.arange(proxy.shape[1])]
        for j in range(val.shape[0]):
            if val[j] > best[0]:
                best = (val[j], f0 + j, (xs[pos[j], j], xs[pos[j] + 1, j]))
    return None if best[1] < 0 else best


def grow(X, y, weights, max_depth=None, min_samples_split=2, min_samples_leaf=1, pairwise=False):
    """One tree on float32 ``X`` [n, F], float64 ``y`` [n, O] and integer ``weights`` [n].  Returns sklearn's ``tree_`` arrays
    plus ``leaf_of_sample`` [n] (the leaf of every in-bag sample, -1 out of bag)."""
    X = np.asarray(X, np.float32)
    y = np.asarray(y, np.float64).reshape(X.shape[0], -1)
    w = np.asarray(weights, np.float64)
    O = y.shape[1]
    out = {k: [] for k in ("children_left", "children_right", "feature", "threshold", "value", "impurity", "n_node_samples",
                           "weighted_n_node_samples", "missing_go_to_left")}
    leaf_of = np.full(X.shape[0], -1, np.int64)
    stack = [(np.flatnonzero(w > 0), 0, -1, False)]
    while stack:
        idx, depth, parent, is_right = stack.pop()
        node = len(out["feature"])
        if parent >= 0:
            out["children_right" if is_right else "children_left"][parent] = node
        yn, wn = y[idx], w[idx]
        wy = wn[:, None] * yn
        if pairwise:
            S, W, sq = wy.sum(axis=0), wn.sum(), (wy * yn).sum()
        else:
            S, W, sq = _seq(wy, 0), wn.sum(), np.cumsum((wy * yn).ravel())[-1]
        imp = sq / W
        for k in range(O):
            imp -= (S[k] / W) ** 2.0
        imp /= O
        m = idx.shape[0]
        leaf = ((max_depth is not None and depth >= max_depth) or m < min_samples_split or m < 2 * min_samples_leaf
                or imp <= EPS)
        split = None if leaf else _best_split(X[idx], yn, wn, min_samples_leaf, pairwise)
        out["value"].append(S / W)
        out["impurity"].append(imp)
        out["n_node_samples"].append(m)
        out["weighted_n_node_samples"].append(W)
        out["children_left"].append(-1)
        out["children_right"].append(-1)
        if split is None:
            out["feature"].append(-2)
            out["threshold"].append(-2.0)
            out["missing_go_to_left"].append(0)
            leaf_of[idx] = node
            continue
        _, f, (xa, xb) = split
        thr = np.float64(xa) / 2.0 + np.float64(xb) / 2.0
        if thr == xb or np.isinf(thr):
            thr = np.float64(xa)
        go_left = X[idx, f].astype(np.float64) <= thr
        out["feature"].append(f)
        out["threshold"].append(thr)
        out["missing_go_to_left"].append(int(go_left.sum() > m - go_left.sum()))
        stack.append((idx[~go_left], depth + 1, node, True))
        stack.append((idx[go_left], depth + 1, node, False))   # popped first: the left subtree is numbered first
    dtypes = {"children_left": np.int64, "children_right": np.int64, "feature": np.int64, "threshold": np.float64,
              "value": np.float64, "impurity": np.float64, "n_node_samples": np.int64, "weighted_n_node_samples": np.float64,
              "missing_go_to_left": np.uint8}
    tree = {k: np.asarray(v, dtypes[k]) for k, v in out.items()}
    tree["value"] = tree["value"].reshape(-1, O)
    tree["leaf_of_sample"] = leaf_of
    return tree


def grow_forest(X, y, n_estimators, random_state=0, max_depth=None, min_samples_split=2, min_samples_leaf=1, bootstrap=True,
                max_samples=None, pairwise=False):
    """[(weights, tree)] per estimator, seeded as ``RandomForestRegressor`` seeds its trees."""
    n = np.asarray(X).shape[0]
    trees = []
    for seed in tree_seeds(random_state, n_estimators):
        w = bootstrap_counts(seed, n, n_bootstrap(n, max_samples)) if bootstrap else np.ones(n, np.int64)
        trees.append((w, grow(X, y, w, max_depth, min_samples_split, min_samples_leaf, pairwise=pairwise)))
    return trees


def importances(tree, n_features):
    """sklearn's ``Tree.compute_feature_importances``: the weighted impurity decrease of every split, summed by feature, over the
    root's weight, normalised to sum 1 (all zeros for a tree that is one leaf)."""
    left, right = tree["children_left"], tree["children_right"]
    w, imp = tree["weighted_n_node_samples"], tree["impurity"]
    out = np.zeros(n_features)
    for node in np.flatnonzero(left != -1):
        lc, rc = left[node], right[node]
        out[tree["feature"][node]] += w[node] * imp[node] - w[lc] * imp[lc] - w[rc] * imp[rc]
    out /= w[0]
    total = out.sum()
    return out / total if total > 0.0 else out


def leaf_partition(leaf_ids):
    """The partition that leaf ids induce, as a set of frozensets of positions: equal for two trees iff they put the same
    samples together, whatever they call their leaves."""
    leaf_ids = np.asarray(leaf_ids)
    order = np.argsort(leaf_ids, kind="stable")
    cuts = np.flatnonzero(np.diff(leaf_ids[order])) + 1
    return {frozenset(g.tolist()) for g in np.split(order, cuts)}
