"""One level of the random-forest trainer in plain numpy and Python integers: everything ``fv3hip_forest_train_begin`` and
``fv3hip_forest_train_level`` write (include/fv3hip.h, "training random forests"), from the same inputs.

With whole-number targets every sum -- the columns ``w y_k``, ``w``, ``w sum_k y_k^2`` along a segment, and the sums of squares
over the outputs -- is formed in Python integers, so it is exact, and only the documented roundings remain, in float64 and in
the documented order: ``S_k / W`` (value), ``pl / wl + pr / wr`` (proxy), ``xa / 2 + xb / 2`` (threshold), and for the impurity
``Q / W``, then ``- (S_k / W)^2`` output after output, then ``/ O``.  A device whose sums stay below 2^53 must then give the
same bits whatever the order of its sums; ``max_int`` of the result is the greatest integer any sum reached.  With other targets
the same sums run in ``np.longdouble`` and are rounded once.

``layout`` deals samples to hand-made segments, ``chain`` runs ``begin`` and the levels to the end of a tree.
"""
import numpy as np

POS_NONE = np.iinfo(np.int64).max   # best_pos where no position of the (node, feature) is admissible
EXACT_LIMIT = 1 << 53


def is_whole(y):
    return bool(np.all(np.asarray(y) == np.rint(y)))


def columns(y, weight):
    """[n, O + 2]: ``w y_k``, ``w``, ``w sum_k y_k^2`` per sample; Python integers for whole-number targets, else longdouble."""
    y = np.asarray(y, np.float64)
    n, O = y.shape
    if is_whole(y):
        assert not np.signbit(y[y == 0]).any(), "a target of -0.0 gives sums of -0.0, which integers do not have"
        yi = np.array([[int(v) for v in row] for row in y], dtype=object).reshape(n, O)
        wi = np.array([int(v) for v in weight], dtype=object)
        out = np.empty((n, O + 2), dtype=object)
        out[:, :O] = yi * wi[:, None]
        out[:, O] = wi
        out[:, O + 1] = (yi * yi).sum(axis=1) * wi if O else 0
        return out
    yl, wl = y.astype(np.longdouble), np.asarray(weight).astype(np.longdouble)
    return np.concatenate([yl * wl[:, None], wl[:, None], ((yl * yl).sum(axis=1) * wl)[:, None]], axis=1)


def _f64(a):
    return np.asarray(a).astype(np.float64)


def begin(order, weight):
    """``fv3hip_forest_train_begin``: every row of ``order`` [F, n] filtered by ``weight > 0``; one segment, the root."""
    order, weight = np.asarray(order), np.asarray(weight)
    keep = weight[order] > 0
    m = int(np.count_nonzero(weight > 0))
    lst = np.stack([row[k] for row, k in zip(order, keep)]).astype(np.int32)
    assert lst.shape == (order.shape[0], m)
    return {"list": lst, "seg": np.array([0, m], np.int64), "node": np.array([0], np.int32), "level": np.array([1, m, 1, 0], np.int64)}


def level(xt, y, weight, lst, seg, node, n_nodes, depth, max_depth, min_samples_split, min_samples_leaf):
    """``fv3hip_forest_train_level`` with all phases.  ``lst`` [F, m], ``seg`` [K + 1], ``node`` [K].  Returns a dict: per open
    node k ``stats`` [K, O + 2], ``value`` [K, O], ``impurity``, ``weighted_n``, ``n_samples``, ``feature``, ``threshold``,
    ``missing_left``, ``left``, ``right`` (the records of tree node ``node[k]``) and ``n_left``; ``proxy`` [F, m], ``best_proxy``
    and ``best_pos`` [K, F] (None on a final level); ``seg_next``, ``node_next``, ``list_next`` [F, level[1]] and ``level``."""
    xt = np.asarray(xt, np.float32)
    y = np.asarray(y, np.float64)
    F, O = xt.shape[0], y.shape[1]
    lst, seg, node = np.asarray(lst), np.asarray(seg, np.int64), np.asarray(node)
    K = node.shape[0]
    m = int(seg[K])
    assert lst.shape == (F, m) and seg[0] == 0 and (np.diff(seg) >= 1).all()
    exact = is_whole(y)
    cols = columns(y, weight)
    final = max_depth is not None and max_depth >= 0 and depth >= max_depth
    eps = np.finfo(np.float64).eps
    tiny = np.float32(1e-7)
    max_int = 0

    out = {
        "stats": np.zeros((K, O + 2)), "value": np.zeros((K, O)), "impurity": np.zeros(K), "weighted_n": np.zeros(K),
        "n_samples": np.zeros(K, np.int32), "feature": np.full(K, -2, np.int32), "threshold": np.full(K, -2.0),
        "missing_left": np.zeros(K, np.uint8), "left": np.full(K, -1, np.int32), "right": np.full(K, -1, np.int32),
        "n_left": np.zeros(K, np.int64),
        "proxy": None if final else np.full((F, m), -np.inf), "best_proxy": None if final else np.full((K, F), -np.inf),
        "best_pos": None if final else np.full((K, F), POS_NONE, np.int64),
        "impurity_scale": np.zeros(K),   # Q / (W O): what the impurity's roundings are relative to
    }
    totals = []
    for k in range(K):
        a, b = int(seg[k]), int(seg[k + 1])
        tot = cols[lst[0, a:b]].sum(axis=0)
        totals.append(tot)
        st = _f64(tot)
        if exact:
            max_int = max(max_int, max(abs(int(v)) for v in tot))
            W = st[O]
            imp = st[O + 1] / W
            for c in range(O):
                mean = st[c] / W
                imp = imp - mean * mean
            imp = imp / O
            value = st[:O] / W
        else:
            W = tot[O]
            mean = tot[:O] / W
            imp = np.float64((tot[O + 1] / W - (mean * mean).sum()) / O)
            value = _f64(mean)
        out["stats"][k], out["value"][k], out["impurity"][k] = st, value, imp
        out["weighted_n"][k], out["n_samples"][k] = st[O], b - a
        out["impurity_scale"][k] = st[O + 1] / (st[O] * O)

    if not final:
        for k in range(K):
            a, b = int(seg[k]), int(seg[k + 1])
            nn = b - a
            if nn < 2:
                continue
            n_left = np.arange(1, nn)
            counts_ok = (n_left >= min_samples_leaf) & (nn - n_left >= min_samples_leaf)
            tot = totals[k]
            for f in range(F):
                ids = lst[f, a:b]
                x = xt[f, ids]
                run = np.cumsum(cols[ids], axis=0)[:-1]
                sl, sr = run[:, :O], tot[:O] - run[:, :O]
                pl, pr = (sl * sl).sum(axis=1), (sr * sr).sum(axis=1)
                wl, wr = run[:, O], tot[O] - run[:, O]
                if exact:
                    max_int = max(max_int, int(max(pl.max(), pr.max())), max(abs(int(v)) for v in run.ravel()))
                ok = counts_ok & ~(x[1:] <= x[:-1] + tiny) & (_f64(wl) > 0) & (_f64(wr) > 0)
                if exact:
                    value = _f64(pl) / _f64(wl) + _f64(pr) / _f64(wr)
                else:
                    value = _f64(pl / wl + pr / wr)
                proxy = np.where(ok, value, -np.inf)
                out["proxy"][f, a:b - 1] = proxy
                p = int(np.argmax(proxy))   # the first, so the lowest, of the greatest
                if proxy[p] > -np.inf:
                    out["best_proxy"][k, f], out["best_pos"][k, f] = proxy[p], a + p

    # the split records, the children and the partition
    seg_next, node_next, parts = [0], [], [[] for _ in range(F)]
    for k in range(K):
        a, b = int(seg[k]), int(seg[k + 1])
        nn = b - a
        if final or nn < min_samples_split or nn < 2 * min_samples_leaf or out["impurity"][k] <= eps:
            continue
        bf, best = -1, -np.inf
        for f in range(F):
            if out["best_proxy"][k, f] > best:
                bf, best = f, out["best_proxy"][k, f]
        if bf < 0:
            continue
        pos = int(out["best_pos"][k, bf])
        xa, xb = np.float64(xt[bf, lst[bf, pos]]), np.float64(xt[bf, lst[bf, pos + 1]])
        with np.errstate(over="ignore"):
            thr = xa / 2.0 + xb / 2.0
        if thr == xb or np.isinf(thr):
            thr = xa
        nl = pos + 1 - a
        child = n_nodes + len(node_next)
        out["feature"][k], out["threshold"][k], out["missing_left"][k], out["n_left"][k] = bf, thr, nl > nn - nl, nl
        out["left"][k], out["right"][k] = child, child + 1
        node_next += [child, child + 1]
        seg_next += [seg_next[-1] + nl, seg_next[-1] + nn]
        for f in range(F):
            ids = lst[f, a:b]
            goes_left = xt[bf, ids].astype(np.float64) <= thr
            assert int(goes_left.sum()) == nl
            parts[f] += [ids[goes_left], ids[~goes_left]]
    out["seg_next"] = np.asarray(seg_next, np.int64)
    out["node_next"] = np.asarray(node_next, np.int32)
    out["list_next"] = np.stack([np.concatenate(p) if p else np.zeros(0, np.int32) for p in parts]).astype(np.int32)
    out["level"] = np.array([len(node_next), seg_next[-1], n_nodes + len(node_next), 0], np.int64)
    out["max_int"] = max_int
    return out


def chain(X, y, weight, max_depth=None, min_samples_split=2, min_samples_leaf=1):
    """``begin`` and every level to the end: the tree as the device leaves it (numbered level by level, sklearn's names), and
    the list of the levels' results."""
    X = np.asarray(X, np.float32)
    xt = np.ascontiguousarray(X.T)
    order = np.argsort(xt, axis=1, kind="stable").astype(np.int32)
    state = begin(order, weight)
    lst, seg, node = state["list"], state["seg"], state["node"]
    n_open, _, n_nodes, _ = (int(v) for v in state["level"])
    md = -1 if max_depth is None else max_depth
    names = {"left": "children_left", "right": "children_right", "feature": "feature", "threshold": "threshold",
             "missing_left": "missing_go_to_left", "value": "value", "impurity": "impurity", "n_samples": "n_node_samples",
             "weighted_n": "weighted_n_node_samples"}
    tree = {v: [] for v in names.values()}
    levels, depth = [], 0
    while n_open > 0:
        r = level(xt, y, weight, lst, seg, node, n_nodes, depth, md, min_samples_split, min_samples_leaf)
        levels.append(r)
        assert node.tolist() == list(range(n_nodes - n_open, n_nodes))
        for k, v in names.items():
            tree[v].append(r[k])
        lst, seg, node = r["list_next"], r["seg_next"], r["node_next"]
        n_open, _, n_nodes, _ = (int(v) for v in r["level"])
        depth += 1
    return {k: np.concatenate(v) for k, v in tree.items()}, levels


def layout(X, weight, lengths, first_node=0, seed=0):
    """Deals the in-bag samples (``weight > 0``), shuffled by ``seed`` (None: in index order), to ``len(lengths)`` open nodes of
    those sizes.  Returns ``list`` [F, sum(lengths)] with every segment sorted stably by its feature (ties by sample index),
    ``seg`` and ``node`` (``first_node`` onwards, in a shuffled order unless ``seed`` is None)."""
    X = np.asarray(X, np.float32)
    inbag = np.flatnonzero(np.asarray(weight) > 0)
    lengths = [int(v) for v in lengths]
    m, K = sum(lengths), len(lengths)
    assert min(lengths) >= 1 and m <= inbag.shape[0]
    rng = None if seed is None else np.random.default_rng(seed)
    dealt = inbag[:m] if rng is None else rng.permutation(inbag)[:m]
    seg = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    lst = np.zeros((X.shape[1], m), np.int32)
    for k in range(K):
        ids = np.sort(dealt[seg[k]:seg[k + 1]])
        for f in range(X.shape[1]):
            lst[f, seg[k]:seg[k + 1]] = ids[np.argsort(X[ids, f], kind="stable")]
    node = first_node + (np.arange(K) if rng is None else rng.permutation(K))
    return lst, seg, node.astype(np.int32)
