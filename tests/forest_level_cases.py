"""The single-level cases of ``test_gpu_forest_train_levels.py``: data, hand-made segment layouts and, per case, the conditions
it claims to meet (``check``), which ``test_host_forest_train_levels.py`` asserts on the CPU against ``forest_level_np``.

Targets are whole numbers in [-8, 8] and weights whole numbers in [1, 7] (zero only where a case starts from ``begin``), so that
every sum of the device is exact below 2^53 and its outputs are compared bit for bit.  The scan works in chunks of C = 256 list
positions and LDS tiles of up to 32 rows, ``ft_best_kernel`` in strides of 128, ``ft_children_kernel`` in rounds of 1024 nodes,
``ft_count_carry_kernel`` in blocks of 256 features.
"""
import dataclasses
import functools
from typing import Callable, List, Optional

import numpy as np

import forest_level_np as L

C = 256
FLT_MAX = np.finfo(np.float32).max


@dataclasses.dataclass
class LevelCase:
    name: str
    X: np.ndarray                 # [n, F] float32
    y: np.ndarray                 # [n, O] float64
    weight: np.ndarray            # [n] int32
    lengths: Optional[List[int]] = None   # the segments of one hand-made level; None: ``begin`` and up to ``levels`` levels
    levels: int = 1
    parity: int = 0
    depth: int = 0
    max_depth: int = -1
    min_samples_split: int = 2
    min_samples_leaf: int = 1
    first_node: int = 5
    seed: Optional[int] = 0       # of the layout's shuffle; None: samples dealt in index order
    check: Optional[Callable] = None      # check(case, steps): the conditions the case claims
    exact: bool = True

    def __repr__(self):
        return self.name


def int_data(n, F, O, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)).astype(np.float32)
    y = rng.integers(-8, 9, size=(n, O)).astype(np.float64)
    w = rng.integers(1, 8, size=n).astype(np.int32)
    return X, y, w


def from_heads(positions, m):
    return np.diff(list(positions) + [m]).tolist()


# ---- the reference's run of a case ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name):
    """The steps of a case: [{"list", "seg", "node", "n_nodes", "depth", "parity", "result"}], after {"begin": ...} if any."""
    case = BY_NAME[name]
    xt = np.ascontiguousarray(case.X.T)
    out = {"begin": None, "steps": []}
    if case.lengths is None:
        order = np.argsort(xt, axis=1, kind="stable").astype(np.int32)
        b = L.begin(order, case.weight)
        out["begin"], out["order"] = b, order
        lst, seg, node, n_nodes, parity = b["list"], b["seg"], b["node"], 1, 0
    else:
        lst, seg, node = L.layout(case.X, case.weight, case.lengths, case.first_node, case.seed)
        n_nodes, parity = case.first_node + len(case.lengths), case.parity
    depth = case.depth
    for _ in range(case.levels):
        r = L.level(xt, case.y, case.weight, lst, seg, node, n_nodes, depth, case.max_depth, case.min_samples_split,
                    case.min_samples_leaf)
        out["steps"].append({"list": lst, "seg": seg, "node": node, "n_nodes": n_nodes, "depth": depth, "parity": parity, "result": r})
        lst, seg, node = r["list_next"], r["seg_next"], r["node_next"]
        n_open, _, n_nodes, _ = (int(v) for v in r["level"])
        depth, parity = depth + 1, 1 - parity
        if n_open == 0:
            break
    return out


def caps(name):
    """(k_cap, node_cap) exactly as the header requires for the levels the case runs."""
    steps = reference(name)["steps"]
    k_cap = max([len(s["node"]) for s in steps] + [int(s["result"]["level"][0]) for s in steps])
    return max(k_cap, 1), int(steps[-1]["result"]["level"][2])


# ---- the conditions -------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def _check_heads(mod256=(), mod32=(), no_head_chunks=(), ends_on_chunk_edge=False, single_at=()):
    def check(case, steps):
        seg = steps[0]["seg"]
        h, m = seg[:-1], int(seg[-1])
        for v in mod256:
            assert (h % C == v).any(), f"no head at p % 256 == {v}"
        for v in mod32:
            assert (h % 32 == v).any(), f"no head at p % 32 == {v}"
        for ch in no_head_chunks:
            assert ch * C + C <= m and not ((h >= ch * C) & (h < ch * C + C)).any(), f"chunk {ch} holds a head"
        if ends_on_chunk_edge:
            assert ((seg[1:] % C == 0) & (np.diff(seg) > 1)).any()
        for p in single_at:
            k = int(np.flatnonzero(h == p)[0])
            assert seg[k + 1] == p + 1
    return check


def _check_children_rounds(case, steps):
    s, r = steps[0], steps[0]["result"]
    K = len(s["node"])
    split = r["n_left"] > 0
    assert K >= 1024
    # the running count of splits differs from the node index on both sides of every 1024 boundary that the level crosses,
    # and nodes split on both sides of it
    for edge in range(1024, K, 1024):
        assert 0 < int(split[:edge].sum()) < edge - 300 and split[edge - 2:edge].any() and split[edge:edge + 2].any()
    assert (~split).sum() == len(range(2, K, 3)) and not split[2::3].any()
    assert int(r["level"][0]) == 2 * int(split.sum())


def _check_count_carry(case, steps):
    s, r = steps[0], steps[0]["result"]
    assert case.X.shape[1] >= C and ((s["seg"][:-1] >= C) & (s["seg"][:-1] < 2 * C)).any()
    assert r["n_left"][0] > 0 and r["feature"][0] >= 0   # the segment that spans chunks 0 and 1 is partitioned


def _check_leaf_binds(case, steps):
    s, r = steps[0], steps[0]["result"]
    leaf = case.min_samples_leaf
    seg = s["seg"]
    straddles = 0
    for k in range(len(s["node"])):
        a, b = int(seg[k]), int(seg[k + 1])
        if b - a >= 2 * leaf + 1:
            assert np.isinf(r["proxy"][:, a:a + leaf - 1]).all() and np.isinf(r["proxy"][:, b - leaf:b]).all()
            assert np.isfinite(r["proxy"][:, a + leaf - 1]).all() and np.isfinite(r["proxy"][:, b - leaf - 1]).all()
            straddles += (a // C != (b - 1) // C) and (a // 32 != (b - 1) // 32)
    assert straddles >= 1


def _check_split_refuses(case, steps):
    s, r = steps[0], steps[0]["result"]
    nn = np.diff(s["seg"])
    refused = (nn >= 2 * case.min_samples_leaf) & (nn < case.min_samples_split)
    assert refused.sum() >= 2 and (r["n_left"][refused] == 0).all() and np.isfinite(r["best_proxy"][refused]).all()
    assert (r["n_left"][nn >= case.min_samples_split] > 0).all()


def _check_palindrome(distance=None):
    def check(case, steps):
        r = steps[0]["result"]
        m = int(steps[0]["seg"][-1])
        p = np.arange(m - 1)
        assert (_bits(r["proxy"][0, p]) == _bits(r["proxy"][0, m - 2 - p])).all(), "the mirrored positions do not tie"
        best = int(r["best_pos"][0, 0])
        assert np.isfinite(r["best_proxy"][0, 0]) and best < m - 2 - best
        assert _bits(r["proxy"][0, best]) == _bits(r["proxy"][0, m - 2 - best])
        assert (r["proxy"][0, :m - 1] <= r["proxy"][0, best]).all()
        if distance is not None:
            assert m - 2 - 2 * best == distance
        assert r["feature"][0] == 0 and r["n_left"][0] == best + 1
    return check


def _check_feature_tie(case, steps):
    r = steps[0]["result"]
    assert _bits(r["best_proxy"][0, 1]) == _bits(r["best_proxy"][0, 2]) and r["best_pos"][0, 1] != r["best_pos"][0, 2]
    assert r["best_proxy"][0, 0] < r["best_proxy"][0, 1] and r["feature"][0] == 1


def _check_feature_values(case, steps):
    s, r = steps[0], steps[0]["result"]
    seg, lst, x = s["seg"], s["list"], case.X[:, 0]
    names = ["zeros", "duplicates", "nextafter", "close", "flt_max", "subnormal"]
    k = {name: i for i, name in enumerate(names)}
    assert (s["node"] == case.first_node + np.arange(len(names))).all()

    def xs(name):
        return x[lst[0, seg[k[name]]:seg[k[name] + 1]]]

    def proxies(name):
        return r["proxy"][0, seg[k[name]]:seg[k[name] + 1] - 1]

    z = xs("zeros")
    both_zero = (z[:-1] == 0) & (z[1:] == 0)
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all() and both_zero.sum() >= 4
    assert np.isinf(proxies("zeros")[both_zero]).all() and np.isfinite(proxies("zeros")[~both_zero]).all()
    d = xs("duplicates")
    assert np.isinf(proxies("duplicates")[d[:-1] == d[1:]]).all() and (d[:-1] == d[1:]).sum() > 30
    lo, hi = np.float32(1e6), np.nextafter(np.float32(1e6), np.float32(2e6))
    assert r["feature"][k["nextafter"]] == 0 and r["threshold"][k["nextafter"]] == (np.float64(lo) + np.float64(hi)) / 2
    assert lo < r["threshold"][k["nextafter"]] < hi
    c = xs("close")
    assert c[1] > c[0] and c[1] <= c[0] + np.float32(1e-7) and np.isinf(proxies("close")[0]) and r["n_left"][k["close"]] == 2
    assert r["feature"][k["flt_max"]] == 0 and r["threshold"][k["flt_max"]] == 0.0 and r["n_left"][k["flt_max"]] == 2
    sub = xs("subnormal")
    tiny = np.finfo(np.float32).tiny
    assert ((sub > 0) & (sub < tiny)).sum() >= 3 and np.isinf(proxies("subnormal")[sub[1:] < tiny]).all()
    assert r["threshold"][k["subnormal"]] == np.float64(sub[sub < tiny].max()) / 2 + 0.5


def _check_real_gap(case, steps):
    """Best and second-best proxy of every node that may split differ by more than the sums' bound times 2 max|S| / min(wl, wr)."""
    n = case.X.shape[0]
    bound = 4 * n * 2.0 ** -53 * np.abs(case.weight[:, None] * case.y).max()
    searched = 0
    for s in steps:
        r = s["result"]
        if r["proxy"] is None:
            continue
        for k in range(len(s["node"])):
            a, b = int(s["seg"][k]), int(s["seg"][k + 1])
            cand = np.sort(r["proxy"][:, a:b - 1].ravel())
            cand = cand[np.isfinite(cand)]
            if cand.shape[0] < 2:
                continue
            ids = s["list"][0, a:b]
            max_s = np.abs(case.weight[ids, None] * case.y[ids]).sum(axis=0).max()   # no partial sum of the node is greater
            min_w = case.min_samples_leaf * case.weight[ids].min()
            gap = cand[-1] - cand[-2]
            assert gap > bound * 2 * max_s / min_w, f"node {s['node'][k]}: gap {gap:.3e}"
            searched += 1
    assert searched >= 3


# ---- the cases ------------------------------------------------------------------------------------------------------------
def _hand(name, n, F, O, lengths, seed, **kw):
    X, y, w = int_data(n, F, O, seed)
    return LevelCase(name, X, y, w, lengths=list(lengths), **kw)


def _one_segment():
    out = []
    for i, m in enumerate((1, 2, 31, 32, 33, 255, 256, 257, 512, 513, 769)):
        for O in (1, 2):
            for parity in (0, 1):
                out.append(_hand(f"one_segment_m{m}_o{O}_parity{parity}", m + 3, 3, O, [m], 100 + i, parity=parity, first_node=parity))
    return out


def _many_segments():
    out = []
    h = [0, 31, 32, 255, 256, 257, 511, 512, 513, 600, 767, 800]
    out.append(_hand("heads_at_chunk_and_tile_edges", 910, 3, 2, from_heads(h, 900), 120,
                     check=_check_heads(mod256=(0, 1, 255), mod32=(0, 31), single_at=(31, 255, 256, 511, 512))))
    out.append(_hand("segments_end_on_a_chunks_last_position", 610, 3, 2, from_heads([0, 100, 256, 300, 512], 600), 121,
                     check=_check_heads(ends_on_chunk_edge=True)))
    out.append(_hand("single_samples_at_255_and_256", 400, 3, 2, from_heads([0, 255, 256, 257], 400), 122,
                     check=_check_heads(single_at=(255, 256))))
    spanning = from_heads([0, 200, 900], 1000)
    out.append(_hand("segment_over_four_chunks", 1003, 3, 2, spanning, 123, check=_check_heads(no_head_chunks=(1, 2))))
    out.append(_hand("segment_over_four_chunks_final_depth", 1003, 3, 2, spanning, 123, depth=3, max_depth=3,
                     check=_check_heads(no_head_chunks=(1, 2))))
    return out


def _many_nodes():
    out = []
    for K in (1024, 1025, 2500):
        lengths = [2 + (k % 2) for k in range(K)]
        X, y, w = int_data(sum(lengths) + 1, 2, 1, 130 + K)
        lst, seg, _ = L.layout(X, w, lengths, 0, 0)
        for k in range(2, K, 3):          # every third node is pure: a leaf
            y[lst[0, seg[k]:seg[k + 1]]] = float(k % 17 - 8)
        for k in range(K):                # and no other is
            if k % 3 != 2:
                ids = lst[0, seg[k]:seg[k + 1]]
                y[ids[0]], y[ids[1]] = 3.0, -5.0
        out.append(LevelCase(f"open_nodes_{K}", X, y, w, lengths=lengths, first_node=K - 1, depth=11, check=_check_children_rounds))
    return out


def _many_features():
    return [_hand(f"features_{F}_head_in_chunk_1", 300, F, 1, [260, 40], 140 + F, check=_check_count_carry) for F in (256, 257, 300)]


def _many_outputs():
    out = [_hand(f"outputs_{O}", 283, 2, O, [150, 130], 150 + O) for O in (254, 255, 300)]
    out += [_hand(f"outputs_{O}", 64, 2, O, [40, 24], 150 + O) for O in (1000, 3821)]
    return out


def _min_samples():
    out = [_hand(f"min_samples_leaf_{leaf}_binds", 450, 3, 1, [20, 250, 100, 35, 34, 3, 4], 160 + leaf, min_samples_leaf=leaf,
                 min_samples_split=2 * leaf, check=_check_leaf_binds) for leaf in (2, 17)]
    out.append(_hand("min_samples_split_refuses", 330, 3, 1, [6, 9, 10, 250, 40, 4], 163, min_samples_leaf=2, min_samples_split=10,
                     check=_check_split_refuses))
    return out


def _ties():
    out = []
    m = 300
    rng = np.random.default_rng(170)
    half = rng.integers(-8, 9, size=m // 2)
    wh = rng.integers(1, 8, size=m // 2)
    X = np.stack([np.arange(m), np.full(m, 0.5)], axis=1).astype(np.float32)   # (a constant second feature: never split on)
    y = np.concatenate([half, half[::-1]]).astype(np.float64)[:, None]
    w = np.concatenate([wh, wh[::-1]]).astype(np.int32)
    out.append(LevelCase("tie_palindrome", X, y, w, lengths=[m], seed=None, check=_check_palindrome()))
    for p in (10, 85, 21):                # a top hat: the two best positions are 278, 128 and 256 apart
        i = np.arange(m)
        y = np.where((i <= p) | (i >= m - 1 - p), 8.0, -8.0)[:, None]
        out.append(LevelCase(f"tie_positions_{m - 2 - 2 * p}_apart", X, y, np.full(m, 3, np.int32), lengths=[m], seed=None,
                             check=_check_palindrome(m - 2 - 2 * p)))
    x = rng.permutation(m).astype(np.float32)
    X = np.stack([rng.normal(size=m).astype(np.float32), x, -x], axis=1)
    y = (np.where(x > 120, 6.0, -7.0) + rng.integers(-1, 2, size=m))[:, None]
    out.append(LevelCase("tie_between_features", X, y, rng.integers(1, 8, size=m).astype(np.int32), lengths=[m], check=_check_feature_tie))
    return out


def _feature_values():
    rng = np.random.default_rng(180)
    lo, hi = np.float32(1e6), np.nextafter(np.float32(1e6), np.float32(2e6))
    near = np.float32(0.1) + np.float32(5e-8)
    groups = [
        (np.array([-1, -0.0, 0.0, -0.0, 0.0, 1, 0.0, -0.0, 2, -0.0], np.float32), None),
        (rng.integers(0, 4, size=40).astype(np.float32), None),
        (np.array([lo, hi, lo, hi, hi, lo], np.float32), [-8, 8, -8, 8, 8, -8]),
        (np.array([0.1, near, 0.5, 0.9, 1.3], np.float32), [-8, 8, 8, 8, 8]),
        (np.array([-FLT_MAX, FLT_MAX, -FLT_MAX, FLT_MAX], np.float32), [-8, 8, -8, 8]),
        (np.array([1e-45, 3e-45, 0.0, 1e-40, 1.0, 2.0, 1e-39], np.float32), [-8, -8, -8, -8, 8, 8, -8]),
    ]
    x = np.concatenate([g for g, _ in groups])
    y = np.concatenate([rng.integers(-8, 9, size=g.shape[0]) if t is None else np.asarray(t) for g, t in groups]).astype(np.float64)
    X = np.stack([x, -x], axis=1)
    w = rng.integers(1, 8, size=x.shape[0]).astype(np.int32)
    return [LevelCase("feature_values", X, y[:, None], w, lengths=[g.shape[0] for g, _ in groups], seed=None, check=_check_feature_values)]


def _begin():
    out = []
    for n in (1, 255, 256, 257, 1000):
        X, y, w = int_data(n, 3, 1, 190 + n)
        last = np.zeros(n, np.int32)
        last[-1] = 4
        alternate = np.where(np.arange(n) % 2 == 0, w, 0).astype(np.int32)
        for label, weight in (("all_positive", w), ("only_the_last_positive", last), ("alternating", alternate)):
            out.append(LevelCase(f"begin_n{n}_{label}", X, y, weight, levels=3))
    return out


def _real():
    rng = np.random.default_rng(201)
    n = 300
    X = rng.normal(size=(n, 2)).astype(np.float32)
    y = 0.5 * np.tanh(X.astype(np.float64) @ rng.normal(size=(2, 2)) + 0.3 * rng.normal(size=(n, 2)))
    w = rng.integers(0, 4, size=n).astype(np.int32)
    return [LevelCase("real_targets", X, y, w, levels=3, min_samples_leaf=5, min_samples_split=10, exact=False, check=_check_real_gap)]


CASES = (_one_segment() + _many_segments() + _many_nodes() + _many_features() + _many_outputs() + _min_samples() + _ties()
         + _feature_values() + _begin() + _real())
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
