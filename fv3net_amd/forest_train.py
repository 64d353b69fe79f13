"""Random-forest training on the device: sklearn's ``RandomForestRegressor.fit`` (squared error, exact best split, every
feature considered) through ``csrc/forest_train.hip``.

``ForestTrainer`` keeps the inputs, the targets, one stable argsort per feature and the workspaces on the device and grows one
tree per ``grow`` call, level by level (``fv3hip_forest_train_begin`` / ``_level``); the host reads one small record per level
and, at the end, the tree, which it renumbers into sklearn's order (depth first, left subtree first).  ``grow_forest`` draws the
trees' seeds and bootstrap counts as sklearn draws them; ``forest_arrays`` concatenates trees into ``forest.TREE_ARRAYS`` plus
``forest.TREE_STATS``.  Among splits of equal proxy the lowest feature index wins, where sklearn keeps the first in the order of
a private random stream: the trees partition the training samples into the same leaves with the same values, but need not
name the same feature at a node where two features induce the same partition.
"""
import ctypes
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .forest import TREE_STATS, float32_floor
from .ops import _require_device, _stream

# what ``ForestTrainer.grow`` returns for one tree (sklearn's ``tree_`` arrays of the same names)
GROWN_ARRAYS = ("children_left", "children_right", "feature", "threshold", "missing_go_to_left", "value", "impurity",
                "n_node_samples", "weighted_n_node_samples")


def tree_seeds(random_state: Optional[int], n_estimators: int) -> List[int]:
    """The ``random_state`` of every tree (``ensemble._base._set_random_states``)."""
    rs = np.random.RandomState(random_state)
    return [int(rs.randint(np.iinfo(np.int32).max)) for _ in range(n_estimators)]


def n_bootstrap_samples(n: int, max_samples: Union[int, float, None]) -> int:
    """``ensemble._forest._get_n_samples_bootstrap``."""
    if max_samples is None:
        return n
    if isinstance(max_samples, (int, np.integer)) and not isinstance(max_samples, bool):
        if not 1 <= max_samples <= n:
            raise ValueError(f"max_samples must be in [1, {n}], got {max_samples}")
        return int(max_samples)
    if not 0.0 < max_samples <= 1.0:
        raise ValueError(f"a float max_samples must be in (0, 1], got {max_samples}")
    return max(round(n * max_samples), 1)


def bootstrap_counts(seed: int, n: int, n_draws: int) -> np.ndarray:
    """How often each sample is drawn for the tree seeded ``seed`` (``_generate_sample_indices`` + ``bincount``)."""
    return np.bincount(np.random.RandomState(seed).randint(0, n, n_draws), minlength=n).astype(np.int32)


def resolve_min_samples(n: int, min_samples_split: Union[int, float], min_samples_leaf: Union[int, float]):
    """sklearn's reading of the two ``min_samples_*`` (``BaseDecisionTree._fit``): a float is a fraction of ``n``."""
    leaf = int(min_samples_leaf) if isinstance(min_samples_leaf, (int, np.integer)) else int(np.ceil(min_samples_leaf * n))
    split = int(min_samples_split) if isinstance(min_samples_split, (int, np.integer)) else max(2, int(np.ceil(min_samples_split * n)))
    if leaf < 1 or split < 2:
        raise ValueError(f"min_samples_leaf must be at least 1 and min_samples_split at least 2, got {min_samples_leaf} and "
                         f"{min_samples_split}")
    return max(split, 2 * leaf), leaf


def check_max_features(max_features, n_features: int) -> None:
    """Pass where ``max_features`` means every feature -- ``"auto"``, ``None``, the float 1.0 or the integer feature count (by
    type: the integer 1 is one feature per node, and ``True == 1.0``) -- and refuse everything else."""
    is_int = isinstance(max_features, (int, np.integer)) and not isinstance(max_features, (bool, np.bool_))
    is_float = isinstance(max_features, (float, np.floating))
    if max_features is None or (isinstance(max_features, str) and max_features == "auto") or (is_float and max_features == 1.0) \
            or (is_int and max_features == n_features):
        return
    raise NotImplementedError(
        f"max_features={max_features!r}: a subset of the features at every node is drawn from sklearn's private feature-sampling "
        "stream, which this trainer does not reproduce; only all features ('auto', None, 1.0 or the feature count) are supported")


class ForestTrainer:
    """Resident training data of one forest: float32 ``X`` [n, F], float64 ``y`` [n, O] (already normalised)."""

    def __init__(self, X, y, device="cuda"):
        X = np.ascontiguousarray(np.asarray(X, np.float32))
        y = np.asarray(y, np.float64)
        y = np.ascontiguousarray(y.reshape(y.shape[0], -1))
        if X.ndim != 2 or X.shape[0] != y.shape[0] or X.shape[0] < 1 or X.shape[1] < 1 or y.shape[1] < 1:
            raise ValueError(f"X {X.shape} and y {y.shape} must be [n, F] and [n, O] with n, F, O >= 1")
        if not np.isfinite(X).all() or not np.isfinite(y).all():
            raise ValueError("the random-forest trainer needs finite inputs and targets (sklearn refuses NaN targets and infinities)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            _require_device(torch.empty(0, device=self.device))  # raises: there is no CPU path
        self.n, self.F = X.shape
        self.O = y.shape[1]
        dev = self.device
        with torch.cuda.device(dev):
            _require_device(torch.empty(1, device=dev))
            self.chunk = int(_lib.load().fv3hip_forest_train_chunk())
            self._xt = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)
            self._y = torch.from_numpy(y).to(dev)
            self._ysq = torch.from_numpy(np.cumsum(y * y, axis=1)[:, -1].copy()).to(dev)  # in output order
            # ties by sample index; once per forest
            self._order = torch.sort(self._xt, dim=1, stable=True).indices.to(torch.int32).contiguous()
            n, F, O = self.n, self.F, self.O
            chunks = -(-n // self.chunk)
            self._weight = torch.zeros(n, dtype=torch.int32, device=dev)
            self._bufs = {
                "list_a": torch.zeros((F, n), dtype=torch.int32, device=dev),
                "list_b": torch.zeros((F, n), dtype=torch.int32, device=dev),
                "side": torch.zeros(n, dtype=torch.uint8, device=dev),
                "pos_node": torch.zeros(n, dtype=torch.int32, device=dev),
                "carry": torch.zeros((F, chunks, O + 2), dtype=torch.float64, device=dev),
                "count": torch.zeros((F, chunks), dtype=torch.int32, device=dev),
                "proxy": torch.zeros((F, n), dtype=torch.float64, device=dev),
                "level": torch.zeros(4, dtype=torch.int64, device=dev),
            }
            self._caps = (0, 0)
            self._sized: Dict[str, torch.Tensor] = {}
        self.scan_bytes = 0   # of the last grow: in-bag positions x F x O x 8 over the levels that searched for splits
        self.levels = 0

    def _size_for(self, k_cap: int, node_cap: int) -> None:
        """The per-node buffers, grown to the largest tree asked for so far."""
        if k_cap <= self._caps[0] and node_cap <= self._caps[1]:
            return
        k_cap, node_cap = max(k_cap, self._caps[0]), max(node_cap, self._caps[1])
        dev, F, O = self.device, self.F, self.O
        i32, i64, f64 = torch.int32, torch.int64, torch.float64
        with torch.cuda.device(dev):
            self._sized = {
                "seg_a": torch.zeros(k_cap + 1, dtype=i64, device=dev), "seg_b": torch.zeros(k_cap + 1, dtype=i64, device=dev),
                "node_a": torch.zeros(k_cap, dtype=i32, device=dev), "node_b": torch.zeros(k_cap, dtype=i32, device=dev),
                "stats": torch.zeros((k_cap, O + 2), dtype=f64, device=dev),
                "best_proxy": torch.zeros((k_cap, F), dtype=f64, device=dev),
                "best_pos": torch.zeros((k_cap, F), dtype=i64, device=dev),
                "n_left": torch.zeros(k_cap, dtype=i64, device=dev), "dst_left": torch.zeros(k_cap, dtype=i64, device=dev),
                "dst_right": torch.zeros(k_cap, dtype=i64, device=dev),
                "left": torch.zeros(node_cap, dtype=i32, device=dev), "right": torch.zeros(node_cap, dtype=i32, device=dev),
                "feature": torch.zeros(node_cap, dtype=i32, device=dev),
                "threshold": torch.zeros(node_cap, dtype=f64, device=dev),
                "missing_left": torch.zeros(node_cap, dtype=torch.uint8, device=dev),
                "value": torch.zeros((node_cap, O), dtype=f64, device=dev),
                "impurity": torch.zeros(node_cap, dtype=f64, device=dev),
                "weighted_n": torch.zeros(node_cap, dtype=f64, device=dev),
                "n_samples": torch.zeros(node_cap, dtype=i32, device=dev),
            }
        self._caps = (k_cap, node_cap)

    def _workspace(self) -> "_lib.ForestTrain":
        ws = _lib.ForestTrain()
        ws.n, ws.F, ws.O = self.n, self.F, self.O
        ws.xt, ws.y, ws.ysq = self._xt.data_ptr(), self._y.data_ptr(), self._ysq.data_ptr()
        ws.order, ws.weight = self._order.data_ptr(), self._weight.data_ptr()
        for name, t in list(self._bufs.items()) + list(self._sized.items()):
            setattr(ws, name, t.data_ptr())
        ws.k_cap, ws.node_cap = self._caps
        return ws

    def grow(self, weights, max_depth: Optional[int] = None, min_samples_split: int = 2, min_samples_leaf: int = 1) -> Dict[str, np.ndarray]:
        """One tree on the samples with ``weights`` > 0 (integer bootstrap counts), as ``GROWN_ARRAYS`` in sklearn's node order.
        ``min_samples_*`` are counts."""
        return self._grow(weights, max_depth, min_samples_split, min_samples_leaf)

    def _grow(self, weights, max_depth, min_samples_split, min_samples_leaf, scan_events: Optional[list] = None):
        """``grow``; with ``scan_events`` (a list; benchmarks/forest_train.py) every level runs its phases in three calls and
        appends the pair of ``torch.cuda.Event`` around the scan launches."""
        w = np.asarray(weights)
        if w.shape != (self.n,) or (w < 0).any() or not np.array_equal(w, np.floor(w)):
            raise ValueError(f"weights must be {self.n} non-negative whole numbers")
        if max_depth is not None and max_depth < 1:
            raise ValueError(f"max_depth must be at least 1 or None, got {max_depth}")
        if min_samples_split < 2 or min_samples_leaf < 1:
            raise ValueError("min_samples_split must be at least 2 and min_samples_leaf at least 1")
        m = int(np.count_nonzero(w))
        if m < 1:
            raise ValueError("no sample has a positive weight")
        depth_cap = 62 if max_depth is None else min(int(max_depth), 62)
        self._size_for(min(m, 1 << depth_cap), min(2 * m - 1, (1 << (depth_cap + 1)) - 1))
        dev = self.device
        md = -1 if max_depth is None else int(max_depth)
        with torch.cuda.device(dev):
            self._weight.copy_(torch.from_numpy(w.astype(np.int32)))
            ws = self._workspace()
            stream = _stream(dev)
            _lib.call("fv3hip_forest_train_begin", ctypes.byref(ws), m, stream)
            n_open, n_pos, n_nodes, depth = 1, m, 1, 0
            self.scan_bytes, self.levels = 0, 0
            while n_open > 0:
                searched = md < 0 or depth < md
                args = (ctypes.byref(ws), depth & 1, n_open, n_pos, n_nodes, depth, md, int(min_samples_split), int(min_samples_leaf))
                if scan_events is None:
                    _lib.call("fv3hip_forest_train_level", *args, _lib.FOREST_TRAIN_ALL, stream)
                else:
                    pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    _lib.call("fv3hip_forest_train_level", *args, _lib.FOREST_TRAIN_SUMS, stream)
                    pair[0].record()
                    _lib.call("fv3hip_forest_train_level", *args, _lib.FOREST_TRAIN_SCAN, stream)
                    pair[1].record()
                    _lib.call("fv3hip_forest_train_level", *args, _lib.FOREST_TRAIN_SPLIT, stream)
                    if searched:
                        scan_events.append(pair)
                if searched:
                    self.scan_bytes += n_pos * self.F * self.O * 8
                self.levels += 1
                n_open, n_pos, n_nodes, error = (int(v) for v in self._bufs["level"].cpu())
                if error:
                    raise RuntimeError("the forest-training workspace is too small for the tree (internal error)")
                depth += 1
            s = self._sized
            tree = {
                "children_left": s["left"][:n_nodes].cpu().numpy(), "children_right": s["right"][:n_nodes].cpu().numpy(),
                "feature": s["feature"][:n_nodes].cpu().numpy(), "threshold": s["threshold"][:n_nodes].cpu().numpy(),
                "missing_go_to_left": s["missing_left"][:n_nodes].cpu().numpy(), "value": s["value"][:n_nodes].cpu().numpy(),
                "impurity": s["impurity"][:n_nodes].cpu().numpy(),
                "n_node_samples": s["n_samples"][:n_nodes].cpu().numpy(),
                "weighted_n_node_samples": s["weighted_n"][:n_nodes].cpu().numpy(),
            }
        return depth_first(tree)


def depth_first(tree: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A tree numbered level by level, renumbered as sklearn numbers its nodes: depth first, the left subtree first."""
    left, right = tree["children_left"], tree["children_right"]
    n = left.shape[0]
    new_of_old = np.full(n, -1, np.int64)
    stack, count = [0], 0
    while stack:
        node = stack.pop()
        new_of_old[node] = count
        count += 1
        if left[node] != -1:
            stack.append(int(right[node]))
            stack.append(int(left[node]))
    if count != n:
        raise RuntimeError(f"the grown tree has {n} nodes but {count} hang from its root (internal error)")
    old_of_new = np.argsort(new_of_old)
    out = {k: np.ascontiguousarray(v[old_of_new]) for k, v in tree.items()}
    for k in ("children_left", "children_right"):
        c = out[k].astype(np.int64)
        out[k] = np.where(c == -1, -1, new_of_old[np.maximum(c, 0)]).astype(np.int32)
    return out


def forest_arrays(trees: Sequence[Dict[str, np.ndarray]]) -> Dict[str, np.ndarray]:
    """``GROWN_ARRAYS`` of every tree, concatenated into ``forest.TREE_ARRAYS`` (thresholds through ``float32_floor``, the
    leaves' values in one table) plus ``forest.TREE_STATS``."""
    offsets, leaf_row, values, n_rows = [0], [], [], 0
    for t in trees:
        is_leaf = t["children_left"] == -1
        rows = np.full(is_leaf.shape, -1, np.int32)
        rows[is_leaf] = n_rows + np.arange(int(is_leaf.sum()), dtype=np.int32)
        n_rows += int(is_leaf.sum())
        offsets.append(offsets[-1] + is_leaf.shape[0])
        leaf_row.append(rows)
        values.append(np.asarray(t["value"], np.float64)[is_leaf])

    def cat(key, dtype):
        return np.concatenate([np.asarray(t[key], dtype) for t in trees])

    out = {
        "node_offset": np.asarray(offsets, np.int64),
        "children_left": cat("children_left", np.int32),
        "children_right": cat("children_right", np.int32),
        "feature": cat("feature", np.int32),
        "threshold": np.concatenate([float32_floor(t["threshold"]) for t in trees]),
        "missing_go_to_left": cat("missing_go_to_left", np.uint8),
        "leaf_row": np.concatenate(leaf_row),
        "leaf_values": np.ascontiguousarray(np.concatenate(values, axis=0)),
        "impurity": cat("impurity", np.float64),
        "n_node_samples": cat("n_node_samples", np.int64),
        "weighted_n_node_samples": cat("weighted_n_node_samples", np.float64),
    }
    assert set(TREE_STATS) <= set(out)
    return out


def grow_forest(X, y, n_estimators: int = 100, random_state: Optional[int] = 0, max_depth: Optional[int] = None,
                min_samples_split: Union[int, float] = 2, min_samples_leaf: Union[int, float] = 1, max_features="auto",
                max_samples: Union[int, float, None] = None, bootstrap: bool = True, device="cuda",
                trainer: Optional[ForestTrainer] = None) -> List[Dict[str, np.ndarray]]:
    """The trees of ``RandomForestRegressor(n_estimators, random_state=..., ...).fit(X, y)``, one ``grow`` each."""
    X = np.asarray(X)
    if n_estimators < 1:
        raise ValueError(f"n_estimators must be at least 1, got {n_estimators}")
    check_max_features(max_features, X.shape[1])
    n = X.shape[0]
    if not bootstrap and max_samples is not None:
        raise ValueError("`max_samples` cannot be set if `bootstrap=False`")
    n_draws = n_bootstrap_samples(n, max_samples) if bootstrap else n
    split, leaf = resolve_min_samples(n, min_samples_split, min_samples_leaf)
    trainer = trainer or ForestTrainer(X, y, device=device)
    trees = []
    for seed in tree_seeds(random_state, n_estimators):
        w = bootstrap_counts(seed, n, n_draws) if bootstrap else np.ones(n, np.int32)
        trees.append(trainer.grow(w, max_depth, split, leaf))
    return trees


def feature_importances(trees: Dict[str, np.ndarray], n_features: int) -> np.ndarray:
    """[tree, feature]: sklearn's ``feature_importances_`` of every tree of ``TREE_ARRAYS`` + ``TREE_STATS`` -- over the internal
    nodes, ``w imp - w_L imp_L - w_R imp_R`` added to the split feature, over the root's weight, normalised to sum 1."""
    offsets = np.asarray(trees["node_offset"], np.int64)
    out = np.zeros((offsets.shape[0] - 1, n_features))
    for t in range(out.shape[0]):
        sl = slice(int(offsets[t]), int(offsets[t + 1]))
        left, right, feat = (np.asarray(trees[k][sl], np.int64) for k in ("children_left", "children_right", "feature"))
        w = np.asarray(trees["weighted_n_node_samples"][sl], np.float64)
        imp = np.asarray(trees["impurity"][sl], np.float64)
        for node in np.flatnonzero(left != -1):   # in node order, as Tree.compute_feature_importances adds them
            out[t, feat[node]] += w[node] * imp[node] - w[left[node]] * imp[left[node]] - w[right[node]] * imp[right[node]]
        out[t] /= w[0]
        total = out[t].sum()
        if total > 0.0:
            out[t] /= total
    return out
