"""Random forest: the arrays of a fitted tree ensemble and its device handle.

``ForestSpec`` holds sklearn's ``tree_`` arrays of every tree, concatenated (see ``fv3hip_forest_desc_t`` in
``include/fv3hip.h``), the leaf values renumbered into one ``[leaf_row, output]`` float64 table, the packed inputs and
outputs, and the target scaler's ``mean`` / ``std``.  ``ForestModel`` uploads it once (``fv3hip_forest_create``) and runs
``fv3hip_forest_predict`` / ``fv3hip_forest_apply`` on device arrays.  ``tree_arrays`` exports a fitted sklearn forest
(numpy only: the estimator is read, sklearn is not imported).
"""
import ctypes
import dataclasses
from typing import Dict, List, Mapping

import numpy as np
import torch

from . import _lib
from .ops import _require_device, _stream

# the arrays of a ForestSpec, in the order they are saved
TREE_ARRAYS = ("node_offset", "children_left", "children_right", "feature", "threshold", "missing_go_to_left", "leaf_row",
               "leaf_values")
# optional per-node training statistics (sklearn's ``tree_`` arrays of the same names), concatenated like the node arrays: a
# forest that carries them can report feature importances
TREE_STATS = ("impurity", "n_node_samples", "weighted_n_node_samples")


def float32_floor(t: np.ndarray) -> np.ndarray:
    """The largest float32 <= each float64 ``t``: for every float32 ``x``, ``x <= float32_floor(t)`` iff ``x <= t``
    (round to nearest, then one step down where that rounded up)."""
    t = np.asarray(t, np.float64)
    r = t.astype(np.float32)
    up = r.astype(np.float64) > t
    r[up] = np.nextafter(r[up], np.float32(-np.inf))
    return r


def tree_arrays(estimator) -> Dict[str, np.ndarray]:
    """sklearn ``tree_`` arrays of every tree of a fitted forest (``estimator.estimators_``), concatenated with tree-local
    node ids, thresholds as ``float32_floor``, and the leaves' values renumbered into one ``[leaf_row, n_out]`` table; plus the
    ``TREE_STATS`` of every node."""
    offsets, left, right, feature, threshold, missing, leaf_row, values = [0], [], [], [], [], [], [], []
    impurity, n_node, weighted_n = [], [], []
    n_rows = 0
    for est in estimator.estimators_:
        t = est.tree_
        cl = np.asarray(t.children_left, np.int32)
        is_leaf = cl == -1
        rows = np.full(cl.shape, -1, np.int32)
        rows[is_leaf] = n_rows + np.arange(int(is_leaf.sum()), dtype=np.int32)
        n_rows += int(is_leaf.sum())
        offsets.append(offsets[-1] + cl.shape[0])
        left.append(cl)
        right.append(np.asarray(t.children_right, np.int32))
        feature.append(np.asarray(t.feature, np.int32))
        threshold.append(float32_floor(t.threshold))
        mgl = getattr(t, "missing_go_to_left", None)  # (sklearn >= 1.3)
        missing.append(np.zeros(cl.shape, np.uint8) if mgl is None else np.asarray(mgl, np.uint8))
        leaf_row.append(rows)
        values.append(np.asarray(t.value, np.float64)[is_leaf, :, 0])
        impurity.append(np.asarray(t.impurity, np.float64))
        n_node.append(np.asarray(t.n_node_samples, np.int64))
        weighted_n.append(np.asarray(t.weighted_n_node_samples, np.float64))
    return {
        "node_offset": np.asarray(offsets, np.int64),
        "children_left": np.concatenate(left),
        "children_right": np.concatenate(right),
        "feature": np.concatenate(feature),
        "threshold": np.concatenate(threshold),
        "missing_go_to_left": np.concatenate(missing),
        "leaf_row": np.concatenate(leaf_row),
        "leaf_values": np.ascontiguousarray(np.concatenate(values, axis=0)),
        "impurity": np.concatenate(impurity),
        "n_node_samples": np.concatenate(n_node),
        "weighted_n_node_samples": np.concatenate(weighted_n),
    }


@dataclasses.dataclass
class ForestInput:
    """Features [start, start + nfeat) of array ``source``: one variable's share of the packed inputs."""

    source: str
    nfeat: int
    start: int = 0


@dataclasses.dataclass
class ForestOutput:
    name: str
    nfeat: int


@dataclasses.dataclass
class ForestSpec:
    inputs: List[ForestInput]
    outputs: List[ForestOutput]
    trees: Dict[str, np.ndarray]  # TREE_ARRAYS
    mean: np.ndarray              # [n_out] target scaler
    std: np.ndarray

    @property
    def n_trees(self) -> int:
        return int(self.trees["node_offset"].shape[0]) - 1

    @property
    def n_in_features(self) -> int:
        return sum(i.nfeat for i in self.inputs)

    @property
    def n_out_features(self) -> int:
        return sum(o.nfeat for o in self.outputs)

    @property
    def sources(self) -> List[str]:
        return [i.source for i in self.inputs]

    @property
    def output_names(self) -> List[str]:
        return [o.name for o in self.outputs]

    @property
    def leaf_table_bytes(self) -> int:
        return int(self.trees["leaf_values"].nbytes)

    def validate(self):
        if len(set(self.sources)) != len(self.inputs):
            raise ValueError(f"an input variable is named twice: {self.sources}")
        nv = self.trees["leaf_values"]
        if nv.ndim != 2 or nv.shape[1] != self.n_out_features:
            raise ValueError(f"leaf values have shape {nv.shape}, expected [rows, {self.n_out_features}]")
        if self.mean.shape != (self.n_out_features,) or self.std.shape != (self.n_out_features,):
            raise ValueError(f"mean and std must have shape ({self.n_out_features},)")


class ForestModel:
    """Device handle of a random forest (``fv3hip_forest_t``)."""

    def __init__(self, spec: ForestSpec, device="cuda"):
        spec.validate()
        self.spec = spec
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ForestModel needs a 'cuda' (ROCm) device; there is no CPU fallback")
        with torch.cuda.device(self.device):
            _require_device(torch.empty(1, device=self.device))
            self._handle = create_handle(spec)

    def _sources(self, sources: Mapping[str, torch.Tensor], layout: str):
        tensors = []
        n_samples = None
        for i in self.spec.inputs:
            t = sources[i.source]
            if t.dim() == 1:
                t = t.unsqueeze(0) if layout == "feature_sample" else t.unsqueeze(1)
            if t.dim() != 2:
                raise ValueError(f"source {i.source!r} must be 1-D or 2-D, got shape {tuple(t.shape)}")
            nf, ns = (t.shape[0], t.shape[1]) if layout == "feature_sample" else (t.shape[1], t.shape[0])
            if nf < i.start + i.nfeat:
                raise ValueError(f"source {i.source!r} has {nf} features, the forest needs {i.start + i.nfeat}")
            if t.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"source {i.source!r} must be float32 or float64, got {t.dtype}")
            if n_samples is None:
                n_samples = int(ns)
            elif int(ns) != n_samples:
                raise ValueError("sources differ in their number of samples")
            tensors.append(t)
        dev = _require_device(*tensors)
        fs_ax, ss_ax = (0, 1) if layout == "feature_sample" else (1, 0)
        n = len(tensors)
        args = ((ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors]),
                (ctypes.c_int * n)(*[_lib.F64 if t.dtype == torch.float64 else _lib.F32 for t in tensors]),
                (ctypes.c_int64 * n)(*[t.stride(fs_ax) for t in tensors]),
                (ctypes.c_int64 * n)(*[t.stride(ss_ax) for t in tensors]))
        return dev, n_samples, args

    def predict(self, sources: Mapping[str, torch.Tensor], layout: str = "feature_sample") -> Dict[str, torch.Tensor]:
        """``sources``: name -> device array, ``[feature, sample]`` (``layout='feature_sample'``, or ``[sample]`` for a
        single-feature variable) or ``[sample, feature]`` (``'sample_feature'``), float32 or float64, any strides.
        Returns name -> float64 ``[feature, sample]`` (or ``[sample, feature]``): the denormalised forest mean."""
        dev, n, src = self._sources(sources, layout)
        outs = {}
        for o in self.spec.outputs:
            shape = (o.nfeat, n) if layout == "feature_sample" else (n, o.nfeat)
            outs[o.name] = torch.empty(shape, dtype=torch.float64, device=dev)
        ol = list(outs.values())
        fs_ax, ss_ax = (0, 1) if layout == "feature_sample" else (1, 0)
        k = len(ol)
        _lib.call_on(dev, "fv3hip_forest_predict", self._handle, *src, n, (ctypes.c_void_p * k)(*[t.data_ptr() for t in ol]),
                     (ctypes.c_int64 * k)(*[t.stride(fs_ax) for t in ol]), (ctypes.c_int64 * k)(*[t.stride(ss_ax) for t in ol]),
                     _stream(dev))
        return outs

    def apply(self, sources: Mapping[str, torch.Tensor], layout: str = "feature_sample") -> torch.Tensor:
        """int32 ``[tree, sample]``: the tree-local id of the leaf each sample reaches (sklearn's ``forest.apply(X).T``)."""
        dev, n, src = self._sources(sources, layout)
        leaves = torch.empty((self.spec.n_trees, n), dtype=torch.int32, device=dev)
        _lib.call_on(dev, "fv3hip_forest_apply", self._handle, *src, n, leaves.data_ptr(), _stream(dev))
        return leaves

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            try:
                _lib.load().fv3hip_forest_destroy(h)
            except Exception:
                pass


def create_handle(spec: ForestSpec):
    """``fv3hip_forest_create`` on the current device (the library validates the arrays before any HIP call)."""
    tr = {k: np.ascontiguousarray(spec.trees[k]) for k in TREE_ARRAYS}
    tr["node_offset"] = tr["node_offset"].astype(np.int64, copy=False)
    for k in ("children_left", "children_right", "feature", "leaf_row"):
        tr[k] = tr[k].astype(np.int32, copy=False)
    tr["threshold"] = tr["threshold"].astype(np.float32, copy=False)
    tr["missing_go_to_left"] = tr["missing_go_to_left"].astype(np.uint8, copy=False)
    tr["leaf_values"] = np.ascontiguousarray(tr["leaf_values"], np.float64)
    n_nodes = int(tr["children_left"].shape[0])
    for k in ("children_right", "feature", "threshold", "missing_go_to_left", "leaf_row"):
        if tr[k].shape != (n_nodes,):
            raise ValueError(f"tree array {k!r} has shape {tr[k].shape}, expected ({n_nodes},)")
    if tr["node_offset"].ndim != 1 or tr["node_offset"].shape[0] < 1 or int(tr["node_offset"][-1]) != n_nodes:
        raise ValueError("node_offset must end at the number of nodes")
    start = np.asarray([i.start for i in spec.inputs], np.intc)
    nfeat = np.asarray([i.nfeat for i in spec.inputs], np.intc)
    onf = np.asarray([o.nfeat for o in spec.outputs], np.intc)
    mean = np.ascontiguousarray(spec.mean, np.float64)
    std = np.ascontiguousarray(spec.std, np.float64)

    def ptr(a, ct):
        return a.ctypes.data_as(ctypes.POINTER(ct))

    d = _lib.ForestDesc()
    d.n_trees = int(tr["node_offset"].shape[0]) - 1
    d.node_offset = ptr(tr["node_offset"], ctypes.c_int64)
    d.children_left = ptr(tr["children_left"], ctypes.c_int32)
    d.children_right = ptr(tr["children_right"], ctypes.c_int32)
    d.feature = ptr(tr["feature"], ctypes.c_int32)
    d.threshold = ptr(tr["threshold"], ctypes.c_float)
    d.missing_go_to_left = ptr(tr["missing_go_to_left"], ctypes.c_uint8)
    d.leaf_row = ptr(tr["leaf_row"], ctypes.c_int32)
    d.n_leaf_rows = int(tr["leaf_values"].shape[0])
    d.leaf_values = ptr(tr["leaf_values"], ctypes.c_double)
    d.n_sources = len(spec.inputs)
    d.src_feat_start = ptr(start, ctypes.c_int)
    d.src_nfeat = ptr(nfeat, ctypes.c_int)
    d.n_outputs = len(spec.outputs)
    d.out_nfeat = ptr(onf, ctypes.c_int)
    d.mean = ptr(mean, ctypes.c_double)
    d.std = ptr(std, ctypes.c_double)
    handle = ctypes.c_void_p()
    _lib.call("fv3hip_forest_create", ctypes.byref(d), ctypes.byref(handle))
    return handle
