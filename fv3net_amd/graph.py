"""Graph U-Net: the arrays of fv3fit's ``"graph"`` model and its device layer.

``GraphUNetSpec`` holds what ``GraphUNetConfig.build`` produces (external/fv3fit/fv3fit/pytorch/graph/unet.py:216-261) and the
``StandardScaler`` of every state variable (pytorch/predict.py:299-387, _shared/scaler.py:56-73) as plain arrays.  The graph is the
cube's five-point graph (graph_builder.py:12-49: every cell, its four neighbours across the seams, itself), so dgl's
``SAGEConv(c_in, c_out, "mean")`` is ``h W_self + mean5(h) W_neigh + b``; the layers are, with ``m = min_filters`` and ``F`` the
state's feature count,

    first        SAGE F -> m, activation
    L0.conv1a/b  SAGE m -> 2m -> 2m, activation each         (level k: c = m 2^k, on n / 2^k cells per edge)
    (2 x 2 mean) L1.conv1a/b ... ; at the bottom  bottom.a/b  SAGE 2c -> 4c -> 4c, activation each
    L0.up        ConvTranspose2d(4c, 2c, 2, stride 2);  cat([conv1 output, up output])
    L0.conv2a/b  SAGE 4c -> 2c -> 2c, activation each
    last         SAGE 2m -> F

``GraphModel`` keeps the weights on the device and runs the layers with the stateless ``fv3hip_graph_*`` kernels on torch's
current stream, one launch after the other (no side streams: a captured rollout is one linear chain).  DESIGN.md section 16.
"""
import dataclasses
from typing import Dict, List, Mapping, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .cube import StatePacker, _Slice, check_cube_shape, cuda_device  # noqa: F401  (check_cube_shape: imported from here)
from .ops import _require_device, _stream

ACTIVATIONS = {"linear": _lib.ACT_LINEAR, "relu": _lib.ACT_RELU, "tanh": _lib.ACT_TANH}
MAX_VARIABLES = 16


def check_architecture(aggregator: str = "mean", pooling_size: int = 2, pooling_stride: int = 2, activation: str = "relu"):
    """The part of ``GraphUNetConfig`` that is built here; anything else is refused by name."""
    if aggregator != "mean":
        raise NotImplementedError(f"aggregator {aggregator!r} is not built; supported: 'mean' (gcn, pool and lstm are out of scope)")
    if int(pooling_size) != 2 or int(pooling_stride) != 2:
        raise NotImplementedError(f"pooling_size = {pooling_size}, pooling_stride = {pooling_stride}: supported is 2 and 2 (the "
                                  "reference's Down and Up reshape to n // 2 and n * 2, so nothing else is meaningful)")
    if activation not in ACTIVATIONS:
        raise NotImplementedError(f"activation {activation!r} is not built; supported: {sorted(ACTIVATIONS)}")


def layer_plan(depth: int, n_features: int, min_filters: int) -> List[Tuple[str, str, int, int, int]]:
    """(name, 'sage' | 'up', c_in, c_out, level) of every layer with weights, in execution order; level k works on cubes of
    ``n / 2**k`` cells per edge (an 'up' layer reads level k + 1 and writes level k)."""
    if depth < 1:
        raise ValueError(f"depth must be at least 1, got {depth}")
    if min_filters < 1 or n_features < 1:
        raise ValueError(f"min_filters and the feature count must be positive, got {min_filters}, {n_features}")
    down, up = [], []
    for k in range(depth):
        c = min_filters * 2 ** k
        down += [(f"L{k}.conv1a", "sage", c, 2 * c, k), (f"L{k}.conv1b", "sage", 2 * c, 2 * c, k)]
        up = [(f"L{k}.up", "up", 4 * c, 2 * c, k), (f"L{k}.conv2a", "sage", 4 * c, 2 * c, k),
              (f"L{k}.conv2b", "sage", 2 * c, 2 * c, k)] + up
    c = min_filters * 2 ** depth
    bottom = [("bottom.a", "sage", c, 2 * c, depth), ("bottom.b", "sage", 2 * c, 2 * c, depth)]
    return ([("first", "sage", n_features, min_filters, 0)] + down + bottom + up
            + [("last", "sage", 2 * min_filters, n_features, 0)])


@dataclasses.dataclass
class GraphVariable:
    """One state variable: ``nfeat`` levels normalised in float64 as ``(x - mean) / std`` per level."""

    name: str
    nfeat: int
    mean: np.ndarray
    std: np.ndarray


@dataclasses.dataclass
class SageLayer:
    """``w_self`` / ``w_neigh`` ``[c_in, c_out]`` (the transpose of torch's ``Linear.weight``), ``bias`` ``[c_out]``."""

    w_self: np.ndarray
    w_neigh: np.ndarray
    bias: np.ndarray


@dataclasses.dataclass
class UpLayer:
    """``weight`` ``[c_in, 2, 2, c_out]`` (torch's ``ConvTranspose2d.weight`` ``[c_in, c_out, kx, ky]`` with the output channel
    moved last), ``bias`` ``[c_out]``."""

    weight: np.ndarray
    bias: np.ndarray


@dataclasses.dataclass
class GraphUNetSpec:
    variables: List[GraphVariable]
    depth: int
    min_filters: int
    activation: str
    layers: Dict[str, object]            # layer_plan name -> SageLayer | UpLayer
    aggregator: str = "mean"
    pooling_size: int = 2
    pooling_stride: int = 2

    def __post_init__(self):
        self.validate()

    @property
    def state_variables(self) -> List[str]:
        return [v.name for v in self.variables]

    @property
    def n_features(self) -> int:
        return sum(v.nfeat for v in self.variables)

    @property
    def plan(self):
        return layer_plan(self.depth, self.n_features, self.min_filters)

    def flops_per_node(self) -> float:
        """Multiply-adds x 2 per cell of the full-resolution cube for one step; a layer at level k runs on 4**-k of the cells
        (an 'up' layer: 4 c_out columns per cell of level k + 1, which is c_out per cell of level k)."""
        return float(sum((4 * ci * co if kind == "sage" else 2 * ci * co) / 4.0 ** k for _, kind, ci, co, k in self.plan))

    def validate(self):
        check_architecture(self.aggregator, self.pooling_size, self.pooling_stride, self.activation)
        if not self.variables:
            raise ValueError("a graph autoregressor needs at least one state variable")
        if len(self.variables) > MAX_VARIABLES:
            raise ValueError(f"at most {MAX_VARIABLES} state variables are supported, got {len(self.variables)}")
        if len(set(self.state_variables)) != len(self.variables):
            raise ValueError(f"a state variable is named twice: {self.state_variables}")
        for v in self.variables:
            mean, std = np.asarray(v.mean), np.asarray(v.std)
            if v.nfeat < 1 or mean.shape != (v.nfeat,) or std.shape != (v.nfeat,):
                raise ValueError(f"variable {v.name!r}: mean and std must have shape ({v.nfeat},)")
            if mean.dtype != np.float64 or std.dtype != np.float64:
                raise ValueError(f"variable {v.name!r}: mean and std must be float64, as the reference's scaler keeps them")
            if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std != 0)):
                raise ValueError(f"variable {v.name!r}: mean and std must be finite and std non-zero")
        plan = self.plan
        if set(self.layers) != {p[0] for p in plan}:
            raise ValueError(f"layers {sorted(self.layers)} differ from those of a depth-{self.depth} network: {[p[0] for p in plan]}")
        for name, kind, ci, co, _ in plan:
            layer = self.layers[name]
            if kind == "sage":
                want = {"w_self": (ci, co), "w_neigh": (ci, co), "bias": (co,)}
                ok = isinstance(layer, SageLayer)
            else:
                want = {"weight": (ci, 2, 2, co), "bias": (co,)}
                ok = isinstance(layer, UpLayer)
            if not ok:
                raise ValueError(f"layer {name!r} must be a {'SageLayer' if kind == 'sage' else 'UpLayer'}")
            for key, shape in want.items():
                a = np.asarray(getattr(layer, key))
                if a.shape != shape or a.dtype != np.float32:
                    raise ValueError(f"layer {name!r}: {key} has shape {a.shape} and dtype {a.dtype}, expected float32 {shape}")

    def check_grid(self, n: int):
        if n % 2 ** self.depth != 0 or n // 2 ** self.depth < 1:
            raise ValueError(f"tiles of {n} cells per edge cannot be halved {self.depth} times (depth = {self.depth}): n must be "
                             f"a positive multiple of {2 ** self.depth}")

    # -- serialisation: (yaml-able metadata, arrays for one npz) -------------------------------------
    def to_arrays(self):
        meta = {
            "activation": self.activation, "depth": int(self.depth), "min_filters": int(self.min_filters),
            "aggregator": self.aggregator, "pooling_size": int(self.pooling_size), "pooling_stride": int(self.pooling_stride),
            "variables": [{"name": str(v.name), "nfeat": int(v.nfeat)} for v in self.variables],
        }
        arrays = {}
        for i, v in enumerate(self.variables):
            arrays[f"var{i}_mean"] = np.asarray(v.mean, np.float64)
            arrays[f"var{i}_std"] = np.asarray(v.std, np.float64)
        for name, layer in self.layers.items():
            for f in dataclasses.fields(layer):
                arrays[f"{name}.{f.name}"] = np.asarray(getattr(layer, f.name), np.float32)
        return meta, arrays

    @classmethod
    def from_arrays(cls, meta: Mapping, arrays: Mapping[str, np.ndarray]) -> "GraphUNetSpec":
        check_architecture(meta.get("aggregator", "mean"), meta.get("pooling_size", 2), meta.get("pooling_stride", 2),
                           meta.get("activation"))
        variables = [GraphVariable(v["name"], int(v["nfeat"]), np.asarray(arrays[f"var{i}_mean"], np.float64),
                                   np.asarray(arrays[f"var{i}_std"], np.float64)) for i, v in enumerate(meta["variables"])]
        depth, m = int(meta["depth"]), int(meta["min_filters"])
        layers = {}
        for name, kind, *_ in layer_plan(depth, sum(v.nfeat for v in variables), m):
            kls = SageLayer if kind == "sage" else UpLayer
            layers[name] = kls(*[np.asarray(arrays[f"{name}.{f.name}"], np.float32) for f in dataclasses.fields(kls)])
        return cls(variables, depth, m, meta["activation"], layers, aggregator=meta.get("aggregator", "mean"),
                   pooling_size=int(meta.get("pooling_size", 2)), pooling_stride=int(meta.get("pooling_stride", 2)))


class GraphModel:
    """The network and the scalers of a ``GraphUNetSpec`` on one device."""

    def __init__(self, spec: GraphUNetSpec, device="cuda"):
        spec.validate()
        self.spec = spec
        self.device = cuda_device(device, "GraphModel")
        _lib.load()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self._weights = {name: {f.name: up(getattr(layer, f.name)) for f in dataclasses.fields(layer)}
                         for name, layer in spec.layers.items()}
        self._packer = StatePacker([(v.name, v.nfeat) for v in spec.variables], np.concatenate([v.mean for v in spec.variables]),
                                   np.concatenate([v.std for v in spec.variables]), self.device)
        self._act = ACTIVATIONS[spec.activation]

    # -- layers ------------------------------------------------------------------------------------
    def _sage(self, name, src: _Slice, dst: _Slice, S, n, c_in, c_out, act):
        w = self._weights[name]
        _lib.call_on(self.device, "fv3hip_graph_sage", src.ptr, src.ld, src.off, src.stride, w["w_self"].data_ptr(),
                     w["w_neigh"].data_ptr(), w["bias"].data_ptr(), dst.ptr, dst.ld, dst.off, dst.stride, S, n, c_in, c_out, act,
                     _stream(self.device))

    def _buffer(self, S, n, c) -> _Slice:
        return _Slice(torch.empty((S, 6, n, n, c), dtype=torch.float32, device=self.device), c)

    def _forward(self, src: _Slice, dst: _Slice, S: int, n: int):
        """One step: ``src`` -> ``dst`` (both F channels wide)."""
        spec, act, st = self.spec, self._act, _stream(self.device)
        F, m = spec.n_features, spec.min_filters
        x = self._buffer(S, n, m)
        self._sage("first", src, x, S, n, F, m, act)
        cats = []
        for k in range(spec.depth):          # down: conv1, the second layer writes the first half of the level's cat buffer
            c, nk = m * 2 ** k, n >> k
            t = self._buffer(S, nk, 2 * c)
            cat = self._buffer(S, nk, 4 * c)
            self._sage(f"L{k}.conv1a", x, t, S, nk, c, 2 * c, act)
            self._sage(f"L{k}.conv1b", t, cat, S, nk, 2 * c, 2 * c, act)
            x = self._buffer(S, nk // 2, 2 * c)
            _lib.call_on(self.device, "fv3hip_graph_pool2", cat.ptr, cat.ld, 0, x.ptr, x.ld, 0, S, nk, 2 * c, st)
            cats.append(cat)
        c, nk = m * 2 ** spec.depth, n >> spec.depth
        t, low = self._buffer(S, nk, 2 * c), self._buffer(S, nk, 2 * c)
        self._sage("bottom.a", x, t, S, nk, c, 2 * c, act)
        self._sage("bottom.b", t, low, S, nk, 2 * c, 2 * c, act)
        for k in reversed(range(spec.depth)):  # up: the transposed convolution writes the second half of the cat buffer
            c, nk = m * 2 ** k, n >> k
            cat, w = cats[k], self._weights[f"L{k}.up"]
            _lib.call_on(self.device, "fv3hip_graph_up2", low.ptr, low.ld, 0, w["weight"].data_ptr(), w["bias"].data_ptr(), cat.ptr,
                         cat.ld, 2 * c, S, nk // 2, 4 * c, 2 * c, st)
            t, low = self._buffer(S, nk, 2 * c), self._buffer(S, nk, 2 * c)
            self._sage(f"L{k}.conv2a", cat, t, S, nk, 4 * c, 2 * c, act)
            self._sage(f"L{k}.conv2b", t, low, S, nk, 2 * c, 2 * c, act)
        self._sage("last", low, dst, S, n, 2 * m, F, _lib.ACT_LINEAR)

    def _check_state(self, state: torch.Tensor):
        if not isinstance(state, torch.Tensor) or state.dim() != 5:
            raise ValueError("the state must be a [sample, tile, x, y, feature] tensor")
        check_cube_shape(state.shape)
        if state.shape[-1] != self.spec.n_features:
            raise ValueError(f"the state has {state.shape[-1]} features, the network needs {self.spec.n_features}")
        self.spec.check_grid(int(state.shape[2]))
        if state.dtype != torch.float32:
            raise TypeError(f"the normalised state must be float32, got {state.dtype}")
        _require_device(state)
        if state.shape[0] * 6 > 65535:
            raise ValueError(f"at most 10922 samples per call, got {state.shape[0]}")

    def step(self, state: torch.Tensor) -> torch.Tensor:
        """Normalised ``[S, 6, n, n, F]`` float32 -> the next normalised state, a new tensor."""
        self._check_state(state)
        state = state.contiguous()
        S, n, F = int(state.shape[0]), int(state.shape[2]), self.spec.n_features
        out = torch.empty_like(state)
        if S:
            self._forward(_Slice(state, F), _Slice(out, F), S, n)
        return out

    def rollout(self, state: torch.Tensor, timesteps: int) -> torch.Tensor:
        """``[S, 6, n, n, F]`` -> ``[S, timesteps + 1, 6, n, n, F]`` with the initial state at time 0.  Every step reads its
        input from, and writes its output to, the returned array: nothing is copied to the host or waited for."""
        self._check_state(state)
        if timesteps < 0:
            raise ValueError(f"timesteps must not be negative, got {timesteps}")
        S, n, F = int(state.shape[0]), int(state.shape[2]), self.spec.n_features
        out = torch.empty((S, timesteps + 1) + tuple(state.shape[1:]), dtype=torch.float32, device=state.device)
        out[:, 0].copy_(state)
        cube = 6 * n * n * F
        for i in range(timesteps if S else 0):
            self._forward(_Slice(out[:, i], F, 0, (timesteps + 1) * cube), _Slice(out[:, i + 1], F, 0, (timesteps + 1) * cube), S, n)
        return out

    # -- the scalers ---------------------------------------------------------------------------------
    def pack(self, sources: Sequence[torch.Tensor], n_windows: int, timesteps: int) -> torch.Tensor:
        """``sources[v]``: a ``[time, tile, x, y, level]`` view (any strides, float32 or float64) of state variable v ->
        normalised float32 ``[n_windows, timesteps + 1, 6, n, n, F]``, window w from times ``w * timesteps ...``."""
        return self._packer.pack(sources, n_windows, timesteps + 1, timesteps)

    def unpack(self, state: torch.Tensor) -> List[torch.Tensor]:
        """Normalised float32 ``[..., 6, n, n, F]`` -> per variable float64 ``[..., 6, n, n, nfeat]``, ``x * std + mean``."""
        return self._packer.unpack(state)
