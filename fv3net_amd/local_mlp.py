"""The "dense-local" microphysics emulator: one MLP shared by all levels, applied to every
(level, column) point -- the architecture of the reference's production gscond regressor and of its
classifier (projects/microphysics/configs/models/gscond.yaml:28-33, classifier.yaml:24-28;
external/fv3fit/fv3fit/emulation/layers/architecture.py:518-527: ``combine_sequence_inputs`` ->
``MLPBlock`` -> ``RNNOutput(share_conv_weights=True)``, i.e. kernel-size-1 convolutions).

``LocalMlpSpec`` describes the saved model's whole graph: the forward tensor transforms the reference
bakes into the SavedModel (log inputs), the per-level input normalisation (``FieldInput``), the
network, the per-level output de-normalisation (``FieldOutput``) and the backward transforms
(``ConditionallyScaledTransform.backward``, ``Difference.backward``).  ``LocalMlpModel`` runs it as
three device steps: ``fv3hip_local_pack`` per input -> ``fv3hip_mlp_predict`` on the packed
``[n_inputs][nz * ncol]`` array (a point is a sample) -> ``fv3hip_local_unpack`` per output channel.
"""
import dataclasses
from typing import Callable, Dict, List, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .mlp import InputSpec, MlpModel, MlpSpec, OutputSpec, _dtype_code, _unique, resolve_arithmetic
from .ops import _ptr, _require_device, _stream, device_info


@dataclasses.dataclass
class LocalInput:
    """One network input: array ``source`` ([nz, ncol], or [ncol] / [1, ncol] broadcast over the levels),
    optionally ``log(max(x, eps))``, then ``(x - center[z]) / scale[z]``.  ``name`` is the network's
    input name: inputs are concatenated sorted by it (architecture.py:53-75)."""

    name: str
    source: str
    transform: str = "none"  # "none" | "log"
    eps: float = 0.0
    center: Optional[np.ndarray] = None  # scalar or [nz]; None = 0
    scale: Optional[np.ndarray] = None   # scalar or [nz]; None = 1


@dataclasses.dataclass
class ConditionalScale:
    """ConditionallyScaledTransform.backward (transforms.py:219-224): ``name = y * max(scale(on), min_scale)
    + center(on)`` with ``scale``/``center`` piecewise constant in ``on`` over ``edges`` (left edges of the bins)."""

    name: str
    on: str
    edges: np.ndarray   # [n_bins]
    scale: np.ndarray   # [n_bins]
    center: np.ndarray  # [n_bins]
    min_scale: float = 0.0


@dataclasses.dataclass
class LocalOutput:
    """One output variable with ``channels`` values per point.  channels == 1: ``[nz, ncol]`` fields,
    de-normalised per level, optionally un-scaled conditionally and/or added to ``before``
    (Difference.backward, ``after = before + difference``).  channels > 1 (classifier logits):
    ``[channels, nz, ncol]``, unscaled."""

    name: str
    channels: int = 1
    scale: Optional[np.ndarray] = None   # scalar or [nz]
    center: Optional[np.ndarray] = None
    conditional: Optional[ConditionalScale] = None
    after: Optional[str] = None          # name of the Difference's `after` output
    before: Optional[str] = None         # source array the difference is added to
    # LimitValueTransform.backward (transforms.py:131-158) on the value the Difference adds (the conditionally
    # un-scaled one if configured, else the output itself) and on `after`: (lower, upper), None = no bound
    value_limit: Tuple[Optional[float], Optional[float]] = (None, None)
    after_limit: Tuple[Optional[float], Optional[float]] = (None, None)
    single_level: bool = False           # RNN architectures: a [1, ncol] output read off the last (surface) step


# -- what the three spec classes share: the input-order rule and the flat (yaml meta, npz arrays) form of their lists ------

def _check_input_order(inputs: List[LocalInput]) -> None:
    if [i.name for i in inputs] != sorted(i.name for i in inputs):
        raise ValueError("inputs must be listed sorted by their network name (combine_sequence_inputs)")


def _tables_to_arrays(item, prefix: str, arrays: Dict[str, np.ndarray]) -> None:
    for key in ("center", "scale"):
        if getattr(item, key) is not None:
            arrays[f"{prefix}_{key}"] = np.atleast_1d(np.asarray(getattr(item, key), np.float32))


def _inputs_to_arrays(inputs: List[LocalInput], arrays: Dict[str, np.ndarray]) -> list:
    """The meta's ``inputs`` list; the tables go into ``arrays`` (``in{n}_center``, ``in{n}_scale``)."""
    for n, i in enumerate(inputs):
        _tables_to_arrays(i, f"in{n}", arrays)
    return [{"name": i.name, "source": i.source, "transform": i.transform, "eps": float(i.eps)} for i in inputs]


def _inputs_from_arrays(meta: list, arrays: Mapping[str, np.ndarray]) -> List[LocalInput]:
    return [LocalInput(name=m["name"], source=m["source"], transform=m.get("transform", "none"), eps=float(m.get("eps", 0.0)),
                       center=arrays.get(f"in{n}_center"), scale=arrays.get(f"in{n}_scale")) for n, m in enumerate(meta)]


def _outputs_to_arrays(outputs: List[LocalOutput], arrays: Dict[str, np.ndarray]) -> list:
    """The meta's ``outputs`` list; the tables go into ``arrays`` (``out{n}_center``, ``out{n}_scale``, ``out{n}_cs_*``)."""
    meta = []
    for n, o in enumerate(outputs):
        m = {"name": o.name, "channels": int(o.channels), "after": o.after, "before": o.before,
             "value_limit": [None if v is None else float(v) for v in o.value_limit],
             "after_limit": [None if v is None else float(v) for v in o.after_limit], "single_level": bool(o.single_level)}
        _tables_to_arrays(o, f"out{n}", arrays)
        if o.conditional is not None:
            c = o.conditional
            m["conditional"] = {"name": c.name, "on": c.on, "min_scale": float(c.min_scale)}
            for key in ("edges", "scale", "center"):
                arrays[f"out{n}_cs_{key}"] = np.asarray(getattr(c, key), np.float32)
        meta.append(m)
    return meta


def _outputs_from_arrays(meta: list, arrays: Mapping[str, np.ndarray]) -> List[LocalOutput]:
    outputs = []
    for n, m in enumerate(meta):
        cond = None
        if m.get("conditional"):
            c = m["conditional"]
            cond = ConditionalScale(name=c["name"], on=c["on"], min_scale=float(c.get("min_scale", 0.0)),
                                    **{key: np.asarray(arrays[f"out{n}_cs_{key}"]) for key in ("edges", "scale", "center")})
        outputs.append(LocalOutput(name=m["name"], channels=int(m.get("channels", 1)), scale=arrays.get(f"out{n}_scale"),
                                   center=arrays.get(f"out{n}_center"), conditional=cond, after=m.get("after"),
                                   before=m.get("before"), value_limit=tuple(m.get("value_limit") or (None, None)),
                                   after_limit=tuple(m.get("after_limit") or (None, None)),
                                   single_level=bool(m.get("single_level", False))))
    return outputs


@dataclasses.dataclass
class LocalMlpSpec:
    inputs: List[LocalInput]            # in the network's (sorted-by-name) order
    hidden_kernels: List[np.ndarray]    # Keras layout [in, out]
    hidden_biases: List[np.ndarray]
    outputs: List[LocalOutput]
    out_kernel: np.ndarray              # [width, sum(channels)]
    out_bias: np.ndarray
    architecture = "dense-local"

    @property
    def sources(self) -> List[str]:
        names = [i.source for i in self.inputs]
        for o in self.outputs:
            if o.conditional is not None:
                names.append(o.conditional.on)
            if o.before is not None:
                names.append(o.before)
        return _unique(names)

    @property
    def output_names(self) -> List[str]:
        names = []
        for o in self.outputs:
            names.append(o.name)
            if o.conditional is not None:
                names.append(o.conditional.name)
            if o.after is not None:
                names.append(o.after)
        return names

    @property
    def n_channels(self) -> int:
        return sum(o.channels for o in self.outputs)

    def validate(self):
        _check_input_order(self.inputs)
        if not self.hidden_kernels or len(self.hidden_kernels) != len(self.hidden_biases):
            raise ValueError("at least one hidden layer, one bias per kernel")
        if int(self.hidden_kernels[0].shape[0]) != len(self.inputs):
            raise ValueError(f"first kernel has {self.hidden_kernels[0].shape[0]} rows, the model has {len(self.inputs)} inputs")
        w = int(self.hidden_kernels[0].shape[1])
        if tuple(self.out_kernel.shape) != (w, self.n_channels) or tuple(self.out_bias.shape) != (self.n_channels,):
            raise ValueError(f"output kernel has shape {self.out_kernel.shape}, expected {(w, self.n_channels)}")
        for o in self.outputs:
            if o.channels != 1 and (o.conditional is not None or o.after is not None or o.scale is not None):
                raise ValueError(f"multi-channel output {o.name!r} must be unscaled")
            if (o.after is None) != (o.before is None):
                raise ValueError(f"output {o.name!r}: 'after' and 'before' go together")

    # -- flat (yaml meta, npz arrays) serialisation ------------------------------------------
    def to_arrays(self) -> Tuple[dict, Dict[str, np.ndarray]]:
        arrays: Dict[str, np.ndarray] = {}
        meta = {"architecture": self.architecture, "inputs": _inputs_to_arrays(self.inputs, arrays),
                "outputs": _outputs_to_arrays(self.outputs, arrays), "n_hidden": len(self.hidden_kernels)}
        for n, (kern, b) in enumerate(zip(self.hidden_kernels, self.hidden_biases)):
            arrays[f"hidden{n}_kernel"] = np.asarray(kern, np.float32)
            arrays[f"hidden{n}_bias"] = np.asarray(b, np.float32)
        arrays["out_kernel"] = np.asarray(self.out_kernel, np.float32)
        arrays["out_bias"] = np.asarray(self.out_bias, np.float32)
        return meta, arrays

    @classmethod
    def from_arrays(cls, meta: Mapping, arrays: Mapping[str, np.ndarray]) -> "LocalMlpSpec":
        nh = int(meta["n_hidden"])
        return cls(inputs=_inputs_from_arrays(meta["inputs"], arrays),
                   hidden_kernels=[np.asarray(arrays[f"hidden{n}_kernel"]) for n in range(nh)],
                   hidden_biases=[np.asarray(arrays[f"hidden{n}_bias"]) for n in range(nh)],
                   outputs=_outputs_from_arrays(meta["outputs"], arrays),
                   out_kernel=np.asarray(arrays["out_kernel"]), out_bias=np.asarray(arrays["out_bias"]))


@dataclasses.dataclass
class RnnLayer:
    """One ``tf.keras.layers.SimpleRNN(channels, activation='relu', return_sequences=True)``:
    ``h_t = relu(x_t @ kernel + h_{t-1} @ recurrent_kernel + bias)``, ``h_{-1} = 0``."""

    kernel: np.ndarray            # [in, channels]
    recurrent_kernel: np.ndarray  # [channels, channels]
    bias: np.ndarray              # [channels]

    def check(self, fan: int, what: str) -> int:
        """Refuse shapes that do not fit ``fan`` inputs; returns the channel count (the fan-in of what follows)."""
        ch = int(self.kernel.shape[1])
        if tuple(self.kernel.shape) != (fan, ch) or tuple(self.recurrent_kernel.shape) != (ch, ch) or tuple(self.bias.shape) != (ch,):
            raise ValueError(f"{what}: kernel {self.kernel.shape}, recurrent kernel {self.recurrent_kernel.shape}, "
                             f"bias {self.bias.shape} do not fit {fan} inputs")
        return ch

    def to_arrays(self, prefix: str, arrays: Dict[str, np.ndarray]) -> None:
        for key in ("kernel", "recurrent_kernel", "bias"):
            arrays[f"{prefix}_{key}"] = np.asarray(getattr(self, key), np.float32)

    @classmethod
    def from_arrays(cls, prefix: str, arrays: Mapping[str, np.ndarray]) -> "RnnLayer":
        return cls(*[np.asarray(arrays[f"{prefix}_{key}"]) for key in ("kernel", "recurrent_kernel", "bias")])


@dataclasses.dataclass
class RnnSpec:
    """The "rnn-v1-shared-weights" / "rnn-v1" architecture -- the reference's production precpd emulator
    (projects/microphysics/configs/models/precpd.yaml:36-41; architecture.py:149-226 ``RNNBlock``: stacked
    SimpleRNNs that recurse over the levels from the model top (last index) to the surface (index 0), then
    ``RNNOutput`` kernel-size-1 convolutions; single-level outputs are read off the surface step,
    architecture.py:403-407).  Inputs and outputs are described as for ``LocalMlpSpec``."""

    inputs: List[LocalInput]
    layers: List[RnnLayer]
    outputs: List[LocalOutput]
    out_kernel: np.ndarray   # [channels, sum(output channels)]
    out_bias: np.ndarray
    architecture = "rnn-v1-shared-weights"

    sources = LocalMlpSpec.sources
    output_names = LocalMlpSpec.output_names
    n_channels = LocalMlpSpec.n_channels

    def validate(self):
        _check_input_order(self.inputs)
        if not self.layers:
            raise ValueError("at least one recurrent layer")
        fan = len(self.inputs)
        for n, layer in enumerate(self.layers):
            fan = layer.check(fan, f"recurrent layer {n}")
        if tuple(self.out_kernel.shape) != (fan, self.n_channels) or tuple(self.out_bias.shape) != (self.n_channels,):
            raise ValueError(f"output kernel has shape {self.out_kernel.shape}, expected {(fan, self.n_channels)}")
        for o in self.outputs:
            if o.channels != 1:
                raise ValueError("multi-channel outputs are not supported by the RNN architectures here")
            if (o.after is None) != (o.before is None):
                raise ValueError(f"output {o.name!r}: 'after' and 'before' go together")
            if o.single_level and (o.conditional is not None or o.after is not None):
                raise ValueError(f"single-level output {o.name!r} cannot carry level-wise transforms")

    def to_arrays(self) -> Tuple[dict, Dict[str, np.ndarray]]:
        arrays: Dict[str, np.ndarray] = {}
        meta = {"architecture": self.architecture, "inputs": _inputs_to_arrays(self.inputs, arrays),
                "outputs": _outputs_to_arrays(self.outputs, arrays), "n_hidden": 0, "n_rnn": len(self.layers)}
        arrays["out_kernel"] = np.asarray(self.out_kernel, np.float32)
        arrays["out_bias"] = np.asarray(self.out_bias, np.float32)
        for n, layer in enumerate(self.layers):
            layer.to_arrays(f"rnn{n}", arrays)
        return meta, arrays

    @classmethod
    def from_arrays(cls, meta: Mapping, arrays: Mapping[str, np.ndarray]) -> "RnnSpec":
        return cls(inputs=_inputs_from_arrays(meta["inputs"], arrays),
                   layers=[RnnLayer.from_arrays(f"rnn{n}", arrays) for n in range(int(meta["n_rnn"]))],
                   outputs=_outputs_from_arrays(meta["outputs"], arrays),
                   out_kernel=np.asarray(arrays["out_kernel"]), out_bias=np.asarray(arrays["out_bias"]))


@dataclasses.dataclass
class HybridRnnSpec:
    """The "rnn" architecture (architecture.py:78-147 ``HybridRNN``, key "rnn" at :453-461):
    ``combine_sequence_inputs`` -> one ``SimpleRNN(channels, activation, go_backwards)`` that returns only its FINAL
    state -> ``MLPBlock(dense_width, dense_depth)`` -> ``StandardOutput`` dense heads (whole-column outputs).

    ``head`` describes everything after the recurrence as an ``MlpSpec`` whose one network input is the source
    ``STATE`` (``channels`` features, unnormalised); its outputs carry the per-level de-normalisation, limits and
    residuals (``Difference.backward``) like a "dense" emulator's, residual sources being ``[nz, ncol]`` arrays of the
    call.  ``dense_depth = 0`` is a head without hidden layers."""

    STATE = "rnn_state"
    inputs: List[LocalInput]
    rnn: RnnLayer
    head: MlpSpec
    go_backwards: bool = True   # recurse from the last index (the model top in the physics' arrays) to index 0
    architecture = "rnn"

    @property
    def sources(self) -> List[str]:
        return _unique([i.source for i in self.inputs] + [r.source for r in self.head.residuals])

    @property
    def output_names(self) -> List[str]:
        return self.head.output_names

    def validate(self):
        _check_input_order(self.inputs)
        ch = self.rnn.check(len(self.inputs), "recurrent layer")
        if [(i.source, i.nfeat, i.start) for i in self.head.inputs] != [(self.STATE, ch, 0)]:
            raise ValueError(f"the head's only input must be the {ch} features of {self.STATE!r}")
        if self.head.hidden_output:
            raise ValueError("the head returns outputs, not its hidden layer")
        if any(r.source == self.STATE for r in self.head.residuals):
            raise ValueError("a residual cannot be added to the recurrent state")
        self.head.validate()

    def to_arrays(self) -> Tuple[dict, Dict[str, np.ndarray]]:
        head_meta, head_arrays = self.head.to_arrays()
        arrays = {f"head_{k}": v for k, v in head_arrays.items()}
        meta = {"architecture": self.architecture, "go_backwards": bool(self.go_backwards), "head": head_meta,
                "inputs": _inputs_to_arrays(self.inputs, arrays)}
        self.rnn.to_arrays("rnn", arrays)
        return meta, arrays

    @classmethod
    def from_arrays(cls, meta: Mapping, arrays: Mapping[str, np.ndarray]) -> "HybridRnnSpec":
        head = MlpSpec.from_arrays(meta["head"], {k[len("head_"):]: v for k, v in arrays.items() if k.startswith("head_")})
        return cls(inputs=_inputs_from_arrays(meta["inputs"], arrays), rnn=RnnLayer.from_arrays("rnn", arrays), head=head,
                   go_backwards=bool(meta.get("go_backwards", True)))


def _cell_spec(layer: RnnLayer, out_kernel: Optional[np.ndarray] = None, out_bias: Optional[np.ndarray] = None) -> MlpSpec:
    """A SimpleRNN cell as a fused-MLP model: one hidden layer ``relu([in, rec] @ [kernel; recurrent_kernel] + bias)`` that
    is returned as the hidden output "h" (the new state).  With ``out_kernel`` / ``out_bias`` the launch also applies that
    output layer to the new state (output "y"); without, the model has no outputs."""
    fan, ch = int(layer.kernel.shape[0]), int(layer.kernel.shape[1])
    last = out_kernel is not None
    return MlpSpec(
        inputs=[InputSpec("in", fan), InputSpec("rec", ch)],
        hidden_kernels=[np.concatenate([layer.kernel, layer.recurrent_kernel], axis=0).astype(np.float32)],
        hidden_biases=[np.asarray(layer.bias, np.float32)], outputs=[OutputSpec("y", int(out_kernel.shape[1]))] if last else [],
        out_kernel=np.asarray(out_kernel, np.float32) if last else np.zeros((ch, 0), np.float32),
        out_bias=np.asarray(out_bias, np.float32) if last else np.zeros(0, np.float32), hidden_output="h")


def _state_pair(width: int, ncol: int, dev) -> List[torch.Tensor]:
    """The ping-pong buffers of one recurrent layer's state: [h_{-1} = 0, not yet written]."""
    return [torch.zeros((width, ncol), dtype=torch.float32, device=dev), torch.empty((width, ncol), dtype=torch.float32, device=dev)]


def _per_level(values, nz: int, default: float, what: str) -> np.ndarray:
    if values is None:
        return np.full(nz, default, np.float32)
    a = np.atleast_1d(np.asarray(values, np.float32))
    if a.shape == (1,):
        return np.full(nz, a[0], np.float32)
    if a.shape != (nz,):
        raise ValueError(f"{what} has {a.shape[0]} levels, the state has {nz}")
    return np.ascontiguousarray(a)


class _PointModel:
    """What the dense-local and the RNN models share: source checks, the pack pass, the unpack pass, and for the RNN models
    the replay of their level sweep as a HIP graph."""

    def __init__(self, spec, device):
        spec.validate()
        self.spec = spec
        self.device = torch.device(device)
        self._tables: Dict[Tuple[str, int], torch.Tensor] = {}
        self._graphs: Dict[Tuple[int, int], tuple] = {}  # (nz, ncol) -> (graph, its static buffers); one shape at a time
        self._n_cu: Optional[int] = None

    def _table(self, key: str, values, nz: Optional[int], default: float = 0.0) -> torch.Tensor:
        """Small per-level / per-bin float tables, uploaded once per (table, nz)."""
        ck = (key, -1 if nz is None else nz)
        if ck not in self._tables:
            a = np.ascontiguousarray(np.asarray(values, np.float32)) if nz is None else _per_level(values, nz, default, key)
            self._tables[ck] = torch.from_numpy(a).to(self.device)
        return self._tables[ck]

    def _gather(self, sources: Mapping[str, torch.Tensor]):
        arrs: Dict[str, torch.Tensor] = {}
        nz = ncol = None
        for name in self.spec.sources:
            t = sources[name]
            if t.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"source {name!r} must be float32 or float64, got {t.dtype}")
            if t.dim() == 1:
                t = t.unsqueeze(0)
            if t.dim() != 2:
                raise ValueError(f"source {name!r} must be [nz, ncol] or [ncol], got shape {tuple(t.shape)}")
            if ncol is None:
                ncol = int(t.shape[1])
            elif int(t.shape[1]) != ncol:
                raise ValueError("sources differ in their number of columns")
            if t.shape[0] != 1:
                if nz is None:
                    nz = int(t.shape[0])
                elif int(t.shape[0]) != nz:
                    raise ValueError("sources differ in their number of levels")
            arrs[name] = t.contiguous()
        nz = 1 if nz is None else nz
        for o in getattr(self.spec, "outputs", ()):
            for need in ([o.conditional.on] if o.conditional else []) + ([o.before] if o.before else []):
                if arrs[need].shape[0] != nz:
                    raise ValueError(f"source {need!r} must have {nz} levels")
        return arrs, nz, ncol, _require_device(*arrs.values())

    def _pack(self, arrs, nz: int, ncol: int, dev) -> torch.Tensor:
        x = torch.empty((len(self.spec.inputs), nz * ncol), dtype=torch.float32, device=dev)
        self._pack_into(arrs, nz, ncol, dev, x)
        return x

    def _pack_into(self, arrs, nz: int, ncol: int, dev, x: torch.Tensor) -> None:
        for n, i in enumerate(self.spec.inputs):
            t = arrs[i.source]
            _lib.call_on(dev, "fv3hip_local_pack", _ptr(t), _dtype_code(t.dtype), int(t.shape[0] != 1),
                      _lib.TRANSFORM_LOG if i.transform == "log" else _lib.TRANSFORM_NONE, float(i.eps),
                      _ptr(self._table(f"in{n}_center", i.center, nz, 0.0)), _ptr(self._table(f"in{n}_scale", i.scale, nz, 1.0)),
                      nz, ncol, _ptr(x[n]), _stream(dev))

    def _unpack_one(self, n: int, o: LocalOutput, rows: torch.Tensor, level_stride: int, arrs, nz: int, ncol: int, dev,
                    out: Dict[str, torch.Tensor]) -> None:
        """Output ``o`` (index ``n``) from its network rows (level z at ``rows + z * level_stride``)."""
        direct = torch.empty((nz, ncol), dtype=torch.float32, device=dev)
        cond, unscaled, after = o.conditional, None, None
        cond_args = [None, 0, None, None, None, 0, 0.0]
        if cond is not None:
            unscaled = torch.empty_like(direct)
            on = arrs[cond.on]
            cond_args = [_ptr(on), _dtype_code(on.dtype), _ptr(self._table(f"out{n}_cs_edges", cond.edges, None)),
                         _ptr(self._table(f"out{n}_cs_scale", cond.scale, None)),
                         _ptr(self._table(f"out{n}_cs_center", cond.center, None)), int(len(cond.edges)), float(cond.min_scale)]
        before_args = [None, 0]
        if o.before is not None:
            after = torch.empty_like(direct)
            before_args = [_ptr(arrs[o.before]), _dtype_code(arrs[o.before].dtype)]
        bounds = list(o.value_limit) + list(o.after_limit)
        flags = sum(1 << b for b, v in enumerate(bounds) if v is not None)
        _lib.call_on(dev, "fv3hip_local_unpack", _ptr(rows), int(level_stride),
                  _ptr(self._table(f"out{n}_scale", o.scale, nz, 1.0)) if o.scale is not None else None,
                  _ptr(self._table(f"out{n}_center", o.center, nz, 0.0)) if o.center is not None else None,
                  *cond_args, *before_args, flags, *[0.0 if v is None else float(v) for v in bounds], nz, ncol,
                  _ptr(direct), _ptr(unscaled), _ptr(after), _stream(dev))
        out[o.name] = direct
        if cond is not None:
            out[cond.name] = unscaled
        if o.after is not None:
            out[o.after] = after

    def _leaves_cus_idle(self, ncol: int) -> bool:
        """Fewer than ~128 columns per CU: the launches of one recurrent layer leave most of the chip idle."""
        if self._n_cu is None:
            self._n_cu = int(device_info()["compute_units"])
        return ncol < 128 * self._n_cu

    def _graphed(self, key: Tuple[int, int], arrs, dev, buffers: Callable[[], tuple], sweep: Callable[..., object]) -> tuple:
        """The level sweep of a call of shape ``key`` = (nz, ncol) as the replay of a HIP graph (bit-identical to the eager
        launches).  ``buffers()`` allocates the graph's static buffers, ``(x, state pairs, ...)``: the packed input, one
        ``_state_pair`` per recurrent layer, whatever else the sweep writes; ``sweep(*buffers)`` launches the recurrence.
        The first call of a shape packs, sweeps once eagerly on the current stream (the kernels' one-time allocations happen
        there; the side streams a pipelined sweep creates are the ones the capture then records as parallel branches),
        synchronises, and captures the zeroing of the first state buffers followed by the sweep.  Every call packs into
        ``x`` and replays.  Returns the static buffers: valid until the next call, the caller consumes them before it
        returns."""
        nz, ncol = key
        entry = self._graphs.get(key)
        if entry is None:
            self._graphs.clear()  # one shape at a time: the static buffers of another shape are released
            bufs = buffers()
            self._pack_into(arrs, nz, ncol, dev, bufs[0])
            sweep(*bufs)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for pair in bufs[1]:
                    pair[0].zero_()
                sweep(*bufs)
            entry = self._graphs[key] = (graph, bufs)
        graph, bufs = entry
        self._pack_into(arrs, nz, ncol, dev, bufs[0])
        graph.replay()
        return bufs


class LocalMlpModel(_PointModel):
    """Device handle of a dense-local emulator."""

    def __init__(self, spec: LocalMlpSpec, device="cuda", arithmetic: Optional[str] = None):
        """``arithmetic``: "fp32" (the product kernel) or "split-bf16" (opt-in, experimental: the network on the bf16 matrix
        cores with every operand split into three bf16 pieces, csrc/mlp_bf16x3.hip); default: the environment variable
        ``mlp.ARITHMETIC_ENV``, else "fp32" (``mlp.resolve_arithmetic``).  A network the split kernel does not implement
        raises here."""
        super().__init__(spec, device)
        k, c = len(spec.inputs), spec.n_channels
        self.arithmetic, inner_cls = resolve_arithmetic(arithmetic)
        self._inner = inner_cls(MlpSpec(
            inputs=[InputSpec("X", k)], hidden_kernels=spec.hidden_kernels, hidden_biases=spec.hidden_biases,
            outputs=[OutputSpec("Y", c)], out_kernel=spec.out_kernel, out_bias=spec.out_bias), device=self.device)
        self.flops_per_point = self._inner.flops_per_sample

    def predict(self, sources: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """``sources``: name -> device array ``[nz, ncol]`` (or ``[ncol]`` / ``[1, ncol]``), float32 or float64.
        Returns name -> float32 ``[nz, ncol]`` (``[channels, nz, ncol]`` for multi-channel outputs)."""
        arrs, nz, ncol, dev = self._gather(sources)
        x = self._pack(arrs, nz, ncol, dev)
        y = self._inner.predict({"X": x})["Y"]  # [sum(channels), nz * ncol]
        del x
        out: Dict[str, torch.Tensor] = {}
        row = 0
        for n, o in enumerate(self.spec.outputs):
            rows = y[row:row + o.channels]
            row += o.channels
            if o.channels != 1:
                out[o.name] = rows.reshape(o.channels, nz, ncol)
            else:
                self._unpack_one(n, o, rows, ncol, arrs, nz, ncol, dev, out)
        return out


class RnnModel(_PointModel):
    """Device handle of an RNN emulator.  Every SimpleRNN step of every layer is one launch of the fused MLP
    kernel over all columns: hidden layer = the cell, ``relu([x_t, h_{t-1}] @ [kernel; recurrent_kernel] + bias)``,
    returned as the launch's hidden output (the new state); the last layer's launch also applies the output
    convolutions, whose rows go straight into the level's slice of the output array.  79 levels x depth launches
    per call, each with ``ncol`` samples; the states ping-pong between two buffers per layer."""

    def __init__(self, spec: RnnSpec, device="cuda", use_graph: Optional[bool] = None, arithmetic: Optional[str] = None):
        """``arithmetic``: as for ``LocalMlpModel`` ("fp32" / opt-in "split-bf16"; default from the environment)."""
        super().__init__(spec, device)
        self.arithmetic, cell_cls = resolve_arithmetic(arithmetic)
        # ``use_graph``: capture the level sweep (nz x depth launches) once per (nz, ncol) into a HIP graph on static
        # buffers and replay it (bit-identical).  None = where it pays: the column counts of one model rank, whose launches
        # are ~20-40 us each on the feature-split kernel -- 158 of them cost more host time than device time when launched
        # one by one (3.9 ms replayed against 5.3 ms eager at 2 304 columns) -- and not for snapshot-sized calls, where a
        # launch lasts milliseconds.  (Round 2 measured no gain at all: a step was then bound by the ~60 us one 128-sample
        # tile needs on each of the 18 CUs it occupied.)
        self._use_graph = use_graph
        last = len(spec.layers) - 1
        self._cells: List[MlpModel] = [
            cell_cls(_cell_spec(layer, spec.out_kernel, spec.out_bias) if n == last else _cell_spec(layer), device=self.device)
            for n, layer in enumerate(spec.layers)]
        self.flops_per_point = sum(m.flops_per_sample for m in self._cells)

    def predict(self, sources: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """As ``LocalMlpModel.predict``; single-level outputs come back as ``[1, ncol]``."""
        spec = self.spec
        arrs, nz, ncol, dev = self._gather(sources)
        k, c = len(spec.inputs), spec.n_channels
        # (column counts that leave most CUs idle: the layers on a stream each, layer n + 1 of level z beside layer n of
        # level z - 1; a capture records the side streams' work as parallel branches of the graph)
        idle = self._leaves_cus_idle(ncol)
        use_graph = self._use_graph if self._use_graph is not None else (self.arithmetic == "fp32" and idle)
        if use_graph:
            def buffers():
                x = torch.empty((k, nz, ncol), dtype=torch.float32, device=dev)
                y = torch.empty((c, nz, ncol), dtype=torch.float32, device=dev)
                return x, self._new_states(ncol, dev), y

            x, _, y = self._graphed((nz, ncol), arrs, dev, buffers, lambda x, states, y: self._sweep(x, y, states, nz, pipelined=idle))
        else:
            x = self._pack(arrs, nz, ncol, dev).view(k, nz, ncol)
            y = torch.empty((c, nz, ncol), dtype=torch.float32, device=dev)
            self._sweep(x, y, self._new_states(ncol, dev), nz, pipelined=idle)
        del x
        out: Dict[str, torch.Tensor] = {}
        for n, o in enumerate(spec.outputs):
            if o.single_level:  # the surface step holds the whole column's information (architecture.py:403-407)
                self._unpack_one(n, o, y[n, 0], ncol, arrs, 1, ncol, dev, out)
            else:
                self._unpack_one(n, o, y[n], ncol, arrs, nz, ncol, dev, out)
        return out

    def _new_states(self, ncol: int, dev):
        return [_state_pair(m.spec.width, ncol, dev) for m in self._cells]

    def _sweep(self, x: torch.Tensor, y: torch.Tensor, states, nz: int, pipelined: bool = False) -> None:
        """The recurrence, from the model top (last index) to the surface.  ``pipelined`` (column counts that leave most
        CUs idle): a wavefront over (layer, level) -- at tick t layer n works on step t - n, all layers of a tick side by
        side on a stream each, joined before the next tick.  Fork / join by ``wait_stream`` only, which a HIP-graph capture
        records as parallel branches (per-step events across three streams crashed the runtime's capture_end).  Hazards: the
        state ping-pong buffers -- layer n reads at step s what layer n - 1 wrote at step s (the tick before: joined), and the
        layers of one tick touch different halves of every pair (layer n - 1 writes [cur(s)] while layer n reads [nxt(s)])."""
        depth = len(self._cells)

        def cell(n: int, step: int):
            z = nz - 1 - step
            cur, nxt = step & 1, (step & 1) ^ 1
            below = x[:, z] if n == 0 else states[n - 1][nxt]
            outs = {"h": states[n][nxt]}
            if n == depth - 1:
                outs["y"] = y[:, z]
            self._cells[n].predict({"in": below, "rec": states[n][cur]}, out=outs)

        if not (pipelined and depth > 1):
            for step in range(nz):
                for n in range(depth):
                    cell(n, step)
            return
        dev = x.device
        main = torch.cuda.current_stream(dev)
        if not hasattr(self, "_streams"):
            self._streams = [torch.cuda.Stream(dev) for _ in range(depth - 1)]
        for tick in range(nz + depth - 1):
            active = [(n, tick - n) for n in range(depth) if 0 <= tick - n < nz]
            side = active[1:]
            for (n, step), st in zip(side, self._streams):
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    cell(n, step)
            cell(*active[0])
            for _, st in zip(side, self._streams):
                main.wait_stream(st)


class HybridRnnModel(_PointModel):
    """Device handle of a "rnn" (``HybridRnnSpec``) emulator: the pack pass, one fused-MLP launch per level for the
    recurrence (the cell is a hidden-output model without outputs: ``h_t = relu([x_t, h_{t-1}] @ [kernel;
    recurrent_kernel] + bias)``, the states ping-pong between two buffers), then ONE launch of the head on the final
    state, whose epilogue writes the de-normalised, limited outputs and the residual sums.  For the column counts of a
    model rank the level sweep is captured once per shape into a HIP graph and replayed (as ``RnnModel``)."""

    def __init__(self, spec: HybridRnnSpec, device="cuda", use_graph: Optional[bool] = None):
        super().__init__(spec, device)
        self._cell = MlpModel(_cell_spec(spec.rnn), device=self.device)
        self._head = MlpModel(spec.head, device=self.device)
        self._use_graph = use_graph
        self.flops_per_column_level = self._cell.flops_per_sample
        self.flops_per_column_head = self._head.flops_per_sample

    def _sweep(self, x: torch.Tensor, states, nz: int) -> torch.Tensor:
        order = range(nz - 1, -1, -1) if self.spec.go_backwards else range(nz)
        for step, z in enumerate(order):
            cur = step & 1
            self._cell.predict({"in": x[:, z], "rec": states[cur]}, out={"h": states[cur ^ 1]})
        return states[nz & 1]

    def predict(self, sources: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """``sources``: name -> device array ``[nz, ncol]`` (or ``[ncol]`` / ``[1, ncol]``); returns name -> float32
        ``[nfeat, ncol]``."""
        spec = self.spec
        arrs, nz, ncol, dev = self._gather(sources)
        k, ch = len(spec.inputs), self._cell.spec.width
        use_graph = self._use_graph if self._use_graph is not None else self._leaves_cus_idle(ncol)
        if use_graph:
            _, (states,) = self._graphed(
                (nz, ncol), arrs, dev, lambda: (torch.empty((k, nz, ncol), dtype=torch.float32, device=dev), [_state_pair(ch, ncol, dev)]),
                lambda x, pairs: self._sweep(x, pairs[0], nz))
            final = states[nz & 1]
        else:
            x = self._pack(arrs, nz, ncol, dev).view(k, nz, ncol)
            final = self._sweep(x, _state_pair(ch, ncol, dev), nz)
        head_sources = {HybridRnnSpec.STATE: final}
        for r in spec.head.residuals:
            if arrs[r.source].dtype != torch.float32:  # (one source dtype per launch: the state is float32)
                arrs[r.source] = arrs[r.source].to(torch.float32)
            head_sources[r.source] = arrs[r.source]
        return self._head.predict(head_sources)
