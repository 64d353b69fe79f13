"""The full-model-replacement (FMR) recurrent generator: the arrays of fv3fit's ``"fmr"`` model and its device layer.

``RecurrentGeneratorSpec`` holds what ``RecurrentGeneratorConfig.build`` produces
(external/fv3fit/fv3fit/pytorch/recurrent/generator.py:185-400) as plain arrays in torch's own layouts.  With
``m = int(max_filters / 2**n_convolutions)``, ``C`` state channels, ``c_l = m 2**l`` on faces of ``n / 2**l`` cells per edge
and the context ``ctx`` = x, y, z of the bottom face's cells (``use_geographic_features``) followed by sin and cos of a 24-hour
clock (``samples_per_day``), the layers are

    encode   first        conv 7 x 7 of (x + input_bias || x, y, z at nx), C (+ 3) -> m; instance norm; ReLU
             down{l}      conv 4 x 4 stride 2, c_l -> c_{l+1}; instance norm; ReLU       l = 0 ... n_convolutions - 1
    step     "resnet"     res{j}.a/.b  x + IN(conv k x k(ReLU(IN(conv k x k(x || ctx)))))   j = 0 ... n_resnet - 1
             "conv"       step.a/.b    ReLU(IN(conv k x k(ReLU(IN(conv k x k(x || ctx))))))
    decode   up{l}        ConvTranspose2d 4 x 4 stride 2 (halo 1, crop 3), c_{l+1} -> c_l; instance norm; ReLU
             last         conv 7 x 7, m -> C; + output_bias

``forward`` encodes once, decodes, and then steps and decodes ``ntime - 1`` times; the clock is at ``i - 1`` in step ``i`` and
restarts in every call.  ``RecurrentGeneratorModel`` runs the layers with the stateless ``fv3hip_cyclegan_*`` kernels on torch's
current stream.  The context is never stored with the latent: ``fv3hip_cyclegan_conv_context`` reads the per-cell table and the
clock's two numbers from where they lie.  DESIGN.md section 18.
"""
import ctypes
import dataclasses
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .cyclegan import (INSTANCE_NORM_EPS, KINDS, MAX_VARIABLES, REFERENCE_BATCH, _NONE, _Pending, _ptr, _Slice,
                       check_architecture, check_convolution_type, check_grid, split_transposed_weight, weight_shape)
from .graph import check_cube_shape
from .ops import _require_device, _stream

STEP_TYPES = ("resnet", "conv")
N_XYZ, N_CLOCK = 3, 2


def check_step_type(step_type: str):
    if step_type not in STEP_TYPES:
        raise ValueError(f"Unknown step type {step_type!r}, expected 'resnet' or 'conv'")


def check_filters(n_convolutions: int, max_filters: int):
    """The step layers have ``max_filters`` channels, the encoder hands them ``int(max_filters / 2**n) * 2**n``."""
    if int(max_filters / 2 ** int(n_convolutions)) * 2 ** int(n_convolutions) != max_filters:
        raise ValueError(f"max_filters = {max_filters} is no multiple of 2**{n_convolutions}: the encoder's last layer and the "
                         "step layers would differ in their channels")


def clock_table(samples_per_day: int) -> np.ndarray:
    """``[samples_per_day][2]``: ``float32(np.sin(2 pi k / spd))``, ``float32(np.cos(...))`` -- the float64 value rounded once,
    as assigning it into a float32 tensor rounds it (generator.py:149-152)."""
    k = np.arange(int(samples_per_day))
    return np.stack([np.sin(2 * np.pi * k / samples_per_day), np.cos(2 * np.pi * k / samples_per_day)], axis=1).astype(np.float32)


def layer_plan(channels: int, n_convolutions: int, n_resnet: int, kernel_size: int, max_filters: int, step_type: str,
               use_geographic_features: bool, samples_per_day: Optional[int]) -> List[Tuple[str, str, int, int, int, int]]:
    """(name, kind, c_in with the context channels, c_out, k, level of the OUTPUT) of every convolution: encode, one step, decode."""
    m, nc = int(max_filters / 2 ** n_convolutions), n_convolutions
    c = lambda l: m * 2 ** l
    xyz = N_XYZ if use_geographic_features else 0
    ctx = xyz + (N_CLOCK if samples_per_day is not None else 0)
    plan = [("first", "regular", channels + xyz, m, 7, 0)]
    plan += [(f"down{l}", "strided", c(l), c(l + 1), 4, l + 1) for l in range(nc)]
    for stem in ([f"res{j}" for j in range(n_resnet)] if step_type == "resnet" else ["step"]):
        plan += [(f"{stem}.a", "regular", c(nc) + ctx, c(nc), kernel_size, nc), (f"{stem}.b", "regular", c(nc), c(nc), kernel_size, nc)]
    plan += [(f"up{l}", "transposed", c(l + 1), c(l), 4, l) for l in reversed(range(nc))]
    return plan + [("last", "regular", m, channels, 7, 0)]


@dataclasses.dataclass
class RecurrentGeneratorSpec:
    """``weights[name]`` in torch's layout (context channels last along ``c_in``), ``biases[name]`` ``[c_out]``; the geographic
    biases ``[6, channels, nx, nx]`` (``None``: ``use_geographic_bias`` is off); ``xyz`` ``[6, 3, nx, nx]`` and ``xyz_bottom``
    ``[6, 3, nb, nb]`` with ``nb = nx >> n_convolutions`` (``None``: ``use_geographic_features`` is off), all float32.  The
    reference reads both grids from a catalogue; here they are data of the model."""

    channels: int
    nx: int
    weights: Dict[str, np.ndarray]
    biases: Dict[str, np.ndarray]
    n_convolutions: int = 3
    n_resnet: int = 3
    kernel_size: int = 3
    strided_kernel_size: int = 4
    max_filters: int = 256
    step_type: str = "resnet"
    samples_per_day: Optional[int] = None
    input_bias: Optional[np.ndarray] = None
    output_bias: Optional[np.ndarray] = None
    xyz: Optional[np.ndarray] = None
    xyz_bottom: Optional[np.ndarray] = None

    def __post_init__(self):
        self.validate()

    @property
    def use_geographic_bias(self) -> bool:
        return self.input_bias is not None

    @property
    def use_geographic_features(self) -> bool:
        return self.xyz is not None

    @property
    def min_filters(self) -> int:
        return int(self.max_filters / 2 ** self.n_convolutions)

    @property
    def nx_bottom(self) -> int:
        return self.nx >> self.n_convolutions

    @property
    def context_channels(self) -> Tuple[int, int]:
        """(per-cell, uniform) context channels of the step layers."""
        return (N_XYZ if self.use_geographic_features else 0, N_CLOCK if self.samples_per_day is not None else 0)

    @property
    def plan(self):
        return layer_plan(self.channels, self.n_convolutions, self.n_resnet, self.kernel_size, self.max_filters, self.step_type,
                          self.use_geographic_features, self.samples_per_day)

    @property
    def step_stems(self) -> List[str]:
        return [f"res{j}" for j in range(self.n_resnet)] if self.step_type == "resnet" else ["step"]

    def _flops(self, select) -> float:
        return float(sum(2 * (4 if kind == "transposed" else k * k) * ci * co * 6 * (self.nx >> level) ** 2
                         for name, kind, ci, co, k, level in self.plan if select(name)))

    def flops_per_step(self) -> float:
        """One time of the rollout after the first, per window: the step layers and the decoder (``2 taps c_in c_out`` per
        output cell, context channels included)."""
        return self._flops(lambda name: not (name == "first" or name.startswith("down")))

    def flops_decode(self) -> float:
        return self._flops(lambda name: name.startswith("up") or name == "last")

    def flops_encode(self) -> float:
        return self._flops(lambda name: name == "first" or name.startswith("down"))

    def validate(self):
        check_architecture(self.n_convolutions, self.n_resnet, self.kernel_size, self.strided_kernel_size, self.max_filters)
        check_step_type(self.step_type)
        check_filters(self.n_convolutions, self.max_filters)
        if self.channels < 1:
            raise ValueError(f"a generator needs at least one channel, got {self.channels}")
        if self.samples_per_day is not None and int(self.samples_per_day) < 1:
            raise ValueError(f"samples_per_day must be at least 1 (or None), got {self.samples_per_day}")
        check_grid(self.nx, self.nx, self.n_convolutions)
        plan = self.plan
        names = {p[0] for p in plan}
        if set(self.weights) != names or set(self.biases) != names:
            raise ValueError(f"weights {sorted(self.weights)} / biases {sorted(self.biases)} differ from the layers {sorted(names)}")
        for name, kind, ci, co, k, _ in plan:
            for what, a, shape in (("weight", self.weights[name], weight_shape(kind, ci, co, k)), ("bias", self.biases[name], (co,))):
                a = np.asarray(a)
                if a.shape != shape or a.dtype != np.float32:
                    raise ValueError(f"layer {name!r}: {what} has shape {a.shape} and dtype {a.dtype}, expected float32 {shape}")
        n, nb, C = self.nx, self.nx_bottom, self.channels
        if (self.input_bias is None) != (self.output_bias is None):
            raise ValueError("input_bias and output_bias come together (use_geographic_bias)")
        if (self.xyz is None) != (self.xyz_bottom is None):
            raise ValueError("xyz and xyz_bottom come together (use_geographic_features)")
        for what, a, shape in (("input_bias", self.input_bias, (6, C, n, n)), ("output_bias", self.output_bias, (6, C, n, n)),
                               ("xyz", self.xyz, (6, 3, n, n)), ("xyz_bottom", self.xyz_bottom, (6, 3, nb, nb))):
            if a is not None and (np.asarray(a).shape != shape or np.asarray(a).dtype != np.float32):
                raise ValueError(f"{what} has shape {np.asarray(a).shape} and dtype {np.asarray(a).dtype}, expected float32 {shape}")

    _OPTIONAL = ("input_bias", "output_bias", "xyz", "xyz_bottom")

    def to_arrays(self, prefix: str = ""):
        meta = {"channels": int(self.channels), "nx": int(self.nx), "n_convolutions": int(self.n_convolutions),
                "n_resnet": int(self.n_resnet), "kernel_size": int(self.kernel_size),
                "strided_kernel_size": int(self.strided_kernel_size), "max_filters": int(self.max_filters),
                "step_type": str(self.step_type),
                "samples_per_day": None if self.samples_per_day is None else int(self.samples_per_day),
                "use_geographic_bias": self.use_geographic_bias, "use_geographic_features": self.use_geographic_features}
        arrays = {}
        for name in self.weights:
            arrays[f"{prefix}{name}.weight"] = np.asarray(self.weights[name], np.float32)
            arrays[f"{prefix}{name}.bias"] = np.asarray(self.biases[name], np.float32)
        for key in self._OPTIONAL:
            if getattr(self, key) is not None:
                arrays[f"{prefix}{key}"] = np.asarray(getattr(self, key), np.float32)
        return meta, arrays

    @classmethod
    def from_arrays(cls, meta: Mapping, arrays: Mapping[str, np.ndarray], prefix: str = "") -> "RecurrentGeneratorSpec":
        check_architecture(meta["n_convolutions"], meta["n_resnet"], meta["kernel_size"], meta.get("strided_kernel_size", 4),
                           meta["max_filters"])
        check_step_type(meta["step_type"])
        spd = meta.get("samples_per_day")
        plan = layer_plan(int(meta["channels"]), int(meta["n_convolutions"]), int(meta["n_resnet"]), int(meta["kernel_size"]),
                          meta["max_filters"], meta["step_type"], bool(meta["use_geographic_features"]), spd)
        get = lambda key: np.asarray(arrays[prefix + key], np.float32)
        flags = {"input_bias": "use_geographic_bias", "output_bias": "use_geographic_bias", "xyz": "use_geographic_features",
                 "xyz_bottom": "use_geographic_features"}
        return cls(int(meta["channels"]), int(meta["nx"]), {p[0]: get(p[0] + ".weight") for p in plan},
                   {p[0]: get(p[0] + ".bias") for p in plan}, int(meta["n_convolutions"]), int(meta["n_resnet"]),
                   int(meta["kernel_size"]), int(meta.get("strided_kernel_size", 4)), meta["max_filters"], meta["step_type"],
                   None if spd is None else int(spd), **{key: get(key) if meta[flag] else None for key, flag in flags.items()})


@dataclasses.dataclass
class FullModelReplacementSpec:
    """The generator, the state variables ``(name, feature count)`` in the network's channel order, and per variable the
    scaler's float64 ``(mean, std)`` ``[nfeat]`` under the variable's own name (recurrent/reloadable.py:78-118)."""

    generator: RecurrentGeneratorSpec
    variables: List[Tuple[str, int]]
    scalers: Dict[str, Tuple[np.ndarray, np.ndarray]]
    convolution_type: str = "halo_conv2d"

    def __post_init__(self):
        self.variables = [(str(n), int(f)) for n, f in self.variables]
        self.validate()

    @property
    def state_variables(self) -> List[str]:
        return [n for n, _ in self.variables]

    @property
    def n_features(self) -> int:
        return sum(f for _, f in self.variables)

    def scaler_arrays(self) -> Tuple[np.ndarray, np.ndarray]:
        return (np.concatenate([self.scalers[n][0] for n, _ in self.variables]),
                np.concatenate([self.scalers[n][1] for n, _ in self.variables]))

    def validate(self):
        check_convolution_type(self.convolution_type)
        if not self.variables:
            raise ValueError("a full-model replacement needs at least one state variable")
        if len(self.variables) > MAX_VARIABLES:
            raise ValueError(f"at most {MAX_VARIABLES} state variables are supported, got {len(self.variables)}")
        if len(set(self.state_variables)) != len(self.variables):
            raise ValueError(f"a state variable is named twice: {self.state_variables}")
        self.generator.validate()
        if self.generator.channels != self.n_features:
            raise ValueError(f"the generator has {self.generator.channels} channels, the state variables {self.n_features} features")
        if set(self.scalers) != set(self.state_variables):
            raise ValueError(f"scalers {sorted(self.scalers)} differ from {sorted(self.state_variables)}")
        for name, nfeat in self.variables:
            mean, std = (np.asarray(v) for v in self.scalers[name])
            if nfeat < 1 or mean.shape != (nfeat,) or std.shape != (nfeat,) or mean.dtype != np.float64 or std.dtype != np.float64:
                raise ValueError(f"scaler {name}: mean and std must be float64 of shape ({nfeat},)")
            if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std != 0)):
                raise ValueError(f"scaler {name}: mean and std must be finite and std non-zero")

    def to_arrays(self):
        gen_meta, arrays = self.generator.to_arrays("generator.")
        meta = {"convolution_type": self.convolution_type, "variables": [{"name": n, "nfeat": f} for n, f in self.variables],
                "generator": gen_meta}
        for key, (mean, std) in self.scalers.items():
            arrays[f"scaler.{key}.mean"] = np.asarray(mean, np.float64)
            arrays[f"scaler.{key}.std"] = np.asarray(std, np.float64)
        return meta, arrays

    @classmethod
    def from_arrays(cls, meta: Mapping, arrays: Mapping[str, np.ndarray]) -> "FullModelReplacementSpec":
        check_convolution_type(meta["convolution_type"])
        variables = [(v["name"], int(v["nfeat"])) for v in meta["variables"]]
        scalers = {n: (np.asarray(arrays[f"scaler.{n}.mean"], np.float64), np.asarray(arrays[f"scaler.{n}.std"], np.float64))
                   for n, _ in variables}
        return cls(RecurrentGeneratorSpec.from_arrays(meta["generator"], arrays, "generator."), variables, scalers,
                   meta["convolution_type"])


class RecurrentGeneratorModel:
    """One recurrent generator on one device: the weights uploaded once in the kernels' layout (a layer that reads context
    channels as the source's rows and the context's rows), the two ``xyz`` tables and the clock table, and a workspace that is
    kept between calls.  Windows are worked through in chunks of at most ``max_chunk`` whose workspace stays within
    ``workspace_limit`` bytes; a window's result does not depend on the chunk it falls into."""

    def __init__(self, spec: RecurrentGeneratorSpec, convolution_type: str = "halo_conv2d", device="cuda",
                 workspace_limit: int = 2 << 30, max_chunk: int = REFERENCE_BATCH):
        spec.validate()
        self.spec = spec
        self.halo_mode = check_convolution_type(convolution_type)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("RecurrentGeneratorModel needs a 'cuda' (ROCm) device; there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if max_chunk < 1 or workspace_limit < 1:
            raise ValueError(f"max_chunk and workspace_limit must be positive, got {max_chunk}, {workspace_limit}")
        _lib.load()
        self.workspace_limit, self.max_chunk = int(workspace_limit), int(max_chunk)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)
        c_cell, c_uni = spec.context_channels
        self._layers = {p[0]: p for p in spec.plan}
        self._w, self._w_ctx, self._b = {}, {}, {}
        for name, kind, ci, co, k, _ in spec.plan:
            w = np.asarray(spec.weights[name])
            n_ctx = (c_cell if name == "first" else c_cell + c_uni) if name == "first" or name.endswith(".a") else 0
            if n_ctx:     # [k][k][c][c_out] for the source's channels and for the context's
                self._w_ctx[name] = up(w[:, ci - n_ctx:].transpose(2, 3, 1, 0))
                w = w[:, :ci - n_ctx]
            self._w[name] = up(split_transposed_weight(w) if kind == "transposed" else w.transpose(2, 3, 1, 0))
            self._b[name] = up(spec.biases[name])
        last = lambda a: None if a is None else up(np.asarray(a).transpose(0, 2, 3, 1))    # [6][n][n][c]
        self._input_bias, self._output_bias = last(spec.input_bias), last(spec.output_bias)
        self._xyz, self._xyz_bottom = last(spec.xyz), last(spec.xyz_bottom)
        self._clock = None if spec.samples_per_day is None else up(clock_table(spec.samples_per_day))
        self._ws: Dict[str, torch.Tensor] = {}
        self._ws_chunk = 0

    # -- workspace -----------------------------------------------------------------------------------
    def _buffers(self) -> Dict[str, Tuple[int, int]]:
        """name -> (cells per edge, channels) of every activation buffer of one window."""
        s = self.spec
        out = {f"raw{l}": (s.nx >> l, s.min_filters * 2 ** l) for l in range(s.n_convolutions + 1)}
        out.update({key: (s.nx_bottom, s.max_filters) for key in ("x", "a", "b")})
        return out

    def _stat_keys(self) -> Dict[str, int]:
        s = self.spec
        out = {"st:first": s.min_filters, "st:a": s.max_filters, "st:b": s.max_filters}
        for l in range(s.n_convolutions):
            out[f"st:down{l}"], out[f"st:up{l}"] = s.min_filters * 2 ** (l + 1), s.min_filters * 2 ** l
        return out

    def workspace_bytes_per_sample(self) -> int:
        return 4 * (sum(6 * n * n * c for n, c in self._buffers().values()) + sum(2 * 6 * c for c in self._stat_keys().values()))

    def chunk_size(self, n_samples: int) -> int:
        return max(1, min(self.max_chunk, self.workspace_limit // self.workspace_bytes_per_sample(), max(n_samples, 1)))

    def _workspace(self, chunk: int):
        if chunk > self._ws_chunk:
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
            self._ws = {key: new(chunk, 6, n, n, c) for key, (n, c) in self._buffers().items()}
            self._ws.update({key: new(2, chunk, 6, c) for key, c in self._stat_keys().items()})
            self._ws_chunk = chunk
        return self._ws

    # -- layer launches ------------------------------------------------------------------------------
    def _conv(self, name, src: _Slice, pend: _Pending, dst: _Slice, S, n_in, out_bias=None, ctx_cell=None, ctx_uniform: int = 0):
        """``ctx_uniform``: a device address (0: none).  A layer without context rows goes through the same entry point."""
        _, kind, ci, co, k, _ = self._layers[name]
        w_ctx = self._w_ctx.get(name)
        c_cell = 0 if ctx_cell is None else int(ctx_cell.shape[-1])
        c_uni = N_CLOCK if ctx_uniform else 0
        _lib.call_on(self.device, "fv3hip_cyclegan_conv_context", src.ptr, src.ld, src.off, src.stride, _ptr(pend.mean),
                     _ptr(pend.rstd), _ptr(pend.bias), int(pend.relu), self._w[name].data_ptr(), self._b[name].data_ptr(),
                     _ptr(out_bias), dst.ptr, dst.ld, dst.off, dst.stride, S, n_in, ci - c_cell - c_uni, co, KINDS[kind], k,
                     self.halo_mode, _ptr(ctx_cell), c_cell, ctx_uniform or None, c_uni, _ptr(w_ctx), _stream(self.device))

    def _stats(self, key, src: _Slice, S, n, c, relu=True) -> _Pending:
        st = self._ws[key]
        _lib.call_on(self.device, "fv3hip_cyclegan_stats", src.ptr, src.ld, src.off, src.stride, st[0].data_ptr(), st[1].data_ptr(), S,
                     n, c, INSTANCE_NORM_EPS, _stream(self.device))
        return _Pending(st[0], st[1], None, relu)

    def _apply(self, src: _Slice, pend: _Pending, dst: _Slice, S, n, c, res: Optional[_Slice] = None):
        r = res or _Slice(src.tensor, 1)
        _lib.call_on(self.device, "fv3hip_cyclegan_apply", src.ptr, src.ld, src.off, src.stride, _ptr(pend.mean), _ptr(pend.rstd),
                     _ptr(pend.bias), int(pend.relu), r.ptr if res else None, r.ld, r.off, r.stride, dst.ptr, dst.ld, dst.off,
                     dst.stride, S, n, c, _stream(self.device))

    def _buf(self, key) -> _Slice:
        return _Slice(self._ws[key], self._ws[key].shape[-1])

    # -- the three parts on one chunk ----------------------------------------------------------------
    def _encode_chunk(self, state: torch.Tensor, x: _Slice):
        s = self.spec
        S, n, m, nc = int(state.shape[0]), s.nx, s.min_filters, s.n_convolutions
        raw0 = self._buf("raw0")
        # the geographic bias is added, and x, y, z read, by the loader of the 7 x 7 convolution: no input pass
        self._conv("first", _Slice(state, s.channels), _Pending(bias=self._input_bias), raw0, S, n, ctx_cell=self._xyz)
        cur, pend = raw0, self._stats("st:first", raw0, S, n, m)
        for l in range(nc):
            dst = self._buf(f"raw{l + 1}")
            self._conv(f"down{l}", cur, pend, dst, S, n >> l)
            cur, pend = dst, self._stats(f"st:down{l}", dst, S, n >> (l + 1), m * 2 ** (l + 1))
        self._apply(cur, pend, x, S, s.nx_bottom, s.max_filters)

    def _step_chunk(self, x: _Slice, i: int, S: int):
        s = self.spec
        nb, cb = s.nx_bottom, s.max_filters
        a, b = self._buf("a"), self._buf("b")
        # row (i - 1) % spd of the clock table: two floats
        clock = 0 if self._clock is None else self._clock.data_ptr() + 4 * N_CLOCK * ((i - 1) % s.samples_per_day)
        for stem in s.step_stems:
            self._conv(f"{stem}.a", x, _NONE, a, S, nb, ctx_cell=self._xyz_bottom, ctx_uniform=clock)
            pa = self._stats("st:a", a, S, nb, cb)
            self._conv(f"{stem}.b", a, pa, b, S, nb)
            if s.step_type == "resnet":
                self._apply(b, self._stats("st:b", b, S, nb, cb, relu=False), x, S, nb, cb, res=x)
            else:
                self._apply(b, self._stats("st:b", b, S, nb, cb), x, S, nb, cb)

    def _decode_chunk(self, x: _Slice, out: _Slice, S: int):
        s = self.spec
        n, m, nc = s.nx, s.min_filters, s.n_convolutions
        cur, pend = x, _NONE
        for l in reversed(range(nc)):
            dst = self._buf(f"raw{l}")
            self._conv(f"up{l}", cur, pend, dst, S, n >> (l + 1))
            cur, pend = dst, self._stats(f"st:up{l}", dst, S, n >> l, m * 2 ** l)
        self._apply(cur, pend, cur, S, n, m)      # in place: the 49 taps of the last layer read it as it is
        self._conv("last", cur, _NONE, out, S, n, out_bias=self._output_bias)

    # -- checks --------------------------------------------------------------------------------------
    def _check_state(self, state) -> torch.Tensor:
        s = self.spec
        if not isinstance(state, torch.Tensor) or state.dim() != 5:
            raise ValueError("the state must be a [window, tile, x, y, feature] tensor")
        check_cube_shape(state.shape)
        if state.shape[-1] != s.channels:
            raise ValueError(f"the state has {state.shape[-1]} features, the network needs {s.channels}")
        if state.shape[2] != s.nx:
            raise ValueError(f"the state has faces of {state.shape[2]} cells per edge, the generator was built for nx = {s.nx}")
        if state.dtype != torch.float32:
            raise TypeError(f"the normalised state must be float32, got {state.dtype}")
        _require_device(state)
        return state.contiguous()

    def _check_latent(self, latent) -> torch.Tensor:
        s = self.spec
        want = (6, s.nx_bottom, s.nx_bottom, s.max_filters)
        if not isinstance(latent, torch.Tensor) or latent.dim() != 5 or tuple(latent.shape[1:]) != want:
            raise ValueError(f"the latent must be a [window, {', '.join(map(str, want))}] tensor, got "
                             f"{tuple(latent.shape) if isinstance(latent, torch.Tensor) else type(latent).__name__}")
        if latent.dtype != torch.float32:
            raise TypeError(f"the latent must be float32, got {latent.dtype}")
        _require_device(latent)
        if not latent.is_contiguous():
            raise ValueError("the latent must be contiguous")
        return latent

    def _chunks(self, S: int, chunk: Optional[int]):
        chunk = self.chunk_size(S) if chunk is None else max(1, int(chunk))
        self._workspace(chunk)
        return [(i, min(S, i + chunk)) for i in range(0, S, chunk)]

    # -- public --------------------------------------------------------------------------------------
    def encode(self, state: torch.Tensor, chunk: Optional[int] = None) -> torch.Tensor:
        """Normalised float32 ``[S, 6, n, n, C]`` -> the latent ``[S, 6, nb, nb, max_filters]``, a new tensor."""
        state = self._check_state(state)
        s = self.spec
        latent = torch.empty((state.shape[0], 6, s.nx_bottom, s.nx_bottom, s.max_filters), dtype=torch.float32, device=state.device)
        for i, j in self._chunks(int(state.shape[0]), chunk):
            self._encode_chunk(state[i:j], _Slice(latent[i:j], s.max_filters))
        return latent

    def step(self, latent: torch.Tensor, i: int, chunk: Optional[int] = None) -> torch.Tensor:
        """Step ``i`` (1-based: the clock is at ``(i - 1) % samples_per_day``) of the latent, in place; returns it."""
        latent = self._check_latent(latent)
        if int(i) < 1:
            raise ValueError(f"steps are counted from 1, got {i}")
        for lo, hi in self._chunks(int(latent.shape[0]), chunk):
            self._step_chunk(_Slice(latent[lo:hi], self.spec.max_filters), int(i), hi - lo)
        return latent

    def decode(self, latent: torch.Tensor, out: Optional[torch.Tensor] = None, chunk: Optional[int] = None) -> torch.Tensor:
        """The latent -> the normalised state ``[S, 6, n, n, C]``.  ``out``: a float32 view of that shape whose cubes are
        contiguous (any stride between the windows, such as one time of ``[S, ntime, 6, n, n, C]``).  The latent is left as it is."""
        latent = self._check_latent(latent)
        s = self.spec
        S, shape = int(latent.shape[0]), (int(latent.shape[0]), 6, s.nx, s.nx, s.channels)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=latent.device)
        if tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != latent.device:
            raise ValueError(f"out must be a float32 {shape} tensor on {latent.device}")
        if S and (not out[0].is_contiguous() or (S > 1 and out.stride(0) < out[0].numel())):
            raise ValueError("out must hold contiguous cubes")
        for i, j in self._chunks(S, chunk):
            self._decode_chunk(_Slice(latent[i:j], s.max_filters), _Slice(out[i:j], s.channels, 0, out.stride(0)), j - i)
        return out

    def forward(self, state: torch.Tensor, ntime: int, chunk: Optional[int] = None) -> torch.Tensor:
        """Normalised float32 ``[S, 6, n, n, C]`` -> ``[S, ntime, 6, n, n, C]``: time 0 is the decoded encoding of the state,
        time ``i`` the decoded latent after ``i`` steps.  Every decode writes its time directly; the clock starts at 0."""
        state = self._check_state(state)
        if int(ntime) < 1:
            raise ValueError(f"ntime must be at least 1, got {ntime}")
        s, ntime = self.spec, int(ntime)
        S = int(state.shape[0])
        out = torch.empty((S, ntime, 6, s.nx, s.nx, s.channels), dtype=torch.float32, device=state.device)
        for i, j in self._chunks(S, chunk):
            x = self._buf("x")
            self._encode_chunk(state[i:j], x)
            for t in range(ntime):
                if t:
                    self._step_chunk(x, t, j - i)
                self._decode_chunk(x, _Slice(out[i:j, t], s.channels, 0, out.stride(0)), j - i)
        return out


class FullModelReplacementModel:
    """The generator and the scalers of a ``FullModelReplacementSpec`` on one device."""

    def __init__(self, spec: FullModelReplacementSpec, device="cuda", **generator_kwargs):
        spec.validate()
        self.spec = spec
        self.generator = RecurrentGeneratorModel(spec.generator, spec.convolution_type, device, **generator_kwargs)
        self.device = self.generator.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(self.device)
        self._mean, self._std = (up(a) for a in spec.scaler_arrays())
        self._nfeat = (ctypes.c_int * len(spec.variables))(*[f for _, f in spec.variables])

    def pack(self, sources: Sequence[torch.Tensor], n_windows: int, timesteps: int) -> torch.Tensor:
        """``sources[v]``: a ``[time, tile, x, y, level]`` view (any strides, float32 or float64) of state variable v ->
        float32 ``[n_windows, timesteps + 1, 6, n, n, F]``, ``(x - mean) / std`` in float64, window w from times
        ``w * timesteps ...`` (``fv3hip_graph_pack``)."""
        spec = self.spec
        if len(sources) != len(spec.variables):
            raise ValueError(f"{len(spec.variables)} sources are needed, got {len(sources)}")
        dev = _require_device(*sources)
        for (name, nfeat), t in zip(spec.variables, sources):
            if t.dim() != 5 or t.shape[-1] != nfeat:
                raise ValueError(f"variable {name!r} must be [time, tile, x, y, {nfeat}], got shape {tuple(t.shape)}")
            check_cube_shape(t.shape[:-1] + (0,), f"variable {name!r}")
            if tuple(t.shape[:4]) != tuple(sources[0].shape[:4]):
                raise ValueError("the state variables differ in their time, tile, x or y extent")
            if t.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"variable {name!r} must be float32 or float64, got {t.dtype}")
        if timesteps < 1 or n_windows < 0 or n_windows * timesteps + 1 > sources[0].shape[0]:
            raise ValueError(f"{n_windows} windows of {timesteps} steps do not fit {sources[0].shape[0]} times")
        n, k = int(sources[0].shape[2]), len(sources)
        state = torch.empty((n_windows, timesteps + 1, 6, n, n, spec.n_features), dtype=torch.float32, device=dev)
        _lib.call_on(dev, "fv3hip_graph_pack", (ctypes.c_void_p * k)(*[t.data_ptr() for t in sources]),
                     (ctypes.c_int * k)(*[_lib.F64 if t.dtype == torch.float64 else _lib.F32 for t in sources]),
                     (ctypes.c_int64 * (5 * k))(*[s for t in sources for s in t.stride()]), k, self._nfeat, self._mean.data_ptr(),
                     self._std.data_ptr(), n_windows, timesteps + 1, timesteps, n, state.data_ptr(), _stream(dev))
        return state

    def unpack(self, state: torch.Tensor) -> List[torch.Tensor]:
        """Float32 ``[..., 6, n, n, F]`` -> per variable float64 ``[..., 6, n, n, nfeat]``, ``float64(x) * std + mean``."""
        check_cube_shape(state.shape)
        if state.dtype != torch.float32 or state.shape[-1] != self.spec.n_features:
            raise ValueError(f"the state must be float32 with {self.spec.n_features} features")
        dev = _require_device(state)
        state = state.contiguous()
        lead, n = tuple(state.shape[:-1]), int(state.shape[-2])
        outs = [torch.empty(lead + (f,), dtype=torch.float64, device=dev) for _, f in self.spec.variables]
        rows = int(np.prod(lead[:-3])) if lead[:-3] else 1
        _lib.call_on(dev, "fv3hip_graph_unpack", state.data_ptr(), rows, n, len(outs), self._nfeat, self._mean.data_ptr(),
                     self._std.data_ptr(), (ctypes.c_void_p * len(outs))(*[t.data_ptr() for t in outs]), _stream(dev))
        return outs
