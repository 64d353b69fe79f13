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
import dataclasses
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from .cube import StatePacker, _Slice
from .cyclegan import (MAX_VARIABLES, REFERENCE_BATCH, _NONE, _GeneratorRuntime, _Pending, check_architecture,
                       check_convolution_type, check_grid, check_optional_arrays, check_plan_arrays, spec_from_arrays,
                       spec_to_arrays)
from .ops import _require_device

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
        check_plan_arrays(self.plan, self.weights, self.biases)
        n, nb, C = self.nx, self.nx_bottom, self.channels
        if (self.input_bias is None) != (self.output_bias is None):
            raise ValueError("input_bias and output_bias come together (use_geographic_bias)")
        if (self.xyz is None) != (self.xyz_bottom is None):
            raise ValueError("xyz and xyz_bottom come together (use_geographic_features)")
        check_optional_arrays(self, {"input_bias": (6, C, n, n), "output_bias": (6, C, n, n), "xyz": (6, 3, n, n),
                                     "xyz_bottom": (6, 3, nb, nb)})

    _FLAGS = {"input_bias": "use_geographic_bias", "output_bias": "use_geographic_bias", "xyz": "use_geographic_features",
              "xyz_bottom": "use_geographic_features"}

    def to_arrays(self, prefix: str = ""):
        meta = {"channels": int(self.channels), "nx": int(self.nx), "n_convolutions": int(self.n_convolutions),
                "n_resnet": int(self.n_resnet), "kernel_size": int(self.kernel_size),
                "strided_kernel_size": int(self.strided_kernel_size), "max_filters": int(self.max_filters),
                "step_type": str(self.step_type),
                "samples_per_day": None if self.samples_per_day is None else int(self.samples_per_day),
                "use_geographic_bias": self.use_geographic_bias, "use_geographic_features": self.use_geographic_features}
        return meta, spec_to_arrays(self, prefix, self._FLAGS)

    @classmethod
    def from_arrays(cls, meta: Mapping, arrays: Mapping[str, np.ndarray], prefix: str = "") -> "RecurrentGeneratorSpec":
        check_architecture(meta["n_convolutions"], meta["n_resnet"], meta["kernel_size"], meta.get("strided_kernel_size", 4),
                           meta["max_filters"])
        check_step_type(meta["step_type"])
        spd = meta.get("samples_per_day")
        plan = layer_plan(int(meta["channels"]), int(meta["n_convolutions"]), int(meta["n_resnet"]), int(meta["kernel_size"]),
                          meta["max_filters"], meta["step_type"], bool(meta["use_geographic_features"]), spd)
        weights, biases, optional = spec_from_arrays(arrays, prefix, plan, meta, cls._FLAGS)
        return cls(int(meta["channels"]), int(meta["nx"]), weights, biases, int(meta["n_convolutions"]), int(meta["n_resnet"]),
                   int(meta["kernel_size"]), int(meta.get("strided_kernel_size", 4)), meta["max_filters"], meta["step_type"],
                   None if spd is None else int(spd), **optional)


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


class RecurrentGeneratorModel(_GeneratorRuntime):
    """One recurrent generator on one device: the shared runtime of cyclegan.py (a layer that reads context channels holds its
    weights as the source's rows and the context's rows), the two ``xyz`` tables and the clock table.  A sample is a window."""

    _SAMPLE, _bottom = "window", True

    def __init__(self, spec: RecurrentGeneratorSpec, convolution_type: str = "halo_conv2d", device="cuda",
                 workspace_limit: int = 2 << 30, max_chunk: int = REFERENCE_BATCH):
        super().__init__(spec, convolution_type, device, workspace_limit, max_chunk)
        self._xyz, self._xyz_bottom = self._channel_last(spec.xyz), self._channel_last(spec.xyz_bottom)
        self._clock = None if spec.samples_per_day is None else self._up(clock_table(spec.samples_per_day))

    def _context_channels(self, name: str) -> int:
        c_cell, c_uni = self.spec.context_channels
        return c_cell if name == "first" else c_cell + c_uni if name.endswith(".a") else 0

    # -- the three parts on one chunk ----------------------------------------------------------------
    def _encode_chunk(self, state: torch.Tensor, x: _Slice):
        s = self.spec
        S = int(state.shape[0])
        # the geographic bias is added, and x, y, z read, by the loader of the 7 x 7 convolution: no input pass
        cur, pend = self._down_chain(_Slice(state, s.channels), _Pending(bias=self._input_bias), S, ctx_cell=self._xyz)
        self._apply(cur, pend, x, S, s.nx_bottom, s.max_filters)

    def _step_chunk(self, x: _Slice, i: int, S: int):
        s = self.spec
        nb, cb = s.nx_bottom, s.max_filters
        a, b = self._buf("a"), self._buf("b")
        # row (i - 1) % spd of the clock table: two floats
        clock = 0 if self._clock is None else self._clock.data_ptr() + 4 * N_CLOCK * ((i - 1) % s.samples_per_day)
        for stem in s.step_stems:
            self._conv(f"{stem}.a", x, _NONE, a, S, nb, ctx_cell=self._xyz_bottom, ctx_uniform=clock, c_uni=N_CLOCK)
            pa = self._stats("st:a", a, S, nb, cb)
            self._conv(f"{stem}.b", a, pa, b, S, nb)
            if s.step_type == "resnet":
                self._apply(b, self._stats("st:b", b, S, nb, cb, relu=False), x, S, nb, cb, res=x)
            else:
                self._apply(b, self._stats("st:b", b, S, nb, cb), x, S, nb, cb)

    def _decode_chunk(self, x: _Slice, out: _Slice, S: int):
        self._up_chain(x, _NONE, out, S)

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
        self._packer = StatePacker(spec.variables, *spec.scaler_arrays(), self.device)

    def pack(self, sources: Sequence[torch.Tensor], n_windows: int, timesteps: int) -> torch.Tensor:
        """``sources[v]``: a ``[time, tile, x, y, level]`` view (any strides, float32 or float64) of state variable v ->
        float32 ``[n_windows, timesteps + 1, 6, n, n, F]``, ``(x - mean) / std`` in float64, window w from times
        ``w * timesteps ...`` (``fv3hip_graph_pack``)."""
        return self._packer.pack(sources, n_windows, timesteps + 1, timesteps)

    def unpack(self, state: torch.Tensor) -> List[torch.Tensor]:
        """Float32 ``[..., 6, n, n, F]`` -> per variable float64 ``[..., 6, n, n, nfeat]``, ``float64(x) * std + mean``."""
        return self._packer.unpack(state)
