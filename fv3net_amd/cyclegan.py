"""CycleGAN generators: the arrays of fv3fit's ``"cycle_gan"`` model and its device layer.

``GeneratorSpec`` holds what ``GeneratorConfig.build`` produces (external/fv3fit/fv3fit/pytorch/cyclegan/generator.py:19-270)
as plain arrays in torch's own layouts, ``CycleGanSpec`` the two generators with the ``a_*`` / ``b_*`` ``StandardScaler`` of
every state variable (cyclegan/reloadable.py:43-253).  With ``m = int(max_filters / 2**n_convolutions)``, ``C`` state channels
and ``c_l = m 2**l`` on faces of ``n / 2**l`` cells per edge, the layers are

    input        x + input_bias; append sin(lon + theta), cos(lon + theta), x, y, z
    first        conv 7 x 7, C (+ 5) -> m; instance norm; + embedded_bias; ReLU
    down{l}      conv 4 x 4 stride 2, c_l -> c_{l+1}; instance norm; ReLU              l = 0 ... n_convolutions - 1
    res{j}.a/.b  x + IN(conv k x k(ReLU(IN(conv k x k(x)))))                           j = 0 ... n_resnet - 1
    up{l}        ConvTranspose2d 4 x 4 stride 2 (halo 1, crop 3), c_{l+1} -> c_l; instance norm; ReLU
    last         conv 7 x 7, m -> C; + output_bias

``GeneratorModel`` keeps the weights on the device in the kernels' layout and runs the layers with the stateless
``fv3hip_cyclegan_*`` kernels on torch's current stream, one launch after the other.  A layer's instance norm, embedded bias and
ReLU are applied by the loader of the convolution that reads it; only the residual sums and the last ``up`` layer are written
out normalised.  DESIGN.md section 17.
"""
import dataclasses
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .cube import StatePacker, _Slice, check_cube_shape, cuda_device
from .ops import _require_device, _stream

CONVOLUTION_TYPES = {"halo_conv2d": _lib.CYCLEGAN_HALO_CUBE, "conv2d": _lib.CYCLEGAN_HALO_ZEROS}
KINDS = {"regular": _lib.CYCLEGAN_CONV_REGULAR, "strided": _lib.CYCLEGAN_CONV_STRIDED, "transposed": _lib.CYCLEGAN_CONV_TRANSPOSED}
N_GEOGRAPHIC_FEATURES = 5
INSTANCE_NORM_EPS = 1e-5
SECONDS_PER_DAY = 86400
MAX_VARIABLES = 16
REFERENCE_BATCH = 100          # reloadable.py:173: the reference's own loop runs 100 samples at a time


def check_convolution_type(convolution_type: str) -> int:
    if convolution_type not in CONVOLUTION_TYPES:
        raise ValueError(f"Unknown convolution type: {convolution_type!r}; supported: {sorted(CONVOLUTION_TYPES)}")
    return CONVOLUTION_TYPES[convolution_type]


def check_architecture(n_convolutions: int = 3, n_resnet: int = 3, kernel_size: int = 3, strided_kernel_size: int = 4,
                       max_filters: int = 256, disable_convolutions: bool = False):
    """The part of ``GeneratorConfig`` that is built here; anything else is refused with the offending value."""
    if disable_convolutions:
        raise NotImplementedError("disable_convolutions = True is not built: the network is the convolutions")
    if int(strided_kernel_size) != 4:
        raise NotImplementedError(f"strided_kernel_size = {strided_kernel_size} is not built; supported: 4 (the reference's "
                                  "projects use 4, odd sizes need output_padding)")
    if int(kernel_size) not in (3, 5, 7):
        raise NotImplementedError(f"kernel_size = {kernel_size} is not built; supported: 3, 5 and 7")
    if int(n_convolutions) < 1:
        raise ValueError(f"n_convolutions must be at least 1, got {n_convolutions}")
    if int(n_resnet) < 0:
        raise ValueError(f"n_resnet must not be negative, got {n_resnet}")
    if int(max_filters / 2 ** int(n_convolutions)) < 1:
        raise ValueError(f"max_filters = {max_filters} leaves int(max_filters / 2**{n_convolutions}) = 0 filters in the first layer")


def check_grid(nx: int, ny: int, n_convolutions: int):
    """Faces the network can run on; raised before any launch."""
    if nx != ny:
        raise ValueError(f"cube faces are square (nx == ny), got {nx} x {ny}")
    if nx < 3:
        raise ValueError(f"nx = {nx}: the 7 x 7 layers need a halo of 3 cells, so nx >= 3")
    f = 2 ** int(n_convolutions)
    if nx % f != 0:
        raise ValueError(f"nx = {nx} cannot be halved {n_convolutions} times: nx must be a multiple of {f}")
    if nx // f < 2:
        raise ValueError(f"nx = {nx} leaves faces of {nx // f} x {nx // f} cells after {n_convolutions} strided layers: instance "
                         "norm needs more than one cell per face (nx // 2**n_convolutions >= 2)")


def layer_plan(channels: int, n_convolutions: int, n_resnet: int, kernel_size: int, max_filters: int,
               use_geographic_features: bool) -> List[Tuple[str, str, int, int, int, int]]:
    """(name, kind, c_in, c_out, k, level of the OUTPUT) of every convolution in execution order."""
    m = int(max_filters / 2 ** n_convolutions)
    c = lambda l: m * 2 ** l
    plan = [("first", "regular", channels + (N_GEOGRAPHIC_FEATURES if use_geographic_features else 0), m, 7, 0)]
    plan += [(f"down{l}", "strided", c(l), c(l + 1), 4, l + 1) for l in range(n_convolutions)]
    for j in range(n_resnet):
        plan += [(f"res{j}.{ab}", "regular", c(n_convolutions), c(n_convolutions), kernel_size, n_convolutions) for ab in "ab"]
    plan += [(f"up{l}", "transposed", c(l + 1), c(l), 4, l) for l in reversed(range(n_convolutions))]
    return plan + [("last", "regular", m, channels, 7, 0)]


def weight_shape(kind: str, c_in: int, c_out: int, k: int) -> Tuple[int, ...]:
    """torch's layout: ``Conv2d`` ``[c_out, c_in, k, k]``, ``ConvTranspose2d`` ``[c_in, c_out, k, k]``."""
    return (c_in, c_out, k, k) if kind == "transposed" else (c_out, c_in, k, k)


def split_transposed_weight(w: np.ndarray) -> np.ndarray:
    """``ConvTranspose2d(4, stride 2)``'s weight ``[c_in, c_out, 4, 4]`` -> ``[px, py, a, b, c_in, c_out]``, the four 2 x 2
    convolutions of the four output parities: along an axis output ``2 m`` takes tap 1 of cell ``m`` (a = 0) and tap 3 of cell
    ``m - 1`` (a = 1), output ``2 m + 1`` tap 0 of cell ``m + 1`` (a = 0) and tap 2 of cell ``m`` (a = 1)."""
    w = np.asarray(w)
    tap = lambda p, a: 1 + 2 * a if p == 0 else 2 * a
    out = np.empty((2, 2, 2, 2) + w.shape[:2], w.dtype)
    for px in range(2):
        for py in range(2):
            for a in range(2):
                for b in range(2):
                    out[px, py, a, b] = w[:, :, tap(px, a), tap(py, b)]
    return out


def transposed_source_offset(parity: int, a: int) -> int:
    """The cell, relative to ``m``, that tap ``a`` of output ``2 m + parity`` reads."""
    return (1 - a) if parity else -a


def seconds_since_1970(time) -> np.ndarray:
    """``cftime.date2num(time, "seconds since 1970-01-01").astype(np.float32)`` (reloadable.py:247-249) for ``datetime64``
    values, plain numbers of seconds, or ``cftime`` objects where that module exists."""
    a = np.atleast_1d(np.asarray(time.values if hasattr(time, "values") else time))
    if np.issubdtype(a.dtype, np.datetime64):
        ns = a.astype("datetime64[ns]").astype(np.int64)
        return (ns // 10 ** 9 + (ns % 10 ** 9) / 1e9).astype(np.float32)
    if a.dtype == object:
        try:
            import cftime
        except ImportError as e:
            raise TypeError("time holds objects; cftime is needed to read them as dates") from e
        return np.asarray(cftime.date2num(a, "seconds since 1970-01-01")).astype(np.float32)
    return a.astype(np.float64).astype(np.float32)


def theta_from_seconds(seconds: np.ndarray) -> np.ndarray:
    """``time % 86400 / 86400 * 2 * pi`` with every step in float32, as torch evaluates modules.py:90-92 on a float32 tensor."""
    t = np.asarray(seconds, np.float32)
    day = np.float32(SECONDS_PER_DAY)
    return ((np.remainder(t, day) / day) * np.float32(2)) * np.float32(np.pi)


def check_plan_arrays(plan, weights: Mapping[str, np.ndarray], biases: Mapping[str, np.ndarray]):
    """Every layer of the plan has its float32 weight (``weight_shape``) and bias ``[c_out]``, and there are no others."""
    names = {p[0] for p in plan}
    if set(weights) != names or set(biases) != names:
        raise ValueError(f"weights {sorted(weights)} / biases {sorted(biases)} differ from the layers {sorted(names)}")
    for name, kind, ci, co, k, _ in plan:
        for what, a, shape in (("weight", weights[name], weight_shape(kind, ci, co, k)), ("bias", biases[name], (co,))):
            a = np.asarray(a)
            if a.shape != shape or a.dtype != np.float32:
                raise ValueError(f"layer {name!r}: {what} has shape {a.shape} and dtype {a.dtype}, expected float32 {shape}")


def check_optional_arrays(spec, shapes: Mapping[str, Tuple[int, ...]]):
    """The optional arrays of a generator spec that are given are float32 of their shapes."""
    for what, shape in shapes.items():
        a = getattr(spec, what)
        if a is not None and (np.asarray(a).shape != shape or np.asarray(a).dtype != np.float32):
            raise ValueError(f"{what} has shape {np.asarray(a).shape} and dtype {np.asarray(a).dtype}, expected float32 {shape}")


def spec_to_arrays(spec, prefix: str, optional: Sequence[str]) -> Dict[str, np.ndarray]:
    """``"{prefix}{layer}.weight"`` / ``.bias`` of every layer and ``"{prefix}{key}"`` of every optional array that is given."""
    arrays = {}
    for name in spec.weights:
        arrays[f"{prefix}{name}.weight"] = np.asarray(spec.weights[name], np.float32)
        arrays[f"{prefix}{name}.bias"] = np.asarray(spec.biases[name], np.float32)
    for key in optional:
        if getattr(spec, key) is not None:
            arrays[f"{prefix}{key}"] = np.asarray(getattr(spec, key), np.float32)
    return arrays


def spec_from_arrays(arrays: Mapping[str, np.ndarray], prefix: str, plan, meta: Mapping, flags: Mapping[str, str]):
    """The reverse: (weights, biases, optional arrays -- ``None`` where ``meta[flags[key]]`` is off)."""
    get = lambda key: np.asarray(arrays[prefix + key], np.float32)
    return ({p[0]: get(p[0] + ".weight") for p in plan}, {p[0]: get(p[0] + ".bias") for p in plan},
            {key: get(key) if meta[flag] else None for key, flag in flags.items()})


@dataclasses.dataclass
class GeneratorSpec:
    """One generator.  ``weights[name]`` in torch's layout (``weight_shape``), ``biases[name]`` ``[c_out]``; the geographic
    biases ``[6, channels, nx, nx]`` (``None``: the flag is off), ``lon`` ``[6, nx, nx]`` and ``xyz`` ``[6, 3, nx, nx]``
    (``None``: ``use_geographic_features`` is off), all float32."""

    channels: int
    nx: int
    weights: Dict[str, np.ndarray]
    biases: Dict[str, np.ndarray]
    n_convolutions: int = 3
    n_resnet: int = 3
    kernel_size: int = 3
    strided_kernel_size: int = 4
    max_filters: int = 256
    input_bias: Optional[np.ndarray] = None
    output_bias: Optional[np.ndarray] = None
    embedded_bias: Optional[np.ndarray] = None
    lon: Optional[np.ndarray] = None
    xyz: Optional[np.ndarray] = None
    disable_convolutions: bool = False

    def __post_init__(self):
        self.validate()

    @property
    def use_geographic_bias(self) -> bool:
        return self.input_bias is not None

    @property
    def use_geographic_features(self) -> bool:
        return self.lon is not None

    @property
    def use_geographic_embedded_bias(self) -> bool:
        return self.embedded_bias is not None

    @property
    def min_filters(self) -> int:
        return int(self.max_filters / 2 ** self.n_convolutions)

    @property
    def plan(self):
        return layer_plan(self.channels, self.n_convolutions, self.n_resnet, self.kernel_size, self.max_filters,
                          self.use_geographic_features)

    def flops_per_sample(self) -> float:
        """Sum over the layers of ``2 taps c_in c_out 6 n_l**2`` with ``n_l`` the layer's output edge; ``taps = k**2``, for a
        transposed layer the 4 taps every output cell reads."""
        return float(sum(2 * (4 if kind == "transposed" else k * k) * ci * co * 6 * (self.nx >> level) ** 2
                         for _, kind, ci, co, k, level in self.plan))

    def validate(self):
        check_architecture(self.n_convolutions, self.n_resnet, self.kernel_size, self.strided_kernel_size, self.max_filters,
                           self.disable_convolutions)
        if self.channels < 1:
            raise ValueError(f"a generator needs at least one channel, got {self.channels}")
        check_grid(self.nx, self.nx, self.n_convolutions)
        check_plan_arrays(self.plan, self.weights, self.biases)
        n, C, m = self.nx, self.channels, self.min_filters
        if (self.input_bias is None) != (self.output_bias is None):
            raise ValueError("input_bias and output_bias come together (use_geographic_bias)")
        if (self.lon is None) != (self.xyz is None):
            raise ValueError("lon and xyz come together (use_geographic_features)")
        check_optional_arrays(self, {"input_bias": (6, C, n, n), "output_bias": (6, C, n, n), "embedded_bias": (6, m, n, n),
                                     "lon": (6, n, n), "xyz": (6, 3, n, n)})

    _FLAGS = {"input_bias": "use_geographic_bias", "output_bias": "use_geographic_bias", "embedded_bias": "use_geographic_embedded_bias",
              "lon": "use_geographic_features", "xyz": "use_geographic_features"}

    def to_arrays(self, prefix: str = ""):
        meta = {"channels": int(self.channels), "nx": int(self.nx), "n_convolutions": int(self.n_convolutions),
                "n_resnet": int(self.n_resnet), "kernel_size": int(self.kernel_size),
                "strided_kernel_size": int(self.strided_kernel_size), "max_filters": int(self.max_filters),
                "use_geographic_bias": self.use_geographic_bias, "use_geographic_features": self.use_geographic_features,
                "use_geographic_embedded_bias": self.use_geographic_embedded_bias, "disable_convolutions": False}
        return meta, spec_to_arrays(self, prefix, self._FLAGS)

    @classmethod
    def from_arrays(cls, meta: Mapping, arrays: Mapping[str, np.ndarray], prefix: str = "") -> "GeneratorSpec":
        check_architecture(meta["n_convolutions"], meta["n_resnet"], meta["kernel_size"], meta.get("strided_kernel_size", 4),
                           meta["max_filters"], meta.get("disable_convolutions", False))
        plan = layer_plan(int(meta["channels"]), int(meta["n_convolutions"]), int(meta["n_resnet"]), int(meta["kernel_size"]),
                          meta["max_filters"], bool(meta["use_geographic_features"]))
        weights, biases, optional = spec_from_arrays(arrays, prefix, plan, meta, cls._FLAGS)
        return cls(int(meta["channels"]), int(meta["nx"]), weights, biases, int(meta["n_convolutions"]), int(meta["n_resnet"]),
                   int(meta["kernel_size"]), int(meta.get("strided_kernel_size", 4)), meta["max_filters"], **optional)


@dataclasses.dataclass
class CycleGanSpec:
    """Both generators, the state variables ``(name, feature count)`` in the network's channel order, and per domain and
    variable the scaler's float64 ``(mean, std)`` ``[nfeat]`` under ``"a_<name>"`` / ``"b_<name>"``."""

    generator_a_to_b: GeneratorSpec
    generator_b_to_a: GeneratorSpec
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

    def generator(self, reverse: bool = False) -> GeneratorSpec:
        return self.generator_b_to_a if reverse else self.generator_a_to_b

    def scaler_arrays(self, domain: str) -> Tuple[np.ndarray, np.ndarray]:
        """The domain's means and stds of all channels, concatenated."""
        return (np.concatenate([self.scalers[f"{domain}_{n}"][0] for n, _ in self.variables]),
                np.concatenate([self.scalers[f"{domain}_{n}"][1] for n, _ in self.variables]))

    def validate(self):
        check_convolution_type(self.convolution_type)
        if not self.variables:
            raise ValueError("a CycleGAN needs at least one state variable")
        if len(self.variables) > MAX_VARIABLES:
            raise ValueError(f"at most {MAX_VARIABLES} state variables are supported, got {len(self.variables)}")
        if len(set(self.state_variables)) != len(self.variables):
            raise ValueError(f"a state variable is named twice: {self.state_variables}")
        for g in (self.generator_a_to_b, self.generator_b_to_a):
            g.validate()
            if g.channels != self.n_features:
                raise ValueError(f"a generator has {g.channels} channels, the state variables {self.n_features} features")
        if self.generator_a_to_b.nx != self.generator_b_to_a.nx:
            raise ValueError("the two generators differ in nx")
        want = {f"{d}_{n}" for d in "ab" for n, _ in self.variables}
        if set(self.scalers) != want:
            raise ValueError(f"scalers {sorted(self.scalers)} differ from {sorted(want)}")
        for d in "ab":
            for name, nfeat in self.variables:
                mean, std = (np.asarray(v) for v in self.scalers[f"{d}_{name}"])
                if nfeat < 1 or mean.shape != (nfeat,) or std.shape != (nfeat,) or mean.dtype != np.float64 or std.dtype != np.float64:
                    raise ValueError(f"scaler {d}_{name}: mean and std must be float64 of shape ({nfeat},)")
                if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std != 0)):
                    raise ValueError(f"scaler {d}_{name}: mean and std must be finite and std non-zero")

    def to_arrays(self):
        meta = {"convolution_type": self.convolution_type, "variables": [{"name": n, "nfeat": f} for n, f in self.variables],
                "generators": {}}
        arrays = {}
        for key in ("a_to_b", "b_to_a"):
            meta["generators"][key], part = getattr(self, f"generator_{key}").to_arrays(f"{key}.")
            arrays.update(part)
        for key, (mean, std) in self.scalers.items():
            arrays[f"scaler.{key}.mean"] = np.asarray(mean, np.float64)
            arrays[f"scaler.{key}.std"] = np.asarray(std, np.float64)
        return meta, arrays

    @classmethod
    def from_arrays(cls, meta: Mapping, arrays: Mapping[str, np.ndarray]) -> "CycleGanSpec":
        check_convolution_type(meta["convolution_type"])
        variables = [(v["name"], int(v["nfeat"])) for v in meta["variables"]]
        gens = {key: GeneratorSpec.from_arrays(meta["generators"][key], arrays, f"{key}.") for key in ("a_to_b", "b_to_a")}
        scalers = {f"{d}_{n}": (np.asarray(arrays[f"scaler.{d}_{n}.mean"], np.float64), np.asarray(arrays[f"scaler.{d}_{n}.std"], np.float64))
                   for d in "ab" for n, _ in variables}
        return cls(gens["a_to_b"], gens["b_to_a"], variables, scalers, meta["convolution_type"])


class _Pending:
    """What the next reader of a raw convolution output applies while loading: ``relu((v - mean) * rstd + bias)``."""

    def __init__(self, mean=None, rstd=None, bias=None, relu=False):
        self.mean, self.rstd, self.bias, self.relu = mean, rstd, bias, relu


_NONE = _Pending()
_ptr = lambda t: None if t is None else t.data_ptr()


class _GeneratorRuntime:
    """What ``GeneratorModel`` and ``RecurrentGeneratorModel`` (fmr.py) share: the weights uploaded once in the kernels' layout,
    a workspace that is kept between calls, the three layer launches, and the two chains both networks run -- ``first`` ->
    ``down{l}`` and ``up{l}`` -> ``last``.  Samples are worked through in chunks of at most ``max_chunk`` whose workspace stays
    within ``workspace_limit`` bytes; a sample's result does not depend on the chunk it falls into.

    A subclass sets ``_SAMPLE`` (what it calls a sample), ``_bottom`` (whether the ``x``, ``a``, ``b`` buffers of the bottom
    level exist) and ``_in_channels`` (the channels of the ``in`` buffer of an input pass; 0: none)."""

    _SAMPLE, _in_channels = "sample", 0

    def __init__(self, spec, convolution_type, device, workspace_limit, max_chunk):
        spec.validate()
        self.spec = spec
        self.halo_mode = check_convolution_type(convolution_type)
        self.device = cuda_device(device, type(self).__name__)
        if max_chunk < 1 or workspace_limit < 1:
            raise ValueError(f"max_chunk and workspace_limit must be positive, got {max_chunk}, {workspace_limit}")
        _lib.load()
        self.workspace_limit, self.max_chunk = int(workspace_limit), int(max_chunk)
        self._layers = {p[0]: p for p in spec.plan}
        self._w, self._w_ctx, self._b = {}, {}, {}
        for name, kind, ci, *_ in spec.plan:
            w = np.asarray(spec.weights[name])
            n_ctx = self._context_channels(name)
            if n_ctx:     # [k][k][c][c_out] for the source's channels and for the context's
                self._w_ctx[name] = self._up(w[:, ci - n_ctx:].transpose(2, 3, 1, 0))
                w = w[:, :ci - n_ctx]
            # [k][k][c_in][c_out]; the transposed layer as its four parity sub-kernels [px][py][a][b][c_in][c_out]
            self._w[name] = self._up(split_transposed_weight(w) if kind == "transposed" else w.transpose(2, 3, 1, 0))
            self._b[name] = self._up(spec.biases[name])
        self._input_bias, self._output_bias = self._channel_last(spec.input_bias), self._channel_last(spec.output_bias)
        self._ws: Dict[str, torch.Tensor] = {}
        self._ws_chunk = 0

    def _context_channels(self, name: str) -> int:
        """How many of layer ``name``'s input channels, the last ones, are context channels."""
        return 0

    def _up(self, a) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.device)

    def _channel_last(self, a) -> Optional[torch.Tensor]:
        """``[6][c][n][n]`` -> ``[6][n][n][c]`` on the device."""
        return None if a is None else self._up(np.asarray(a).transpose(0, 2, 3, 1))

    # -- workspace -----------------------------------------------------------------------------------
    def _buffers(self) -> Dict[str, Tuple[int, int]]:
        """name -> (cells per edge, channels) of every activation buffer of one sample."""
        s = self.spec
        n, m, nc = s.nx, s.min_filters, s.n_convolutions
        out = {f"raw{l}": (n >> l, m * 2 ** l) for l in range(nc + 1)}
        if self._in_channels:
            out["in"] = (n, self._in_channels)
        if self._bottom:
            out.update({key: (n >> nc, m * 2 ** nc) for key in ("x", "a", "b")})
        return out

    def _stat_keys(self) -> Dict[str, int]:
        """name -> channels of every pair of instance-norm statistics (mean, rstd) ``[2][S][6][c]``, in the order of the
        layers; the ``.a`` layers of the bottom level share one pair, the ``.b`` layers another."""
        out = {}
        for name, _, _, co, _, _ in self.spec.plan:
            if name != "last":
                out.setdefault("st:" + (name[-1] if name[-2:] in (".a", ".b") else name), co)
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

    def _buf(self, key) -> _Slice:
        return _Slice(self._ws[key], self._ws[key].shape[-1])

    def _chunks(self, S: int, chunk: Optional[int]) -> List[Tuple[int, int]]:
        """The (first, end) sample of every chunk, with the workspace made ready for them."""
        if S == 0:
            return []
        chunk = self.chunk_size(S) if chunk is None else max(1, int(chunk))
        self._workspace(chunk)
        return [(i, min(S, i + chunk)) for i in range(0, S, chunk)]

    # -- layer launches ------------------------------------------------------------------------------
    def _conv(self, name, src: _Slice, pend: _Pending, dst: _Slice, S, n_in, out_bias=None, ctx_cell=None, ctx_uniform: int = 0,
              c_uni: int = 0):
        """``ctx_cell``: per-cell context ``[6][n][n][c]``; ``ctx_uniform``: the device address of ``c_uni`` values (0: none).
        A layer without context rows goes through the same entry point."""
        _, kind, ci, co, k, _ = self._layers[name]
        c_cell = 0 if ctx_cell is None else int(ctx_cell.shape[-1])
        c_uni = c_uni if ctx_uniform else 0
        _lib.call_on(self.device, "fv3hip_cyclegan_conv_context", src.ptr, src.ld, src.off, src.stride, _ptr(pend.mean),
                     _ptr(pend.rstd), _ptr(pend.bias), int(pend.relu), self._w[name].data_ptr(), self._b[name].data_ptr(),
                     _ptr(out_bias), dst.ptr, dst.ld, dst.off, dst.stride, S, n_in, ci - c_cell - c_uni, co, KINDS[kind], k,
                     self.halo_mode, _ptr(ctx_cell), c_cell, ctx_uniform or None, c_uni, _ptr(self._w_ctx.get(name)),
                     _stream(self.device))

    def _stats(self, key, src: _Slice, S, n, c, bias=None, relu=True) -> _Pending:
        st = self._ws[key]
        _lib.call_on(self.device, "fv3hip_cyclegan_stats", src.ptr, src.ld, src.off, src.stride, st[0].data_ptr(), st[1].data_ptr(), S,
                     n, c, INSTANCE_NORM_EPS, _stream(self.device))
        return _Pending(st[0], st[1], bias, relu)

    def _apply(self, src: _Slice, pend: _Pending, dst: _Slice, S, n, c, res: Optional[_Slice] = None):
        r = res or _Slice(src.tensor, 1)
        _lib.call_on(self.device, "fv3hip_cyclegan_apply", src.ptr, src.ld, src.off, src.stride, _ptr(pend.mean), _ptr(pend.rstd),
                     _ptr(pend.bias), int(pend.relu), r.ptr if res else None, r.ld, r.off, r.stride, dst.ptr, dst.ld, dst.off,
                     dst.stride, S, n, c, _stream(self.device))

    # -- the two chains ------------------------------------------------------------------------------
    def _down_chain(self, src: _Slice, pend: _Pending, S: int, ctx_cell=None, first_bias=None) -> Tuple[_Slice, _Pending]:
        """``first`` and the ``down{l}`` layers; returns the raw output of the last one and what its reader applies."""
        s = self.spec
        n, m = s.nx, s.min_filters
        raw0 = self._buf("raw0")
        self._conv("first", src, pend, raw0, S, n, ctx_cell=ctx_cell)
        cur, pend = raw0, self._stats("st:first", raw0, S, n, m, bias=first_bias)
        for l in range(s.n_convolutions):
            dst = self._buf(f"raw{l + 1}")
            self._conv(f"down{l}", cur, pend, dst, S, n >> l)
            cur, pend = dst, self._stats(f"st:down{l}", dst, S, n >> (l + 1), m * 2 ** (l + 1))
        return cur, pend

    def _up_chain(self, cur: _Slice, pend: _Pending, out: _Slice, S: int):
        """The ``up{l}`` layers and ``last``, which writes ``out``."""
        s = self.spec
        n, m = s.nx, s.min_filters
        for l in reversed(range(s.n_convolutions)):
            dst = self._buf(f"raw{l}")
            self._conv(f"up{l}", cur, pend, dst, S, n >> (l + 1))
            cur, pend = dst, self._stats(f"st:up{l}", dst, S, n >> l, m * 2 ** l)
        self._apply(cur, pend, cur, S, n, m)      # in place: the 49 taps of the last layer read it as it is
        self._conv("last", cur, _NONE, out, S, n, out_bias=self._output_bias)

    def _check_state(self, state) -> torch.Tensor:
        s = self.spec
        if not isinstance(state, torch.Tensor) or state.dim() != 5:
            raise ValueError(f"the state must be a [{self._SAMPLE}, tile, x, y, feature] tensor")
        check_cube_shape(state.shape)
        if state.shape[-1] != s.channels:
            raise ValueError(f"the state has {state.shape[-1]} features, the network needs {s.channels}")
        if state.shape[2] != s.nx:
            raise ValueError(f"the state has faces of {state.shape[2]} cells per edge, the generator was built for nx = {s.nx}")
        if state.dtype != torch.float32:
            raise TypeError(f"the normalised state must be float32, got {state.dtype}")
        _require_device(state)
        return state.contiguous()


class GeneratorModel(_GeneratorRuntime):
    """One generator on one device.  ``forward`` works through the samples in chunks (see ``_GeneratorRuntime``)."""

    def __init__(self, spec: GeneratorSpec, convolution_type: str = "halo_conv2d", device="cuda",
                 workspace_limit: int = 2 << 30, max_chunk: int = REFERENCE_BATCH):
        super().__init__(spec, convolution_type, device, workspace_limit, max_chunk)
        self._bottom = spec.n_resnet > 0
        if spec.use_geographic_features or spec.use_geographic_bias:
            self._in_channels = spec.channels + (N_GEOGRAPHIC_FEATURES if spec.use_geographic_features else 0)
        self._embedded_bias = self._channel_last(spec.embedded_bias)
        self._lon = None if spec.lon is None else self._up(spec.lon)
        self._xyz = self._channel_last(spec.xyz)

    def _forward_chunk(self, state: torch.Tensor, theta: Optional[torch.Tensor], out: torch.Tensor):
        s = self.spec
        S, n, C = int(state.shape[0]), s.nx, s.channels
        cur = _Slice(state, C)
        if "in" in self._ws:
            dst = self._buf("in")
            _lib.call_on(self.device, "fv3hip_cyclegan_input", cur.ptr, C, 0, 0, _ptr(self._input_bias), _ptr(self._lon),
                         _ptr(self._xyz), _ptr(theta), dst.ptr, dst.ld, 0, 0, S, n, C, _stream(self.device))
            cur = dst
        cur, pend = self._down_chain(cur, _NONE, S, first_bias=self._embedded_bias)
        if s.n_resnet:
            nb, cb = n >> s.n_convolutions, s.min_filters * 2 ** s.n_convolutions
            x, a, b = self._buf("x"), self._buf("a"), self._buf("b")
            self._apply(cur, pend, x, S, nb, cb)
            for j in range(s.n_resnet):
                self._conv(f"res{j}.a", x, _NONE, a, S, nb)
                pa = self._stats("st:a", a, S, nb, cb)
                self._conv(f"res{j}.b", a, pa, b, S, nb)
                pb = self._stats("st:b", b, S, nb, cb, relu=False)
                self._apply(b, pb, x, S, nb, cb, res=x)
            cur, pend = x, _NONE
        self._up_chain(cur, pend, _Slice(out, C), S)

    def forward(self, state: torch.Tensor, theta: Optional[torch.Tensor] = None, chunk: Optional[int] = None) -> torch.Tensor:
        """Normalised ``[S, 6, n, n, C]`` float32 and ``theta`` ``[S]`` float32 (the local-time offset of every sample in
        radians; not needed without geographic features) -> the generated normalised state, a new tensor."""
        state = self._check_state(state)
        S = int(state.shape[0])
        if self.spec.use_geographic_features:
            if theta is None:
                raise ValueError("a generator with geographic features needs the time of every sample (theta)")
            theta = torch.as_tensor(theta, dtype=torch.float32).to(self.device).contiguous()
            if tuple(theta.shape) != (S,):
                raise ValueError(f"theta must have shape ({S},), got {tuple(theta.shape)}")
        else:
            theta = None
        out = torch.empty_like(state)
        for i, j in self._chunks(S, chunk):
            self._forward_chunk(state[i:j], None if theta is None else theta[i:j], out[i:j])
        return out


class CycleGanModel:
    """Both generators and the scalers of a ``CycleGanSpec`` on one device; a generator is uploaded when first used."""

    def __init__(self, spec: CycleGanSpec, device="cuda", **generator_kwargs):
        spec.validate()
        self.spec, self.device, self._kwargs = spec, cuda_device(device, "CycleGanModel"), generator_kwargs
        _lib.load()
        self._generators: Dict[bool, GeneratorModel] = {}
        self._packers = {d: StatePacker(spec.variables, *spec.scaler_arrays(d), self.device) for d in "ab"}

    def generator(self, reverse: bool = False) -> GeneratorModel:
        if reverse not in self._generators:
            self._generators[reverse] = GeneratorModel(self.spec.generator(reverse), self.spec.convolution_type, self.device, **self._kwargs)
        return self._generators[reverse]

    def pack(self, sources: Sequence[torch.Tensor], domain: str) -> torch.Tensor:
        """``sources[v]``: a ``[time, tile, x, y, level]`` view (any strides, float32 or float64) of state variable v ->
        float32 ``[time, 6, n, n, F]``, ``(x - mean) / std`` in float64 with the domain's scalers: one time per window."""
        return self._packers[domain].pack(sources, None, 1, 1).squeeze(1)

    def unpack(self, state: torch.Tensor, domain: str) -> List[torch.Tensor]:
        """Float32 ``[time, 6, n, n, F]`` -> per variable float64 ``[time, 6, n, n, nfeat]``, ``float64(x) * std + mean``."""
        return self._packers[domain].unpack(state)
