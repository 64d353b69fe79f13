"""The CycleGAN: ``fv3fit``'s ``"cycle_gan"`` training function returns a ``CycleGAN`` predictor
(external/fv3fit/fv3fit/pytorch/cyclegan/reloadable.py:43-253, generator.py:19-270) that translates the cubed-sphere state of
one climate into another, one time at a time.  ``HipCycleGAN`` is that predictor on the MI355X at predict time: the dataset's
arrays are normalised and packed in place by ``fv3hip_graph_pack``, the generator runs on the resident state through the
``fv3hip_cyclegan_*`` layer kernels, and ``fv3hip_graph_unpack`` writes ``predicted`` with the other domain's scalers.  The
artifact is ``name`` ("hip-cyclegan") + ``config.yaml`` (``state_variables``) + ``spec.yaml`` + ``weights.npz``; it carries both
generators, the ``a_*`` / ``b_*`` scalers and no discriminators.  ``lon`` and ``xyz``, which the reference reads from a grid
catalogue, are data of the model here.

``GeneratorTwin`` is the generator in plain ``torch.nn`` plus ``append_halos_tensor`` with the reference's parameter names: the
float32 / float64 chain that the tests and the benchmark compare the kernels with.
"""
import os
from typing import Any, Dict, Mapping, Optional, Sequence

import numpy as np
import torch
import yaml

from ..cubedsphere._device import compute_device, download_all, on_device
from ..cubedsphere.halos import append_halos_tensor, append_halos_tensor_reference_order
from ..cyclegan import (N_GEOGRAPHIC_FEATURES, SECONDS_PER_DAY, CycleGanModel, CycleGanSpec, GeneratorSpec, check_architecture,
                        check_convolution_type, check_grid, layer_plan, seconds_since_1970, theta_from_seconds)
from ..xr_compat import DataArray, Dataset, from_compat, to_compat
from . import io
from .predictor import Predictor

_LEAD_DIMS = ("time", "tile", "x", "y")
_OUT_DIMS = ("time", "tile", "x", "y", "z")
nn = torch.nn


# ---------------------------------------------------------------------------------------------
# the network in plain torch, module for module as the reference nests them
# ---------------------------------------------------------------------------------------------
class _Fold(nn.Module):
    """``FoldFirstDimension``: a ``[batch, channel, x, y]`` module on ``[batch, tile, channel, x, y]`` data."""

    def __init__(self, wrapped):
        super().__init__()
        self._wrapped = wrapped

    def forward(self, x):
        y = self._wrapped(x.reshape(-1, *x.shape[2:]))
        return y.reshape(x.shape[0], x.shape[1], *y.shape[1:])


class _AppendHalos(nn.Module):
    """``reference_order_gradients`` (off unless a trainer turns it on, ``set_reference_order_gradients``): pad tile by tile, so
    that autograd adds a cell's gradient terms in the order of the reference's ``AppendHalos``; the values are the same."""

    def __init__(self, n_halo: int):
        super().__init__()
        self.n_halo = n_halo
        self.reference_order_gradients = False

    def forward(self, x):   # [batch, tile, channel, x, y]
        if self.reference_order_gradients:
            return append_halos_tensor_reference_order(x, self.n_halo, tile_dim=1)
        return append_halos_tensor(x.movedim(1, 0), self.n_halo).movedim(0, 1)


def set_reference_order_gradients(network: nn.Module, on: bool = True) -> nn.Module:
    """Every halo padding of a twin: batched (``append_halos_tensor``, the default) or tile by tile in the reference's order of
    gradient accumulation (``append_halos_tensor_reference_order``: bitwise the reference's float64 gradients, six autograd
    nodes and six full-size zero tensors per pad in the backward pass)."""
    for module in network.modules():
        if isinstance(module, _AppendHalos):
            module.reference_order_gradients = bool(on)
    return network


class _Crop(nn.Module):
    def __init__(self, n_halo: int):
        super().__init__()
        self.n_halo = n_halo

    def forward(self, x):
        return x[..., self.n_halo:-self.n_halo, self.n_halo:-self.n_halo].contiguous()


class _GeographicBias(nn.Module):
    def __init__(self, channels: int, nx: int):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(6, channels, nx, nx))

    def forward(self, x):
        return x + self.bias


def _single_tile_convolution(c_in, c_out, k, stride=1, transpose=False, padding=None):
    padding = (k - 1) // 2 if padding is None else padding
    if transpose:
        return _Fold(nn.ConvTranspose2d(c_in, c_out, k, stride=stride, padding=padding))
    return _Fold(nn.Conv2d(c_in, c_out, k, stride=stride, padding=padding))


def _halo_convolution(c_in, c_out, k, stride=1, transpose=False):
    padding = (k - 1) // 2
    conv = _single_tile_convolution(c_in, c_out, k, stride, transpose, padding=0)
    if transpose:
        conv = nn.Sequential(conv, _Crop(padding * stride + (k - 1) // 2))
    return nn.Sequential(_AppendHalos(padding), conv)


class _ConvBlock(nn.Module):
    def __init__(self, conv, c_out, relu=True):
        super().__init__()
        self.conv_block = nn.Sequential(conv, _Fold(nn.InstanceNorm2d(c_out)), nn.ReLU() if relu else nn.Identity())

    def forward(self, x):
        return self.conv_block(x)


class _ResnetBlock(nn.Module):
    def __init__(self, channels, conv):
        super().__init__()
        self.conv_block = nn.Sequential(_ConvBlock(conv(channels, channels), channels), _ConvBlock(conv(channels, channels), channels, relu=False))
        self.identity = nn.Identity()

    def forward(self, x):
        return self.conv_block(x) + self.identity(x)


class _EncoderDecoder(nn.Module):
    def __init__(self, down, up, bottom, depth, c):
        super().__init__()
        self._down = down(c, 2 * c)
        self._up = up(2 * c, c)
        self._lower = bottom(2 * c) if depth == 1 else _EncoderDecoder(down, up, bottom, depth - 1, 2 * c)

    def forward(self, x):
        return self._up(self._lower(self._down(x)))


class GeneratorTwin(nn.Module):
    """``Generator`` (generator.py:82-212) with ``lon`` ``[6, nx, nx]`` and ``xyz`` ``[6, 3, nx, nx]`` given, not read from a
    catalogue; its ``state_dict`` has the reference's keys.  ``forward(time, state)``: ``time`` ``[batch]`` seconds since 1970,
    ``state`` ``[batch, tile, channel, x, y]``."""

    def __init__(self, channels: int, nx: int, n_convolutions: int = 3, n_resnet: int = 3, kernel_size: int = 3,
                 strided_kernel_size: int = 4, max_filters: int = 256, use_geographic_bias: bool = True,
                 use_geographic_features: bool = True, use_geographic_embedded_bias: bool = False,
                 convolution_type: str = "halo_conv2d", lon=None, xyz=None, disable_convolutions: bool = False):
        super().__init__()
        check_architecture(n_convolutions, n_resnet, kernel_size, strided_kernel_size, max_filters, disable_convolutions)
        check_convolution_type(convolution_type)
        check_grid(nx, nx, n_convolutions)
        conv = _halo_convolution if convolution_type == "halo_conv2d" else _single_tile_convolution
        m, k4 = int(max_filters / 2 ** n_convolutions), strided_kernel_size
        first = [conv(channels + (N_GEOGRAPHIC_FEATURES if use_geographic_features else 0), m, 7), _Fold(nn.InstanceNorm2d(m))]
        if use_geographic_embedded_bias:
            first.append(_GeographicBias(m, nx))
        first.append(nn.ReLU())
        encoder_decoder = _EncoderDecoder(
            down=lambda ci, co: _ConvBlock(conv(ci, co, k4, stride=2), co),
            up=lambda ci, co: _ConvBlock(conv(ci, co, k4, stride=2, transpose=True), co),
            bottom=lambda c: nn.Sequential(*[_ResnetBlock(c, lambda ci, co: conv(ci, co, kernel_size)) for _ in range(n_resnet)]),
            depth=n_convolutions, c=m)
        self._main = nn.Sequential(nn.Sequential(*first), encoder_decoder, nn.Sequential(conv(m, channels, 7)))
        self._input_bias = _GeographicBias(channels, nx) if use_geographic_bias else nn.Identity()
        self._output_bias = _GeographicBias(channels, nx) if use_geographic_bias else nn.Identity()
        self.use_geographic_features = use_geographic_features
        if use_geographic_features:
            if lon is None or xyz is None:
                raise ValueError("a generator with geographic features needs lon [6, nx, nx] and xyz [6, 3, nx, nx]")
            # plain attributes, as in the reference: not part of the state dict
            self.local_time_zero_radians = torch.as_tensor(np.asarray(lon)).float()[:, None]
            self.xyz = torch.as_tensor(np.asarray(xyz)).float()

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self.use_geographic_features:
            self.local_time_zero_radians, self.xyz = fn(self.local_time_zero_radians), fn(self.xyz)
        return self

    def forward(self, time, state):
        x = self._input_bias(state)
        if self.use_geographic_features:
            offset = time % SECONDS_PER_DAY / SECONDS_PER_DAY * 2 * np.pi
            local = self.local_time_zero_radians[None, :] + offset[:, None, None, None, None]
            xyz = torch.stack([self.xyz for _ in range(x.shape[0])])
            x = torch.cat([x, torch.sin(local), torch.cos(local), xyz], dim=-3)
        return self._output_bias(self._main(x))


def _module_path(name: str, n_convolutions: int, halo: bool) -> str:
    """``layer_plan`` name -> the state-dict prefix of its ``Conv2d`` / ``ConvTranspose2d``."""
    wrapped = "1._wrapped" if halo else "_wrapped"
    if name == "first":
        return f"_main.0.0.{wrapped}"
    if name == "last":
        return f"_main.2.0.{wrapped}"
    if name.startswith("res"):
        j, ab = name[3:].split(".")
        return "_main.1" + "._lower" * n_convolutions + f".{j}.conv_block.{'ab'.index(ab)}.conv_block.0.{wrapped}"
    level = int(name[4:] if name.startswith("down") else name[2:])
    base = "_main.1" + "._lower" * level
    if name.startswith("down"):
        return f"{base}._down.conv_block.0.{wrapped}"
    return f"{base}._up.conv_block.0." + ("1.0._wrapped" if halo else "_wrapped")


def _generator_keys(spec_like: Mapping[str, Any], halo: bool) -> Dict[str, str]:
    """spec array name (``first.weight``, ``input_bias`` ...) -> state-dict key."""
    plan = layer_plan(spec_like["channels"], spec_like["n_convolutions"], spec_like["n_resnet"], spec_like["kernel_size"],
                      spec_like["max_filters"], spec_like["use_geographic_features"])
    keys = {}
    for name, *_ in plan:
        path = _module_path(name, spec_like["n_convolutions"], halo)
        keys[f"{name}.weight"], keys[f"{name}.bias"] = f"{path}.weight", f"{path}.bias"
    if spec_like["use_geographic_bias"]:
        keys["input_bias"], keys["output_bias"] = "_input_bias.bias", "_output_bias.bias"
    if spec_like["use_geographic_embedded_bias"]:
        keys["embedded_bias"] = "_main.0.2.bias"
    return keys


def generator_spec_from_state_dict(state_dict: Mapping[str, Any], channels: int, nx: int, n_convolutions: int = 3, n_resnet: int = 3,
                                   kernel_size: int = 3, strided_kernel_size: int = 4, max_filters: int = 256,
                                   use_geographic_bias: bool = True, use_geographic_features: bool = True,
                                   use_geographic_embedded_bias: bool = False, convolution_type: str = "halo_conv2d", lon=None,
                                   xyz=None, disable_convolutions: bool = False, prefix: str = "") -> GeneratorSpec:
    """One ``Generator.state_dict()`` (a plain mapping of its keys to arrays or tensors) as a spec."""
    check_architecture(n_convolutions, n_resnet, kernel_size, strided_kernel_size, max_filters, disable_convolutions)
    check_convolution_type(convolution_type)
    halo = convolution_type == "halo_conv2d"
    cfg = dict(channels=channels, n_convolutions=n_convolutions, n_resnet=n_resnet, kernel_size=kernel_size, max_filters=max_filters,
               use_geographic_bias=use_geographic_bias, use_geographic_features=use_geographic_features,
               use_geographic_embedded_bias=use_geographic_embedded_bias)

    def arr(key):
        try:
            a = state_dict[prefix + key]
        except KeyError as missing:
            raise ValueError(f"the state dict has no {missing}") from missing
        return np.ascontiguousarray(np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a), np.float32)

    got = {name: arr(key) for name, key in _generator_keys(cfg, halo).items()}
    if use_geographic_features and (lon is None or xyz is None):
        raise ValueError("a generator with geographic features needs lon [6, nx, nx] and xyz [6, 3, nx, nx]")
    geo = lambda a: np.ascontiguousarray(a, np.float32) if use_geographic_features else None
    return GeneratorSpec(channels, nx, {k[:-7]: v for k, v in got.items() if k.endswith(".weight")},
                         {k[:-5]: v for k, v in got.items() if k.endswith(".bias")}, n_convolutions, n_resnet, kernel_size,
                         strided_kernel_size, max_filters, got.get("input_bias"), got.get("output_bias"), got.get("embedded_bias"),
                         geo(lon), geo(xyz))


def _scaler_pair(s):
    mean, std = (s.mean, s.std) if hasattr(s, "mean") else s
    if mean is None or std is None:
        raise ValueError("a scaler has not been fit")
    mean = np.atleast_1d(np.asarray(mean, np.float64))
    return mean, np.broadcast_to(np.atleast_1d(np.asarray(std, np.float64)), mean.shape).copy()


def cyclegan_spec_from_state_dict(state_dict: Mapping[str, Any], state_variables: Sequence[str], scalers: Mapping[str, Any], nx: int,
                                  convolution_type: str = "halo_conv2d", lon=None, xyz=None, **generator_config) -> CycleGanSpec:
    """The reference's trained ``CycleGANModule`` as a spec.  ``state_dict``: a plain mapping keyed as
    ``CycleGANModule.state_dict()`` (``generator_a_to_b....``, ``generator_b_to_a....``; discriminator entries are ignored);
    ``scalers``: ``"a_<name>"`` / ``"b_<name>"`` -> a ``StandardScaler`` (an object with ``mean`` and ``std``) or a
    ``(mean, std)`` pair; ``generator_config``: the fields of ``GeneratorConfig``."""
    pairs = {f"{d}_{name}": _scaler_pair(scalers[f"{d}_{name}"]) for d in "ab" for name in state_variables}
    variables = [(str(name), int(pairs[f"a_{name}"][0].shape[0])) for name in state_variables]
    channels = sum(f for _, f in variables)
    gens = [generator_spec_from_state_dict(state_dict, channels, nx, convolution_type=convolution_type, lon=lon, xyz=xyz,
                                           prefix=f"generator_{key}.", **generator_config) for key in ("a_to_b", "b_to_a")]
    return CycleGanSpec(gens[0], gens[1], variables, pairs, convolution_type)


def generator_state_dict(spec: GeneratorSpec, convolution_type: str = "halo_conv2d", prefix: str = "") -> Dict[str, torch.Tensor]:
    meta, arrays = spec.to_arrays()
    keys = _generator_keys(meta, convolution_type == "halo_conv2d")
    return {prefix + key: torch.from_numpy(np.array(arrays[name])) for name, key in keys.items()}


def state_dict_from_spec(spec: CycleGanSpec) -> Dict[str, torch.Tensor]:
    """The inverse of ``cyclegan_spec_from_state_dict``: the generators' part of ``CycleGANModule.state_dict()``."""
    out = generator_state_dict(spec.generator_a_to_b, spec.convolution_type, "generator_a_to_b.")
    out.update(generator_state_dict(spec.generator_b_to_a, spec.convolution_type, "generator_b_to_a."))
    return out


cyclegan_state_dict_from_spec = state_dict_from_spec     # (the name under which ``fit`` exports it, beside the graph model's)


def twin_from_spec(spec: GeneratorSpec, convolution_type: str = "halo_conv2d", dtype=torch.float32, device="cpu") -> GeneratorTwin:
    twin = GeneratorTwin(spec.channels, spec.nx, spec.n_convolutions, spec.n_resnet, spec.kernel_size, spec.strided_kernel_size,
                         spec.max_filters, spec.use_geographic_bias, spec.use_geographic_features, spec.use_geographic_embedded_bias,
                         convolution_type, spec.lon, spec.xyz)
    twin.load_state_dict(generator_state_dict(spec, convolution_type), strict=True)
    return twin.to(device=device, dtype=dtype).eval()


# ---------------------------------------------------------------------------------------------
# the predictor
# ---------------------------------------------------------------------------------------------
@io.register("hip-cyclegan")
class HipCycleGAN(Predictor):
    """CycleGAN generators over the six-tile cube, running on the MI355X."""

    _CONFIG_FILENAME = "config.yaml"
    _SPEC_FILENAME = "spec.yaml"
    _WEIGHTS_FILENAME = "weights.npz"
    _REFERENCE_MODEL_FILENAME = "weight.pt"

    _DISCRIMINATOR_PREFIX = "discriminators."

    def __init__(self, state_variables: Sequence[str], model: CycleGanSpec, discriminators: Optional[Mapping[str, Any]] = None):
        """``discriminators`` (optional; ``fit.train_cyclegan`` gives them, ``predict`` never reads them): ``{"config": the
        fields of ``DiscriminatorTwin``, "state_dict": {"discriminator_a.<key>": array, "discriminator_b.<key>": array}}``."""
        super().__init__(list(state_variables), list(state_variables))
        self.state_variables = list(state_variables)
        self.spec = model
        self.discriminators = None if discriminators is None else {
            "config": dict(discriminators["config"]),
            "state_dict": {str(k): np.ascontiguousarray(np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v),
                                                        np.float32) for k, v in discriminators["state_dict"].items()}}
        self.history: Optional[Dict[str, list]] = None   # per-epoch losses, where the model was trained here
        if [str(v) for v in self.state_variables] != model.state_variables:
            raise ValueError(f"state variables {self.state_variables} differ from the network's {model.state_variables}")
        self._model: Optional[CycleGanModel] = None   # created on first predict (needs the GPU)

    @property
    def model(self) -> CycleGanModel:
        if self._model is None:
            self._model = CycleGanModel(self.spec, device=compute_device())
        return self._model

    def _sources(self, x: Dataset):
        """Per state variable the array as it lies in the dataset and its dims; every shape is checked here, on the host."""
        found, sizes = [], None
        for name, nfeat in self.spec.variables:
            da = x[name]   # KeyError for a missing variable
            dims = list(da.dims)
            if set(dims) - {"z"} != set(_LEAD_DIMS) or len(dims) != len(set(dims)):
                raise ValueError(f"received variable {name} with unexpected dimensions {tuple(dims)}: expected "
                                 f"{_LEAD_DIMS} (and 'z'), in any order")
            nz = da.sizes["z"] if "z" in dims else 1
            if nz != nfeat:
                raise ValueError(f"variable {name!r} has {nz} levels, the model was trained with {nfeat}")
            lead = tuple(int(da.sizes[d]) for d in _LEAD_DIMS)
            if lead[1] != 6:
                raise ValueError(f"variable {name!r} must hold the six tiles of the cube, got {lead[1]} tiles")
            if sizes is not None and lead != sizes:
                raise ValueError(f"variable {name!r} has (time, tile, x, y) = {lead}, the variables before it {sizes}")
            sizes = lead
            found.append((da, dims))
        gen = self.spec.generator_a_to_b
        check_grid(sizes[2], sizes[3], gen.n_convolutions)
        if sizes[2] != gen.nx:
            raise ValueError(f"the data has faces of {sizes[2]} cells per edge, the model was built for nx = {gen.nx}")
        return found, sizes

    def predict(self, X, reverse: bool = False):
        """``X``: the state variables with dims ``time, tile, x, y`` (and ``z``) in any order, float32 or float64, and ``time``
        (``datetime64``, seconds since 1970, or ``cftime`` objects).  Returns the state translated from domain a to domain b
        (``reverse``: from b to a) with dims ``[time, tile, x, y(, z)]``, float64, and ``time`` as given.  Does not mutate ``X``;
        host data in, host data out (one download); device data in, device data out."""
        x = to_compat(X)
        found, sizes = self._sources(x)
        generator_spec = self.spec.generator(reverse)
        theta = None
        if generator_spec.use_geographic_features:
            if "time" not in x:
                raise ValueError("the dataset needs a 'time' variable: the generator appends the local time of day")
            seconds = seconds_since_1970(x["time"])
            if seconds.shape != (sizes[0],):
                raise ValueError(f"'time' has shape {seconds.shape}, the state variables {sizes[0]} times")
            theta = torch.from_numpy(theta_from_seconds(seconds))
        host_input, views = None, []
        for da, dims in found:
            if host_input is None:
                host_input = da.data
            t = on_device(da.data)
            if t.dtype not in (torch.float32, torch.float64):
                t = t.to(torch.float64)
            if "z" not in dims:
                t, dims = t.unsqueeze(-1), dims + ["z"]
            views.append(t.permute(*[dims.index(d) for d in _LEAD_DIMS + ("z",)]))   # a view: the kernel reads through strides
        model = self.model
        src, dst = ("b", "a") if reverse else ("a", "b")
        state = model.pack(views, src)
        generated = model.generator(reverse).forward(state, theta)
        shaped, dims_of = {}, {}
        for (name, nfeat), t in zip(self.spec.variables, model.unpack(generated, dst)):
            shaped[name] = t.squeeze(-1) if nfeat == 1 else t
            dims_of[name] = _OUT_DIMS[:4] if nfeat == 1 else _OUT_DIMS
        if not (isinstance(host_input, torch.Tensor) and host_input.is_cuda):
            shaped = download_all(shaped)
        ds = Dataset()
        for name in self.state_variables:
            ds[name] = DataArray(shaped[str(name)], dims=dims_of[str(name)])
        if "time" in x:
            ds["time"] = x["time"]
        return from_compat(ds, X)

    # -- serialisation ----------------------------------------------------------------------
    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        meta, arrays = self.spec.to_arrays()
        if self.discriminators is not None:   # (written only when present: an artifact without them is byte for byte as before)
            meta["discriminators"] = self.discriminators["config"]
            arrays.update({self._DISCRIMINATOR_PREFIX + k: v for k, v in self.discriminators["state_dict"].items()})
        np.savez(os.path.join(path, self._WEIGHTS_FILENAME), **arrays)
        with open(os.path.join(path, self._SPEC_FILENAME), "w") as f:
            yaml.safe_dump(meta, f)
        with open(os.path.join(path, self._CONFIG_FILENAME), "w") as f:
            yaml.safe_dump({"state_variables": [str(v) for v in self.state_variables]}, f)

    @classmethod
    def load(cls, path: str) -> "HipCycleGAN":
        if not os.path.exists(os.path.join(path, cls._WEIGHTS_FILENAME)):
            if os.path.exists(os.path.join(path, cls._REFERENCE_MODEL_FILENAME)):
                raise ValueError(f"{path} holds the reference's {cls._REFERENCE_MODEL_FILENAME}, a pickled torch module that is not "
                                 "read here; where fv3fit exists, export it with HipCycleGAN(state_variables, "
                                 "cyclegan_spec_from_state_dict(model.state_dict(), state_variables, scalers, nx, ...)).dump(path)")
            raise ValueError(f"{path} holds no {cls._WEIGHTS_FILENAME}")
        with open(os.path.join(path, cls._CONFIG_FILENAME)) as f:
            config = yaml.safe_load(f)
        with open(os.path.join(path, cls._SPEC_FILENAME)) as f:
            meta = yaml.safe_load(f)
        with np.load(os.path.join(path, cls._WEIGHTS_FILENAME), allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        discriminators = None
        if "discriminators" in meta:
            n = len(cls._DISCRIMINATOR_PREFIX)
            discriminators = {"config": meta["discriminators"],
                              "state_dict": {k[n:]: v for k, v in arrays.items() if k.startswith(cls._DISCRIMINATOR_PREFIX)}}
        return cls(config["state_variables"], CycleGanSpec.from_arrays(meta, arrays), discriminators)
