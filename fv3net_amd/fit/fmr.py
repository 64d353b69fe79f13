"""The full-model replacement: ``fv3fit``'s ``"fmr"`` model (external/fv3fit/fv3fit/pytorch/recurrent/reloadable.py:26-154)
wraps a ``RecurrentGenerator`` (recurrent/generator.py:185-400) that encodes the normalised cubed-sphere state once, steps the
latent forward in time and decodes every step.  ``HipFullModelReplacement`` is that predictor on the MI355X at predict time:
the dataset's arrays are normalised and packed into windows in place by ``fv3hip_graph_pack``, the rollout runs on the resident
state through the ``fv3hip_cyclegan_*`` layer kernels (the step layers read their context channels through
``fv3hip_cyclegan_conv_context``), and ``fv3hip_graph_unpack`` writes ``predicted`` and ``reference``.  The artifact is ``name``
("hip-fmr") + ``config.yaml`` (``state_variables``) + ``spec.yaml`` + ``weights.npz``; it carries the generator, the scalers
(keyed by the variable's name) and the two ``xyz`` tables the reference reads from a grid catalogue, and -- only where
``fit.train_fmr`` wrote it -- the discriminator, from which training resumes.

``RecurrentGeneratorTwin`` is the generator in plain ``torch.nn`` with the reference's parameter names: the float32 / float64
chain that the tests and the benchmark compare the kernels with.
"""
import os
from typing import Any, Dict, Mapping, Optional, Sequence

import numpy as np
import torch
import yaml

from ..cubedsphere._device import compute_device, download_all, on_device
from ..cyclegan import check_architecture, check_convolution_type, check_grid
from ..fmr import (N_CLOCK, N_XYZ, FullModelReplacementModel, FullModelReplacementSpec, RecurrentGeneratorSpec, check_filters,
                   check_step_type, layer_plan)
from ..xr_compat import DataArray, Dataset, from_compat, to_compat
from . import io
from .cyclegan import _ConvBlock, _Fold, _GeographicBias, _halo_convolution, _scaler_pair, _single_tile_convolution
from .graph import n_windows_of
from .predictor import Predictor

_LEAD_DIMS = ("time", "tile", "x", "y")
_OUT_DIMS = ("window", "time", "tile", "x", "y", "z")
nn = torch.nn


# ---------------------------------------------------------------------------------------------
# the network in plain torch, module for module as the reference nests them
# ---------------------------------------------------------------------------------------------
class _GeographicFeatures(nn.Module):
    """Appends x, y, z of every cell; ``xyz`` ``[6, 3, n, n]`` is a plain attribute, as in the reference: not in the state dict."""

    def __init__(self, xyz):
        super().__init__()
        self.xyz = torch.as_tensor(np.asarray(xyz)).float()

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self.xyz = fn(self.xyz)
        return self

    def forward(self, x):   # [sample, tile, channel, x, y]
        return torch.concat([x, torch.stack([self.xyz for _ in range(x.shape[0])], dim=0)], dim=-3)


class _DiurnalFeatures(nn.Module):
    """generator.py:127-153: sin and cos of the hour hand, the float64 value assigned into a float32 tensor (so a ``.double()``
    generator reads the float32 values too); the clock then advances."""

    def __init__(self, samples_per_day: int):
        super().__init__()
        self.samples_per_day = samples_per_day
        self.clock = 0

    def reset(self):
        self.clock = 0

    def forward(self, x):   # [sample, channel, x, y]
        features = torch.zeros(x.shape[0], 2, x.shape[2], x.shape[3], device=x.device, dtype=torch.float32)
        features[:, 0, :, :] = np.sin(2 * np.pi * self.clock / self.samples_per_day)
        features[:, 1, :, :] = np.cos(2 * np.pi * self.clock / self.samples_per_day)
        self.clock = (self.clock + 1) % self.samples_per_day
        return torch.cat([x, features], dim=-3)


def _pass_context(out, inputs, context_channels):
    if context_channels > 0:
        out = torch.cat([out, torch.zeros_like(inputs[:, :, -context_channels:, :])], dim=-3)
    return out


class _ContextResnetBlock(nn.Module):
    def __init__(self, channels, conv, context_channels):
        super().__init__()
        self.conv_block = nn.Sequential(_ConvBlock(conv(channels + context_channels, channels), channels),
                                        _ConvBlock(conv(channels, channels), channels, relu=False))
        self.identity = nn.Identity()
        self.context_channels = context_channels

    def forward(self, x):
        return _pass_context(self.conv_block(x), x, self.context_channels) + self.identity(x)


class _PersistContext(nn.Module):
    def __init__(self, op, context_channels):
        super().__init__()
        self.op = op
        self.context_channels = context_channels

    def forward(self, x):
        return _pass_context(self.op(x), x, self.context_channels)


class _SelectChannels(nn.Module):
    def __init__(self, stop):
        super().__init__()
        self._slice = slice(0, stop, 1)

    def forward(self, x):
        return x[..., self._slice, :, :]


class RecurrentGeneratorTwin(nn.Module):
    """``RecurrentGenerator`` with ``xyz`` ``[6, 3, nx, nx]`` and ``xyz_bottom`` ``[6, 3, nx >> n_convolutions, ...]`` given, not
    read from a catalogue; its ``state_dict`` has the reference's keys for both convolution types.  ``forward(state, ntime)``:
    ``[batch, tile, channel, x, y]`` -> ``[batch, time, tile, channel, x, y]``."""

    def __init__(self, channels: int, nx: int, n_convolutions: int = 3, n_resnet: int = 3, kernel_size: int = 3,
                 strided_kernel_size: int = 4, max_filters: int = 256, use_geographic_bias: bool = True,
                 use_geographic_features: bool = True, step_type: str = "resnet", samples_per_day: Optional[int] = None,
                 convolution_type: str = "halo_conv2d", xyz=None, xyz_bottom=None):
        super().__init__()
        check_architecture(n_convolutions, n_resnet, kernel_size, strided_kernel_size, max_filters)
        check_step_type(step_type)
        check_filters(n_convolutions, max_filters)
        check_convolution_type(convolution_type)
        check_grid(nx, nx, n_convolutions)
        if use_geographic_features and (xyz is None or xyz_bottom is None):
            raise ValueError("a generator with geographic features needs xyz [6, 3, nx, nx] and xyz_bottom at nx >> n_convolutions")
        conv = _halo_convolution if convolution_type == "halo_conv2d" else _single_tile_convolution
        m, k4, mf = int(max_filters / 2 ** n_convolutions), strided_kernel_size, max_filters
        n_xyz = N_XYZ if use_geographic_features else 0
        ctx = n_xyz + (N_CLOCK if samples_per_day is not None else 0)
        step_conv = lambda ci, co: conv(ci, co, kernel_size)
        self.first_conv = nn.Sequential(conv(channels + n_xyz, m, 7), _Fold(nn.InstanceNorm2d(m)), nn.ReLU())
        self.encoder = nn.Sequential(*[_ConvBlock(conv(m * 2 ** i, m * 2 ** (i + 1), k4, stride=2), m * 2 ** (i + 1))
                                       for i in range(n_convolutions)])
        context_modules = []
        if use_geographic_features:
            context_modules.append(_GeographicFeatures(xyz_bottom))
        self.clock = None
        if samples_per_day is not None:
            self.clock = _DiurnalFeatures(samples_per_day)
            context_modules.append(_Fold(self.clock))
        if step_type == "resnet":
            step = nn.Sequential(*[_ContextResnetBlock(mf, step_conv, ctx) for _ in range(n_resnet)])
        else:
            step = _PersistContext(nn.Sequential(_ConvBlock(step_conv(mf + ctx, mf), mf), _ConvBlock(step_conv(mf, mf), mf)), ctx)
        self.resnet = nn.Sequential(*context_modules, step, _SelectChannels(mf))
        self.decoder = nn.Sequential(*[_ConvBlock(conv(int(mf / 2 ** i), int(mf / 2 ** (i + 1)), k4, stride=2, transpose=True),
                                                  int(mf / 2 ** (i + 1))) for i in range(n_convolutions)])
        self.out_conv = nn.Sequential(conv(m, channels, 7))
        self.input_bias = _GeographicBias(channels, nx) if use_geographic_bias else nn.Identity()
        self.output_bias = _GeographicBias(channels, nx) if use_geographic_bias else nn.Identity()
        if use_geographic_features:
            self.input_bias = nn.Sequential(self.input_bias, _GeographicFeatures(xyz))

    def forward(self, inputs, ntime: int):
        if self.clock is not None:
            self.clock.reset()
        x = self._encode(inputs)
        out_states = [self._decode(x)]
        for _ in range(ntime - 1):
            x = self._step(x)
            out_states.append(self._decode(x))
        return torch.stack(out_states, dim=1)

    def _encode(self, inputs):
        return self.encoder(self.first_conv(self.input_bias(inputs)))

    def _step(self, x):
        return self.resnet(x)

    def _decode(self, x):
        return self.output_bias(self.out_conv(self.decoder(x)))


def _module_path(name: str, spec_like: Mapping[str, Any], halo: bool) -> str:
    """``layer_plan`` name -> the state-dict prefix of its ``Conv2d`` / ``ConvTranspose2d``."""
    wrapped = "1._wrapped" if halo else "_wrapped"
    nc = spec_like["n_convolutions"]
    if name == "first":
        return f"first_conv.0.{wrapped}"
    if name == "last":
        return f"out_conv.0.{wrapped}"
    if name.startswith("down"):
        return f"encoder.{int(name[4:])}.conv_block.0.{wrapped}"
    if name.startswith("up"):
        return f"decoder.{nc - 1 - int(name[2:])}.conv_block.0." + ("1.0._wrapped" if halo else "_wrapped")
    at = int(bool(spec_like["use_geographic_features"])) + int(spec_like["samples_per_day"] is not None)   # after the context modules
    stem, ab = name.split(".")
    block = f"resnet.{at}.op" if stem == "step" else f"resnet.{at}.{int(stem[3:])}.conv_block"
    return f"{block}.{'ab'.index(ab)}.conv_block.0.{wrapped}"


def _generator_keys(spec_like: Mapping[str, Any], halo: bool) -> Dict[str, str]:
    """spec array name (``first.weight``, ``input_bias`` ...) -> state-dict key."""
    plan = layer_plan(spec_like["channels"], spec_like["n_convolutions"], spec_like["n_resnet"], spec_like["kernel_size"],
                      spec_like["max_filters"], spec_like["step_type"], spec_like["use_geographic_features"],
                      spec_like["samples_per_day"])
    keys = {}
    for name, *_ in plan:
        path = _module_path(name, spec_like, halo)
        keys[f"{name}.weight"], keys[f"{name}.bias"] = f"{path}.weight", f"{path}.bias"
    if spec_like["use_geographic_bias"]:
        keys["input_bias"] = "input_bias.0.bias" if spec_like["use_geographic_features"] else "input_bias.bias"
        keys["output_bias"] = "output_bias.bias"
    return keys


def recurrent_generator_spec_from_state_dict(state_dict: Mapping[str, Any], channels: int, nx: int, n_convolutions: int = 3,
                                             n_resnet: int = 3, kernel_size: int = 3, strided_kernel_size: int = 4,
                                             max_filters: int = 256, use_geographic_bias: bool = True,
                                             use_geographic_features: bool = True, step_type: str = "resnet",
                                             samples_per_day: Optional[int] = None, convolution_type: str = "halo_conv2d", xyz=None,
                                             xyz_bottom=None, prefix: str = "") -> RecurrentGeneratorSpec:
    """One ``RecurrentGenerator.state_dict()`` (a plain mapping of its keys to arrays or tensors) as a spec."""
    check_architecture(n_convolutions, n_resnet, kernel_size, strided_kernel_size, max_filters)
    check_step_type(step_type)
    check_convolution_type(convolution_type)
    cfg = dict(channels=channels, n_convolutions=n_convolutions, n_resnet=n_resnet, kernel_size=kernel_size, max_filters=max_filters,
               use_geographic_bias=use_geographic_bias, use_geographic_features=use_geographic_features, step_type=step_type,
               samples_per_day=samples_per_day)

    def arr(key):
        try:
            a = state_dict[prefix + key]
        except KeyError as missing:
            raise ValueError(f"the state dict has no {missing}") from missing
        return np.ascontiguousarray(np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a), np.float32)

    got = {name: arr(key) for name, key in _generator_keys(cfg, convolution_type == "halo_conv2d").items()}
    if use_geographic_features and (xyz is None or xyz_bottom is None):
        raise ValueError("a generator with geographic features needs xyz [6, 3, nx, nx] and xyz_bottom at nx >> n_convolutions")
    geo = lambda a: np.ascontiguousarray(a, np.float32) if use_geographic_features else None
    return RecurrentGeneratorSpec(channels, nx, {k[:-7]: v for k, v in got.items() if k.endswith(".weight")},
                                  {k[:-5]: v for k, v in got.items() if k.endswith(".bias")}, n_convolutions, n_resnet, kernel_size,
                                  strided_kernel_size, max_filters, step_type, samples_per_day, got.get("input_bias"),
                                  got.get("output_bias"), geo(xyz), geo(xyz_bottom))


def fmr_spec_from_state_dict(state_dict: Mapping[str, Any], state_variables: Sequence[str], scalers: Mapping[str, Any], nx: int,
                             convolution_type: str = "halo_conv2d", xyz=None, xyz_bottom=None,
                             **generator_config) -> FullModelReplacementSpec:
    """The reference's trained ``FMRModule`` as a spec.  ``state_dict``: a plain mapping keyed as ``FMRModule.state_dict()``
    (``generator....``; discriminator entries are ignored); ``scalers``: the variable's name -> a ``StandardScaler`` (an object
    with ``mean`` and ``std``) or a ``(mean, std)`` pair; ``xyz`` / ``xyz_bottom``: ``get_grid_xyz`` at ``nx`` and at
    ``nx >> n_convolutions`` as ``GeographicFeatures`` holds them, ``[6, 3, n, n]``; ``generator_config``: the fields of
    ``RecurrentGeneratorConfig``."""
    pairs = {str(name): _scaler_pair(scalers[name]) for name in state_variables}
    variables = [(str(name), int(pairs[str(name)][0].shape[0])) for name in state_variables]
    generator = recurrent_generator_spec_from_state_dict(state_dict, sum(f for _, f in variables), nx, convolution_type=convolution_type,
                                                         xyz=xyz, xyz_bottom=xyz_bottom, prefix="generator.", **generator_config)
    return FullModelReplacementSpec(generator, variables, pairs, convolution_type)


def recurrent_generator_state_dict(spec: RecurrentGeneratorSpec, convolution_type: str = "halo_conv2d",
                                   prefix: str = "") -> Dict[str, torch.Tensor]:
    meta, arrays = spec.to_arrays()
    keys = _generator_keys(meta, convolution_type == "halo_conv2d")
    return {prefix + key: torch.from_numpy(np.array(arrays[name])) for name, key in keys.items()}


def fmr_state_dict_from_spec(spec: FullModelReplacementSpec) -> Dict[str, torch.Tensor]:
    """The inverse of ``fmr_spec_from_state_dict``: the generator's part of ``FMRModule.state_dict()``."""
    return recurrent_generator_state_dict(spec.generator, spec.convolution_type, "generator.")


def recurrent_twin_from_spec(spec: RecurrentGeneratorSpec, convolution_type: str = "halo_conv2d", dtype=torch.float32,
                             device="cpu") -> RecurrentGeneratorTwin:
    twin = RecurrentGeneratorTwin(spec.channels, spec.nx, spec.n_convolutions, spec.n_resnet, spec.kernel_size,
                                  spec.strided_kernel_size, spec.max_filters, spec.use_geographic_bias, spec.use_geographic_features,
                                  spec.step_type, spec.samples_per_day, convolution_type, spec.xyz, spec.xyz_bottom)
    twin.load_state_dict(recurrent_generator_state_dict(spec, convolution_type), strict=True)
    return twin.to(device=device, dtype=dtype).eval()


# ---------------------------------------------------------------------------------------------
# the predictor
# ---------------------------------------------------------------------------------------------
def window_times(n_times: int, timesteps: int) -> np.ndarray:
    """``[n_windows, timesteps + 1]``: the index into the dataset's times of every time of every window
    (pytorch/predict.py:326-352): window ``w`` holds times ``w * timesteps ... (w + 1) * timesteps``, so its last time is the
    next window's first; times after ``n_windows * timesteps`` are dropped."""
    return np.arange(n_windows_of(n_times, timesteps))[:, None] * int(timesteps) + np.arange(int(timesteps) + 1)[None, :]


@io.register("hip-fmr")
class HipFullModelReplacement(Predictor):
    """The full-model-replacement recurrent generator over the six-tile cube, running on the MI355X."""

    _CONFIG_FILENAME = "config.yaml"
    _SPEC_FILENAME = "spec.yaml"
    _WEIGHTS_FILENAME = "weights.npz"
    _REFERENCE_MODEL_FILENAME = "weight.pt"
    _DISCRIMINATOR_PREFIX = "discriminator."

    def __init__(self, state_variables: Sequence[str], model: FullModelReplacementSpec, discriminator: Optional[Mapping[str, Any]] = None):
        """``discriminator`` (optional; ``fit.train_fmr`` gives it so that ``reload_path`` can resume, ``predict`` never reads
        it): ``{"config": the fields of ``DiscriminatorTwin``, "state_dict": its parameters under the reference's keys}``."""
        super().__init__(list(state_variables), list(state_variables))
        self.state_variables = list(state_variables)
        self.spec = model
        self.discriminator = None if discriminator is None else {
            "config": dict(discriminator["config"]),
            "state_dict": {str(k): np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, np.float32)
                           for k, v in discriminator["state_dict"].items()}}
        if [str(v) for v in self.state_variables] != model.state_variables:
            raise ValueError(f"state variables {self.state_variables} differ from the network's {model.state_variables}")
        self._model: Optional[FullModelReplacementModel] = None   # created on first predict (needs the GPU)

    @property
    def model(self) -> FullModelReplacementModel:
        if self._model is None:
            self._model = FullModelReplacementModel(self.spec, device=compute_device())
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
        gen = self.spec.generator
        check_grid(sizes[2], sizes[3], gen.n_convolutions)
        if sizes[2] != gen.nx:
            raise ValueError(f"the data has faces of {sizes[2]} cells per edge, the model was built for nx = {gen.nx}")
        return found, sizes

    @staticmethod
    def _views(found):
        """Per state variable a ``[time, tile, x, y, z]`` device view, and whether the dataset was resident."""
        host_input, views = found[0][0].data, []
        for da, dims in found:
            t = on_device(da.data)
            if t.dtype not in (torch.float32, torch.float64):
                t = t.to(torch.float64)
            if "z" not in dims:
                t, dims = t.unsqueeze(-1), dims + ["z"]
            views.append(t.permute(*[dims.index(d) for d in _LEAD_DIMS + ("z",)]))   # a view: the kernel reads through strides
        return views, isinstance(host_input, torch.Tensor) and host_input.is_cuda

    def pack_to_tensor(self, ds, timesteps: int) -> torch.Tensor:
        """The dataset as normalised float32 windows ``[window, time, tile, x, y, feature]`` on the device
        (pytorch/predict.py:299-360): ``(n_times - 1) // timesteps`` windows of ``timesteps + 1`` times, each window's last time
        the next one's first, trailing times dropped; ``(x - mean) / std`` in float64, then float32."""
        found, sizes = self._sources(to_compat(ds))
        n_windows = n_windows_of(sizes[0], timesteps)
        return self.model.pack(self._views(found)[0], n_windows, timesteps)

    def unpack_tensor(self, data: torch.Tensor, on_host: bool = True) -> Dataset:
        """Normalised ``[window, time, tile, x, y, feature]`` -> a dataset of float64 ``[window, time, tile, x, y(, z)]``
        variables, ``float64(x) * std + mean``."""
        shaped, dims_of = {}, {}
        for (name, nfeat), t in zip(self.spec.variables, self.model.unpack(data)):
            shaped[name] = t.squeeze(-1) if nfeat == 1 else t
            dims_of[name] = _OUT_DIMS[:5] if nfeat == 1 else _OUT_DIMS
        if on_host:
            shaped = download_all(shaped)
        ds = Dataset()
        for name in self.state_variables:
            ds[name] = DataArray(shaped[str(name)], dims=dims_of[str(name)])
        return ds

    def step_model(self, state: torch.Tensor, timesteps: int) -> torch.Tensor:
        """Normalised ``[sample, tile, x, y, feature]`` -> ``[sample, time, tile, x, y, feature]`` with ``timesteps + 1`` times:
        time 0 is the generator's reconstruction of the state, not a copy of it."""
        if timesteps < 1:
            raise ValueError(f"timesteps must be at least 1, got {timesteps}")
        return self.model.generator.forward(state, timesteps + 1)

    def predict(self, X, timesteps: int):
        """``X``: the state variables with dims ``time, tile, x, y`` (and ``z``) in any order, float32 or float64.  Returns
        ``(predicted, reference)`` with dims ``[window, time, tile, x, y(, z)]``, float64: window ``w`` starts at time
        ``w * timesteps``, has ``timesteps + 1`` times and, in ``predicted``, is rolled out from its first time.  Does not
        mutate ``X``; host data in, host data out (one download per dataset); device data in, device data out."""
        x = to_compat(X)
        found, sizes = self._sources(x)
        n_windows = n_windows_of(sizes[0], timesteps)
        views, resident = self._views(found)
        tensor = self.model.pack(views, n_windows, timesteps)
        outputs = self.step_model(tensor[:, 0], timesteps)
        predicted, reference = (from_compat(self.unpack_tensor(t, on_host=not resident), X) for t in (outputs, tensor))
        return predicted, reference

    # -- serialisation ----------------------------------------------------------------------
    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        meta, arrays = self.spec.to_arrays()
        if self.discriminator is not None:   # (written only when present: an artifact without it is byte for byte as before)
            meta["discriminator"] = self.discriminator["config"]
            arrays.update({self._DISCRIMINATOR_PREFIX + k: v for k, v in self.discriminator["state_dict"].items()})
        np.savez(os.path.join(path, self._WEIGHTS_FILENAME), **arrays)
        with open(os.path.join(path, self._SPEC_FILENAME), "w") as f:
            yaml.safe_dump(meta, f)
        with open(os.path.join(path, self._CONFIG_FILENAME), "w") as f:
            yaml.safe_dump({"state_variables": [str(v) for v in self.state_variables]}, f)

    @classmethod
    def load(cls, path: str) -> "HipFullModelReplacement":
        if not os.path.exists(os.path.join(path, cls._WEIGHTS_FILENAME)):
            if os.path.exists(os.path.join(path, cls._REFERENCE_MODEL_FILENAME)):
                raise ValueError(f"{path} holds the reference's {cls._REFERENCE_MODEL_FILENAME}, a pickled torch module that is not "
                                 "read here; where fv3fit exists, export it with HipFullModelReplacement(state_variables, "
                                 "fmr_spec_from_state_dict(model.model.state_dict(), state_variables, scalers, nx, ...)).dump(path)")
            raise ValueError(f"{path} holds no {cls._WEIGHTS_FILENAME}")
        with open(os.path.join(path, cls._CONFIG_FILENAME)) as f:
            config = yaml.safe_load(f)
        with open(os.path.join(path, cls._SPEC_FILENAME)) as f:
            meta = yaml.safe_load(f)
        with np.load(os.path.join(path, cls._WEIGHTS_FILENAME), allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        discriminator = None
        if "discriminator" in meta:
            n = len(cls._DISCRIMINATOR_PREFIX)
            discriminator = {"config": meta["discriminator"],
                             "state_dict": {k[n:]: v for k, v in arrays.items() if k.startswith(cls._DISCRIMINATOR_PREFIX)}}
        return cls(config["state_variables"], FullModelReplacementSpec.from_arrays(meta, arrays), discriminator)
