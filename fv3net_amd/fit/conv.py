"""The convolutional predictor: ``fv3fit``'s ``"convolutional"`` training function returns a ``PureKerasModel`` with
``unstacked_dims=("x", "y", "z")`` and ``n_halo = halos_required`` (external/fv3fit/fv3fit/keras/_models/convolutional.py:141-149);
``predict_on_dataset`` pads every tile with halos from its neighbours before the network runs
(_shared/xr_prediction.py:120-129).  ``HipConvolutionalModel`` is that predictor on the MI355X: the network runs in
``fv3hip_conv_predict``, which reads the dataset's arrays in place and takes the halo cells from the neighbouring faces of a
resident cube, or -- with the cube sharded by tile over ``torch.distributed`` ranks -- from strips exchanged in one
all-gather (``parallel.exchange_edge_strips``).  ``train_convolutional_model`` is the training function
(convolutional.py:101-150): Adam on the std-scaled MSE with the ``TransposeInvariant`` kernel constraint, through torch's
autograd or -- ``backend="hip"`` -- through the project's own kernels (``conv_train.ConvTrainer``).  The
artifact is ``name`` ("hip-convolutional") + ``config.yaml`` (the reference's four keys) + ``spec.yaml`` + ``weights.npz``.
"""
import dataclasses
import os
from typing import Any, Dict, Hashable, Iterable, List, Optional, Sequence

import numpy as np
import torch
import yaml

from ..conv import ConvInput, ConvModel, ConvOutput, ConvSpec, halos_required
from ..cubedsphere._device import compute_device, download_all, on_device
from ..xr_compat import DataArray, Dataset, from_compat, to_compat
from . import io
from .predictor import Predictor
from .stacking import match_prediction_to_input_coords
from .training import check_backend, epoch_minibatches, resolve_backend


@io.register("hip-convolutional")
class HipConvolutionalModel(Predictor):
    """Convolutional network over ``[x, y, z]`` fields with cube halos, running on the MI355X."""

    _CONFIG_FILENAME = "config.yaml"
    _SPEC_FILENAME = "spec.yaml"
    _WEIGHTS_FILENAME = "weights.npz"

    def __init__(self, input_variables: Iterable[Hashable], output_variables: Iterable[Hashable], model: ConvSpec,
                 unstacked_dims: Sequence[str] = ("x", "y", "z"), n_halo: Optional[int] = None):
        super().__init__(list(input_variables), list(output_variables))
        self.spec = model
        if n_halo is not None and int(n_halo) != model.halos_required:
            raise ValueError(f"n_halo = {n_halo}, but a network of depth {model.depth} with {model.kernel_size} x "
                             f"{model.kernel_size} kernels needs {model.halos_required} halo cells")
        self._n_halo = model.halos_required
        self._unstacked_dims = list(unstacked_dims)
        if len(self._unstacked_dims) != 3:
            raise ValueError(f"a convolutional model's unstacked_dims are (x, y, z), got {self._unstacked_dims}")
        if list(model.sources) != [str(v) for v in self.input_variables]:
            raise ValueError(f"input variables {self.input_variables} differ from the network's inputs {model.sources}")
        missing = [v for v in self.output_variables if v not in model.output_names]
        if missing:
            raise ValueError(f"output variables {missing} are not produced by the network ({model.output_names})")
        self._model: Optional[ConvModel] = None  # created on first predict (needs the GPU)

    @property
    def n_halo(self) -> int:
        return self._n_halo

    @property
    def model(self) -> ConvModel:
        if self._model is None:
            self._model = ConvModel(self.spec, device=compute_device())
        return self._model

    # -- prediction -------------------------------------------------------------------------
    def _halo_route(self, n_tile_dim: Optional[int], tile_coord):
        """('input' | 'cube' | 'exchange', this rank's tiles): where the halo cells come from."""
        from ..parallel import tiles_of_rank, world

        if self._n_halo == 0:
            return "input", None
        rank, size = world()
        if n_tile_dim is None:
            if size == 6:
                return "exchange", [rank]
            if size > 6 and size % 6 == 0:
                raise ValueError(f"{size} ranks: a tile split over several ranks (layout > 1) is out of scope of this "
                                 "predictor; run one rank per tile or give the whole cube")
            raise ValueError("either dataset must have tile dimension or MPI must be present")
        mine = list(range(6)) if (size == 1 or n_tile_dim == 6) else tiles_of_rank(size, rank)
        if n_tile_dim != len(mine) or not mine:
            raise ValueError(f"dataset must have exactly six tiles to append halos (or, sharded by tile, this rank's tiles "
                             f"{mine}), got {n_tile_dim}")
        if tile_coord is not None and np.asarray(tile_coord).tolist() != mine:
            raise ValueError(f"`tile` coordinate must be {mine}, in this order")
        return ("cube" if len(mine) == 6 else "exchange"), mine

    def predict(self, X):
        """Predict an output dataset from an input dataset whose variables have ``x`` and ``y`` (and, unless single-level,
        ``z``) dimensions, a ``tile`` dimension unless every rank holds one tile, and any batch dimensions, in any order.
        Does not mutate ``X``; host data in, host data out; device data in, device data out."""
        from ..cubedsphere.halos import edge_strips, halo_strips
        from ..parallel import exchange_edge_strips

        x = to_compat(X)
        xd, yd, zd = self._unstacked_dims
        arrays = {name: x[name] for name in self.input_variables}  # KeyError for a missing variable
        batch, sizes = [], {}
        for name, da in arrays.items():
            for dim in (xd, yd):
                if dim not in da.dims:
                    raise ValueError(f"variable {name!r} has no {dim!r} dimension")
            for dim, n in da.sizes.items():
                if sizes.setdefault(dim, n) != n:
                    raise ValueError(f"conflicting sizes for dimension {dim!r}")
                if dim not in (xd, yd, zd, "tile") and dim not in batch:
                    batch.append(dim)
        has_tile = "tile" in sizes
        route, mine = self._halo_route(sizes.get("tile"), x.coords.get("tile") if has_tile else None)
        lead = batch + (["tile"] if has_tile else [])
        host_input, sources = None, {}
        for i, (name, da) in zip(self.spec.inputs, arrays.items()):
            if set(da.dims) - {zd} != set(lead) | {xd, yd}:
                raise ValueError(f"variable {name!r} has dims {da.dims}, expected {lead + [xd, yd]} (and {zd!r})")
            if host_input is None:
                host_input = da.data
            t = on_device(da.data)
            names = list(da.dims)
            if zd not in names:
                t, names = t.unsqueeze(0), [zd] + names
            t = t.permute(*[names.index(dim) for dim in lead + [zd, yd, xd]])  # a view: the kernel reads through strides
            if route == "exchange" and not has_tile:
                t = t.unsqueeze(-4)
            sources[i.source] = t
        if route == "exchange":  # the one exchange step: the edge strips of this rank's tiles against everybody's
            h, nb = self._n_halo, len(batch)
            ts = list(sources.values())
            if any(t.dtype != ts[0].dtype for t in ts):
                ts = [t.to(torch.float64) for t in ts]
            # [batch.., tile, z, y, x] -> [tile, batch.., z, x, y] -> edges [tile, 4, h, batch.., z, n]
            edges = torch.cat([edge_strips(t.movedim(nb, 0).transpose(-1, -2), h) for t in ts], dim=-2)
            table = exchange_edge_strips(edges.contiguous())
            strips = halo_strips(table, mine)                                   # [tile, 4, h, batch.., C, n]
            strips = strips.permute(*range(3, 3 + nb), 0, 1, 2, 3 + nb, 4 + nb)   # [batch.., tile, 4, h, C, n]
            outs = self.model.predict(sources, halo="strips", strips=strips)
        else:
            outs = self.model.predict(sources, halo=route)

        shaped, dims_of = {}, {}
        nfeat = {o.name: o.nfeat for o in self.spec.outputs}
        for name in self.output_variables:
            t = outs[str(name)]
            if route == "exchange" and not has_tile:
                t = t.squeeze(-4)
            if nfeat[str(name)] == 1:
                shaped[name], dims_of[name] = t.squeeze(-3), tuple(lead + [yd, xd])
            else:
                shaped[name], dims_of[name] = t, tuple(lead + [zd, yd, xd])
        if not (isinstance(host_input, torch.Tensor) and host_input.is_cuda):
            shaped = download_all(shaped)  # host data in -> host data out, one copy for all outputs
        result = Dataset()
        for name in self.output_variables:
            result[name] = DataArray(shaped[name], dims=dims_of[name])
        return from_compat(match_prediction_to_input_coords(x, result), X)

    # -- serialisation ----------------------------------------------------------------------
    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        meta, arrays = self.spec.to_arrays()
        np.savez(os.path.join(path, self._WEIGHTS_FILENAME), **arrays)
        with open(os.path.join(path, self._SPEC_FILENAME), "w") as f:
            yaml.safe_dump(meta, f)
        with open(os.path.join(path, self._CONFIG_FILENAME), "w") as f:
            yaml.safe_dump(
                {"input_variables": list(self.input_variables), "output_variables": list(self.output_variables),
                 "unstacked_dims": list(self._unstacked_dims), "n_halo": self._n_halo}, f)

    @classmethod
    def load(cls, path: str) -> "HipConvolutionalModel":
        with open(os.path.join(path, cls._CONFIG_FILENAME)) as f:
            config = yaml.safe_load(f)
        with open(os.path.join(path, cls._SPEC_FILENAME)) as f:
            meta = yaml.safe_load(f)
        with np.load(os.path.join(path, cls._WEIGHTS_FILENAME), allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        return cls(config["input_variables"], config["output_variables"], ConvSpec.from_arrays(meta, arrays),
                   unstacked_dims=config.get("unstacked_dims", ("x", "y", "z")), n_halo=config.get("n_halo"))


def conv_spec_from_arrays(
    input_variables: Sequence[str],
    input_means: Sequence[np.ndarray],
    input_stds: Sequence[np.ndarray],
    hidden_kernels: Sequence[np.ndarray],
    hidden_biases: Optional[Sequence[np.ndarray]],
    output_variables: Sequence[str],
    output_kernels: Sequence[np.ndarray],
    output_biases: Sequence[np.ndarray],
    output_means: Sequence[np.ndarray],
    output_stds: Sequence[np.ndarray],
    activation: str = "relu",
    epsilon: float = 1e-7,
) -> ConvSpec:
    """Assemble the predict graph of convolutional.py:153-210 from its weights, Keras layouts: hidden kernels
    ``[k, k, c_in, filters]``, head kernels ``[1, 1, filters, z]`` (or ``[filters, z]``).  ``input_stds`` are the fitted standard
    deviations; the forward scale is ``std + epsilon`` in float32.  ``hidden_biases=None``: a network without them."""
    inputs = []
    for name, mean, std in zip(input_variables, input_means, input_stds):
        mean, std = np.atleast_1d(np.asarray(mean, np.float32)), np.atleast_1d(np.asarray(std, np.float32))
        inputs.append(ConvInput(str(name), int(mean.shape[0]), mean, std + np.float32(epsilon)))
    outputs = []
    for name, kern, bias, mean, std in zip(output_variables, output_kernels, output_biases, output_means, output_stds):
        kern = np.asarray(kern, np.float32)
        kern = kern.reshape(kern.shape[-2:])
        nf = int(kern.shape[1])
        outputs.append(ConvOutput(str(name), nf, kern, np.asarray(bias, np.float32).reshape(nf),
                                  np.broadcast_to(np.asarray(std, np.float32), (nf,)).copy(),
                                  np.broadcast_to(np.asarray(mean, np.float32), (nf,)).copy()))
    return ConvSpec(inputs, [np.asarray(k, np.float32) for k in hidden_kernels],
                    None if hidden_biases is None else [np.asarray(b, np.float32) for b in hidden_biases], outputs,
                    activation=activation)


# ---------------------------------------------------------------------------------------------
# offline training (PyTorch-ROCm, or the project's own kernels with backend="hip")
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class ConvolutionalHyperparameters:
    """fv3fit's ``ConvolutionalHyperparameters`` (convolutional.py:27-61) with its ``ConvolutionalNetworkConfig``
    (convolutional_network.py:59-101), ``TrainingLoopConfig`` and Adam's learning rate flattened into one class.  The fields
    after ``seed`` are accepted so that a reference configuration reads, but only at their defaults (see ``_REJECTED``)."""

    input_variables: List[str]
    output_variables: List[str]
    filters: int = 32
    depth: int = 3                      # convolutional layers, the 1 x 1 output layer included
    kernel_size: int = 3
    activation_function: str = "relu"
    transpose_invariant: bool = True
    epochs: int = 3
    batch_size: int = 1                 # tile-samples per step
    learning_rate: float = 1e-3
    normalization_fit_samples: int = 30   # one sample is one tile
    seed: int = 0
    diffusive: bool = False
    gaussian_noise: float = 0.0
    spectral_normalization: bool = False
    kernel_regularizer: Optional[Any] = None
    clip_config: Dict[Hashable, Any] = dataclasses.field(default_factory=dict)
    loss_type: str = "mse"
    loss_scaling: str = "standard"


# field -> the values it may have (the reference's defaults); the reference's conv graph never clips its outputs (build_model
# takes no clip_config, convolutional.py:153-210), so a clip_config would change the targets only
_REJECTED = {"diffusive": (False,), "gaussian_noise": (0.0, 0), "spectral_normalization": (False,), "kernel_regularizer": (None, "none"),
             "clip_config": ({}, None), "loss_type": ("mse",), "loss_scaling": ("standard",)}
_TWIN_ACTIVATIONS = {"relu": torch.relu, "linear": lambda v: v, "tanh": torch.tanh}


def _check_hyperparameters(hp: ConvolutionalHyperparameters, backend: str) -> None:
    for name, allowed in _REJECTED.items():
        value = getattr(hp, name)
        if not any(type(value) is type(a) and value == a for a in allowed):
            raise NotImplementedError(f"{name}={value!r} is not supported by train_convolutional_model (only {allowed[0]!r})")
    if hp.filters == 0:
        raise NotImplementedError("filters=0 causes a floating point exception, and we haven't written a workaround")
    halos_required(hp.kernel_size, hp.depth)
    if hp.activation_function not in _TWIN_ACTIVATIONS:
        raise ValueError(f"activation_function {hp.activation_function!r} is not supported; supported: {sorted(_TWIN_ACTIVATIONS)}")
    if backend == "hip" and hp.activation_function not in ("relu", "linear"):
        raise ValueError(f"backend='hip' trains with activation_function 'relu' or 'linear', got {hp.activation_function!r}; "
                         "use backend='torch'")
    if hp.batch_size < 1 or hp.epochs < 0:
        raise ValueError("batch_size must be positive and epochs not negative")


def _cubes_for_training(batches, names: Sequence[str]) -> List[np.ndarray]:
    """Every variable as float32 ``[sample, tile, x, y, z]`` (a variable without ``z`` gets a trailing axis of 1:
    convolutional.py:77-78), the batches concatenated along ``sample``."""
    from ..xr_compat import to_compat

    cols: List[List[np.ndarray]] = [[] for _ in names]
    for ds in batches:
        ds = to_compat(ds)
        for i, name in enumerate(names):
            da = ds[name]
            for dim in ("tile", "x", "y"):
                if dim not in da.dims:
                    raise ValueError(f"variable {name!r} must have 'tile', 'x', and 'y' dimensions, got {tuple(da.dims)}")
            zs = [d for d in da.dims if d in ("z", "z_interface")]
            lead = [d for d in da.dims if d not in ("tile", "x", "y") and d not in zs]
            a = np.asarray(da.transpose(*lead, "tile", "x", "y", *zs).values)
            nz = a.shape[-1] if zs else 1
            n_tiles, nx, ny = (da.sizes[d] for d in ("tile", "x", "y"))
            cols[i].append(a.reshape(-1, n_tiles, nx, ny, nz).astype(np.float32))
    return [np.concatenate(c, axis=0) for c in cols]


@dataclasses.dataclass
class _ConvTraining:
    """What both backends of ``train_convolutional_model`` start from: the fitted normalisation, the normalised halo-padded
    inputs, the targets and the freshly initialised layers (created on the host, so that the start does not depend on the
    device)."""

    n_halo: int
    xin: np.ndarray                 # [tile-sample, nx + 2 h, ny + 2 h, C] padded, then normalised
    y: List[np.ndarray]             # [tile-sample, nx, ny, nfeat] each
    x_mean: List[np.ndarray]
    x_std: List[np.ndarray]
    y_mean: List[np.ndarray]
    y_std: List[np.ndarray]
    loss_std: List[np.ndarray]
    hidden: List[torch.nn.Conv2d]   # weight [f, c, a, b]: the Keras kernel is weight.permute(2, 3, 1, 0)
    heads: List[torch.nn.Conv2d]


def _keras_kernel(conv: torch.nn.Conv2d) -> np.ndarray:
    return np.ascontiguousarray(conv.weight.detach().cpu().numpy().transpose(2, 3, 1, 0))


def _prepare_conv_training(hp: ConvolutionalHyperparameters, train_batches) -> _ConvTraining:
    """convolutional.py:64-98, 126-137 and shared/utils.py:84-105 on the host."""
    from ..cubedsphere.halos import append_halos

    torch.manual_seed(hp.seed)
    h = halos_required(hp.kernel_size, hp.depth)
    X5 = _cubes_for_training(train_batches, hp.input_variables)
    y5 = _cubes_for_training(train_batches, hp.output_variables)
    for a in X5 + y5:
        if a.shape[1] != 6:
            raise ValueError(f"dataset must have 6 tiles to halo update, got {a.shape[1]}")

    def pad_and_fold(a):   # [sample, tile, x, y, z] -> [sample * tile, x + 2 h, y + 2 h, z]
        if h > 0 and a.shape[2] == a.shape[3]:
            a = append_halos(np.ascontiguousarray(a.transpose(1, 0, 4, 2, 3)), h).transpose(1, 0, 3, 4, 2)
        elif h > 0:   # (not a cube: reported below with the reference's message)
            a = np.pad(a, ((0, 0), (0, 0), (h, h), (h, h), (0, 0)))
        return np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]))

    X = [pad_and_fold(a) for a in X5]
    y = [np.ascontiguousarray(a.reshape((-1,) + a.shape[2:])) for a in y5]
    for item in X + y:
        if item.shape[1] != item.shape[2]:
            raise ValueError(f"x and y dimensions should be the same length, got shape {item.shape}")
    nfit = hp.normalization_fit_samples
    flat = lambda a: a[:nfit].reshape(-1, a.shape[-1])   # halo cells and the raw-zero corners are part of the fit, as in the reference's X
    x_mean = [flat(a).mean(axis=0).astype(np.float32) for a in X]
    x_std = [flat(a).std(axis=0).astype(np.float32) for a in X]
    y_mean = [flat(a).mean(axis=0).astype(np.float32) for a in y]
    y_std = [flat(a).std(axis=0).astype(np.float32) for a in y]
    loss_std = [np.std(flat(a), axis=0, dtype=np.float32) for a in y]
    eps = np.float32(1e-7)
    xin = np.concatenate([(a - m) / (s + eps) for a, m, s in zip(X, x_mean, x_std)], axis=-1)   # padded first, normalised after

    def layer(c_in, c_out, k):   # Keras Conv2D default: glorot_uniform (fans k k c_in, k k c_out), zero bias
        conv = torch.nn.Conv2d(c_in, c_out, k)
        torch.nn.init.xavier_uniform_(conv.weight)
        torch.nn.init.zeros_(conv.bias)
        return conv

    hidden, fan = [], xin.shape[-1]
    for _ in range(hp.depth - 1):
        hidden.append(layer(fan, hp.filters, hp.kernel_size))
        fan = hp.filters
    heads = [layer(fan, a.shape[-1], 1) for a in y]
    return _ConvTraining(n_halo=h, xin=np.ascontiguousarray(xin, np.float32), y=y, x_mean=x_mean, x_std=x_std, y_mean=y_mean,
                         y_std=y_std, loss_std=loss_std, hidden=hidden, heads=heads)


def _conv_weights(prep: _ConvTraining):
    """The four weight lists of ``conv_spec_from_arrays`` from the (trained or fresh) torch layers."""
    return ([_keras_kernel(c) for c in prep.hidden], [c.bias.detach().cpu().numpy().copy() for c in prep.hidden],
            [_keras_kernel(c)[0, 0] for c in prep.heads], [c.bias.detach().cpu().numpy().copy() for c in prep.heads])


def _conv_batches(hp: ConvolutionalHyperparameters, n: int, dev: torch.device):
    """The minibatches of tile-samples, the same for both backends."""
    for batches in epoch_minibatches(n, hp.batch_size, hp.epochs, hp.seed, dev):
        yield from batches


def _train_conv_torch(hp: ConvolutionalHyperparameters, prep: _ConvTraining, dev: torch.device):
    """Adam on the std-scaled MSE through ``torch.nn.functional.conv2d`` and autograd; the kernel constraint after
    ``opt.step()``, where Keras applies it."""
    F = torch.nn.functional
    xin = torch.from_numpy(prep.xin).to(dev).permute(0, 3, 1, 2)   # [s, c, x, y]
    hidden, heads = [c.to(dev) for c in prep.hidden], [c.to(dev) for c in prep.heads]
    targets = [torch.from_numpy(a).to(dev) for a in prep.y]
    t_mean = [torch.from_numpy(m).to(dev) for m in prep.y_mean]
    t_std = [torch.from_numpy(s).to(dev) for s in prep.y_std]
    l_std = [torch.from_numpy(np.maximum(s, 1e-12)).to(dev) for s in prep.loss_std]
    act = _TWIN_ACTIVATIONS[hp.activation_function]
    params = [p for c in hidden + heads for p in c.parameters()]
    opt = torch.optim.Adam(params, lr=hp.learning_rate)
    for idx in _conv_batches(hp, xin.shape[0], dev):
        a = xin[idx]
        for c in hidden:
            a = act(F.conv2d(a, c.weight, c.bias))
        loss = 0.0
        for j, head in enumerate(heads):
            pred = F.conv2d(a, head.weight, head.bias).permute(0, 2, 3, 1) * t_std[j] + t_mean[j]
            loss = loss + torch.mean(((pred - targets[j][idx]) / l_std[j]) ** 2)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if hp.transpose_invariant:
            with torch.no_grad():
                for c in hidden:
                    c.weight.copy_(0.5 * (c.weight + c.weight.transpose(2, 3)))
    return _conv_weights(prep)


def conv_mse_loss(prep: _ConvTraining):
    """The loss of ``_train_conv_torch`` as the per-feature arrays the device step takes (``fv3net_amd.train.MseLoss``)."""
    from ..train import MseLoss

    nfs = [a.shape[-1] for a in prep.y]
    inv = [(1.0 / np.maximum(s, 1e-12).astype(np.float64) ** 2).astype(np.float32) for s in prep.loss_std]
    total = sum(nfs)
    return MseLoss(scale=np.concatenate(prep.y_std), center=np.concatenate(prep.y_mean), inv_cstd2=np.concatenate(inv),
                   lo=np.full(total, -np.inf, np.float32), hi=np.full(total, np.inf, np.float32), keep=np.ones(total, np.float32),
                   kept=np.concatenate([np.full(nf, nf, np.float64) for nf in nfs]))


def conv_trainer(hp: ConvolutionalHyperparameters, prep: _ConvTraining, dev: torch.device):
    """The device training state of ``backend="hip"``: the layers of ``prep``, the resident inputs and targets, the loss."""
    from ..conv_train import ConvTrainer

    kernels, biases, out_k, out_b = _conv_weights(prep)
    targets = np.concatenate([a.reshape(-1, a.shape[-1]) for a in prep.y], axis=1)
    return ConvTrainer(kernels, biases, np.concatenate(out_k, axis=1), np.concatenate(out_b), prep.xin, targets, conv_mse_loss(prep),
                       device=dev, max_batch=min(hp.batch_size, prep.xin.shape[0]), learning_rate=hp.learning_rate,
                       relu=hp.activation_function == "relu", transpose_invariant=hp.transpose_invariant)


def _train_conv_hip(hp: ConvolutionalHyperparameters, prep: _ConvTraining, dev: torch.device):
    """The same tile-samples in the same order through ``fv3net_amd.conv_train.ConvTrainer`` (csrc/conv_train.hip)."""
    trainer = conv_trainer(hp, prep, dev)
    for idx in _conv_batches(hp, prep.xin.shape[0], dev):
        trainer.step(idx)
    return trainer.parameters([a.shape[-1] for a in prep.y])


def train_convolutional_model(hyperparameters: ConvolutionalHyperparameters, train_batches, device: Optional[str] = None,
                              backend: Optional[str] = None) -> HipConvolutionalModel:
    """Pad every tile of ``train_batches`` (datasets whose variables have ``tile``, ``x``, ``y`` and, unless single-level, ``z``
    dimensions, plus any sample dimensions) with cube halos, fit the normalisation on the first ``normalization_fit_samples``
    tile-samples, train ``Conv2D(filters, k, valid, activation) x (depth - 1) -> 1 x 1 Conv2D per output`` with Adam on the
    std-scaled MSE, and return the predictor (convolutional.py:101-210).

    ``backend``: ``None`` / ``"torch"`` steps through ``torch.nn.functional.conv2d``, autograd and ``torch.optim.Adam``; ``"hip"``
    through the project's own kernels (needs a GPU).  Preparation, initialisation and the minibatch sequence are shared: both
    start from bitwise-equal parameters and see the same tile-samples in the same order."""
    hp = hyperparameters
    _check_hyperparameters(hp, check_backend(backend))   # (before the device is asked for: what is not built is refused anywhere)
    backend, dev = resolve_backend(backend, device)
    prep = _prepare_conv_training(hp, train_batches)

    def model(weights):
        spec = conv_spec_from_arrays(hp.input_variables, prep.x_mean, prep.x_std, weights[0], weights[1], hp.output_variables,
                                     weights[2], weights[3], prep.y_mean, prep.y_std, activation=hp.activation_function)
        return HipConvolutionalModel(hp.input_variables, hp.output_variables, spec, unstacked_dims=("x", "y", "z"), n_halo=prep.n_halo)

    model(_conv_weights(prep))   # (a network that cannot be saved -- depth = 1 -- fails here, before any step)
    return model((_train_conv_hip if backend == "hip" else _train_conv_torch)(hp, prep, dev))
