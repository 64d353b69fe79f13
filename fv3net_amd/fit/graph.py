"""The graph autoregressor: ``fv3fit``'s ``"graph"`` training function trains a ``GraphUNet`` and returns a
``PytorchAutoregressor`` (external/fv3fit/fv3fit/pytorch/graph/train.py:65-119, graph/unet.py:216-261, pytorch/predict.py:136-250),
a global emulator that steps the whole cubed-sphere state forward in time.  ``HipGraphAutoregressor`` is that predictor on the
MI355X: the dataset's arrays are normalised and packed in place by ``fv3hip_graph_pack``, the rollout runs on the resident state
through ``fv3hip_graph_sage`` / ``_pool2`` / ``_up2`` with no copy to the host between steps, and ``fv3hip_graph_unpack`` writes
``predicted`` and ``reference``.  The artifact is ``name`` ("hip-graph-autoregressor") + ``config.yaml`` (``state_variables``) +
``spec.yaml`` + ``weights.npz``.

``GraphUNetTwin`` is the network in plain torch (an index gather, a mean and ``nn.Linear``; no dgl) with the reference's
parameter names: it is what ``train_graph_model`` trains, and the float32 / float64 chain that the tests and the benchmark
compare the kernels with.
"""
import copy
import dataclasses
import os
from typing import Any, Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch
import yaml

from ..cubedsphere._device import compute_device, download_all, on_device
from ..graph import (GraphModel, GraphUNetSpec, GraphVariable, SageLayer, UpLayer, check_architecture, check_cube_shape,
                     layer_plan)
from ..xr_compat import DataArray, Dataset, from_compat, to_compat
from . import io
from .training import check_backend, epoch_minibatches, resolve_backend

_TORCH_ACTIVATIONS = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "linear": torch.nn.Identity}
_LEAD_DIMS = ("time", "tile", "x", "y")
_OUT_DIMS = ("window", "time", "tile", "x", "y", "z")


# ---------------------------------------------------------------------------------------------
# the network in plain torch
# ---------------------------------------------------------------------------------------------
_TABLES: Dict[Any, torch.Tensor] = {}


def neighbour_table(n: int, device="cpu") -> torch.Tensor:
    """``[6 n n, 5]`` cell ids: the cell itself, then its x-low, x-high, y-low and y-high neighbours, taken across the cube seams
    as the one-cell halo of ``append_halos`` shows them (graph_builder.py:12-49 builds its edges the same way)."""
    from ..cubedsphere.halos import append_halos_tensor

    key = (int(n), str(device))
    if key not in _TABLES:
        ids = torch.arange(6 * n * n, dtype=torch.int64).reshape(6, n, n)
        p = append_halos_tensor(ids, 1)
        table = torch.stack([ids, p[:, :-2, 1:-1], p[:, 2:, 1:-1], p[:, 1:-1, :-2], p[:, 1:-1, 2:]], dim=-1)
        _TABLES[key] = table.reshape(-1, 5).to(device)
    return _TABLES[key]


class _SageMean(torch.nn.Module):
    """dgl 0.9's ``SAGEConv(c_in, c_out, "mean")`` on the five-point graph, parameters named as dgl names them."""

    def __init__(self, c_in: int, c_out: int):
        super().__init__()
        self.fc_self = torch.nn.Linear(c_in, c_out, bias=False)
        self.fc_neigh = torch.nn.Linear(c_in, c_out, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(c_out))
        gain = torch.nn.init.calculate_gain("relu")      # dgl's reset_parameters
        torch.nn.init.xavier_uniform_(self.fc_self.weight, gain=gain)
        torch.nn.init.xavier_uniform_(self.fc_neigh.weight, gain=gain)

    def forward(self, x):   # [S, 6, n, n, c]
        S, _, n, _, c = x.shape
        flat = x.reshape(S, 6 * n * n, c)
        mean = flat[:, neighbour_table(n, x.device)].mean(dim=2)   # the gathered copy [S, N, 5, c] the kernel never makes
        return (self.fc_self(flat) + self.fc_neigh(mean) + self.bias).reshape(S, 6, n, n, -1)


class _CubeOp(torch.nn.Module):
    def __init__(self, graph_op):
        super().__init__()
        self.graph_op = graph_op

    def forward(self, x):
        return self.graph_op(x)


class _DoubleConv(torch.nn.Module):
    def __init__(self, c_in, c_hidden, act):
        super().__init__()
        self.conv = torch.nn.Sequential(_CubeOp(_SageMean(c_in, c_hidden)), act(), _CubeOp(_SageMean(c_hidden, c_hidden)), act())

    def forward(self, x):
        return self.conv(x)


class _Up(torch.nn.Module):
    def __init__(self, c_in):
        super().__init__()
        self.up = torch.nn.ConvTranspose2d(c_in, c_in // 2, kernel_size=2, stride=2)

    def forward(self, x):
        S, _, n, _, c = x.shape
        y = self.up(x.permute(0, 1, 4, 2, 3).reshape(S * 6, c, n, n))
        return y.reshape(S, 6, c // 2, 2 * n, 2 * n).permute(0, 1, 3, 4, 2)


class _UNet(torch.nn.Module):
    def __init__(self, depth, c, act):
        super().__init__()
        self.conv1 = _DoubleConv(c, 2 * c, act)
        self.conv2 = _DoubleConv(4 * c, 2 * c, act)
        self._lower = _DoubleConv(2 * c, 4 * c, act) if depth == 1 else _UNet(depth - 1, 2 * c, act)
        self._up = _Up(4 * c)

    def forward(self, x):
        before = self.conv1(x)
        S, _, n, _, c = before.shape
        pooled = before.reshape(S, 6, n // 2, 2, n // 2, 2, c).mean(dim=(3, 5))
        return self.conv2(torch.cat([before, self._up(self._lower(pooled))], dim=-1))


class GraphUNetTwin(torch.nn.Module):
    """``GraphUNet`` (unet.py:216-261) without dgl; its ``state_dict`` has the reference's keys."""

    def __init__(self, n_features: int, depth: int = 1, min_filters: int = 4, activation: str = "relu"):
        super().__init__()
        check_architecture(activation=activation)
        if depth < 1:
            raise ValueError(f"depth must be at least 1, got {depth}")
        act = _TORCH_ACTIVATIONS[activation]
        self._first_conv = torch.nn.Sequential(_CubeOp(_SageMean(n_features, min_filters)), act())
        self._last_conv = _CubeOp(_SageMean(2 * min_filters, n_features))
        self._unet = _UNet(depth, min_filters, act)

    def forward(self, x):
        return self._last_conv(self._unet(self._first_conv(x)))


def _module_prefix(name: str, depth: int) -> str:
    """``layer_plan`` name -> the reference's module path (without ``graph_op`` / ``up``)."""
    if name == "first":
        return "_first_conv.0"
    if name == "last":
        return "_last_conv"
    where, what = name.split(".")
    level = depth if where == "bottom" else int(where[1:])
    base = "_unet" + "._lower" * level
    if where == "bottom":
        return f"{base}.conv.{0 if what == 'a' else 2}"
    if what == "up":
        return f"{base}._up"
    return f"{base}.{what[:5]}.conv.{0 if what[5] == 'a' else 2}"


def graph_unet_spec_from_state_dict(state_variables: Sequence[str], state_dict: Mapping[str, Any], scalers: Mapping[str, Any],
                                    depth: int = 1, min_filters: int = 4, activation: str = "relu") -> GraphUNetSpec:
    """The reference's trained module as a spec: ``state_dict`` is any mapping of the names of ``GraphUNet.state_dict()`` to
    arrays (``_first_conv.0.graph_op.fc_self.weight`` ...), ``scalers`` maps every state variable to its ``StandardScaler`` (an
    object with ``mean`` and ``std``) or to a ``(mean, std)`` pair.  Per SAGE layer whichever of ``bias``, ``fc_self.bias`` and
    ``fc_neigh.bias`` are present are summed (dgl 0.9 keeps one bias, older releases one per linear map)."""
    check_architecture(activation=activation)

    def arr(key):
        a = state_dict[key]
        return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)

    variables = []
    for name in state_variables:
        s = scalers[name]
        mean, std = (s.mean, s.std) if hasattr(s, "mean") else s
        if mean is None or std is None:
            raise ValueError(f"the scaler of {name!r} has not been fit")
        mean, std = np.atleast_1d(np.asarray(mean, np.float64)), np.atleast_1d(np.asarray(std, np.float64))
        variables.append(GraphVariable(str(name), int(mean.shape[0]), mean, np.broadcast_to(std, mean.shape).copy()))
    layers: Dict[str, Any] = {}
    for name, kind, ci, co, _ in layer_plan(depth, sum(v.nfeat for v in variables), min_filters):
        prefix = _module_prefix(name, depth)
        try:
            if kind == "up":
                w = arr(f"{prefix}.up.weight").astype(np.float32)               # [c_in, c_out, kx, ky]
                layers[name] = UpLayer(np.ascontiguousarray(w.transpose(0, 2, 3, 1)), arr(f"{prefix}.up.bias").astype(np.float32))
                continue
            op = f"{prefix}.graph_op"
            bias = np.zeros(co, np.float32)
            for key in (f"{op}.bias", f"{op}.fc_self.bias", f"{op}.fc_neigh.bias"):
                if key in state_dict:
                    bias = bias + arr(key).astype(np.float32)
            layers[name] = SageLayer(np.ascontiguousarray(arr(f"{op}.fc_self.weight").astype(np.float32).T),
                                     np.ascontiguousarray(arr(f"{op}.fc_neigh.weight").astype(np.float32).T), bias)
        except KeyError as missing:
            raise ValueError(f"the state dict has no {missing} (layer {name!r} of a depth-{depth} GraphUNet)") from missing
    return GraphUNetSpec(variables, int(depth), int(min_filters), activation, layers)


def state_dict_from_spec(spec: GraphUNetSpec) -> Dict[str, torch.Tensor]:
    """The inverse of ``graph_unet_spec_from_state_dict`` in dgl 0.9's layout: what ``GraphUNetTwin.load_state_dict`` takes."""
    out = {}
    for name, kind, *_ in spec.plan:
        prefix, layer = _module_prefix(name, spec.depth), spec.layers[name]
        if kind == "up":
            out[f"{prefix}.up.weight"] = torch.from_numpy(np.ascontiguousarray(np.asarray(layer.weight).transpose(0, 3, 1, 2)))
            out[f"{prefix}.up.bias"] = torch.from_numpy(np.array(layer.bias))
        else:
            out[f"{prefix}.graph_op.fc_self.weight"] = torch.from_numpy(np.ascontiguousarray(np.asarray(layer.w_self).T))
            out[f"{prefix}.graph_op.fc_neigh.weight"] = torch.from_numpy(np.ascontiguousarray(np.asarray(layer.w_neigh).T))
            out[f"{prefix}.graph_op.bias"] = torch.from_numpy(np.array(layer.bias))
    return out


def twin_from_spec(spec: GraphUNetSpec, dtype=torch.float32, device="cpu") -> GraphUNetTwin:
    twin = GraphUNetTwin(spec.n_features, spec.depth, spec.min_filters, spec.activation)
    twin.load_state_dict(state_dict_from_spec(spec))
    return twin.to(device=device, dtype=dtype).eval()


# ---------------------------------------------------------------------------------------------
# the predictor
# ---------------------------------------------------------------------------------------------
def n_windows_of(n_times: int, timesteps: int) -> int:
    """predict.py:326-330: windows of ``timesteps + 1`` times that share their end points; trailing times that do not fill a
    window are dropped."""
    if timesteps < 1:
        raise ValueError(f"timesteps must be at least 1, got {timesteps}")
    n = (int(n_times) - 1) // int(timesteps)
    if n < 1:
        raise ValueError(f"{n_times} times do not hold one window of {timesteps} steps")
    return n


@io.register("hip-graph-autoregressor")
class HipGraphAutoregressor:
    """Graph U-Net autoregressor over the six-tile cube, running on the MI355X."""

    _CONFIG_FILENAME = "config.yaml"
    _SPEC_FILENAME = "spec.yaml"
    _WEIGHTS_FILENAME = "weights.npz"
    _REFERENCE_MODEL_FILENAME = "weight.pt"

    def __init__(self, state_variables: Sequence[str], model: GraphUNetSpec):
        self.state_variables = list(state_variables)
        self.spec = model
        if [str(v) for v in self.state_variables] != model.state_variables:
            raise ValueError(f"state variables {self.state_variables} differ from the network's {model.state_variables}")
        self._model: Optional[GraphModel] = None   # created on first predict (needs the GPU)

    @property
    def model(self) -> GraphModel:
        if self._model is None:
            self._model = GraphModel(self.spec, device=compute_device())
        return self._model

    def _sources(self, x: Dataset):
        """Per state variable the array as it lies in the dataset and its dims; every shape is checked here, on the host."""
        found, sizes = [], None
        for v in self.spec.variables:
            da = x[v.name]   # KeyError for a missing variable
            dims = list(da.dims)
            if set(dims) - {"z"} != set(_LEAD_DIMS) or len(dims) != len(set(dims)):
                raise ValueError(f"received variable {v.name} with unexpected dimensions {tuple(dims)}: expected "
                                 f"{_LEAD_DIMS} (and 'z'), in any order")
            nz = da.sizes["z"] if "z" in dims else 1
            if nz != v.nfeat:
                raise ValueError(f"variable {v.name!r} has {nz} levels, the model was trained with {v.nfeat}")
            lead = tuple(int(da.sizes[d]) for d in _LEAD_DIMS)
            check_cube_shape(lead[1:] + (nz,), f"variable {v.name!r}")
            if sizes is not None and lead != sizes:
                raise ValueError(f"variable {v.name!r} has (time, tile, x, y) = {lead}, the variables before it {sizes}")
            sizes = lead
            found.append((da, dims))
        self.spec.check_grid(sizes[2])
        return found, sizes

    def predict(self, X, timesteps: int):
        """``X``: the state variables with dims ``time, tile, x, y`` (and ``z``) in any order, float32 or float64.  Returns
        ``(predicted, reference)`` with dims ``[window, time, tile, x, y(, z)]``, float64: window ``w`` starts at time
        ``w * timesteps``, has ``timesteps + 1`` times and, in ``predicted``, is rolled out from its first time.  Does not
        mutate ``X``; host data in, host data out (one download); device data in, device data out."""
        x = to_compat(X)
        found, sizes = self._sources(x)
        n_windows = n_windows_of(sizes[0], timesteps)
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
        state = model.pack(views, n_windows, timesteps)
        rolled = model.rollout(state[:, 0], timesteps)
        shaped, dims_of = {}, {}
        for kind, tensor in (("predicted", rolled), ("reference", state)):
            for v, t in zip(self.spec.variables, model.unpack(tensor)):
                shaped[kind, v.name] = t.squeeze(-1) if v.nfeat == 1 else t
                dims_of[v.name] = _OUT_DIMS[:5] if v.nfeat == 1 else _OUT_DIMS
        if not (isinstance(host_input, torch.Tensor) and host_input.is_cuda):
            shaped = download_all(shaped)
        results = []
        for kind in ("predicted", "reference"):
            ds = Dataset()
            for name in self.state_variables:
                ds[name] = DataArray(shaped[kind, str(name)], dims=dims_of[str(name)])
            results.append(from_compat(ds, X))
        return results[0], results[1]

    # -- serialisation ----------------------------------------------------------------------
    def dump(self, path: str) -> None:
        os.makedirs(path, exist_ok=True)
        meta, arrays = self.spec.to_arrays()
        np.savez(os.path.join(path, self._WEIGHTS_FILENAME), **arrays)
        with open(os.path.join(path, self._SPEC_FILENAME), "w") as f:
            yaml.safe_dump(meta, f)
        with open(os.path.join(path, self._CONFIG_FILENAME), "w") as f:
            yaml.safe_dump({"state_variables": [str(v) for v in self.state_variables]}, f)

    @classmethod
    def load(cls, path: str) -> "HipGraphAutoregressor":
        if not os.path.exists(os.path.join(path, cls._WEIGHTS_FILENAME)):
            if os.path.exists(os.path.join(path, cls._REFERENCE_MODEL_FILENAME)):
                raise ValueError(f"{path} holds the reference's {cls._REFERENCE_MODEL_FILENAME}, a pickled torch module that needs "
                                 "dgl to be read; where dgl exists, export it with HipGraphAutoregressor(state_variables, "
                                 "graph_unet_spec_from_state_dict(state_variables, model.state_dict(), scalers, depth, "
                                 "min_filters, activation)).dump(path)")
            raise ValueError(f"{path} holds no {cls._WEIGHTS_FILENAME}")
        with open(os.path.join(path, cls._CONFIG_FILENAME)) as f:
            config = yaml.safe_load(f)
        with open(os.path.join(path, cls._SPEC_FILENAME)) as f:
            meta = yaml.safe_load(f)
        with np.load(os.path.join(path, cls._WEIGHTS_FILENAME), allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        return cls(config["state_variables"], GraphUNetSpec.from_arrays(meta, arrays))


# ---------------------------------------------------------------------------------------------
# offline training (PyTorch-ROCm)
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class GraphHyperparameters:
    """The part of fv3fit's ``GraphHyperparameters`` (graph/train.py:30-59) with ``GraphUNetConfig`` (unet.py:9-31) and
    ``AutoregressiveTrainingConfig`` (training_loop.py:75-92) that shapes and trains the network."""

    state_variables: List[str]
    depth: int = 1
    min_filters: int = 4
    activation: str = "relu"
    aggregator: str = "mean"
    pooling_size: int = 2
    pooling_stride: int = 2
    optimizer: str = "AdamW"
    optimizer_kwargs: Dict[str, Any] = dataclasses.field(default_factory=dict)
    n_epoch: int = 20
    samples_per_batch: int = 1
    multistep: int = 1
    normalization_fit_samples: int = 50_000
    seed: int = 0


def fit_scalers(samples: Mapping[str, np.ndarray]) -> Dict[str, Any]:
    """``get_standard_scaler_mapping`` (scaler.py:103-111): per variable the mean and ``std + 1e-12`` over the five sample dims
    ``[batch, time, tile, x, y]`` -- per level for a variable with ``z``, one number without -- as float64."""
    out = {}
    for name, a in samples.items():
        a = np.asarray(a)
        axes = tuple(range(5))
        out[name] = (np.mean(a, axis=axes).astype(np.float64), np.std(a, axis=axes).astype(np.float64) + 1e-12)
    return out


def _normalised_samples(batches, names, scalers) -> torch.Tensor:
    """``[sample, time, tile, x, y, F]`` float32: every batch scaled in its own precision, the variables joined along ``z``."""
    out = []
    for batch in batches:
        cols = []
        for name in names:
            a = np.asarray(batch[name].cpu() if isinstance(batch[name], torch.Tensor) else batch[name])
            mean, std = scalers[name]
            a = (a - mean) / std
            cols.append(a if a.ndim == 6 else a[..., None])
        out.append(torch.from_numpy(np.concatenate(cols, axis=-1).astype(np.float32)))
    return torch.cat(out, dim=0)


def _multistep_loss(model, batch, multistep):
    """training_loop.py:136-148: the mean over the steps of the MSE of the state rolled out from the batch's first time."""
    total, state = 0.0, batch[:, 0]
    for step in range(multistep):
        state = model(state)
        total = total + torch.nn.functional.mse_loss(state, batch[:, step + 1])
    return total / multistep


_HIP_OPTIMIZER_KWARGS = ("lr", "betas", "eps", "weight_decay")


def train_graph_model(hyperparameters: GraphHyperparameters, train_batches: Sequence[Mapping[str, Any]],
                      validation_batches: Optional[Sequence[Mapping[str, Any]]] = None,
                      device: Optional[str] = None, backend: Optional[str] = None) -> HipGraphAutoregressor:
    """Fit the scalers on up to ``normalization_fit_samples`` samples, train the network on the normalised state with the
    multistep MSE and, where validation data is given, keep the weights of the epoch that validated best (train.py:65-119,
    training_loop.py:151-198).  Batches map every state variable to ``[batch, time, tile, x, y(, z)]``.

    ``backend``: ``"torch"`` (the default, also for ``None``) steps ``GraphUNetTwin`` through autograd and ``torch.optim``;
    ``"hip"`` steps ``graph_train.GraphTrainer`` (this project's kernels; ``optimizer`` ``"AdamW"`` or
    ``"Adam"`` with ``lr``, ``betas``, ``eps``, ``weight_decay``).  The scalers, the initialisation of the network on the host
    under ``torch.manual_seed(seed)``, the ``torch.randperm`` sequence and the keep-the-best rule are one piece of code, so both
    backends start from bitwise-equal parameters and see the same batches."""
    hp = hyperparameters
    backend = check_backend(backend)
    check_architecture(hp.aggregator, hp.pooling_size, hp.pooling_stride, hp.activation)
    if backend == "hip":
        if hp.optimizer not in ("AdamW", "Adam"):
            raise NotImplementedError(f"optimizer {hp.optimizer!r} is not built for backend 'hip'; supported: 'AdamW', 'Adam'")
        for key in hp.optimizer_kwargs:
            if key not in _HIP_OPTIMIZER_KWARGS:
                raise NotImplementedError(f"optimizer argument {key!r} is not built for backend 'hip'; supported: {_HIP_OPTIMIZER_KWARGS}")
    torch.manual_seed(hp.seed)
    backend, dev = resolve_backend(backend, device)
    names = list(hp.state_variables)
    to_np = lambda a: np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)
    head = {name: np.concatenate([to_np(b[name]) for b in train_batches], axis=0)[:hp.normalization_fit_samples] for name in names}
    scalers = fit_scalers(head)
    train = _normalised_samples(train_batches, names, scalers).to(dev)
    valid = None if validation_batches is None else _normalised_samples(validation_batches, names, scalers).to(dev)
    check_cube_shape(tuple(train.shape[2:]), "training data")
    if train.shape[1] < hp.multistep + 1:
        raise ValueError(f"samples of {train.shape[1]} times do not hold {hp.multistep} steps")
    model = GraphUNetTwin(int(train.shape[-1]), hp.depth, hp.min_filters, hp.activation)   # initialised on the host
    to_spec = lambda state: graph_unet_spec_from_state_dict(names, state, scalers, hp.depth, hp.min_filters, hp.activation)
    if backend == "hip":
        from ..graph_train import GraphTrainer

        trainer = GraphTrainer(to_spec(model.state_dict()), train, multistep=hp.multistep, max_batch=hp.samples_per_batch, device=dev,
                               optimizer=hp.optimizer, **hp.optimizer_kwargs)
        take_step = trainer.step
        validate = lambda: trainer.validation_loss(valid)
        snapshot = lambda: trainer.params.clone()
        restore = lambda best: trainer.params.copy_(best)
    else:
        model = model.to(dev)
        opt = getattr(torch.optim, hp.optimizer)(model.parameters(), **hp.optimizer_kwargs)

        def take_step(idx):
            opt.zero_grad()
            loss = _multistep_loss(model, train[idx], hp.multistep)
            loss.backward()
            opt.step()

        def validate():
            model.eval()
            with torch.no_grad():
                return float(_multistep_loss(model, valid, hp.multistep))

        snapshot = lambda: copy.deepcopy(model.state_dict())
        restore = model.load_state_dict
    best, best_loss = None, float("inf")
    for batches in epoch_minibatches(train.shape[0], hp.samples_per_batch, hp.n_epoch, hp.seed, dev):
        model.train()
        for idx in batches:
            take_step(idx)
        if valid is not None:
            val_loss = validate()
            if val_loss < best_loss:
                best_loss, best = val_loss, snapshot()
    if best is not None:
        restore(best)
    spec = trainer.spec() if backend == "hip" else to_spec(model.state_dict())
    return HipGraphAutoregressor(names, spec)
