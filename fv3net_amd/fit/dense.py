"""The dense column predictor: ``fv3fit``'s ``PureKerasModel`` + ``DenseModel`` training,
re-done for MI355X.

* ``HipDenseModel`` is the drop-in for ``fv3fit.keras.PureKerasModel``
  (external/fv3fit/fv3fit/keras/_models/shared/pure_keras.py:22-102): same constructor meaning,
  ``predict(X) -> Dataset``, ``dump`` / ``load`` through the ``name``-file registry.  The network
  runs in the fused HIP kernel; the dataset is consumed in its native ``[z, ...]`` layout, there
  is no stack / unstack copy (xr_prediction.py:111-139 does two).
* ``train_dense_model`` is the offline training step (dense.py:90-107,165-310): ``backend="torch"`` (the default) steps through
  PyTorch-ROCm, ``backend="hip"`` through ``fv3net_amd.train.DenseTrainer`` and the kernels of csrc/mlp_train.hip.
* ``HipDenseModel.input_sensitivity`` is the reference's Jacobian report (pure_keras.py:127-145) on the same kernels.
* The artifact is ``name`` ("hip-dense") + ``config.yaml`` (the reference's keys) +
  ``spec.yaml`` + ``weights.npz``; TensorFlow SavedModels cannot be read without TensorFlow.
"""
import dataclasses
import os
from typing import Dict, Hashable, Iterable, List, Mapping, Optional, Sequence

import numpy as np
import torch
import yaml

from ..cubedsphere._device import compute_device, download_all, on_device
from ..mlp import InputSpec, MlpModel, MlpSpec, OutputSpec
from ..xr_compat import DataArray, Dataset, from_compat, to_compat
from . import io
from .input_sensitivity import InputSensitivity, nondimensionalize_jacobians
from .predictor import Predictor
from .stacking import column_sources, match_prediction_to_input_coords
from .training import epoch_minibatches, linear_arrays, resolve_backend


CONFIG_FILENAME = "config.yaml"
SPEC_FILENAME = "spec.yaml"
WEIGHTS_FILENAME = "weights.npz"


def write_artifact(path: str, spec: MlpSpec, config: Mapping) -> None:
    """The files a column predictor's directory holds beside ``name``: ``config.yaml``, ``spec.yaml``, ``weights.npz``."""
    os.makedirs(path, exist_ok=True)
    meta, arrays = spec.to_arrays()
    np.savez(os.path.join(path, WEIGHTS_FILENAME), **arrays)
    with open(os.path.join(path, SPEC_FILENAME), "w") as f:
        yaml.safe_dump(meta, f)
    with open(os.path.join(path, CONFIG_FILENAME), "w") as f:
        yaml.safe_dump(dict(config), f)


def read_artifact(path: str):
    """(config, spec) of a directory written by ``write_artifact``."""
    with open(os.path.join(path, CONFIG_FILENAME)) as f:
        config = yaml.safe_load(f)
    with open(os.path.join(path, SPEC_FILENAME)) as f:
        meta = yaml.safe_load(f)
    with np.load(os.path.join(path, WEIGHTS_FILENAME), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    return config, MlpSpec.from_arrays(meta, arrays)


@io.register("hip-dense")
class HipDenseModel(Predictor):
    """Column MLP predictor running on the MI355X fused kernel."""

    _CONFIG_FILENAME = CONFIG_FILENAME
    _SPEC_FILENAME = SPEC_FILENAME
    _WEIGHTS_FILENAME = WEIGHTS_FILENAME

    def __init__(self, input_variables: Iterable[Hashable], output_variables: Iterable[Hashable], model: MlpSpec,
                 unstacked_dims: Sequence[str] = ("z",), n_halo: int = 0):
        super().__init__(list(input_variables), list(output_variables))
        if n_halo != 0:
            raise ValueError("dense column models take no halo (dense.py:233); n_halo must be 0")
        self.spec = model
        self._n_halo = n_halo
        self._unstacked_dims = list(unstacked_dims) if unstacked_dims is not None else []
        names = model.output_names
        missing = [v for v in self.output_variables if v not in names]
        if missing:
            raise ValueError(f"output variables {missing} are not produced by the network ({names})")
        self._model: Optional[MlpModel] = None  # created on first predict (needs the GPU)
        self._trainer = None                    # created on first input_sensitivity

    @property
    def model(self) -> MlpModel:
        if self._model is None:
            self._model = MlpModel(self.spec, device=compute_device())
        return self._model

    # -- prediction -------------------------------------------------------------------------
    def predict(self, X):
        """Predict an output dataset from an input dataset.  Does not mutate ``X``."""
        x = to_compat(X)
        sources, sample_dims, sizes, zname, host_input = column_sources(x, self.spec.sources, self._unstacked_dims)
        outs = self.model.predict(sources, layout="feature_sample")

        result = Dataset()
        nfeat_out = {o.name: o.nfeat for o in self.spec.outputs}
        for r in self.spec.residuals:
            nfeat_out[r.name] = nfeat_out[r.output]
        shaped, dims_of = {}, {}
        for name in self.output_variables:
            t = outs[name]
            if nfeat_out[name] == 1:
                shaped[name], dims_of[name] = t.reshape([sizes[d] for d in sample_dims]), tuple(sample_dims)
            else:
                shaped[name] = t.reshape([nfeat_out[name]] + [sizes[d] for d in sample_dims])
                dims_of[name] = (zname,) + tuple(sample_dims)
        if not (isinstance(host_input, torch.Tensor) and host_input.is_cuda):
            shaped = download_all(shaped)  # host data in -> host data out, one copy for all outputs
        for name in self.output_variables:
            result[name] = DataArray(shaped[name], dims=dims_of[name])
        return from_compat(match_prediction_to_input_coords(x, result), X)

    # -- sensitivity ------------------------------------------------------------------------
    def jacobians(self, profiles: Mapping[str, np.ndarray]):
        """``{output: {input: d output / d input}}`` of the predict graph at one profile per input (see
        ``fv3net_amd.train.predict_graph_jacobians``), for the model's output variables."""
        from ..train import DenseTrainer, predict_graph_jacobians

        if self._trainer is None:
            self._trainer = DenseTrainer.from_spec(self.spec, compute_device())
        jac = predict_graph_jacobians(self.spec, profiles, trainer=self._trainer)
        return {name: jac[name] for name in self.output_variables if name in jac}

    def input_sensitivity(self, stacked_sample) -> InputSensitivity:
        """The Jacobian of every output with respect to every input at the sample-mean profile, times ``std(input)`` along the
        columns and over ``std(output)`` along the rows (pure_keras.py:127-145).  ``stacked_sample`` holds the inputs and the
        outputs as ``[sample, feature]`` (``[sample]``: one feature); an output missing from it raises ``KeyError``."""
        sample = to_compat(stacked_sample)
        data = {}
        for var in list(self.input_variables) + list(self.output_variables):
            values = sample[var].values
            data[var] = values.reshape(-1, 1) if values.ndim == 1 else values
        jac = self.jacobians({name: data[name].mean(axis=0) for name in self.input_variables})
        std = {name: np.std(values, axis=0) for name, values in data.items()}
        return InputSensitivity(jacobians=nondimensionalize_jacobians(jac, std))

    # -- serialisation ----------------------------------------------------------------------
    def dump(self, path: str) -> None:
        write_artifact(path, self.spec, {"input_variables": list(self.input_variables), "output_variables": list(self.output_variables),
                                         "unstacked_dims": list(self._unstacked_dims), "n_halo": self._n_halo})

    @classmethod
    def load(cls, path: str) -> "HipDenseModel":
        config, spec = read_artifact(path)
        return cls(config["input_variables"], config["output_variables"], spec,
                   unstacked_dims=config.get("unstacked_dims", None), n_halo=config.get("n_halo", 0))


# ---------------------------------------------------------------------------------------------
# building a spec from arrays (an exporter run where TensorFlow exists produces exactly these)
# ---------------------------------------------------------------------------------------------
def spec_from_arrays(
    input_variables: Sequence[str],
    input_means: Sequence[np.ndarray],
    input_stds: Sequence[np.ndarray],
    hidden_kernels: Sequence[np.ndarray],
    hidden_biases: Sequence[np.ndarray],
    output_variables: Sequence[str],
    output_kernels: Sequence[np.ndarray],
    output_biases: Sequence[np.ndarray],
    output_means: Sequence[np.ndarray],
    output_stds: Sequence[np.ndarray],
    clip: Optional[Mapping[str, slice]] = None,
    limits: Optional[Mapping[str, Sequence[Optional[float]]]] = None,
    epsilon: float = 1e-7,
) -> MlpSpec:
    """Assemble the predict graph of dense.py:239-310 from its weights.  ``input_stds`` are the
    fitted standard deviations; the forward scale is ``std + epsilon`` in float32
    (normalization.py:39-46).  ``clip[name]`` keeps a slice of an input's levels (clip.py:48-62)
    and zero-masks the complement of an output's (clip.py:33-46); means/stds of clipped inputs
    are those of the kept levels."""
    clip = dict(clip or {})
    limits = dict(limits or {})
    inputs = []
    for name, mean, std in zip(input_variables, input_means, input_stds):
        mean, std = np.atleast_1d(np.asarray(mean, np.float32)), np.atleast_1d(np.asarray(std, np.float32))
        start = 0
        if name in clip:
            start = clip[name].start or 0
        inputs.append(InputSpec(source=name, nfeat=int(mean.shape[0]), start=int(start), center=mean,
                                scale=std + np.float32(epsilon)))
    outputs = []
    for name, kern, mean, std in zip(output_variables, output_kernels, output_means, output_stds):
        nf = int(np.asarray(kern).shape[1])
        mask = None
        if name in clip:
            s = clip[name]
            mask = np.zeros(nf, np.float32)
            mask[(s.start or 0):(s.stop if s.stop is not None else nf)] = 1.0
        lo, hi = limits.get(name, (None, None))
        outputs.append(OutputSpec(name=name, nfeat=nf, scale=np.broadcast_to(np.asarray(std, np.float32), (nf,)).copy(),
                                  center=np.broadcast_to(np.asarray(mean, np.float32), (nf,)).copy(), min=lo, max=hi,
                                  mask=mask))
    return MlpSpec(
        inputs=inputs,
        hidden_kernels=[np.asarray(k, np.float32) for k in hidden_kernels],
        hidden_biases=[np.asarray(b, np.float32) for b in hidden_biases],
        outputs=outputs,
        out_kernel=np.concatenate([np.asarray(k, np.float32) for k in output_kernels], axis=1),
        out_bias=np.concatenate([np.asarray(b, np.float32) for b in output_biases]),
    )


# ---------------------------------------------------------------------------------------------
# offline training (PyTorch-ROCm, or the project's own kernels with backend="hip")
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class DenseHyperparameters:
    """The subset of fv3fit's ``DenseHyperparameters`` (dense.py:39-87) that shapes the network."""

    input_variables: List[str]
    output_variables: List[str]
    width: int = 8            # DenseNetworkConfig.width   (dense_network.py:31)
    depth: int = 3            # DenseNetworkConfig.depth: hidden layers + 1 (dense_network.py:32)
    epochs: int = 3           # TrainingLoopConfig.epochs
    batch_size: int = 512
    learning_rate: float = 1e-3
    normalization_fit_samples: int = 500_000   # dense.py:211-217
    clip: Dict[str, slice] = dataclasses.field(default_factory=dict)
    limits: Dict[str, Sequence[Optional[float]]] = dataclasses.field(default_factory=dict)
    unstacked_dims: Sequence[str] = ("z",)
    seed: int = 0


def _stack_for_training(batches: Sequence[Dataset], names: Sequence[str], unstacked_dims) -> List[np.ndarray]:
    cols: List[List[np.ndarray]] = [[] for _ in names]
    for ds in batches:
        ds = to_compat(ds)
        for i, name in enumerate(names):
            da = ds[name]
            zs = [d for d in da.dims if d in unstacked_dims]
            rest = [d for d in da.dims if d not in unstacked_dims]
            a = da.transpose(*rest, *zs).values
            cols[i].append(a.reshape(-1, a.shape[-1]) if zs else a.reshape(-1, 1))  # ensure_nd (dense.py:146)
    return [np.concatenate(c, axis=0).astype(np.float32) for c in cols]


@dataclasses.dataclass
class _DenseTraining:
    """What both backends of ``train_dense_model`` start from: the fitted normalisation, the normalised inputs, the targets and
    the freshly initialised layers (created on the host, so that the start does not depend on the device)."""

    xin: np.ndarray                 # [n, K] normalised, clipped inputs
    y: List[np.ndarray]             # the outputs as stacked, [n, nfeat] each
    yc: List[np.ndarray]            # ... with the output clip applied
    x_mean: List[np.ndarray]
    x_std: List[np.ndarray]
    y_mean: List[np.ndarray]
    y_std: List[np.ndarray]
    yc_std: List[np.ndarray]
    trunk: torch.nn.Sequential
    heads: torch.nn.ModuleList


def _prepare_dense_training(hp: DenseHyperparameters, train_batches: Sequence[Dataset]) -> _DenseTraining:
    torch.manual_seed(hp.seed)
    X = _stack_for_training(train_batches, hp.input_variables, hp.unstacked_dims)
    y = _stack_for_training(train_batches, hp.output_variables, hp.unstacked_dims)
    nfit = hp.normalization_fit_samples

    def clipped(arr, name):
        return arr[..., hp.clip[name]] if name in hp.clip else arr

    Xc = [clipped(a, n) for a, n in zip(X, hp.input_variables)]
    yc = [clipped(a, n) for a, n in zip(y, hp.output_variables)]
    x_mean = [a[:nfit].mean(axis=0).astype(np.float32) for a in Xc]
    x_std = [a[:nfit].std(axis=0).astype(np.float32) for a in Xc]
    y_mean = [a[:nfit].mean(axis=0).astype(np.float32) for a in y]
    y_std = [a[:nfit].std(axis=0).astype(np.float32) for a in y]
    yc_std = [np.std(a[:nfit], axis=0, dtype=np.float32) for a in yc]

    eps = np.float32(1e-7)
    xin = np.concatenate([(a - m) / (s + eps) for a, m, s in zip(Xc, x_mean, x_std)], axis=1)
    layers: List[torch.nn.Module] = []
    fan = xin.shape[1]
    for _ in range(hp.depth - 1):
        lin = torch.nn.Linear(fan, hp.width)
        torch.nn.init.xavier_uniform_(lin.weight)  # Keras Dense default: glorot_uniform, zero bias
        torch.nn.init.zeros_(lin.bias)
        layers += [lin, torch.nn.ReLU()]
        fan = hp.width
    trunk = torch.nn.Sequential(*layers)
    heads = torch.nn.ModuleList()
    for a in y:
        lin = torch.nn.Linear(fan, a.shape[1])
        torch.nn.init.xavier_uniform_(lin.weight)
        torch.nn.init.zeros_(lin.bias)
        heads.append(lin)
    return _DenseTraining(xin=xin, y=y, yc=yc, x_mean=x_mean, x_std=x_std, y_mean=y_mean, y_std=y_std, yc_std=yc_std, trunk=trunk,
                          heads=heads)


def _train_torch(hp: DenseHyperparameters, prep: _DenseTraining, dev: torch.device):
    """Adam on the std-scaled MSE through ``torch.nn.Linear`` and autograd; returns the four weight lists."""
    xin = torch.from_numpy(prep.xin).to(dev)
    trunk, heads = prep.trunk.to(dev), prep.heads.to(dev)
    targets = [torch.from_numpy(a).to(dev) for a in prep.yc]
    t_mean = [torch.from_numpy(m).to(dev) for m in prep.y_mean]
    t_std = [torch.from_numpy(s).to(dev) for s in prep.y_std]
    t_cstd = [torch.from_numpy(np.maximum(s, 1e-12)).to(dev) for s in prep.yc_std]
    opt = torch.optim.Adam(list(trunk.parameters()) + list(heads.parameters()), lr=hp.learning_rate)
    for batches in epoch_minibatches(xin.shape[0], hp.batch_size, hp.epochs, hp.seed, dev):
        for idx in batches:
            hidden = trunk(xin[idx])
            loss = 0.0
            for j, name in enumerate(hp.output_variables):
                pred = heads[j](hidden) * t_std[j] + t_mean[j]
                lo, hi = hp.limits.get(name, (None, None))
                if lo is not None or hi is not None:
                    pred = torch.clamp(pred, min=lo, max=hi)
                if name in hp.clip:
                    pred = pred[..., hp.clip[name]]
                loss = loss + torch.mean(((pred - targets[j][idx]) / t_cstd[j]) ** 2)
            opt.zero_grad()
            loss.backward()
            opt.step()
    return (*linear_arrays([m for m in trunk if isinstance(m, torch.nn.Linear)]), *linear_arrays(heads))


def dense_mse_loss(hp: DenseHyperparameters, prep: _DenseTraining):
    """The loss of ``_train_torch`` as the per-feature arrays the device step takes (``fv3net_amd.train.MseLoss``)."""
    from ..train import MseLoss

    inv, lo_all, hi_all, keep, kept = [], [], [], [], []
    for name, a, cstd in zip(hp.output_variables, prep.y, prep.yc_std):
        nf = a.shape[1]
        mask = np.zeros(nf, np.float32)
        mask[hp.clip[name] if name in hp.clip else slice(None)] = 1.0
        full = np.zeros(nf, np.float64)
        full[mask != 0] = 1.0 / np.maximum(cstd, 1e-12).astype(np.float64) ** 2
        lo, hi = hp.limits.get(name, (None, None))
        inv.append(full.astype(np.float32))
        lo_all.append(np.full(nf, -np.inf if lo is None else lo, np.float32))
        hi_all.append(np.full(nf, np.inf if hi is None else hi, np.float32))
        keep.append(mask)
        kept.append(np.full(nf, mask.sum(), np.float64))
    return MseLoss(scale=np.concatenate(prep.y_std), center=np.concatenate(prep.y_mean), inv_cstd2=np.concatenate(inv),
                   lo=np.concatenate(lo_all), hi=np.concatenate(hi_all), keep=np.concatenate(keep), kept=np.concatenate(kept))


def dense_trainer(hp: DenseHyperparameters, prep: _DenseTraining, dev: torch.device):
    """The device training state of ``backend="hip"``: the layers of ``prep``, the resident inputs and targets, the loss."""
    from ..train import DenseTrainer

    kernels, biases = linear_arrays([m for m in prep.trunk if isinstance(m, torch.nn.Linear)])
    head_kernels, head_biases = linear_arrays(prep.heads)
    kernels.append(np.concatenate(head_kernels, axis=1))
    biases.append(np.concatenate(head_biases))
    return DenseTrainer(kernels, biases, device=dev, xin=prep.xin, targets=np.concatenate(prep.y, axis=1), loss=dense_mse_loss(hp, prep),
                        max_batch=min(hp.batch_size, prep.xin.shape[0]), learning_rate=hp.learning_rate)


def _train_hip(hp: DenseHyperparameters, prep: _DenseTraining, dev: torch.device):
    """The same minibatches in the same order through ``fv3net_amd.train.DenseTrainer`` (csrc/mlp_train.hip)."""
    trainer = dense_trainer(hp, prep, dev)
    for batches in epoch_minibatches(prep.xin.shape[0], hp.batch_size, hp.epochs, hp.seed, dev):
        for idx in batches:
            trainer.step(idx)
    return trainer.parameters([a.shape[1] for a in prep.y])


def train_dense_model(hyperparameters: DenseHyperparameters, train_batches: Sequence[Dataset],
                      device: Optional[str] = None, backend: Optional[str] = None) -> HipDenseModel:
    """Fit normalisation on up to ``normalization_fit_samples`` samples, train
    ``Dense(width, relu) x (depth-1) -> Dense per output`` with Adam on the std-scaled MSE of the
    (clipped) outputs, and return the predictor (dense.py:165-310, training_loop.py:86-138).

    ``backend``: ``None`` / ``"torch"`` steps through ``torch.nn.Linear``, autograd and ``torch.optim.Adam``; ``"hip"`` through
    the project's own kernels (needs a GPU).  Normalisation, initialisation and the minibatch sequence are shared: both start
    from bitwise-equal parameters and see the same rows in the same order."""
    hp = hyperparameters
    backend, dev = resolve_backend(backend, device)
    prep = _prepare_dense_training(hp, train_batches)
    weights = (_train_hip if backend == "hip" else _train_torch)(hp, prep, dev)
    spec = spec_from_arrays(hp.input_variables, prep.x_mean, prep.x_std, weights[0], weights[1], hp.output_variables, weights[2],
                            weights[3], prep.y_mean, prep.y_std, clip=hp.clip, limits=hp.limits)
    return HipDenseModel(hp.input_variables, hp.output_variables, spec, unstacked_dims=hp.unstacked_dims)
