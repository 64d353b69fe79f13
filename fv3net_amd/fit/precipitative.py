"""The precipitative column predictor: ``fv3fit``'s ``"precipitative"`` training function
(external/fv3fit/fv3fit/keras/_models/precipitative.py), re-done for MI355X.

The graph (precipitative.py:181-279) is the dense column network with a closed column water budget.  A shared trunk feeds
three live heads -- ``dQ1`` and ``dQ2`` residuals and a column-precipitation moistening profile ``cp`` (its layer is named
``q_tendency_due_to_precip`` and it is denormalised with dQ2's mean and std, :231-238) -- and then

    total_precipitation_rate = physics_precip + float32(-1 / g) * sum_k(cp[k] * delp[k])        (:35-53, :246-253)
    dQ1 = t_res + float32(-LV / CPD) * cp,   dQ2 = q_res + cp      (couple_precip_to_dQ1_dQ2, :239-244)

with ``delp`` the raw, unclipped input.  The fourth head the reference builds (one feature, for total_precipitation_rate)
never reaches an output (``unpacked_output[2]`` is unused) and is not stored.

* ``HipPrecipitativeModel``: the network in the fused HIP kernel (``MlpModel``), then ONE ``fv3hip_precip_closure`` launch
  on the same stream, in place over the residual heads.  The sum's order is fixed (float32, ascending levels, products
  rounded), so a numpy float32 loop reproduces it bit for bit.
* ``precipitative_spec_from_arrays``: the exporter's entry.
* ``train_precipitative_model``: the offline step, through PyTorch or (``backend="hip"``) through the project's own kernels with
  the loss behind the closure in one launch (``fv3hip_train_precip_loss_grad``).
"""
import dataclasses
from typing import Dict, Hashable, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops
from ..cubedsphere._device import compute_device, download_all
from ..mlp import MlpModel, MlpSpec
from ..xr_compat import DataArray, Dataset, from_compat, to_compat
from . import io
from .dense import _stack_for_training, read_artifact, spec_from_arrays, write_artifact
from .input_sensitivity import InputSensitivity, nondimensionalize_jacobians
from .predictor import Predictor
from .stacking import column_sources, match_prediction_to_input_coords
from .training import epoch_minibatches, linear_arrays, resolve_backend

LV = 2.5e6          # latent heat of evaporation [J/kg]            (precipitative.py:21)
CPD = 1004.6        # specific heat of dry air at constant pressure  (:23)
GRAVITY = 9.80665   # (:24)

DELP_NAME = "pressure_thickness_of_atmospheric_layer"
T_NAME = "air_temperature"
Q_NAME = "specific_humidity"
PHYS_PRECIP_NAME = "physics_precip"
PRECIP_NAME = "total_precipitation_rate"
T_TENDENCY_NAME = "dQ1"
Q_TENDENCY_NAME = "dQ2"
COLUMN_PRECIP_NAME = "q_tendency_due_to_precip"   # the reference's own layer name (:235)

INPUT_VARIABLES = (T_NAME, Q_NAME, DELP_NAME, PHYS_PRECIP_NAME)          # (:150-155)
OUTPUT_VARIABLES = (T_TENDENCY_NAME, Q_TENDENCY_NAME, PRECIP_NAME)       # (:157-159, asserted at :258-262)
HEAD_NAMES = (T_TENDENCY_NAME, Q_TENDENCY_NAME, COLUMN_PRECIP_NAME)


@io.register("hip-precipitative")
class HipPrecipitativeModel(Predictor):
    """Column MLP with the precipitative water-budget closure: two launches per ``predict``."""

    def __init__(self, input_variables: Iterable[Hashable], output_variables: Iterable[Hashable], model: MlpSpec,
                 couple_precip_to_dQ1_dQ2: bool = True, unstacked_dims: Sequence[str] = ("z",), n_halo: int = 0):
        super().__init__(list(input_variables), list(output_variables))
        if n_halo != 0:
            raise ValueError("precipitative column models take no halo; n_halo must be 0")
        if list(self.output_variables) != list(OUTPUT_VARIABLES):
            raise ValueError(f"output variables must be {list(OUTPUT_VARIABLES)} in that order (precipitative.py:258-262), "
                             f"got {list(self.output_variables)}")
        heads = [o.name for o in model.outputs]
        if heads != list(HEAD_NAMES) or model.residuals or model.hidden_output:
            raise ValueError(f"the network must have exactly the heads {list(HEAD_NAMES)}, got {model.output_names}")
        sizes = {o.nfeat for o in model.outputs}
        if len(sizes) != 1:
            raise ValueError(f"the three heads must have one size (the number of levels), got {[o.nfeat for o in model.outputs]}")
        missing = [v for v in (DELP_NAME, PHYS_PRECIP_NAME) if v not in self.input_variables or v not in model.sources]
        if missing:
            raise ValueError(f"the closure needs {missing} among the inputs")
        self.spec = model
        self.couple_precip_to_dQ1_dQ2 = bool(couple_precip_to_dQ1_dQ2)
        self._nz = sizes.pop()
        self._n_halo = n_halo
        self._unstacked_dims = list(unstacked_dims) if unstacked_dims is not None else []
        self._model: Optional[MlpModel] = None  # created on first predict (needs the GPU)
        self._trainer = None                    # created on first input_sensitivity

    @property
    def model(self) -> MlpModel:
        if self._model is None:
            self._model = MlpModel(self.spec, device=compute_device())
        return self._model

    # -- prediction -------------------------------------------------------------------------
    def predict(self, X):
        """Predict ``dQ1``, ``dQ2`` ``[z, ...]`` and ``total_precipitation_rate`` ``[...]`` (float32).  Does not mutate ``X``.
        On device-resident input: two launches on the current stream, nothing read back, no allocation outside torch's."""
        x = to_compat(X)
        sources, sample_dims, sizes, zname, host_input = column_sources(x, self.spec.sources, self._unstacked_dims)
        delp, physics_precip = sources[DELP_NAME], sources[PHYS_PRECIP_NAME]  # their own views: dtype and strides as they lie
        if int(delp.shape[0]) != self._nz:
            raise ValueError(f"{DELP_NAME} has {int(delp.shape[0])} levels, the model's heads have {self._nz}")
        if int(physics_precip.shape[0]) != 1:
            raise ValueError(f"{PHYS_PRECIP_NAME} must have no vertical dim")
        outs = self.model.predict(sources, layout="feature_sample")
        dq1, dq2, precip = ops.precip_closure(outs[T_TENDENCY_NAME], outs[Q_TENDENCY_NAME], outs[COLUMN_PRECIP_NAME], delp,
                                              physics_precip, couple=self.couple_precip_to_dQ1_dQ2, in_place=True)
        shape = [sizes[d] for d in sample_dims]
        shaped = {T_TENDENCY_NAME: dq1.reshape([self._nz] + shape), Q_TENDENCY_NAME: dq2.reshape([self._nz] + shape),
                  PRECIP_NAME: precip.reshape(shape)}
        dims_of = {T_TENDENCY_NAME: (zname,) + tuple(sample_dims), Q_TENDENCY_NAME: (zname,) + tuple(sample_dims),
                   PRECIP_NAME: tuple(sample_dims)}
        if not (isinstance(host_input, torch.Tensor) and host_input.is_cuda):
            shaped = download_all(shaped)  # host data in -> host data out, one copy for all outputs
        result = Dataset()
        for name in self.output_variables:
            result[name] = DataArray(shaped[name], dims=dims_of[name])
        return from_compat(match_prediction_to_input_coords(x, result), X)

    # -- sensitivity ------------------------------------------------------------------------
    def _head_jacobians(self, profiles: Mapping[str, np.ndarray]):
        """The device part: the three heads' Jacobians and the column-precipitation head's value at the profiles."""
        from ..train import DenseTrainer, predict_graph_jacobians

        if self._trainer is None:
            self._trainer = DenseTrainer.from_spec(self.spec, compute_device())
        values: Dict[str, np.ndarray] = {}
        jac = predict_graph_jacobians(self.spec, profiles, trainer=self._trainer, values=values)
        return jac, values[COLUMN_PRECIP_NAME]

    def jacobians(self, profiles: Mapping[str, np.ndarray]):
        """``{output: {input: d output / d input}}`` of the predict graph at one profile per input: the heads' Jacobians from the
        device (``fv3net_amd.train.predict_graph_jacobians``), the closure composed on the host (``compose_closure_jacobians``)."""
        head_jac, cp = self._head_jacobians(profiles)
        return compose_closure_jacobians(head_jac, cp, profiles[DELP_NAME], self.couple_precip_to_dQ1_dQ2)

    def input_sensitivity(self, stacked_sample) -> InputSensitivity:
        """The Jacobian of every output with respect to every input at the sample-mean profile, times ``std(input)`` along the
        columns and over ``std(output)`` along the rows (pure_keras.py:127-145), as ``HipDenseModel.input_sensitivity``."""
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
                                         "unstacked_dims": list(self._unstacked_dims), "n_halo": self._n_halo,
                                         "couple_precip_to_dQ1_dQ2": self.couple_precip_to_dQ1_dQ2})

    @classmethod
    def load(cls, path: str) -> "HipPrecipitativeModel":
        config, spec = read_artifact(path)
        return cls(config["input_variables"], config["output_variables"], spec,
                   couple_precip_to_dQ1_dQ2=config["couple_precip_to_dQ1_dQ2"],
                   unstacked_dims=config.get("unstacked_dims", None), n_halo=config.get("n_halo", 0))


def compose_closure_jacobians(head_jacobians: Mapping[str, Mapping[str, np.ndarray]], col_precip: np.ndarray, delp: np.ndarray,
                              couple: bool) -> Dict[str, Dict[str, np.ndarray]]:
    """The closure applied to the Jacobians of the three heads (``{head: {source: [nz, len(source)]}}``), in float64:

        J[dQ1] = J_t + c_heat J_cp,  J[dQ2] = J_q + J_cp       (under ``couple``; else the heads' own)
        J[total_precipitation_rate][src] = c_g sum_k delp[k] J_cp[k, :]   (+ c_g cp[k] in column k of the thickness, + 1 for physics_precip)

    with the float32 constants of the graph, ``delp`` the profile cast to float32 as ``predict`` casts it and ``col_precip`` the
    column-precipitation head's value at the profile."""
    c_heat, c_g = np.float64(np.float32(-LV / CPD)), np.float64(np.float32(-1.0 / GRAVITY))
    d = np.atleast_1d(np.asarray(delp)).astype(np.float32).astype(np.float64)
    cp = np.asarray(col_precip, np.float64)
    j_cp = {src: np.asarray(j, np.float64) for src, j in head_jacobians[COLUMN_PRECIP_NAME].items()}
    out: Dict[str, Dict[str, np.ndarray]] = {T_TENDENCY_NAME: {}, Q_TENDENCY_NAME: {}, PRECIP_NAME: {}}
    for src, jc in j_cp.items():
        j_t = np.asarray(head_jacobians[T_TENDENCY_NAME][src], np.float64)
        j_q = np.asarray(head_jacobians[Q_TENDENCY_NAME][src], np.float64)
        out[T_TENDENCY_NAME][src] = j_t + c_heat * jc if couple else j_t.copy()
        out[Q_TENDENCY_NAME][src] = j_q + jc if couple else j_q.copy()
        row = c_g * (d[None, :] @ jc)
        if src == DELP_NAME:
            row = row + c_g * cp[None, :]
        elif src == PHYS_PRECIP_NAME:
            row = row + 1.0
        out[PRECIP_NAME][src] = row
    return out


# ---------------------------------------------------------------------------------------------
# building a spec from arrays (an exporter run where TensorFlow exists produces exactly these)
# ---------------------------------------------------------------------------------------------
def precipitative_spec_from_arrays(
    input_variables: Sequence[str],
    input_means: Sequence[np.ndarray],
    input_stds: Sequence[np.ndarray],
    hidden_kernels: Sequence[np.ndarray],
    hidden_biases: Sequence[np.ndarray],
    head_kernels: Sequence[np.ndarray],
    head_biases: Sequence[np.ndarray],
    output_means: Sequence[np.ndarray],
    output_stds: Sequence[np.ndarray],
    clip: Optional[Mapping[str, slice]] = None,
    epsilon: float = 1e-7,
) -> MlpSpec:
    """Assemble the network of precipitative.py:192-238 from its weights.  ``head_kernels`` / ``head_biases``: the three
    live heads in the order dQ1, dQ2, column precipitation (the one-feature head is dead and is not taken).
    ``output_means`` / ``output_stds``: those of dQ1 and dQ2; the column-precipitation head is denormalised with dQ2's
    (:234-238).  ``clip`` is applied to the inputs only (:193-203): the predict graph masks no output level and has no
    output limits, so there are neither here."""
    if len(head_kernels) != 3 or len(head_biases) != 3:
        raise ValueError("three heads are expected: dQ1, dQ2 and the column precipitation")
    if len(output_means) != 2 or len(output_stds) != 2:
        raise ValueError("two output means / stds are expected: those of dQ1 and dQ2")
    input_clip = {name: s for name, s in dict(clip or {}).items() if name in input_variables}
    return spec_from_arrays(
        input_variables, input_means, input_stds, hidden_kernels, hidden_biases, list(HEAD_NAMES), head_kernels, head_biases,
        [output_means[0], output_means[1], output_means[1]], [output_stds[0], output_stds[1], output_stds[1]],
        clip=input_clip, epsilon=epsilon)


# ---------------------------------------------------------------------------------------------
# offline training (PyTorch-ROCm, or the project's own kernels with backend="hip")
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class PrecipitativeHyperparameters:
    """The fields of fv3fit's ``PrecipitativeHyperparameters`` (precipitative.py:117-134) that shape the graph."""

    additional_input_variables: List[str] = dataclasses.field(default_factory=list)
    width: int = 16           # DenseNetworkConfig(width=16)  (:121-123)
    depth: int = 3            # DenseNetworkConfig.depth: hidden layers + 1
    epochs: int = 3
    batch_size: int = 512
    learning_rate: float = 1e-3
    normalization_fit_samples: int = 500_000
    clip: Dict[str, slice] = dataclasses.field(default_factory=dict)   # clip_config: inputs only
    couple_precip_to_dQ1_dQ2: bool = True
    unstacked_dims: Sequence[str] = ("z",)
    seed: int = 0
    # residual_regularizer_config (:124-126) as (name, kwargs): "none", "l1", "l2" or "l1_l2" with Keras's kwargs
    residual_regularizer: Optional[Tuple[str, Mapping]] = None

    @property
    def input_variables(self) -> List[str]:
        return list(INPUT_VARIABLES) + list(self.additional_input_variables)

    @property
    def output_variables(self) -> List[str]:
        return list(OUTPUT_VARIABLES)


@dataclasses.dataclass
class _PrecipitativeTraining:
    """What both backends of ``train_precipitative_model`` start from: the fitted normalisation, the normalised inputs, the raw
    thickness, the targets and the freshly initialised layers (created on the host, so that the start does not depend on the
    device).  ``heads``: dQ1, dQ2, the dead one-feature head, the column precipitation -- the order the initialiser draws in."""

    xin: np.ndarray                 # [n, K] normalised, clipped inputs
    delp: np.ndarray                # [n, nz] unclipped (:246)
    physics_precip: np.ndarray      # [n]
    y: List[np.ndarray]             # dQ1 [n, nz], dQ2 [n, nz], total_precipitation_rate [n, 1]
    x_mean: List[np.ndarray]
    x_std: List[np.ndarray]
    y_mean: List[np.ndarray]
    y_std: List[np.ndarray]
    loss_std: List[np.ndarray]
    trunk: torch.nn.Sequential
    heads: torch.nn.ModuleList
    l1: float
    l2: float
    has_dead: bool


def _prepare_precipitative_training(hp: PrecipitativeHyperparameters, train_batches: Sequence[Dataset]) -> _PrecipitativeTraining:
    unknown = [name for name in hp.clip if name not in hp.input_variables]
    if unknown:
        raise ValueError(f"only inputs can be clipped (the predict graph masks no output level), got {unknown}")
    l1, l2, has_dead = regularizer_coefficients(hp.residual_regularizer)
    torch.manual_seed(hp.seed)
    names_in, names_out = hp.input_variables, hp.output_variables
    X = _stack_for_training(train_batches, names_in, hp.unstacked_dims)
    y = _stack_for_training(train_batches, names_out, hp.unstacked_dims)
    nfit = hp.normalization_fit_samples
    Xc = [a[..., hp.clip[n]] if n in hp.clip else a for a, n in zip(X, names_in)]
    x_mean = [a[:nfit].mean(axis=0).astype(np.float32) for a in Xc]
    x_std = [a[:nfit].std(axis=0).astype(np.float32) for a in Xc]
    y_mean = [a[:nfit].mean(axis=0).astype(np.float32) for a in y]
    y_std = [a[:nfit].std(axis=0).astype(np.float32) for a in y]
    loss_std = [np.std(a[:nfit], axis=0, dtype=np.float32) for a in y]

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
    for nfeat in [a.shape[1] for a in y] + [y[1].shape[1]]:   # dQ1, dQ2, the dead one-feature head, column precipitation
        lin = torch.nn.Linear(fan, nfeat)
        torch.nn.init.xavier_uniform_(lin.weight)
        torch.nn.init.zeros_(lin.bias)
        heads.append(lin)
    return _PrecipitativeTraining(xin=xin, delp=X[names_in.index(DELP_NAME)], physics_precip=X[names_in.index(PHYS_PRECIP_NAME)][:, 0],
                                  y=y, x_mean=x_mean, x_std=x_std, y_mean=y_mean, y_std=y_std, loss_std=loss_std, trunk=trunk,
                                  heads=heads, l1=l1, l2=l2, has_dead=has_dead)


def _train_torch(hp: PrecipitativeHyperparameters, prep: _PrecipitativeTraining, dev: torch.device):
    """Adam through ``torch.nn.Linear`` and autograd; returns the four weight lists (the heads: dQ1, dQ2, column precipitation)."""
    xin = torch.from_numpy(prep.xin).to(dev)
    delp = torch.from_numpy(prep.delp).to(dev)
    physics_precip = torch.from_numpy(prep.physics_precip).to(dev)
    trunk, heads = prep.trunk.to(dev), prep.heads.to(dev)
    targets = [torch.from_numpy(a).to(dev) for a in prep.y]
    targets[2] = targets[2][:, 0]
    t_mean = [torch.from_numpy(m).to(dev) for m in prep.y_mean]
    t_std = [torch.from_numpy(s).to(dev) for s in prep.y_std]
    t_lstd = [torch.from_numpy(np.maximum(s, 1e-12)).to(dev) for s in prep.loss_std]
    t_lstd[2] = t_lstd[2][0]
    c_heat, c_g = float(np.float32(-LV / CPD)), float(np.float32(-1.0 / GRAVITY))
    opt = torch.optim.Adam(list(trunk.parameters()) + list(heads.parameters()), lr=hp.learning_rate)
    for batches in epoch_minibatches(xin.shape[0], hp.batch_size, hp.epochs, hp.seed, dev):
        for idx in batches:
            hidden = trunk(xin[idx])
            raw = [heads[0](hidden), heads[1](hidden)]
            t_tend = raw[0] * t_std[0] + t_mean[0]
            q_tend = raw[1] * t_std[1] + t_mean[1]
            col_precip = heads[3](hidden) * t_std[1] + t_mean[1]      # dQ2's mean and std (:234-238)
            if hp.couple_precip_to_dQ1_dQ2:
                t_tend = t_tend + c_heat * col_precip
                q_tend = q_tend + col_precip
            precip = physics_precip[idx] + c_g * torch.sum(col_precip * delp[idx], dim=1)
            loss = 0.0
            for pred, j in ((t_tend, 0), (q_tend, 1), (precip, 2)):
                loss = loss + torch.mean(((pred - targets[j][idx]) / t_lstd[j]) ** 2)
            if prep.has_dead:   # activity_regularizer on the three dense_network_output_i heads: regularizer(output) / batch size
                for out in raw + [heads[2](hidden)]:
                    loss = loss + (prep.l1 * out.abs().sum() + prep.l2 * (out * out).sum()) / idx.shape[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
    return (*linear_arrays([m for m in trunk if isinstance(m, torch.nn.Linear)]), *linear_arrays([heads[0], heads[1], heads[3]]))


def precipitative_loss(hp: PrecipitativeHyperparameters, prep: _PrecipitativeTraining):
    """The loss of ``_train_torch`` as the arrays the device step takes (``fv3net_amd.train.PrecipLoss``)."""
    from ..train import PrecipLoss

    inv = [(1.0 / np.maximum(s, 1e-12).astype(np.float64) ** 2).astype(np.float32) for s in prep.loss_std]
    return PrecipLoss(scale1=prep.y_std[0], center1=prep.y_mean[0], scale2=prep.y_std[1], center2=prep.y_mean[1], inv_cstd2_1=inv[0],
                      inv_cstd2_2=inv[1], inv_cstd2_3=float(inv[2][0]), couple=bool(hp.couple_precip_to_dQ1_dQ2), has_dead=prep.has_dead,
                      l1=prep.l1, l2=prep.l2)


def precipitative_trainer(hp: PrecipitativeHyperparameters, prep: _PrecipitativeTraining, dev: torch.device):
    """The device training state of ``backend="hip"``: the layers of ``prep`` (the dead head only where it is trained), the
    resident inputs, thickness and targets, the loss."""
    from ..train import PrecipitativeTrainer

    kernels, biases = linear_arrays([m for m in prep.trunk if isinstance(m, torch.nn.Linear)])
    head_kernels, head_biases = linear_arrays([h for j, h in enumerate(prep.heads) if j != 2 or prep.has_dead])
    kernels.append(np.concatenate(head_kernels, axis=1))
    biases.append(np.concatenate(head_biases))
    return PrecipitativeTrainer(kernels, biases, device=dev, xin=prep.xin, delp=prep.delp, physics_precip=prep.physics_precip,
                                targets=prep.y, loss=precipitative_loss(hp, prep), max_batch=min(hp.batch_size, prep.xin.shape[0]),
                                learning_rate=hp.learning_rate)


def _head_sizes(prep: _PrecipitativeTraining) -> List[int]:
    nz = prep.y[0].shape[1]
    return [nz, nz] + ([1] if prep.has_dead else []) + [nz]


def _train_hip(hp: PrecipitativeHyperparameters, prep: _PrecipitativeTraining, dev: torch.device):
    """The same minibatches in the same order through ``fv3net_amd.train.PrecipitativeTrainer`` (csrc/mlp_train.hip)."""
    trainer = precipitative_trainer(hp, prep, dev)
    for batches in epoch_minibatches(prep.xin.shape[0], hp.batch_size, hp.epochs, hp.seed, dev):
        for idx in batches:
            trainer.step(idx)
    hidden_k, hidden_b, out_k, out_b = trainer.parameters(_head_sizes(prep))
    if prep.has_dead:   # dropped on export
        out_k, out_b = out_k[:2] + out_k[3:], out_b[:2] + out_b[3:]
    return hidden_k, hidden_b, out_k, out_b


def regularizer_coefficients(config: Optional[Tuple[str, Mapping]]) -> Tuple[float, float, bool]:
    """``(l1, l2, set)`` of a ``residual_regularizer``: Keras's ``regularizers.l1(l1=0.01)``, ``l2(l2=0.01)`` and
    ``l1_l2(l1=0.01, l2=0.01)``; ``None`` and ``"none"`` are no regulariser."""
    if config is None:
        return 0.0, 0.0, False
    name, kwargs = config
    kwargs = dict(kwargs or {})
    allowed = {"none": (), "l1": ("l1",), "l2": ("l2",), "l1_l2": ("l1", "l2")}
    if name not in allowed:
        raise ValueError(f"residual_regularizer must be one of {sorted(allowed)}, got {name!r}")
    unknown = [k for k in kwargs if k not in allowed[name]]
    if unknown:
        raise ValueError(f"regulariser {name!r} takes {list(allowed[name])}, got {unknown}")
    l1 = float(kwargs.get("l1", 0.01)) if "l1" in allowed[name] else 0.0
    l2 = float(kwargs.get("l2", 0.01)) if "l2" in allowed[name] else 0.0
    if not (l1 >= 0 and l2 >= 0 and np.isfinite(l1) and np.isfinite(l2)):
        raise ValueError(f"regulariser coefficients must be finite and >= 0, got l1={l1}, l2={l2}")
    return l1, l2, name != "none"


def train_precipitative_model(hyperparameters: PrecipitativeHyperparameters, train_batches: Sequence[Dataset],
                              device: Optional[str] = None, backend: Optional[str] = None) -> HipPrecipitativeModel:
    """Fit normalisation on up to ``normalization_fit_samples`` samples and train the graph of precipitative.py:181-279
    with Adam: ``Dense(width, relu) x (depth-1)``, four linear heads, the closure from the unclipped ``delp`` inside the training
    graph, and the std-scaled MSE summed over ``dQ1``, ``dQ2`` and ``total_precipitation_rate`` as ``train_dense_model``
    computes it.  The one-feature head for total_precipitation_rate reaches no output: without ``residual_regularizer`` it
    receives no gradient; with it, it is trained through the activity regulariser alone.  It is dropped on export either way.

    ``backend``: ``None`` / ``"torch"`` steps through ``torch.nn.Linear``, autograd and ``torch.optim.Adam``; ``"hip"`` through
    the project's own kernels (``fv3net_amd.train.PrecipitativeTrainer``; needs a GPU).  Normalisation, initialisation (all four
    heads are drawn, in the reference's order) and the minibatch sequence are shared: both start from bitwise-equal parameters and
    see the same rows in the same order.  The callbacks and ``validation_batches`` of the reference are out of scope."""
    hp = hyperparameters
    backend, dev = resolve_backend(backend, device)
    prep = _prepare_precipitative_training(hp, train_batches)
    weights = (_train_hip if backend == "hip" else _train_torch)(hp, prep, dev)
    names_in, names_out = hp.input_variables, hp.output_variables
    spec = precipitative_spec_from_arrays(names_in, prep.x_mean, prep.x_std, weights[0], weights[1], weights[2], weights[3],
                                          prep.y_mean[:2], prep.y_std[:2], clip=hp.clip)
    return HipPrecipitativeModel(names_in, names_out, spec, couple_precip_to_dQ1_dQ2=hp.couple_precip_to_dQ1_dQ2,
                                 unstacked_dims=hp.unstacked_dims)
