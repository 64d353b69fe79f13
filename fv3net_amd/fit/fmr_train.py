"""Training the full-model replacement: ``fv3fit``'s ``"fmr"`` trainer (external/fv3fit/fv3fit/pytorch/recurrent/train_fmr.py,
discriminator.py, image_pool.py) with ``backend="torch"`` -- ``RecurrentGeneratorTwin`` and ``DiscriminatorTwin`` under autograd
on any device in any dtype -- and ``backend="hip"`` -- ``HipRecurrentGenerator`` and ``HipDiscriminator`` on the training
kernels, the window loss and its gradient by ``fv3hip_fmr_loss_grad``, the GAN loss and the optimisers
torch's.  The hip backend needs the GPU and has no fallback.

Two things differ from the reference as written, both on purpose:

  * its ``train_on_batch`` hands the discriminator the 6-D ``[sample, time, tile, channel, x, y]`` tensor, which the
    discriminator's convolutions refuse; here the time dimension is folded into the samples, as the reference's own comment
    intends.  Every loss is a mean over all elements, so nothing else changes.
  * its generator wraps every step in ``torch.utils.checkpoint``, whose recomputation advances the Python clock a second time:
    with ``samples_per_day`` set the reference's gradient is not the gradient of its loss.  Both backends here compute the
    true gradient -- step ``i`` reads the clock at ``i - 1`` forwards and backwards -- and keep the step activations.
"""
import dataclasses
import random
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch

from .. import fmr_train as layers
from ..cyclegan import check_convolution_type
from .cyclegan_train import (CycleGANOptimizerConfig, DiscriminatorTwin, HipDiscriminator, ImagePool, LossConfig, TwinExports, _nested,
                             _normalised, flat_scaler_pairs, initialise_twins, set_requires_grad)
from .fmr import (RecurrentGeneratorTwin, fmr_spec_from_state_dict, fmr_state_dict_from_spec, recurrent_generator_spec_from_state_dict,
                  recurrent_generator_state_dict)
from .training import check_backend

nn = torch.nn

LOSS_KEYS = ("target_loss", "identity_loss", "gan_loss", "generator_loss", "discriminator_loss", "train_loss")


# ---------------------------------------------------------------------------------------------
# configuration: the reference's dataclasses, field for field
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class RecurrentGeneratorConfig:
    """``RecurrentGeneratorConfig`` (recurrent/generator.py:22-83)."""

    n_convolutions: int = 3
    n_resnet: int = 3
    kernel_size: int = 3
    strided_kernel_size: int = 4
    max_filters: int = 256
    use_geographic_bias: bool = True
    use_geographic_features: bool = True
    step_type: str = "resnet"
    samples_per_day: Optional[int] = None

    def __post_init__(self):
        if self.step_type not in ("resnet", "conv"):
            raise ValueError(f"step_type must be 'resnet' or 'conv', got {self.step_type!r}")

    def build(self, channels: int, nx: int, convolution_type: str, xyz=None, xyz_bottom=None) -> RecurrentGeneratorTwin:
        return RecurrentGeneratorTwin(channels, nx, self.n_convolutions, self.n_resnet, self.kernel_size, self.strided_kernel_size,
                                      self.max_filters, self.use_geographic_bias, self.use_geographic_features, self.step_type,
                                      self.samples_per_day, convolution_type, xyz, xyz_bottom)


@dataclasses.dataclass
class RecurrentDiscriminatorConfig:
    """The recurrent ``DiscriminatorConfig`` (recurrent/discriminator.py:15-49): no geographic features."""

    n_convolutions: int = 3
    kernel_size: int = 3
    strided_kernel_size: int = 3
    max_filters: int = 256

    def build(self, channels: int, nx: int, convolution_type: str) -> DiscriminatorTwin:
        return DiscriminatorTwin(channels, nx, self.n_convolutions, self.kernel_size, self.strided_kernel_size, self.max_filters,
                                 use_geographic_features=False, use_geographic_embedded_bias=False, convolution_type=convolution_type)


@dataclasses.dataclass
class FMRNetworkConfig:
    """``FMRNetworkConfig`` (train_fmr.py:54-149); nested configurations may be given as mappings, whose unknown keys are
    refused."""

    generator_optimizer: CycleGANOptimizerConfig = dataclasses.field(default_factory=lambda: CycleGANOptimizerConfig("Adam"))
    discriminator_optimizer: CycleGANOptimizerConfig = dataclasses.field(default_factory=lambda: CycleGANOptimizerConfig("Adam"))
    generator: RecurrentGeneratorConfig = dataclasses.field(default_factory=RecurrentGeneratorConfig)
    discriminator: RecurrentDiscriminatorConfig = dataclasses.field(default_factory=RecurrentDiscriminatorConfig)
    convolution_type: str = "conv2d"
    identity_loss: LossConfig = dataclasses.field(default_factory=LossConfig)
    target_loss: LossConfig = dataclasses.field(default_factory=LossConfig)
    gan_loss: LossConfig = dataclasses.field(default_factory=LossConfig)
    identity_weight: float = 1.0
    target_weight: float = 1.0
    generator_weight: float = 1.0
    discriminator_weight: float = 1.0
    reload_path: Optional[str] = None

    def __post_init__(self):
        self.generator_optimizer = _nested(self.generator_optimizer, CycleGANOptimizerConfig, "generator_optimizer")
        self.discriminator_optimizer = _nested(self.discriminator_optimizer, CycleGANOptimizerConfig, "discriminator_optimizer")
        self.generator = _nested(self.generator, RecurrentGeneratorConfig, "generator")
        self.discriminator = _nested(self.discriminator, RecurrentDiscriminatorConfig, "discriminator")
        for key in ("identity_loss", "target_loss", "gan_loss"):
            setattr(self, key, _nested(getattr(self, key), LossConfig, key))
        if self.convolution_type not in ("conv2d", "halo_conv2d"):
            raise ValueError(f"convolution_type {self.convolution_type} not supported")

    def build(self, n_state: int, nx: int, n_batch: int, xyz=None, xyz_bottom=None, seed: int = 0, backend: str = "torch", device=None,
              dtype=torch.float32, state_dict: Optional[Mapping[str, Any]] = None,
              reference_order_gradients: bool = True) -> "FMRTrainer":
        """The two networks, built and initialised on the host under ``torch.manual_seed(seed)`` in the reference's order
        (generator, discriminator, then ``init_weights`` on each), or loaded from ``state_dict`` (keyed as
        ``FMRModule.state_dict()``); the two optimisers and the trainer.  Both backends start from bitwise-equal parameters.
        ``reference_order_gradients``: the twins pad tile by tile (``fit.cyclegan.set_reference_order_gradients``), so that a
        float64 step of the torch backend is the reference's (fold and direct-call checkpoint applied) bit for bit -- the
        biases in front of an instance norm, whose gradient is rounding noise, included."""
        torch.manual_seed(seed)
        twins = {"generator": self.generator.build(n_state, nx, self.convolution_type, xyz, xyz_bottom),
                 "discriminator": self.discriminator.build(n_state, nx, self.convolution_type)}
        initialise_twins(twins, state_dict, reference_order_gradients)
        return FMRTrainer(twins, self, n_batch, n_state, nx, backend=backend, device=device, dtype=dtype)


@dataclasses.dataclass
class FMRTrainingConfig:
    """``FMRTrainingConfig`` (train_fmr.py:354-438)."""

    n_epoch: int = 20
    shuffle_buffer_size: int = 10
    samples_per_batch: int = 1
    validation_batch_size: Optional[int] = None
    in_memory: bool = False


@dataclasses.dataclass
class FMRHyperparameters:
    """``FMRHyperparameters`` (train_fmr.py:311-339)."""

    state_variables: List[str]
    normalization_fit_samples: int = 50_000
    network: FMRNetworkConfig = dataclasses.field(default_factory=FMRNetworkConfig)
    training: FMRTrainingConfig = dataclasses.field(default_factory=FMRTrainingConfig)

    def __post_init__(self):
        self.network = _nested(self.network, FMRNetworkConfig, "network")
        self.training = _nested(self.training, FMRTrainingConfig, "training")

    @property
    def samples_per_batch(self) -> int:
        return self.training.samples_per_batch

    @property
    def variables(self):
        return tuple(self.state_variables)


# ---------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------
def _fold(x):
    """``[sample, time, ...]`` -> ``[sample * time, ...]``."""
    return x.reshape(x.shape[0] * x.shape[1], *x.shape[2:])


class PreparedBatch:
    """A batch as a trainer's networks take it (``FMRTrainer.prepare``): on its device, in its dtype and layout."""

    def __init__(self, tensor: torch.Tensor):
        self.tensor = tensor


class FMRTrainer(TwinExports):
    """``FMRTrainer.train_on_batch`` (train_fmr.py:222-294) in the reference's order: the generator stage with the discriminator
    frozen, then real, pooled fake (``ImagePool(50)``, queried also when evaluating) and the discriminator's step.

    ``twins``: the initialised plain-torch ``generator`` and ``discriminator`` of ``n_state`` channels on faces of ``nx``
    cells.  ``backend="torch"`` trains them as they are (on ``device``, in ``dtype``); ``backend="hip"`` trains
    ``HipRecurrentGenerator`` / ``HipDiscriminator`` copies of them on the GPU.  A batch is ``[sample, time, tile, channel, x, y]``
    with at least two times, on the host or on the device, for both backends.  ``observer(stage)``, if given to
    ``train_on_batch``, is called after the backward pass of each stage (``"generator"``, ``"discriminator"``) and before its
    optimiser's step: ``gradients(stage)`` then holds that stage's gradients under the reference's ``state_dict`` keys."""

    NETWORKS = ("generator", "discriminator")
    generator_state_dict = staticmethod(recurrent_generator_state_dict)

    def __init__(self, twins: Mapping[str, nn.Module], config: FMRNetworkConfig, batch_size: int, n_state: int, nx: int,
                 backend: str = "torch", device=None, dtype=torch.float32):
        backend = check_backend(backend)
        check_convolution_type(config.convolution_type)
        self.backend, self.config, self.batch_size, self.n_state, self.nx = backend, config, batch_size, n_state, nx
        self.twins = dict(twins)
        if backend == "hip":
            from ..cube import cuda_device

            self.device, self.dtype = cuda_device(device or "cuda", "FMRTrainer(backend='hip')"), torch.float32
            self.networks = {"generator": layers.HipRecurrentGenerator(self._generator_spec(), config.convolution_type).to(self.device),
                             "discriminator": HipDiscriminator(self.twins["discriminator"]).to(self.device)}
        else:
            self.device, self.dtype = torch.device(device or "cpu"), dtype
            self.networks = {key: twin.to(device=self.device, dtype=dtype) for key, twin in self.twins.items()}
        self.optimizer_generator = config.generator_optimizer.instance(self.networks["generator"].parameters())
        self.optimizer_discriminator = config.discriminator_optimizer.instance(self.networks["discriminator"].parameters())
        self.identity_loss, self.target_loss, self.gan_loss = (config.identity_loss.instance, config.target_loss.instance,
                                                               config.gan_loss.instance)
        self.identity_weight, self.target_weight = config.identity_weight, config.target_weight
        self.generator_weight, self.discriminator_weight = config.generator_weight, config.discriminator_weight
        self.target_real: Optional[torch.Tensor] = None
        self.target_fake: Optional[torch.Tensor] = None
        self.fake_buffer = ImagePool(50)   # image pool size of 50 used by Zhu et al. (2017)

    def _generator_spec(self):
        twin = self.twins["generator"]
        geo = self.config.generator.use_geographic_features
        xyz = twin.input_bias[1].xyz.detach().cpu().numpy() if geo else None
        xyz_bottom = twin.resnet[0].xyz.detach().cpu().numpy() if geo else None
        return recurrent_generator_spec_from_state_dict(twin.state_dict(), self.n_state, self.nx, convolution_type=self.config.convolution_type,
                                                        xyz=xyz, xyz_bottom=xyz_bottom, **dataclasses.asdict(self.config.generator))

    # -- the batch ------------------------------------------------------------------------------------
    def prepare(self, real) -> PreparedBatch:
        """The batch moved and laid out once, for a caller that trains on it in every epoch."""
        return real if isinstance(real, PreparedBatch) else PreparedBatch(self._prepare(real))

    def _prepare(self, real) -> torch.Tensor:
        if isinstance(real, PreparedBatch):
            return real.tensor
        real = torch.as_tensor(real)
        if real.dim() != 6 or real.shape[2] != 6:
            raise ValueError(f"a batch must be [sample, time, tile, channel, x, y], got shape {tuple(real.shape)}")
        if real.shape[1] < 2:
            raise ValueError(f"a batch needs at least two times (the target loss is a mean over the times after the first), got {real.shape[1]}")
        if self.backend == "hip":   # activations are channel-last
            return real.to(device=self.device, dtype=torch.float32).movedim(3, -1).contiguous()
        return real.to(device=self.device, dtype=self.dtype)

    def _targets(self, pred):
        if self.target_real is None or self.target_real.shape != pred.shape or self.target_real.dtype != pred.dtype:
            self.target_real, self.target_fake = torch.ones_like(pred), torch.zeros_like(pred)
        return self.target_real, self.target_fake

    def _discriminate(self, state):
        """The discriminator on ``[sample, time, ...]``, the time dimension folded into the samples."""
        net = self.networks["discriminator"]
        return net(None, _fold(state))

    # -- the generator stage of the two backends: (identity, target, gan) losses, gradients left in .grad -------------------------
    def _generator_stage_torch(self, real, evaluate_only, observer):
        fake = self.networks["generator"](real[:, 0], real.shape[1])
        pred_fake = self._discriminate(fake)
        target_real, _ = self._targets(pred_fake)
        loss_identity = self.identity_loss(real[:, 0], fake[:, 0]) * self.identity_weight
        loss_target = self.target_loss(real[:, 1:], fake[:, 1:]) * self.target_weight
        loss_gan = self.gan_loss(pred_fake, target_real) * self.generator_weight
        if not evaluate_only:
            self.optimizer_generator.zero_grad()
            (loss_identity + loss_target + loss_gan).backward()
            if observer is not None:
                observer("generator")
            self.optimizer_generator.step()
        return fake.detach(), float(loss_identity.detach()), float(loss_target.detach()), float(loss_gan.detach())

    def _generator_stage_hip(self, real, evaluate_only, observer):
        from .. import ops

        fake = self.networks["generator"](real[:, 0], real.shape[1])   # the [sample, time] view of a time-major tensor
        major = fake.transpose(0, 1)
        leaf = major.detach().requires_grad_(not evaluate_only)
        pred_fake = self._discriminate(leaf)        # (the fold is time-major here: every loss is a mean over all elements)
        target_real, _ = self._targets(pred_fake)
        loss_gan = self.gan_loss(pred_fake, target_real) * self.generator_weight
        kinds = (self.config.identity_loss.loss_type, self.identity_weight, self.config.target_loss.loss_type, self.target_weight)
        if evaluate_only:
            values = ops.fmr_loss_grad(fake.detach(), real, None, None, *kinds)
        else:
            dgan = torch.autograd.grad(loss_gan, leaf)[0].contiguous()
            dfake = torch.empty_like(dgan)
            values = ops.fmr_loss_grad(fake.detach(), real, dgan.transpose(0, 1), dfake.transpose(0, 1), *kinds)
            self.optimizer_generator.zero_grad()
            major.backward(dfake)
            if observer is not None:
                observer("generator")
            self.optimizer_generator.step()
        identity, target = values.tolist()
        return fake.detach(), identity, target, float(loss_gan.detach())

    def train_on_batch(self, real, evaluate_only: bool = False, observer: Optional[Callable[[str], None]] = None) -> Dict[str, float]:
        real = self._prepare(real)
        discriminator = self.networks["discriminator"]
        # don't update the discriminator when training the generator to fool it
        set_requires_grad([discriminator], requires_grad=False)
        stage = self._generator_stage_hip if self.backend == "hip" else self._generator_stage_torch
        fake, loss_identity, loss_target, loss_gan = stage(real, evaluate_only, observer)
        loss_g = loss_identity + loss_target + loss_gan

        # do update the discriminator when training it to identify samples
        set_requires_grad([discriminator], requires_grad=True)
        pred_real = self._discriminate(real)
        target_real, target_fake = self._targets(pred_real)
        loss_d_real = self.gan_loss(pred_real, target_real) * self.discriminator_weight
        # window by window, each a copy of its own: the pool keeps what it is given, and a window of the generator's output is
        # a view that would keep the whole batch alive (the draws from ``random`` are those of one query over all windows)
        fake = torch.cat([self.fake_buffer.query((torch.zeros(1), fake[w:w + 1].clone()))[1] for w in range(fake.shape[0])], 0)
        pred_fake = self._discriminate(fake.detach())
        loss_d_fake = self.gan_loss(pred_fake, target_fake) * self.discriminator_weight
        loss_d = loss_d_real + loss_d_fake
        if not evaluate_only:
            self.optimizer_discriminator.zero_grad()
            loss_d.backward()
            if observer is not None:
                observer("discriminator")
            self.optimizer_discriminator.step()
        loss_d = float(loss_d.detach())
        return {"target_loss": loss_target, "identity_loss": loss_identity, "gan_loss": loss_gan, "generator_loss": loss_g,
                "discriminator_loss": loss_d, "train_loss": loss_g + loss_d}

    def evaluate_on_dataset(self, dataset) -> Dict[str, float]:
        """The mean of every loss over the batches of ``dataset``, without a step (the image pool is queried all the same)."""
        losses = []
        for batch in dataset:
            with torch.no_grad():
                losses.append(self.train_on_batch(batch, evaluate_only=True))
        return {name: float(np.mean([data[name] for data in losses])) for name in losses[0]}

    # (``state_dict`` and ``gradients``: ``TwinExports``, keyed as ``FMRModule.state_dict()``)

# ---------------------------------------------------------------------------------------------
# the training function
# ---------------------------------------------------------------------------------------------
def _joined(batches, names: Sequence[str]) -> Dict[str, np.ndarray]:
    to_np = lambda a: np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)   # noqa: E731
    return {name: np.concatenate([to_np(b[name]) for b in batches], axis=0) for name in names}


def train_fmr(hyperparameters: FMRHyperparameters, train_batches, validation_batches=None, device=None, backend: Optional[str] = None,
              xyz=None, xyz_bottom=None, seed: int = 0):
    """The reference's ``"fmr"`` training function (train_fmr.py:446-509) on in-memory batches.

    ``train_batches``: a sequence of mappings of every state variable to ``[sample, time, tile, x, y(, z)]``.  Per variable a
    ``StandardScaler(n_sample_dims=5)`` is fitted on up to ``normalization_fit_samples`` samples.  As in ``fit_loop``: with
    ``shuffle_buffer_size > 1`` the samples are shuffled (here with Python's ``random``, over all of them) and then cut into
    batches of ``samples_per_batch``; the batches are shuffled with ``random.shuffle`` after every epoch; the validation
    samples are evaluated in batches of ``validation_batch_size`` (None: all at once); every epoch ``fit.dump`` writes the model
    to ``model_epoch_{i:04d}_loss_{target_loss:0.4f}`` under the working directory.  ``in_memory`` keeps the batches on the
    trainer's device.  ``network.reload_path``: an artifact written here *with* its discriminator, from whose parameters and
    scalers training resumes.  ``xyz`` ``[6, 3, nx, nx]`` / ``xyz_bottom`` ``[6, 3, nx >> n_convolutions, ...]``: the grids of the
    geographic features, data of the model here.  ``backend="torch"`` (the default) runs the twins under autograd on ``device``;
    ``"hip"`` runs the training kernels and needs the GPU.  Returns a ``HipFullModelReplacement`` that carries the discriminator
    and, as ``history``, the per-epoch mean of the six losses (and ``val_*`` where validation batches are given)."""
    from . import io
    from .fmr import HipFullModelReplacement
    from .graph import fit_scalers

    hp = hyperparameters
    backend = "torch" if backend is None else backend
    names = [str(n) for n in hp.state_variables]
    if not train_batches:
        raise ValueError("train_fmr needs at least one batch")
    arrays = _joined(train_batches, names)
    state_dict = None
    if hp.network.reload_path is not None:
        reloaded = io.load(hp.network.reload_path)
        if not isinstance(reloaded, HipFullModelReplacement) or reloaded.discriminator is None:
            raise ValueError(f"{hp.network.reload_path} holds no full-model replacement with its discriminator: training cannot resume from it")
        scalers = dict(reloaded.spec.scalers)
        state_dict = {**fmr_state_dict_from_spec(reloaded.spec),
                      **{f"discriminator.{k}": torch.from_numpy(v) for k, v in reloaded.discriminator["state_dict"].items()}}
        xyz = reloaded.spec.generator.xyz if xyz is None else xyz
        xyz_bottom = reloaded.spec.generator.xyz_bottom if xyz_bottom is None else xyz_bottom
    else:
        scalers = fit_scalers({n: a[:hp.normalization_fit_samples] for n, a in arrays.items()})
    real = _normalised(arrays, names, scalers)
    n_state, nx = int(real.shape[3]), int(real.shape[-1])
    trainer = hp.network.build(n_state, nx, hp.training.samples_per_batch, xyz, xyz_bottom, seed=seed, backend=backend, device=device,
                               state_dict=state_dict)
    order = list(range(len(real)))
    if hp.training.shuffle_buffer_size > 1:
        random.shuffle(order)
    step = hp.training.samples_per_batch
    batches = [real[order[i:i + step]] for i in range(0, len(order), step)]
    if hp.training.in_memory:
        batches = [trainer.prepare(b) for b in batches]
    validation = []
    if validation_batches:
        val = _normalised(_joined(validation_batches, names), names, scalers)
        size = len(val) if hp.training.validation_batch_size is None else hp.training.validation_batch_size
        validation = [val[i:i + size] for i in range(0, len(val), size)]

    def model():
        state = trainer.state_dict()
        spec = fmr_spec_from_state_dict(state, names, flat_scaler_pairs(scalers), nx, hp.network.convolution_type, xyz, xyz_bottom,
                                        **dataclasses.asdict(hp.network.generator))
        prefix = "discriminator."
        out = HipFullModelReplacement(names, spec, {"config": dict(trainer.twins["discriminator"].config),
                                                    "state_dict": {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}})
        out.history = {k: list(v) for k, v in history.items()}
        return out

    history: Dict[str, List[float]] = {}
    for epoch in range(1, hp.training.n_epoch + 1):
        rows = [trainer.train_on_batch(batch) for batch in batches]
        for key in LOSS_KEYS:
            history.setdefault(key, []).append(float(np.mean([r[key] for r in rows])))
        if validation:
            for key, value in trainer.evaluate_on_dataset(validation).items():
                history.setdefault(f"val_{key}", []).append(value)
        io.dump(model(), f"model_epoch_{epoch:04d}_loss_{history['target_loss'][-1]:0.4f}")
        random.shuffle(batches)
    return model()
