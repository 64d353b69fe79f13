"""Training the CycleGAN: ``fv3fit``'s ``"cyclegan"`` trainer (external/fv3fit/fv3fit/pytorch/cyclegan/cyclegan_trainer.py:412-693,
image_pool.py, discriminator.py:68-169) with ``backend="torch"`` -- the plain-torch twins under autograd on any device -- and
``backend="hip"`` -- the same networks on the training kernels of DESIGN section 27, which need the GPU and have no fallback.

``DiscriminatorTwin`` is the reference's ``Discriminator`` in plain ``torch.nn`` on ``append_halos_tensor`` with the reference's
``state_dict`` keys, the counterpart of ``GeneratorTwin``; ``HipDiscriminator`` is the same network on the kernels, channel-last,
with its parameters in the kernels' weight layout.  Both backends are initialised on the host under ``torch.manual_seed(seed)``
through the twins, so they start from bitwise-equal parameters.
"""
import dataclasses
import itertools
import random
from typing import Any, Callable, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import cyclegan_train as layers
from ..cyclegan import N_GEOGRAPHIC_FEATURES, SECONDS_PER_DAY, check_convolution_type, theta_from_seconds
from .cyclegan import (GeneratorTwin, _ConvBlock, _GeographicBias, _halo_convolution, _single_tile_convolution,   # noqa: F401
                       generator_spec_from_state_dict, generator_state_dict, set_reference_order_gradients)
from .training import check_backend, strict_fields

nn = torch.nn

LOSS_KEYS = ("b_to_a_gan_loss", "a_to_b_gan_loss", "discriminator_a_loss", "discriminator_b_loss", "cycle_loss", "identity_loss",
             "generator_loss", "discriminator_loss", "train_loss")


def _nested(value, cls, what):
    return value if isinstance(value, cls) else cls(**strict_fields(cls, value, what))


# ---------------------------------------------------------------------------------------------
# the discriminator
# ---------------------------------------------------------------------------------------------
def check_discriminator(nx: int, n_convolutions: int = 3, kernel_size: int = 3, strided_kernel_size: int = 3, max_filters: int = 256):
    """What is built of ``DiscriminatorConfig``; anything else is refused with the offending value."""
    if int(strided_kernel_size) not in (3, 4):
        raise NotImplementedError(f"strided_kernel_size = {strided_kernel_size} is not built; supported: 3 and 4")
    if int(kernel_size) not in (3, 5, 7):
        raise NotImplementedError(f"kernel_size = {kernel_size} is not built; supported: 3, 5 and 7")
    if int(n_convolutions) < 1:
        raise ValueError(f"n_convolutions must be at least 1, got {n_convolutions}")
    if int(max_filters / 2 ** (int(n_convolutions) - 1)) < 1:
        raise ValueError(f"max_filters = {max_filters} leaves no filters in the first of {n_convolutions} strided layers")
    for level in range(int(n_convolutions)):
        if (int(nx) >> level) % 2 or (int(nx) >> level) < 2:
            raise ValueError(f"strided layer {level} of the discriminator has an input edge of {int(nx) / 2 ** level:g} cells (nx = {nx}): "
                             "the stride-2 convolutions need an even edge")


def discriminator_plan(channels: int, n_convolutions: int, kernel_size: int, strided_kernel_size: int, max_filters: int,
                       use_geographic_features: bool) -> List[Tuple[str, str, int, int, int]]:
    """(name, kind, c_in, c_out, k) of every convolution in execution order."""
    m = int(max_filters / 2 ** (n_convolutions - 1))
    plan = [("strided0", "strided", channels + (N_GEOGRAPHIC_FEATURES if use_geographic_features else 0), m, strided_kernel_size)]
    plan += [(f"strided{i}", "strided", m * 2 ** (i - 1), m * 2 ** i, strided_kernel_size) for i in range(1, n_convolutions)]
    return plan + [("final", "regular", max_filters, max_filters, kernel_size), ("patch", "regular", max_filters, 1, 3)]


class _LeakyConvBlock(nn.Module):
    """``ConvBlock`` with the discriminator's activation."""

    def __init__(self, conv, c_out):
        super().__init__()
        from .cyclegan import _Fold

        self.conv_block = nn.Sequential(conv, _Fold(nn.InstanceNorm2d(c_out)), nn.LeakyReLU(0.2))

    def forward(self, x):
        return self.conv_block(x)


class DiscriminatorTwin(nn.Module):
    """``Discriminator`` (discriminator.py:68-169) with ``lon`` ``[6, nx, nx]`` and ``xyz`` ``[6, 3, nx, nx]`` given, not read
    from a catalogue; its ``state_dict`` has the reference's keys.  ``forward(time, state)``: ``time`` ``[batch]`` seconds since
    1970, ``state`` ``[batch, tile, channel, x, y]`` -> ``[batch, tile, 1, x', y']``."""

    def __init__(self, in_channels: int, nx: int, n_convolutions: int = 3, kernel_size: int = 3, strided_kernel_size: int = 3,
                 max_filters: int = 256, use_geographic_features: bool = True, use_geographic_embedded_bias: bool = False,
                 convolution_type: str = "halo_conv2d", lon=None, xyz=None):
        super().__init__()
        check_discriminator(nx, n_convolutions, kernel_size, strided_kernel_size, max_filters)
        check_convolution_type(convolution_type)
        conv = _halo_convolution if convolution_type == "halo_conv2d" else _single_tile_convolution
        plan = discriminator_plan(in_channels, n_convolutions, kernel_size, strided_kernel_size, max_filters, use_geographic_features)
        _, _, ci, co, k = plan[0]
        convs = [conv(ci, co, k, stride=2)]
        if use_geographic_embedded_bias:
            convs.append(_GeographicBias(co, nx // 2))
        convs.append(nn.LeakyReLU(0.2))
        for _, kind, ci, co, k in plan[1:-1]:
            convs.append(_LeakyConvBlock(conv(ci, co, k, stride=2 if kind == "strided" else 1), co))
        _, _, ci, co, k = plan[-1]
        self._sequential = nn.Sequential(*convs, conv(ci, co, k))
        self.config = dict(in_channels=in_channels, nx=nx, n_convolutions=n_convolutions, kernel_size=kernel_size,
                           strided_kernel_size=strided_kernel_size, max_filters=max_filters,
                           use_geographic_features=use_geographic_features, use_geographic_embedded_bias=use_geographic_embedded_bias,
                           convolution_type=convolution_type)
        self.use_geographic_features = use_geographic_features
        if use_geographic_features:
            if lon is None or xyz is None:
                raise ValueError("a discriminator with geographic features needs lon [6, nx, nx] and xyz [6, 3, nx, nx]")
            self.local_time_zero_radians = torch.as_tensor(np.asarray(lon)).float()[:, None]
            self.xyz = torch.as_tensor(np.asarray(xyz)).float()

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self.use_geographic_features:
            self.local_time_zero_radians, self.xyz = fn(self.local_time_zero_radians), fn(self.xyz)
        return self

    def forward(self, time, state):
        x = state
        if self.use_geographic_features:
            offset = time % SECONDS_PER_DAY / SECONDS_PER_DAY * 2 * np.pi
            local = self.local_time_zero_radians[None, :] + offset[:, None, None, None, None]
            xyz = torch.stack([self.xyz for _ in range(x.shape[0])])
            x = torch.cat([x, torch.sin(local), torch.cos(local), xyz], dim=-3)
        return self._sequential(x)

    def conv_keys(self) -> Dict[str, str]:
        """plan name -> the state-dict prefix of its ``Conv2d``."""
        c = self.config
        wrapped = "1._wrapped" if c["convolution_type"] == "halo_conv2d" else "_wrapped"
        shift = 1 + (1 if c["use_geographic_embedded_bias"] else 0)   # modules after the first convolution, before the blocks
        keys = {"strided0": f"_sequential.0.{wrapped}"}
        for i in range(1, c["n_convolutions"]):
            keys[f"strided{i}"] = f"_sequential.{shift + i}.conv_block.0.{wrapped}"
        keys["final"] = f"_sequential.{shift + c['n_convolutions']}.conv_block.0.{wrapped}"
        keys["patch"] = f"_sequential.{shift + c['n_convolutions'] + 1}.{wrapped}"
        return keys


class HipDiscriminator(nn.Module):
    """``DiscriminatorTwin`` on the training kernels, channel-last: ``forward(theta, state)`` with ``theta`` ``[S]`` float32
    radians and ``state`` ``[S, 6, n, n, C]`` -> ``[S, 6, n', n', 1]``.  The first layer's leaky ReLU (no norm before it) and
    the embedded-bias add are torch's."""

    def __init__(self, twin: DiscriminatorTwin):
        super().__init__()
        c = self.config = dict(twin.config)
        state = twin.state_dict()
        self.plan = discriminator_plan(c["in_channels"], c["n_convolutions"], c["kernel_size"], c["strided_kernel_size"], c["max_filters"],
                                       c["use_geographic_features"])
        self.convs = nn.ModuleDict()
        for (name, kind, ci, co, k), prefix in zip(self.plan, twin.conv_keys().values()):
            conv = layers.CubeConv(ci, co, kind, k, c["convolution_type"])
            conv.load_torch(state[f"{prefix}.weight"].detach().cpu().numpy(), state[f"{prefix}.bias"].detach().cpu().numpy())
            self.convs[name] = conv
        self.embedded_bias = None
        if c["use_geographic_embedded_bias"]:
            self.embedded_bias = nn.Parameter(state["_sequential.1.bias"].detach().float().permute(0, 2, 3, 1).contiguous().clone())
        self.use_geographic_features = c["use_geographic_features"]
        if self.use_geographic_features:
            self.register_buffer("lon", twin.local_time_zero_radians[:, 0].float().contiguous().clone(), persistent=False)
            self.register_buffer("xyz", twin.xyz.float().permute(0, 2, 3, 1).contiguous().clone(), persistent=False)

    def forward(self, theta, state):
        x = state
        if self.use_geographic_features:
            x = layers._InputFeatures.apply(x, self.lon, self.xyz, theta.to(torch.float32).contiguous())
        x = self.convs["strided0"](x)
        if self.embedded_bias is not None:
            x = x + self.embedded_bias
        x = torch.nn.functional.leaky_relu(x, 0.2)
        for name, *_ in self.plan[1:-1]:
            x = layers.instance_norm_act(self.convs[name](x), None, 0.2)
        return self.convs["patch"](x)

    def twin_state_dict(self, twin: DiscriminatorTwin) -> Dict[str, torch.Tensor]:
        """The parameters as they stand under the reference's keys."""
        out = {}
        for name, prefix in twin.conv_keys().items():
            w, b = self.convs[name].torch_arrays()
            out[f"{prefix}.weight"], out[f"{prefix}.bias"] = torch.from_numpy(w), torch.from_numpy(b)
        if self.embedded_bias is not None:
            out["_sequential.1.bias"] = self.embedded_bias.detach().cpu().permute(0, 3, 1, 2).contiguous()
        return out


# ---------------------------------------------------------------------------------------------
# configuration: the reference's dataclasses, field for field
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class LossConfig:
    loss_type: str = "mse"

    def __post_init__(self):
        if self.loss_type not in ("mse", "mae"):
            raise ValueError(f"loss_type must be 'mse' or 'mae', got '{self.loss_type}'")

    @property
    def instance(self) -> nn.Module:
        return nn.MSELoss() if self.loss_type == "mse" else nn.L1Loss()


@dataclasses.dataclass
class CycleGANOptimizerConfig:
    """``fv3fit.pytorch.optimizer.OptimizerConfig``: a ``torch.optim`` class by name."""

    name: str = "AdamW"
    kwargs: Mapping[str, Any] = dataclasses.field(default_factory=dict)

    def instance(self, params):
        if not hasattr(torch.optim, self.name):
            raise ValueError(f"torch.optim has no optimizer {self.name!r}")
        return getattr(torch.optim, self.name)(params=params, **self.kwargs)


class _NullScheduler:
    def step(self):
        pass


@dataclasses.dataclass
class CycleGANSchedulerConfig:
    """``fv3fit.pytorch.optimizer.SchedulerConfig``: a ``torch.optim.lr_scheduler`` class by name, or none."""

    name: Optional[str] = None
    kwargs: Mapping[str, Any] = dataclasses.field(default_factory=dict)

    def instance(self, optimizer):
        if self.name is None:
            return _NullScheduler()
        if not hasattr(torch.optim.lr_scheduler, self.name):
            raise ValueError(f"torch.optim.lr_scheduler has no scheduler {self.name!r}")
        return getattr(torch.optim.lr_scheduler, self.name)(optimizer, **self.kwargs)


@dataclasses.dataclass
class CycleGANGeneratorConfig:
    """``GeneratorConfig`` (generator.py:19-60)."""

    n_convolutions: int = 3
    n_resnet: int = 3
    kernel_size: int = 3
    strided_kernel_size: int = 4
    max_filters: int = 256
    use_geographic_bias: bool = True
    disable_convolutions: bool = False
    use_geographic_features: bool = True
    use_geographic_embedded_bias: bool = False

    def build(self, channels: int, nx: int, convolution_type: str, lon=None, xyz=None) -> GeneratorTwin:
        return GeneratorTwin(channels, nx, self.n_convolutions, self.n_resnet, self.kernel_size, self.strided_kernel_size, self.max_filters,
                             self.use_geographic_bias, self.use_geographic_features, self.use_geographic_embedded_bias, convolution_type,
                             lon, xyz, self.disable_convolutions)


@dataclasses.dataclass
class DiscriminatorConfig:
    """``DiscriminatorConfig`` (discriminator.py:16-65)."""

    n_convolutions: int = 3
    kernel_size: int = 3
    strided_kernel_size: int = 3
    max_filters: int = 256
    use_geographic_features: bool = True
    use_geographic_embedded_bias: bool = False

    def build(self, channels: int, nx: int, convolution_type: str, lon=None, xyz=None) -> DiscriminatorTwin:
        return DiscriminatorTwin(channels, nx, self.n_convolutions, self.kernel_size, self.strided_kernel_size, self.max_filters,
                                 self.use_geographic_features, self.use_geographic_embedded_bias, convolution_type, lon, xyz)


@dataclasses.dataclass
class CycleGANNetworkConfig:
    """``CycleGANNetworkConfig`` (cyclegan_trainer.py:31-138); nested configurations may be given as mappings, whose unknown keys
    are refused."""

    optimizer: CycleGANOptimizerConfig = dataclasses.field(default_factory=lambda: CycleGANOptimizerConfig("Adam"))
    generator: CycleGANGeneratorConfig = dataclasses.field(default_factory=CycleGANGeneratorConfig)
    discriminator: DiscriminatorConfig = dataclasses.field(default_factory=DiscriminatorConfig)
    convolution_type: str = "conv2d"
    identity_loss: LossConfig = dataclasses.field(default_factory=LossConfig)
    cycle_loss: LossConfig = dataclasses.field(default_factory=LossConfig)
    gan_loss: LossConfig = dataclasses.field(default_factory=LossConfig)
    identity_weight: float = 0.5
    cycle_weight: float = 1.0
    generator_weight: float = 1.0
    discriminator_weight: float = 1.0

    def __post_init__(self):
        self.optimizer = _nested(self.optimizer, CycleGANOptimizerConfig, "optimizer")
        self.generator = _nested(self.generator, CycleGANGeneratorConfig, "generator")
        self.discriminator = _nested(self.discriminator, DiscriminatorConfig, "discriminator")
        for key in ("identity_loss", "cycle_loss", "gan_loss"):
            setattr(self, key, _nested(getattr(self, key), LossConfig, key))
        if self.convolution_type not in ("conv2d", "halo_conv2d"):
            raise ValueError(f"convolution_type {self.convolution_type} not supported")

    def build(self, n_state: int, nx: int, n_batch: int, lon=None, xyz=None, seed: int = 0, backend: str = "torch", device=None,
              dtype=torch.float32, state_dict: Optional[Mapping[str, torch.Tensor]] = None,
              reference_order_gradients: bool = True) -> "CycleGANTrainer":
        """The four networks, initialised on the host under ``torch.manual_seed(seed)`` as the reference's ``init_weights``
        leaves them (or loaded from ``state_dict``, keyed as ``CycleGANModule.state_dict()``), the two optimisers and the trainer.
        ``reference_order_gradients``: the twins pad tile by tile, so that a float64 step of the torch backend is the
        reference's bit for bit (``fit.cyclegan.set_reference_order_gradients``); off, they pad with the batched gathers, which
        is faster backwards and differs in the last bit of a gradient."""
        torch.manual_seed(seed)
        twins = {"generator_a_to_b": self.generator.build(n_state, nx, self.convolution_type, lon, xyz),
                 "generator_b_to_a": self.generator.build(n_state, nx, self.convolution_type, lon, xyz),
                 "discriminator_a": self.discriminator.build(n_state, nx, self.convolution_type, lon, xyz),
                 "discriminator_b": self.discriminator.build(n_state, nx, self.convolution_type, lon, xyz)}
        initialise_twins(twins, state_dict, reference_order_gradients)
        return CycleGANTrainer(twins, self, n_batch, n_state, nx, backend=backend, device=device, dtype=dtype)


@dataclasses.dataclass
class CycleGANTrainingConfig:
    """``CycleGANTrainingConfig`` (train_cyclegan.py:81-106); batching is in memory here whatever ``in_memory`` says, and
    ``shuffle_buffer_size`` and ``histogram_vmax`` are accepted so that a reference configuration parses."""

    n_epoch: int = 20
    shuffle_buffer_size: int = 10
    samples_per_batch: int = 1
    in_memory: bool = False
    histogram_vmax: float = 100.0
    checkpoint_path: Optional[str] = None
    scheduler: CycleGANSchedulerConfig = dataclasses.field(default_factory=CycleGANSchedulerConfig)

    def __post_init__(self):
        self.scheduler = _nested(self.scheduler, CycleGANSchedulerConfig, "scheduler")


@dataclasses.dataclass
class CycleGANHyperparameters:
    """``CycleGANHyperparameters`` (train_cyclegan.py:51-78)."""

    state_variables: List[str]
    normalization_fit_samples: int = 50_000
    network: CycleGANNetworkConfig = dataclasses.field(default_factory=CycleGANNetworkConfig)
    training: CycleGANTrainingConfig = dataclasses.field(default_factory=CycleGANTrainingConfig)
    reload_path: Optional[str] = None

    def __post_init__(self):
        self.network = _nested(self.network, CycleGANNetworkConfig, "network")
        self.training = _nested(self.training, CycleGANTrainingConfig, "training")

    @property
    def variables(self):
        return tuple(self.state_variables) + ("time",)


def initialise_twins(twins: Mapping[str, nn.Module], state_dict: Optional[Mapping[str, Any]], reference_order_gradients: bool) -> None:
    """The freshly built ``twins`` (name -> network) left as the reference's ``init_weights`` leaves them, one after the other in
    their order, or -- with ``state_dict`` -- each loaded from the entries under its name; then
    ``fit.cyclegan.set_reference_order_gradients`` on each."""
    if state_dict is None:
        for twin in twins.values():
            init_weights(twin)
    else:
        for key, twin in twins.items():
            twin.load_state_dict({k[len(key) + 1:]: torch.as_tensor(v) for k, v in state_dict.items() if k.startswith(key + ".")},
                                 strict=True)
    for twin in twins.values():
        set_reference_order_gradients(twin, reference_order_gradients)


def init_weights(net: nn.Module, init_gain: float = 0.02):
    """``init_weights`` (cyclegan_trainer.py:141-182) with its default "normal": N(0, 0.02) weights and zero biases on
    ``Conv2d`` only -- ``ConvTranspose2d`` keeps torch's default initialisation."""
    def init_func(module):
        if hasattr(module, "weight") and module.__class__.__name__ == "Conv2d":
            torch.nn.init.normal_(module.weight.data, 0.0, init_gain)
            if hasattr(module, "bias") and module.bias is not None:
                torch.nn.init.constant_(module.bias.data, 0.0)

    net.apply(init_func)


# ---------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------
class ImagePool:
    """``ImagePool`` (image_pool.py:10-72): a history of generated images with their times, drawn from with Python's
    ``random``."""

    def __init__(self, pool_size: int):
        self.pool_size = pool_size
        if self.pool_size > 0:
            self.num_imgs = 0
            self.images: List[torch.Tensor] = []
            self.times: List[torch.Tensor] = []

    def query(self, images: Tuple[torch.Tensor, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.pool_size == 0:
            return images
        return_times, return_images = [], []
        for time, image in zip(*images):
            time, image = torch.unsqueeze(time.data, 0), torch.unsqueeze(image.data, 0)
            if self.num_imgs < self.pool_size:
                self.num_imgs = self.num_imgs + 1
                self.times.append(time)
                self.images.append(image)
                return_times.append(time)
                return_images.append(image)
            else:
                p = random.uniform(0, 1)
                if p > 0.5:
                    random_id = random.randint(0, self.pool_size - 1)
                    tmp_time, tmp_img = self.times[random_id].clone(), self.images[random_id].clone()
                    self.times[random_id], self.images[random_id] = time, image
                    return_times.append(tmp_time)
                    return_images.append(tmp_img)
                else:
                    return_times.append(time)
                    return_images.append(image)
        return torch.cat(return_times, 0), torch.cat(return_images, 0)


def set_requires_grad(nets: Sequence[nn.Module], requires_grad: bool = False):
    for net in nets:
        for param in net.parameters():
            param.requires_grad = requires_grad


def unpack_state(state_a, state_b):
    """Folds the window dimension into the samples (cyclegan_trainer.py:847-868)."""
    fold = lambda t: t.reshape([t.shape[0] * t.shape[1]] + list(t.shape[2:]))   # noqa: E731
    return state_a[0].flatten(), state_b[0].flatten(), fold(state_a[1]), fold(state_b[1])


class TwinExports:
    """How a GAN trainer hands out its ``networks`` (name -> network of the backend, in the order of ``NETWORKS``; a name begins
    with ``generator`` or ``discriminator``) under the keys of its ``twins``.  A trainer sets ``NETWORKS`` and
    ``generator_state_dict(spec, convolution_type)``, which gives the spec of its HIP generator under the twin's keys."""

    def _export(self, key: str, what: str) -> Dict[str, torch.Tensor]:
        """One network's parameters (``what = "data"``) or gradients (``"grad"``) under its twin's keys, torch's layout, on the
        host; a parameter without a gradient is left out."""
        network, twin = self.networks[key], self.twins[key]
        if self.backend == "torch":
            pick = (lambda p: p.grad) if what == "grad" else (lambda p: p.data)
            return {name: pick(p).detach().cpu().clone() for name, p in network.named_parameters() if pick(p) is not None}
        holder = _grad_view(network) if what == "grad" else network
        if holder is None:
            return {}
        if key.startswith("generator"):
            return self.generator_state_dict(holder.to_spec(), self.config.convolution_type)
        return holder.twin_state_dict(twin)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """All parameters keyed as the reference module's ``state_dict()``."""
        return {f"{key}.{name}": t for key in self.NETWORKS for name, t in self._export(key, "data").items()}

    def gradients(self, stage: str) -> Dict[str, torch.Tensor]:
        """The gradients of the stage's networks as they stand, keyed as ``state_dict()``."""
        if stage not in ("generator", "discriminator"):
            raise ValueError(f"stage must be 'generator' or 'discriminator', got {stage!r}")
        return {f"{key}.{name}": t for key in self.NETWORKS if key.startswith(stage) for name, t in self._export(key, "grad").items()}


class CycleGANTrainer(TwinExports):
    """``CycleGANTrainer.train_on_batch`` (cyclegan_trainer.py:538-693), line for line, without the results aggregator.

    ``twins``: the four initialised plain-torch networks of ``n_state`` channels on faces of ``nx`` cells.  ``backend="torch"`` trains them as they are (on ``device``, in
    ``dtype``); ``backend="hip"`` trains ``HipGenerator`` / ``HipDiscriminator`` copies of them on the GPU.  A batch is a pair
    ``(time [sample, window] seconds since 1970, state [sample, window, tile, channel, x, y])`` per domain, on the host or on
    the device, as the reference lays it out, for both backends.  ``observer(stage)``, if given to ``train_on_batch``, is called
    after the backward pass of each stage (``"generator"``, ``"discriminator"``) and before its optimiser's step:
    ``gradients(stage)`` then holds that stage's gradients under the reference's ``state_dict`` keys, in torch's layout."""

    NETWORKS = ("generator_a_to_b", "generator_b_to_a", "discriminator_a", "discriminator_b")
    generator_state_dict = staticmethod(generator_state_dict)

    def __init__(self, twins: Mapping[str, nn.Module], config: CycleGANNetworkConfig, batch_size: int, n_state: int, nx: int,
                 backend: str = "torch", device=None, dtype=torch.float32):
        self.backend, self.config, self.batch_size = check_backend(backend), config, batch_size
        self.twins = dict(twins)
        if self.backend == "hip":
            from ..cube import cuda_device

            self.device, self.dtype = cuda_device(device or "cuda", "CycleGANTrainer(backend='hip')"), torch.float32
            halo = config.convolution_type
            self.networks = {}
            for key, twin in self.twins.items():
                if key.startswith("generator"):
                    spec = generator_spec_from_state_dict(
                        twin.state_dict(), n_state, nx, convolution_type=halo,
                        lon=None if not twin.use_geographic_features else twin.local_time_zero_radians[:, 0].numpy(),
                        xyz=None if not twin.use_geographic_features else twin.xyz.numpy(), **dataclasses.asdict(config.generator))
                    self.networks[key] = layers.HipGenerator(spec, halo).to(self.device)
                else:
                    self.networks[key] = HipDiscriminator(twin).to(self.device)
        else:
            self.device, self.dtype = torch.device(device or "cpu"), dtype
            self.networks = {key: twin.to(device=self.device, dtype=dtype) for key, twin in self.twins.items()}
        n = self.networks
        self.optimizer_generator = config.optimizer.instance(
            itertools.chain(n["generator_a_to_b"].parameters(), n["generator_b_to_a"].parameters()))
        self.optimizer_discriminator = config.optimizer.instance(
            itertools.chain(n["discriminator_a"].parameters(), n["discriminator_b"].parameters()))
        self.identity_loss, self.cycle_loss, self.gan_loss = (config.identity_loss.instance, config.cycle_loss.instance,
                                                              config.gan_loss.instance)
        self.identity_weight, self.cycle_weight = config.identity_weight, config.cycle_weight
        self.generator_weight, self.discriminator_weight = config.generator_weight, config.discriminator_weight
        self.target_real: Optional[torch.Tensor] = None
        self.target_fake: Optional[torch.Tensor] = None
        self.fake_a_buffer, self.fake_b_buffer = ImagePool(50), ImagePool(50)   # image pool size of 50 used by Zhu et al. (2017)

    # -- the batch as the backend's networks take it --------------------------------------------------
    def _prepare(self, state):
        time, data = state
        time, data = torch.as_tensor(time), torch.as_tensor(data)
        if self.backend == "hip":
            # the local-time offset is taken on the host in float32, as at predict time; activations are channel-last
            theta = torch.from_numpy(theta_from_seconds(time.detach().cpu().numpy().astype(np.float32)))
            return theta.to(self.device), data.to(device=self.device, dtype=torch.float32).movedim(3, -1).contiguous()
        return time.to(device=self.device, dtype=self.dtype), data.to(device=self.device, dtype=self.dtype)

    def train_on_batch(self, state_a, state_b, training: bool = True, observer: Optional[Callable[[str], None]] = None) -> Dict[str, float]:
        net = self.networks
        generator_a_to_b, generator_b_to_a = net["generator_a_to_b"], net["generator_b_to_a"]
        discriminator_a, discriminator_b = net["discriminator_a"], net["discriminator_b"]
        time_a, time_b, real_a, real_b = unpack_state(self._prepare(state_a), self._prepare(state_b))

        fake_b = generator_a_to_b(time_a, real_a)
        fake_a = generator_b_to_a(time_b, real_b)
        reconstructed_a = generator_b_to_a(time_a, fake_b)
        reconstructed_b = generator_a_to_b(time_b, fake_a)

        # Generators A2B and B2A: don't update discriminators when training generators to fool them
        if training:
            set_requires_grad([discriminator_a, discriminator_b], requires_grad=False)

        same_b = generator_a_to_b(time_b, real_b)
        loss_identity_b = self.identity_loss(same_b, real_b) * self.identity_weight
        same_a = generator_b_to_a(time_a, real_a)
        loss_identity_a = self.identity_loss(same_a, real_a) * self.identity_weight
        loss_identity = loss_identity_a + loss_identity_b

        pred_fake_b = discriminator_b(time_a, fake_b)
        if self.target_real is None or self.target_real.shape[0] < pred_fake_b.shape[0]:
            self.target_real = torch.ones(pred_fake_b.shape, dtype=pred_fake_b.dtype, device=pred_fake_b.device)
            self.target_fake = torch.zeros(pred_fake_b.shape, dtype=pred_fake_b.dtype, device=pred_fake_b.device)
        n_samples = pred_fake_b.shape[0]
        # last batch may have fewer samples, so we slice the target output 1/0's
        target_real, target_fake = self.target_real[:n_samples], self.target_fake[:n_samples]
        loss_gan_a_to_b = self.gan_loss(pred_fake_b, target_real) * self.generator_weight
        pred_fake_a = discriminator_a(time_b, fake_a)
        loss_gan_b_to_a = self.gan_loss(pred_fake_a, target_real) * self.generator_weight
        loss_gan = loss_gan_a_to_b + loss_gan_b_to_a

        loss_cycle_a_b_a = self.cycle_loss(reconstructed_a, real_a) * self.cycle_weight
        loss_cycle_b_a_b = self.cycle_loss(reconstructed_b, real_b) * self.cycle_weight
        loss_cycle = loss_cycle_a_b_a + loss_cycle_b_a_b

        loss_g = loss_identity + loss_gan + loss_cycle

        if training:
            self.optimizer_generator.zero_grad()
            loss_g.backward()
            if observer is not None:
                observer("generator")
            self.optimizer_generator.step()

        # Discriminators A and B: do update discriminators when training them to identify samples
        if training:
            set_requires_grad([discriminator_a, discriminator_b], requires_grad=True)

        pred_real = discriminator_a(time_a, real_a)
        loss_d_a_real = self.gan_loss(pred_real, target_real) * self.discriminator_weight
        if training:
            time_b, fake_a = self.fake_a_buffer.query((time_b.detach(), fake_a.detach()))
        pred_a_fake = discriminator_a(time_b, fake_a)
        loss_d_a_fake = self.gan_loss(pred_a_fake, target_fake) * self.discriminator_weight

        pred_real = discriminator_b(time_b, real_b)
        loss_d_b_real = self.gan_loss(pred_real, target_real) * self.discriminator_weight
        if training:
            time_a, fake_b = self.fake_b_buffer.query((time_a.detach(), fake_b.detach()))
        pred_b_fake = discriminator_b(time_a, fake_b)
        loss_d_b_fake = self.gan_loss(pred_b_fake, target_fake) * self.discriminator_weight

        loss_d = loss_d_b_real + loss_d_b_fake + loss_d_a_real + loss_d_a_fake
        if training:
            self.optimizer_discriminator.zero_grad()
            loss_d.backward()
            if observer is not None:
                observer("discriminator")
            self.optimizer_discriminator.step()

        return {
            "b_to_a_gan_loss": float((loss_gan_b_to_a).detach()),
            "a_to_b_gan_loss": float((loss_gan_a_to_b).detach()),
            "discriminator_a_loss": float((loss_d_a_fake + loss_d_a_real).detach()),
            "discriminator_b_loss": float((loss_d_b_fake + loss_d_b_real).detach()),
            "cycle_loss": float((loss_cycle).detach()),
            "identity_loss": float((loss_identity).detach()),
            "generator_loss": float((loss_g).detach()),
            "discriminator_loss": float((loss_d).detach()),
            "train_loss": float((loss_g + loss_d).detach()),
        }


def _grad_view(network: nn.Module) -> Optional[nn.Module]:
    """A shallow copy of a HIP network whose parameters are the gradients of the original's (None: there are none yet)."""
    import copy

    if any(p.grad is None for p in network.parameters()):
        return None
    view = copy.deepcopy(network)
    with torch.no_grad():
        for p, q in zip(view.parameters(), network.parameters()):
            p.copy_(q.grad)
    return view


# ---------------------------------------------------------------------------------------------
# the training function
# ---------------------------------------------------------------------------------------------
def _domain_arrays(batches, domain: int, names: Sequence[str]):
    """Every variable of one domain joined over the batches, ``[sample, time, tile, x, y(, z)]``, and the times ``[sample, time]``."""
    to_np = lambda a: np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)   # noqa: E731
    return ({name: np.concatenate([to_np(b[domain][name]) for b in batches], axis=0) for name in names},
            np.concatenate([to_np(b[domain]["time"]) for b in batches], axis=0))


def _normalised(arrays: Mapping[str, np.ndarray], names: Sequence[str], scalers) -> torch.Tensor:
    """``[sample, time, tile, channel, x, y]`` float32, the variables joined along the channels in the order of ``names``."""
    cols = []
    for name in names:
        mean, std = scalers[name]
        a = (np.asarray(arrays[name], np.float64) - mean) / std
        cols.append(a if a.ndim == 6 else a[..., None])
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(np.concatenate(cols, axis=-1), -1, 3).astype(np.float32)))


def flat_scaler_pairs(scalers: Mapping[str, Any]) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
    """name -> ``(mean, std)`` of fitted scalers as float64 vectors of one length, as the spec builders take them."""
    return {k: (np.asarray(m, np.float64).reshape(-1), np.broadcast_to(np.asarray(s, np.float64), np.shape(m)).reshape(-1).copy())
            for k, (m, s) in scalers.items()}


def train_cyclegan(hyperparameters: CycleGANHyperparameters, train_batches, validation_batches=None, device=None,
                   backend: Optional[str] = None, lon=None, xyz=None, seed: int = 0):
    """The reference's ``"cyclegan"`` training function (train_cyclegan.py:393-474) on in-memory batches.

    ``train_batches``: a sequence of pairs ``(mapping_a, mapping_b)``; each mapping has ``time`` ``[sample, time]`` (seconds
    since 1970) and every state variable as ``[sample, time, tile, x, y(, z)]``.  Per variable and domain a
    ``StandardScaler(n_sample_dims=5)`` is fitted on up to ``normalization_fit_samples`` samples; the time dimension is folded
    into the samples by the trainer; the samples are cut into batches of ``samples_per_batch`` once and the batches shuffled
    with ``random.shuffle`` between epochs; the schedulers step per epoch; ``checkpoint_path`` receives ``fit.dump`` of every
    epoch (``epoch_000`` ...).  ``reload_path``: an artifact written here *with* its discriminators, from whose parameters and
    scalers training resumes.  ``lon`` ``[6, nx, nx]`` / ``xyz`` ``[6, 3, nx, nx]``: the grid of the geographic features, data of
    the model here.  ``backend="torch"`` (the default) runs the twins under autograd on ``device``; ``"hip"`` runs the training
    kernels and needs the GPU.  Returns a ``HipCycleGAN`` that carries the discriminators and, as ``history``, the per-epoch
    mean of the nine losses (and ``val_*`` where validation batches are given)."""
    import os

    from . import io
    from .cyclegan import HipCycleGAN, cyclegan_spec_from_state_dict
    from .graph import fit_scalers

    hp = hyperparameters
    backend = "torch" if backend is None else backend
    names = [str(n) for n in hp.state_variables]
    if not train_batches:
        raise ValueError("train_cyclegan needs at least one batch")
    (arrays_a, time_a), (arrays_b, time_b) = _domain_arrays(train_batches, 0, names), _domain_arrays(train_batches, 1, names)
    state_dict = None
    if hp.reload_path is not None:
        reloaded = io.load(hp.reload_path)
        if not isinstance(reloaded, HipCycleGAN) or reloaded.discriminators is None:
            raise ValueError(f"{hp.reload_path} holds no CycleGAN with its discriminators: training cannot resume from it")
        from .cyclegan import state_dict_from_spec

        scalers = dict(reloaded.spec.scalers)
        state_dict = {**state_dict_from_spec(reloaded.spec), **{k: torch.from_numpy(v) for k, v in reloaded.discriminators["state_dict"].items()}}
        lon = reloaded.spec.generator_a_to_b.lon if lon is None else lon
        xyz = reloaded.spec.generator_a_to_b.xyz if xyz is None else xyz
    else:
        head = lambda arrays: {n: a[:hp.normalization_fit_samples] for n, a in arrays.items()}   # noqa: E731
        scalers = {f"{d}_{n}": v for d, arrays in (("a", arrays_a), ("b", arrays_b)) for n, v in fit_scalers(head(arrays)).items()}
    domain = lambda d: {n: scalers[f"{d}_{n}"] for n in names}   # noqa: E731
    real_a, real_b = _normalised(arrays_a, names, domain("a")), _normalised(arrays_b, names, domain("b"))
    n_state, nx = int(real_a.shape[3]), int(real_a.shape[-1])
    trainer = hp.network.build(n_state, nx, hp.training.samples_per_batch, lon, xyz, seed=seed, backend=backend, device=device,
                               state_dict=state_dict)
    schedulers = [hp.training.scheduler.instance(trainer.optimizer_generator), hp.training.scheduler.instance(trainer.optimizer_discriminator)]

    def cut(ta, ra, tb, rb):
        n, step = min(len(ra), len(rb)), hp.training.samples_per_batch
        return [((torch.as_tensor(ta[i:i + step]), ra[i:i + step]), (torch.as_tensor(tb[i:i + step]), rb[i:i + step])) for i in range(0, n, step)]

    batches = cut(time_a, real_a, time_b, real_b)
    validation = []
    if validation_batches:
        (va, vta), (vb, vtb) = _domain_arrays(validation_batches, 0, names), _domain_arrays(validation_batches, 1, names)
        validation = cut(vta, _normalised(va, names, domain("a")), vtb, _normalised(vb, names, domain("b")))

    def model():
        state = trainer.state_dict()
        spec = cyclegan_spec_from_state_dict(state, names, flat_scaler_pairs(scalers), nx, hp.network.convolution_type, lon, xyz,
                                             **dataclasses.asdict(hp.network.generator))
        config = dict(trainer.twins["discriminator_a"].config)
        out = HipCycleGAN(names, spec, {"config": config, "state_dict": {k: v for k, v in state.items() if k.startswith("discriminator")}})
        out.history = {k: list(v) for k, v in history.items()}
        return out

    history: Dict[str, List[float]] = {}
    mean = lambda rows, key: float(np.mean([r[key] for r in rows]))   # noqa: E731
    for epoch in range(hp.training.n_epoch):
        if epoch:
            random.shuffle(batches)
        rows = [trainer.train_on_batch(a, b) for a, b in batches]
        for key in LOSS_KEYS:
            history.setdefault(key, []).append(mean(rows, key))
        if validation:
            rows = [trainer.train_on_batch(a, b, training=False) for a, b in validation]
            for key in LOSS_KEYS:
                history.setdefault(f"val_{key}", []).append(mean(rows, key))
        for scheduler in schedulers:
            scheduler.step()
        if hp.training.checkpoint_path is not None:
            io.dump(model(), os.path.join(hp.training.checkpoint_path, f"epoch_{epoch:03d}"))
    return model()
