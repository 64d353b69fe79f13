"""Writes ``cyclegan_train_reference.npz``: the reference's own ``Discriminator`` (pytorch/cyclegan/discriminator.py:68-169) and
two consecutive ``CycleGANTrainer.train_on_batch`` steps (cyclegan_trainer.py:538-693) on the CPU, with ``_compile = False`` and
the modules converted with ``.double()``.

    python tests/golden/make_cyclegan_train_golden.py <path of the reference checkout>

Configuration: nx = 12; generator n_convolutions 2, n_resnet 2, max_filters 12; discriminator n_convolutions 2, max_filters 8,
strided_kernel_size 3; ``halo_conv2d``; ``mae`` identity and cycle losses, ``mse`` GAN loss, weights 0.5 / 10 / 1 / 1; Adam
lr 2e-4; batch 2; two variables, 3 channels.  The networks are built by ``CycleGANNetworkConfig.build`` (so ``init_weights`` has
run: N(0, 0.02) on ``Conv2d``, torch's default on ``ConvTranspose2d``); the geographic biases of the generators and the
embedded biases of the discriminators are then drawn non-zero once.

The reference's modules are loaded from the checkout by path.  What they import and this machine lacks is stubbed: ``vcm.grid``
by the synthetic grid of ``make_cyclegan_golden.py``, ``fv3fit.pytorch.system.DEVICE`` by the CPU, ``toolz.curry`` by a
partial-application stand-in, ``fv3fit._shared`` (``io.register``, ``Reloadable``, ``StandardScaler``), ``fv3fit.pytorch.predict``,
``fv3fit.wandb``, ``xarray``, ``cftime``, ``PIL`` and ``vcm.cubedsphere`` by empty stand-ins (none of them is called here);
``fv3fit.pytorch.loss`` and ``.optimizer`` are the reference's own files.  Only data goes into the fixture:

    state0.<key>, state2.<key>   ``CycleGANModule.state_dict()`` before the first and after the second step (float64)
    lon, xyz                     the grid the geographic features were built from
    time_a, time_b, real_a, real_b   ``[step, sample, window]`` seconds and ``[step, sample, window, tile, channel, x, y]`` states
    disc.time, disc.state, disc.out_a, disc.out_b, disc.out32_a, disc.out32_b   the two discriminators on the first step's
                                 domain-a batch with the initial parameters, in float64 and (inputs and modules) in float32
    losses                       ``[step, 9]`` in the order of ``loss_keys``
"""
import importlib
import importlib.machinery
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_cyclegan_golden import curry, synthetic_grid   # noqa: E402

NX, CHANNELS, BATCH, STEPS = 12, 3, 2, 2
LOSS_KEYS = ("b_to_a_gan_loss", "a_to_b_gan_loss", "discriminator_a_loss", "discriminator_b_loss", "cycle_loss", "identity_loss",
             "generator_loss", "discriminator_loss", "train_loss")


def load_reference(reference: str):
    xyz, lon, lat = synthetic_grid(NX)
    register = lambda name: (lambda cls: cls)   # noqa: E731
    stubs = (("vcm", {}), ("vcm.grid", {"get_grid_xyz": lambda nx: xyz, "get_grid": lambda nx: (lon, lat)}),
             ("vcm.cubedsphere", {"to_cross": None}), ("fv3fit", {"wandb": types.SimpleNamespace(Image=object)}),
             ("fv3fit._shared", {"io": types.SimpleNamespace(register=register)}),
             ("fv3fit._shared.predictor", {"Reloadable": object}), ("fv3fit._shared.scaler", {"StandardScaler": object}),
             ("fv3fit.pytorch", {}), ("fv3fit.pytorch.system", {"DEVICE": torch.device("cpu")}),
             ("fv3fit.pytorch.predict", {"_dump_pytorch": None, "_load_pytorch": None, "_unpack_tensor": None}),
             ("toolz", {"curry": curry}), ("xarray", {"Dataset": object, "DataArray": object}), ("cftime", {}), ("PIL", {}))
    for name, attrs in stubs:
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        mod.__path__ = []  # (a package, so that the dotted names below it import)
        mod.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)   # (torch looks optional modules up by spec)
        sys.modules.setdefault(name, mod)
    sys.modules.setdefault("matplotlib", None)   # (plots are not made: the trainer's own `except ModuleNotFoundError` takes it)
    # loss.py and optimizer.py are the reference's own (torch only)
    sys.modules["fv3fit.pytorch"].__path__ = [os.path.join(reference, "external", "fv3fit", "fv3fit", "pytorch")]
    package = types.ModuleType("_reference_cyclegan")
    package.__path__ = [os.path.join(reference, "external", "fv3fit", "fv3fit", "pytorch", "cyclegan")]
    sys.modules["_reference_cyclegan"] = package
    return importlib.import_module("_reference_cyclegan.cyclegan_trainer")


def to_double(module):
    module.double()
    for net in (module.generator_a_to_b, module.generator_b_to_a, module.discriminator_a, module.discriminator_b):
        features = net._geographic_features
        features.xyz, features.local_time_zero_radians = features.xyz.double(), features.local_time_zero_radians.double()


def main(reference: str):
    trainer_module = load_reference(reference)
    generator = sys.modules["_reference_cyclegan.generator"]
    discriminator = sys.modules["_reference_cyclegan.discriminator"]
    loss, optimizer = sys.modules["fv3fit.pytorch.loss"], sys.modules["fv3fit.pytorch.optimizer"]
    torch.manual_seed(0)
    random.seed(0)
    rng = np.random.default_rng(0)
    config = trainer_module.CycleGANNetworkConfig(
        optimizer=optimizer.OptimizerConfig("Adam", {"lr": 2e-4}),
        generator=generator.GeneratorConfig(n_convolutions=2, n_resnet=2, max_filters=12),
        discriminator=discriminator.DiscriminatorConfig(n_convolutions=2, max_filters=8, strided_kernel_size=3,
                                                        use_geographic_embedded_bias=True),
        convolution_type="halo_conv2d", identity_loss=loss.LossConfig("mae"), cycle_loss=loss.LossConfig("mae"),
        gan_loss=loss.LossConfig("mse"), identity_weight=0.5, cycle_weight=10.0, generator_weight=1.0, discriminator_weight=1.0)
    trainer = config.build(CHANNELS, NX, NX, BATCH, ["air_temperature", "surface_pressure"], ({}, {}))
    trainer._compile = False
    module = trainer.cycle_gan.model
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("_input_bias.bias") or name.endswith("_output_bias.bias") or name.endswith("_sequential.1.bias"):
                p.normal_(0.0, 0.3)    # (they initialise to zero)
    seconds = lambda: 1.7e9 + 977 + 3600.0 * rng.integers(0, 48, (STEPS, BATCH, 1)).astype(np.float64)   # noqa: E731
    states = lambda: rng.normal(0, 1, (STEPS, BATCH, 1, 6, CHANNELS, NX, NX))                               # noqa: E731
    out = {"time_a": seconds(), "time_b": seconds(), "real_a": states(), "real_b": states()}
    time, state = torch.from_numpy(out["time_a"][0].reshape(-1)), torch.from_numpy(out["real_a"][0][:, 0])
    out["disc.time"], out["disc.state"] = time.numpy().copy(), state.numpy().copy()
    with torch.no_grad():   # float32 as built, then the same modules in float64
        out["disc.out32_a"] = module.discriminator_a(time.float(), state.float()).numpy().copy()
        out["disc.out32_b"] = module.discriminator_b(time.float(), state.float()).numpy().copy()
        to_double(module)
        out["disc.out_a"] = module.discriminator_a(time, state).numpy().copy()
        out["disc.out_b"] = module.discriminator_b(time, state).numpy().copy()
    out.update({f"state0.{k}": v.numpy().copy() for k, v in module.state_dict().items()})
    features = module.generator_a_to_b._geographic_features
    out["lon"], out["xyz"] = features.local_time_zero_radians[:, 0].numpy().copy(), features.xyz.numpy().copy()

    # the trainer would make its 1 / 0 targets float32 on first use, which autograd refuses beside float64 predictions
    trainer.target_real = torch.ones(out["disc.out_a"].shape, dtype=torch.float64)
    trainer.target_fake = torch.zeros(out["disc.out_a"].shape, dtype=torch.float64)
    losses = []
    for step in range(STEPS):
        batch = lambda d: (torch.from_numpy(out[f"time_{d}"][step]), torch.from_numpy(out[f"real_{d}"][step]))   # noqa: E731
        result = trainer.train_on_batch(batch("a"), batch("b"))
        losses.append([result[k] for k in LOSS_KEYS])
    out["losses"], out["loss_keys"] = np.array(losses, np.float64), np.array(LOSS_KEYS)
    out.update({f"state2.{k}": v.numpy().copy() for k, v in module.state_dict().items()})
    with open(os.path.join(HERE, "cyclegan_train_reference.npz"), "wb") as f:
        np.savez_compressed(f, **out)
    print({k: v for k, v in zip(LOSS_KEYS, losses[-1])})


if __name__ == "__main__":
    main(sys.argv[1])
