"""Writes ``fmr_train_reference.npz``: two consecutive ``FMRTrainer.train_on_batch`` steps of the reference's own trainer
(external/fv3fit/fv3fit/pytorch/recurrent/train_fmr.py:152-294) on the CPU in float64.

    python tests/golden/make_fmr_train_golden.py <path of the reference checkout>

Configuration: nx = 8; generator n_convolutions 2, n_resnet 2, max_filters 16, ``resnet`` steps, ``samples_per_day`` 4,
geographic features and both geographic biases (drawn non-zero once); discriminator n_convolutions 2, max_filters 8,
strided_kernel_size 3; ``halo_conv2d``; ``mae`` identity, ``mse`` target and GAN losses; weights identity 0.5, target 10,
generator 2, discriminator 0.5; Adam lr 2e-4 for both; batch 2, 4 times, 3 channels.  The networks are built by the reference's
``FMRNetworkConfig.build`` (so ``init_weights`` has run) and converted with ``.double()``.

Two things are done to the reference so that it runs and its gradient is the gradient of its loss:

  * ``train_on_batch`` hands the discriminator the 6-D ``[sample, time, tile, channel, x, y]`` tensor, which its convolutions
    refuse.  The stand-in for ``recurrent.reloadable.FullModelReplacement`` below hands the trainer a discriminator that folds
    the time dimension into the samples and reshapes the result back -- what the reference's own comment says it intends.
  * ``RecurrentGenerator.forward`` wraps every step in ``torch.utils.checkpoint``, whose recomputation advances the Python
    clock of ``DiurnalFeatures`` a second time.  The name ``checkpoint`` in the loaded ``generator`` module is replaced by a
    direct call.

The reference's modules are loaded from the checkout by path (``train_fmr.py``, ``generator.py``, ``discriminator.py``,
``shapes.py``, ``image_pool.py``, the ``cyclegan`` package's ``modules.py`` and ``cyclegan_trainer.init_weights``, ``loss.py``,
``optimizer.py``).  What they import and this machine lacks is stubbed as in ``make_cyclegan_train_golden.py``, plus
``tensorflow``, ``tensorflow_datasets``, ``fv3fit.tfdataset``, ``fv3fit._shared.hyperparameters``, ``fv3fit.pytorch.graph.train``
and ``fv3fit.pytorch.recurrent.reloadable`` (none of them is called here but the last).  Only data goes into the fixture:

    state0.<key>, state2.<key>   ``FMRModule.state_dict()`` before the first and after the second step (float64)
    xyz, xyz_bottom              the grids of the geographic features
    real                         ``[step, sample, time, tile, channel, x, y]``
    losses                       ``[step, 6]`` in the order of ``loss_keys``
    random_seed                  what Python's ``random`` was seeded with (the image pool draws from it once it is full)
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

NX, CHANNELS, BATCH, NTIME, STEPS, SEED = 8, 3, 2, 4, 2, 0
LOSS_KEYS = ("target_loss", "identity_loss", "gan_loss", "generator_loss", "discriminator_loss", "train_loss")


class FMRModule(torch.nn.Module):
    """Stand-in for ``reloadable.FMRModule``: the two networks under the reference's names."""

    def __init__(self, generator, discriminator):
        super().__init__()
        self.generator, self.discriminator = generator, discriminator


class FoldTime:
    """The discriminator on ``[sample * time, tile, channel, x, y]``, its output reshaped back."""

    def __init__(self, net):
        self.net = net

    def parameters(self):
        return self.net.parameters()

    def __call__(self, x):
        y = self.net(x.reshape(x.shape[0] * x.shape[1], *x.shape[2:]))
        return y.reshape(x.shape[0], x.shape[1], *y.shape[1:])


class FullModelReplacement:
    """Stand-in for ``reloadable.FullModelReplacement``: what ``FMRTrainer`` reads of it."""

    def __init__(self, model, scalers, state_variables):
        self.model, self.scalers, self.state_variables = model, scalers, state_variables

    @property
    def generator(self):
        return self.model.generator

    @property
    def discriminator(self):
        return FoldTime(self.model.discriminator)


def load_reference(reference: str):
    pytorch = os.path.join(reference, "external", "fv3fit", "fv3fit", "pytorch")
    register = lambda *args: (lambda obj: obj)   # noqa: E731
    tf = {"data": types.SimpleNamespace(Dataset=object), "Tensor": object}
    stubs = (("vcm", {}), ("vcm.grid", {"get_grid_xyz": lambda nx: synthetic_grid(nx)[0], "get_grid": lambda nx: synthetic_grid(nx)[1:]}),
             ("vcm.cubedsphere", {"to_cross": None}), ("fv3fit", {"wandb": types.SimpleNamespace(Image=object)}),
             ("fv3fit._shared", {"io": types.SimpleNamespace(register=register), "register_training_function": register}),
             ("fv3fit._shared.hyperparameters", {"Hyperparameters": object}),
             ("fv3fit._shared.predictor", {"Reloadable": object}),
             ("fv3fit._shared.scaler", {"StandardScaler": object, "get_standard_scaler_mapping": None, "get_mapping_standard_scale_func": None}),
             ("fv3fit.tfdataset", {"apply_to_mapping": None, "sequence_size": None, "ensure_nd": None}),
             ("fv3fit.pytorch", {}), ("fv3fit.pytorch.system", {"DEVICE": torch.device("cpu")}),
             ("fv3fit.pytorch.predict", {"_dump_pytorch": None, "_load_pytorch": None, "_unpack_tensor": None}),
             ("fv3fit.pytorch.graph", {}), ("fv3fit.pytorch.graph.train", {"get_Xy_map_fn": None}),
             ("fv3fit.pytorch.recurrent.reloadable", {"FMRModule": FMRModule, "FullModelReplacement": FullModelReplacement}),
             ("tensorflow", tf), ("tensorflow_datasets", {}),
             ("toolz", {"curry": curry}), ("xarray", {"Dataset": object, "DataArray": object}), ("cftime", {}), ("PIL", {}))
    for name, attrs in stubs:
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        mod.__path__ = []  # (a package, so that the dotted names below it import)
        mod.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)   # (torch looks optional modules up by spec)
        sys.modules.setdefault(name, mod)
    sys.modules.setdefault("matplotlib", None)
    sys.modules["fv3fit.pytorch"].__path__ = [pytorch]   # loss.py and optimizer.py are the reference's own (torch only)
    for sub in ("cyclegan", "recurrent"):      # empty shells: their __init__ is not run, their modules are found by path
        package = types.ModuleType(f"fv3fit.pytorch.{sub}")
        package.__path__ = [os.path.join(pytorch, sub)]
        sys.modules[package.__name__] = package
    train_fmr = importlib.import_module("fv3fit.pytorch.recurrent.train_fmr")
    generator = sys.modules["fv3fit.pytorch.recurrent.generator"]
    generator.checkpoint = lambda function, *args, **kwargs: function(*args, **kwargs)
    return train_fmr


def to_double(module):
    """``.double()`` converts parameters and buffers; the ``xyz`` tables are plain attributes."""
    module.double()
    for mod in module.modules():
        if type(mod).__name__ == "GeographicFeatures":
            mod.xyz = mod.xyz.double()


def main(reference: str):
    train_fmr = load_reference(reference)
    generator = sys.modules["fv3fit.pytorch.recurrent.generator"]
    discriminator = sys.modules["fv3fit.pytorch.recurrent.discriminator"]
    shapes = sys.modules["fv3fit.pytorch.recurrent.shapes"]
    loss, optimizer = sys.modules["fv3fit.pytorch.loss"], sys.modules["fv3fit.pytorch.optimizer"]
    torch.manual_seed(SEED)
    random.seed(SEED)
    rng = np.random.default_rng(SEED)
    config = train_fmr.FMRNetworkConfig(
        generator_optimizer=optimizer.OptimizerConfig("Adam", {"lr": 2e-4}),
        discriminator_optimizer=optimizer.OptimizerConfig("Adam", {"lr": 2e-4}),
        generator=generator.RecurrentGeneratorConfig(n_convolutions=2, n_resnet=2, max_filters=16, step_type="resnet", samples_per_day=4),
        discriminator=discriminator.DiscriminatorConfig(n_convolutions=2, max_filters=8, strided_kernel_size=3),
        convolution_type="halo_conv2d", identity_loss=loss.LossConfig("mae"), target_loss=loss.LossConfig("mse"),
        gan_loss=loss.LossConfig("mse"), identity_weight=0.5, target_weight=10.0, generator_weight=2.0, discriminator_weight=0.5)
    shape = shapes.RecurrentShape(nx=NX, ny=NX, n_state=CHANNELS, n_time=NTIME, n_batch=BATCH)
    trainer = config.build(shape, ["air_temperature", "surface_pressure"], {})
    module = trainer.fmr.model
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name in ("generator.input_bias.0.bias", "generator.output_bias.bias"):    # (they initialise to zero)
                p.normal_(0.0, 0.3)
    to_double(module)
    out = {f"state0.{k}": v.numpy().copy() for k, v in module.state_dict().items()}
    out["xyz"] = module.generator.input_bias[1].xyz.numpy().copy()
    out["xyz_bottom"] = module.generator.resnet[0].xyz.numpy().copy()
    out["real"] = rng.normal(0, 1, (STEPS, BATCH, NTIME, 6, CHANNELS, NX, NX))
    # the trainer would make its 1 / 0 targets float32 on first use, which autograd refuses beside float64 predictions
    with torch.no_grad():
        pred_shape = trainer.discriminator(torch.from_numpy(out["real"][0])).shape
    trainer.target_real, trainer.target_fake = torch.ones(pred_shape, dtype=torch.float64), torch.zeros(pred_shape, dtype=torch.float64)
    losses = []
    for step in range(STEPS):
        result = trainer.train_on_batch(torch.from_numpy(out["real"][step]))
        assert tuple(result) == LOSS_KEYS and all(np.isfinite(v) for v in result.values()), result
        losses.append([result[k] for k in LOSS_KEYS])
    out["losses"], out["loss_keys"], out["random_seed"] = np.array(losses, np.float64), np.array(LOSS_KEYS), np.array(SEED)
    out.update({f"state2.{k}": v.numpy().copy() for k, v in module.state_dict().items()})
    with open(os.path.join(HERE, "fmr_train_reference.npz"), "wb") as f:
        np.savez_compressed(f, **out)
    print(pred_shape, {k: v for k, v in zip(LOSS_KEYS, losses[-1])})


if __name__ == "__main__":
    main(sys.argv[1])
