"""The configuration and batches of the FMR training tests: the reference fixture's (tests/golden/make_fmr_train_golden.py)."""
import os

import numpy as np

import fmr_cases as fc
from fv3net_amd.fit import fmr_train as ft

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fmr_train_reference.npz")


def fixture_config(**changes):
    """Generator 2 / 2 / 16 ``resnet`` with ``samples_per_day`` 4, discriminator 2 strided 3 x 3 levels / 8, ``halo_conv2d``, mae
    identity, mse target and GAN losses, weights 0.5 / 10 / 2 / 0.5, Adam lr 2e-4."""
    fields = dict(generator_optimizer=dict(name="Adam", kwargs=dict(lr=2e-4)), discriminator_optimizer=dict(name="Adam", kwargs=dict(lr=2e-4)),
                  generator=dict(n_convolutions=2, n_resnet=2, max_filters=16, step_type="resnet", samples_per_day=4),
                  discriminator=dict(n_convolutions=2, max_filters=8, strided_kernel_size=3), convolution_type="halo_conv2d",
                  identity_loss=dict(loss_type="mae"), target_loss=dict(loss_type="mse"), gan_loss=dict(loss_type="mse"),
                  identity_weight=0.5, target_weight=10.0, generator_weight=2.0, discriminator_weight=0.5)
    fields.update(changes)
    return ft.FMRNetworkConfig(**fields)


def grids(nx, n_convolutions=2):
    return fc.grid_xyz(nx), fc.grid_xyz(nx >> n_convolutions)


def training_batches(n_batches=3, samples=2, ntime=3, nx=12, seed=0):
    """Mappings of raw fields: a 2-level and a 1-level variable, ``[sample, time, tile, x, y(, z)]``."""
    rng = np.random.default_rng(seed)
    return [{"air_temperature": 250 + 10 * rng.normal(0, 1, (samples, ntime, 6, nx, nx, 2)),
             "surface_pressure": 1e5 + 1e3 * rng.normal(0, 1, (samples, ntime, 6, nx, nx))} for _ in range(n_batches)]


def training_hyperparameters(network=None, **training):
    return ft.FMRHyperparameters(["air_temperature", "surface_pressure"], network=network or fixture_config(),
                                 training=dict(n_epoch=1, samples_per_batch=2, **training))


def zero_gradient_biases(keys):
    """The convolution biases that feed an instance norm, whose gradient is mathematically zero: every generator convolution
    bias but the output layer's, the discriminator's but the first and the patch-output layers' (two strided levels)."""
    out = set()
    for k in keys:
        if not k.endswith("_wrapped.bias"):
            continue
        net, rest = k.split(".", 1)
        if (net == "generator" and not rest.startswith("out_conv.")) or \
                (net == "discriminator" and not (rest.startswith("_sequential.0.") or rest.startswith("_sequential.4."))):
            out.add(k)
    return out
