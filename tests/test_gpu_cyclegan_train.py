"""The CycleGAN networks and trainer on the training kernels, at nx = 12 with the configuration of the reference fixture
(tests/golden/make_cyclegan_train_golden.py): generator 2 / 2 / 12, discriminator 2 strided 3 x 3 levels / 8, ``halo_conv2d``,
mae identity and cycle losses, mse GAN loss, weights 0.5 / 10 / 1 / 1, Adam lr 2e-4, batch 2, 3 channels.

Gradients are compared at nx = 12 (3 x 3 faces at the bottom), not 8: on 2 x 2 bottom faces the instance norm over four cells
makes two float32 evaluations of the twin differ 80-fold for one seed in three."""
import os
import random

import numpy as np
import pytest
import torch

import cyclegan_cases as cc
from cyclegan_train_cases import GOLDEN, fixture_config, training_batches, training_hyperparameters

pytestmark = pytest.mark.gpu

NX, CHANNELS, BATCH = 12, 3, 2


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def batches(seed, steps=1):
    rng = np.random.default_rng(seed)
    # seconds as the float32 the reference's loader makes of them, so that every dtype sees the same local time
    seconds = lambda: (1.7e9 + 977 + 3600.0 * rng.integers(0, 48, (steps, BATCH, 1))).astype(np.float32).astype(np.float64)   # noqa: E731
    states = lambda: rng.normal(0, 1, (steps, BATCH, 1, 6, CHANNELS, NX, NX)).astype(np.float32)           # noqa: E731
    ta, tb, ra, rb = seconds(), seconds(), states(), states()
    return [((torch.from_numpy(ta[i]), torch.from_numpy(ra[i])), (torch.from_numpy(tb[i]), torch.from_numpy(rb[i]))) for i in range(steps)]


def build(golden, backend, device=None, dtype=torch.float32, seed=3):
    return fixture_config().build(CHANNELS, NX, BATCH, golden["lon"], golden["xyz"], seed=seed, backend=backend, device=device, dtype=dtype)


@pytest.mark.parametrize("embedded", [False, True], ids=["plain", "embedded-bias"])
def test_training_generator_equals_the_predictor_bitwise(device, embedded):
    """``HipGenerator`` (the training layers: materialised norm + activation) against ``GeneratorModel.forward`` (the predictor:
    the same float32 expression in the next layer's loader), both directions of a CycleGAN spec."""
    from fv3net_amd.cyclegan import GeneratorModel, theta_from_seconds
    from fv3net_amd.cyclegan_train import HipGenerator

    rng = np.random.default_rng(11)
    spec = cc.make_spec(rng, {"air_temperature": 2, "surface_pressure": 1}, NX, 2, 2, 12, embedded=embedded)
    state = torch.from_numpy(rng.normal(0, 1, (3, 6, NX, NX, CHANNELS)).astype(np.float32)).to(device)
    theta = torch.from_numpy(theta_from_seconds(np.float32(1.7e9) + np.float32(3600) * np.arange(3, dtype=np.float32))).to(device)
    for reverse in (False, True):
        g = spec.generator(reverse)
        want = GeneratorModel(g, spec.convolution_type, device).forward(state, theta)
        net = HipGenerator(g, spec.convolution_type).to(device)
        with torch.no_grad():
            got = net(theta, state)
        assert torch.equal(got, want), (reverse, float((got - want).abs().max()))
        back = net.to_spec()    # the two weight layouts hold the same numbers
        assert all(np.array_equal(back.weights[k], g.weights[k]) and np.array_equal(back.biases[k], g.biases[k]) for k in g.weights)
        assert np.array_equal(back.input_bias, g.input_bias) and np.array_equal(back.xyz, g.xyz)


def zero_gradient_biases(keys):
    """The convolution biases that feed an instance norm: every generator convolution bias but the output layer's, every
    discriminator's but the first and the patch-output layers'."""
    out = set()
    for k in keys:
        if not k.endswith("_wrapped.bias"):
            continue
        net, rest = k.split(".", 1)
        first_or_patch = rest.startswith("_sequential.0.") or rest.startswith("_sequential.5.")
        if (net.startswith("generator") and not rest.startswith("_main.2.")) or (net.startswith("discriminator") and not first_or_patch):
            out.add(k)
    return out


def masks(trainer, batch):
    """Every ReLU / leaky-ReLU input sign of one generator-stage forward of a CPU twin trainer."""
    signs, hooks = [], []
    for net in trainer.networks.values():
        for m in net.modules():
            if isinstance(m, (torch.nn.ReLU, torch.nn.LeakyReLU)):
                hooks.append(m.register_forward_hook(lambda mod, inp, out: signs.append((inp[0] > 0).flatten())))
    trainer.train_on_batch(*batch, training=False)
    for h in hooks:
        h.remove()
    return torch.cat(signs)


def test_first_step_gradients_and_losses(device, golden):
    """Both stages' first-step gradients of ``backend="hip"`` against the float64 twin on the CPU, with the float32 twin on the
    CPU as the yardstick: per parameter tensor with a live gradient |g_hip - g64|_2 <= 4 |g32 - g64|_2.  A convolution bias that
    feeds an instance norm has a mathematically zero gradient: finite and |db|_inf <= 1e-4 |dW|_2 of the same layer.  The nine
    losses are within 1e-5 relative of the float64 twin's.

    Measured on the MI355X (seed 3, batch seed 21): the worst ratio over the 40 live tensors is 2.15, the 22 zero-gradient biases
    are at most 8.9e-8 of their layer's |dW|_2, the nine losses within 7.6e-8 relative of float64.  The two one-element bias
    gradients of the discriminators' patch-output layers are what the float64 sum of db is for: as the ones row of the
    weight-gradient MFMA (a sequential float32 sum) they were two to four ulp off and missed this gate."""
    seed, batch = 3, batches(21)[0]
    grads, losses = {}, {}
    for name, kwargs in (("64", dict(backend="torch", dtype=torch.float64)), ("32", dict(backend="torch", dtype=torch.float32)),
                         ("hip", dict(backend="hip", device=device))):
        random.seed(0)
        trainer = build(golden, seed=seed, **kwargs)
        if name != "hip":
            if name == "64":
                mask64 = masks(trainer, batch)
            else:
                assert torch.equal(masks(trainer, batch), mask64), "the float32 and float64 twins disagree on an activation mask: pick another seed"
        seen = {}
        losses[name] = trainer.train_on_batch(*batch, observer=lambda stage: seen.update(trainer.gradients(stage)))
        grads[name] = {k: v.double().cpu() for k, v in seen.items()}
    assert set(grads["hip"]) == set(grads["64"]) == set(grads["32"]) and len(grads["64"]) == 62
    zero = zero_gradient_biases(grads["64"])
    assert len(zero) == 22
    worst, worst_bias, missed = 0.0, 0.0, {}
    for key, g64 in grads["64"].items():
        hip, g32 = grads["hip"][key], grads["32"][key]
        assert torch.all(torch.isfinite(hip)), key
        if key in zero:
            dw = grads["hip"][key[:-len("bias")] + "weight"]
            ratio = float(hip.abs().max() / dw.norm())
            worst_bias = max(worst_bias, ratio)
            assert ratio <= 1e-4, (key, ratio)
            continue
        assert float(g64.norm()) > 0, key
        # (the yardstick floored at one float32 rounding of the gradient, so that a twin that happens to equal float64 neither
        # divides by zero nor asks for more than the format holds)
        err, yard = float((hip - g64).norm()), max(float((g32 - g64).norm()), 2.0 ** -24 * float(g64.norm()))
        worst = max(worst, err / yard)
        if not err <= 4 * yard:
            missed[key] = (round(err / yard, 2), yard / float(g64.norm()), tuple(g64.shape))
    print(f"worst |g_hip - g64| / |g32 - g64| over the live tensors: {worst:.2f}; worst |db|_inf / |dW|_2 of a zero-gradient bias: {worst_bias:.1e}")
    assert not missed, missed    # tensor -> (ratio, relative error of the float32 twin, shape)
    for key, want in losses["64"].items():
        err, yard = abs(losses["hip"][key] - want) / abs(want), abs(losses["32"][key] - want) / abs(want)
        print(f"{key}: hip {err:.1e}, float32 twin {yard:.1e}")
        assert err <= 1e-5, (key, err, yard)


def test_three_steps_are_bitwise_reproducible(device, golden):
    runs = []
    for _ in range(2):
        random.seed(4)
        trainer = build(golden, "hip", device, seed=8)
        losses = [trainer.train_on_batch(*b) for b in batches(5, steps=3)]
        runs.append((losses, trainer.state_dict()))
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(v, runs[1][1][k]) for k, v in runs[0][1].items())
    assert all(np.isfinite(v) for step in runs[0][0] for v in step.values())


def test_train_cyclegan_backends_agree(device):
    """One epoch of 3 batches with ``backend="hip"`` against ``backend="torch"`` on the same device from the same seeds: the
    epoch-mean losses agree to 1e-3 relative."""
    from fv3net_amd import fit

    lon, xyz = cc.synthetic_grid(NX)
    history = {}
    for backend in ("torch", "hip"):
        random.seed(0)
        model = fit.train_cyclegan(training_hyperparameters(), training_batches(), device=device, backend=backend, lon=lon, xyz=xyz, seed=2)
        history[backend] = model.history
    for key, (want,) in history["torch"].items():
        (got,) = history["hip"][key]
        print(f"{key}: torch {want:.6f} hip {got:.6f} rel {abs(got - want) / abs(want):.1e}")
        assert abs(got - want) <= 1e-3 * abs(want), key
