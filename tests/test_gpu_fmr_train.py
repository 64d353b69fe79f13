"""The FMR recurrent generator and its trainer on the training kernels, after ``test_gpu_cyclegan_train.py``
and with its gates.  The trainer runs the configuration of the reference fixture (tests/golden/make_fmr_train_golden.py:
generator 2 / 2 / 16 ``resnet`` with ``samples_per_day`` 4, discriminator 2 strided 3 x 3 levels / 8, ``halo_conv2d``, mae
identity, mse target and GAN losses, weights 0.5 / 10 / 2 / 0.5, Adam lr 2e-4) on batches of 2 windows of 3 times.

Gradients are compared at nx = 12 (3 x 3 faces at the bottom), not 8, for the reason given in ``test_gpu_cyclegan_train.py``: on
2 x 2 bottom faces the instance norm over four cells makes two float32 evaluations of the twin differ many-fold."""
import os
import random

import numpy as np
import pytest
import torch

import fmr_cases as fc
from fmr_train_cases import fixture_config, grids, training_batches, training_hyperparameters, zero_gradient_biases

pytestmark = pytest.mark.gpu

NX, CHANNELS, BATCH, NTIME = 12, 3, 2, 3


def batches(seed, steps=1):
    rng = np.random.default_rng(seed)
    real = rng.normal(0, 1, (steps, BATCH, NTIME, 6, CHANNELS, NX, NX)).astype(np.float32)
    return [torch.from_numpy(real[i]) for i in range(steps)]


def build(backend, device=None, dtype=torch.float32, seed=3):
    return fixture_config().build(CHANNELS, NX, BATCH, *grids(NX), seed=seed, backend=backend, device=device, dtype=dtype)


@pytest.mark.parametrize("convolution_type,step_type,bias,ntime", [("halo_conv2d", "resnet", True, 6), ("conv2d", "conv", False, 4)],
                         ids=["halo-resnet", "conv2d-conv"])
def test_training_generator_equals_the_predictor_bitwise(device, convolution_type, step_type, bias, ntime):
    """``HipRecurrentGenerator`` (materialised norm + activation, all times decoded in one batch) against
    ``RecurrentGeneratorModel.forward`` (the same float32 expressions in the next layer's loader, one decode per time), for the
    two configurations of the predictor's golden files: nx 8, 2 / 2 / 16, ``samples_per_day`` 4 (with 6 times the clock wraps)."""
    from fv3net_amd.fmr import RecurrentGeneratorModel
    from fv3net_amd.fmr_train import HipRecurrentGenerator

    rng = np.random.default_rng(11)
    spec = fc.make_generator(rng, CHANNELS, 8, 2, 2, 16, step_type=step_type, samples_per_day=4, bias=bias)
    state = torch.from_numpy(rng.normal(0, 1, (3, 6, 8, 8, CHANNELS)).astype(np.float32)).to(device)
    want = RecurrentGeneratorModel(spec, convolution_type, device).forward(state, ntime)
    net = HipRecurrentGenerator(spec, convolution_type).to(device)
    with torch.no_grad():
        got = net(state, ntime)
    assert tuple(got.shape) == tuple(want.shape) == (3, ntime, 6, 8, 8, CHANNELS)
    assert torch.equal(got, want), float((got - want).abs().max())
    back = net.to_spec()    # the two weight layouts hold the same numbers, the context rows included
    assert all(np.array_equal(back.weights[k], spec.weights[k]) and np.array_equal(back.biases[k], spec.biases[k]) for k in spec.weights)
    assert np.array_equal(back.xyz, spec.xyz) and np.array_equal(back.xyz_bottom, spec.xyz_bottom)
    assert (back.input_bias is None) == (not bias) and (not bias or np.array_equal(back.input_bias, spec.input_bias))


def masks(trainer, batch):
    """Every ReLU / leaky-ReLU input sign of one evaluation of a CPU twin trainer."""
    signs, hooks = [], []
    for net in trainer.networks.values():
        for m in net.modules():
            if isinstance(m, (torch.nn.ReLU, torch.nn.LeakyReLU)):
                hooks.append(m.register_forward_hook(lambda mod, inp, out: signs.append((inp[0] > 0).flatten())))
    trainer.train_on_batch(batch, evaluate_only=True)
    for h in hooks:
        h.remove()
    return torch.cat(signs)


def test_first_step_gradients_and_losses(device):
    """Both stages' first-step gradients of ``backend="hip"`` against the float64 twin on the CPU, with the float32 twin on the
    CPU as the yardstick: per parameter tensor with a live gradient |g_hip - g64|_2 <= 4 |g32 - g64|_2.  A convolution bias that
    feeds an instance norm has a mathematically zero gradient: finite and |db|_inf <= 1e-4 |dW|_2 of the same layer.  The six
    losses are within 1e-5 relative of the float64 twin's.

    Measured on the MI355X (seed 3, batch seed 21): the worst ratio over the 19 live tensors is 3.24, the 11 zero-gradient biases
    are at most 4.7e-8 of their layer's |dW|_2, the six losses within 1.6e-8 relative of float64 (the float32 twin: 6.6e-8)."""
    seed, batch = 3, batches(21)[0]
    grads, losses = {}, {}
    for name, kwargs in (("64", dict(backend="torch", dtype=torch.float64)), ("32", dict(backend="torch", dtype=torch.float32)),
                         ("hip", dict(backend="hip", device=device))):
        random.seed(0)
        trainer = build(seed=seed, **kwargs)
        if name == "64":
            mask64 = masks(trainer, batch)
        elif name == "32":
            assert torch.equal(masks(trainer, batch), mask64), "the float32 and float64 twins disagree on an activation mask: pick another seed"
        seen = {}
        losses[name] = trainer.train_on_batch(batch, observer=lambda stage: seen.update(trainer.gradients(stage)))
        grads[name] = {k: v.double().cpu() for k, v in seen.items()}
    assert set(grads["hip"]) == set(grads["64"]) == set(grads["32"]) and len(grads["64"]) == 30
    zero = zero_gradient_biases(grads["64"])
    assert len(zero) == 11
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
        # (the yardstick floored at one float32 rounding of the gradient, as in test_gpu_cyclegan_train.py)
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


def test_three_steps_are_bitwise_reproducible(device):
    runs = []
    for _ in range(2):
        random.seed(4)
        trainer = build("hip", device, seed=8)
        losses = [trainer.train_on_batch(b) for b in batches(5, steps=3)]
        runs.append((losses, trainer.state_dict()))
    assert runs[0][0] == runs[1][0]
    assert all(torch.equal(v, runs[1][1][k]) for k, v in runs[0][1].items())
    assert all(np.isfinite(v) for step in runs[0][0] for v in step.values())


def test_train_fmr_backends_agree_and_the_artifact_round_trips(device, tmp_path, monkeypatch):
    """One epoch of 2 batches with ``backend="hip"`` against ``backend="torch"`` on the same device from the same seeds: the
    epoch-mean losses agree to 1e-3 relative.  The hip backend's artifact round-trips with its discriminator, and ``predict`` of the
    reloaded artifact runs on a small dataset with the scalers that ``train_fmr`` fitted."""
    from fv3net_amd import fit

    monkeypatch.chdir(tmp_path)
    xyz, xyz_bottom = grids(NX)
    history, models = {}, {}
    for backend in ("torch", "hip"):
        random.seed(0)
        models[backend] = fit.train_fmr(training_hyperparameters(), training_batches(n_batches=2), device=device, backend=backend, xyz=xyz,
                                        xyz_bottom=xyz_bottom, seed=2)
        history[backend] = models[backend].history
    for key, (want,) in history["torch"].items():
        (got,) = history["hip"][key]
        print(f"{key}: torch {want:.6f} hip {got:.6f} rel {abs(got - want) / abs(want):.1e}")
        assert abs(got - want) <= 1e-3 * abs(want), key
    model = models["hip"]
    fit.dump(model, str(tmp_path / "a"))
    loaded = fit.load(str(tmp_path / "a"))
    fit.dump(loaded, str(tmp_path / "b"))
    import filecmp

    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b"))
    assert all(filecmp.cmp(tmp_path / "a" / f, tmp_path / "b" / f, shallow=False) for f in os.listdir(tmp_path / "a"))
    assert len(loaded.discriminator["state_dict"]) == 8
    assert all(np.array_equal(v, model.discriminator["state_dict"][k]) for k, v in loaded.discriminator["state_dict"].items())
    state = torch.zeros((1, 6, NX, NX, CHANNELS), device=device)
    out = loaded.step_model(state, 2)
    assert tuple(out.shape) == (1, 3, 6, NX, NX, CHANNELS) and bool(torch.all(torch.isfinite(out)))
    assert torch.equal(out, model.step_model(state, 2))
    # predict of the trained and reloaded artifact: the scalers that train_fmr fitted, pack, rollout, unpack
    from fv3net_amd.xr_compat import DataArray, Dataset

    raw = {name: np.asarray(a)[0] for name, a in training_batches(n_batches=1, seed=7)[0].items()}    # [time, tile, x, y(, z)]
    dims = ("time", "tile", "x", "y", "z")
    X = Dataset({name: DataArray(a, dims=dims[:a.ndim]) for name, a in raw.items()})
    predicted, reference = loaded.predict(X, 2)
    again, _ = model.predict(X, 2)
    for name, a in raw.items():
        got, ref = np.asarray(predicted[name].values), np.asarray(reference[name].values)
        assert got.shape == ref.shape == (1,) + a.shape and got.dtype == np.float64 and np.all(np.isfinite(got)), name
        # the reference is the input through (x - mean) / std in float32 and back: one float32 rounding of a value of a few std
        assert np.allclose(ref[0], a, rtol=1e-6, atol=0), name
        assert np.array_equal(got, np.asarray(again[name].values)), name
        # the generator was trained for two batches: its output is in the data's range, not the normalised one
        mean, std = loaded.spec.scalers[name]
        assert np.all(np.abs(got - mean) <= 20 * std), name
