"""The plain-torch side of FMR training against the reference's own run (tests/golden/make_fmr_train_golden.py: the reference's
``FMRTrainer`` in float64 with the time fold and the direct-call ``checkpoint`` of DESIGN section 28), the configurations and
``train_fmr`` with the torch backend.  Nothing here needs a GPU."""
import os
import random

import numpy as np
import pytest
import torch

from fmr_train_cases import GOLDEN, fixture_config, grids, training_batches, training_hyperparameters, zero_gradient_biases

# the losses: ten times the worst relative deviation measured, floored at one float64 ulp (see
# test_torch_trainer_reproduces_two_reference_steps_in_float64)
GATE = 10 * 2.0 ** -52
PARAMETER_GATE = 1.6e-13   # of the tensor's max-norm, for the elements that have a gradient: ten times the 1.6e-14 measured
N_CLOCK = 2


def noise_only(key, shape):
    """The elements of parameter ``key`` whose gradient is mathematically zero: the whole of a convolution bias in front of an
    instance norm; in the ``.a`` step layers' weights the clock channels (the last two input channels) at the five taps that
    are no corner of the 3 x 3 kernel -- a corner tap of a face's corner cell reads a halo corner, which is zero, so its sum
    misses one cell and is live."""
    mask = np.zeros(shape, bool)
    if key in zero_gradient_biases([key]):
        mask[...] = True
    elif key.startswith("generator.resnet.") and ".conv_block.0.conv_block.0." in key and key.endswith("_wrapped.weight"):
        mask[:, -N_CLOCK:, 1, :] = True
        mask[:, -N_CLOCK:, :, 1] = True
    return mask


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def from_golden(golden, **kwargs):
    state0 = {k[len("state0."):]: torch.from_numpy(v) for k, v in golden.items() if k.startswith("state0.")}
    random.seed(int(golden["random_seed"]))
    return state0, fixture_config().build(3, 8, 2, golden["xyz"], golden["xyz_bottom"], state_dict=state0, **kwargs)


def test_torch_trainer_reproduces_two_reference_steps_in_float64(golden):
    """The six losses of both steps relative to themselves, and every parameter element after the second step relative to
    its tensor's max-norm.

    Measured: where the fixture was written, with 1, 4, 16 and 64 threads, the worst deviation is 0 for the twelve losses and 0
    for all 30 parameter tensors, bitwise equal, because the twins pad tile by tile in the reference's order
    (``reference_order_gradients``; with the batched padding the second step's losses were off by 3.2e-16).  On a second x86
    CPU model, whose float64 sums round in another order, the losses were within 3.2e-16 and the elements that have a gradient
    within 1.6e-14 of their tensor's max-norm.  The gates are ten times that: 10 x 3.2e-16, floored at ten float64 ulps =
    2.2e-15, for the losses, and ``PARAMETER_GATE`` = 1.6e-13 of the tensor's max-norm for every element that has a gradient.

    The elements whose gradient is mathematically zero cannot be gated relatively: what they receive is the rounding residue
    of a float64 sum, Adam divides it by its own size, and on the second CPU model they differed from the fixture by more
    than their own size (4.7e-11; they had moved 7.5e-11 from their start).  They are chosen by key and slice (``noise_only``): the 11 convolution biases in front
    of an instance norm, and in the ``.a`` step layers the weights of the two clock channels at the five non-corner taps: the
    clock is uniform over a face and its halo, so their gradient is a face sum of dy, zero behind the instance norm.  For them the test asserts what can be derived:
    the residue of a float64 sum of N = 2 x 4 x 6 x 8 x 8 = 3072 terms of size <= 1 is at most N 2^-53 = 3.4e-13; Adam's step
    lr m / (sqrt(v) + eps) for such a gradient is at most lr 3.4e-13 / eps; so two steps move such an element by at most
    B = 2 x 2e-4 x 3.4e-13 / 1e-8 = 1.4e-8 from where it started -- a live element moves by the order of lr = 2e-4 per step --
    in the reference's run and in this one, which therefore differ by at most 2 B."""
    from fv3net_amd.fit import fmr_train as ft

    state0, trainer = from_golden(golden, dtype=torch.float64)
    assert set(trainer.state_dict()) == set(state0) and all(torch.equal(v, state0[k]) for k, v in trainer.state_dict().items())
    worst_loss = 0.0
    for step in range(2):
        losses = trainer.train_on_batch(golden["real"][step])
        assert tuple(losses) == ft.LOSS_KEYS == tuple(golden["loss_keys"])
        for value, want in zip(losses.values(), golden["losses"][step]):
            worst_loss = max(worst_loss, abs(value - want) / abs(want))
    worst = {k: float(np.max(np.abs(v.numpy() - golden[f"state2.{k}"])) / np.max(np.abs(golden[f"state2.{k}"])))
             for k, v in trainer.state_dict().items()}
    print(f"worst relative deviation: losses {worst_loss:.1e}, parameters {max(worst.values()):.1e} over {len(worst)} tensors")
    assert worst_loss <= GATE, worst_loss
    bound = 2 * 2e-4 * (3072 * 2.0 ** -53) / 1e-8
    final = {k: v.numpy() for k, v in trainer.state_dict().items()}
    masks = {k: noise_only(k, v.shape) for k, v in final.items()}
    assert sum(m.all() for m in masks.values()) == 11 and sum(m.any() and not m.all() for m in masks.values()) == 2
    live, noise, moved = {}, {}, {}
    for k, got in final.items():
        want, start, mask = golden[f"state2.{k}"], golden[f"state0.{k}"], masks[k]
        diff = np.abs(got - want)
        live[k] = float(np.max(diff[~mask], initial=0.0) / np.max(np.abs(want)))
        noise[k] = float(np.max(diff[mask], initial=0.0))
        moved[k] = max(float(np.max(np.abs(run - start)[mask], initial=0.0)) for run in (got, want))
    print(f"worst deviation: elements with a gradient {max(live.values()):.1e} of the max-norm (gate {PARAMETER_GATE:.0e}); "
          f"noise-only elements {max(noise.values()):.1e}, moved by {max(moved.values()):.1e} (bound {bound:.1e})")
    assert not {k: v for k, v in live.items() if v > PARAMETER_GATE}
    assert not {k: v for k, v in moved.items() if v > bound}
    assert not {k: v for k, v in noise.items() if v > 2 * bound}
    key = "generator.out_conv.0.1._wrapped.weight"
    assert float(np.max(np.abs(final[key] - golden[f"state0.{key}"]))) > 1e-4, "a live parameter moves by the order of lr per step"


def test_the_trainer_folds_the_time_dimension_for_the_discriminator(golden):
    """A 6-D batch goes in; the discriminator sees ``[sample * time, tile, channel, x, y]``."""
    _, trainer = from_golden(golden, dtype=torch.float64)
    seen = []
    hook = trainer.networks["discriminator"].register_forward_hook(lambda mod, inp, out: seen.append((tuple(inp[1].shape), tuple(out.shape))))
    losses = trainer.train_on_batch(golden["real"][0], evaluate_only=True)
    hook.remove()
    assert seen == [((8, 6, 3, 8, 8), (8, 6, 1, 2, 2))] * 3      # fake, real, pooled fake
    assert all(np.isfinite(v) for v in losses.values())
    assert trainer.fake_buffer.num_imgs == 2                      # the pool is queried when evaluating too, window by window


def test_evaluating_changes_no_parameter(golden):
    state0, trainer = from_golden(golden, dtype=torch.float64)
    mean = trainer.evaluate_on_dataset([golden["real"][0], golden["real"][1][:1]])   # the second batch is smaller
    assert set(mean) == set(golden["loss_keys"]) and all(np.isfinite(v) for v in mean.values())
    assert all(torch.equal(v, state0[k]) for k, v in trainer.state_dict().items())


def test_refusals(golden):
    from fv3net_amd import fit
    from fv3net_amd.fit import fmr_train as ft

    _, trainer = from_golden(golden)
    with pytest.raises(ValueError, match="at least two times"):
        trainer.train_on_batch(golden["real"][0][:, :1])
    with pytest.raises(ValueError, match="must be \\[sample, time, tile, channel, x, y\\]"):
        trainer.train_on_batch(golden["real"][0][:, 0])
    with pytest.raises(ValueError, match="stage must be"):
        trainer.gradients("both")
    with pytest.raises(ValueError, match="no fields \\['n_resnets'\\]"):
        fixture_config(generator=dict(n_resnets=2))
    with pytest.raises(ValueError, match="no fields \\['use_geographic_features'\\]"):
        fixture_config(discriminator=dict(use_geographic_features=True))
    with pytest.raises(ValueError, match="no fields \\['cycle_loss'\\]"):
        ft.FMRHyperparameters(["a"], network=dict(cycle_loss=dict(loss_type="mse")))
    with pytest.raises(ValueError, match="no fields \\['epochs'\\]"):
        ft.FMRHyperparameters(["a"], training=dict(epochs=3))
    with pytest.raises(ValueError, match="loss_type must be 'mse' or 'mae', got 'huber'"):
        fixture_config(target_loss=dict(loss_type="huber"))
    with pytest.raises(ValueError, match="convolution_type wrapped_conv2d not supported"):
        fixture_config(convolution_type="wrapped_conv2d")
    with pytest.raises(ValueError, match="step_type must be"):
        fixture_config(generator=dict(step_type="lstm"))
    with pytest.raises(NotImplementedError, match="strided_kernel_size = 5"):
        fixture_config(discriminator=dict(n_convolutions=2, max_filters=8, strided_kernel_size=5)).build(3, 8, 2, *grids(8))
    with pytest.raises(ValueError, match="backend must be"):
        fixture_config().build(3, 8, 2, *grids(8), backend="triton")
    with pytest.raises(ValueError, match="needs xyz"):
        fixture_config().build(3, 8, 2)
    defaults = fit.FMRHyperparameters(["a"])
    assert (defaults.normalization_fit_samples, defaults.training.n_epoch, defaults.samples_per_batch) == (50_000, 20, 1)
    assert (defaults.training.shuffle_buffer_size, defaults.training.validation_batch_size, defaults.training.in_memory) == (10, None, False)
    network = defaults.network
    assert network.convolution_type == "conv2d" and network.generator_optimizer.name == network.discriminator_optimizer.name == "Adam"
    assert (network.identity_weight, network.target_weight, network.generator_weight, network.discriminator_weight) == (1.0, 1.0, 1.0, 1.0)
    assert network.reload_path is None and network.discriminator.strided_kernel_size == 3 and network.generator.strided_kernel_size == 4
    assert network.generator.samples_per_day is None and network.generator.step_type == "resnet" and defaults.variables == ("a",)


def test_both_backends_start_from_the_same_seeded_parameters():
    a, b, c = (fixture_config().build(3, 8, 2, *grids(8), seed=seed).state_dict() for seed in (5, 5, 6))
    assert all(torch.equal(a[k], b[k]) for k in a) and not all(torch.equal(a[k], c[k]) for k in a)


def same_files(a, b):
    import filecmp

    return sorted(os.listdir(a)) == sorted(os.listdir(b)) and all(filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False)
                                                                   for f in os.listdir(a))


def test_train_fmr_with_the_torch_backend(tmp_path, monkeypatch):
    from fv3net_amd import fit
    from fv3net_amd.fit import fmr_train as ft

    monkeypatch.chdir(tmp_path)     # the per-epoch dump goes under the working directory, as the reference's
    xyz, xyz_bottom = grids(12)
    batches = training_batches()
    random.seed(0)
    model = fit.train_fmr(training_hyperparameters(validation_batch_size=1), batches, batches[:1], xyz=xyz, xyz_bottom=xyz_bottom)
    assert isinstance(model, fit.HipFullModelReplacement)
    assert set(model.history) == set(ft.LOSS_KEYS) | {f"val_{k}" for k in ft.LOSS_KEYS}
    assert all(len(v) == 1 and np.isfinite(v[0]) for v in model.history.values())
    (epoch,) = os.listdir(tmp_path)
    assert epoch == f"model_epoch_0001_loss_{model.history['target_loss'][0]:0.4f}"
    # the artifact round-trips with its discriminator
    fit.dump(model, str(tmp_path / "a"))
    loaded = fit.load(str(tmp_path / "a"))
    fit.dump(loaded, str(tmp_path / "b"))
    assert same_files(tmp_path / "a", tmp_path / "b") and same_files(tmp_path / "a", tmp_path / epoch)
    assert len(loaded.discriminator["state_dict"]) == 8 and loaded.discriminator["config"]["strided_kernel_size"] == 3
    assert loaded.spec.generator.samples_per_day == 4 and loaded.spec.state_variables == ["air_temperature", "surface_pressure"]
    # an artifact without a discriminator loads, and is written byte for byte, as before
    golden_dir = os.path.join(os.path.dirname(GOLDEN), "fmr_reference", "halo_resnet")
    old = fit.load(golden_dir)
    assert old.discriminator is None
    fit.dump(old, str(tmp_path / "old"))
    assert all(same_bytes(os.path.join(golden_dir, f), tmp_path / "old" / f) for f in os.listdir(tmp_path / "old"))
    # reload_path resumes from bitwise-equal parameters and the same scalers
    resume = training_hyperparameters(network=fixture_config(reload_path=str(tmp_path / "a")))
    resume.training.n_epoch = 0
    resumed = fit.train_fmr(resume, batches)
    (_, a), (_, b) = model.spec.to_arrays(), resumed.spec.to_arrays()
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(np.array_equal(v, resumed.discriminator["state_dict"][k]) for k, v in model.discriminator["state_dict"].items())
    with pytest.raises(ValueError, match="holds no full-model replacement with its discriminator"):
        fit.train_fmr(training_hyperparameters(network=fixture_config(reload_path=golden_dir)), batches)


def same_bytes(a, b):
    import filecmp

    return filecmp.cmp(str(a), str(b), shallow=False)


def test_trained_model_predicts_after_a_round_trip(tmp_path, monkeypatch):
    """``train_fmr(backend="torch")`` -> dump -> load gives the predictor's spec: its twin rolls a window out (``predict``
    itself runs the kernels and is covered on the GPU)."""
    from fv3net_amd import fit

    monkeypatch.chdir(tmp_path)
    xyz, xyz_bottom = grids(12)
    batches = training_batches(n_batches=1)
    random.seed(0)
    model = fit.train_fmr(training_hyperparameters(shuffle_buffer_size=1), batches, xyz=xyz, xyz_bottom=xyz_bottom)
    fit.dump(model, str(tmp_path / "m"))
    loaded = fit.load(str(tmp_path / "m"))
    twin = fit.recurrent_twin_from_spec(loaded.spec.generator, loaded.spec.convolution_type)
    with torch.no_grad():
        out = twin(torch.zeros(1, 6, 3, 12, 12), 3)
    assert tuple(out.shape) == (1, 3, 6, 3, 12, 12) and bool(torch.all(torch.isfinite(out)))
