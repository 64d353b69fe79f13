"""``fit.train_convolutional_model(backend="hip")`` and ``conv_train.ConvTrainer`` end to end, on the tiny
network of tests/test_host_conv_train.py: six 8 x 8 tiles, three samples (18 tile-samples), ``field`` (4 levels) and ``surface``
in, ``tendency`` (3 levels) and ``flux`` out, 5 -> 8 -> 8 -> 3 + 1 with 3 x 3 kernels, batches of 4 tile-samples.

The gradient is compared with tests/conv_train_np.py within the contraction bounds composed through the layers
(``conv_train_np.step``, as ``train_np.step`` composes them).  How close the trained hip and torch losses are is measured and
printed, not gated."""
import functools

import numpy as np
import pytest
import torch

import conv_cases
import conv_np
import conv_train_np as C
import tolerances
from fv3net_amd import fit
from fv3net_amd.fit import conv as fit_conv
from fv3net_amd.xr_compat import DataArray, Dataset

pytestmark = pytest.mark.gpu

EPOCHS, LEARNING_RATE, BATCH = 4, 1e-2, 4   # the host test's


def hyperparameters(**kw):
    base = dict(filters=8, depth=3, kernel_size=3, epochs=EPOCHS, batch_size=BATCH, learning_rate=LEARNING_RATE)
    base.update(kw)
    return fit.ConvolutionalHyperparameters(list(C.TINY_INPUTS), list(C.TINY_OUTPUTS), **base)


def dataset():
    dims = {5: ["sample", "tile", "x", "y", "z"], 4: ["sample", "tile", "x", "y"]}
    return Dataset({name: DataArray(a, dims=dims[a.ndim]) for name, a in C.tiny_cube().items()})


@functools.lru_cache(maxsize=None)
def trained(backend, epochs=EPOCHS):
    return fit.train_convolutional_model(hyperparameters(epochs=epochs), [dataset()], backend=backend,
                                         device="cpu" if backend == "torch" else None)


def _bits(spec):
    meta, arrays = spec.to_arrays()
    return meta, {k: np.asarray(v).tobytes() for k, v in arrays.items()}


def _trainer(device):
    hp = hyperparameters()
    prep = fit_conv._prepare_conv_training(hp, [dataset()])
    return hp, prep, fit_conv.conv_trainer(hp, prep, torch.device(device))


def _flat(parts):
    """(hidden kernels, hidden biases, head kernels, head biases) -> [kernel, bias] per hidden layer, then the heads joined."""
    kernels, biases, out_k, out_b = parts
    return [x for kb in zip(kernels, biases) for x in kb] + [np.concatenate(out_k, axis=1), np.concatenate(out_b)]


def test_first_step_gradient_and_loss(device):
    hp, prep, trainer = _trainer(device)
    idx = np.array([3, 17, 0, 9])
    kernels, biases, out_k, out_b = trainer.parameters()
    trainer.backward(torch.from_numpy(idx).to(device))
    got = _flat(trainer.gradients())
    targets = np.concatenate([a.reshape(-1, a.shape[-1]) for a in prep.y], axis=1)
    grads, bounds, value, loss_bound = C.step(kernels, biases, out_k[0], out_b[0], prep.xin, targets, fit_conv.conv_mse_loss(prep), idx)
    want = [x for g in grads for x in g]
    gates = [x for b in bounds for x in b]
    names = ["dW0", "db0", "dW1", "db1", "dW heads", "db heads"]
    for name, g, w, gate in zip(names, got, want, gates):
        assert np.all(np.isfinite(g)) and np.any(w != 0)
        frac = float(np.max(np.abs(g.astype(np.float64) - w) / gate))
        print(f"first step {name}: {frac:.2e} of the composed gate")
        assert frac <= 1.0
    loss = trainer.loss()
    print(f"first step loss {loss:.9f} (float64 {value:.9f}): {abs(loss - value) / loss_bound:.2e} of the gate")
    assert abs(loss - value) <= loss_bound


def test_one_step_is_adam_then_the_constraint(device):
    """The update of the device's own gradient against float64 Adam and the constraint.  Gate, per element: the float32 update
    ``step_size * m / (sqrt(v) / bc2_sqrt + eps)`` goes through eleven roundings (three rounded constants, the fma of m, two
    products under the root counting half each, the root, two quotients, the sum with eps, the product with step_size), each
    at most 2^-24 of the update; the subtraction from the parameter adds half an ulp of the result.  A constrained element is
    the mean of two such values, and its sum rounds once more: half an ulp of the result."""
    hp, prep, trainer = _trainer(device)
    idx = torch.from_numpy(np.array([5, 5, 11, 2])).to(device)
    before = _flat(trainer.parameters())
    trainer.step(idx)
    grads, after = _flat(trainer.gradients()), _flat(trainer.parameters())
    zeros = [np.zeros_like(p, dtype=np.float64) for p in before]
    plain, _, _ = C.update(before, grads, zeros, zeros, 1, lr=LEARNING_RATE)
    want, _, _ = C.update(before, grads, zeros, zeros, 1, lr=LEARNING_RATE, constrained=(0, 2))
    half_ulp = lambda a: 0.5 * np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
    for i, (g, w, u, p0) in enumerate(zip(after, want, plain, before)):
        gate = 11 * C.U * np.abs(u - p0) + half_ulp(u)
        if i in (0, 2):
            gate = 0.5 * (gate + gate.transpose(1, 0, 2, 3)) + half_ulp(w)
        frac = float(np.max(np.abs(g.astype(np.float64) - w) / gate))
        print(f"one step, parameter array {i}: {frac:.3f} of the gate")
        assert frac <= 1.0 and not np.array_equal(g, before[i])
    for w in after[0], after[2]:
        assert np.array_equal(w.view(np.uint32), w.transpose(1, 0, 2, 3).view(np.uint32)), "hidden kernels are bitwise symmetric"
    assert not np.array_equal(before[0], before[0].transpose(1, 0, 2, 3))
    assert int(trainer.step_count.cpu()[0]) == 1


def test_three_replays_equal_three_eager_steps(device):
    batches = [np.array([0, 1, 2, 3]), np.array([17, 4, 4, 9]), np.array([8, 7, 6, 5]), np.array([16, 0, 12, 3])]
    _, _, eager = _trainer(device)
    losses = []
    for b in batches:
        eager.step(torch.from_numpy(b).to(device))
        losses.append(eager.loss())
    _, _, replayed = _trainer(device)
    idx = torch.from_numpy(batches[0]).to(device)
    graph = replayed.capture(idx)   # (takes the first step eagerly)
    assert int(replayed.step_count.cpu()[0]) == 1, "capturing runs nothing"
    for b, want in zip(batches[1:], losses[1:]):
        idx.copy_(torch.from_numpy(b))
        graph.replay()
        assert replayed.loss() == want
    assert int(replayed.step_count.cpu()[0]) == 4
    for a, b in zip(_flat(eager.parameters()), _flat(replayed.parameters())):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_a_short_last_batch_and_an_oversized_one(device):
    _, _, trainer = _trainer(device)
    trainer.step(torch.from_numpy(np.array([16, 17])).to(device))   # 18 tile-samples in batches of 4 end with 2
    assert np.isfinite(trainer.loss())
    with pytest.raises(ValueError, match="does not fit the buffers"):
        trainer.step(torch.arange(5, device=device))


def test_epochs_0_equals_the_torch_backend():
    assert _bits(trained("hip", 0).spec) == _bits(trained("torch", 0).spec)


def test_training_lowers_the_loss_like_the_torch_backend():
    cube = C.tiny_cube()
    start = C.evaluate_loss(trained("hip", 0).spec, cube)
    hip, twin = C.evaluate_loss(trained("hip").spec, cube), C.evaluate_loss(trained("torch").spec, cube)
    print(f"training loss after {EPOCHS} epochs at seed 0: start {start:.6f}, hip {hip:.6f}, torch (CPU) {twin:.6f}, "
          f"relative difference {abs(hip - twin) / twin:.2e}")
    assert hip < start
    for w in trained("hip").spec.hidden_kernels:
        assert np.array_equal(w.view(np.uint32), w.transpose(1, 0, 2, 3).view(np.uint32))


def test_same_seed_same_model():
    again = fit.train_convolutional_model(hyperparameters(), [dataset()], backend="hip")
    assert _bits(again.spec) == _bits(trained("hip").spec)


def test_the_trained_model_predicts_its_spec(device):
    model = trained("hip")
    assert isinstance(model, fit.HipConvolutionalModel) and model.n_halo == 2
    cube = C.tiny_cube()
    got = model.predict(dataset())
    ref = C.prepare([cube["field"], cube["surface"][..., None]], [cube["tendency"], cube["flux"][..., None]], 2, 30)
    padded = dict(zip(C.TINY_INPUTS, ref["X"]))
    truth = conv_np.forward(model.spec, padded)
    cpu32 = conv_cases.torch_chain(model.spec, {k: v.astype(np.float32) for k, v in padded.items()}, torch.float32)
    for name, dims in (("tendency", ["sample", "tile", "x", "y", "z"]), ("flux", ["sample", "tile", "x", "y"])):
        g = np.asarray(got[name].transpose(*dims).values)
        nf = 3 if name == "tendency" else 1
        tolerances.assert_close_per_level(g.reshape(-1, nf), truth[name].reshape(-1, nf), cpu32=cpu32[name].reshape(-1, nf), name=name)
