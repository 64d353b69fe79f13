"""``fit.train_precipitative_model(backend="hip")`` and ``HipPrecipitativeModel.input_sensitivity`` end to end (DESIGN.md section
25), as tests/test_gpu_train_dense.py does for the dense model.

Data: 2 048 synthetic columns (tests/precip_train_cases.py) -- T, q, delp on 79 levels and physics_precip in, dQ1, dQ2 and
total_precipitation_rate out (238 -> 8 -> 8 -> 3 x 79), the targets a fixed smooth function of the inputs.  Width 8, depth 3,
batch 512.  The gradient and the Jacobian are compared with tests/precip_train_np.py within the bounds composed through the layers;
the trained loss is judged by the torch backend's own spread over seeds."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import precip_train_cases as C
import precip_train_np as PT
import precipitative_cases as PC
import precipitative_np as P
import train_np as T
from fv3net_amd import fit
from fv3net_amd.fit import precipitative as fp
from fv3net_amd.xr_compat import DataArray, Dataset
from tolerances import assert_close_per_level

pytestmark = pytest.mark.gpu

NZ = 79
CLIP = {C.T_NAME: slice(10, NZ)}


def hyper(**kw):
    args = dict(width=8, depth=3, epochs=3, batch_size=512, learning_rate=1e-2, seed=0)
    args.update(kw)
    return fit.PrecipitativeHyperparameters(**args)


def sources():
    return {n: C.columns(n) for n in C.INPUTS}


def training_loss(model):
    """Sum over the three outputs of mean(((prediction - target) / std) ** 2) over all 2 048 columns, in float64."""
    out = P.forward(model.spec, model.couple_precip_to_dQ1_dQ2, sources(), dtype=np.float64)
    total = 0.0
    for name in C.OUTPUTS:
        y = C.columns(name).astype(np.float64)
        pred = out[name].reshape(y.shape)
        total += np.mean(((pred - y) / np.maximum(y.std(axis=0), 1e-12)) ** 2)
    return float(total)


def same_spec(a, b):
    (ma, aa), (mb, ab) = a.to_arrays(), b.to_arrays()
    return ma == mb and aa.keys() == ab.keys() and all(np.array_equal(aa[k], ab[k]) for k in aa)


@functools.lru_cache(maxsize=None)
def hip_model():
    return fit.train_precipitative_model(hyper(), C.batches(), backend="hip")


@pytest.mark.parametrize("regularizer", [None, ("l2", {"l2": 0.01})], ids=["plain", "l2"])
def test_epochs_0_equals_the_torch_backend(regularizer):
    hp = hyper(epochs=0, residual_regularizer=regularizer)
    hip = fit.train_precipitative_model(hp, C.batches(), backend="hip")
    ref = fit.train_precipitative_model(hp, C.batches(), backend="torch", device="cpu")
    assert same_spec(hip.spec, ref.spec)
    assert [o.name for o in hip.spec.outputs] == list(fp.HEAD_NAMES) and hip.spec.out_kernel.shape[1] == 3 * NZ, "no dead head is exported"


@pytest.mark.parametrize("couple,regularizer", [(True, None), (False, None), (True, ("l2", {"l2": 0.01}))], ids=["coupled", "uncoupled", "coupled-l2"])
def test_first_step_gradient(device, couple, regularizer):
    """The gradient of the first minibatch, read from the trainer's buffer, with clipped air_temperature levels."""
    hp = hyper(clip=CLIP, couple_precip_to_dQ1_dQ2=couple, residual_regularizer=regularizer)
    prep = fp._prepare_precipitative_training(hp, C.batches())
    trainer = fp.precipitative_trainer(hp, prep, device)
    idx = torch.randperm(prep.xin.shape[0], generator=torch.Generator().manual_seed(0))[:512]
    trainer.backward(idx.to(device))
    got_k, got_b, got_ok, got_ob = trainer.gradients()
    kernels, biases, out_k, out_b = trainer.parameters()
    has_dead = regularizer is not None
    assert out_k[0].shape == (8, 3 * NZ + int(has_dead)) and prep.xin.shape[1] == 3 * NZ + 1 - 10
    loss = fp.precipitative_loss(hp, prep)
    grads, bounds, value, value_gate = PT.step(kernels + out_k, biases + out_b, prep.xin, prep.delp, prep.physics_precip, prep.y, loss,
                                               idx.numpy())
    worst = 0.0
    for l, (gw, gb) in enumerate(zip(got_k + got_ok, got_b + got_ob)):
        for got, want, gate in ((gw, grads[l][0], bounds[l][0]), (gb, grads[l][1], bounds[l][1])):
            assert np.all(np.isfinite(got))
            frac = float(np.max(np.abs(got - want) / gate))
            rel = float(np.max(gate) / max(np.max(np.abs(want)), 1e-300))
            print(f"layer {l}: {frac:.3f} of the gate (the gate is {rel:.1e} of the largest gradient)")
            worst = max(worst, frac)
    assert worst <= 1.0
    print(f"loss {trainer.loss()} vs {value}: {abs(trainer.loss() - value) / value_gate:.3f} of its gate")
    assert abs(trainer.loss() - value) <= value_gate
    # the composed gates are wide (worst-case forward bounds through the coupling and the integral: see DESIGN section 25), so
    # check that they still tell this graph from the one with the coupling switched
    other, _, _, _ = PT.step(kernels + out_k, biases + out_b, prep.xin, prep.delp, prep.physics_precip, prep.y,
                             dataclasses.replace(loss, couple=not couple), idx.numpy())
    apart = float(np.max(np.abs(other[-1][0] - grads[-1][0]) / bounds[-1][0]))
    print(f"the head layer's gradient with the coupling switched lies {apart:.0f} gates away")
    assert apart > 1
    cp0 = 2 * NZ + int(has_dead)
    assert np.any(got_ok[0][:, cp0:] != 0) and np.any(got_ok[0][:, :NZ] != 0)
    if has_dead:
        assert np.all(got_ok[0][:, 2 * NZ] != 0) and got_ob[0][2 * NZ] != 0, "the regulariser reaches the dead head"
        exported = fit.train_precipitative_model(hyper(epochs=1, residual_regularizer=regularizer), C.batches(), backend="hip")
    else:
        exported = hip_model()
    assert [o.name for o in exported.spec.outputs] == list(fp.HEAD_NAMES) and exported.spec.out_kernel.shape[1] == 3 * NZ


def test_three_epochs_train_like_the_torch_backend():
    start = training_loss(fit.train_precipitative_model(hyper(epochs=0), C.batches(), backend="torch", device="cpu"))
    torch_losses = [training_loss(fit.train_precipitative_model(hyper(seed=s), C.batches(), backend="torch", device="cpu")) for s in range(5)]
    hip = training_loss(hip_model())
    width = max(torch_losses) - min(torch_losses)
    print(f"loss at epochs=0 {start:.6f}; torch seeds 0-4 {[round(v, 6) for v in torch_losses]}; hip seed 0 {hip:.6f}")
    assert hip < start
    assert min(torch_losses) - width <= hip <= max(torch_losses) + width


def test_same_seed_same_model():
    again = fit.train_precipitative_model(hyper(), C.batches(), backend="hip")
    assert same_spec(again.spec, hip_model().spec)


def test_captured_step_equals_eager_steps(device):
    hp = hyper(residual_regularizer=("l1_l2", {}))
    prep = fp._prepare_precipitative_training(hp, C.batches())
    perm = torch.randperm(prep.xin.shape[0], generator=torch.Generator().manual_seed(1)).to(device)
    batches = [perm[i:i + 512] for i in range(0, 4 * 512, 512)]
    eager = fp.precipitative_trainer(hp, prep, device)
    for b in batches:
        eager.step(b)
    replayed = fp.precipitative_trainer(hp, prep, device)
    idx = batches[0].clone()
    graph = replayed.capture(idx)   # (takes the first step eagerly)
    for b in batches[1:]:
        idx.copy_(b)
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(replayed.params, eager.params) and torch.equal(replayed.m, eager.m) and torch.equal(replayed.v, eager.v)
    assert int(replayed.step_count.cpu()[0]) == 4 and replayed.loss() == eager.loss()
    assert not torch.equal(eager.params, fp.precipitative_trainer(hp, prep, device).params)


def test_artifact_round_trip(tmp_path):
    model = hip_model()
    ds = C.batches()[0]
    out = model.predict(ds)
    src = sources()
    truth = P.forward(model.spec, True, src, dtype=np.float64)
    cpu32 = P.forward(model.spec, True, src, dtype=np.float32)
    for name in ("dQ1", "dQ2"):
        got = out[name].values.reshape(NZ, -1).T
        assert_close_per_level(got, truth[name], cpu32=cpu32[name], name=name)
    PC.assert_precip_gate(out[P.PRECIP].values.reshape(-1), truth[P.PRECIP], cpu32[P.PRECIP], {k: v if v.shape[1] > 1 else v[:, 0] for k, v in src.items()},
                          truth[P.COL_PRECIP], name="trained model")
    fit.dump(model, str(tmp_path / "m"))
    loaded = fit.load(str(tmp_path / "m"))
    assert isinstance(loaded, fit.HipPrecipitativeModel) and same_spec(loaded.spec, model.spec)
    assert loaded.couple_precip_to_dQ1_dQ2 is True
    again = loaded.predict(ds)
    for name in C.OUTPUTS:
        assert np.array_equal(again[name].values, out[name].values)


def _sensitivity_model(couple):
    """A network of the trained one's shape with clipped air_temperature levels.  Its weights are random and its input centres
    sit off the sample mean: at the mean profile the trained network's hidden units are all off, which makes a Jacobian of zeros
    (tests/test_gpu_train_dense.py).  The first layer's row of physics_precip is zero, so the network does not see it and
    d total_precipitation_rate / d physics_precip is the closure's own 1."""
    rng = np.random.default_rng(11)
    keep = {n: CLIP.get(n, slice(None)) for n in C.INPUTS}
    stds = [C.columns(n).std(axis=0)[keep[n]] for n in C.INPUTS]
    means = [C.columns(n).mean(axis=0)[keep[n]] + 0.5 * s * rng.normal(0, 1, s.shape[0]) for n, s in zip(C.INPUTS, stds)]
    k = sum(s.shape[0] for s in stds)
    hidden = [rng.normal(0, 1, (k, 8)) / np.sqrt(k), rng.normal(0, 1, (8, 8)) / np.sqrt(8)]
    hidden[0][k - 1] = 0.0   # physics_precip is the last input
    hidden_biases = [rng.normal(0, 0.3, 8) for _ in hidden]
    heads = [rng.normal(0, 1, (8, NZ)) / np.sqrt(8) for _ in range(3)]
    spec = fit.precipitative_spec_from_arrays(C.INPUTS, means, stds, hidden, hidden_biases, heads, [rng.normal(0, 0.1, NZ) for _ in range(3)],
                                              [C.columns(n).mean(axis=0) for n in ("dQ1", "dQ2")],
                                              [C.columns(n).std(axis=0) for n in ("dQ1", "dQ2")], clip=CLIP)
    return fit.HipPrecipitativeModel(C.INPUTS, C.OUTPUTS, spec, couple_precip_to_dQ1_dQ2=couple)


def _column_precip_at(spec, profile):
    """(value, bound) of the de-normalised column-precipitation head at the profile: ``train_np.jacobian_raw``'s forward bound
    through the de-normalisation (one product, one sum)."""
    cols = []
    for i in spec.inputs:
        x = np.asarray(profile[i.source]).astype(np.float32).astype(np.float64)[i.start:i.start + i.nfeat]
        cols.append((x - np.asarray(i.center, np.float64)) / np.asarray(i.scale, np.float64))
    kernels, biases = list(spec.hidden_kernels) + [spec.out_kernel], list(spec.hidden_biases) + [spec.out_bias]
    _, _, yhat, e_y = T.jacobian_raw(kernels, biases, np.concatenate(cols).astype(np.float32))
    o = spec.outputs[2]
    assert o.name == P.COL_PRECIP
    sl = slice(2 * NZ, 3 * NZ)
    scale, center = np.asarray(o.scale, np.float64), np.asarray(o.center, np.float64)
    return yhat[sl] * scale + center, e_y[sl] * np.abs(scale) + 4 * T.U * (np.abs(yhat[sl] * scale) + np.abs(center))


@pytest.mark.parametrize("couple", [True, False], ids=["coupled", "uncoupled"])
def test_input_sensitivity(couple):
    model = _sensitivity_model(couple)
    width = {n: C.columns(n).shape[1] for n in C.INPUTS + C.OUTPUTS}
    sample = Dataset({n: DataArray(C.columns(n) if width[n] > 1 else C.columns(n)[:, 0], dims=["sample", "z"] if width[n] > 1 else ["sample"])
                      for n in C.INPUTS + C.OUTPUTS})
    profile = {n: C.columns(n).mean(axis=0) for n in C.INPUTS}
    raw = model.jacobians(profile)
    head_jac, head_gate = T.predict_jacobians(model.spec, profile)
    cp, e_cp = _column_precip_at(model.spec, profile)
    want, gate = PT.compose_jacobians(head_jac, head_gate, cp, e_cp, profile[C.DELP], couple)
    worst = 0.0
    assert set(raw) == set(C.OUTPUTS)
    for o in C.OUTPUTS:
        assert set(raw[o]) == set(C.INPUTS)
        for i in C.INPUTS:
            assert raw[o][i].shape == (width[o], width[i]) and np.all(np.isfinite(raw[o][i]))
            read = gate[o][i] > 0   # (a column no input reads has no gate: it must be exactly what the closure adds)
            assert np.all(raw[o][i][~read] == want[o][i][~read])
            if read.any():
                frac = float(np.max(np.abs(raw[o][i] - want[o][i])[read] / gate[o][i][read]))
                rel = float(np.max(gate[o][i]) / max(np.max(np.abs(want[o][i])), 1e-300))
                print(f"d {o} / d {i}: {frac:.3f} of the gate (the gate is {rel:.1e} of the largest entry)")
                worst = max(worst, frac)
    assert worst <= 1.0
    assert raw[P.PRECIP][C.PP].shape == (1, 1) and raw[P.PRECIP][C.PP][0, 0] == 1.0
    assert np.all(raw["dQ1"][C.PP] == 0) and np.all(raw["dQ2"][C.PP] == 0)
    for o in C.OUTPUTS:
        assert np.all(raw[o][C.T_NAME][:, :10] == 0), "clipped-away air_temperature levels"
        assert np.any(raw[o][C.T_NAME][:, 10:] != 0) and np.any(raw[o][C.DELP] != 0)
    if not couple:   # the residual heads are the network's own
        assert all(np.array_equal(raw["dQ1"][i], model._head_jacobians(profile)[0]["dQ1"][i]) for i in C.INPUTS)

    got = model.input_sensitivity(sample)
    assert isinstance(got, fit.InputSensitivity) and got.rf_feature_importances is None and set(got.jacobians) == set(C.OUTPUTS)
    std = {n: np.std(C.columns(n), axis=0) for n in C.INPUTS + C.OUTPUTS}
    scaled = T.nondimensionalize(raw, std)
    for o in C.OUTPUTS:
        for i in C.INPUTS:
            assert got.jacobians[o][i].shape == (width[o], width[i])
            np.testing.assert_allclose(got.jacobians[o][i], scaled[o][i], rtol=1e-12, atol=0)
    with pytest.raises(KeyError):
        model.input_sensitivity(Dataset({n: sample[n] for n in C.INPUTS + ["dQ1"]}))
