"""What training the dense network on the device rests on, where no GPU is needed: the float64 restatement the GPU tests
compare against (tests/train_np.py) is itself checked against torch's autograd and ``torch.optim.Adam`` in float64 on the CPU,
and the host-side pieces -- the ``backend`` argument, the input-sensitivity dataclasses, the shared preparation -- behave as
DESIGN.md section 21 says."""
import dataclasses

import numpy as np
import pytest
import torch

import train_np as T
from fv3net_amd import fit
from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec
from fv3net_amd.train import MseLoss
from fv3net_amd.xr_compat import DataArray, Dataset


def _network(rng, k=5, width=4, heads=(3, 4)):
    kernels = [rng.normal(0, 1, (k, width)), rng.normal(0, 1, (width, width)), rng.normal(0, 1, (width, sum(heads)))]
    biases = [rng.normal(0, 0.3, width), rng.normal(0, 0.3, width), rng.normal(0, 0.3, sum(heads))]
    kernels[0][:, 0] = 0.0   # unit 0 of the first layer: pre-activation exactly 0 for every row (relu'(0) = 0)
    biases[0][0] = 0.0
    return kernels, biases


class _Loss64(MseLoss):
    """``MseLoss`` with the unrounded float64 norm (the device's is float32), for the comparison with autograd."""

    def wnorm(self, n):
        return 1.0 / (float(n) * self.kept)


def _loss(rng, n_rows):
    """Two outputs: "a" (3 features) with limits that bind, "b" (4 features) of which the clip keeps [1, 3)."""
    f = 7
    keep = np.array([1, 1, 1, 0, 1, 1, 0], np.float64)
    cstd = rng.uniform(0.5, 2, f)
    return _Loss64(scale=rng.uniform(0.5, 2, f), center=rng.normal(0, 1, f), inv_cstd2=keep / cstd ** 2,
                   lo=np.array([-0.5] * 3 + [-np.inf] * 4), hi=np.array([0.7] * 3 + [np.inf] * 4), keep=keep,
                   kept=np.array([3, 3, 3, 2, 2, 2, 2], np.float64)), cstd


def _torch_loss(params, x, t, loss, cstd):
    (w0, b0, w1, b1, w2, b2) = params
    h = torch.relu(torch.relu(x @ w0 + b0) @ w1 + b1)
    yhat = h @ w2 + b2
    pred = yhat * torch.from_numpy(loss.scale) + torch.from_numpy(loss.center)
    a = torch.clamp(pred[:, :3], min=-0.5, max=0.7)
    b = pred[:, 3:][:, 1:3]
    cs = torch.from_numpy(cstd)
    return torch.mean(((a - t[:, :3]) / cs[:3]) ** 2) + torch.mean(((b - t[:, 3:][:, 1:3]) / cs[3:][1:3]) ** 2)


def test_step_gradient_equals_autograd():
    rng = np.random.default_rng(0)
    kernels, biases = _network(rng)
    loss, cstd = _loss(rng, 40)
    xin, targets = rng.normal(0, 1, (40, 5)), rng.normal(0, 1, (40, 7))
    idx = np.array([5, 5, 39, 0, 17, 3, 2, 1, 30, 29, 28])
    grads, _, value, _ = T.step(kernels, biases, xin, targets, loss, idx)

    params = [torch.from_numpy(np.asarray(p, np.float64)).requires_grad_() for kb in zip(kernels, biases) for p in kb]
    x, t = torch.from_numpy(xin[idx]), torch.from_numpy(targets[idx])
    total = _torch_loss(params, x, t, loss, cstd)
    total.backward()
    pred = (T.linear_forward(T.linear_forward(T.linear_forward(xin, kernels[0], biases[0], idx, True)[0], kernels[1], biases[1], None, True)[0],
                             kernels[2], biases[2])[0] * loss.scale + loss.center)[:, :3]
    assert (pred < -0.5).any() and (pred > 0.7).any() and ((pred > -0.5) & (pred < 0.7)).any(), "the limits must bind somewhere"
    assert abs(value - float(total.detach())) <= 1e-12 * abs(float(total.detach()))
    for l in range(3):
        for got, want in zip(grads[l], (params[2 * l].grad.numpy(), params[2 * l + 1].grad.numpy())):
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    assert np.all(grads[0][0][:, 0] == 0) and grads[0][1][0] == 0, "a pre-activation of exactly 0 passes no gradient"
    assert np.all(grads[2][0][:, [3, 6]] == 0), "clipped-away output features have no gradient"


def test_adam_equals_torch_float64():
    rng = np.random.default_rng(1)
    p0 = rng.normal(0, 1, 50)
    gs = [rng.normal(0, 1, 50) * 10.0 ** rng.integers(-6, 3, 50) for _ in range(5)]
    tp = torch.from_numpy(p0.copy()).requires_grad_()
    opt = torch.optim.Adam([tp], lr=1e-3)
    p, m, v = p0.copy(), np.zeros(50), np.zeros(50)
    for t, g in enumerate(gs, start=1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = T.adam(p, g, m, v, t)
        assert np.max(np.abs(p - tp.detach().numpy()) / np.abs(p)) <= 1e-14


def _sensitivity_spec(rng):
    """An input clipped to levels [2, 6) of 6, a scalar input, a limit that binds and an output with masked levels."""
    k, w = 5, 6
    return MlpSpec(
        inputs=[InputSpec("T", 4, start=2, center=rng.normal(0, 1, 4).astype(np.float32), scale=rng.uniform(0.5, 2, 4).astype(np.float32)),
                InputSpec("c", 1, center=np.float32([0.1]), scale=np.float32([0.7]))],
        hidden_kernels=[rng.normal(0, 1, (k, w)).astype(np.float32), rng.normal(0, 1, (w, w)).astype(np.float32)],
        hidden_biases=[rng.normal(0, 0.3, w).astype(np.float32), rng.normal(0, 0.3, w).astype(np.float32)],
        outputs=[OutputSpec("dQ1", 5, scale=rng.uniform(0.5, 2, 5).astype(np.float32), center=rng.normal(0, 1, 5).astype(np.float32),
                            min=-0.4, max=0.9),
                 OutputSpec("dQ2", 3, scale=rng.uniform(0.5, 2, 3).astype(np.float32), center=rng.normal(0, 1, 3).astype(np.float32),
                            mask=np.float32([0, 1, 1]))],
        out_kernel=rng.normal(0, 1, (w, 8)).astype(np.float32), out_bias=rng.normal(0, 0.3, 8).astype(np.float32))


def _torch_predict(spec, T_, c):
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    cols = []
    for i, src in zip(spec.inputs, (T_, c)):
        cols.append((src[i.start:i.start + i.nfeat] - f64(i.center)) / f64(i.scale))
    h = torch.cat(cols)
    for kern, b in zip(spec.hidden_kernels, spec.hidden_biases):
        h = torch.relu(h @ f64(kern) + f64(b))
    yhat = h @ f64(spec.out_kernel) + f64(spec.out_bias)
    outs, f0 = [], 0
    for o in spec.outputs:
        y = yhat[f0:f0 + o.nfeat] * f64(o.scale) + f64(o.center)
        f0 += o.nfeat
        if o.min is not None or o.max is not None:
            y = torch.clamp(y, min=o.min, max=o.max)
        if o.mask is not None:
            y = y * f64(o.mask)
        outs.append(y)
    return tuple(outs)


def test_predict_jacobian_equals_autograd():
    rng = np.random.default_rng(2)
    spec = _sensitivity_spec(rng)
    prof = {"T": rng.normal(0, 1, 6).astype(np.float32), "c": rng.normal(0, 1, 1).astype(np.float32)}
    got, _ = T.predict_jacobians(spec, prof)
    args = (torch.from_numpy(prof["T"].astype(np.float64)), torch.from_numpy(prof["c"].astype(np.float64)))
    want = torch.autograd.functional.jacobian(lambda a, b: _torch_predict(spec, a, b), args)
    y = [v.numpy() for v in _torch_predict(spec, *args)]
    assert ((y[0] == np.float64(-0.4)) | (y[0] == np.float64(0.9))).any() and ((y[0] > -0.4) & (y[0] < 0.9)).any(), "the limit must bind"
    for oi, o in enumerate(spec.outputs):
        for si, s in enumerate(("T", "c")):
            w = want[oi][si].numpy()
            assert got[o.name][s].shape == w.shape
            assert np.max(np.abs(got[o.name][s] - w)) <= 1e-12 * max(np.max(np.abs(w)), 1.0)
    assert np.all(got["dQ1"]["T"][:, :2] == 0) and np.all(got["dQ2"]["T"][0] == 0) and np.all(got["dQ2"]["c"][0] == 0)
    outside = (y[0] == -0.4) | (y[0] == 0.9)
    assert np.all(got["dQ1"]["T"][outside] == 0) and np.all(got["dQ1"]["c"][outside] == 0)


def _batches(rng, n_batches=2, nz=6):
    out = []
    for _ in range(n_batches):
        a = rng.normal(0, 1, (nz, 8, 8)).astype(np.float32)
        c = rng.normal(0, 1, (8, 8)).astype(np.float32)
        out.append(Dataset({"a": DataArray(a, dims=["z", "y", "x"]), "c": DataArray(c, dims=["y", "x"]),
                            "b": DataArray(2 * a + c, dims=["z", "y", "x"])}))
    return out


def test_backend_argument_errors():
    batches = _batches(np.random.default_rng(3))
    hp = fit.DenseHyperparameters(["a", "c"], ["b"], width=4, depth=2, epochs=0)
    with pytest.raises(ValueError, match="backend"):
        fit.train_dense_model(hp, batches, backend="rocblas")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit.train_dense_model(hp, batches, device="cpu", backend="hip")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fit.train_dense_model(hp, batches, backend="hip")


def test_input_sensitivity_dataclasses():
    rf = fit.RandomForestInputSensitivity(mean_importances=[0.1, 0.2], std_importances=[0.01, 0.02], indices=[0, 1])
    jac = {"b": {"a": np.ones((2, 3))}}
    s = fit.InputSensitivity(jacobians=jac)
    assert s.jacobians is jac and s.rf_feature_importances is None
    s2 = fit.InputSensitivity(rf_feature_importances={"a": rf})
    assert s2.jacobians is None and s2.rf_feature_importances["a"].indices == [0, 1]
    assert {f.name for f in dataclasses.fields(rf)} == {"mean_importances", "std_importances", "indices"}
    assert fit.JacobianInputSensitivity is not None
    from fv3net_amd.fit.input_sensitivity import nondimensionalize_jacobians

    got = nondimensionalize_jacobians(jac, {"a": np.array([1.0, 2.0, 3.0]), "b": np.array([2.0, 0.0])})
    assert np.array_equal(got["b"]["a"][0], [0.5, 1.0, 1.5]) and np.all(np.isinf(got["b"]["a"][1]))
    with pytest.raises(KeyError):
        nondimensionalize_jacobians(jac, {"a": np.ones(3)})


def test_default_backend_starts_as_before():
    """``epochs=0``: the spec holds the fitted normalisation and the initial layers -- glorot-uniform kernels and zero biases
    drawn from ``torch.manual_seed(seed)`` in the order trunk, heads -- whichever way the backend is spelled."""
    batches = _batches(np.random.default_rng(4))
    hp = fit.DenseHyperparameters(["a", "c"], ["b"], width=4, depth=3, epochs=0, seed=7, clip={"a": slice(1, 5)})
    default = fit.train_dense_model(hp, batches, device="cpu").spec
    named = fit.train_dense_model(hp, batches, device="cpu", backend="torch").spec
    torch.manual_seed(7)
    want = []
    for fan_in, fan_out in ((5, 4), (4, 4), (4, 6)):
        lin = torch.nn.Linear(fan_in, fan_out)
        torch.nn.init.xavier_uniform_(lin.weight)
        want.append(lin.weight.detach().numpy().T.copy())
    for spec in (default, named):
        assert np.array_equal(spec.hidden_kernels[0], want[0]) and np.array_equal(spec.hidden_kernels[1], want[1])
        assert np.array_equal(spec.out_kernel, want[2])
        assert not np.any(spec.out_bias) and not any(np.any(b) for b in spec.hidden_biases)
    a = np.concatenate([b["a"].values.reshape(6, -1).T for b in batches])[:, 1:5]
    assert np.array_equal(default.inputs[0].center, a.mean(axis=0).astype(np.float32)) and default.inputs[0].start == 1
    m0, a0 = default.to_arrays()
    m1, a1 = named.to_arrays()
    assert m0 == m1 and a0.keys() == a1.keys() and all(np.array_equal(a0[k], a1[k]) for k in a0)
