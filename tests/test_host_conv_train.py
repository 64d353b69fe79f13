"""What training the convolutional network on the device rests on, where no GPU is needed: the float64
restatement the GPU tests compare against (tests/conv_train_np.py) is itself checked against torch's autograd through
``F.conv2d`` in float64, its constraint against float32 torch, its data preparation against the halo fixture; and the host side
of ``fit.train_convolutional_model`` -- the shared preparation, the torch backend, the hyperparameter checks, the ``backend``
argument -- behaves as the design says."""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

import conv_np
import conv_train_np as C
from fv3net_amd import fit
from fv3net_amd.conv import ConvSpec
from fv3net_amd.fit import conv as fit_conv
from fv3net_amd.xr_compat import DataArray, Dataset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "append_halos_reference.npz")
F = torch.nn.functional


# ---- the restatement against autograd -------------------------------------------------------------------------------------
# id -> (k, c, f, input extent, batch, bias, force a pre-activation of exactly 0)
CONTRACTIONS = {
    "k1": (1, 3, 4, (5, 5), 2, True, False),
    "k3": (3, 3, 4, (7, 7), 2, True, False),
    "k5": (5, 2, 3, (9, 9), 2, True, False),
    "rectangular": (3, 3, 4, (6, 9), 3, True, False),
    "zero_preactivation": (3, 3, 4, (7, 7), 2, True, True),
    "no_bias": (3, 3, 4, (7, 6), 2, False, False),
}


@pytest.mark.parametrize("case", list(CONTRACTIONS))
def test_contractions_equal_autograd(case):
    k, c, f, (X, Y), n, bias, zero = CONTRACTIONS[case]
    rng = np.random.default_rng(sorted(CONTRACTIONS).index(case))
    a, w = rng.normal(0, 1, (n, X, Y, c)), rng.normal(0, 1, (k, k, c, f))
    b = rng.normal(0, 0.3, f) if bias else None
    if zero:   # filter 0: pre-activation exactly 0 everywhere (relu'(0) = 0)
        w[..., 0] = 0.0
        b[0] = 0.0
    ta = torch.from_numpy(a).permute(0, 3, 1, 2).requires_grad_()
    tw = torch.from_numpy(w).permute(3, 2, 0, 1).requires_grad_()
    tb = None if b is None else torch.from_numpy(b).requires_grad_()
    h1 = torch.relu(F.conv2d(ta, tw, tb))
    # a second layer, so that the ReLU mask of the first acts on a gradient with respect to an input
    w2 = rng.normal(0, 1, (k, k, f, 2)) if min(X, Y) >= 2 * k - 1 else rng.normal(0, 1, (1, 1, f, 2))
    tw2 = torch.from_numpy(w2).permute(3, 2, 0, 1).requires_grad_()
    h2 = F.conv2d(h1, tw2)
    cot = rng.normal(0, 1, tuple(h2.shape))
    (h2 * torch.from_numpy(cot)).sum().backward()

    got1, _ = C.conv_forward(a, w, b, relu=True)
    assert np.max(np.abs(got1 - h1.detach().permute(0, 2, 3, 1).numpy())) <= 1e-12
    got2, _ = C.conv_forward(got1, w2)
    assert np.max(np.abs(got2 - h2.detach().permute(0, 2, 3, 1).numpy())) <= 1e-12
    dh2 = cot.transpose(0, 2, 3, 1)
    dw2, _, _, _ = C.conv_backward_weight(got1, dh2, w2.shape[0])
    assert np.max(np.abs(dw2 - tw2.grad.permute(2, 3, 1, 0).numpy())) <= 1e-12 * max(1.0, np.max(np.abs(dw2)))
    dh1, _ = C.conv_backward_data(dh2, w2, p=got1)
    dw1, db1, _, _ = C.conv_backward_weight(a, dh1, k)
    assert np.max(np.abs(dw1 - tw.grad.permute(2, 3, 1, 0).numpy())) <= 1e-12 * max(1.0, np.max(np.abs(dw1)))
    if bias:
        assert np.max(np.abs(db1 - tb.grad.numpy())) <= 1e-12 * max(1.0, np.max(np.abs(db1)))
    da, _ = C.conv_backward_data(dh1, w)
    assert np.max(np.abs(da - ta.grad.permute(0, 2, 3, 1).numpy())) <= 1e-12 * max(1.0, np.max(np.abs(da)))
    if zero:
        assert np.all(got1[..., 0] == 0) and np.all(dh1[..., 0] == 0) and np.all(dw1[..., 0] == 0) and db1[0] == 0, \
            "a pre-activation of exactly 0 passes no gradient"


def test_forward_agrees_with_the_predictors_oracle():
    rng = np.random.default_rng(3)
    a, w = rng.normal(0, 1, (2, 7, 6, 3)), rng.normal(0, 1, (3, 3, 3, 4))
    assert np.max(np.abs(C.conv_forward(a, w)[0] - conv_np.conv2d_valid(a, w))) <= 1e-12


def test_out_of_range_samples_read_as_zeros():
    rng = np.random.default_rng(4)
    a, w = rng.normal(0, 1, (3, 5, 5, 2)), rng.normal(0, 1, (3, 3, 2, 2))
    h, _ = C.conv_forward(a, w, np.ones(2), idx=[2, 2, 7, -1, 0])
    assert np.all(h[2] == 1) and np.all(h[3] == 1) and np.array_equal(h[0], h[1]) and not np.array_equal(h[0], h[4])


@pytest.mark.parametrize("k, c, f", [(1, 3, 2), (3, 5, 7), (5, 2, 3)])
def test_constraint_is_bitwise_torch_float32(k, c, f):
    w = np.random.default_rng(k).normal(0, 1, (k, k, c, f)).astype(np.float32)
    tw = torch.from_numpy(w)
    want = (0.5 * (tw + tw.transpose(0, 1))).numpy()
    got = C.constrain(w)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), got.transpose(1, 0, 2, 3).view(np.uint32)), "bitwise symmetric"


def test_whole_step_equals_autograd_and_adam():
    """``conv_train_np.step`` + ``update`` against the float64 twin: F.conv2d, the std-scaled MSE, autograd, torch's Adam, the
    constraint after the update."""
    from fv3net_amd.train import MseLoss

    class Loss64(MseLoss):   # the unrounded float64 norm (the device's is float32)
        def wnorm(self, n):
            return 1.0 / (float(n) * self.kept)

    rng = np.random.default_rng(9)
    xin, idx = rng.normal(0, 1, (5, 9, 9, 3)), np.array([4, 4, 0, 2])
    ws = [rng.normal(0, 0.5, (3, 3, 3, 4)), rng.normal(0, 0.5, (3, 3, 4, 4))]
    bs = [rng.normal(0, 0.3, 4), rng.normal(0, 0.3, 4)]
    ws[0][..., 0], bs[0][0] = 0.0, 0.0   # a pre-activation of exactly 0
    wo, bo = rng.normal(0, 1, (4, 3)), rng.normal(0, 0.3, 3)
    targets = rng.normal(0, 1, (5 * 25, 3))
    cstd, scale, center = rng.uniform(0.5, 2, 3), rng.uniform(0.5, 2, 3), rng.normal(0, 1, 3)
    loss = Loss64(scale=scale, center=center, inv_cstd2=1 / cstd ** 2, lo=np.full(3, -np.inf), hi=np.full(3, np.inf), keep=np.ones(3),
                  kept=np.array([2.0, 2.0, 1.0]))   # two outputs: features 0-1 and feature 2
    grads, bounds, value, _ = C.step(ws, bs, wo, bo, xin, targets, loss, idx)

    tw = [torch.from_numpy(w).permute(3, 2, 0, 1).contiguous().requires_grad_() for w in ws]
    tb = [torch.from_numpy(b).clone().requires_grad_() for b in bs]
    two, tbo = torch.from_numpy(wo).clone().requires_grad_(), torch.from_numpy(bo).clone().requires_grad_()
    a = torch.from_numpy(xin[idx]).permute(0, 3, 1, 2)
    for w, b in zip(tw, tb):
        a = torch.relu(F.conv2d(a, w, b))
    pred = (a.permute(0, 2, 3, 1).reshape(-1, 4) @ two + tbo) * torch.from_numpy(scale) + torch.from_numpy(center)
    rows = (idx[:, None] * 25 + np.arange(25)[None]).reshape(-1)
    z = (pred - torch.from_numpy(targets[rows])) / torch.from_numpy(cstd)
    total = torch.mean(z[:, :2] ** 2) + torch.mean(z[:, 2:] ** 2)
    params = [tw[0], tb[0], tw[1], tb[1], two, tbo]
    opt = torch.optim.Adam(params, lr=1e-2)
    total.backward()
    assert abs(value - float(total.detach())) <= 1e-12 * abs(float(total.detach()))
    want = [tw[0].grad.permute(2, 3, 1, 0).numpy(), tb[0].grad.numpy(), tw[1].grad.permute(2, 3, 1, 0).numpy(), tb[1].grad.numpy(),
            two.grad.numpy(), tbo.grad.numpy()]
    got = [x for g in grads for x in g]
    for g, w, bound in zip(got, want, [x for b in bounds for x in b]):
        assert np.max(np.abs(g - w)) <= 1e-12 * np.max(np.abs(w)) and g.shape == bound.shape and np.all(bound > 0)
    assert np.all(got[0][..., 0] == 0) and got[1][0] == 0

    opt.step()
    with torch.no_grad():
        for w in tw:
            w.copy_(0.5 * (w + w.transpose(2, 3)))
    before = [ws[0], bs[0], ws[1], bs[1], wo, bo]
    zeros = [np.zeros_like(p) for p in before]
    new, _, _ = C.update(before, got, zeros, zeros, 1, lr=1e-2, constrained=(0, 2))
    after = [tw[0].detach().permute(2, 3, 1, 0).numpy(), tb[0].detach().numpy(), tw[1].detach().permute(2, 3, 1, 0).numpy(),
             tb[1].detach().numpy(), two.detach().numpy(), tbo.detach().numpy()]
    for g, w, g0 in zip(new, after, got):
        # (where a gradient is a rounding residue of the order of eps = 1e-8, Adam's first step is ill-conditioned: left out)
        firm = np.abs(g0) > 1e-6
        assert np.max(np.abs(g - w)[firm]) <= 1e-10


# ---- the data preparation ----------------------------------------------------------------------------------------------------
def _dataset(cube):
    dims = {5: ["sample", "tile", "x", "y", "z"], 4: ["sample", "tile", "x", "y"]}
    return Dataset({name: DataArray(a, dims=dims[a.ndim]) for name, a in cube.items()})


@pytest.mark.parametrize("depth, key", [(2, "padded_1"), (4, "padded_3")])
def test_preparation_pads_with_the_references_halos_then_normalises(depth, key):
    with np.load(GOLDEN) as z:
        ids, padded = z["input"].astype(np.float32), z[key].astype(np.float32)   # [6, c, x, y], [6, c, x + 2 h, y + 2 h]
    h = (padded.shape[-1] - ids.shape[-1]) // 2
    cube = {"ids": ids.transpose(0, 2, 3, 1)[None], "one": ids[None, :, 0], "out": ids.transpose(0, 2, 3, 1)[None, ..., :1]}
    hp = fit.ConvolutionalHyperparameters(["ids", "one"], ["out"], filters=2, depth=depth, kernel_size=3)
    prep = fit_conv._prepare_conv_training(hp, [_dataset(cube)])
    assert prep.n_halo == h
    want = np.concatenate([padded.transpose(0, 2, 3, 1), padded.transpose(0, 2, 3, 1)[..., :1]], axis=-1)   # [6, X, Y, 3] raw
    mean, std = np.concatenate(prep.x_mean), np.concatenate(prep.x_std)
    # the statistics are those of the PADDED cube: halo cells and the raw-zero corners included (fitted in float32 as the
    # reference fits them: a running float32 sum of n terms is good to n 2^-24)
    rtol = want.reshape(-1, 3).shape[0] * 2.0 ** -24
    assert np.allclose(mean, want.reshape(-1, 3).astype(np.float64).mean(axis=0), rtol=rtol)
    assert np.allclose(std, want.reshape(-1, 3).astype(np.float64).std(axis=0), rtol=rtol)
    inner = want[:, h:-h, h:-h].reshape(-1, 3).astype(np.float64).mean(axis=0)
    assert np.all(np.abs(mean - inner) > 1e-3 * np.abs(inner)), "the fixture must tell the two fits apart"
    scale = std + np.float32(1e-7)
    assert prep.xin.dtype == np.float32 and np.array_equal(prep.xin, (want - mean) / scale)
    for corner in (prep.xin[:, :h, :h], prep.xin[:, -h:, :h], prep.xin[:, :h, -h:], prep.xin[:, -h:, -h:]):
        assert np.array_equal(corner, np.broadcast_to((np.float32(0) - mean) / scale, corner.shape))
    # the restatement prepares the same numbers
    ref = C.prepare([cube["ids"], cube["one"][..., None]], [cube["out"]], h, hp.normalization_fit_samples)
    # (mean and scale each within rtol of the float64 fit: the quotient moves by rtol |mean| / scale + rtol |xin|)
    assert np.all(np.abs(prep.xin - ref["xin"]) <= 2 * rtol * (np.abs(mean) / scale + np.abs(ref["xin"])) + 2.0 ** -22)
    assert np.array_equal(prep.y[0], ref["y"][0]) and np.allclose(prep.y_std[0], ref["y_std"][0], rtol=rtol)
    assert np.array_equal(prep.loss_std[0], np.std(ref["y"][0].reshape(-1, 1), axis=0, dtype=np.float32))


def test_preparation_fits_on_the_first_tile_samples_only():
    cube = C.tiny_cube()
    hp = fit.ConvolutionalHyperparameters(C.TINY_INPUTS, C.TINY_OUTPUTS, filters=8, normalization_fit_samples=5)
    prep = fit_conv._prepare_conv_training(hp, [_dataset(cube)])
    ref = C.prepare([cube["field"], cube["surface"][..., None]], [cube["tendency"], cube["flux"][..., None]], 2, 5)
    assert prep.xin.shape == (18, 12, 12, 5) and [a.shape for a in prep.y] == [(18, 8, 8, 3), (18, 8, 8, 1)]
    rtol = 5 * 144 * 2.0 ** -24   # (float32 sums over the 5 fitted tile-samples of 12 x 12 cells)
    assert np.allclose(np.concatenate(prep.x_mean), np.concatenate(ref["x_mean"]), rtol=rtol)
    assert np.allclose(np.concatenate(prep.y_std), np.concatenate(ref["y_std"]), rtol=rtol)
    full = C.prepare([cube["field"], cube["surface"][..., None]], [cube["tendency"], cube["flux"][..., None]], 2, 30)
    assert not np.allclose(np.concatenate(prep.x_mean), np.concatenate(full["x_mean"]), rtol=100 * rtol)


def test_preparation_rejects_what_the_reference_rejects():
    cube = C.tiny_cube(n_samples=1)
    hp = fit.ConvolutionalHyperparameters(C.TINY_INPUTS, C.TINY_OUTPUTS, filters=8)
    with pytest.raises(ValueError, match="dataset must have 6 tiles to halo update, got 5"):
        fit_conv._prepare_conv_training(hp, [_dataset({k: v[:, :5] for k, v in cube.items()})])
    with pytest.raises(ValueError, match="x and y dimensions should be the same length, got shape"):
        fit_conv._prepare_conv_training(hp, [_dataset({k: v[:, :, :, :6] for k, v in cube.items()})])


# ---- the torch backend end to end ----------------------------------------------------------------------------------------------
EPOCHS, LEARNING_RATE, BATCH = 4, 1e-2, 4


def tiny_hyperparameters(**kw):
    base = dict(filters=8, depth=3, kernel_size=3, epochs=EPOCHS, batch_size=BATCH, learning_rate=LEARNING_RATE)
    base.update(kw)
    return fit.ConvolutionalHyperparameters(list(C.TINY_INPUTS), list(C.TINY_OUTPUTS), **base)


@functools.lru_cache(maxsize=None)
def trained(epochs=EPOCHS, seed=0):
    return fit.train_convolutional_model(tiny_hyperparameters(epochs=epochs, seed=seed), [_dataset(C.tiny_cube())], device="cpu",
                                         backend="torch")


def _bits(spec):
    meta, arrays = spec.to_arrays()
    return meta, {k: np.asarray(v).tobytes() for k, v in arrays.items()}


def test_epochs_0_returns_the_initial_weights_in_keras_layout():
    model = trained(epochs=0)
    spec = model.spec
    assert isinstance(spec, ConvSpec) and model.n_halo == 2 and spec.halos_required == 2
    assert [w.shape for w in spec.hidden_kernels] == [(3, 3, 5, 8), (3, 3, 8, 8)]
    assert [o.kernel.shape for o in spec.outputs] == [(8, 3), (8, 1)] and spec.sources == C.TINY_INPUTS
    prep = fit_conv._prepare_conv_training(tiny_hyperparameters(epochs=0), [_dataset(C.tiny_cube())])
    for w, conv in zip(spec.hidden_kernels, prep.hidden):   # the seeded Conv2d initialisation, [f, c, a, b] -> [a, b, c, f]
        assert np.array_equal(w, conv.weight.detach().numpy().transpose(2, 3, 1, 0))
        limit = np.sqrt(6.0 / (9 * w.shape[2] + 9 * w.shape[3]))   # glorot_uniform: fans k k c_in and k k c_out
        assert np.max(np.abs(w)) <= limit and np.max(np.abs(w)) > 0.8 * limit
    assert all(np.all(b == 0) for b in spec.hidden_biases) and all(np.all(o.bias == 0) for o in spec.outputs)
    # Keras applies a constraint after an update, not at initialisation
    assert not np.array_equal(spec.hidden_kernels[0], spec.hidden_kernels[0].transpose(1, 0, 2, 3))


def test_training_lowers_the_loss_and_keeps_the_kernels_symmetric():
    cube = C.tiny_cube()
    before, after = C.evaluate_loss(trained(epochs=0).spec, cube), C.evaluate_loss(trained().spec, cube)
    print(f"training loss: {before:.4f} -> {after:.4f}")
    assert after < before
    for w in trained().spec.hidden_kernels:
        assert np.array_equal(w.view(np.uint32), w.transpose(1, 0, 2, 3).view(np.uint32))


def test_same_seed_gives_the_same_bits_and_another_seed_does_not():
    again = fit.train_convolutional_model(tiny_hyperparameters(), [_dataset(C.tiny_cube())], device="cpu", backend="torch")
    assert _bits(again.spec) == _bits(trained().spec)
    assert _bits(trained(seed=1).spec) != _bits(trained().spec)
    default = fit.train_convolutional_model(tiny_hyperparameters(epochs=1), [_dataset(C.tiny_cube())], device="cpu")
    assert _bits(default.spec) == _bits(trained(epochs=1).spec), "the default backend is torch"


def test_dump_load_round_trip(tmp_path):
    model = trained()
    fit.dump(model, str(tmp_path / "model"))
    loaded = fit.load(str(tmp_path / "model"))
    assert isinstance(loaded, fit.HipConvolutionalModel) and loaded.n_halo == 2
    assert _bits(loaded.spec) == _bits(model.spec)
    assert list(loaded.input_variables) == C.TINY_INPUTS and list(loaded.output_variables) == C.TINY_OUTPUTS


def test_tanh_trains_on_the_torch_backend_only():
    model = fit.train_convolutional_model(tiny_hyperparameters(activation_function="tanh", epochs=1), [_dataset(C.tiny_cube())],
                                          device="cpu", backend="torch")
    assert model.spec.activation == "tanh"
    with pytest.raises(ValueError, match="backend='hip' trains with activation_function 'relu' or 'linear'"):
        fit.train_convolutional_model(tiny_hyperparameters(activation_function="tanh"), [_dataset(C.tiny_cube())], backend="hip")


# ---- what is rejected ------------------------------------------------------------------------------------------------------------
def test_defaults_are_the_references():
    hp = fit.ConvolutionalHyperparameters(["a"], ["b"])
    got = {f.name: getattr(hp, f.name) for f in dataclasses.fields(hp)}
    assert got == dict(input_variables=["a"], output_variables=["b"], filters=32, depth=3, kernel_size=3, activation_function="relu",
                       transpose_invariant=True, epochs=3, batch_size=1, learning_rate=1e-3, normalization_fit_samples=30, seed=0,
                       diffusive=False, gaussian_noise=0.0, spectral_normalization=False, kernel_regularizer=None, clip_config={},
                       loss_type="mse", loss_scaling="standard")


@pytest.mark.parametrize("field, value", [("diffusive", True), ("gaussian_noise", 0.1), ("spectral_normalization", True),
                                          ("kernel_regularizer", "l2"), ("clip_config", {"tendency": slice(1, 3)}),
                                          ("loss_type", "mae"), ("loss_scaling", "uniform")])
def test_unsupported_fields_raise_not_implemented_naming_the_field(field, value):
    with pytest.raises(NotImplementedError, match=field):
        fit.train_convolutional_model(tiny_hyperparameters(**{field: value}), [_dataset(C.tiny_cube())], device="cpu")


def test_bad_networks_and_backends_raise():
    data = [_dataset(C.tiny_cube())]
    with pytest.raises(ValueError, match="depth must be at least 2"):
        fit.train_convolutional_model(tiny_hyperparameters(depth=1), data, device="cpu")
    with pytest.raises(ValueError, match="kernel_size must be odd"):
        fit.train_convolutional_model(tiny_hyperparameters(kernel_size=4), data, device="cpu")
    with pytest.raises(ValueError, match="activation_function 'gelu' is not supported"):
        fit.train_convolutional_model(tiny_hyperparameters(activation_function="gelu"), data, device="cpu")
    with pytest.raises(ValueError, match="backend must be None, 'torch' or 'hip'"):
        fit.train_convolutional_model(tiny_hyperparameters(), data, device="cpu", backend="tensorflow")


def test_hip_backend_needs_a_device():
    with pytest.raises(RuntimeError, match="device tensors only"):
        fit.train_convolutional_model(tiny_hyperparameters(), [_dataset(C.tiny_cube())], device="cpu", backend="hip")
