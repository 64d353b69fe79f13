"""Training the graph U-Net without a GPU: the float64 restatement of the backward entries (tests/graph_train_np.py) against
``torch.autograd`` on ``GraphUNetTwin``, AdamW against ``torch.optim.AdamW``, the self-adjointness of mean5 that the backward
kernels rest on, and the ``backend`` argument of ``fit.train_graph_model``.

``tests/golden/graph_train_torch_backend.npz`` holds the arrays of the spec (``GraphUNetSpec.to_arrays``) that
``train_graph_model`` returned on the CPU for ``_golden_problem()`` at the commit before the ``backend`` argument existed: it was
made by running that commit's ``fit/graph.py`` on exactly these inputs and saving the result with ``np.savez_compressed``.
"""
import os

import numpy as np
import pytest
import torch

import graph_train_np as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_train_torch_backend.npz")


def _twin_layers(twin, depth, n_features, min_filters, grad=False):
    """``layer_plan`` name -> float64 arrays in the spec's layout, from the twin's parameters (or their gradients)."""
    from fv3net_amd.fit.graph import _module_prefix
    from fv3net_amd.graph import layer_plan

    params = dict(twin.named_parameters())
    get = lambda key: (params[key].grad if grad else params[key]).detach().numpy()
    out = {}
    for name, kind, *_ in layer_plan(depth, n_features, min_filters):
        prefix = _module_prefix(name, depth)
        if kind == "up":
            out[name] = (get(f"{prefix}.up.weight").transpose(0, 2, 3, 1), get(f"{prefix}.up.bias"))
        else:
            op = f"{prefix}.graph_op"
            out[name] = (get(f"{op}.fc_self.weight").T, get(f"{op}.fc_neigh.weight").T, get(f"{op}.bias"))
    return out


@pytest.mark.parametrize("multistep", [1, 2])
@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("depth", [1, 2])
def test_restatement_equals_autograd(depth, activation, multistep):
    """Every parameter gradient and the gradient into the first state, to 1e-12 of max(1, the largest entry), in float64 at
    nx = 4, S = 2.  Tile 0 of sample 0 is zero at time 0 and ``first`` has no bias, so the interior cells of that tile have a
    pre-activation of exactly 0 there (relu'(0) = 0 in torch and here)."""
    from fv3net_amd.fit.graph import GraphUNetTwin, _multistep_loss

    torch.manual_seed(depth * 10 + multistep)
    F, m, nx, S = 3, 4, 4, 2
    twin = GraphUNetTwin(F, depth, m, activation).double()
    rng = np.random.default_rng(5)
    with torch.no_grad():
        for key, p in twin.named_parameters():
            if key.endswith("bias") and not key.startswith("_first_conv"):
                p.copy_(torch.from_numpy(rng.normal(0, 0.1, tuple(p.shape))))
    batch = rng.normal(0, 1, (S, multistep + 1, 6, nx, nx, F))
    batch[0, 0, 0] = 0.0
    x = torch.from_numpy(batch).requires_grad_(True)
    loss = _multistep_loss(twin, x, multistep)
    loss.backward()
    if activation == "relu":
        with torch.no_grad():
            pre = twin._first_conv[0](x[:, 0])
        assert int((pre == 0).sum()) > 0, "the case holds no pre-activation of exactly 0"
    layers = _twin_layers(twin, depth, F, m)
    want = _twin_layers(twin, depth, F, m, grad=True)
    got_loss, got, _, d_in, _ = G.network_gradients(layers, depth, m, activation, batch, multistep)
    assert abs(got_loss - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    worst = 0.0
    for name, arrays in want.items():
        for a, b in zip(got[name], arrays):
            err = np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))
            worst = max(worst, err)
            assert err <= 1e-12, (name, err)
    d_want = x.grad[:, 0].numpy()
    err = np.max(np.abs(d_in - d_want)) / max(1.0, np.max(np.abs(d_want)))
    print(f"depth {depth} {activation} multistep {multistep}: worst parameter gradient error {worst:.2e}, input gradient {err:.2e}")
    assert err <= 1e-12


def test_single_entries_equal_autograd():
    """The five entries one by one against autograd on the twin's own modules (float64): a SAGE layer with tanh behind it, the
    transposed convolution and the 2 x 2 mean."""
    from fv3net_amd.fit.graph import _SageMean, _Up

    rng = np.random.default_rng(1)
    S, n, ci, co = 2, 4, 3, 5
    op = _SageMean(ci, co).double()
    p = np.tanh(rng.normal(0, 1, (S, 6, n, n, ci)))            # the post-activation that fed the layer
    x = torch.from_numpy(np.arctanh(p)).requires_grad_(True)
    g = rng.normal(0, 1, (S, 6, n, n, co))
    (op(torch.tanh(x)) * torch.from_numpy(g)).sum().backward()
    ws, wn = op.fc_self.weight.detach().numpy().T, op.fc_neigh.weight.detach().numpy().T
    dx, _ = G.sage_backward_data(g, ws, wn, p, "tanh")
    dws, dwn, db, *_ = G.sage_backward_weight(p, g)
    assert np.max(np.abs(dx - x.grad.numpy())) <= 1e-12
    assert np.max(np.abs(dws - op.fc_self.weight.grad.numpy().T)) <= 1e-12
    assert np.max(np.abs(dwn - op.fc_neigh.weight.grad.numpy().T)) <= 1e-12
    assert np.max(np.abs(db - op.bias.grad.numpy())) <= 1e-12

    up = _Up(2 * co).double()
    low = torch.from_numpy(rng.normal(0, 1, (S, 6, n, n, 2 * co))).requires_grad_(True)
    dcat = rng.normal(0, 1, (S, 6, 2 * n, 2 * n, co))
    (up(torch.relu(low)) * torch.from_numpy(dcat)).sum().backward()
    w = up.up.weight.detach().numpy().transpose(0, 2, 3, 1)
    post = np.maximum(low.detach().numpy(), 0)
    dlow, _ = G.up2_backward_data(dcat, w, post, "relu")
    dw, dbu, *_ = G.up2_backward_weight(post, dcat)
    assert np.max(np.abs(dlow - low.grad.numpy())) <= 1e-12
    assert np.max(np.abs(dw - up.up.weight.grad.numpy().transpose(0, 2, 3, 1))) <= 1e-12
    assert np.max(np.abs(dbu - up.up.bias.grad.numpy())) <= 1e-12

    before = torch.from_numpy(rng.normal(0, 1, (S, 6, n, n, co))).requires_grad_(True)
    skip, dpool = rng.normal(0, 1, (S, 6, n, n, co)), rng.normal(0, 1, (S, 6, n // 2, n // 2, co))
    y = torch.relu(before)
    pooled = y.reshape(S, 6, n // 2, 2, n // 2, 2, co).mean(dim=(3, 5))
    ((y * torch.from_numpy(skip)).sum() + (pooled * torch.from_numpy(dpool)).sum()).backward()
    got, _ = G.pool2_backward(skip, dpool, y.detach().numpy(), "relu")
    assert np.max(np.abs(got - before.grad.numpy())) <= 1e-12


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_adamw_equals_torch_float64(weight_decay):
    rng = np.random.default_rng(2)
    p0 = rng.normal(0, 1, 257)
    p = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=0.005, betas=(0.8, 0.99), eps=1e-7, weight_decay=weight_decay)
    mine, m, v = p0.copy(), np.zeros(257), np.zeros(257)
    for t in range(1, 6):
        g = rng.normal(0, 1, 257) * 10.0 ** rng.integers(-3, 3, 257)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        mine, m, v = G.adamw(mine, g, m, v, t, lr=0.005, beta1=0.8, beta2=0.99, eps=1e-7, weight_decay=weight_decay)
        assert np.max(np.abs(mine - p.detach().numpy())) <= 1e-14, t


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_adamw_float32_restatement_is_torch_bitwise(weight_decay):
    """The float32 restatement that the GPU test compares the kernel with bit by bit is itself torch's CPU update.  The
    restatement follows torch's scalar association of ``step_size m / denom``; a vectorised CPU path may associate the update
    differently, one rounding of an update of about 1e-3, which cannot show in a parameter of 1 <= |p| < 2 more than once in
    a great while (half an ulp of p is 6e-8 or more): the parameters start there, as in the GPU test; the moments, which do
    not depend on that association, are compared too."""
    rng = np.random.default_rng(3)
    p0 = (rng.choice([-1.0, 1.0], 1000) * rng.uniform(1, 2, 1000)).astype(np.float32)
    p = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=weight_decay, foreach=False)
    mine, m, v = p0.copy(), np.zeros(1000, np.float32), np.zeros(1000, np.float32)
    for t in range(1, 4):
        g = rng.choice(np.array([0.0, 1e-20, -1e-20, 1e4, -1e4, 0.3], np.float32), 1000)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        mine, m, v = G.adamw_f32(mine, g, m, v, t, weight_decay=weight_decay)
        assert np.array_equal(mine, p.detach().numpy()), t
        assert np.array_equal(m, opt.state[p]["exp_avg"].numpy()) and np.array_equal(v, opt.state[p]["exp_avg_sq"].numpy()), t


@pytest.mark.parametrize("nx", [2, 3, 4, 6])
def test_mean5_is_self_adjoint(nx):
    """<mean5(a), b> = <a, mean5(b)>: on integers, with the five-cell sums (5 mean5), exactly."""
    rng = np.random.default_rng(nx)
    a, b = (rng.integers(-9, 10, (2, 6, nx, nx, 3)).astype(np.int64) for _ in range(2))
    assert int(np.sum(G.sum5(a) * b)) == int(np.sum(a * G.sum5(b)))
    assert np.array_equal(G.mean5(a), G.sum5(a) / 5.0)


def _golden_problem():
    from fv3net_amd.fit.graph import GraphHyperparameters

    rng = np.random.default_rng(7)
    batches = [{"a": rng.normal(0, 1, (2, 3, 6, 4, 4, 2)), "b": rng.normal(0, 1, (2, 3, 6, 4, 4))} for _ in range(4)]
    hp = GraphHyperparameters(state_variables=["a", "b"], depth=1, min_filters=4, n_epoch=3, samples_per_batch=2, multistep=2,
                              optimizer="AdamW", optimizer_kwargs={"lr": 0.005}, seed=3)
    return hp, batches[:3], batches[3:]


@pytest.mark.parametrize("backend", [None, "torch"])
def test_torch_backend_is_what_it_was(backend):
    from fv3net_amd.fit.graph import train_graph_model

    hp, train, valid = _golden_problem()
    _, arrays = train_graph_model(hp, train, valid, device="cpu", backend=backend).spec.to_arrays()
    with np.load(GOLDEN) as want:
        assert sorted(want.files) == sorted(arrays)
        for key in want.files:
            assert np.array_equal(want[key], arrays[key]) and want[key].dtype == arrays[key].dtype, key


def test_backend_refusals():
    from fv3net_amd.fit.graph import train_graph_model

    hp, train, valid = _golden_problem()
    with pytest.raises(ValueError, match="bogus"):
        train_graph_model(hp, train, valid, device="cpu", backend="bogus")
    with pytest.raises(RuntimeError, match="device"):
        train_graph_model(hp, train, valid, device="cpu", backend="hip")
    hp.optimizer = "SGD"
    with pytest.raises(NotImplementedError, match="SGD"):
        train_graph_model(hp, train, valid, device="cpu", backend="hip")
    hp.optimizer, hp.optimizer_kwargs = "AdamW", {"amsgrad": True}
    with pytest.raises(NotImplementedError, match="amsgrad"):
        train_graph_model(hp, train, valid, device="cpu", backend="hip")


def test_entry_points_check_their_arguments_before_any_hip_call():
    """Every refusal comes back from the host-side checks: no GPU is needed (the pointers are never followed)."""
    import ctypes

    from fv3net_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    a, b = ctypes.addressof(buf), ctypes.addressof(buf) + 8192
    sage = lambda **kw: lib.fv3hip_graph_sage_backward_data(*[kw.get(k, d) for k, d in (
        ("dh", a), ("dh_ld", 2), ("dh_off", 0), ("dh_ss", 0), ("ws", a), ("wn", a), ("p", None), ("p_ld", 0), ("p_off", 0), ("p_ss", 0),
        ("act", _lib.ACT_RELU), ("dst", b), ("dst_ld", 2), ("dst_off", 0), ("dst_ss", 0), ("acc", 0), ("S", 1), ("n", 2), ("ci", 2),
        ("co", 2), ("stream", None))])
    assert sage(dst=a) == _lib.EINVAL and b"overlap" in lib.fv3hip_last_error()
    assert sage(act=17) == _lib.EUNSUPPORTED
    assert sage(dh=None) == _lib.EINVAL and sage(ci=0) == _lib.EINVAL and sage(dst_ld=1) == _lib.EINVAL
    assert sage(p=b, p_ld=2) == _lib.EINVAL   # the activation behind dst must not be dst itself
    pool = lambda **kw: lib.fv3hip_graph_pool2_backward(*[kw.get(k, d) for k, d in (
        ("dpool", a), ("ld", 2), ("off", 0), ("p", None), ("p_ld", 0), ("p_off", 0), ("act", _lib.ACT_TANH), ("dst", b), ("dst_ld", 2),
        ("dst_off", 0), ("S", 1), ("n", 2), ("c", 2), ("stream", None))])
    assert pool(dst=a) == _lib.EINVAL and pool(n=3) == _lib.EINVAL and pool(act=9) == _lib.EUNSUPPORTED
    up = lambda **kw: lib.fv3hip_graph_up2_backward_data(*[kw.get(k, d) for k, d in (
        ("dcat", a), ("ld", 2), ("off", 0), ("w", a), ("p", None), ("p_ld", 0), ("p_off", 0), ("act", 0), ("dst", b), ("dst_ld", 2),
        ("dst_off", 0), ("S", 1), ("n", 1), ("ci", 2), ("co", 2), ("stream", None))])
    assert up(dst=a) == _lib.EINVAL and up(w=None) == _lib.EINVAL
    chunk = lib.fv3hip_graph_train_chunk_cells()
    assert chunk == 512
    assert lib.fv3hip_graph_sage_backward_weight_workspace_bytes(1, 8, 3, 5) == 0           # 384 cells: one chunk
    assert lib.fv3hip_graph_sage_backward_weight_workspace_bytes(1, 16, 3, 5) == 3 * 7 * 5 * 4
    assert lib.fv3hip_graph_up2_backward_weight_workspace_bytes(1, 8, 3, 5) == 1 * 4 * 20 * 4
    # a batch of more than one chunk without its workspace
    assert lib.fv3hip_graph_sage_backward_weight(a, 3, 0, 0, b, 5, 0, 0, a, a, a, 0, None, 0, 1, 16, 3, 5, None) == _lib.EINVAL
    assert b"workspace" in lib.fv3hip_last_error()
    # results that overlap each other, an input or the workspace (16 x 16: three chunks, a workspace of 3 * 7 * 5 floats)
    big = (ctypes.c_float * (6 * 256 * 8 + 4096))()
    x, g, out = ctypes.addressof(big), ctypes.addressof(big) + 4 * 6 * 256 * 3, ctypes.addressof(big) + 4 * 6 * 256 * 8
    weight = lambda **kw: lib.fv3hip_graph_sage_backward_weight(x, 3, 0, 0, g, 5, 0, 0, kw.get("dws", out), kw.get("dwn", out + 60),
                                                                 kw.get("db", out + 120), 0, kw.get("ws", out + 160), 420, 1, 16, 3, 5,
                                                                 None)
    for bad in ({"dwn": out}, {"db": out + 116}, {"ws": out + 100}, {"dws": x + 40}, {"ws": g}):
        assert weight(**bad) == _lib.EINVAL and b"overlap" in lib.fv3hip_last_error(), bad
    assert lib.fv3hip_train_adamw(a, a, a, a, 4, a, 1e-3, 0.9, 0.999, 1e-8, -1.0, None) == _lib.EINVAL
