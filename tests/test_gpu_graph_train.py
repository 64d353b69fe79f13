"""``GraphTrainer`` and ``fit.train_graph_model(backend="hip")`` on the device.

The first-step gradients of the whole network are compared with the float64 restatement ``graph_train_np.network_gradients``
(which tests/test_host_graph_train.py holds to 1e-12 of ``torch.autograd`` on the float64 twin), within the layer gates carried
through the layers as tests/test_gpu_conv_train.py carries them: an operand known to within E adds ``E |W|``; an element whose
mask is decided by an activation within that activation's own bound counts in full.  A depth-2 network halves the cube twice,
so its second grid is nx = 20 (18 is not a multiple of 4): 16 x 16 tiles with a rim at level 0, 10 and 5 cells below.
Such a worst-case bound compounds through every layer forwards and backwards: only at depth 1 and multistep 1 is it below the
gradient itself (observed there: at most 5.9e-6 of it); at depth 2 or multistep 2 it exceeds the gradient by orders of magnitude
and by itself would pass a zero or sign-flipped gradient.  It is kept as the issue states it; what checks the values in every
case, multistep 2 included, is ``test_every_layer_of_every_rollout_step_is_within_its_own_gate`` below, with the per-layer
gates of tests/test_gpu_graph_train_layers.py.
"""
import numpy as np
import pytest
import torch

import graph_cases
import graph_train_np as G

pytestmark = pytest.mark.gpu


def _trainer(spec, samples, device, **kw):
    from fv3net_amd.graph_train import GraphTrainer

    return GraphTrainer(spec, samples, device=device, **kw)


def _layers(spec):
    import dataclasses

    return {name: tuple(getattr(layer, f.name) for f in dataclasses.fields(layer)) for name, layer in spec.layers.items()}


def _case(nx, depth, multistep, activation="relu", n_samples=3, seed=0):
    rng = np.random.default_rng(seed + nx)
    spec = graph_cases.make_spec(rng, {"a": 2, "b": 1}, depth=depth, min_filters=4, activation=activation)
    samples = rng.normal(0, 1, (n_samples, multistep + 1, 6, nx, nx, 3)).astype(np.float32)
    return spec, samples


@pytest.mark.parametrize("multistep", [1, 2])
@pytest.mark.parametrize("nx,depth,activation", [(4, 1, "relu"), (4, 2, "relu"), (18, 1, "relu"), (20, 2, "relu"), (4, 1, "tanh")])
def test_first_step_gradients(device, nx, depth, activation, multistep):
    spec, samples = _case(nx, depth, multistep, activation)
    trainer = _trainer(spec, samples, device, multistep=multistep, max_batch=2)
    idx = np.array([2, 0])
    trainer.backward(torch.from_numpy(idx).to(device))
    want_loss, want, bounds, _, _ = G.network_gradients(_layers(spec), depth, 4, activation, samples[idx], multistep)
    got = trainer.gradients()
    worst = 0.0
    for name in want:
        for a, b, e in zip(got[name], want[name], bounds[name]):
            assert np.all(np.isfinite(a)) and np.any(a != 0), name
            frac = float(np.max(np.abs(a.astype(np.float64) - b) / e))
            worst = max(worst, frac)
            assert frac <= 1.0, (name, frac)
    loss = trainer.loss()
    print(f"nx {nx} depth {depth} {activation} multistep {multistep}: worst gradient {worst:.2e} of its composed gate; "
          f"loss {loss:.6f} against {want_loss:.6f}")
    assert abs(loss - want_loss) <= 1e-4 * want_loss


def _check_rollout_step(trainer, k, K, A, D, W, dW, state, target, later, activation, fractions):
    """Every buffer that ``_backward_step(k)`` wrote against the restatement of ITS layer applied to the device's own float32
    inputs of that layer.  ``later``: ``(D, dW)`` as step k + 1 left them (None at the last step): the loss gradient then holds
    step k + 1's gradient into the state as well, and every parameter gradient is that step's plus this one's."""
    depth, m, nx = trainer.depth, trainer.m, trainer.n

    def check(name, got, want, gate):
        assert np.all(np.isfinite(got)), name
        fractions[f"step {k} {name}"] = frac = float(np.max(np.abs(np.asarray(got, np.float64) - want) / gate))
        assert frac <= 1.0, (k, name, frac)

    def parameter(name, i, want, gate):
        if later is not None:   # old + new: one more rounding
            want = later[1][name][i].astype(np.float64) + want
            gate = gate + 2 * G.U * np.abs(want)
        assert np.any(dW[name][i] != 0), (k, name)
        check(f"{name}[{i}]", dW[name][i], want, gate)

    def sage(name, x, g, p=None, dx=None):
        dws, dwn, db, gs, gn, gb = G.sage_backward_weight(x, g)
        for i, (want, gate) in enumerate(zip((dws, dwn, db), (gs, gn, gb))):
            parameter(name, i, want, gate)
        if dx is not None:
            want, gate = G.sage_backward_data(g, W[name][0], W[name][1], p, activation if p is not None else "linear")
            check(f"{name}.data", dx, want, gate)

    wnorm = float(np.float32(1.0 / (2 * 6 * nx * nx * 3 * K)))
    want = 2.0 * (A["y"] - target) * wnorm
    gate = 8 * G.U * (np.abs(A["y"]) + np.abs(target)) * 2 * wnorm + G.TINY
    if later is not None:   # step k + 1's gradient into the state, added to the loss's before `last` is differentiated
        d_state, g_state = G.sage_backward_data(later[0]["x0"], W["first"][0], W["first"][1])
        assert np.any(d_state != 0)
        want = want + d_state
        gate = gate + g_state + 2 * G.U * np.abs(want)
    check("loss gradient (+ the state gradient)", D["y"], want, gate)
    sage("last", A["low.0"], D["y"], A["low.0"], D["low.0"])
    raw = {}
    for lev in range(depth):
        c = m * 2 ** lev
        t2, cat, below = f"t2.{lev}", f"cat.{lev}", (f"low.{lev + 1}" if lev + 1 < depth else "low.b")
        sage(f"L{lev}.conv2b", A[t2], D[f"low.{lev}"], A[t2], D[t2])
        sage(f"L{lev}.conv2a", A[cat], D[t2])
        want, gate = G.sage_backward_data(D[t2], W[f"L{lev}.conv2a"][0], W[f"L{lev}.conv2a"][1])
        raw[lev] = (want[..., :2 * c], gate[..., :2 * c])
        dup = D[cat][..., 2 * c:]
        check(f"L{lev}.conv2a.data (the up half)", dup, want[..., 2 * c:], gate[..., 2 * c:])
        dw, db, gw, gb = G.up2_backward_weight(A[below], dup)
        parameter(f"L{lev}.up", 0, dw, gw)
        parameter(f"L{lev}.up", 1, db, gb)
        want, gate = G.up2_backward_data(dup, W[f"L{lev}.up"][0], A[below], activation)
        check(f"L{lev}.up.data", D[below], want, gate)
    x = f"pool.{depth - 1}"
    sage("bottom.b", A["t.b"], D["low.b"], A["t.b"], D["t.b"])
    sage("bottom.a", A[x], D["t.b"], None, D[x])
    for lev in reversed(range(depth)):
        c = m * 2 ** lev
        t1, cat = f"t1.{lev}", f"cat.{lev}"
        before, g_before = A[cat][..., :2 * c], D[cat][..., :2 * c]
        want, gate = G.pool2_backward(raw[lev][0], D[f"pool.{lev}"], before, activation)
        check(f"L{lev}.pool backward", g_before, want, gate + raw[lev][1])
        x = f"pool.{lev - 1}" if lev else "x0"
        sage(f"L{lev}.conv1b", A[t1], g_before, A[t1], D[t1])
        sage(f"L{lev}.conv1a", A[x], D[t1], A[x] if lev == 0 else None, D[x])
    sage("first", state, D["x0"])


@pytest.mark.parametrize("multistep", [1, 2])
@pytest.mark.parametrize("nx,depth,activation", [(4, 1, "relu"), (4, 2, "relu"), (18, 1, "relu"), (20, 2, "relu"), (4, 1, "tanh")])
def test_every_layer_of_every_rollout_step_is_within_its_own_gate(device, nx, depth, activation, multistep):
    """The tight form of the test above, on the same cases: the rollout is driven step by step as ``backward`` drives it (the
    batch staged, every step's forwards, then ``_backward_step(k)`` for k = multistep - 1 ... 0) and after every step every
    gradient buffer and every parameter gradient is compared with the restatement of ITS layer applied to the device's own
    float32 inputs of that layer, within that layer's gate (tests/test_gpu_graph_train_layers.py's).  Nothing compounds, so a
    wrong buffer, mask, sign, order of the skip connection's two parts, a missing state gradient or a weight gradient that is
    written where it should be accumulated shows.  The loss gradient's gate is section 21's, ``8 2^-24 (|y| + |t|) 2 wnorm``;
    the pool's backward adds the gate of conv2a's unmasked data gradient that it reads; a sum of two gated terms adds one
    rounding each way.  The forward wiring is checked the same way (``first`` of step k on the state step k reads, and the
    targets through the loss), and ``backward`` itself must give the same bits as the steps driven here."""
    spec, samples = _case(nx, depth, multistep, activation)
    trainer = _trainer(spec, samples, device, multistep=multistep, max_batch=2)
    idx, K, S = np.array([1, 2]), multistep, 2
    dev_idx = torch.from_numpy(idx).to(device)
    host = lambda slices: {key: v.tensor.cpu().numpy().astype(np.float64) for key, v in slices.items()}
    batch = samples[idx].astype(np.float64)
    W = trainer.parameters()
    torch.index_select(trainer.samples, 0, dev_idx, out=trainer._batch[:S])
    for k in range(K):
        trainer._forward(k, S)
    acts = [host(a) for a in trainer._act]
    states = [batch[:, 0]] + [a["y"] for a in acts[:-1]]
    fractions, later = {}, None
    for k in range(K):
        want, gate = G.sage_forward(states[k], np.zeros_like(states[k]), W["first"], activation)
        frac = float(np.max(np.abs(acts[k]["x0"] - want) / (gate + G.TINY)))
        fractions[f"step {k} first forward"] = frac
        assert frac <= 1.0, (k, frac)
    for k in reversed(range(K)):
        trainer._backward_step(k, S)
        D, dW = host(trainer._d), trainer.gradients()
        _check_rollout_step(trainer, k, K, acts[k], D, W, dW, states[k], batch[:, k + 1], later, activation, fractions)
        later = (D, dW)
    driven = trainer.grads.clone()
    loss = trainer.loss()
    trainer.grads.fill_(float("nan"))
    trainer.backward(dev_idx)
    assert torch.equal(trainer.grads, driven) and trainer.loss() == loss
    worst = max(fractions, key=fractions.get)
    print(f"nx {nx} depth {depth} {activation} multistep {multistep}: {len(fractions)} buffers, worst {fractions[worst]:.3f} of its "
          f"gate ({worst})")


def _state(trainer):
    return [t.clone() for t in (trainer.params, trainer.mom, trainer.var, trainer.step_count)]


def test_the_same_step_twice_is_bitwise_equal(device):
    spec, samples = _case(18, 1, 2)
    trainer = _trainer(spec, samples, device, multistep=2, max_batch=2)
    idx = torch.tensor([1, 2], device=device)
    before = _state(trainer)
    trainer.step(idx)
    first = _state(trainer)
    assert not torch.equal(first[0], before[0]) and int(first[3].cpu()[0]) == 1
    for t, b in zip((trainer.params, trainer.mom, trainer.var, trainer.step_count), before):
        t.copy_(b)
    trainer.grads.fill_(float("nan"))   # nothing of the last step may be read
    trainer.step(idx)
    for a, b in zip(_state(trainer), first):
        assert torch.equal(a, b)


def test_replays_of_a_captured_step_equal_eager_steps(device):
    spec, samples = _case(6, 1, 2, n_samples=4)
    batches = [[0, 1], [3, 2], [1, 3], [2, 0]]
    eager = _trainer(spec, samples, device, multistep=2, max_batch=2)
    for b in batches:
        eager.step(torch.tensor(b, device=device))
    replayed = _trainer(spec, samples, device, multistep=2, max_batch=2)
    idx = torch.tensor(batches[0], device=device)
    graph = replayed.capture(idx)          # (the eager step it takes first is the first batch)
    for b in batches[1:]:
        idx.copy_(torch.tensor(b, device=device))
        graph.replay()
    torch.cuda.synchronize(device)
    for a, b in zip(_state(replayed), _state(eager)):
        assert torch.equal(a, b)
    assert int(replayed.step_count.cpu()[0]) == 4 and replayed.loss() == eager.loss()


def _flip_problem():
    rng = np.random.default_rng(0)
    return graph_cases.flip_series(rng, 20, 2, 2, 6, 2), graph_cases.flip_series(rng, 3, 2, 2, 6, 2), graph_cases.flip_series(rng, 1, 1, 100, 6, 2)[0]


def _loss_of(predictor, batches):
    """The one-step MSE of the normalised state on the float64 twin, on the CPU: one measure for both backends."""
    from fv3net_amd.fit.graph import _multistep_loss, _normalised_samples, twin_from_spec

    scalers = {v.name: (v.mean if v.nfeat > 1 else v.mean[0], v.std if v.nfeat > 1 else v.std[0]) for v in predictor.spec.variables}
    x = _normalised_samples(batches, ["a", "b"], scalers).double()
    with torch.no_grad():
        return float(_multistep_loss(twin_from_spec(predictor.spec, torch.float64), x, 1))


def test_no_epochs_give_the_torch_backends_spec(device):
    from fv3net_amd.fit.graph import GraphHyperparameters, train_graph_model

    train, valid, _ = _flip_problem()
    hp = GraphHyperparameters(state_variables=["a", "b"], n_epoch=0, seed=2, min_filters=8, activation="tanh")
    a = train_graph_model(hp, train[:2], valid[:1], device=str(device), backend="hip").spec.to_arrays()
    b = train_graph_model(hp, train[:2], valid[:1], device="cpu", backend="torch").spec.to_arrays()
    assert a[0] == b[0] and sorted(a[1]) == sorted(b[1])
    for key in a[1]:
        assert np.array_equal(a[1][key], b[1][key]), key


EPOCHS = 5


@pytest.fixture(scope="module")
def flip_models(device):
    """The known-answer problem (graph/test_graph.py:64-103) for EPOCHS epochs: the torch backend on the CPU at seeds 0 .. 4,
    the hip backend at seed 0 and at seed 2 (the seed tests/test_host_graph.py fixes), and the untrained network of seed 2."""
    from fv3net_amd.fit.graph import GraphHyperparameters, train_graph_model

    train, valid, test = _flip_problem()
    hp = lambda seed, epochs=EPOCHS: GraphHyperparameters(state_variables=["a", "b"], n_epoch=epochs, optimizer_kwargs={"lr": 0.005}, seed=seed)
    torch_models = [train_graph_model(hp(seed), train, valid, device="cpu") for seed in range(5)]
    hip = {seed: train_graph_model(hp(seed), train, valid, device=str(device), backend="hip") for seed in (0, 2)}
    start = train_graph_model(hp(2, 0), train, valid, device=str(device), backend="hip")
    return train, test, torch_models, hip, start


def test_known_answer_problem_trains_as_the_torch_backend_does(flip_models):
    """The training loss falls, and after the same number of epochs the hip backend's loss at seed 0 lies within the torch
    backend's seed spread (max - min over seeds 0 .. 4) of the torch backend's loss at seed 0.  The threshold is a measured
    margin, not a derived one: DESIGN.md section 24 records the losses and the spread."""
    train, _, torch_models, hip, start = flip_models
    torch_losses = [_loss_of(p, train) for p in torch_models]
    spread = max(torch_losses) - min(torch_losses)
    hip0, hip2, start2 = _loss_of(hip[0], train), _loss_of(hip[2], train), _loss_of(start, train)
    print(f"{EPOCHS} epochs: torch backend, seeds 0 .. 4: {', '.join(f'{v:.5f}' for v in torch_losses)} (spread {spread:.5f}); "
          f"hip backend, seed 0: {hip0:.5f}; seed 2: {start2:.5f} -> {hip2:.5f}")
    assert hip2 < start2
    assert abs(hip0 - torch_losses[0]) <= spread


def test_trained_model_predicts_and_survives_dump_and_load(flip_models, tmp_path, device):
    from fv3net_amd import fit
    from fv3net_amd.xr_compat import DataArray, Dataset

    _, test, _, hip, _ = flip_models
    predictor = hip[2]
    ds = Dataset({"a": DataArray(test["a"][0][:9], dims=("time", "tile", "x", "y", "z")),
                  "b": DataArray(test["b"][0][:9], dims=("time", "tile", "x", "y"))})
    predicted, reference = predictor.predict(ds, 1)
    fit.dump(predictor, str(tmp_path / "model"))
    again, _ = fit.load(str(tmp_path / "model")).predict(ds, 1)
    for name in ("a", "b"):
        got = predicted[name].values
        assert got.shape[:2] == (8, 2) and np.all(np.isfinite(got))
        assert np.array_equal(got, again[name].values)
        err = reference[name].values[:, 1] - got[:, 1]
        print(f"{name}: one-step rmse after {EPOCHS} epochs {np.sqrt(np.mean(err ** 2)):.4f}")
