"""The host side of the precipitative training step, without a GPU: the float64 restatement
tests/precip_train_np.py against autograd, its bound against a float32 evaluation (and against a wrong one), the torch
backend of ``fit.train_precipitative_model`` against a copy of the loop it replaced, the ``backend`` argument, and the closure
composed onto the heads' Jacobians."""
from typing import List

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
from fv3net_amd.fit.dense import _stack_for_training
from oracle import mlp_np

REGULARIZERS = {"none": (0.0, 0.0), "l1": (0.01, 0.0), "l2": (0.0, 0.01), "l1_l2": (0.01, 0.02)}


# ---- the restatement against autograd --------------------------------------------------------------------------------------------
def _autograd(a, couple, has_dead, l1, l2):
    """The loss expression of the torch loop of ``fit.train_precipitative_model`` on the raw head outputs, in float64.  The
    loop's ``torch.mean`` divides by ``n nz`` (and ``n``); the kernel multiplies by the float32 value of the reciprocal, which
    is part of its definition, so the mean is written as ``sum * float32(1 / count)`` here.  ``/ lstd`` squared is ``* inv``."""
    n, nz = a["yhat"].shape[0], a["scale1"].shape[0]
    y = torch.tensor(a["yhat"].astype(np.float64), requires_grad=True)
    t64 = lambda v: torch.tensor(np.asarray(v, np.float64))   # noqa: E731
    heads = [y[:, :nz], y[:, nz:2 * nz]] + ([y[:, 2 * nz:2 * nz + 1]] if has_dead else [])
    cp_raw = y[:, 2 * nz + int(has_dead):]
    t_tend = heads[0] * t64(a["scale1"]) + t64(a["center1"])
    q_tend = heads[1] * t64(a["scale2"]) + t64(a["center2"])
    col_precip = cp_raw * t64(a["scale2"]) + t64(a["center2"])
    if couple:
        t_tend = t_tend + float(P.C_HEAT) * col_precip
        q_tend = q_tend + col_precip
    precip = t64(a["pp"]) + float(P.C_G) * torch.sum(col_precip * t64(a["delp"]), dim=1)
    w12, w3 = (float(w) for w in PT.weights(n, nz))
    loss = torch.sum((t_tend - t64(a["t1"])) ** 2 * t64(a["inv1"])) * w12 + torch.sum((q_tend - t64(a["t2"])) ** 2 * t64(a["inv2"])) * w12 + \
        torch.sum((precip - t64(a["t3"])) ** 2 * float(np.float32(a["inv3"]))) * w3
    if l1 or l2:
        for out in heads:
            loss = loss + (float(np.float32(l1)) * out.abs().sum() + float(np.float32(l2)) * (out * out).sum()) / n
    loss.backward()
    return y.grad.numpy(), float(loss.detach())


@pytest.mark.parametrize("kind", sorted(REGULARIZERS))
@pytest.mark.parametrize("couple", [True, False])
def test_restatement_is_the_gradient_of_the_loops_loss(couple, kind):
    l1, l2 = REGULARIZERS[kind]
    has_dead = kind != "none"
    a = C.launch_inputs(5, 3, has_dead=has_dead, seed=7)
    dy, loss, _, _, _ = PT.loss_grad(*C.reference_args(a), couple=couple, has_dead=has_dead, l1=l1, l2=l2)
    want, want_loss = _autograd(a, couple, has_dead, l1, l2)
    assert dy.shape == want.shape == (5, 9 + int(has_dead))
    assert np.max(np.abs(dy - want)) <= 1e-12 * np.max(np.abs(want))
    for block in (slice(0, 3), slice(3, 6), slice(6 + int(has_dead), None)):   # each head on its own scale
        assert np.max(np.abs(dy[:, block] - want[:, block])) <= 1e-12 * np.max(np.abs(want[:, block]))
    assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
    if has_dead:
        assert np.all(dy[:, 6] != 0), "the dead head is reached by the regulariser"


def test_restatement_row_table_convention():
    a = C.launch_inputs(4, 3, rows=6, seed=1)
    idx = np.array([5, 0, 6, 5])
    dy, loss, bound, _, pred = PT.loss_grad(*C.reference_args(a), idx=idx)
    picked = dict(a, delp=a["delp"][[5, 0, 0, 5]], pp=a["pp"][[5, 0, 0, 5]], t1=a["t1"][[5, 0, 0, 5]], t2=a["t2"][[5, 0, 0, 5]],
                  t3=a["t3"][[5, 0, 0, 5]])
    want, _, _, _, _ = PT.loss_grad(*C.reference_args(picked))
    assert np.array_equal(dy[[0, 1, 3]], want[[0, 1, 3]])
    assert np.all(np.isnan(dy[2])) and np.isnan(loss) and np.all(np.isfinite(dy[[0, 1, 3]]))
    cp = a["yhat"][2, 6:].astype(np.float64) * a["scale2"] + a["center2"]
    assert pred["precip"][2] == 0.0 and np.array_equal(pred["dq2"][2], a["yhat"][2, 3:6].astype(np.float64) * a["scale2"] + a["center2"] + cp)


# ---- a float32 evaluation against the bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("couple,kind", [(True, "none"), (False, "none"), (True, "l1_l2")])
def test_float32_evaluation_lies_inside_the_bound_and_a_wrong_one_outside(couple, kind):
    l1, l2 = REGULARIZERS[kind]
    has_dead = kind != "none"
    a = C.launch_inputs(64, 79, has_dead=has_dead, seed=3)
    dy, loss, bound, loss_bound, _ = PT.loss_grad(*C.reference_args(a), couple=couple, has_dead=has_dead, l1=l1, l2=l2)
    got, got_loss = PT.loss_grad32(*C.reference_args(a), couple=couple, has_dead=has_dead, l1=l1, l2=l2)
    frac = np.abs(got - dy) / bound
    print(f"float32 numpy: {frac.max():.3f} of the gate; the gate is {np.max(bound) / np.max(np.abs(dy)):.1e} of the largest entry; "
          f"loss {abs(got_loss - loss) / loss_bound:.3f} of its gate")
    assert frac.max() <= 1.0 and abs(got_loss - loss) <= loss_bound
    wrong, _ = PT.loss_grad32(*C.reference_args(a), couple=couple, has_dead=has_dead, l1=l1, l2=l2, drop_integral_term=True)
    cp = slice(2 * 79 + int(has_dead), None)
    outside = np.abs(wrong - dy)[:, cp] > bound[:, cp]
    print(f"without (c_g delp) g3: {outside.mean():.3f} of the column-precipitation entries are outside the gate")
    assert outside.mean() > 0.99
    assert np.array_equal(wrong[:, :cp.start], got[:, :cp.start])


# ---- the torch backend is unchanged -----------------------------------------------------------------------------------------------
def _loop_before_the_split(hp, train_batches):
    """``train_precipitative_model`` as it stood before it had backends (PyTorch on the CPU), kept here to pin the torch backend."""
    torch.manual_seed(hp.seed)
    dev = torch.device("cpu")
    names_in, names_out = hp.input_variables, hp.output_variables
    X = _stack_for_training(train_batches, names_in, hp.unstacked_dims)
    y = _stack_for_training(train_batches, names_out, hp.unstacked_dims)
    nfit = hp.normalization_fit_samples
    Xc = [a[..., hp.clip[n]] if n in hp.clip else a for a, n in zip(X, names_in)]
    x_mean = [a[:nfit].mean(axis=0).astype(np.float32) for a in Xc]
    x_std = [a[:nfit].std(axis=0).astype(np.float32) for a in Xc]
    y_mean = [a[:nfit].mean(axis=0).astype(np.float32) for a in y]
    y_std = [a[:nfit].std(axis=0).astype(np.float32) for a in y]
    loss_std = [np.std(a[:nfit], axis=0, dtype=np.float32) for a in y]
    eps = np.float32(1e-7)
    xin = torch.from_numpy(np.concatenate([(a - m) / (s + eps) for a, m, s in zip(Xc, x_mean, x_std)], axis=1)).to(dev)
    delp = torch.from_numpy(X[names_in.index(fp.DELP_NAME)]).to(dev)
    physics_precip = torch.from_numpy(X[names_in.index(fp.PHYS_PRECIP_NAME)][:, 0]).to(dev)
    layers: List[torch.nn.Module] = []
    fan = xin.shape[1]
    for _ in range(hp.depth - 1):
        lin = torch.nn.Linear(fan, hp.width)
        torch.nn.init.xavier_uniform_(lin.weight)
        torch.nn.init.zeros_(lin.bias)
        layers += [lin, torch.nn.ReLU()]
        fan = hp.width
    trunk = torch.nn.Sequential(*layers).to(dev)
    heads = torch.nn.ModuleList()
    for nfeat in [a.shape[1] for a in y] + [y[1].shape[1]]:
        lin = torch.nn.Linear(fan, nfeat)
        torch.nn.init.xavier_uniform_(lin.weight)
        torch.nn.init.zeros_(lin.bias)
        heads.append(lin)
    heads = heads.to(dev)
    targets = [torch.from_numpy(a).to(dev) for a in y]
    targets[2] = targets[2][:, 0]
    t_mean = [torch.from_numpy(m).to(dev) for m in y_mean]
    t_std = [torch.from_numpy(s).to(dev) for s in y_std]
    t_lstd = [torch.from_numpy(np.maximum(s, 1e-12)).to(dev) for s in loss_std]
    t_lstd[2] = t_lstd[2][0]
    c_heat, c_g = float(np.float32(-fp.LV / fp.CPD)), float(np.float32(-1.0 / fp.GRAVITY))
    opt = torch.optim.Adam(list(trunk.parameters()) + list(heads.parameters()), lr=hp.learning_rate)
    n = xin.shape[0]
    g = torch.Generator().manual_seed(hp.seed)
    for _ in range(hp.epochs):
        perm = torch.randperm(n, generator=g).to(dev)
        for i in range(0, n, hp.batch_size):
            idx = perm[i:i + hp.batch_size]
            hidden = trunk(xin[idx])
            t_tend = heads[0](hidden) * t_std[0] + t_mean[0]
            q_tend = heads[1](hidden) * t_std[1] + t_mean[1]
            col_precip = heads[3](hidden) * t_std[1] + t_mean[1]
            if hp.couple_precip_to_dQ1_dQ2:
                t_tend = t_tend + c_heat * col_precip
                q_tend = q_tend + col_precip
            precip = physics_precip[idx] + c_g * torch.sum(col_precip * delp[idx], dim=1)
            loss = 0.0
            for pred, j in ((t_tend, 0), (q_tend, 1), (precip, 2)):
                loss = loss + torch.mean(((pred - targets[j][idx]) / t_lstd[j]) ** 2)
            opt.zero_grad()
            loss.backward()
            opt.step()
    lin_layers = [m for m in trunk if isinstance(m, torch.nn.Linear)]
    live = [heads[0], heads[1], heads[3]]
    return fit.precipitative_spec_from_arrays(
        names_in, x_mean, x_std,
        [m.weight.detach().cpu().numpy().T.copy() for m in lin_layers], [m.bias.detach().cpu().numpy().copy() for m in lin_layers],
        [h.weight.detach().cpu().numpy().T.copy() for h in live], [h.bias.detach().cpu().numpy().copy() for h in live],
        y_mean[:2], y_std[:2], clip=hp.clip)


def same_spec(a, b):
    (ma, aa), (mb, ab) = a.to_arrays(), b.to_arrays()
    return ma == mb and aa.keys() == ab.keys() and all(np.array_equal(aa[k], ab[k]) for k in aa)


SMALL = dict(nz=7, ny=6, nx=11)   # 66 columns: two full batches of 24 and one of 18


def small_hyper(**kw):
    args = dict(width=6, depth=3, epochs=2, batch_size=24, learning_rate=1e-2, seed=3)
    args.update(kw)
    return fit.PrecipitativeHyperparameters(**args)


@pytest.mark.parametrize("kw", [{}, {"couple_precip_to_dQ1_dQ2": False, "clip": {C.T_NAME: slice(2, None)}}], ids=["default", "uncoupled-clipped"])
def test_torch_backend_returns_what_the_loop_returned(kw):
    want = _loop_before_the_split(small_hyper(**kw), C.batches(**SMALL))
    for backend in (None, "torch"):
        got = fit.train_precipitative_model(small_hyper(**kw), C.batches(**SMALL), device="cpu", backend=backend)
        assert same_spec(got.spec, want)
    assert fit.PrecipitativeHyperparameters().residual_regularizer is None
    none = fit.train_precipitative_model(small_hyper(residual_regularizer=("none", {}), **kw), C.batches(**SMALL), device="cpu")
    assert same_spec(none.spec, want), "'none' is no regulariser"


def test_regulariser_is_honoured_by_the_torch_backend():
    plain = fit.train_precipitative_model(small_hyper(), C.batches(**SMALL), device="cpu")
    reg = fit.train_precipitative_model(small_hyper(residual_regularizer=("l2", {"l2": 0.5})), C.batches(**SMALL), device="cpu")
    assert not same_spec(plain.spec, reg.spec)
    assert [o.name for o in reg.spec.outputs] == list(fp.HEAD_NAMES), "the dead head is dropped on export"
    heads = slice(0, 2 * SMALL["nz"])   # the regularised heads shrink
    assert np.linalg.norm(reg.spec.out_kernel[:, heads]) < np.linalg.norm(plain.spec.out_kernel[:, heads])


def test_regulariser_coefficients():
    assert fp.regularizer_coefficients(None) == (0.0, 0.0, False)
    assert fp.regularizer_coefficients(("none", {})) == (0.0, 0.0, False)
    assert fp.regularizer_coefficients(("l1", {})) == (0.01, 0.0, True)
    assert fp.regularizer_coefficients(("l2", {"l2": 0.3})) == (0.0, 0.3, True)
    assert fp.regularizer_coefficients(("l1_l2", {"l1": 0.2})) == (0.2, 0.01, True)
    for bad in (("l3", {}), ("l1", {"l2": 0.1}), ("l2", {"l2": -1.0})):
        with pytest.raises(ValueError):
            fp.regularizer_coefficients(bad)


# ---- backend validation -------------------------------------------------------------------------------------------------------------
def test_backend_is_validated():
    with pytest.raises(ValueError, match="backend"):
        fit.train_precipitative_model(small_hyper(), C.batches(**SMALL), backend="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fit.train_precipitative_model(small_hyper(), C.batches(**SMALL), device="cpu", backend="hip")


# ---- the Jacobian composition ---------------------------------------------------------------------------------------------------------
def _hand_built_model(couple, nz=5):
    args = PC.arrays_for_spec(nz=nz, width=6, depth=3, clip={C.T_NAME: slice(1, None)}, seed=4)
    rng = np.random.default_rng(8)   # centres off the profile, so that hidden units are on
    args["input_means"] = [m + (0.5 * s * rng.normal(0, 1, s.shape[0])).astype(np.float32) for m, s in zip(args["input_means"], args["input_stds"])]
    spec = fit.precipitative_spec_from_arrays(**args)
    return fit.HipPrecipitativeModel(PC.NAMES_IN, PC.NAMES_OUT, spec, couple_precip_to_dQ1_dQ2=couple)


@pytest.mark.parametrize("couple", [True, False])
def test_closure_is_composed_onto_the_head_jacobians(couple, monkeypatch):
    nz = 5
    model = _hand_built_model(couple, nz)
    profile = {k: v.mean(axis=0) for k, v in PC.state(16, nz, seed=2).items()}
    profile[P.PHYS_PRECIP] = np.atleast_1d(profile[P.PHYS_PRECIP])
    head_jac, head_bound = T.predict_jacobians(model.spec, profile)
    cp = mlp_np.forward(model.spec, {k: v[None] for k, v in profile.items()}, dtype=np.float64)[P.COL_PRECIP][0]
    monkeypatch.setattr(model, "_head_jacobians", lambda profiles: (head_jac, cp))   # (the device call)
    got = model.jacobians(profile)
    want, _ = PT.compose_jacobians(head_jac, head_bound, cp, np.zeros(nz), profile[P.DELP], couple)
    assert set(got) == set(PC.NAMES_OUT)
    for o in PC.NAMES_OUT:
        assert set(got[o]) == set(PC.NAMES_IN)
        for i in PC.NAMES_IN:
            assert got[o][i].shape == (1 if o == P.PRECIP else nz, 1 if i == P.PHYS_PRECIP else nz) and got[o][i].dtype == np.float64
            np.testing.assert_allclose(got[o][i], want[o][i], rtol=1e-14, atol=0)
    assert np.all(got["dQ1"][C.T_NAME][:, 0] == 0) and np.all(got[P.PRECIP][C.T_NAME][:, 0] == 0), "level 0 of T is clipped away"
    assert np.any(got[P.PRECIP][C.T_NAME][:, 1:] != 0)
    if not couple:
        assert all(np.array_equal(got["dQ1"][i], head_jac["dQ1"][i]) for i in PC.NAMES_IN)

    # and against the graph itself: central differences of the float64 predict graph.  The network is piecewise linear and the
    # closure bilinear, so a central difference is exact but for rounding (2^-53 |f| / h, h = 2^-12 |x|: under 1e-11 relative)
    # unless a ReLU turns within the step; steps are taken between float32 values, as the graph casts its inputs.
    def run(p):
        out = P.forward(model.spec, couple, {k: np.asarray(v, np.float64)[None] for k, v in p.items()}, dtype=np.float64)
        return {o: np.atleast_1d(out[o][0]) for o in PC.NAMES_OUT}

    base = {k: np.asarray(v).astype(np.float32).astype(np.float64) for k, v in profile.items()}
    for i in PC.NAMES_IN:
        for col in range(base[i].shape[0]):
            up, down = {k: v.copy() for k, v in base.items()}, {k: v.copy() for k, v in base.items()}
            h = abs(base[i][col]) * 2.0 ** -12
            up[i][col] = np.float32(base[i][col] + h)
            down[i][col] = np.float32(base[i][col] - h)
            fu, fd = run(up), run(down)
            for o in PC.NAMES_OUT:
                fdiff = (fu[o] - fd[o]) / (up[i][col] - down[i][col])
                scale = np.max(np.abs(got[o][i])) + 1e-300
                assert np.max(np.abs(fdiff - got[o][i][:, col])) <= 1e-6 * scale, (o, i, col)
