"""Reservoir training on the device against the numpy restatement (tests/reservoir_train_np.py):
the Gram sums of ``csrc/gram.hip`` with their derived gate and bitwise properties, the training series of
``fv3hip_reservoir_train_series``, the solve, and ``train_reservoir_model`` end to end.

Gates.  Gram sums, per element: ``2 (T + 2) 2^-53 sum_t |x_ti| |x_tj|`` (the bound of a T-term inner product in any order;
numpy's product obeys it too, hence the 2).  Series: the chained-step gate of section 12, 1e-12 absolute.  Solve: the
backward error against ``np.linalg.solve``'s on the same sums, 16 x that or ``J1 2^-52``.  End to end, relative to the
restatement's weights: ``kappa (eps_A + eps_B) / (1 - kappa eps_A) + J1 2^-52 kappa`` with ``kappa = cond_2(A + l2 I)`` and
``eps`` the Gram gates relative to ``||A||`` and ``||B||``.  Every test prints its worst fraction of its gate."""
import numpy as np
import pytest
import torch

import reservoir_cases as C
import reservoir_np as R
import reservoir_train_np as T

pytestmark = pytest.mark.gpu

EPS53 = 2.0 ** -53


def _accumulator(n_sub, J, n_out, bias, device):
    from fv3net_amd.reservoir import GramAccumulator

    return GramAccumulator(n_sub, J, n_out, add_bias=bias, device=device)


def _with_bias(X, bias):
    return np.concatenate([X, np.ones(X.shape[:-1] + (1,))], axis=-1) if bias else X


def gram_want(X, Y, bias, t_total=None):
    """(A, B, gate of A, gate of B) per subdomain from [t, subdomain, feature] arrays, in numpy float64."""
    X1 = _with_bias(X, bias)
    n = X.shape[0] if t_total is None else t_total
    with np.errstate(invalid="ignore"):
        A = np.stack([X1[:, s].T @ X1[:, s] for s in range(X.shape[1])])
        B = np.stack([X1[:, s].T @ Y[:, s] for s in range(X.shape[1])])
        bound = 2 * (n + 2) * EPS53
        gA = bound * np.stack([np.abs(X1[:, s]).T @ np.abs(X1[:, s]) for s in range(X.shape[1])])
        gB = bound * np.stack([np.abs(X1[:, s]).T @ np.abs(Y[:, s]) for s in range(X.shape[1])])
    return A, B, gA, gB


def _get(acc):
    a, b = acc.get()
    return a.cpu().numpy(), b.cpu().numpy()


# J x bias over the tile edges 16 and 64 of J1; n_out, T and n_sub cycle through their lists so that each value occurs
_J = (1, 14, 15, 16, 63, 64, 65, 129)
_N_OUT, _T, _N_SUB = (1, 9, 18, 65), (1, 3, 4, 5, 67), (1, 6, 33)
GRAM_CASES = [(J, bias, _N_OUT[i % 4], _T[i % 5], _N_SUB[i % 3])
              for i, (J, bias) in enumerate((J, bias) for J in _J for bias in (True, False))]


def test_gram_cases_cover_the_listed_shapes():
    assert {c[2] for c in GRAM_CASES} == set(_N_OUT) and {c[3] for c in GRAM_CASES} == set(_T)
    assert {c[4] for c in GRAM_CASES} == set(_N_SUB)
    assert {c[0] + c[1] for c in GRAM_CASES} >= {15, 16, 17, 63, 64, 65, 66}


@pytest.mark.parametrize("J,bias,n_out,n_t,n_sub", GRAM_CASES)
def test_gram_update_matches_numpy(device, J, bias, n_out, n_t, n_sub):
    rng = np.random.RandomState(C._seed("gram", J, bias))
    X, Y = rng.randn(n_t, n_sub, J), rng.randn(n_t, n_sub, n_out)
    acc = _accumulator(n_sub, J, n_out, bias, device)
    acc.update(torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device))
    A, B = _get(acc)
    wA, wB, gA, gB = gram_want(X, Y, bias)
    worst = max(C.check(A, wA, gA, "A"), C.check(B, wB, gB, "B"))
    print(f"gram J={J} bias={bias} n_out={n_out} T={n_t} n_sub={n_sub}: worst fraction of the gate {worst:.3f}")
    assert np.array_equal(A, A.transpose(0, 2, 1))


def test_gram_update_from_strided_views(device):
    rng = np.random.RandomState(C._seed("gram-strided"))
    n_t, n_sub, J, n_out = 7, 6, 65, 9
    big_x = torch.from_numpy(rng.randn(n_t, 2 * n_sub, J + 3)).to(device)
    big_y = torch.from_numpy(rng.randn(2 * n_t, n_sub, n_out + 1)).to(device)
    X, Y = big_x[:, ::2, :J], big_y[1::2, :, :n_out]
    assert not X.is_contiguous() and not Y.is_contiguous()
    acc = _accumulator(n_sub, J, n_out, True, device)
    acc.update(X, Y)
    A, B = _get(acc)
    wA, wB, gA, gB = gram_want(X.cpu().numpy(), Y.cpu().numpy(), True)
    worst = max(C.check(A, wA, gA, "A"), C.check(B, wB, gB, "B"))
    print(f"gram strided: worst fraction of the gate {worst:.3f}")
    # the states[:-1] / targets[1:] views of the training loop, and a transposed view that has to be copied
    acc.reset()
    acc.update(big_x[:-1, :n_sub, :J], big_y[1:n_t, :, :n_out])
    A2, _ = _get(acc)
    wA2 = gram_want(big_x[:-1, :n_sub, :J].cpu().numpy(), big_y[1:n_t, :, :n_out].cpu().numpy(), True)
    C.check(A2, wA2[0], wA2[2], "A of shifted views")
    acc.reset()
    acc.update(X.transpose(0, 1).contiguous().transpose(0, 1), Y)
    assert np.array_equal(_get(acc)[0], A)


def test_gram_bitwise_properties(device):
    rng = np.random.RandomState(C._seed("gram-bits"))
    n_sub, J, n_out = 6, 65, 18
    X, Y = rng.randn(13, n_sub, J), rng.randn(13, n_sub, n_out)
    dx, dy = torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device)
    acc = _accumulator(n_sub, J, n_out, True, device)
    assert acc.K_STEP == 4
    acc.update(dx, dy)
    A, B = _get(acc)
    assert np.array_equal(A, A.transpose(0, 2, 1))
    again = _accumulator(n_sub, J, n_out, True, device)
    again.update(dx, dy)
    A2, B2 = _get(again)
    assert np.array_equal(A, A2) and np.array_equal(B, B2)
    # T1 a multiple of the k step: the same chain, bit for bit
    acc.reset()
    zeros = _get(acc)
    assert not zeros[0].any() and not zeros[1].any()
    acc.update(dx[:8], dy[:8])
    acc.update(dx[8:], dy[8:])
    A3, B3 = _get(acc)
    assert np.array_equal(A, A3) and np.array_equal(B, B3)
    # otherwise within the gate of the 13 terms
    acc.reset()
    acc.update(dx[:5], dy[:5])
    acc.update(dx[5:], dy[5:])
    A4, B4 = _get(acc)
    wA, wB, gA, gB = gram_want(X, Y, True)
    worst = max(C.check(A4, wA, gA, "A"), C.check(B4, wB, gB, "B"))
    print(f"gram 5 + 8 steps: worst fraction of the gate {worst:.3f}")
    assert np.array_equal(A4, A4.transpose(0, 2, 1))
    # one subdomain read back alone is the same block
    a1, b1 = acc.get(4)
    assert np.array_equal(a1.cpu().numpy(), A4[4]) and np.array_equal(b1.cpu().numpy(), B4[4])


def test_gram_non_finite(device):
    rng = np.random.RandomState(C._seed("gram-nan"))
    n_t, n_sub, J, n_out = 6, 3, 70, 9
    X, Y = rng.randn(n_t, n_sub, J), rng.randn(n_t, n_sub, n_out)
    clean = _accumulator(n_sub, J, n_out, True, device)
    clean.update(torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device))
    cA, cB = _get(clean)
    bad = X.copy()
    bad[2, 1, 66] = np.nan
    acc = _accumulator(n_sub, J, n_out, True, device)
    acc.update(torch.from_numpy(bad).to(device), torch.from_numpy(Y).to(device))
    A, B = _get(acc)
    wA, wB, gA, gB = gram_want(bad, Y, True)
    assert np.isnan(wA[1, 66]).all() and np.isnan(wA[1, :, 66]).all() and np.isnan(wA[1]).sum() == 2 * 71 - 1
    C.check(A, wA, gA, "A with a NaN")
    C.check(B, wB, gB, "B with a NaN")
    for s in (0, 2):
        assert np.array_equal(A[s], cA[s]) and np.array_equal(B[s], cB[s])
    # a NaN only behind the end of the series, in a larger buffer, changes nothing
    big_x = torch.full((n_t + 3, n_sub, J), float("nan"), dtype=torch.float64, device=device)
    big_y = torch.full((n_t + 3, n_sub, n_out), float("nan"), dtype=torch.float64, device=device)
    big_x[:n_t], big_y[:n_t] = torch.from_numpy(X).to(device), torch.from_numpy(Y).to(device)
    acc = _accumulator(n_sub, J, n_out, True, device)
    acc.update(big_x[:n_t], big_y[:n_t])
    A, B = _get(acc)
    assert np.array_equal(A, cA) and np.array_equal(B, cB)


# ---------------------------------------------------------------------------------------------
# series stepping
# ---------------------------------------------------------------------------------------------

SERIES = {
    "plain": dict(),
    "square": dict(square=True),
    "hybrid": dict(hybrid_sizes=(1, 2), square=True),
    "hybrid-mask": dict(hybrid_sizes=(1, 2), hybrid_mask=np.float64),
    "noise": dict(noise=True),
    "scale-spatial": dict(in_kind="scale-spatial", out_kind="scale-spatial", hybrid_kind="scale-spatial", in_sizes=(2, 2),
                          out_sizes=(2,), hybrid_sizes=(2,), in_tf_mask=np.float64, out_tf_mask=np.float64, square=True),
}
N_STEPS = 12


@pytest.mark.parametrize("name", list(SERIES))
def test_train_series_matches_restatement(device, name):
    kw = dict(SERIES[name])
    noise, square = kw.pop("noise", False), kw.pop("square", False)
    kw.setdefault("in_sizes", (2, 1, 3))
    kw.setdefault("out_sizes", (2, 1))
    rng = np.random.RandomState(C._seed("series", name))
    m = C.make_model(rng, (2, 3), (2, 3), overlap=1, state_size=41, **kw)
    ns, n_in = 6, C.n_in_of(m)
    if noise:  # the 0/1 mask that training enforces: (u + noise) * mask == u * mask + noise * mask
        m["input_mask"] = (rng.random_sample((ns, n_in)) > 0.2).astype(np.float64)
    dtype = np.float32 if kw.get("in_kind") == "scale-spatial" else np.float64
    series = lambda sizes, extent: [np.stack(a) for a in zip(*[C.make_arrays(rng, sizes, extent, dtype)  # noqa: E731
                                                               for _ in range(N_STEPS)])]
    inputs = series(m["input"]["sizes"], C.ov_extent(m))
    hybrid = series(m["hybrid"]["sizes"], m["rank"]) if m["hybrid"] is not None else None
    targets = series(m["output"]["sizes"], m["rank"])
    noise_arr = 0.05 * rng.randn(N_STEPS, ns, n_in) if noise else None

    model = C.package_model(m)
    handle = model._model()
    to = lambda arrays: [torch.from_numpy(a).to(device) for a in arrays]  # noqa: E731
    dev_inputs = to(inputs)
    X = handle.train_series(dev_inputs, None if hybrid is None else to(hybrid),
                            noise=None if noise_arr is None else torch.from_numpy(noise_arr).to(device),
                            square_even_elements=square).cpu().numpy()
    state_after = handle.get_state().cpu().numpy()
    Y = handle.encode_targets(to(targets)).cpu().numpy()

    states, last = T.state_series(m, np.zeros((ns, 41)), inputs, noise_arr)
    hyb = T.encoded_series(m, m["hybrid"], hybrid, m.get("hybrid_mask")) if hybrid is not None else None
    want = R.square_even_terms(states, axis=-1) if square else states
    want = np.concatenate([want, hyb], axis=-1) if hyb is not None else want
    worst = C.check(X, want, 1e-12, f"X of {name}")
    print(f"series {name}: worst fraction of the 1e-12 gate {worst:.4f}")
    # the targets are an encoding alone: exact
    assert np.array_equal(Y, T.encoded_series(m, m["output"], targets).astype(np.float64))
    if hyb is not None:
        assert np.array_equal(X[..., 41:], hyb.astype(np.float64))
    # the state after the series is that of the same steps taken one by one, bit for bit
    if not noise:
        eager = C.package_model(m)
        for t in range(N_STEPS):
            eager.increment_state([a[t] for a in dev_inputs])
        assert np.array_equal(eager.get_state(), state_after)
        assert np.array_equal(X[-1, :, 1:41:2], state_after[:, 1::2])
    C.check(state_after, last, 1e-12, "state after the series")


def test_train_series_checks_its_shapes(device):
    rng = np.random.RandomState(C._seed("series-shapes"))
    m = C.make_model(rng, (2, 3), (2, 3), overlap=1, state_size=41, in_sizes=(2,), hybrid_sizes=(1,))
    handle = C.package_model(m)._model()
    good = torch.zeros((3, 6, 11, 2), dtype=torch.float64, device=device)
    hyb = torch.zeros((3, 4, 9, 1), dtype=torch.float64, device=device)
    with pytest.raises(ValueError, match="input array 0 has shape"):
        handle.train_series([good[:, :5]], [hyb])
    with pytest.raises(ValueError, match="hybrid array 0 has shape"):
        handle.train_series([good], [hyb[:2]])
    with pytest.raises(ValueError, match="noise must be"):
        handle.train_series([good], [hyb], noise=torch.zeros((3, 6, 5), dtype=torch.float64, device=device))
    with pytest.raises(ValueError, match="output array 0 has shape"):
        handle.encode_targets([good])


# ---------------------------------------------------------------------------------------------
# the solve
# ---------------------------------------------------------------------------------------------


def _backward_error(lhs, W, B):
    return np.linalg.norm(lhs @ W - B) / (np.linalg.norm(lhs) * np.linalg.norm(W) + np.linalg.norm(B))


@pytest.mark.parametrize("add_bias", [True, False])
def test_solve_backward_error(device, add_bias):
    from fv3net_amd.fit import BatchLinearRegressor, BatchLinearRegressorHyperparameters, NotFittedError

    rng = np.random.RandomState(C._seed("solve", add_bias))
    n_t, n_sub, J, n_out, l2 = 90, 3, 65, 9, 1e-3
    X, Y = rng.randn(n_t, n_sub, J), rng.randn(n_t, n_sub, n_out)
    if not add_bias:
        X[..., -1] = 1.0
    lr = BatchLinearRegressor(BatchLinearRegressorHyperparameters(l2=l2, add_bias_term=add_bias), device=device)
    with pytest.raises(NotFittedError):
        lr.get_weights()
    lr.batch_update(X[:40], Y[:40])
    lr.batch_update(torch.from_numpy(X[40:]).to(device), torch.from_numpy(Y[40:]).to(device))
    coefficients, intercepts = lr.get_weights()
    J1 = J + int(add_bias)
    assert coefficients.shape == (n_sub, J1 - 1, n_out) and intercepts.shape == (n_sub, n_out)
    A, B = (t.cpu().numpy() for t in lr.sums())
    worst = 0.0
    for s in range(n_sub):
        lhs = A[s] + l2 * np.identity(J1)
        W = np.concatenate([coefficients[s], intercepts[s][None]])
        ours, numpys = _backward_error(lhs, W, B[s]), _backward_error(lhs, np.linalg.solve(lhs, B[s]), B[s])
        gate = max(16 * numpys, J1 * 2.0 ** -52)
        print(f"solve bias={add_bias} subdomain {s}: backward error {ours:.3e}, numpy's {numpys:.3e}, ratio "
              f"{ours / numpys:.2f}, fraction of the gate {ours / gate:.3f}")
        assert ours <= gate
        worst = max(worst, ours / gate)
    if not add_bias:
        with pytest.raises(ValueError, match="Last column of X array must all be ones"):
            lr.batch_update(rng.randn(4, n_sub, J), Y[:4])
    # least squares on the host, and the reference's [time, feature] form
    small = BatchLinearRegressor(BatchLinearRegressorHyperparameters(l2=0, use_least_squares_solve=True), device=device)
    Xk, Yk = np.array([[1.0, 2, 1], [2, 3, 0]]), np.array([[12.0, 8], [11, 7]])
    small.batch_update(Xk, Yk)
    ck, ik = small.get_weights()
    assert ck.shape == (3, 2) and ik.shape == (2,)
    np.testing.assert_array_almost_equal(Xk @ ck + ik, Yk)


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------


def _training_data(rng, hybrid):
    """Three batches of 20 steps over 4 x 4 cells with a halo of 1; "b" comes as [t, x, y], the mask as [x, y]."""
    batches = []
    mask = (rng.random_sample((6, 6)) > 0.2).astype(np.float64)
    for _ in range(3):
        batch = {"a": rng.randn(20, 6, 6, 1), "b": rng.randn(20, 6, 6), "m": mask}
        if hybrid:
            batch["h"] = rng.randn(20, 6, 6, 1)
        batches.append(batch)
    return batches


def _config(hybrid, **kw):
    from fv3net_amd.fit import (BatchLinearRegressorHyperparameters, CubedsphereSubdomainConfig, ReservoirHyperparameters,
                                ReservoirTrainingConfig)

    base = dict(input_variables=["a", "b"], output_variables=["a"],
                subdomain=CubedsphereSubdomainConfig(layout=(2, 2), overlap=1, rank_dims=["x", "y"]),
                reservoir_hyperparameters=ReservoirHyperparameters(state_size=40, adjacency_matrix_sparsity=0.8,
                                                                   spectral_radius=0.9, seed=2, input_coupling_scaling=0.3),
                readout_hyperparameters=BatchLinearRegressorHyperparameters(l2=1e-2), n_timesteps_synchronize=25,
                input_noise=0.01 if hybrid else 0.0, seed=5, square_half_hidden_state=True)
    if hybrid:
        base.update(hybrid_variables=["h"], mask_reservoir_inputs=True, mask_hybrid_inputs=True, mask_variable="m")
    base.update(kw)
    return ReservoirTrainingConfig(**base)


def _transformers():
    from fv3net_amd.fit import TransformerGroup
    from fv3net_amd.reservoir import DoNothingTransformer

    return TransformerGroup(DoNothingTransformer([1, 1]), DoNothingTransformer([1]), DoNothingTransformer([1]))


def _restatement_model(model):
    """The restatement's dictionary of a trained package model."""
    tf = lambda t: {"kind": "do-nothing", "sizes": list(t.original_feature_sizes)}  # noqa: E731
    csr = lambda w: (*w.csr(), w.shape)  # noqa: E731
    hybrid = hasattr(model, "hybrid_variables")
    return {"layout": model.rank_divider.subdomain_layout, "overlap": model.rank_divider.overlap,
            "rank": model.rank_divider.rank_extent, "input": tf(model.transformers.input),
            "output": tf(model.transformers.output), "hybrid": tf(model.transformers.hybrid) if hybrid else None,
            "hybrid_mask": model._hybrid_input_mask if hybrid else None, "w_in": csr(model.reservoir.W_in),
            "w_res": csr(model.reservoir.W_res), "input_mask": model.reservoir.input_mask_array}


@pytest.mark.parametrize("hybrid", [False, True], ids=["pure", "hybrid"])
def test_train_reservoir_model_end_to_end(device, tmp_path, hybrid):
    from fv3net_amd import fit
    from fv3net_amd.xr_compat import DataArray, Dataset

    rng = np.random.RandomState(C._seed("end-to-end", hybrid))
    batches = _training_data(rng, hybrid)
    config = _config(hybrid)
    adapter = fit.train_reservoir_model(config, batches, _transformers())
    assert type(adapter).__name__ == ("HybridReservoirDatasetAdapter" if hybrid else "ReservoirDatasetAdapter")
    model = adapter.model
    J1 = 40 + (4 if hybrid else 0) + 1
    assert model.readout.coefficients.shape == (4, J1 - 1, 4) and model.readout.intercepts.shape == (4, 4)

    m = _restatement_model(model)
    noises = None
    if hybrid:
        noise_rs = np.random.RandomState(config.seed)
        noises = [noise_rs.normal(0.0, config.input_noise, (20, 4, 32)) for _ in batches]
        assert set(np.unique(m["input_mask"])) == {0, 1} and m["hybrid_mask"].shape == (4, 4)
    full = lambda b: {k: (v if v.ndim == 4 else v[..., None]) for k, v in b.items() if k != "m"}  # noqa: E731
    want = T.train(m, [[full(b) for b in batches]], ["a", "b"], ["a"], 25, 1e-2, ["h"] if hybrid else None, True, noises)
    # 34 samples enter: the last 15 of batch 2's 19 and all 19 of batch 3
    assert want["X"].shape == (34, 4, J1 - 1) and want["Y"].shape == (34, 4, 4)
    _, _, gate_a, gate_b = gram_want(want["X"], want["Y"], True)
    worst = 0.0
    for s, regressor in enumerate(want["regressors"]):
        lhs = regressor.A + 1e-2 * np.identity(J1)
        kappa = np.linalg.cond(lhs)
        assert kappa <= 1e8, kappa
        eps_a = np.linalg.norm(gate_a[s]) / np.linalg.norm(regressor.A)
        eps_b = np.linalg.norm(gate_b[s]) / np.linalg.norm(regressor.B)
        gate = kappa * (eps_a + eps_b) / (1 - kappa * eps_a) + J1 * 2.0 ** -52 * kappa
        W = np.concatenate([want["coefficients"][s], want["intercepts"][s][None]])
        got = np.concatenate([model.readout.coefficients[s], model.readout.intercepts[s][None]])
        rel = np.linalg.norm(got - W) / np.linalg.norm(W)
        print(f"end to end hybrid={hybrid} subdomain {s}: kappa {kappa:.3e}, relative difference {rel:.3e}, gate {gate:.3e}, "
              f"fraction {rel / gate:.4f}")
        assert rel <= gate
        worst = max(worst, rel / gate)
    C.check(model.get_state(), want["state"], 1e-12, "state after training")

    # dump -> load -> predict, bit for bit
    path = str(tmp_path / "model")
    fit.dump(adapter, path)
    loaded = fit.load(path)
    assert type(loaded) is type(adapter)
    ds = Dataset()
    for name in (["h"] if hybrid else []):
        ds[name] = DataArray(rng.randn(4, 4), dims=("x", "y"))
    first, second = adapter.predict(ds), loaded.predict(ds)
    assert np.isfinite(np.asarray(first["a"].data)).all() and np.asarray(first["a"].data).any()
    assert np.array_equal(np.asarray(first["a"].data), np.asarray(second["a"].data))


def test_training_reports_the_references_errors(device):
    from fv3net_amd import fit

    rng = np.random.RandomState(C._seed("errors"))
    batches = _training_data(rng, True)
    with pytest.raises(KeyError, match="'m' must be included in training data if the mask_variable is specified"):
        fit.train_reservoir_model(_config(True), [{k: v for k, v in b.items() if k != "m"} for b in batches],
                                  _transformers())
    bad = [dict(b, m=b["m"] * 0.5) for b in batches]
    with pytest.raises(ValueError, match="Mask variable values in field m are not all in {0, 1}."):
        fit.train_reservoir_model(_config(True), bad, _transformers())
    with pytest.raises(ValueError, match="out of scope"):
        fit.train_reservoir_model(_config(False), batches, None)
    # a sequence of sequences resets the state at each first batch: two one-batch sequences never finish synchronizing
    with pytest.raises(fit.NotFittedError):
        fit.train_reservoir_model(_config(False), [[batches[0]], [batches[1]]], _transformers())
