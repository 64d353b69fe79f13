"""Reservoir training without a GPU: the numpy restatement (tests/reservoir_train_np.py) pinned by the
reference's own known answers (external/fv3fit/tests/reservoir/test_readout.py:56-72, :92-124, :127-152), the tracker's
off-by-one, the configuration's validation errors and ``Reservoir.generate``."""
import numpy as np
import pytest

import reservoir_train_np as T
from fv3net_amd.fit import (BatchLinearRegressor, BatchLinearRegressorHyperparameters, CubedsphereSubdomainConfig,
                            NotFittedError, Reservoir, ReservoirHyperparameters, ReservoirTrainingConfig,
                            SynchronizationTracker)

# y0 = 1*x0 + 2*x1 + 4*x3 + 3, y1 = 1*x0 + 2*x1 + 4*x3 - 1
X_KNOWN = np.array([[1, 2, 1], [2, 3, 0]])
Y_KNOWN = np.array([[12.0, 8], [11, 7]])


def test_restatement_regressor_known_answer():
    lr = T.BatchLinearRegressor(0, add_bias_term=True, use_least_squares_solve=True)
    lr.batch_update(X_KNOWN, Y_KNOWN)
    coefficients, intercepts = lr.get_weights()
    np.testing.assert_array_almost_equal(np.dot(X_KNOWN, coefficients) + intercepts, Y_KNOWN)


def test_restatement_regressor_bias_column_given_or_added():
    with_bias = np.array([[1, 2, 1, 1], [2, 3, 0, 1]])
    add = T.BatchLinearRegressor(0, add_bias_term=True, use_least_squares_solve=True)
    given = T.BatchLinearRegressor(0, add_bias_term=False, use_least_squares_solve=True)
    add.batch_update(X_KNOWN, Y_KNOWN)
    given.batch_update(with_bias, Y_KNOWN)
    for a, b in zip(add.get_weights(), given.get_weights()):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="Last column of X array must all be ones"):
        given.batch_update(np.array([[1, 2, 1, 10], [2, 3, 0, 2]]), Y_KNOWN)


def test_restatement_regressor_iterative_equals_one_shot():
    rng = np.random.RandomState(0)
    x_dim, y_dim, n, n_batches = 25, 5, 50, 5
    truth = rng.rand(y_dim, x_dim + 1)
    noise = rng.normal(-0.1, 0.1, size=(n, y_dim))
    xs = [np.concatenate([rng.rand(n, x_dim), np.ones((n, 1))], axis=1) for _ in range(n_batches)]
    ys = [np.dot(x, truth.T) + noise for x in xs]
    batched = T.BatchLinearRegressor(0.1, use_least_squares_solve=True)
    for x, y in zip(xs, ys):
        batched.batch_update(x, y)
    full = T.BatchLinearRegressor(0.1, use_least_squares_solve=True)
    full.batch_update(np.concatenate(xs), np.concatenate(ys))
    for a, b in zip(batched.get_weights(), full.get_weights()):
        np.testing.assert_array_almost_equal(a, b)


def test_regressors_refuse_to_solve_before_an_update():
    with pytest.raises(T.NotFittedError):
        T.BatchLinearRegressor(0.1).get_weights()
    with pytest.raises(NotFittedError, match="batch_update"):
        BatchLinearRegressor(BatchLinearRegressorHyperparameters(l2=0.1)).get_weights()


@pytest.mark.parametrize("tracker", [T.SynchronizationTracker, SynchronizationTracker], ids=["restatement", "package"])
def test_tracker_counts_as_the_reference_does(tracker):
    arr = np.arange(10)
    # n_synchronize = 0: complete after the first batch, and the whole batch is kept
    t = tracker(0)
    assert not t.completed_synchronization
    t.count_synchronization_steps(10)
    assert t.completed_synchronization
    np.testing.assert_array_equal(t.trim_synchronization_samples_if_needed(arr), arr)
    # n_synchronize = the batch length: exactly n_synchronize counted steps are NOT complete (more than is required)
    t = tracker(10)
    t.count_synchronization_steps(10)
    assert not t.completed_synchronization
    assert len(t.trim_synchronization_samples_if_needed(arr)) == 0
    t.count_synchronization_steps(10)
    assert t.completed_synchronization
    np.testing.assert_array_equal(t.trim_synchronization_samples_if_needed(arr), arr)
    # spanning two batches: 15 of 2 x 10 steps synchronize, the last 5 samples of the second batch are kept -- and of a
    # 9-sample array (X and Y lose one time step to the shift) the last 5 likewise
    t = tracker(15)
    t.count_synchronization_steps(10)
    assert not t.completed_synchronization
    t.count_synchronization_steps(10)
    assert t.completed_synchronization
    np.testing.assert_array_equal(t.trim_synchronization_samples_if_needed(arr), arr[-5:])
    np.testing.assert_array_equal(t.trim_synchronization_samples_if_needed(arr[:9]), arr[4:9])
    # one step past: a single sample
    t = tracker(9)
    t.count_synchronization_steps(10)
    np.testing.assert_array_equal(t.trim_synchronization_samples_if_needed(arr), arr[-1:])


def test_construct_readout_inputs_outputs_shifts_and_squares_elements():
    rng = np.random.RandomState(1)
    states, targets, hybrid = rng.randn(6, 3, 5), rng.randn(6, 3, 2), rng.randn(6, 3, 4)
    X, Y = T.construct_readout_inputs_outputs(states, targets, True, hybrid)
    assert X.shape == (5, 3, 9) and Y.shape == (5, 3, 2)
    np.testing.assert_array_equal(X[..., 0:5:2], states[:-1, :, 0::2] ** 2)  # even elements, of every subdomain
    np.testing.assert_array_equal(X[..., 1:5:2], states[:-1, :, 1::2])
    np.testing.assert_array_equal(X[..., 5:], hybrid[:-1])
    np.testing.assert_array_equal(Y, targets[1:])


def _config(**kw):
    base = dict(input_variables=["a", "b"], output_variables=["a"],
                subdomain=CubedsphereSubdomainConfig(layout=(2, 2), overlap=1, rank_dims=["x", "y"]),
                reservoir_hyperparameters=ReservoirHyperparameters(state_size=40, adjacency_matrix_sparsity=0.8,
                                                                   spectral_radius=0.9),
                readout_hyperparameters=BatchLinearRegressorHyperparameters(l2=1e-2), n_timesteps_synchronize=5,
                input_noise=0.0)
    base.update(kw)
    return base


def test_config_defaults_and_validation():
    c = ReservoirTrainingConfig(**_config())
    assert (c.seed, c.n_jobs, c.square_half_hidden_state, c.hybrid_variables, c.mask_variable) == (0, 1, False, None, None)
    assert c.readout_hyperparameters.add_bias_term and not c.readout_hyperparameters.use_least_squares_solve
    assert (c.reservoir_hyperparameters.input_coupling_sparsity, c.reservoir_hyperparameters.input_coupling_scaling) == (0, 1)
    assert c.variables == {"a", "b"}
    with pytest.raises(ValueError, match="cannot overlap with input variables"):
        ReservoirTrainingConfig(**_config(hybrid_variables=["b", "c"]))
    for flag in ("mask_reservoir_inputs", "mask_hybrid_inputs"):
        with pytest.raises(ValueError, match="mask_variable must be specified if masking is enabled"):
            ReservoirTrainingConfig(**_config(**{flag: True}))
    c = ReservoirTrainingConfig(**_config(hybrid_variables=["c"], mask_hybrid_inputs=True, mask_variable="m"))
    assert c.variables == {"a", "b", "c", "m"}


def test_config_from_dict():
    d = _config(subdomain={"layout": [2, 3], "overlap": 1, "rank_dims": ["x", "y"]},
                reservoir_hyperparameters={"state_size": 40, "adjacency_matrix_sparsity": 0.8, "spectral_radius": 1},
                readout_hyperparameters={"l2": 1})
    c = ReservoirTrainingConfig.from_dict(d)
    assert c.subdomain.layout == (2, 3) and isinstance(c.readout_hyperparameters.l2, float)
    assert isinstance(c.reservoir_hyperparameters.spectral_radius, float) and c.transformers.input is None
    with pytest.raises(ValueError, match="no field"):
        ReservoirTrainingConfig.from_dict({**d, "readout_hyperparameters": {"l2": 1, "ridge": 2}})
    with pytest.raises(ValueError, match="missing"):
        ReservoirTrainingConfig.from_dict({**d, "readout_hyperparameters": {}})
    with pytest.raises(ValueError, match="cannot overlap"):
        ReservoirTrainingConfig.from_dict({**d, "hybrid_variables": ["a"]})


@pytest.mark.parametrize("sparsity", [0.0, 0.5, 0.9])
def test_generate_draws_the_reservoir_the_reference_describes(sparsity):
    hp = ReservoirHyperparameters(state_size=60, adjacency_matrix_sparsity=0.8, spectral_radius=0.9, seed=3,
                                  input_coupling_sparsity=sparsity, input_coupling_scaling=0.25)
    r = Reservoir.generate(hp, input_size=7)
    w_in, w_res = r.W_in.toarray(), r.W_res.toarray()
    assert w_in.shape == (60, 7) and w_res.shape == (60, 60)
    # every input reaches the same number of state elements
    stored = np.diff(np.asarray(r.W_in.arrays["indptr"]))
    assert r.W_in.format == "csc" and np.all(stored == round((1 - sparsity) * 60))
    assert np.abs(w_in).max() <= 0.25 and (w_in < 0).any() and (w_in > 0).any()
    assert r.W_res.nnz == round(0.2 * 60 * 60) and w_res.min() >= 0
    assert abs(np.abs(np.linalg.eigvals(w_res)).max() - 0.9) <= 1e-8
    again = Reservoir.generate(hp, input_size=7)
    np.testing.assert_array_equal(again.W_in.toarray(), w_in)
    np.testing.assert_array_equal(again.W_res.toarray(), w_res)
    other = Reservoir.generate(ReservoirHyperparameters(60, 0.8, 0.9, seed=4, input_coupling_sparsity=sparsity), 7)
    assert not np.array_equal(other.W_res.toarray(), w_res)
    assert r.hyperparameters["state_size"] == 60 and r.input_size == 7


def test_generated_reservoir_round_trips_through_its_files(tmp_path):
    hp = ReservoirHyperparameters(state_size=12, adjacency_matrix_sparsity=0.5, spectral_radius=0.8, seed=1)
    r = Reservoir.generate(hp, input_size=5, input_mask_array=np.ones((4, 5)))
    r.dump(str(tmp_path / "r"))
    back = Reservoir.load(str(tmp_path / "r"))
    np.testing.assert_array_equal(back.W_in.toarray(), r.W_in.toarray())
    np.testing.assert_array_equal(back.W_res.toarray(), r.W_res.toarray())
    assert back.hyperparameters == r.hyperparameters and back.input_mask_array.shape == (4, 5)
