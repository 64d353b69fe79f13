"""The graph autoregressor on the MI355X (``GraphModel``, ``fit.HipGraphAutoregressor``) against the float64 numpy oracle
``graph_np``, with the project's per-level gate (``tolerances.assert_close_per_level``: every feature within 1e-5 of its scale
over all cells, and no worse than 8x the float32 plain-torch twin on the CPU), on the normalised state.

Float32 twin against the float64 oracle on these cases, worst per-level ratio of one step, measured on the CPU before the cases
were fixed (cases were to be kept up to half the gate, 5e-6): MEASURED_RATIOS below, 2.8e-7 ... 1.5e-6; none had to be dropped.
The three-step rollout uses the compounding form of the gate (1e-5 of the scale + 4x the twin's own error), both chains starting
every step from the float32 state of the step before; the twin's own ratios there: 3.5e-7 ... 1.4e-6 over steps 1 to 3.
"""
import numpy as np
import pytest
import torch

import graph_cases
import graph_np
import tolerances

pytestmark = pytest.mark.gpu

VARS_C48 = {"T": 79, "q": 79, "ps": 1, "ts": 1}
VARS_SMALL = {"T": 7, "q": 3, "ps": 1}
# id -> (variables, depth, min_filters, n, activation, source dtype, dim order in the dataset)
CASES = {
    "c48_d2_m32_relu": (VARS_C48, 2, 32, 48, "relu", np.float32, ("time", "tile", "x", "y", "z")),
    "c48_d1_m4_tanh": (VARS_C48, 1, 4, 48, "tanh", np.float32, ("time", "tile", "z", "y", "x")),
    "c8_d2_m5_tanh_f64": (VARS_SMALL, 2, 5, 8, "tanh", np.float64, ("z", "time", "tile", "y", "x")),
    "c8_d1_m32_relu_f64": (VARS_SMALL, 1, 32, 8, "relu", np.float64, ("tile", "time", "x", "y", "z")),
    "c4_d1_m4_relu": (VARS_SMALL, 1, 4, 4, "relu", np.float32, ("time", "tile", "x", "y", "z")),
    "c4_d2_m4_relu_yx": (VARS_SMALL, 2, 4, 4, "relu", np.float32, ("time", "z", "tile", "y", "x")),
    "c8_d2_m32_tanh": (VARS_SMALL, 2, 32, 8, "tanh", np.float32, ("x", "y", "z", "tile", "time")),
    "c8_d1_m5_relu_one_var": ({"T": 6}, 1, 5, 8, "relu", np.float32, ("time", "tile", "x", "y", "z")),
}
MEASURED_RATIOS = {   # float32 twin on the CPU vs the float64 oracle, one step
    "c48_d2_m32_relu": 1.5e-6, "c48_d1_m4_tanh": 4.7e-7, "c8_d2_m5_tanh_f64": 4.1e-7, "c8_d1_m32_relu_f64": 8.3e-7,
    "c4_d1_m4_relu": 4.1e-7, "c4_d2_m4_relu_yx": 3.2e-7, "c8_d2_m32_tanh": 4.7e-7, "c8_d1_m5_relu_one_var": 2.8e-7,
}


def build_case(case, n_times=3):
    variables, depth, m, n, activation, dtype, order = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case))
    spec = graph_cases.make_spec(rng, variables, depth, m, activation)
    return spec, graph_cases.make_dataset(rng, spec, n_times, n, dtype, order)


def _dataset(data, device=None):
    from fv3net_amd.xr_compat import DataArray, Dataset

    return Dataset({k: DataArray(a if device is None else torch.from_numpy(a).to(device), dims=dims) for k, (dims, a) in data.items()})


def _flat(a):
    return np.asarray(a).reshape(-1, a.shape[-1])


@pytest.mark.parametrize("case", list(CASES))
def test_one_step_matches_the_float64_oracle(device, case):
    """Through ``predict``: the dataset is read in its own dim order and dtype; ``reference`` is numpy's pack -> float32 ->
    unpack bit for bit; the step on the packed state passes the gate; ``predicted`` is numpy's unpack of that step bit for bit."""
    from fv3net_amd import fit

    spec, data = build_case(case)
    arrays = graph_cases.canonical(data)
    model = fit.HipGraphAutoregressor(spec.state_variables, spec)
    X = _dataset(data)
    before = {k: a.copy() for k, (_, a) in data.items()}
    predicted, reference = model.predict(X, timesteps=1)
    for k, (_, a) in data.items():
        assert np.array_equal(a, before[k]), f"predict changed {k}"
    packed = graph_np.pack(spec, arrays, 1)
    want_reference = graph_np.unpack(spec, packed)
    for v in spec.variables:
        got = reference[v.name]
        assert got.dims == ("window", "time", "tile", "x", "y", "z")[:6 if v.nfeat > 1 else 5]
        assert isinstance(got.data, np.ndarray) and got.dtype == np.float64
        assert np.array_equal(got.values, want_reference[v.name]), f"reference {v.name}"
    state = torch.from_numpy(packed[:, 0]).to(device)
    stepped = model.model.step(state).cpu().numpy()
    truth = graph_np.forward(spec, packed[:, 0])
    cpu32 = graph_cases.twin_step(spec)(packed[:, 0])
    print(f"{case}: float32 twin vs oracle {graph_cases.worst_ratio(cpu32, truth):.2e}, device {graph_cases.worst_ratio(stepped, truth):.2e}")
    tolerances.assert_close_per_level(_flat(stepped), _flat(truth), cpu32=_flat(cpu32), name=case, rel=1e-5)
    want_predicted = graph_np.unpack(spec, np.stack([packed[:, 0], stepped], axis=1))
    for v in spec.variables:
        assert np.array_equal(predicted[v.name].values, want_predicted[v.name]), f"predicted {v.name}"


@pytest.mark.parametrize("case", ["c8_d2_m5_tanh_f64", "c4_d1_m4_relu", "c8_d2_m32_tanh"])
def test_three_step_rollout(device, case):
    from fv3net_amd.graph import GraphModel

    spec, data = build_case(case, n_times=7)
    packed = graph_np.pack(spec, graph_cases.canonical(data), 3)      # two windows
    assert packed.shape[:2] == (2, 4)
    model = GraphModel(spec, device)
    got = model.rollout(torch.from_numpy(packed[:, 0]).to(device), 3)
    assert tuple(got.shape) == (2, 4) + packed.shape[2:] and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert np.array_equal(got[:, 0], packed[:, 0])
    truth = graph_np.rollout(spec, packed[:, 0], 3)
    cpu32 = graph_np.rollout(spec, packed[:, 0], 3, graph_cases.twin_step(spec))
    for t in (1, 2, 3):
        tolerances.assert_close_per_level(_flat(got[:, t]), _flat(truth[:, t]), cpu32=_flat(cpu32[:, t]), name=f"{case} step {t}",
                                          rel=1e-5, compounding=True)
    # a rollout is the steps one after the other, bit for bit
    state = torch.from_numpy(packed[:, 0]).to(device)
    for t in (1, 2, 3):
        state = model.step(state)
        assert np.array_equal(state.cpu().numpy().view(np.uint32), got[:, t].view(np.uint32))


def test_graph_replay_equals_the_eager_rollout(device):
    from fv3net_amd.graph import GraphModel
    from fv3net_amd.graphs import GraphedCall

    spec, data = build_case("c8_d2_m5_tanh_f64", n_times=9)
    packed = graph_np.pack(spec, graph_cases.canonical(data), 4)
    model = GraphModel(spec, device)
    state = torch.from_numpy(packed[:, 0]).to(device)
    eager = model.rollout(state, 4).cpu().numpy()
    call = GraphedCall(lambda: model.rollout(state, 4), device=device)
    replayed = call.replay().cpu().numpy()
    assert np.array_equal(replayed.view(np.uint32), eager.view(np.uint32))
    other = torch.from_numpy(packed[::-1, 1].copy()).to(device)     # new values in the captured input: the replay follows them
    state.copy_(other)
    replayed = call.replay().cpu().numpy()
    assert np.array_equal(replayed.view(np.uint32), model.rollout(other, 4).cpu().numpy().view(np.uint32))


def test_windows_device_data_and_trailing_times(device):
    """Eight times and two steps: three windows, the last time dropped; device data in, device data out, unchanged."""
    from fv3net_amd import fit

    spec, data = build_case("c4_d2_m4_relu_yx", n_times=8)
    arrays = graph_cases.canonical(data)
    model = fit.HipGraphAutoregressor(spec.state_variables, spec)
    X = _dataset(data, device)
    before = {k: X[k].data.clone() for k in data}
    predicted, reference = model.predict(X, timesteps=2)
    for k in data:
        assert X[k].data.is_cuda and torch.equal(X[k].data, before[k])
    want_reference = graph_np.unpack(spec, graph_np.pack(spec, arrays, 2))
    host_predicted, host_reference = model.predict(_dataset(data), timesteps=2)
    for v in spec.variables:
        assert predicted[v.name].data.is_cuda and reference[v.name].data.is_cuda
        assert tuple(reference[v.name].shape)[:3] == (3, 3, 6)
        assert np.array_equal(reference[v.name].data.cpu().numpy(), want_reference[v.name])
        assert np.array_equal(predicted[v.name].data.cpu().numpy(), host_predicted[v.name].values)
        assert np.array_equal(host_reference[v.name].values, want_reference[v.name])
        assert np.array_equal(predicted[v.name].data[:, 0].cpu().numpy(), want_reference[v.name][:, 0])   # time 0 is the input


def test_dumped_model_predicts_the_same(device, tmp_path):
    from fv3net_amd import fit

    spec, data = build_case("c8_d1_m32_relu_f64", n_times=4)
    model = fit.HipGraphAutoregressor(spec.state_variables, spec)
    fit.dump(model, str(tmp_path / "m"))
    loaded = fit.load(str(tmp_path / "m"))
    assert isinstance(loaded, fit.HipGraphAutoregressor)
    X = _dataset(data)
    for a, b in zip(model.predict(X, 3), loaded.predict(X, 3)):
        for v in spec.variables:
            assert np.array_equal(a[v.name].values.view(np.uint64), b[v.name].values.view(np.uint64))


def test_known_answer_of_the_reference(device):
    """graph/test_graph.py:64-103 through ``HipGraphAutoregressor``, with the model that ``graph_cases.trained_flip_model``
    trains (stored under tests/golden/graph_flip_model; test_host_graph.py trains it again and checks it by the oracle)."""
    import os

    from fv3net_amd import fit
    from fv3net_amd.xr_compat import DataArray, Dataset

    model = fit.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_flip_model"))
    rng = np.random.default_rng(0)
    graph_cases.flip_series(rng, 20, 2, 2, 6, 2), graph_cases.flip_series(rng, 3, 2, 2, 6, 2)   # (the draws of the training data)
    test = graph_cases.flip_series(rng, 1, 1, 100, 6, 2)[0]
    X = Dataset({"a": DataArray(test["a"][0], dims=("time", "tile", "x", "y", "z")), "b": DataArray(test["b"][0], dims=("time", "tile", "x", "y"))})
    predicted, reference = model.predict(X, timesteps=1)
    assert predicted["a"].shape == (99, 2, 6, 6, 6, 2) and predicted["b"].shape == (99, 2, 6, 6, 6)
    graph_cases.check_flip_skill({k: predicted[k].values for k in "ab"}, {k: reference[k].values for k in "ab"})


def test_step_refuses_wrong_shapes(device):
    from fv3net_amd.graph import GraphModel

    spec, _ = build_case("c4_d2_m4_relu_yx")
    model = GraphModel(spec, device)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=device)
    with pytest.raises(ValueError, match="six tiles"):
        model.step(z(1, 5, 4, 4, 11))
    with pytest.raises(ValueError, match="square"):
        model.step(z(1, 6, 4, 8, 11))
    with pytest.raises(ValueError, match="multiple of 4"):
        model.step(z(1, 6, 6, 6, 11))
    with pytest.raises(ValueError, match="multiple of 4"):
        model.rollout(z(1, 6, 2, 2, 11), 2)
    with pytest.raises(ValueError, match="features"):
        model.step(z(1, 6, 4, 4, 10))
    assert tuple(model.step(z(0, 6, 4, 4, 11)).shape) == (0, 6, 4, 4, 11)
