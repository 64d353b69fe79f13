"""The FMR rollout on the MI355X (``RecurrentGeneratorModel``, ``fit.HipFullModelReplacement``) against the float64 evaluation of
the same network (``RecurrentGeneratorTwin.double()``) and against the reference's own float64 run (the fixtures), on the
normalised state.

The gate is the compounding form of ``tolerances.assert_close_per_level`` with the "level" axis flattened over (time, channel):
1e-5 of the channel's scale at that time + 4 x the float32 CPU run's own error at that time.  The error of any float32
evaluation grows with the step: the reference's float32 run stays under 1e-4 of a channel's scale through 9 times with
"resnet" steps and passes it at the 5th or 6th time with "conv" steps (about 3 x per step with random weights), so "conv"
cases have at most 4 times and "resnet" cases at most 9.  MEASURED_RATIOS: the float32 twin against the float64 twin at the
last time of every case (the fixtures: the reference's own two runs), measured on the CPU before the device ran them; the
device's ratios are printed beside them.

The rollout is not captured as a HIP graph, so there is no replay to compare.
"""
import os

import numpy as np
import pytest
import torch

import fmr_cases as fc
import tolerances

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fmr_reference")
ORDER = fc.ORDER
# id -> (variables, nx, n_convolutions, n_resnet, max_filters, convolution type, flags, windows, timesteps, source dtype, dim order)
CASES = {
    "c4_smallest": ({"ps": 1}, 4, 1, 1, 8, "halo_conv2d", {}, 1, 3, np.float32, ORDER),
    "c8_conv_step_f64": ({"T": 3, "ps": 1}, 8, 2, 1, 16, "conv2d", dict(step_type="conv"), 2, 3, np.float64, ("z", "time", "tile", "y", "x")),
    "c12_no_clock": ({"T": 2, "ps": 1}, 12, 1, 2, 16, "conv2d", dict(samples_per_day=None, bias=False), 2, 4, np.float32, ORDER),
    "c16_d3_no_features": ({"T": 3, "q": 1, "ps": 1}, 16, 3, 1, 64, "halo_conv2d", dict(features=False, samples_per_day=3), 2, 5, np.float32, ORDER),
}
FIXTURE_NTIME = {"halo_resnet": 6, "conv2d_conv": 4}
MEASURED_RATIOS = {   # float32 on the CPU vs float64 at the last time, worst channel
    "c4_smallest": 2.7e-6, "c8_conv_step_f64": 1.3e-5, "c12_no_clock": 1.1e-6, "c16_d3_no_features": 1.3e-5,
    "fixture halo_resnet": 2.5e-5, "fixture conv2d_conv": 3.3e-6,     # the reference's own float32 run vs its float64 run
}


def build_case(case):
    variables, nx, nc, nr, mf, conv, flags, n_windows, timesteps, dtype, order = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case))
    spec = fc.make_spec(rng, variables, nx, nc, nr, mf, conv, **flags)
    data = fc.make_dataset(rng, spec, n_windows * timesteps + 2, dtype, order)       # one trailing time that is dropped
    return spec, data, timesteps


def canonical_windows(spec, data, timesteps):
    from cyclegan_cases import canonical

    return fc.windows(fc.pack(spec, canonical(data)), timesteps)


def _dataset(data, device=None):
    from fv3net_amd.xr_compat import DataArray, Dataset

    return Dataset({k: DataArray(a if device is None else torch.from_numpy(a).to(device), dims=dims) for k, (dims, a) in data.items()})


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _forward(model, first, ntime, device, **kwargs):
    return model.model.generator.forward(torch.from_numpy(np.ascontiguousarray(first)).to(device), ntime, **kwargs).cpu().numpy()


def _gate(got, truth, cpu32, name, recorded):
    r32, rdev = fc.ratio_per_time(cpu32, truth), fc.ratio_per_time(got, truth)
    print(f"{name}: float32 on the CPU vs float64 per time {np.array2string(r32, precision=1)} (recorded at the last time: {recorded}), "
          f"device {np.array2string(rdev, precision=1)}")
    assert r32[-1] <= 1e-4, "the case is too long: its own float32 error passes 1e-4 at the last time"
    tolerances.assert_close_per_level(fc.time_channel(got), fc.time_channel(truth), cpu32=fc.time_channel(cpu32), name=name, rel=1e-5,
                                      compounding=True)


@pytest.mark.parametrize("case", list(CASES))
def test_rollout_matches_the_float64_twin(device, case):
    """Through ``predict``: the dataset is read in its own dim order and dtype and is left unchanged; the rollout from the packed
    first times passes the gate; ``predicted`` is numpy's unpack of that rollout and ``reference`` numpy's unpack of the packed
    windows, bit for bit, float64, dims ``window, time, tile, x, y(, z)``; time 0 of ``predicted`` is the generator's
    reconstruction of the initial state, not a copy of it."""
    from fv3net_amd import fit

    spec, data, timesteps = build_case(case)
    model = fit.HipFullModelReplacement(spec.state_variables, spec)
    before = {k: a.copy() for k, (_, a) in data.items()}
    predicted, reference = model.predict(_dataset(data), timesteps)
    for k, (_, a) in data.items():
        assert np.array_equal(a, before[k]), f"predict changed {k}"
    state = canonical_windows(spec, data, timesteps)
    assert state.shape[:2] == (CASES[case][7], timesteps + 1)
    packed = model.pack_to_tensor(_dataset(data), timesteps)
    assert packed.is_cuda and np.array_equal(_bits(packed.cpu().numpy()), _bits(state)), "pack_to_tensor is not numpy's windows"
    got = _forward(model, state[:, 0], timesteps + 1, device)
    assert np.array_equal(_bits(model.step_model(packed[:, 0], timesteps).cpu().numpy()), _bits(got))
    truth = fc.twin_forward(spec.generator, spec.convolution_type, state[:, 0], timesteps + 1, torch.float64)
    cpu32 = fc.twin_forward(spec.generator, spec.convolution_type, state[:, 0], timesteps + 1)
    _gate(got, truth, cpu32, case, MEASURED_RATIOS[case])
    want, ref = fc.unpack(spec, got), fc.unpack(spec, state)
    for name, nf in spec.variables:
        for ds, expect in ((predicted, want), (reference, ref)):
            p = ds[name]
            assert p.dims == ("window",) + ORDER[:5 if nf > 1 else 4] and isinstance(p.data, np.ndarray) and p.dtype == np.float64
            assert np.array_equal(_bits(p.values), _bits(expect[name])), name
        assert not np.array_equal(predicted[name].values[:, 0], reference[name].values[:, 0]), "time 0 is a copy of the input"
    assert set(predicted.data_vars) == set(reference.data_vars) == set(spec.state_variables)


@pytest.mark.parametrize("key", list(FIXTURE_NTIME))
def test_known_answer_of_the_reference(device, key):
    """The fixtures: the reference's own ``RecurrentGenerator`` run in float64 on the CPU is the truth, its float32 run the
    yardstick; the float64 twin is gated the same way."""
    from fv3net_amd import fit

    with np.load(os.path.join(GOLDEN, key, "reference.npz")) as z:
        golden = {k: z[k] for k in z.files}
    model = fit.load(os.path.join(GOLDEN, key))
    assert isinstance(model, fit.HipFullModelReplacement)
    spec, ntime = model.spec, FIXTURE_NTIME[key]
    arrays = {name: golden[f"input.{name}"] for name, _ in spec.variables}
    state = fc.windows(fc.pack(spec, arrays), ntime - 1)
    got = _forward(model, state[:, 0], ntime, device)
    truth, ref32 = (golden[k].transpose(0, 1, 2, 4, 5, 3) for k in ("out64", "out32"))
    _gate(got, truth, ref32, f"fixture {key}", MEASURED_RATIOS[f"fixture {key}"])
    twin64 = fc.twin_forward(spec.generator, spec.convolution_type, state[:, 0], ntime, torch.float64)
    tolerances.assert_close_per_level(fc.time_channel(got), fc.time_channel(twin64), cpu32=fc.time_channel(ref32), name=key + " (twin)",
                                      rel=1e-5, compounding=True)
    from fv3net_amd.xr_compat import DataArray, Dataset

    predicted, reference = model.predict(Dataset({name: DataArray(a, dims=ORDER[:a.ndim]) for name, a in arrays.items()}), ntime - 1)
    want, ref = fc.unpack(spec, got), fc.unpack(spec, state)
    for name, _ in spec.variables:
        assert np.array_equal(_bits(predicted[name].values), _bits(want[name])) and np.array_equal(_bits(reference[name].values), _bits(ref[name]))


@pytest.mark.parametrize("key", list(FIXTURE_NTIME))
def test_one_step_at_every_clock_value(device, key):
    """Step parity without compounding: the float64 twin's latent, rounded to float32, through ``step(latent, i)`` against the
    float64 twin's ``_step`` of the same latent with the clock at ``i - 1``; the float32 twin's step is the yardstick.  i runs
    past ``samples_per_day``, so the table wraps."""
    from fv3net_amd import fit

    model = fit.load(os.path.join(GOLDEN, key))
    spec = model.spec
    g, spd = spec.generator, spec.generator.samples_per_day
    with np.load(os.path.join(GOLDEN, key, "reference.npz")) as z:
        arrays = {name: z[f"input.{name}"] for name, _ in spec.variables}
    first = fc.windows(fc.pack(spec, arrays), FIXTURE_NTIME[key] - 1)[:, 0]
    twin64, twin32 = fc.twin_of(g, spec.convolution_type, torch.float64), fc.twin_of(g, spec.convolution_type)
    last = lambda t: t.permute(0, 1, 3, 4, 2).contiguous().numpy()
    with torch.no_grad():
        latent = twin64._encode(torch.from_numpy(first).double().permute(0, 1, 4, 2, 3)).float()      # [S, 6, C, nb, nb]
        encoded = model.model.generator.encode(torch.from_numpy(first).to(device)).cpu().numpy()
        tolerances.assert_close_per_level(encoded.reshape(-1, g.max_filters), last(latent.double()).reshape(-1, g.max_filters),
                                          cpu32=last(twin32._encode(torch.from_numpy(first).permute(0, 1, 4, 2, 3))).reshape(-1, g.max_filters),
                                          name=f"{key} encode", rel=1e-5, compounding=True)
        for i in range(1, spd + 2):
            twin64.clock.clock = twin32.clock.clock = (i - 1) % spd
            truth, cpu32 = last(twin64._step(latent.double())), last(twin32._step(latent))
            dev_latent = torch.from_numpy(last(latent)).to(device)
            got = model.model.generator.step(dev_latent, i)
            assert got is dev_latent
            r = tolerances.assert_close_per_level(got.cpu().numpy().reshape(-1, g.max_filters), truth.reshape(-1, g.max_filters),
                                                  cpu32=cpu32.reshape(-1, g.max_filters), name=f"{key} step {i}", rel=1e-5, compounding=True)
            print(f"{key} step {i}: device vs float64 {r:.2e}")
            if i == spd + 1:
                again = model.model.generator.step(torch.from_numpy(last(latent)).to(device), 1)
                assert torch.equal(again, got), "step spd + 1 does not read the clock's first row"


def test_bitwise_properties(device):
    """Two calls give identical bits (the clock restarts); ``forward(state, 1)`` is ``decode(encode(state))`` and ``decode``
    leaves the latent alone; chunks of one window and of all windows give identical bits, as does a workspace limit of one
    window; time ``t`` of 6 times is time ``t`` of 4 times; a window alone is that window among others."""
    from fv3net_amd import fit
    from fv3net_amd.fmr import RecurrentGeneratorModel

    rng = np.random.default_rng(11)
    spec = fc.make_spec(rng, {"T": 2, "ps": 1}, 8, 2, 2, 16)
    model = fit.HipFullModelReplacement(spec.state_variables, spec)
    first = rng.normal(0, 1, (3, 6, 8, 8, 3)).astype(np.float32)
    whole = _forward(model, first, 6, device)
    assert whole.shape == (3, 6, 6, 8, 8, 3) and np.all(np.isfinite(whole))
    assert np.array_equal(_bits(_forward(model, first, 6, device)), _bits(whole)), "a second call differs"
    for chunk in (1, 2, 3):
        assert np.array_equal(_bits(_forward(model, first, 6, device, chunk=chunk)), _bits(whole)), f"chunks of {chunk}"
    assert np.array_equal(_bits(_forward(model, first, 4, device)), _bits(whole[:, :4])), "4 times are not the first 4 of 6"
    for i in range(3):
        assert np.array_equal(_bits(_forward(model, first[i:i + 1], 6, device)), _bits(whole[i:i + 1])), f"window {i} alone"
    gen = model.model.generator
    state = torch.from_numpy(first).to(device)
    latent = gen.encode(state)
    kept = latent.clone()
    decoded = gen.decode(latent)
    assert torch.equal(latent, kept), "decode changed the latent"
    assert np.array_equal(_bits(decoded.cpu().numpy()), _bits(whole[:, 0])) and np.array_equal(_bits(_forward(model, first, 1, device)[:, 0]), _bits(whole[:, 0]))
    for t in range(1, 6):           # the public parts chained by hand are the rollout
        gen.step(latent, t, chunk=2)
        assert np.array_equal(_bits(gen.decode(latent, chunk=1).cpu().numpy()), _bits(whole[:, t])), f"time {t}"
    small = RecurrentGeneratorModel(spec.generator, spec.convolution_type, device, workspace_limit=1)      # one window per chunk
    assert small.chunk_size(3) == 1
    assert np.array_equal(_bits(small.forward(state, 6).cpu().numpy()), _bits(whole))


def test_device_inputs_and_the_dumped_model_give_the_same_bits(device, tmp_path):
    from fv3net_amd import fit

    spec, data, timesteps = build_case("c8_conv_step_f64")
    model = fit.HipFullModelReplacement(spec.state_variables, spec)
    host = model.predict(_dataset(data), timesteps)
    X = _dataset(data, device)
    before = {k: X[k].data.clone() for k in data}
    on_device = model.predict(X, timesteps)
    fit.dump(model, str(tmp_path / "m"))
    loaded = fit.load(str(tmp_path / "m"))
    assert isinstance(loaded, fit.HipFullModelReplacement)
    reloaded = loaded.predict(_dataset(data), timesteps)
    for name, _ in spec.variables:
        assert X[name].data.is_cuda and torch.equal(X[name].data, before[name])
        for i in range(2):
            assert on_device[i][name].data.is_cuda and on_device[i][name].data.dtype == torch.float64
            assert np.array_equal(_bits(on_device[i][name].data.cpu().numpy()), _bits(host[i][name].values))
            assert np.array_equal(_bits(reloaded[i][name].values), _bits(host[i][name].values))


def test_the_model_refuses_before_any_launch(device):
    from fv3net_amd.fmr import RecurrentGeneratorModel

    spec, _, _ = build_case("c4_smallest")
    model = RecurrentGeneratorModel(spec.generator, spec.convolution_type, device)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=device)
    with pytest.raises(ValueError, match="six tiles"):
        model.forward(z(1, 5, 4, 4, 1), 2)
    with pytest.raises(ValueError, match="nx = 4"):
        model.forward(z(1, 6, 8, 8, 1), 2)
    with pytest.raises(ValueError, match="the state has 2 features, the network needs 1"):
        model.forward(z(1, 6, 4, 4, 2), 2)
    with pytest.raises(ValueError, match="\\[window, tile, x, y, feature\\]"):
        model.forward(z(6, 4, 4, 1), 2)
    with pytest.raises(TypeError, match="float32, got torch.float64"):
        model.forward(z(1, 6, 4, 4, 1).double(), 2)
    with pytest.raises(RuntimeError, match="device tensors only"):
        model.forward(torch.zeros(1, 6, 4, 4, 1), 2)
    for ntime in (0, -1):
        with pytest.raises(ValueError, match=f"ntime must be at least 1, got {ntime}"):
            model.forward(z(1, 6, 4, 4, 1), ntime)
    with pytest.raises(ValueError, match="the latent must be a \\[window, 6, 2, 2, 8\\] tensor"):
        model.step(z(1, 6, 4, 4, 8), 1)
    with pytest.raises(ValueError, match="steps are counted from 1, got 0"):
        model.step(z(1, 6, 2, 2, 8), 0)
    with pytest.raises(ValueError, match="out must be a float32"):
        model.decode(z(1, 6, 2, 2, 8), z(1, 6, 4, 4, 2))
    with pytest.raises(RuntimeError, match="needs a 'cuda'"):
        RecurrentGeneratorModel(spec.generator, spec.convolution_type, "cpu")
    with pytest.raises(ValueError, match="Unknown convolution type"):
        RecurrentGeneratorModel(spec.generator, "conv3d", device)
    with pytest.raises(ValueError, match="max_chunk and workspace_limit must be positive"):
        RecurrentGeneratorModel(spec.generator, spec.convolution_type, device, max_chunk=0)
    assert tuple(model.forward(z(0, 6, 4, 4, 1), 3).shape) == (0, 3, 6, 4, 4, 1)
