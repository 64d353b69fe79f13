"""The CycleGAN generators on the MI355X (``GeneratorModel``, ``fit.HipCycleGAN``) against the float64 evaluation of the same
network (``GeneratorTwin.double()``), on the normalised state, per output channel.

The gate is the compounding form of ``tolerances.assert_close_per_level``: 1e-5 of the channel's scale + 4 x the float32 twin's
own error on the CPU.  The plain 1e-5 gate does not fit this network: instance norm divides by the standard deviation of a
face, and where the bottom face is 2 x 2 that is a small number, so float32 evaluations of one and the same network differ by
up to 2e-5 of a channel's scale.  MEASURED_RATIOS: the float32 twin against the float64 twin on these cases, measured on the
CPU before the device ran them; the device's ratio is printed beside it.

The forward pass is not captured as a HIP graph, so there is no replay to compare.
"""
import os

import numpy as np
import pytest
import torch

import cyclegan_cases as cc
import tolerances

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cyclegan_reference")
ORDER = ("time", "tile", "x", "y", "z")
# id -> (variables, nx, n_convolutions, n_resnet, max_filters, convolution type, flags, samples, source dtype, dim order)
CASES = {
    "c4_smallest": ({"ps": 1}, 4, 1, 1, 8, "halo_conv2d", {}, 1, np.float32, ORDER),
    "c8_conv2d_f64": ({"T": 3, "ps": 1}, 8, 1, 6, 40, "conv2d", {}, 2, np.float64, ("z", "time", "tile", "y", "x")),
    "c16_d3_no_features": ({"T": 3, "q": 1, "ps": 1}, 16, 3, 1, 64, "halo_conv2d", dict(features=False), 2, np.float32, ORDER),
    "c20_no_resnet_embedded": ({"T": 2}, 20, 1, 0, 8, "halo_conv2d", dict(bias=False, embedded=True), 2, np.float32, ORDER),
    "c48_three_samples": ({"T": 2, "ps": 1}, 48, 2, 1, 64, "halo_conv2d", {}, 3, np.float32, ORDER),
}
MEASURED_RATIOS = {   # float32 twin on the CPU vs the float64 twin, worst channel
    "c4_smallest": 1.2e-6, "c8_conv2d_f64": 1.2e-6, "c16_d3_no_features": 4.7e-6, "c20_no_resnet_embedded": 7.9e-7, "c48_three_samples": 1.2e-6,
    "fixture a_to_b": 7.5e-6, "fixture b_to_a": 3.4e-6,     # the reference's own float32 run vs its float64 run
}


def build_case(case):
    variables, nx, nc, nr, mf, conv, flags, n_times, dtype, order = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case))
    spec = cc.make_spec(rng, variables, nx, nc, nr, mf, conv, **flags)
    data, seconds = cc.make_dataset(rng, spec, n_times, dtype, order)
    return spec, data, seconds


def _dataset(data, time, device=None):
    from fv3net_amd.xr_compat import DataArray, Dataset

    ds = Dataset({k: DataArray(a if device is None else torch.from_numpy(a).to(device), dims=dims) for k, (dims, a) in data.items()})
    ds["time"] = DataArray(np.asarray(time), dims=("time",))
    return ds


def _flat(a):
    return np.asarray(a).reshape(-1, a.shape[-1])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _forward(model, packed, seconds, device, reverse=False, **kwargs):
    from fv3net_amd.cyclegan import theta_from_seconds

    theta = torch.from_numpy(theta_from_seconds(np.asarray(seconds, np.float32)))
    return model.model.generator(reverse).forward(torch.from_numpy(packed).to(device), theta, **kwargs).cpu().numpy()


@pytest.mark.parametrize("case", list(CASES))
def test_generator_matches_the_float64_twin(device, case):
    """Through ``predict``: the dataset is read in its own dim order and dtype and is left unchanged; the generator on the
    packed state passes the gate; ``predicted`` is numpy's unpack of that state bit for bit, float64, dims ``time, tile, x, y
    (, z)``, with the input's ``time``."""
    from fv3net_amd import fit
    from fv3net_amd.cyclegan import seconds_since_1970

    spec, data, seconds = build_case(case)
    model = fit.HipCycleGAN(spec.state_variables, spec)
    X = _dataset(data, seconds)
    before = {k: a.copy() for k, (_, a) in data.items()}
    predicted = model.predict(X)
    for k, (_, a) in data.items():
        assert np.array_equal(a, before[k]), f"predict changed {k}"
    packed = cc.pack(spec, cc.canonical(data), "a")
    s32 = seconds_since_1970(seconds)
    got = _forward(model, packed, s32, device)
    truth = cc.twin_forward(spec.generator_a_to_b, spec.convolution_type, packed, s32, torch.float64)
    cpu32 = cc.twin_forward(spec.generator_a_to_b, spec.convolution_type, packed, s32)
    print(f"{case}: float32 twin vs float64 {cc.worst_ratio(cpu32, truth):.2e} (recorded {MEASURED_RATIOS[case]:.1e}), "
          f"device {cc.worst_ratio(got, truth):.2e}")
    tolerances.assert_close_per_level(_flat(got), _flat(truth), cpu32=_flat(cpu32), name=case, rel=1e-5, compounding=True)
    want = cc.unpack(spec, got, "b")
    for name, nf in spec.variables:
        p = predicted[name]
        assert p.dims == ORDER[:5 if nf > 1 else 4] and isinstance(p.data, np.ndarray) and p.dtype == np.float64
        assert np.array_equal(_bits(p.values), _bits(want[name])), f"predicted {name}"
    assert np.array_equal(predicted["time"].values, np.asarray(seconds))


@pytest.mark.parametrize("reverse", [False, True], ids=["a_to_b", "b_to_a"])
def test_known_answer_of_the_reference(device, reverse):
    """The fixture: the reference's own ``Generator`` run in float64 on the CPU is the truth, its float32 run the yardstick."""
    from fv3net_amd import fit
    from fv3net_amd.cyclegan import seconds_since_1970

    with np.load(os.path.join(GOLDEN, "reference.npz")) as z:
        golden = {k: z[k] for k in z.files}
    model = fit.load(GOLDEN)
    spec, key, (src, dst) = model.spec, "b_to_a" if reverse else "a_to_b", ("b", "a") if reverse else ("a", "b")
    arrays = {name: golden[f"input.{src}.{name}"] for name, _ in spec.variables}
    packed = cc.pack(spec, arrays, src)
    s32 = seconds_since_1970(golden["time"])
    got = _forward(model, packed, s32, device, reverse)
    truth, ref32 = (golden[f"{p}.{key}"].transpose(0, 1, 3, 4, 2) for p in ("out64", "out32"))
    print(f"fixture {key}: reference float32 vs float64 {cc.worst_ratio(ref32, truth):.2e}, device {cc.worst_ratio(got, truth):.2e}")
    tolerances.assert_close_per_level(_flat(got), _flat(truth), cpu32=_flat(ref32), name=key, rel=1e-5, compounding=True)
    twin64 = cc.twin_forward(spec.generator(reverse), spec.convolution_type, packed, s32, torch.float64)
    tolerances.assert_close_per_level(_flat(got), _flat(twin64), cpu32=_flat(ref32), name=key + " (twin)", rel=1e-5, compounding=True)
    from fv3net_amd.xr_compat import DataArray, Dataset

    X = Dataset({name: DataArray(a, dims=ORDER[:a.ndim]) for name, a in arrays.items()})
    X["time"] = DataArray(golden["time"], dims=("time",))           # datetime64
    predicted = model.predict(X, reverse=reverse)
    want = cc.unpack(spec, got, dst)
    for name, _ in spec.variables:
        assert np.array_equal(_bits(predicted[name].values), _bits(want[name])), name
    assert np.array_equal(predicted["time"].values, golden["time"])


def test_chunks_and_batches_do_not_change_a_bit(device):
    from fv3net_amd import fit
    from fv3net_amd.cyclegan import seconds_since_1970

    rng = np.random.default_rng(11)
    spec = cc.make_spec(rng, {"T": 2, "ps": 1}, 8, 2, 2, 40, embedded=True)
    data, seconds = cc.make_dataset(rng, spec, 3)
    packed, s32 = cc.pack(spec, cc.canonical(data), "a"), seconds_since_1970(seconds)
    model = fit.HipCycleGAN(spec.state_variables, spec)
    whole = _forward(model, packed, s32, device)
    for chunk in (1, 2):
        assert np.array_equal(_bits(_forward(model, packed, s32, device, chunk=chunk)), _bits(whole)), f"chunks of {chunk}"
    for i in range(3):
        assert np.array_equal(_bits(_forward(model, packed[i:i + 1], s32[i:i + 1], device)), _bits(whole[i:i + 1])), f"sample {i} alone"
    from fv3net_amd.cyclegan import GeneratorModel

    small = GeneratorModel(spec.generator_a_to_b, spec.convolution_type, device, workspace_limit=1)      # one sample per chunk
    assert small.chunk_size(3) == 1
    from fv3net_amd.cyclegan import theta_from_seconds

    got = small.forward(torch.from_numpy(packed).to(device), torch.from_numpy(theta_from_seconds(s32))).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(whole))


def test_device_inputs_and_the_dumped_model_give_the_same_bits(device, tmp_path):
    from fv3net_amd import fit

    spec, data, seconds = build_case("c8_conv2d_f64")
    model = fit.HipCycleGAN(spec.state_variables, spec)
    host = model.predict(_dataset(data, seconds))
    X = _dataset(data, seconds, device)
    before = {k: X[k].data.clone() for k in data}
    on_device = model.predict(X)
    fit.dump(model, str(tmp_path / "m"))
    loaded = fit.load(str(tmp_path / "m"))
    assert isinstance(loaded, fit.HipCycleGAN)
    reloaded = loaded.predict(_dataset(data, seconds))
    back = model.predict(_dataset(data, seconds), reverse=True)
    for name, _ in spec.variables:
        assert X[name].data.is_cuda and torch.equal(X[name].data, before[name])
        assert on_device[name].data.is_cuda and on_device[name].data.dtype == torch.float64
        assert np.array_equal(_bits(on_device[name].data.cpu().numpy()), _bits(host[name].values))
        assert np.array_equal(_bits(reloaded[name].values), _bits(host[name].values))
        assert not np.array_equal(back[name].values, host[name].values)      # the other generator, the other scalers


def test_forward_refuses_wrong_shapes(device):
    from fv3net_amd.cyclegan import GeneratorModel

    spec, _, _ = build_case("c4_smallest")
    model = GeneratorModel(spec.generator_a_to_b, spec.convolution_type, device)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=device)
    theta = torch.zeros(1)
    with pytest.raises(ValueError, match="six tiles"):
        model.forward(z(1, 5, 4, 4, 1), theta)
    with pytest.raises(ValueError, match="nx = 4"):
        model.forward(z(1, 6, 8, 8, 1), theta)
    with pytest.raises(ValueError, match="features"):
        model.forward(z(1, 6, 4, 4, 2), theta)
    with pytest.raises(ValueError, match="theta"):
        model.forward(z(1, 6, 4, 4, 1))
    with pytest.raises(TypeError, match="float32"):
        model.forward(z(1, 6, 4, 4, 1).double(), theta)
    assert tuple(model.forward(z(0, 6, 4, 4, 1), torch.zeros(0)).shape) == (0, 6, 4, 4, 1)
