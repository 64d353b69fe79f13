"""The host side of the CycleGAN predictor: the plain-torch twin against the reference's own ``Generator`` (the fixture
``tests/golden/cyclegan_reference``, written by ``make_cyclegan_golden.py``), the time of day, the spec codec, the refusals and
the parity split of the transposed convolution.  No GPU."""
import os

import numpy as np
import pytest
import torch

import cyclegan_cases as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cyclegan_reference")
CONFIG = dict(n_convolutions=2, n_resnet=2, max_filters=12, use_geographic_embedded_bias=True)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "reference.npz")) as z:
        return {k: z[k] for k in z.files}


def golden_state(golden, spec, domain):
    return cc.pack(spec, {name: golden[f"input.{domain}.{name}"] for name, _ in spec.variables}, domain)


@pytest.mark.parametrize("key,domain", [("a_to_b", "a"), ("b_to_a", "b")])
def test_twin_loads_the_reference_state_dict_and_reproduces_its_output(golden, key, domain):
    from fv3net_amd import fit
    from fv3net_amd.cyclegan import seconds_since_1970

    model = fit.load(GOLDEN)
    twin = fit.GeneratorTwin(3, 8, lon=golden["lon"], xyz=golden["xyz"], **CONFIG)
    prefix = f"generator_{key}."
    state_dict = {k[len(prefix):]: torch.from_numpy(v) for k, v in golden.items() if k.startswith(prefix)}
    assert "_main.0.0.1._wrapped.weight" in state_dict and "_main.1._lower._down.conv_block.0.1._wrapped.weight" in state_dict
    assert "_input_bias.bias" in state_dict and "_main.1._up.conv_block.0.1.0._wrapped.weight" in state_dict
    twin.load_state_dict(state_dict, strict=True)
    state = torch.from_numpy(golden_state(golden, model.spec, domain)).permute(0, 1, 4, 2, 3)
    with torch.no_grad():
        got = twin.eval()(torch.from_numpy(seconds_since_1970(golden["time"])), state).numpy()
    want, truth = golden[f"out32.{key}"], golden[f"out64.{key}"]
    # Measured where the fixture was written: bit for bit (difference 0).  The assertion is a bound, not bit equality, because
    # another CPU may sum a convolution in another order: two float32 evaluations may differ by twice what one differs from
    # float64, which the fixture itself gives (7.2e-6 and 2.6e-6 of the output's scale for the two generators).
    scale = np.max(np.abs(truth))
    own = np.max(np.abs(want.astype(np.float64) - truth)) / scale
    diff = np.max(np.abs(got - want)) / scale
    print(f"{key}: twin - reference {diff:.2e} of the scale (reference float32 - float64: {own:.2e})")
    assert diff <= 2 * own
    # and the same through the spec: state dict -> spec -> twin
    twin2 = fit.cyclegan.twin_from_spec(model.spec.generator(key == "b_to_a"))
    with torch.no_grad():
        assert np.array_equal(twin2(torch.from_numpy(seconds_since_1970(golden["time"])), state).numpy(), got)


@pytest.mark.parametrize("seconds", [0.0, 86399.0, 1.7e9 + 977, 1.7e9 + 977 + 7 * 3600, -5000.0])
def test_theta_equals_the_torch_float32_expression(seconds):
    from fv3net_amd.cyclegan import seconds_since_1970, theta_from_seconds

    t32 = seconds_since_1970(np.array([seconds]))
    assert t32.dtype == np.float32
    want = (torch.from_numpy(t32) % 86400 / 86400 * 2 * np.pi).numpy()
    got = theta_from_seconds(t32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_time_inputs():
    from fv3net_amd.cyclegan import seconds_since_1970, theta_from_seconds

    stamps = np.array(["2023-11-14T22:29:37", "1970-01-01T00:00:00", "1970-01-01T23:59:59"], dtype="datetime64[s]")
    want = np.array([1.7e9 + 977, 0, 86399], np.float64).astype(np.float32)
    for unit in ("s", "ms", "ns"):
        assert np.array_equal(seconds_since_1970(stamps.astype(f"datetime64[{unit}]")), want)
    assert np.array_equal(seconds_since_1970([1700000977, 0, 86399]), want)
    assert seconds_since_1970(np.float64(1.7e9 + 977))[0] == np.float32(1.7e9 + 1024)      # float32 seconds: 128 s apart
    torch_theta = (torch.from_numpy(want) % 86400 / 86400 * 2 * np.pi).numpy()
    assert np.array_equal(theta_from_seconds(seconds_since_1970(stamps)), torch_theta)
    # cftime objects are read where that module exists
    try:
        import cftime
    except ImportError:
        with pytest.raises(TypeError, match="cftime"):
            seconds_since_1970(np.array([object()], dtype=object))
    else:
        dates = np.array([cftime.DatetimeJulian(2023, 11, 14, 22, 29, 37)], dtype=object)
        assert seconds_since_1970(dates)[0] == np.float32(cftime.date2num(dates[0], "seconds since 1970-01-01"))


def test_spec_round_trips(tmp_path, golden):
    from fv3net_amd import fit
    from fv3net_amd.cyclegan import CycleGanSpec

    rng = np.random.default_rng(0)
    for conv, flags in (("halo_conv2d", dict(embedded=True)), ("conv2d", dict(bias=False, features=False)), ("conv2d", dict(kernel_size=5))):
        spec = cc.make_spec(rng, {"T": 2, "ps": 1}, 8, 2, 1, 12, conv, **flags)
        meta, arrays = spec.to_arrays()
        again = CycleGanSpec.from_arrays(meta, arrays)
        meta2, arrays2 = again.to_arrays()
        assert meta2 == meta and arrays.keys() == arrays2.keys() and all(np.array_equal(arrays[k], arrays2[k]) for k in arrays)
        fit.dump(fit.HipCycleGAN(spec.state_variables, spec), str(tmp_path / conv))
        loaded = fit.load(str(tmp_path / conv))
        assert isinstance(loaded, fit.HipCycleGAN) and loaded.input_variables == ["T", "ps"] and loaded.output_variables == ["T", "ps"]
        meta3, arrays3 = loaded.spec.to_arrays()
        assert meta3 == meta and all(np.array_equal(arrays[k], arrays3[k]) and arrays[k].dtype == arrays3[k].dtype for k in arrays)
        state_dict = fit.cyclegan_state_dict_from_spec(spec)
        g = spec.generator_a_to_b
        back = fit.cyclegan_spec_from_state_dict(state_dict, spec.state_variables, spec.scalers, 8, conv, g.lon, g.xyz, n_convolutions=2,
                                                 n_resnet=1, max_filters=12, kernel_size=g.kernel_size,
                                                 use_geographic_bias=g.use_geographic_bias, use_geographic_features=g.use_geographic_features,
                                                 use_geographic_embedded_bias=g.use_geographic_embedded_bias)
        meta4, arrays4 = back.to_arrays()
        assert meta4 == meta and all(np.array_equal(arrays[k], arrays4[k]) for k in arrays)
    # the fixture's artifact is the fixture's state dict
    model = fit.load(GOLDEN)
    for k, v in fit.cyclegan_state_dict_from_spec(model.spec).items():
        assert np.array_equal(v.numpy(), golden[k]), k
    assert not any(k.startswith("discriminator") for k in fit.cyclegan_state_dict_from_spec(model.spec))
    assert sorted(os.listdir(GOLDEN)) == ["config.yaml", "name", "reference.npz", "spec.yaml", "weights.npz"]


def test_refusals_name_the_offending_value():
    from fv3net_amd import fit
    from fv3net_amd.cyclegan import CycleGanSpec, check_architecture, check_grid

    rng = np.random.default_rng(1)
    with pytest.raises(NotImplementedError, match="strided_kernel_size = 3"):
        check_architecture(strided_kernel_size=3)
    with pytest.raises(NotImplementedError, match="disable_convolutions = True"):
        check_architecture(disable_convolutions=True)
    with pytest.raises(NotImplementedError, match="kernel_size = 4"):
        check_architecture(kernel_size=4)
    with pytest.raises(ValueError, match="n_convolutions must be at least 1, got 0"):
        check_architecture(n_convolutions=0)
    with pytest.raises(ValueError, match="n_resnet must not be negative, got -1"):
        check_architecture(n_resnet=-1)
    with pytest.raises(ValueError, match="8 x 6"):
        check_grid(8, 6, 1)
    with pytest.raises(ValueError, match="nx = 12 cannot be halved 3 times"):
        check_grid(12, 12, 3)
    with pytest.raises(ValueError, match="nx = 4 leaves faces of 1 x 1"):
        check_grid(4, 4, 2)
    with pytest.raises(ValueError, match="nx = 2"):
        check_grid(2, 2, 1)
    with pytest.raises(ValueError, match="nx = 4 leaves faces of 1 x 1"):
        cc.make_generator(rng, 2, 4, 2, 1, 8)
    with pytest.raises(NotImplementedError, match="strided_kernel_size = 6"):
        fit.GeneratorTwin(2, 8, strided_kernel_size=6, lon=0, xyz=0)
    with pytest.raises(ValueError, match="Unknown convolution type: 'conv3d'"):
        cc.make_spec(rng, {"T": 2}, 8, 1, 0, 8, "conv3d")
    spec = cc.make_spec(rng, {"T": 2}, 8, 1, 0, 8)
    meta, arrays = spec.to_arrays()
    meta["generators"]["a_to_b"]["strided_kernel_size"] = 3
    with pytest.raises(NotImplementedError, match="strided_kernel_size = 3"):
        CycleGanSpec.from_arrays(meta, arrays)
    # the predictor checks the data's grid on the host, before anything touches a device
    from fv3net_amd.xr_compat import DataArray, Dataset

    model = fit.HipCycleGAN(["T"], spec)
    for shape, match in (((2, 6, 8, 6, 2), "8 x 6"), ((2, 6, 12, 12, 2), "nx = 8"), ((2, 5, 8, 8, 2), "six tiles")):
        X = Dataset({"T": DataArray(np.zeros(shape), dims=("time", "tile", "x", "y", "z")), "time": DataArray(np.zeros(2), dims=("time",))})
        with pytest.raises(ValueError, match=match):
            model.predict(X)
    with pytest.raises(ValueError, match="no weights.npz"):
        fit.HipCycleGAN.load(os.path.dirname(GOLDEN))


def test_parity_split_reproduces_conv_transpose_and_crop():
    """``ConvTranspose2d(4, stride 2)`` of the input padded by one line, cropped by 3, as the four 2 x 2 convolutions."""
    from fv3net_amd.cyclegan import split_transposed_weight, transposed_source_offset

    rng = np.random.default_rng(5)
    c_in, c_out, n = 3, 4, 5
    xp = rng.normal(0, 1, (1, c_in, n + 2, n + 2))          # the padded input; the halo ring is data like any other
    w = rng.normal(0, 1, (c_in, c_out, 4, 4))
    want = torch.nn.functional.conv_transpose2d(torch.from_numpy(xp), torch.from_numpy(w), stride=2)[0, :, 3:-3, 3:-3].numpy()
    assert want.shape == (c_out, 2 * n, 2 * n)
    split = split_transposed_weight(w)
    got = np.zeros_like(want)
    for px in range(2):
        for py in range(2):
            for a in range(2):
                for b in range(2):
                    ox, oy = 1 + transposed_source_offset(px, a), 1 + transposed_source_offset(py, b)
                    got[:, px::2, py::2] += np.einsum("ixy,io->oxy", xp[0, :, ox:ox + n, oy:oy + n], split[px, py, a, b])
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
    # padding = 1 on the unpadded input is the same index map with zeros off the face
    x = xp[:, :, 1:-1, 1:-1]
    zero_padded = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    a = torch.nn.functional.conv_transpose2d(torch.from_numpy(zero_padded), torch.from_numpy(w), stride=2)[0, :, 3:-3, 3:-3]
    b = torch.nn.functional.conv_transpose2d(torch.from_numpy(x.copy()), torch.from_numpy(w), stride=2, padding=1)[0]
    assert np.allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=1e-12)


def test_flops_and_plan():
    rng = np.random.default_rng(2)
    g = cc.make_generator(rng, 1, 48, 2, 6, 256)
    names = [p[0] for p in g.plan]
    assert names[:3] == ["first", "down0", "down1"] and names[-3:] == ["up1", "up0", "last"] and len(names) == 18
    cells = 6 * 48 * 48
    want = 2 * cells * (49 * 6 * 64 + 49 * 64 * 1) + 2 * 16 * 64 * 128 * cells / 4 + 2 * 16 * 128 * 256 * cells / 16 \
        + 12 * 2 * 9 * 256 * 256 * cells / 16 + 2 * 4 * 256 * 128 * cells / 4 + 2 * 4 * 128 * 64 * cells
    assert g.flops_per_sample() == want and 1.5e10 < want < 1.8e10
