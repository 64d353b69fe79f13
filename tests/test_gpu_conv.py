"""The convolutional predictor on the MI355X against the float64 numpy oracle (``conv_np``), with the project's per-level gate
(``tolerances.assert_close_per_level``: every output level within 1e-5 of its scale and no worse than 8x the float32 CPU
evaluation of the same graph), samples = all pixels of all tiles.

Float32 CPU chain against float64 on these cases (six tiles, zero corners, inputs as ``conv_cases.make_inputs`` draws them),
worst per-level ratio, measured on the CPU before the cases were fixed: 0.3e-6 ... 2.4e-6 over the cases below, the added ones
(F = 1, F = 5, no bias, float64 sources, k = 7) included -- the reference arithmetic alone sits at a quarter of the gate.
"""
import os

import numpy as np
import pytest
import torch

import conv_cases
import conv_np
import tolerances

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "append_halos_reference.npz")

# id -> (n, input channels, filters, depth, k, heads, activation, bias, source dtype, channels_last)
CASES = {
    "c48_T_q_cosz_relu": (48, {"T": 79, "q": 79, "cosz": 1}, 32, 3, 3, {"dQ1": 79, "dQ2": 79}, "relu", True, np.float32, False),
    "c48_T_q_cosz_tanh": (48, {"T": 79, "q": 79, "cosz": 1}, 32, 3, 3, {"dQ1": 79, "dQ2": 79}, "tanh", True, np.float32, False),
    "c24_four_inputs_depth4": (24, {"T": 79, "q": 79, "u": 79, "cosz": 1}, 64, 4, 3, {"dQ1": 79, "rain": 1}, "relu", True,
                                   np.float32, False),
    "c16_k5_depth2": (16, {"T": 19, "lat": 1}, 8, 2, 5, {"dQ1": 19}, "relu", True, np.float32, False),
    "c12_one_input": (12, {"T": 15}, 32, 3, 3, {"dQ1": 15}, "relu", True, np.float32, False),
    "one_filter": (12, {"T": 15, "lat": 1}, 1, 3, 3, {"dQ1": 15}, "relu", True, np.float32, False),
    "five_filters_tanh": (12, {"T": 15, "lat": 1}, 5, 3, 3, {"dQ1": 15, "rain": 1}, "tanh", True, np.float32, False),
    "no_bias_linear": (12, {"T": 15, "lat": 1}, 32, 3, 3, {"dQ1": 15}, "linear", False, np.float32, False),
    "float64_sources": (16, {"T": 19, "lat": 1}, 32, 3, 3, {"dQ1": 19, "rain": 1}, "relu", True, np.float64, False),
    "channels_last": (16, {"T": 19, "lat": 1}, 32, 3, 3, {"dQ1": 19, "rain": 1}, "relu", True, np.float32, True),
    "channels_last_float64_k5": (16, {"T": 19, "lat": 1}, 40, 2, 5, {"dQ1": 19}, "tanh", True, np.float64, True),
    "k7": (16, {"T": 6}, 8, 2, 7, {"dQ1": 6}, "relu", True, np.float32, False),
}


def _pad_cube(fields, h):
    """name -> [6, x, y, z] -> name -> [6, x + 2 h, y + 2 h, z] by the oracle's own halo fill."""
    return {k: np.moveaxis(conv_np.append_halos(np.moveaxis(v, -1, 1), h), 1, -1) for k, v in fields.items()}


def _to_device(fields, dev, channels_last):
    """[..., x, y, z] host arrays -> device tensors in the layout under test."""
    out = {}
    for k, v in fields.items():
        t = torch.from_numpy(np.ascontiguousarray(v if channels_last else np.swapaxes(v, -1, -3)))
        out[k] = t.to(dev)
    return out


def _to_xyz(t, channels_last):
    a = t.cpu().numpy()
    return a if channels_last else np.swapaxes(a, -1, -3)


def _edge_mask(n, h):
    m = np.ones((n, n), bool)
    m[h:n - h, h:n - h] = False
    return m


@pytest.mark.parametrize("case", list(CASES))
def test_predict_matches_the_float64_oracle(device, case):
    from fv3net_amd.conv import ConvModel

    n, channels, filters, depth, k, heads, activation, bias, dtype, channels_last = CASES[case]
    rng = np.random.default_rng(sorted(CASES).index(case))
    spec = conv_cases.make_spec(rng, channels, filters, depth, k, heads, activation=activation, bias=bias)
    h = spec.halos_required
    cube = conv_cases.make_inputs(rng, spec, (6,), n, n, dtype)
    padded = _pad_cube(cube, h)
    truth = conv_np.forward(spec, padded)
    cpu32 = conv_cases.torch_chain(spec, {k_: v.astype(np.float32) for k_, v in padded.items()}, torch.float32)
    got = ConvModel(spec, device).predict(_to_device(cube, device, channels_last), halo="cube", channels_last=channels_last)
    edge = _edge_mask(n, h)
    for name, nf in heads.items():
        assert got[name].dtype == torch.float32
        g = _to_xyz(got[name], channels_last)
        assert g.shape == (6, n, n, nf)
        scale = np.max(np.abs(truth[name]), axis=(0, 1, 2))
        err = np.abs(g - truth[name]) / scale
        print(f"{case} {name}: worst per-level error / scale  seam pixels {err[:, edge].max():.2e}  "
              f"interior {err[:, ~edge].max():.2e}  (float32 CPU chain: {(np.abs(cpu32[name] - truth[name]) / scale).max():.2e})")
        tolerances.assert_close_per_level(g.reshape(-1, nf), truth[name].reshape(-1, nf), cpu32=cpu32[name].reshape(-1, nf),
                                          name=f"{case} {name}")


def test_prepadded_nonsquare_batch(device):
    """An input that carries its halo (what ``nx != ny`` fields use), two batch dims, mixed float32 / float64 sources."""
    from fv3net_amd.conv import ConvModel

    rng = np.random.default_rng(40)
    spec = conv_cases.make_spec(rng, {"T": 19, "lat": 1}, 32, 3, 3, {"dQ1": 19, "rain": 1})
    h = spec.halos_required
    fields = conv_cases.make_inputs(rng, spec, (2, 3), 11 + 2 * h, 15 + 2 * h, np.float32)
    fields["lat"] = fields["lat"].astype(np.float64)
    flat = {k: v.reshape((6,) + v.shape[2:]) for k, v in fields.items()}
    truth = conv_np.forward(spec, flat)
    cpu32 = conv_cases.torch_chain(spec, flat, torch.float32)
    got = ConvModel(spec, device).predict(_to_device(fields, device, False), halo="input")
    for name, nf in (("dQ1", 19), ("rain", 1)):
        assert tuple(got[name].shape) == (2, 3, nf, 15, 11)
        g = _to_xyz(got[name], False).reshape(-1, nf)
        tolerances.assert_close_per_level(g, truth[name].reshape(-1, nf), cpu32=cpu32[name].reshape(-1, nf), name=name)


def _shift_network(k, n_channels):
    """Linear, unit-normalised network of depth 2 whose head s returns the padded input shifted by one of the four corner
    offsets of the k x k window: together the four heads show every cell of the padded field, exactly."""
    from fv3net_amd.conv import ConvInput, ConvOutput, ConvSpec

    c = n_channels
    shifts = [(0, 0), (k - 1, 0), (0, k - 1), (k - 1, k - 1)]
    w = np.zeros((k, k, c, 4 * c), np.float32)
    outputs = []
    for s, (dx, dy) in enumerate(shifts):
        head = np.zeros((4 * c, c), np.float32)
        for ch in range(c):
            w[dx, dy, ch, s * c + ch] = 1.0
            head[s * c + ch, ch] = 1.0
        outputs.append(ConvOutput(f"shift{s}", c, head, np.zeros(c, np.float32), np.ones(c, np.float32), np.zeros(c, np.float32)))
    spec = ConvSpec([ConvInput("ids", c, np.zeros(c, np.float32), np.ones(c, np.float32))], [w], None, outputs, activation="linear")
    return spec, shifts


@pytest.mark.parametrize("n_halo", [1, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_halo_route_equals_the_reference_fixture(device, n_halo, dtype):
    """The loader's neighbour reads on a resident cube, seen through a network that copies its padded input: equal to what
    the reference's ``AppendHalos`` wrote, cell for cell, corners zero."""
    from fv3net_amd.conv import ConvModel

    with np.load(GOLDEN) as z:
        field, want = z["input"].astype(dtype), z[f"padded_{n_halo}"]   # [6, c, x, y]
    k, n = 2 * n_halo + 1, field.shape[-1]
    spec, shifts = _shift_network(k, field.shape[1])
    assert spec.halos_required == n_halo
    src = torch.from_numpy(np.ascontiguousarray(np.swapaxes(field, -1, -2))).to(device)  # [6, z, y, x]
    got = ConvModel(spec, device).predict({"ids": src}, halo="cube")
    seen = np.full(want.shape, -1.0)
    for s, (dx, dy) in enumerate(shifts):
        seen[:, :, dx:dx + n, dy:dy + n] = np.swapaxes(got[f"shift{s}"].cpu().numpy(), -1, -2)
    np.testing.assert_array_equal(seen, want)


@pytest.mark.parametrize("k, depth, n_expected", [(3, 2, 9), (5, 2, 25), (3, 3, 25)])
@pytest.mark.parametrize("activation", ["tanh", "linear"])
def test_receptive_field(device, k, depth, n_expected, activation):
    """tests/keras/test_convolutional_network.py:176-202 of the reference: one changed input cell at the centre of a 17 x 17
    field changes exactly the outputs whose window holds it; everything else is bitwise the same."""
    from fv3net_amd.conv import ConvModel

    rng = np.random.default_rng(k + depth)
    spec = conv_cases.make_spec(rng, {"a": 1}, 32, depth, k, {"out": 1}, activation=activation)
    model = ConvModel(spec, device)
    a = conv_cases.make_inputs(rng, spec, (1,), 17, 17)["a"]          # [1, x, y, 1]
    first = model.predict(_to_device({"a": a}, device, False), halo="input")["out"].cpu().numpy()
    a[0, 8, 8, 0] += 1.0
    second = model.predict(_to_device({"a": a}, device, False), halo="input")["out"].cpu().numpy()
    assert first.shape == (1, 1, 17 - 2 * spec.halos_required, 17 - 2 * spec.halos_required)
    assert int(np.sum(first != second)) == n_expected


def test_cube_strips_and_prepadded_routes_are_bit_identical(device):
    from fv3net_amd.conv import ConvModel
    from fv3net_amd.cubedsphere.halos import edge_strips, halo_strips

    rng = np.random.default_rng(50)
    spec = conv_cases.make_spec(rng, {"T": 19, "lat": 1}, 32, 3, 3, {"dQ1": 19, "rain": 1}, activation="tanh")
    h, n = spec.halos_required, 16
    cube = conv_cases.make_inputs(rng, spec, (6,), n, n)
    cube["lat"] = cube["lat"].astype(np.float64)
    model = ConvModel(spec, device)
    dev_cube = _to_device(cube, device, False)
    resident = model.predict(dev_cube, halo="cube")
    prepadded = model.predict(_to_device(_pad_cube(cube, h), device, False), halo="input")
    # [6, z, y, x] -> [6, z, x, y] -> edges [6, 4, h, z, n], the variables' channels concatenated
    edges = torch.cat([edge_strips(t.transpose(-1, -2).to(torch.float64), h) for t in dev_cube.values()], dim=-2)
    from_strips = model.predict(dev_cube, halo="strips", strips=halo_strips(edges, range(6)))
    for name in ("dQ1", "rain"):
        assert torch.equal(resident[name], prepadded[name]), name
        assert torch.equal(resident[name], from_strips[name]), name


def _dataset(rng, spec, n, on=None):
    from fv3net_amd.xr_compat import DataArray, Dataset

    cube = conv_cases.make_inputs(rng, spec, (2, 6), n, n)  # [time, tile, x, y, z]
    wrap = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(on)) if on is not None else np.ascontiguousarray
    ds = Dataset({
        "T": DataArray(wrap(cube["T"]), dims=("time", "tile", "x", "y", "z"),
                       coords={"time": np.arange(2) * 900.0, "tile": np.arange(6), "z": np.arange(19) + 0.5}),
        "q": DataArray(wrap(cube["q"].transpose(4, 1, 0, 3, 2)), dims=("z", "tile", "time", "y", "x")),
        "lat": DataArray(wrap(cube["lat"][..., 0].transpose(1, 3, 0, 2).astype(np.float64)), dims=("tile", "y", "time", "x")),
    })
    return ds, cube


@pytest.mark.parametrize("where", ["host", "device"])
def test_predictor_on_a_six_tile_dataset(device, where):
    """``HipConvolutionalModel.predict``: any dim order per variable, a single-level variable, float32 and float64, a batch
    dim; values against the oracle fed by its own ``append_halos``; dims, coords, the input left as it was."""
    import fv3net_amd.fit as fit

    rng = np.random.default_rng(60)
    spec = conv_cases.make_spec(rng, {"T": 19, "q": 19, "lat": 1}, 32, 3, 3, {"dQ1": 19, "rain": 1})
    h, n = spec.halos_required, 12
    ds, cube = _dataset(rng, spec, n, on=device if where == "device" else None)
    before = {name: (ds[name].data.clone() if where == "device" else ds[name].data.copy()) for name in ds}
    out = fit.HipConvolutionalModel(["T", "q", "lat"], ["dQ1", "rain"], spec).predict(ds)
    for name in ds:
        assert (torch.equal(ds[name].data, before[name]) if where == "device" else np.array_equal(ds[name].data, before[name]))
    flat = {k: v.reshape((12, n, n, -1)) for k, v in cube.items()}
    padded = {k: np.concatenate([_pad_cube({k: v[i * 6:(i + 1) * 6]}, h)[k] for i in range(2)]) for k, v in flat.items()}
    truth = conv_np.forward(spec, padded)
    cpu32 = conv_cases.torch_chain(spec, padded, torch.float32)
    assert out["dQ1"].dims == ("time", "tile", "x", "y", "z") and out["rain"].dims == ("time", "tile", "x", "y")
    np.testing.assert_array_equal(out.coords["time"], np.arange(2) * 900.0)
    np.testing.assert_array_equal(out.coords["z"], np.arange(19) + 0.5)
    for name, nf in (("dQ1", 19), ("rain", 1)):
        data = out[name].data
        assert isinstance(data, torch.Tensor) and data.is_cuda if where == "device" else isinstance(data, np.ndarray)
        g = (data.cpu().numpy() if where == "device" else data).reshape(-1, nf)
        tolerances.assert_close_per_level(g, truth[name].reshape(-1, nf), cpu32=cpu32[name].reshape(-1, nf), name=name)


def test_predictor_needs_the_cube_or_ranks(device):
    import fv3net_amd.fit as fit
    from fv3net_amd.xr_compat import DataArray, Dataset

    spec = conv_cases.make_spec(np.random.default_rng(61), {"T": 3}, 4, 2, 3, {"dQ1": 3})
    model = fit.HipConvolutionalModel(["T"], ["dQ1"], spec)
    with pytest.raises(ValueError, match="either dataset must have tile dimension or MPI must be present"):
        model.predict(Dataset({"T": DataArray(np.zeros((8, 8, 3), np.float32), dims=("x", "y", "z"))}))
    with pytest.raises(ValueError, match="six tiles"):
        model.predict(Dataset({"T": DataArray(np.zeros((1, 8, 8, 3), np.float32), dims=("tile", "x", "y", "z"))}))


def test_create_refuses_on_the_host(device):
    """The library's own validation (before any HIP call): a zero scale, and a kernel size that is not built."""
    from fv3net_amd import _lib
    from fv3net_amd.conv import ConvModel

    spec = conv_cases.make_spec(np.random.default_rng(62), {"T": 3}, 4, 2, 3, {"dQ1": 3})
    spec.inputs[0].scale[1] = 0.0
    with pytest.raises(_lib.Fv3HipError, match="scale"):
        ConvModel(spec, device)
    big = conv_cases.make_spec(np.random.default_rng(63), {"T": 3}, 4, 2, 9, {"dQ1": 3})
    with pytest.raises(_lib.Fv3HipError, match="kernel_size"):
        ConvModel(big, device)


def test_leading_dims_that_do_not_merge_and_a_bare_single_channel_source(device):
    """Two batch dims stored in the other order cannot be merged into one batch stride as a view: ``predict`` then copies that
    array once and the result has the same bits.  A single-channel source may come without ``z`` -- first in the list too."""
    from fv3net_amd.conv import ConvModel

    rng = np.random.default_rng(80)
    spec = conv_cases.make_spec(rng, {"lat": 1, "T": 19}, 32, 3, 3, {"dQ1": 19})
    h = spec.halos_required
    fields = _to_device(conv_cases.make_inputs(rng, spec, (2, 3), 10 + 2 * h, 10 + 2 * h), device, False)  # [2, 3, z, y, x]
    model = ConvModel(spec, device)
    want = model.predict(fields, halo="input")["dQ1"]
    stored = fields["T"].permute(1, 0, 2, 3, 4).contiguous().permute(1, 0, 2, 3, 4)  # the same values, batch dims swapped in memory
    assert not stored.is_contiguous() and torch.equal(stored, fields["T"])
    got = model.predict({"T": stored, "lat": fields["lat"][:, :, 0]}, halo="input")["dQ1"]
    assert torch.equal(got, want)
