"""The convolutional predictor at the edges ``test_gpu_conv.py`` does not reach, against the float64 oracle (``conv_np``) with
the same gate (``tolerances.assert_close_per_level``: 1e-5 of the level's scale, no worse than 8x the float32 CPU chain):

* extents around the 16 x 16 tile (1 ... 33, non-square), more than 64 filters (``gridDim.z > 1`` in the hidden layers, a
  padded last N block), channel counts that leave a ragged last K chunk for k = 5 and k = 7, and k = 1 -- the pixels of all
  extents pooled per network, in both layouts (both operand orders of the MFMA, both LDS fill patterns);
* cube halos on faces as small as the halo itself, the three halo routes bit for bit;
* NaN and +-Inf in an input cell: the oracle's map of finite / +Inf / -Inf / NaN, the gate on what is finite, not a bit
  changed outside the receptive field;
* strided, float64 and differently ordered sources, independence of the rest of the batch, and the refusals.

The float32 CPU chain alone against float64, worst per-level error / scale (``tests/test_oracle_conv.py -s``): 1.8e-7 ...
6.6e-7 over the seven networks of the sweep, 0.9e-7 ... 8.1e-7 over the small cubes, 2.1e-7 ... 3.7e-7 on the finite part of
the non-finite cases -- at most 0.08 of the gate.
"""
import numpy as np
import pytest
import torch

import conv_cases

pytestmark = pytest.mark.gpu


def _to_device(fields, dev, channels_last):
    """[..., x, y, z] host arrays -> fresh contiguous device tensors in the layout under test."""
    # (a copy: the shared references are read-only arrays)
    return {k: torch.from_numpy(np.array(v if channels_last else np.swapaxes(v, -1, -3), order="C")).to(dev)
            for k, v in fields.items()}


def _to_xyz(t, channels_last):
    a = t.cpu().numpy()
    return a if channels_last else np.swapaxes(a, -1, -3)


def _same_bits(a, b):
    """Equality of the bit patterns (``torch.equal`` is false wherever a NaN sits)."""
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32),
                                                                                       b.contiguous().view(torch.int32))


def _heads(spec):
    return [(o.name, o.nfeat) for o in spec.outputs]


# ---- 1. shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("name", list(conv_cases.EDGE_NETWORKS))
def test_shape_sweep_matches_the_float64_oracle(device, name, channels_last):
    from fv3net_amd.conv import ConvModel

    spec, parts = conv_cases.sweep_case(name)
    model = ConvModel(spec, device)
    got = {}
    for (nx, ny), fields, _, _ in parts:
        out = model.predict(_to_device(fields, device, channels_last), halo="input", channels_last=channels_last)
        for head, nf in _heads(spec):
            assert out[head].dtype == torch.float32
            assert tuple(out[head].shape) == ((2, nx, ny, nf) if channels_last else (2, nf, ny, nx)), (head, nx, ny)
            got[head, nx, ny] = _to_xyz(out[head], channels_last)
    for head, _ in _heads(spec):
        entries = [(ext, got[(head,) + ext], truth[head], cpu32[head]) for ext, _, truth, cpu32 in parts]
        worst = conv_cases.assert_close_pooled(entries, f"{name} {head}")
        print(f"{name} {head} channels_last={channels_last}: worst per-level error / scale {worst:.2e}")


# ---- 2. cube halos on small faces --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(conv_cases.CUBE_NETWORKS))
def test_small_cubes_match_the_float64_oracle(device, name):
    from fv3net_amd.conv import ConvModel

    spec, parts = conv_cases.cube_case(name)
    model = ConvModel(spec, device)
    got = {}
    for n, cube, _, _ in parts:
        out = model.predict(_to_device(cube, device, False), halo="cube")
        for head, nf in _heads(spec):
            assert tuple(out[head].shape) == (6, nf, n, n)
            got[head, n] = _to_xyz(out[head], False)
    for head, _ in _heads(spec):
        entries = [(f"n = {n}", got[head, n], truth[head], cpu32[head]) for n, _, truth, cpu32 in parts]
        worst = conv_cases.assert_close_pooled(entries, f"{name} {head}")
        print(f"{name} {head}: worst per-level error / scale {worst:.2e}")


def _three_routes(model, cube, device):
    """name -> result per halo route for six faces [6, x, y, z] on the host: the resident cube, the input padded by the
    oracle's ``append_halos``, float32 and float64 strips."""
    from fv3net_amd.cubedsphere.halos import edge_strips, halo_strips

    h = model.spec.halos_required
    dev_cube = _to_device(cube, device, False)
    routes = {"cube": model.predict(dev_cube, halo="cube"),
              "input": model.predict(_to_device(conv_cases.pad_cube(cube, h), device, False), halo="input")}
    for dtype in (torch.float32, torch.float64):
        strips = None
        if h > 0:
            # [6, z, y, x] -> [6, z, x, y] -> edges [6, 4, h, z, n], the variables' channels concatenated
            edges = torch.cat([edge_strips(dev_cube[i.source].transpose(-1, -2).to(dtype), h) for i in model.spec.inputs], dim=-2)
            strips = halo_strips(edges, range(6))
        routes[f"strips {dtype}"] = model.predict(dev_cube, halo="strips", strips=strips)
    return routes


@pytest.mark.parametrize("name", list(conv_cases.CUBE_NETWORKS))
def test_small_cubes_three_halo_routes_are_bit_identical(device, name):
    from fv3net_amd.conv import ConvModel

    spec, parts = conv_cases.cube_case(name)
    model = ConvModel(spec, device)
    for n, cube, _, _ in parts:
        routes = _three_routes(model, cube, device)
        for head, _ in _heads(spec):
            for route, out in routes.items():
                assert _same_bits(out[head], routes["cube"][head]), (name, n, head, route)


# ---- 3. non-finite inputs ----------------------------------------------------------------------------
@pytest.mark.parametrize("value", list(conv_cases.NON_FINITE))
@pytest.mark.parametrize("activation", conv_cases.ACTIVATION_NAMES)
def test_non_finite_input_reaches_its_receptive_field_as_in_the_oracle(device, activation, value):
    """A NaN / +Inf / -Inf in one interior cell of one T channel of sample 0 and in lat's halo corner of sample 1: every
    output element is finite, +Inf, -Inf or NaN exactly where the oracle's is (np.maximum(v, 0) keeps a NaN, tanh(+-Inf) = +-1),
    the finite ones pass the gate, and outside the hit's 5 x 5 outputs (and the one output at the corner) nothing differs by
    a bit from the run without it."""
    from fv3net_amd.conv import ConvModel

    spec, (clean, planted) = conv_cases.non_finite_case(activation, conv_cases.NON_FINITE[value])
    nx, ny = conv_cases.NON_FINITE_EXTENT
    model = ConvModel(spec, device)
    first = model.predict(_to_device(clean[1], device, False), halo="input")
    second = model.predict(_to_device(planted[1], device, False), halo="input")
    untouched = np.ones((2, nx, ny), bool)
    untouched[0][conv_cases.footprint_mask(spec, nx, ny)] = False
    untouched[1, 0, 0] = False
    assert int((~untouched).sum()) == 26
    for head, nf in _heads(spec):
        a, b = _to_xyz(first[head], False), _to_xyz(second[head], False)
        assert a.shape == b.shape == (2, nx, ny, nf)
        conv_cases.assert_close_with_non_finite(a, clean[2][head], clean[3][head], name=f"{activation} clean {head}")
        n_bad = conv_cases.assert_close_with_non_finite(b, planted[2][head], planted[3][head], name=f"{activation} {value} {head}")
        print(f"{activation} {value} {head}: {n_bad} of {2 * nx * ny} pixels non-finite")
        np.testing.assert_array_equal(a.view(np.int32)[untouched], b.view(np.int32)[untouched])
        # (what is inside the footprint did change: the test is not looking at two runs of the same input)
        assert np.all(np.any(a.view(np.int32) != b.view(np.int32), axis=-1)[~untouched]), head


def test_nan_crosses_a_cube_seam_as_in_the_oracle(device):
    """A NaN at T[tile 0, x = 0, y = 3] of a cube with n = 8 (k = 3, depth 3: a halo of 2): the class map equals the oracle's
    on every tile -- on tile 0 and, through the halo, on tile 4 across that seam -- and the three halo routes agree bit for bit."""
    from fv3net_amd.conv import ConvModel

    import conv_np

    rng = np.random.default_rng(310)
    spec = conv_cases.make_spec(rng, {"T": 7, "lat": 1}, 5, 3, 3, {"dQ1": 7, "rain": 1}, activation="relu")
    cube = conv_cases.make_inputs(rng, spec, (6,), 8, 8)
    cube["T"][0, 0, 3, 2] = np.nan
    truth, cpu32 = conv_cases.reference(spec, conv_cases.pad_cube(cube, spec.halos_required))
    assert conv_np.CONNECTIONS[0]["x"][0][0] == 4
    hit = np.isnan(truth["dQ1"]).any(axis=-1)   # [6, x, y]
    assert hit[0].sum() == 3 * 5 and hit[4].sum() == 2 * 5 and hit[[1, 2, 3, 5]].sum() == 0
    routes = _three_routes(ConvModel(spec, device), cube, device)
    for head, _ in _heads(spec):
        got = _to_xyz(routes["cube"][head], False)
        conv_cases.assert_close_with_non_finite(got, truth[head], cpu32[head], name=f"seam {head}")
        for route, out in routes.items():
            assert _same_bits(out[head], routes["cube"][head]), (head, route)


# ---- 4. strides, batch, refusals ---------------------------------------------------------------------
def _strided_setup(device, channels_last, seed):
    from fv3net_amd.conv import ConvModel

    rng = np.random.default_rng(seed)
    spec = conv_cases.make_spec(rng, {"T": 7, "lat": 1}, 33, 3, 3, {"dQ1": 7, "rain": 1})
    h = spec.halos_required
    fields = _to_device(conv_cases.make_inputs(rng, spec, (2,), 11 + 2 * h, 17 + 2 * h), device, channels_last)
    model = ConvModel(spec, device)
    return model, fields, model.predict(fields, halo="input", channels_last=channels_last)


def _x_axis(channels_last):
    return -3 if channels_last else -1


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("how", ["every_second_x", "interior_of_padded_float64", "second_source_other_xy_order"])
def test_strided_sources_give_the_bits_of_contiguous_ones(device, how, channels_last):
    """Views are read in place through their strides.  The first source keeps its x / y order and the layout flag is the same
    in both calls, so the kernel variant (tile orientation, operand order) is the same and only addresses and the LDS fill
    pattern differ: the results are equal bit for bit.  The float64 view holds float32 values, so the conversion is exact."""
    model, fields, want = _strided_setup(device, channels_last, 400)
    x_axis = _x_axis(channels_last)
    if how == "every_second_x":
        views = {}
        for k, t in fields.items():
            shape = list(t.shape)
            shape[x_axis] *= 2
            big = torch.full(shape, float("nan"), dtype=t.dtype, device=device)   # what lies between must not be read
            index = [slice(None)] * t.dim()
            index[x_axis] = slice(0, None, 2)
            big[tuple(index)] = t
            views[k] = big[tuple(index)]
    elif how == "interior_of_padded_float64":
        views = {}
        for k, t in fields.items():
            big = torch.full([2] + [s + 5 for s in t.shape[1:]], float("nan"), dtype=torch.float64 if k == "lat" else t.dtype,
                             device=device)
            index = (slice(None),) + tuple(slice(2, 2 + s) for s in t.shape[1:])
            big[index] = t
            views[k] = big[index]
        assert views["lat"].dtype == torch.float64 and views["T"].dtype == torch.float32
    else:
        lat = fields["lat"]
        stored = lat.transpose(-1, -2).contiguous().transpose(-1, -2) if not channels_last else \
            lat.transpose(-3, -2).contiguous().transpose(-3, -2)
        views = {"T": fields["T"], "lat": stored}
        assert stored.stride() != lat.stride()
    assert not views["lat"].is_contiguous()
    for k, v in views.items():
        assert torch.equal(v.to(torch.float32), fields[k]), k
    got = model.predict(views, halo="input", channels_last=channels_last)
    for head in ("dQ1", "rain"):
        assert _same_bits(got[head], want[head]), (how, head)


def test_source_broadcast_over_the_batch(device):
    """A batch stride of zero (one ``lat`` field expanded over the batch) reads the same cells as its copies."""
    model, fields, _ = _strided_setup(device, False, 401)
    one = fields["lat"][:1]
    want = model.predict({"T": fields["T"], "lat": one.repeat(2, 1, 1, 1)}, halo="input")
    shared = one.expand(2, -1, -1, -1)
    assert shared.stride(0) == 0
    got = model.predict({"T": fields["T"], "lat": shared}, halo="input")
    for head in ("dQ1", "rain"):
        assert _same_bits(got[head], want[head]), head


def test_result_is_independent_of_the_rest_of_the_batch(device):
    """[2, 6, ...] in cube mode: each half equals the prediction of that cube alone, bit for bit."""
    from fv3net_amd.conv import ConvModel

    rng = np.random.default_rng(410)
    spec = conv_cases.make_spec(rng, {"T": 7, "lat": 1}, 33, 3, 3, {"dQ1": 7, "rain": 1}, activation="tanh")
    fields = _to_device(conv_cases.make_inputs(rng, spec, (2, 6), 9, 9), device, False)
    model = ConvModel(spec, device)
    both = model.predict(fields, halo="cube")
    for b in range(2):
        alone = model.predict({k: v[b] for k, v in fields.items()}, halo="cube")
        for head in ("dQ1", "rain"):
            assert tuple(both[head].shape[:2]) == (2, 6)
            assert _same_bits(both[head][b], alone[head]), (b, head)
    assert not _same_bits(both["dQ1"][0], both["dQ1"][1])


def test_empty_batch_returns_empty_outputs(device):
    from fv3net_amd.conv import ConvModel

    spec = conv_cases.make_spec(np.random.default_rng(415), {"T": 3, "lat": 1}, 5, 3, 3, {"dQ1": 3, "rain": 1})
    model = ConvModel(spec, device)
    out = model.predict({"T": torch.zeros((0, 6, 3, 8, 8), device=device), "lat": torch.zeros((0, 6, 8, 8), device=device)}, halo="cube")
    assert tuple(out["dQ1"].shape) == (0, 6, 3, 8, 8) and tuple(out["rain"].shape) == (0, 6, 1, 8, 8)
    out = model.predict({"T": torch.zeros((0, 3, 12, 12), device=device), "lat": torch.zeros((0, 1, 12, 12), device=device)}, halo="input")
    assert tuple(out["dQ1"].shape) == (0, 3, 8, 8)


def test_refusals(device):
    from fv3net_amd import _lib
    from fv3net_amd.conv import ConvModel

    rng = np.random.default_rng(420)
    small = ConvModel(conv_cases.make_spec(rng, {"T": 1}, 4, 2, 3, {"dQ1": 1}), device)   # h = 1
    # the sample index is a grid dimension of at most 65 535
    with pytest.raises(_lib.Fv3HipError, match="65535"):
        small.predict({"T": torch.zeros((65536, 1, 3, 3), device=device)}, halo="input")
    # ... and 65 535 run: the last sample as it comes out alone
    many = torch.from_numpy(conv_cases.make_inputs(rng, small.spec, (65535,), 3, 3)["T"]).to(device).permute(0, 3, 2, 1)
    out = small.predict({"T": many}, halo="input")["dQ1"]
    assert tuple(out.shape) == (65535, 1, 1, 1)
    assert _same_bits(out[-1:], small.predict({"T": many[-1:]}, halo="input")["dQ1"])
    assert bool(torch.isfinite(out).all()) and len(torch.unique(out)) > 60000
    # a halo wider than the face it is read from
    wide = ConvModel(conv_cases.make_spec(rng, {"T": 3}, 3, 2, 7, {"dQ1": 3}), device)    # h = 3
    with pytest.raises(_lib.Fv3HipError, match="wider than the tile"):
        wide.predict({"T": torch.zeros((6, 3, 2, 2), device=device)}, halo="cube")
    for dtype in (torch.int32, torch.float16):
        with pytest.raises(TypeError, match="float32 or float64"):
            wide.predict({"T": torch.zeros((6, 3, 8, 8), dtype=dtype, device=device)}, halo="cube")
    # an input that cannot hold its own halo: 6 x 7 cells for a halo of 3 on either side
    with pytest.raises(ValueError, match="do not hold a halo"):
        wide.predict({"T": torch.zeros((1, 3, 7, 6), device=device)}, halo="input")
