"""Host-side checks of the convolutional predictor: the float64 oracle against a second implementation, the halo rule against
the fixture the reference's own ``AppendHalos`` wrote, the spec's validation and its round trip through the registry, and the
strip exchange on gloo ranks.  No GPU."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml

import conv_cases
import conv_np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "append_halos_reference.npz")


# ---- the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, depth, activation, bias", [(5, 2, "tanh", True), (3, 3, "relu", True), (5, 3, "linear", False)])
def test_conv_np_equals_torch_conv2d_chain(k, depth, activation, bias):
    """Random (hence not transpose-invariant, not symmetric) kernels, k = 5 included, a non-square field: an x / y swap or a
    flipped kernel cannot pass."""
    rng = np.random.default_rng(k * 10 + depth)
    spec = conv_cases.make_spec(rng, {"a": 3, "b": 1}, 5, depth, k, {"p": 4, "q": 1}, activation=activation, bias=bias)
    assert not np.allclose(spec.hidden_kernels[0], spec.hidden_kernels[0].transpose(1, 0, 2, 3))
    h = conv_np.halos_required(k, depth)
    inputs = conv_cases.make_inputs(rng, spec, (2,), 9 + 2 * h, 7 + 2 * h, np.float64)
    got = conv_np.forward(spec, inputs)
    want = conv_cases.torch_chain(spec, inputs, torch.float64)
    for name in ("p", "q"):
        assert got[name].shape == (2, 9, 7, 4 if name == "p" else 1)
        scale = np.max(np.abs(want[name]))
        assert np.max(np.abs(got[name] - want[name])) <= 1e-12 * scale, name


@pytest.mark.parametrize("input_shape, k, depth, features_out, base_output_shape", [
    ((3, 10, 10, 2), 3, 2, 5, (3, 8, 8)),
    ((3, 10, 10, 2), 5, 2, 5, (3, 6, 6)),
    ((3, 10, 10, 2), 3, 3, 5, (3, 6, 6)),
    ((3, 11, 15, 2), 3, 3, 5, (3, 7, 11)),
    ((3, 10, 10, 2), 3, 2, 10, (3, 8, 8)),
])
def test_output_shapes_of_the_reference_table(input_shape, k, depth, features_out, base_output_shape):
    rng = np.random.default_rng(0)
    spec = conv_cases.make_spec(rng, {"a": input_shape[-1]}, 32, depth, k, {"out": features_out})
    out = conv_np.forward(spec, {"a": rng.normal(size=input_shape)})["out"]
    assert out.shape == tuple(base_output_shape) + (features_out,)
    assert spec.halos_required == (input_shape[1] - base_output_shape[1]) // 2


@pytest.mark.parametrize("k, depth, want", [(3, 1, 0), (3, 2, 1), (5, 2, 2), (3, 3, 2), (3, 4, 3), (7, 2, 3), (1, 3, 0)])
def test_halos_required_known_answers(k, depth, want):
    from fv3net_amd.conv import halos_required

    assert halos_required(k, depth) == want == conv_np.halos_required(k, depth)


# ---- halos -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_halo", [1, 3])
def test_append_halos_equals_the_reference_fixture(n_halo):
    from fv3net_amd.cubedsphere.halos import append_halos

    with np.load(GOLDEN) as z:
        field, want = z["input"], z[f"padded_{n_halo}"]
    assert len(np.unique(field)) == field.size
    np.testing.assert_array_equal(append_halos(field, n_halo), want)
    np.testing.assert_array_equal(append_halos(torch.from_numpy(field), n_halo).numpy(), want)
    np.testing.assert_array_equal(conv_np.append_halos(field, n_halo), want)


def _cube_dataset(nz=3, n=6, value=None):
    from fv3net_amd.xr_compat import DataArray, Dataset

    rng = np.random.default_rng(1)
    fill = (lambda shape: np.full(shape, value)) if value is not None else (lambda shape: rng.normal(size=shape))
    return Dataset({
        "a": DataArray(fill((6, n, n, nz)), dims=("tile", "x", "y", "z"), coords={"tile": np.arange(6), "x": np.arange(n) + 0.5}),
        "b": DataArray(fill((2, n, 6, n)), dims=("time", "y", "tile", "x")),
    })


@pytest.mark.parametrize("n_halo", [1, 3])
def test_append_halos_dataset_properties(n_halo):
    """tests/test_halos.py:52-76 of the reference: ones in -> ones on all four strips, zeros in all four corners, x and y
    extended by 2 n_halo, other dims as they were, coordinates dropped."""
    from fv3net_amd.cubedsphere import append_halos

    ds = _cube_dataset(value=1.0)
    out = append_halos(ds, n_halo)
    h, n = n_halo, 6
    for name in ("a", "b"):
        da = out[name]
        assert da.dims == ds[name].dims
        assert {d: s for d, s in da.sizes.items()} == {d: s + (2 * h if d in ("x", "y") else 0) for d, s in ds[name].sizes.items()}
        v = da.transpose("tile", *[d for d in da.dims if d not in ("tile", "x", "y")], "x", "y").values
        for xs in (slice(0, h), slice(h + n, None)):
            for ys in (slice(0, h), slice(h + n, None)):
                assert np.all(v[..., xs, ys] == 0)
            assert np.all(v[..., xs, h:h + n] == 1)
            assert np.all(v[..., h:h + n, xs] == 1)
        assert np.all(v[..., h:h + n, h:h + n] == 1)
    assert "x" not in out.coords


def test_append_halos_zero_halo_and_errors():
    from fv3net_amd.cubedsphere import append_halos
    from fv3net_amd.xr_compat import DataArray, Dataset

    ds = _cube_dataset()
    assert append_halos(ds, 0) is ds
    one = Dataset({"a": DataArray(np.zeros((1, 4, 4)), dims=("tile", "x", "y"))})
    with pytest.raises(ValueError):
        append_halos(one, 1)
    with pytest.raises(ValueError):
        append_halos(Dataset({"a": DataArray(np.zeros((4, 4)), dims=("x", "y"))}), 1)
    with pytest.raises(ValueError):
        append_halos(np.zeros((5, 4, 4)), 1)


def test_line_zero_equals_halos_from_rows():
    """The first halo line is the one-cell halo the coarse-graining path already exchanges (``grid.halos_from_rows``,
    pinned by the reference's pressure-level fixtures)."""
    from fv3net_amd.cubedsphere.grid import halos_from_rows
    from fv3net_amd.cubedsphere.halos import edge_strips, halo_strips

    rng = np.random.default_rng(2)
    field_yx = torch.from_numpy(rng.normal(size=(6, 3, 8, 8)))  # grid.py's layout [tile, z, y, x]
    rows = torch.stack([field_yx[..., :, 0], field_yx[..., :, -1], field_yx[..., 0, :], field_yx[..., -1, :]], dim=1)
    strips = halo_strips(edge_strips(field_yx.transpose(-1, -2), 2), range(6))  # [6, 4, 2, z, n]
    for axis, (lo, hi) in (("x", (0, 1)), ("y", (2, 3))):
        want_lo, want_hi = halos_from_rows(rows, range(6), axis)
        np.testing.assert_array_equal(strips[:, lo, 0].numpy(), want_lo.numpy())
        np.testing.assert_array_equal(strips[:, hi, 0].numpy(), want_hi.numpy())


# ---- spec, predictor, registry -----------------------------------------------------------------------
def _small_spec(**kw):
    args = dict(channels={"T": 4, "lat": 1}, filters=5, depth=3, k=3, heads={"dQ1": 4, "rain": 1}, activation="tanh")
    args.update(kw)
    return conv_cases.make_spec(np.random.default_rng(3), **args)


def test_spec_validation():
    from fv3net_amd.conv import ConvSpec

    spec = _small_spec()
    assert (spec.depth, spec.kernel_size, spec.filters, spec.halos_required, spec.n_in_channels) == (3, 3, 5, 2, 5)
    assert spec.flops_per_pixel == 2 * 9 * 5 * 5 + 2 * 9 * 5 * 5 + 2 * 5 * 5
    with pytest.raises(ValueError, match="depth"):
        ConvSpec(spec.inputs, [], [], spec.outputs, "relu")  # depth = 1
    with pytest.raises(ValueError, match="odd"):
        ConvSpec(spec.inputs, [np.zeros((2, 2, 5, 5), np.float32)], None, spec.outputs, "relu")
    with pytest.raises(ValueError, match="filters=0"):
        ConvSpec(spec.inputs, [np.zeros((3, 3, 5, 0), np.float32)], None, spec.outputs, "relu")
    with pytest.raises(ValueError, match="activation"):
        ConvSpec(spec.inputs, spec.hidden_kernels, spec.hidden_biases, spec.outputs, "gelu")
    with pytest.raises(ValueError, match="shape"):
        ConvSpec(spec.inputs, [spec.hidden_kernels[0], np.zeros((3, 3, 4, 5), np.float32)], None, spec.outputs, "relu")


def test_predictor_round_trip_through_the_registry(tmp_path):
    import fv3net_amd.fit as fit

    spec = _small_spec()
    model = fit.HipConvolutionalModel(["T", "lat"], ["dQ1", "rain"], spec)
    assert model.n_halo == 2
    fit.dump(model, str(tmp_path / "m"))
    assert open(tmp_path / "m" / "name").read() == "hip-convolutional"
    with open(tmp_path / "m" / "config.yaml") as f:
        assert yaml.safe_load(f) == {"input_variables": ["T", "lat"], "output_variables": ["dQ1", "rain"],
                                     "unstacked_dims": ["x", "y", "z"], "n_halo": 2}
    back = fit.load(str(tmp_path / "m"))
    assert isinstance(back, fit.HipConvolutionalModel) and back.spec.activation == "tanh"
    (m0, a0), (m1, a1) = spec.to_arrays(), back.spec.to_arrays()
    assert m0 == m1 and sorted(a0) == sorted(a1)
    for key in a0:
        np.testing.assert_array_equal(a0[key], a1[key])

    # a spec.yaml naming an activation this package does not run must not load as something else
    with open(tmp_path / "m" / "spec.yaml") as f:
        meta = yaml.safe_load(f)
    meta["activation"] = "gelu"
    with open(tmp_path / "m" / "spec.yaml", "w") as f:
        yaml.safe_dump(meta, f)
    with pytest.raises(ValueError, match="gelu"):
        fit.load(str(tmp_path / "m"))


def test_predictor_refusals():
    import fv3net_amd.fit as fit

    spec = _small_spec()
    with pytest.raises(ValueError, match="n_halo"):
        fit.HipConvolutionalModel(["T", "lat"], ["dQ1"], spec, n_halo=1)
    with pytest.raises(ValueError):
        fit.HipConvolutionalModel(["T", "lat"], ["nope"], spec)
    fit.HipConvolutionalModel(["T", "lat"], ["dQ1"], spec, n_halo=2)
    no_bias = _small_spec(bias=False)
    meta, arrays = no_bias.to_arrays()
    assert not meta["hidden_bias"] and not any("hidden0_bias" in k for k in arrays)


def test_conv_spec_from_arrays_takes_keras_layouts():
    import fv3net_amd.fit as fit

    rng = np.random.default_rng(4)
    spec = fit.conv_spec_from_arrays(
        ["T", "lat"], [rng.normal(size=4), 0.5], [rng.uniform(1, 2, 4), 2.0],
        [rng.normal(size=(3, 3, 5, 6)), rng.normal(size=(3, 3, 6, 6))], [np.zeros(6), np.zeros(6)],
        ["dQ1"], [rng.normal(size=(1, 1, 6, 4))], [np.zeros(4)], [np.zeros(4)], [np.ones(4)], activation="relu")
    assert (spec.depth, spec.filters, spec.n_in_channels, spec.halos_required) == (3, 6, 5, 2)
    assert spec.inputs[1].scale[0] == np.float32(2.0) + np.float32(1e-7)
    assert spec.outputs[0].kernel.shape == (6, 4)


# ---- the strip exchange on gloo ranks ----------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _cube(h=2, n=8, nz=3):
    return torch.from_numpy(np.random.default_rng(6).normal(size=(6, nz, n, n)).astype(np.float32))


def _strip_worker(rank, size, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=size)
    from fv3net_amd import parallel
    from fv3net_amd.cubedsphere.halos import edge_strips, halo_strips

    mine = parallel.tiles_of_rank(size, rank)
    local = _cube()[mine]  # the same cube on every rank; each keeps its own tiles
    table = parallel.exchange_edge_strips(edge_strips(local, 2))
    assert tuple(table.shape) == (6, 4, 2, 3, 8)
    np.save(os.path.join(out_dir, f"strips_{rank}.npy"), halo_strips(table, mine).numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("size", [2, 6])
def test_sharded_strips_equal_the_single_process_fill(tmp_path, size):
    from fv3net_amd import parallel
    from fv3net_amd.cubedsphere.halos import append_halos_tensor, edge_strips, fill_halos, halo_strips

    mp.spawn(_strip_worker, args=(size, _free_port(), str(tmp_path)), nprocs=size, join=True)
    cube = _cube()
    want = halo_strips(edge_strips(cube, 2), range(6))
    padded = append_halos_tensor(cube, 2)
    for rank in range(size):
        mine = parallel.tiles_of_rank(size, rank)
        got = np.load(tmp_path / f"strips_{rank}.npy")
        np.testing.assert_array_equal(got, want[mine].numpy())
        np.testing.assert_array_equal(fill_halos(cube[mine], torch.from_numpy(got)).numpy(), padded[mine].numpy())
