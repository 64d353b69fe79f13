"""Reservoir computing on the host: loading the reference's layout, dump/load round trips, refused transformers, the rank
divider's known answers, the restatement against the reference's recorded predictions, and create()'s validation."""
import ctypes
import json
import os

import numpy as np
import pytest

from fv3net_amd import _lib, fit
from fv3net_amd.reservoir import RankXYDivider, ScaleSpatialConcatZTransformer, SparseMatrix, load_transformer

import reservoir_np as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reservoir")


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("fmt", ["csc", "csr", "coo"])
@pytest.mark.parametrize("name", ["pure-reservoir", "hybrid-reservoir", "reservoir-adapter", "hybrid-reservoir-adapter"])
def test_reference_layout_loads_and_round_trips(tmp_path, fmt, name):
    rng = np.random.RandomState(3)
    hybrid = name.startswith("hybrid")
    m = R.make_model(rng, overlap=1, in_kind="scale-spatial", out_kind="scale-spatial",
                     hybrid_kind="do-nothing" if hybrid else None, input_mask=fmt == "csr", hybrid_mask=hybrid and fmt == "coo")
    state = rng.randn(4, 40) if fmt != "coo" else None
    src = R.write_reference_layout(m, str(tmp_path / "ref"), name=name, fmt=fmt, state=state)
    model = fit.load(src)
    inner = model.model if name.endswith("adapter") else model
    assert type(inner).__name__ == ("HybridReservoirComputingModel" if hybrid else "ReservoirComputingModel")
    indptr, idx, val = inner.reservoir.W_in.csr()
    np.testing.assert_array_equal(indptr, m["w_in"][0])
    np.testing.assert_array_equal(idx, m["w_in"][1])
    np.testing.assert_array_equal(val, m["w_in"][2])
    if state is None:
        assert inner.reservoir.state is None
    else:
        np.testing.assert_array_equal(inner.reservoir.state, state)
    assert (inner.reservoir.input_mask_array is None) == (m["input_mask"] is None)
    assert isinstance(inner.transformers.input, ScaleSpatialConcatZTransformer)
    assert inner.transformers.input.spatial_features == (10, 10, 1)

    out = str(tmp_path / "out")
    fit.dump(model, out)
    assert _files(out) == _files(src)
    again = fit.load(out)
    inner2 = again.model if name.endswith("adapter") else again
    for a, b in ((inner.readout.coefficients, inner2.readout.coefficients),
                 (inner.readout.intercepts, inner2.readout.intercepts),
                 (inner.transformers.input.center, inner2.transformers.input.center),
                 (inner.transformers.output.scale, inner2.transformers.output.scale),
                 (inner.transformers.output.mask, inner2.transformers.output.mask)):
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a, b)
    for k in inner.reservoir.W_in.arrays:
        np.testing.assert_array_equal(inner.reservoir.W_in.arrays[k], inner2.reservoir.W_in.arrays[k])
        np.testing.assert_array_equal(inner.reservoir.W_res.arrays[k], inner2.reservoir.W_res.arrays[k])
    assert inner2.rank_divider == inner.rank_divider
    assert inner2.square_half_hidden_state == inner.square_half_hidden_state
    assert list(inner2.input_variables) == ["a", "b"]
    if hybrid:
        assert inner2.hybrid_variables == ["a", "b"]


@pytest.mark.parametrize("leaf, kind", [("encoder.tf", "dense-autoencoder"), ("sk_transformer.pkl", "sk-transformer")])
def test_foreign_transformers_are_refused_by_type(tmp_path, leaf, kind):
    m = R.make_model(np.random.RandomState(0))
    src = R.write_reference_layout(m, str(tmp_path / "ref"), name="pure-reservoir")
    out_dir = os.path.join(src, "transformers", "output_transformer")
    for f in os.listdir(out_dir):
        os.remove(os.path.join(out_dir, f))
    os.makedirs(os.path.join(out_dir, leaf)) if leaf.endswith(".tf") else open(os.path.join(out_dir, leaf), "wb").close()
    with pytest.raises(ValueError, match=kind):
        fit.load(src)
    with pytest.raises(ValueError, match=kind):
        load_transformer(out_dir)


def test_rank_divider_known_answers():
    g = _golden("domain2_known_answers.json")
    domain = np.arange(16).reshape(4, 4)
    for case in g["get_subdomain"]:
        kw = {k: tuple(case[k]) for k in ("rank_extent", "overlap_rank_extent") if k in case}
        d = RankXYDivider(tuple(case["layout"]), case["overlap"], **kw)
        np.testing.assert_array_equal(d.get_subdomain(domain, case["index"]), case["expected"])
        assert d.get_all_subdomains(domain).shape[0] == 4
    with pytest.raises(ValueError):
        RankXYDivider((2, 2), 0, rank_extent=(4, 4)).get_subdomain(domain, 4)
    with pytest.raises(ValueError):
        RankXYDivider((2, 2), 0, rank_extent=(4, 4)).get_subdomain(domain[0:2], 0)
    f = g["with_feature"]
    stacked = np.concatenate([domain[..., None] + i for i in range(3)], axis=-1)
    d = RankXYDivider((2, 2), 0, rank_extent=(4, 4), z_feature_size=3)
    sub = d.get_subdomain(stacked, 0)
    assert list(sub.shape) == f["shape"]
    np.testing.assert_array_equal(sub[..., 0], f["index0_z0"])
    np.testing.assert_array_equal(sub[..., 2], f["index0_z2"])
    np.testing.assert_array_equal(d.get_subdomain(stacked, 3)[..., 0], f["index3_z0"])
    lead = g["with_leading"]
    stacked = np.concatenate([domain[None] + i for i in range(3)], axis=0)
    d = RankXYDivider((2, 2), 0, rank_extent=(4, 4))
    sub = d.get_subdomain(stacked, 0)
    assert list(sub.shape) == lead["shape"]
    np.testing.assert_array_equal(sub[0], lead["index0_t0"])
    np.testing.assert_array_equal(sub[2], lead["index0_t2"])
    np.testing.assert_array_equal(d.get_subdomain(stacked, 3)[0], lead["index3_t0"])
    fl = g["flatten"]
    d = RankXYDivider(tuple(fl["layout"]), 0, rank_extent=tuple(fl["rank_extent"]), z_feature_size=fl["z_feature_size"])
    assert d.flatten_subdomain_features(np.ones(fl["subdomain_shape"])).shape == (fl["flat_len"],)
    data = np.random.RandomState(0).rand(15, 10, 20, 3)
    np.testing.assert_array_equal(d.merge_all_flat_feature_subdomains(d.get_all_subdomains_with_flat_feature(data)), data)
    tr = g["trim_overlap"]
    d = RankXYDivider(tuple(tr["layout"]), tr["overlap"], overlap_rank_extent=tuple(tr["overlap_rank_extent"]))
    np.testing.assert_array_equal(d.trim_halo_from_rank_data(domain), tr["expected"])
    ini = g["init"][0]
    d = RankXYDivider(tuple(ini["layout"]), ini["overlap"], overlap_rank_extent=tuple(ini["overlap_rank_extent"]))
    assert d.rank_extent == tuple(ini["rank_extent"]) and d.n_subdomains == ini["n_subdomains"]
    assert d == RankXYDivider((2, 2), 1, rank_extent=(4, 4))
    d = RankXYDivider((2, 2), 1, overlap_rank_extent=(4, 4))
    with pytest.raises(ValueError, match="Cannot merge subdomains with overlap"):
        d.merge_all_subdomains(d.get_all_subdomains(domain))
    for bad in (dict(rank_extent=(3, 4)), dict(rank_extent=(4, 3)), dict()):
        with pytest.raises(ValueError):
            RankXYDivider((2, 2), 0, **bad)


def test_rank_divider_dump_load(tmp_path):
    for overlap, z in ((0, None), (1, 3)):
        d = RankXYDivider((2, 2), overlap, rank_extent=(4, 4), z_feature_size=z)
        d.dump(str(tmp_path / "d.yaml"))
        assert RankXYDivider.load(str(tmp_path / "d.yaml")) == d


@pytest.mark.parametrize("test, hybrid", [("test_adapter_predict", True), ("test_nonhybrid_adapter_predict", False)])
def test_restatement_reproduces_regtest(test, hybrid):
    g = _golden("regtest_adapter_predict.json")[test]
    m = R.regtest_model(hybrid)
    a, b = R.regtest_data(True)
    out = R.predict(m, np.zeros((4, 25)), [a[2:-2, 2:-2], b[2:-2, 2:-2]] if hybrid else None)
    for name, arr in zip("ab", out):
        flat = arr.reshape(-1)
        for got, want in zip(np.concatenate([flat[:3], flat[-3:]]), g[name]["first"] + g[name]["last"]):
            assert float(f"{got:.4g}") == want, (name, got, want)


def test_sparse_formats_agree():
    rng = np.random.RandomState(1)
    csr = R.random_csr(rng, 7, 5, 0.5)
    dense = np.zeros((7, 5))
    rows = np.repeat(np.arange(7), np.diff(csr[0]))
    dense[rows, csr[1]] = csr[2]
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        for fmt in ("csc", "csr", "coo"):
            p = os.path.join(d, fmt + ".npz")
            R._save_sparse(p, csr, fmt)
            s = SparseMatrix.load(p)
            assert s.format == fmt
            np.testing.assert_array_equal(s.toarray(), dense)


def _desc(keep, **over):
    """A valid 1x1 descriptor: 2x2 rank, no overlap, state 3, one do-nothing variable."""
    d = _lib.ReservoirDesc()
    d.layout_x = d.layout_y = 1
    d.rank_x = d.rank_y = 2
    d.state_size = 3
    d.input_size = 4
    nz = np.ones(1, np.intc)
    keep.append(nz)
    for t in (d.input, d.output, d.hybrid):
        t.kind = 0
        t.n_variables = 1
        t.var_nz = nz.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    arrays = {"w_in_indptr": np.array([0, 1, 2, 3], np.int64), "w_in_indices": np.array([0, 1, 3], np.int32),
              "w_in_data": np.ones(3), "w_res_indptr": np.array([0, 1, 1, 2], np.int64),
              "w_res_indices": np.array([2, 0], np.int32), "w_res_data": np.ones(2), "coefficients": np.ones((1, 3, 4)),
              "intercepts": np.zeros((1, 4))}
    arrays.update(over.pop("arrays", {}))
    ctypes_of = {np.dtype(np.int64): ctypes.c_int64, np.dtype(np.int32): ctypes.c_int32, np.dtype(np.float64): ctypes.c_double}
    for k, a in arrays.items():
        keep.append(a)
        setattr(d, k, a.ctypes.data_as(ctypes.POINTER(ctypes_of[a.dtype])))
    for k, v in over.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("change, message", [
    (dict(layout_x=3), b"not divisible"),
    (dict(overlap=-1), b"overlap"),
    (dict(state_size=0), b"state_size"),
    (dict(input_size=5), b"input_size"),
    (dict(square=3), b"square"),
    (dict(arrays={"w_in_indptr": np.array([0, 2, 1, 3], np.int64)}), b"indptr decreases"),
    (dict(arrays={"w_res_indptr": np.array([1, 1, 1, 2], np.int64)}), b"indptr[0]"),
    (dict(arrays={"w_in_indices": np.array([0, 1, 4], np.int32)}), b"column index"),
    (dict(arrays={"w_res_indices": np.array([3, 0], np.int32)}), b"column index"),
    (dict(n_hybrid=5), b"n_hybrid"),
])
def test_create_refuses_malformed_descriptors(change, message):
    lib = _lib.load()
    keep = []
    d = _desc(keep, **change)
    h = ctypes.c_void_p()
    assert lib.fv3hip_reservoir_create(ctypes.byref(d), ctypes.byref(h)) == _lib.EINVAL
    assert message in lib.fv3hip_last_error(), lib.fv3hip_last_error()
    assert not h.value


def test_create_refuses_transformer_mismatch():
    lib = _lib.load()
    keep = []
    d = _desc(keep)
    d.input.kind = 1  # scale-spatial whose spatial features are not the input extent
    c = np.zeros(4, np.float32)
    keep.append(c)
    d.input.center = d.input.scale = c.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    d.input.nx, d.input.ny = 3, 2
    h = ctypes.c_void_p()
    assert lib.fv3hip_reservoir_create(ctypes.byref(d), ctypes.byref(h)) == _lib.EINVAL
    assert b"spatial features" in lib.fv3hip_last_error()
    d.input.kind = 7
    assert lib.fv3hip_reservoir_create(ctypes.byref(d), ctypes.byref(h)) == _lib.EINVAL
    assert lib.fv3hip_reservoir_create(None, ctypes.byref(h)) == _lib.EINVAL


def test_plan_refuses_null_arguments():
    """fv3hip_reservoir_plan reads host values only; a null handle or a null output is EINVAL, not a crash."""
    lib = _lib.load()
    out = (ctypes.c_int64 * 8)()
    assert lib.fv3hip_reservoir_plan(None, out) == _lib.EINVAL
    assert b"null reservoir handle" in lib.fv3hip_last_error()
