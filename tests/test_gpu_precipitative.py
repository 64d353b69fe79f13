"""fv3hip_precip_closure and the precipitative predictor on the device: the kernel bit for bit against the sequential float32
loop of tests/precipitative_np.py over sizes, dtypes, layouts and aliasing; non-finite values; a cancelling integral; the
whole model against the float64 restatement on both MLP kernels; the dataset API; HIP-graph replay."""
import numpy as np
import pytest
import torch

import precipitative_cases as cases
import precipitative_np as P
from fv3net_amd import fit, ops
from fv3net_amd.graphs import GraphedCall
from fv3net_amd.xr_compat import DataArray, Dataset
from glue_np import assert_same_bits
from tolerances import assert_close_per_level

pytestmark = pytest.mark.gpu


def _device_view(logical, layout, dev):
    """The logical [nz, n] (or [n]) array as a device tensor laid out as ``layout`` says; the gaps of a strided base hold NaN."""
    a = np.asarray(logical)
    if layout == "transposed" and a.ndim == 2:
        return torch.from_numpy(np.ascontiguousarray(a.T)).to(dev).t()
    if layout == "stride2":
        wide = np.full(a.shape[:-1] + (2 * a.shape[-1],), np.nan, a.dtype)
        wide[..., ::2] = a
        return torch.from_numpy(wide).to(dev)[..., ::2]
    if layout == "one_thickness" and a.ndim == 2:
        assert all(np.array_equal(a[0], row) for row in a)
        first = a[:1] if a.shape[0] else np.zeros((1, a.shape[1]), a.dtype)
        return torch.from_numpy(np.ascontiguousarray(first)).to(dev).expand(a.shape[0], a.shape[1])
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run_closure(case, inputs, dev):
    """The kernel on the case's layout and aliasing; checks that what it must not write is unchanged.  Returns numpy."""
    t_res, q_res, cp, delp, pp = inputs
    heads = [None if a is None else torch.from_numpy(a.copy()).to(dev) for a in (t_res, q_res, cp)]   # (None: not read)
    d, p = _device_view(delp, case.layout, dev), _device_view(pp, case.layout, dev)
    if case.layout == "transposed":
        assert d.stride() == (1, case.nz) or case.nz <= 1 or case.n <= 1
    if case.layout == "one_thickness":
        assert d.stride(0) == 0 or case.nz <= 1
    if case.mode == "precip_only":
        dq1, dq2, precip = ops.precip_closure(None, None, heads[2], d, p, couple=False)
        assert dq1 is None and dq2 is None
    else:
        dq1, dq2, precip = ops.precip_closure(heads[0], heads[1], heads[2], d, p, couple=True, in_place=case.mode == "in_place")
        assert (dq1 is heads[0] and dq2 is heads[1]) == (case.mode == "in_place")
    torch.cuda.synchronize()
    assert_same_bits(heads[2].cpu().numpy(), cp, err_msg="col_precip was written")
    if case.mode != "in_place" and t_res is not None:
        assert_same_bits(heads[0].cpu().numpy(), t_res, err_msg="t_res was written")
        assert_same_bits(heads[1].cpu().numpy(), q_res, err_msg="q_res was written")
    assert_same_bits(d.cpu().numpy(), delp, err_msg="delp was written")
    assert_same_bits(p.cpu().numpy(), pp, err_msg="physics_precip was written")
    assert precip.dtype == torch.float32 and tuple(precip.shape) == (case.n,)
    return (None if dq1 is None else dq1.cpu().numpy()), (None if dq2 is None else dq2.cpu().numpy()), precip.cpu().numpy()


def _assert_bitwise(got, want, couple, label):
    assert_same_bits(got[2], want[2], err_msg=f"{label}: precip")
    if couple:
        assert_same_bits(got[0], want[0], err_msg=f"{label}: dQ1")
        assert_same_bits(got[1], want[1], err_msg=f"{label}: dQ2")


@pytest.mark.parametrize("case", cases.KERNEL_CASES, ids=lambda c: c.id)
def test_closure_kernel_is_bitwise_the_sequential_float32_loop(case, device):
    inputs = cases.kernel_inputs(case)
    want = P.closure32(*inputs, couple=case.couple)
    _assert_bitwise(_run_closure(case, inputs, device), want, case.couple, case.id)


def test_closure_kernel_rounds_every_product(device):
    """Values for which a contracted multiply-add gives another sum (checked on the CPU first)."""
    inputs = cases.kernel_inputs(cases.FMA_CASE)
    _, _, cp, delp, pp = inputs
    want = P.closure32(*inputs, couple=False)
    assert np.mean(cases.fma_precip(cp, delp, pp) != want[2]) > 0.5
    _assert_bitwise(_run_closure(cases.FMA_CASE, inputs, device), want, False, "fma")


@pytest.mark.parametrize("value", cases.NONFINITE_VALUES, ids=str)
@pytest.mark.parametrize("which", cases.NONFINITE_ARRAYS)
def test_closure_kernel_with_a_non_finite_value(which, value, device):
    case, col = cases.NONFINITE_CASE, cases.NONFINITE_COLUMN
    clean = cases.kernel_inputs(case, seed=3)
    inputs = cases.nonfinite_inputs(which, value)
    want = P.closure32(*inputs, couple=True)
    if which == "delp" and np.isinf(value):
        assert np.isnan(want[2][col])   # inf * 0
    got = _run_closure(case, inputs, device)
    _assert_bitwise(got, want, True, f"{which}={value}")
    # every other column is what it is without the value
    base = P.closure32(*clean, couple=True)
    others = np.arange(case.n) != col
    for g, b in zip(got, base):
        assert_same_bits(g[..., others], b[..., others], err_msg=f"{which}={value}: other columns")


def test_closure_kernel_on_a_cancelling_integral(device):
    cp, delp, pp = cases.cancellation_inputs()
    _, _, want = P.closure32(None, None, cp, delp, pp, couple=False)
    err, bound, _ = cases.cancellation_gate(want, cp, delp, pp)
    assert np.all(err <= bound)   # (the restatement satisfies its gate by construction)
    case = cases.Case(cp.shape[0], cp.shape[1], "f32", "f32", "contiguous", "precip_only")
    _, _, got = _run_closure(case, (None, None, cp, delp, pp), device)
    err, bound, ratio = cases.cancellation_gate(got, cp, delp, pp)
    print(f"cancellation: worst error / bound {np.max(err / bound):.3f}, median terms / integral {np.median(ratio):.0f}")
    assert np.all(err <= bound), (err.max(), bound.min())
    assert_same_bits(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def _dataset(src, dims, sizes, dtype=np.float64, to=None, coords=None):
    """``src`` (name -> [sample, feature] or [sample]) as a Dataset whose profiles have ``dims`` (one of them "z") and whose
    samples are laid out over the other dims in order; on the device ``to`` if given."""
    sample_dims = [d for d in dims if d != "z"]
    shape = [sizes[d] for d in sample_dims]
    ds = Dataset(coords=coords)
    for name, a in src.items():
        a = np.asarray(a, dtype)
        if a.ndim == 2:
            data = DataArray(a.reshape(shape + [a.shape[1]]), dims=sample_dims + ["z"]).transpose(*dims).values
            var_dims = list(dims)
        else:
            data, var_dims = a.reshape(shape), sample_dims
        data = np.ascontiguousarray(data)
        ds[name] = DataArray(torch.from_numpy(data).to(to) if to is not None else data, dims=var_dims)
    return ds


def _columns(da):
    """A predicted DataArray as [sample, level] (or [sample]) numpy in the sample order of ``_dataset``."""
    if "z" not in da.dims:
        return np.asarray(da.values).reshape(-1)
    rest = [d for d in da.dims if d != "z"]
    return np.asarray(da.transpose(*rest, "z").values).reshape(-1, da.sizes["z"])


@pytest.mark.parametrize("variant", sorted(cases.PARITY_VARIANTS))
def test_model_parity_with_the_float64_restatement(variant, device):
    couple, clip = cases.PARITY_VARIANTS[variant]
    spec = fit.precipitative_spec_from_arrays(**cases.arrays_for_spec(clip=clip))
    model = fit.HipPrecipitativeModel(cases.NAMES_IN, cases.NAMES_OUT, spec, couple_precip_to_dQ1_dQ2=couple)
    model.model.set_small_limit(cases.PARITY_SMALL_LIMIT)
    variants = []
    for n in cases.PARITY_COLUMNS:
        src = cases.state(n)
        out = model.predict(_dataset(src, ("z", "x"), {"x": n}))
        variants.append(model.model.last_variant)
        truth, cpu32 = P.forward(spec, couple, src, dtype=np.float64), P.forward(spec, couple, src, dtype=np.float32)
        for name in ("dQ1", "dQ2"):
            assert out[name].dims == ("z", "x") and out[name].values.dtype == np.float32
            worst = assert_close_per_level(_columns(out[name]), truth[name], cpu32=cpu32[name], name=f"{variant} {name} n={n}")
            print(f"{variant} n={n} {name}: worst level error / level scale {worst:.2e}")
        got = _columns(out["total_precipitation_rate"])
        err, scale, err32 = cases.precip_gate(got, truth["total_precipitation_rate"], cpu32["total_precipitation_rate"], src,
                                              truth["q_tendency_due_to_precip"])
        print(f"{variant} n={n} precip: error {err:.3e}, float32 restatement {err32:.3e}, scale {scale:.3e}")
        cases.assert_precip_gate(got, truth["total_precipitation_rate"], cpu32["total_precipitation_rate"], src,
                                 truth["q_tendency_due_to_precip"], name=f"{variant} n={n}")
    assert variants[0].startswith("mlp_small_kernel") and variants[1].startswith("mlp_fused_kernel"), variants
    assert variants[0] != variants[1]


def _small_model(nz=12, couple=True):
    spec = fit.precipitative_spec_from_arrays(**cases.arrays_for_spec(nz=nz, width=8))
    return fit.HipPrecipitativeModel(cases.NAMES_IN, cases.NAMES_OUT, spec, couple_precip_to_dQ1_dQ2=couple)


def test_dataset_api(tmp_path, device):
    nz, sizes = 12, {"tile": 2, "y": 5, "x": 7}
    n = 2 * 5 * 7
    model = _small_model(nz)
    src = cases.state(n, nz)
    want = P.forward(model.spec, True, src, dtype=np.float32)

    host = _dataset(src, ("tile", "z", "y", "x"), sizes, coords={"x": np.arange(7) * 2.0, "z": np.arange(nz)[::-1].copy()})
    host["unused"] = DataArray(np.zeros(3), dims=["t"])
    before = {k: np.array(v.values, copy=True) for k, v in host.items()}
    out = model.predict(host)
    for k in before:  # predict does not mutate its input
        np.testing.assert_array_equal(host[k].values, before[k])
    assert list(out) == cases.NAMES_OUT
    assert out["dQ1"].dims == out["dQ2"].dims == ("tile", "z", "y", "x")
    assert out["total_precipitation_rate"].dims == ("tile", "y", "x") and "z" not in out["total_precipitation_rate"].dims
    for name in cases.NAMES_OUT:
        assert isinstance(out[name].data, np.ndarray) and out[name].values.dtype == np.float32   # host in, host out
        assert set(out[name].coords) == {"x", "z"} & set(out[name].dims)
        for dim, values in out[name].coords.items():
            np.testing.assert_array_equal(values, host.coords[dim])
    # the kernel's own order of operations: the closure is bit for bit the loop on the heads the device computed, and the
    # whole prediction is close to the float32 restatement
    for name in cases.NAMES_OUT:
        got = _columns(out[name])
        np.testing.assert_allclose(got, want[name], rtol=0, atol=1e-5 * np.max(np.abs(want[name])), err_msg=name)

    # the [..., z] view, device resident: the same numbers, on the device, in the input's order
    dev_ds = _dataset(src, ("y", "x", "z"), {"y": 10, "x": 7}, to=device)
    out_dev = model.predict(dev_ds)
    assert out_dev["dQ1"].dims == ("y", "x", "z") and out_dev["total_precipitation_rate"].dims == ("y", "x")
    for name in cases.NAMES_OUT:
        assert isinstance(out_dev[name].data, torch.Tensor) and out_dev[name].data.is_cuda and out_dev[name].data.dtype == torch.float32
        assert_same_bits(_columns(out_dev[name]), _columns(out[name]), err_msg=name)

    # float32 thickness and float64 physics_precip in one dataset: each is read in its own dtype
    mixed = _dataset(src, ("z", "x"), {"x": n})
    mixed[P.DELP] = DataArray(mixed[P.DELP].values.astype(np.float32), dims=["z", "x"])
    out_mixed = model.predict(mixed)
    src32 = dict(src, **{P.DELP: src[P.DELP].astype(np.float32)})
    want32 = P.forward(model.spec, True, src32, dtype=np.float32)
    got = _columns(out_mixed["total_precipitation_rate"])
    np.testing.assert_allclose(got, want32["total_precipitation_rate"], rtol=0, atol=1e-5 * np.max(np.abs(want32["total_precipitation_rate"])))

    with pytest.raises(KeyError):
        model.predict(Dataset({k: host[k] for k in cases.NAMES_IN if k != P.PHYS_PRECIP}))
    short = _dataset(dict(src, **{P.DELP: src[P.DELP][:, :nz - 1]}), ("z", "x"), {"x": n})
    with pytest.raises(ValueError):
        model.predict(short)

    fit.dump(model, str(tmp_path / "model"))
    loaded = fit.load(str(tmp_path / "model"))
    assert type(loaded) is fit.HipPrecipitativeModel
    again = loaded.predict(host)
    for name in cases.NAMES_OUT:
        assert_same_bits(again[name].values, out[name].values, err_msg=name)


def test_closure_of_the_predictor_is_the_loop_on_the_device_heads(device):
    """The predictor's closure launch against ``closure32`` on the heads the network launch left (read back before the
    closure overwrites them: the same model through ``MlpModel.predict``)."""
    nz, n = 12, 300
    for couple in (True, False):
        model = _small_model(nz, couple)
        src = cases.state(n, nz)
        ds = _dataset(src, ("z", "x"), {"x": n}, to=device)
        heads = model.model.predict({k: ds[k].data.reshape(-1, n) for k in cases.NAMES_IN}, layout="feature_sample")
        heads = {k: v.cpu().numpy() for k, v in heads.items()}
        want = P.closure32(heads["dQ1"], heads["dQ2"], heads["q_tendency_due_to_precip"], src[P.DELP].T, src[P.PHYS_PRECIP], couple)
        out = model.predict(ds)
        assert_same_bits(out["dQ1"].values, want[0])
        assert_same_bits(out["dQ2"].values, want[1])
        assert_same_bits(out["total_precipitation_rate"].values, want[2])


def test_predict_replays_as_a_graph(device):
    nz, n = 12, 520
    model = _small_model(nz)
    ds = _dataset(cases.state(n, nz, seed=1), ("z", "x"), {"x": n}, to=device)
    eager = {k: v.values.copy() for k, v in model.predict(ds).items()}
    call = GraphedCall(lambda: model.predict(ds))   # (the capture records the two launches; a replay runs them)
    result = call.replay()
    torch.cuda.synchronize()
    for name in cases.NAMES_OUT:
        assert result[name].data.is_cuda
        assert_same_bits(result[name].values, eager[name], err_msg=name)
    # new data at the same addresses, then a replay
    second = cases.state(n, nz, seed=2)
    for name in cases.NAMES_IN:
        fresh = np.ascontiguousarray(second[name].T) if second[name].ndim == 2 else second[name]
        ds[name].data.copy_(torch.from_numpy(fresh).to(device))
    eager2 = {k: v.values.copy() for k, v in model.predict(ds).items()}
    assert not np.array_equal(eager2["dQ1"], eager["dQ1"])
    result = call.replay()
    torch.cuda.synchronize()
    for name in cases.NAMES_OUT:
        assert_same_bits(result[name].values, eager2[name], err_msg=name)
