"""The precipitative predictor without a GPU: the argument checks of fv3hip_precip_closure (every one returns before the
first HIP call), known answers of the numpy restatement (tests/precipitative_np.py), the gates of the GPU tests applied to
the float32 restatement itself, construction / artifact round trip, and the offline training step on the CPU."""
import dataclasses

import numpy as np
import pytest
import yaml

import precipitative_cases as cases
import precipitative_np as P
from fv3net_amd import _lib, fit
from fv3net_amd._lib import EINVAL, F32, F64, OK
from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec
from fv3net_amd.xr_compat import DataArray, Dataset
from glue_np import assert_same_bits
from test_host_glue_args import P as PTR, cases as arg_cases, entry
from tolerances import assert_close_per_level

HEAD4 = ["t_res", "q_res", "dq1", "dq2"]
UNCOUPLED = {"couple": 0, **{name: None for name in HEAD4}}

ENTRY = entry(
    [("t_res", PTR), ("q_res", PTR), ("col_precip", PTR), ("delp", PTR), ("delp_dtype", F64), ("delp_feat_stride", 5),
     ("delp_sample_stride", 1), ("physics_precip", PTR), ("pp_dtype", F32), ("pp_stride", 1), ("nz", 3), ("n", 5), ("couple", 1),
     ("dq1", PTR), ("dq2", PTR), ("precip", PTR), ("stream", None)],
    dtypes=["delp_dtype", "pp_dtype"],
    # no columns: nothing to do; no levels: precip = physics_precip + an empty sum is still written, so those two are needed
    # (that call with both set would launch and is not made here)
    extents={"nz": (EINVAL, EINVAL), "n": (EINVAL, OK)},
    required=["t_res", "q_res", "col_precip", "delp", "physics_precip", "dq1", "dq2", "precip"],
    extra=[({"delp_feat_stride": -1}, EINVAL), ({"delp_sample_stride": -1}, EINVAL), ({"pp_stride": -1}, EINVAL),
           ({"n": 0, "delp_dtype": 7}, EINVAL), ({"n": 0, "pp_stride": -1}, EINVAL),
           # without coupling the residual heads are not looked at; the other arrays still are
           ({**UNCOUPLED, "col_precip": None}, EINVAL), ({**UNCOUPLED, "delp": None}, EINVAL),
           ({**UNCOUPLED, "precip": None}, EINVAL), ({**UNCOUPLED, "physics_precip": None}, EINVAL)])


def test_closure_argument_checks():
    assert len(ENTRY["args"]) == len(_lib.SIGNATURES["fv3hip_precip_closure"][1])
    lib = _lib.load()
    listed = list(arg_cases(ENTRY))
    assert all(changes for _, changes, _ in listed)   # every call spoils something: none would launch
    wrong = []
    for label, changes, expected in listed:
        rc = lib.fv3hip_precip_closure(*[changes.get(arg, good) for arg, good in ENTRY["args"]])
        message = lib.fv3hip_last_error()
        if rc != expected or (rc == EINVAL and not message):
            wrong.append((label, rc, expected, message))
    assert not wrong, wrong


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_closure_known_answers():
    f = np.float32
    c_heat, c_g = f(-2.5e6 / 1004.6), f(-1.0 / 9.80665)
    assert P.C_HEAT == c_heat and P.C_G == c_g and P.C_HEAT.dtype == P.C_G.dtype == np.float32
    t_res = np.array([[1.0, 2.0], [3.0, 4.0]], f)
    q_res = np.array([[0.5, 0.25], [0.125, 1.0]], f)
    cp = np.array([[1e-3, -2e-3], [4e-3, 8e-3]], f)
    delp = np.array([[1000.0, 500.0], [250.0, 125.0]])
    pp = np.array([0.5, 0.25])
    dq1, dq2, precip = P.closure32(t_res, q_res, cp, delp, pp, couple=True)
    for k in range(2):
        for i in range(2):
            assert dq1[k, i] == f(t_res[k, i] + f(c_heat * cp[k, i]))
            assert dq2[k, i] == f(q_res[k, i] + cp[k, i])
    for i in range(2):
        acc = f(f(f(0.0) + f(cp[0, i] * f(delp[0, i]))) + f(cp[1, i] * f(delp[1, i])))
        assert precip[i] == f(f(pp[i]) + f(c_g * acc))
    assert abs(precip[0] - (0.5 - (1.0 + 1.0) / 9.80665)) < 1e-6   # column 0: cp * delp = 1 + 1
    assert abs(dq1[0, 0] - (1.0 - 2.5e6 / 1004.6 * 1e-3)) < 1e-6
    # without coupling only the precipitation is computed
    t2, q2, precip2 = P.closure32(t_res, q_res, cp, delp, pp, couple=False)
    assert t2 is t_res and q2 is q_res
    assert_same_bits(precip2, precip)
    # no levels: an empty sum
    _, _, empty = P.closure32(None, None, np.zeros((0, 2), f), np.zeros((0, 2)), pp, couple=False)
    assert_same_bits(empty, pp.astype(f))


def _linear_relation_spec(nz):
    """No hidden layer, identity normalisation: heads that reproduce the relation of the reference's synthetic dataset
    (test_train.py:124-148) through the coupled closure -- cp = -q, q_res = 2 q, t_res = T - 2 LV/CPD q."""
    names = cases.NAMES_IN
    nfeat = [nz, nz, nz, 1]
    k = sum(nfeat)
    eye, zero = np.eye(nz, dtype=np.float32), np.zeros((nz, nz), np.float32)
    kern = np.zeros((k, 3 * nz), np.float32)
    kern[:nz] = np.concatenate([eye, zero, zero], axis=1)                                                  # T
    kern[nz:2 * nz] = np.concatenate([np.float32(-2 * P.LV / P.CPD) * eye, 2 * eye, -eye], axis=1)          # q
    return MlpSpec(inputs=[InputSpec(n, f) for n, f in zip(names, nfeat)], hidden_kernels=[], hidden_biases=[],
                   outputs=[OutputSpec(h, nz) for h in ("dQ1", "dQ2", "q_tendency_due_to_precip")], out_kernel=kern,
                   out_bias=np.zeros(3 * nz, np.float32), activation="linear")


def test_the_reference_relation_comes_back():
    nz, n = 8, 50
    rng = np.random.default_rng(0)
    spec = _linear_relation_spec(nz)
    spec.validate()
    T, q = rng.uniform(200, 300, (n, nz)), rng.uniform(0, 0.02, (n, nz))
    delp = rng.uniform(300, 1500, (n, nz))
    src = {"air_temperature": T, "specific_humidity": q, P.DELP: delp, P.PHYS_PRECIP: np.zeros(n)}
    want = {"dQ1": T - P.LV / P.CPD * q, "dQ2": q, "total_precipitation_rate": np.sum(delp * q, axis=-1) / P.GRAVITY}
    for dtype, rel in ((np.float64, 1e-6), (np.float32, 2e-6)):
        # float64: what is left is the float32 rounding of the inputs and constants; float32: sums of terms up to
        # 2 LV/CPD q ~ 100 and of 8 levels, a few units of 6e-8 each against values of the size of the terms
        out = P.forward(spec, True, src, dtype=dtype)
        for name, w in want.items():
            assert out[name].shape == w.shape and out[name].dtype == dtype
            np.testing.assert_allclose(out[name], w, rtol=0, atol=rel * np.max(np.abs(w)), err_msg=name)


def test_the_integral_takes_every_level_of_the_raw_thickness():
    """``delp`` clipped to slice(10, None) for the network, cp non-zero at every level: the integral includes levels 0-9."""
    nz, n = 14, 3
    args = cases.arrays_for_spec(nz=nz, width=4, clip={P.DELP: slice(10, None)})
    spec = fit.precipitative_spec_from_arrays(**args)
    assert [i.start for i in spec.inputs] == [0, 0, 10, 0] and [i.nfeat for i in spec.inputs] == [nz, nz, nz - 10, 1]
    src = cases.state(n, nz)
    out = P.forward(spec, True, src, dtype=np.float64)
    cp = out["q_tendency_due_to_precip"]
    assert np.all(cp[:, :10] != 0)
    d32 = src[P.DELP].astype(np.float32).astype(np.float64)
    for i in range(n):
        by_hand = float(np.float32(src[P.PHYS_PRECIP][i])) - sum(cp[i, k] * d32[i, k] for k in range(nz)) / 9.80665
        clipped = float(np.float32(src[P.PHYS_PRECIP][i])) - sum(cp[i, k] * d32[i, k] for k in range(10, nz)) / 9.80665
        assert abs(out["total_precipitation_rate"][i] - by_hand) <= 1e-6 * abs(by_hand)
        assert abs(clipped - by_hand) > 1e-2 * abs(by_hand)
    # changing the thickness of a clipped level changes the precipitation and nothing else
    src2 = dict(src)
    src2[P.DELP] = src[P.DELP].copy()
    src2[P.DELP][:, 3] += 100.0
    out2 = P.forward(spec, True, src2, dtype=np.float64)
    np.testing.assert_array_equal(out2["dQ1"], out["dQ1"])
    assert np.all(out2["total_precipitation_rate"] != out["total_precipitation_rate"])


# ---------------------------------------------------------------------------------------------------------------------
# the inputs and gates of the GPU tests, on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_kernel_case_list_covers_what_it_claims():
    listed = cases.KERNEL_CASES
    assert len(listed) < 100 and len({c.id for c in listed}) == len(listed)
    for axis, sizes in (("nz", cases.NZS), ("n", cases.NS)):
        for size in sizes:
            with_size = [c for c in listed if getattr(c, axis) == size]
            assert {c.couple for c in with_size} == {False, True}, (axis, size)
            assert {(c.delp_dtype, c.pp_dtype) for c in with_size} == set(cases.DTYPES), (axis, size)
            assert {c.layout for c in with_size} == set(cases.LAYOUTS), (axis, size)
            assert {c.mode for c in with_size} == set(cases.MODES), (axis, size)


def test_a_contracted_multiply_add_would_show():
    t_res, q_res, cp, delp, pp = cases.kernel_inputs(cases.FMA_CASE)
    _, _, rounded = P.closure32(None, None, cp, delp, pp, couple=False)
    fused = cases.fma_precip(cp, delp, pp)
    assert np.mean(fused != rounded) > 0.5   # (most columns differ; one would do)


def test_a_late_rounding_of_float64_thickness_would_show():
    case = max((c for c in cases.KERNEL_CASES if c.delp_dtype == "f64" and c.nz == 79 and c.layout != "one_thickness"),
               key=lambda c: c.n)
    _, _, cp, delp, pp = cases.kernel_inputs(case)
    _, _, want = P.closure32(None, None, cp, delp, pp, couple=False)
    acc = np.zeros(case.n, np.float32)
    for k in range(case.nz):
        acc = acc + (cp[k].astype(np.float64) * delp[k]).astype(np.float32)   # the product in double, rounded late
    assert np.any(pp.astype(np.float32) + P.C_G * acc != want)


def test_cancellation_gate_holds_for_the_restatement():
    cp, delp, pp = cases.cancellation_inputs()
    _, _, precip = P.closure32(None, None, cp, delp, pp, couple=False)
    err, bound, ratio = cases.cancellation_gate(precip, cp, delp, pp)
    assert np.median(ratio) > 100        # the integral is far smaller than the sum of its terms
    assert np.all(err <= bound), (err.max(), bound.min())


@pytest.mark.parametrize("variant", sorted(cases.PARITY_VARIANTS))
def test_parity_gates_hold_for_the_float32_restatement(variant):
    couple, clip = cases.PARITY_VARIANTS[variant]
    spec = fit.precipitative_spec_from_arrays(**cases.arrays_for_spec(clip=clip))
    for n in cases.PARITY_COLUMNS:
        src = cases.state(n)
        truth, cpu32 = P.forward(spec, couple, src, dtype=np.float64), P.forward(spec, couple, src, dtype=np.float32)
        for name in ("dQ1", "dQ2"):
            assert_close_per_level(cpu32[name], truth[name], cpu32=cpu32[name], name=name)
        cases.assert_precip_gate(cpu32["total_precipitation_rate"], truth["total_precipitation_rate"],
                                 cpu32["total_precipitation_rate"], src, truth["q_tendency_due_to_precip"], name=variant)


# ---------------------------------------------------------------------------------------------------------------------
# construction and artifact
# ---------------------------------------------------------------------------------------------------------------------
def _model(nz=6, couple=True, clip=None, **kwargs):
    spec = fit.precipitative_spec_from_arrays(**cases.arrays_for_spec(nz=nz, width=4, clip=clip))
    return fit.HipPrecipitativeModel(cases.NAMES_IN, cases.NAMES_OUT, spec, couple_precip_to_dQ1_dQ2=couple, **kwargs)


def test_spec_from_arrays_dump_and_load(tmp_path):
    args = cases.arrays_for_spec(nz=6, width=4, clip={P.DELP: slice(2, None), "dQ1": slice(1, 3)})
    spec = fit.precipitative_spec_from_arrays(**args)
    spec.validate()
    assert [o.name for o in spec.outputs] == ["dQ1", "dQ2", "q_tendency_due_to_precip"]
    # the column-precipitation head takes dQ2's mean and std; only the input clip is applied: no mask, no limits
    np.testing.assert_array_equal(spec.outputs[2].scale, spec.outputs[1].scale)
    np.testing.assert_array_equal(spec.outputs[2].center, spec.outputs[1].center)
    np.testing.assert_array_equal(spec.outputs[1].center, args["output_means"][1])
    assert all(o.mask is None and o.min is None and o.max is None for o in spec.outputs)
    assert spec.inputs[2].start == 2 and spec.inputs[2].nfeat == 4
    np.testing.assert_array_equal(spec.inputs[0].scale, args["input_stds"][0] + np.float32(1e-7))
    np.testing.assert_array_equal(spec.out_kernel, np.concatenate(args["head_kernels"], axis=1))

    model = fit.HipPrecipitativeModel(cases.NAMES_IN, cases.NAMES_OUT, spec, couple_precip_to_dQ1_dQ2=False)
    path = str(tmp_path / "model")
    fit.dump(model, path)
    assert open(tmp_path / "model" / "name").read() == "hip-precipitative"
    config = yaml.safe_load(open(tmp_path / "model" / "config.yaml"))
    assert config == {"input_variables": cases.NAMES_IN, "output_variables": cases.NAMES_OUT, "unstacked_dims": ["z"],
                      "n_halo": 0, "couple_precip_to_dQ1_dQ2": False}
    loaded = fit.load(path)
    assert type(loaded) is fit.HipPrecipitativeModel and loaded.couple_precip_to_dQ1_dQ2 is False
    assert loaded.input_variables == cases.NAMES_IN and loaded.output_variables == cases.NAMES_OUT
    meta, arrays = spec.to_arrays()
    meta2, arrays2 = loaded.spec.to_arrays()
    assert meta2 == meta and sorted(arrays2) == sorted(arrays)
    for key in arrays:
        assert_same_bits(arrays2[key], arrays[key], err_msg=key)


def test_constructor_refuses_what_the_graph_is_not():
    args = cases.arrays_for_spec(nz=6, width=4)
    good = fit.precipitative_spec_from_arrays(**args)
    make = lambda spec, ins=cases.NAMES_IN, outs=cases.NAMES_OUT, **kw: fit.HipPrecipitativeModel(ins, outs, spec, **kw)
    make(good)

    def with_outputs(outputs, n_features):
        return MlpSpec(inputs=good.inputs, hidden_kernels=good.hidden_kernels, hidden_biases=good.hidden_biases, outputs=outputs,
                       out_kernel=good.out_kernel[:, :n_features], out_bias=good.out_bias[:n_features])

    with pytest.raises(ValueError, match="output variables"):
        make(good, outs=["dQ2", "dQ1", "total_precipitation_rate"])
    with pytest.raises(ValueError, match="heads"):   # a wrong head name
        make(with_outputs([OutputSpec("dQ1", 6), OutputSpec("dQ2", 6), OutputSpec("column_precip", 6)], 18))
    with pytest.raises(ValueError, match="heads"):   # a missing head
        make(with_outputs([OutputSpec("dQ1", 6), OutputSpec("dQ2", 6)], 12))
    with pytest.raises(ValueError, match="one size"):
        make(with_outputs([OutputSpec("dQ1", 6), OutputSpec("dQ2", 6), OutputSpec("q_tendency_due_to_precip", 5)], 17))
    for gone in (P.DELP, P.PHYS_PRECIP):
        keep = [i for i, name in enumerate(cases.NAMES_IN) if name != gone]
        a = dict(args, input_variables=[cases.NAMES_IN[i] for i in keep], input_means=[args["input_means"][i] for i in keep],
                 input_stds=[args["input_stds"][i] for i in keep])
        a["hidden_kernels"] = [np.zeros((sum(m.shape[0] for m in a["input_means"]), 4), np.float32), args["hidden_kernels"][1]]
        with pytest.raises(ValueError, match=gone):
            make(fit.precipitative_spec_from_arrays(**a), ins=a["input_variables"])
    with pytest.raises(ValueError, match="n_halo"):
        make(good, n_halo=1)
    with pytest.raises(ValueError):
        fit.precipitative_spec_from_arrays(**dict(args, head_kernels=args["head_kernels"][:2]))


# ---------------------------------------------------------------------------------------------------------------------
# training on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def _relation_batches(nz=8, n=384, seed=0):
    """The reference's synthetic relation (test_train.py:124-148) on physical magnitudes."""
    rng = np.random.default_rng(seed)
    T, q = rng.uniform(200, 300, (n, nz)), rng.uniform(0, 0.02, (n, nz))
    delp = rng.uniform(300, 1500, (n, nz))
    ds = Dataset({
        "air_temperature": DataArray(T.astype(np.float32), dims=["sample", "z"]),
        "specific_humidity": DataArray(q, dims=["sample", "z"]),
        P.DELP: DataArray(delp, dims=["sample", "z"]),
        P.PHYS_PRECIP: DataArray(np.zeros(n), dims=["sample"]),
        "dQ1": DataArray(T - P.LV / P.CPD * q, dims=["sample", "z"]),
        "dQ2": DataArray(q, dims=["sample", "z"]),
        "total_precipitation_rate": DataArray(np.sum(delp * q, axis=-1) / P.GRAVITY, dims=["sample"]),
    })
    return [ds]


def _scaled_mse(model, ds):
    src = {name: ds[name].values for name in model.input_variables}
    out = P.forward(model.spec, model.couple_precip_to_dQ1_dQ2, src, dtype=np.float64)
    total = 0.0
    for name in model.output_variables:
        target = ds[name].values.astype(np.float32)
        total += np.mean(((out[name] - target) / np.std(target, axis=0, dtype=np.float32)) ** 2)
    return total


def test_training_on_the_cpu_learns_and_is_deterministic():
    batches = _relation_batches()
    hp = fit.PrecipitativeHyperparameters(width=16, depth=3, epochs=40, batch_size=64, learning_rate=1e-2, seed=0)
    assert hp.input_variables == cases.NAMES_IN and hp.output_variables == cases.NAMES_OUT
    model = fit.train_precipitative_model(hp, batches, device="cpu")
    assert isinstance(model, fit.HipPrecipitativeModel) and model.couple_precip_to_dQ1_dQ2
    model.spec.validate()
    assert [o.name for o in model.spec.outputs] == ["dQ1", "dQ2", "q_tendency_due_to_precip"]
    assert [o.nfeat for o in model.spec.outputs] == [8, 8, 8] and len(model.spec.hidden_kernels) == 2
    again = fit.train_precipitative_model(hp, batches, device="cpu")
    for a, b in zip(model.spec.to_arrays()[1].values(), again.spec.to_arrays()[1].values()):
        assert_same_bits(a, b)
    untrained = fit.train_precipitative_model(dataclasses.replace(hp, epochs=0), batches, device="cpu")
    before, after = _scaled_mse(untrained, batches[0]), _scaled_mse(model, batches[0])
    print(f"std-scaled MSE on the training data: {before:.4g} untrained, {after:.4g} trained")
    assert after < before, (before, after)
    # the uncoupled graph trains too; a clip that names an output is refused (the predict graph masks no output level)
    loose = fit.train_precipitative_model(dataclasses.replace(hp, epochs=1, couple_precip_to_dQ1_dQ2=False), batches, device="cpu")
    assert loose.couple_precip_to_dQ1_dQ2 is False
    with pytest.raises(ValueError, match="inputs"):
        fit.train_precipitative_model(dataclasses.replace(hp, clip={"dQ1": slice(2, None)}), batches, device="cpu")
