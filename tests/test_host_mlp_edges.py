"""What tests/test_gpu_mlp_edges.py relies on, proved without a GPU: the catalogue of tests/mlp_cases.py selects every
kernel instantiation, and the oracle really shows on the edge cases what the device tests compare with.  If a case is
dropped or a knob changed so that an instantiation is no longer reached, this fails where no GPU is needed."""
import numpy as np
import pytest

import mlp_cases as mc
from oracle import mlp_np


def _variant(case, n_cu=256):
    return mc.expected_variant(mc.build_spec(case), case.n, case.src_dtype, case.out_dtype, case.fast_layout, n_cu,
                               case.small_limit)


def test_catalogue_selects_every_instantiation():
    variants = [_variant(c) for c in mc.CATALOGUE]
    assert len(mc.ALL_FUSED) == 36 and len(set(mc.ALL_FUSED)) == 36
    seen = {mc.instantiation(v) for v in variants}
    missing = [k for k in mc.ALL_FUSED + list(mc.SMALL_KERNELS) if k not in seen]
    assert not missing, missing
    assert any(v.startswith("layered") for v in variants)
    assert seen <= set(mc.ALL_FUSED) | set(mc.SMALL_KERNELS) | {"layered"}, seen
    flavours = {v.split("epilogue=")[1] for v in variants if "epilogue=" in v}
    assert flavours == set(mc.EPILOGUES), flavours
    assert len({c.name for c in mc.CATALOGUE}) == len(mc.CATALOGUE)


def test_catalogue_reaches_the_edges_of_the_eight_tile_fast_kernels():
    """1, 2 and 3 output tiles with and without residual outputs on each of the three 8-tile fast-I/O kernels that have
    an output layer; both widths of every tiling; padded hidden features in every tiling; sample counts at the edge."""
    got = set()
    for c in mc.CATALOGUE:
        v = _variant(c)
        g = mc.fused_geometry(mc.build_spec(c)) if v.startswith("mlp_fused") else None
        if c.name.startswith("side-"):
            got.add((mc.instantiation(v), g["nt_out"], bool(c.residuals), v.split("epilogue=")[1]))
    for inst in ("mlp_fused_kernel<8,false,true,false,false,false>", "mlp_fused_kernel<8,true,true,false,false,false>",
                 "mlp_fused_kernel<8,false,true,true,false,false>"):
        for nt in (1, 2, 3):
            assert (inst, nt, False, "plain") in got, (inst, nt)
            res_flavour = "residual" if inst == "mlp_fused_kernel<8,false,true,false,false,false>" else "general"
            assert (inst, nt, True, res_flavour) in got, (inst, nt)
    for ht, widths in mc.WIDTHS.items():
        used = {c.width for c in mc.CATALOGUE if c.n_hidden and c.width <= 256 and mc.fused_geometry(mc.build_spec(c))["HT"] == ht}
        assert set(widths) <= used, (ht, used)
    for c in mc.CATALOGUE:
        v = _variant(c)
        if v.startswith("mlp_fused"):
            xbulk = v.split(",")[2] == "true"
            assert c.n == (160 if xbulk else 161), c.name


def test_expected_variant_follows_the_sample_count_and_the_limit():
    """The same model on the default rule: at most 32 samples per compute unit go to the feature-split kernel."""
    case = next(c for c in mc.CATALOGUE if c.name == "fast-ht8")
    spec = mc.build_spec(case)
    small = "mlp_small_kernel<false> (32-sample workgroups, features split over 8 waves)"
    assert mc.expected_variant(spec, 8192, "float32", "float32", True, 256, None) == small
    assert mc.expected_variant(spec, 8224, "float32", "float32", True, 256, None).startswith("mlp_fused_kernel<8,false,true,")
    assert mc.expected_variant(spec, 8225, "float32", "float32", True, 256, None).startswith("mlp_fused_kernel<8,false,false,")
    assert mc.expected_variant(spec, 160, "float32", "float32", False, 256, 0).startswith("mlp_fused_kernel<8,false,false,")
    assert mc.expected_variant(spec, 160, "float32", "float64", True, 256, 0) == \
        "mlp_fused_kernel<8,false,true,false,false,false> epilogue=general"
    hout = next(c for c in mc.CATALOGUE if c.name == "hout_fast-ht1")
    with pytest.raises(mc.VariantRefused):
        mc.expected_variant(mc.build_spec(hout), 160, "float64", "float32", True, 256, 0)


def test_log_floor_inputs_in_the_oracle():
    """log(max(x, eps)): an input that is 0, negative, -inf or below eps gives (log(eps) - center) / scale, +inf gives +inf
    and NaN gives NaN -- the table the device kernels' floor ``v < eps ? eps : v`` must reproduce."""
    from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec

    eps, center, scale = 1e-8, -7.5, 3.0
    spec = MlpSpec(inputs=[InputSpec("q", 1, transform="log", eps=eps, center=np.float32(center), scale=np.float32(scale))],
                   hidden_kernels=[], hidden_biases=[], outputs=[OutputSpec("y", 1)],
                   out_kernel=np.ones((1, 1), np.float32), out_bias=np.zeros(1, np.float32))
    x = np.array([0.0, -2.0, -np.inf, 1e-12, 1e-8, 1e-3, np.inf, np.nan])
    with np.errstate(invalid="ignore"):
        y = mlp_np.forward(spec, {"q": x[:, None]}, dtype=np.float64)["y"][:, 0]
    floor = (np.log(np.float64(np.float32(eps))) - center) / scale
    assert np.array_equal(y[:5], np.full(5, floor))
    assert y[5] == (np.log(np.float64(np.float32(1e-3))) - center) / scale
    assert y[6] == np.inf and np.isnan(y[7])


@pytest.mark.parametrize("case", mc.poison_cases(), ids=lambda c: c.name)
def test_poisoned_cases_in_the_oracle(case):
    """NaN-poisoned samples are NaN in every oracle output; the +-inf-poisoned ones hold at least one infinity and at
    least one NaN in the float32 oracle (so the class comparison on the device compares something); samples whose log
    input is floored and all unpoisoned ones are finite."""
    spec = mc.build_spec(case)
    clean, bad, classes = mc.poisoned_sources(case)
    positions = set(classes)
    assert {0, 31, 32, 63, 127, 128, case.n - 4, case.n - 1} <= positions
    with np.errstate(invalid="ignore", over="ignore"):
        o32 = mlp_np.forward(spec, bad, dtype=np.float32)
        o64 = mlp_np.forward(spec, bad, dtype=np.float64)
    all32 = np.concatenate([o32[k] for k in spec.output_names], axis=1)
    all64 = np.concatenate([o64[k] for k in spec.output_names], axis=1)
    nan_s = [s for s, c in classes.items() if c == "nan"]
    inf_s = [s for s, c in classes.items() if c == "inf"]
    rest = np.array([s for s in range(case.n) if classes.get(s) not in ("nan", "inf")])
    assert nan_s and inf_s
    assert np.isnan(all32[nan_s]).all() and np.isnan(all64[nan_s]).all()
    assert np.isinf(all32[inf_s]).any() and np.isnan(all32[inf_s]).any()
    assert not np.isfinite(all32[inf_s]).all(axis=1).any()  # every +-inf-poisoned sample shows it somewhere
    assert np.isfinite(all32[rest]).all() and np.isfinite(all64[rest]).all()
    if any(c == "floor" for c in classes.values()):
        floor_s = [s for s, c in classes.items() if c == "floor"]
        clean64 = np.concatenate([mlp_np.forward(spec, clean, dtype=np.float64)[k] for k in spec.output_names], axis=1)
        assert (all64[floor_s] != clean64[floor_s]).any(axis=1).all()  # the floor changed those samples


@pytest.mark.parametrize("fast", [True, False])
def test_padding_bias_case_in_the_oracle(fast):
    """The oracle of the padding-row case is finite everywhere, its input table has padding rows (K = 33 of 64), and the
    two biases are what turns into +inf when the first four float32 biases of the packed block are read as two doubles."""
    case = mc.padding_case(fast)
    spec = mc.build_spec(case)
    g = mc.fused_geometry(spec)
    assert g["K"] % 32 != 0 and g["padded_input_rows"] == 31 and spec.width >= 8
    assert spec.hidden_biases[0][4] == np.float32(2.0e5) and spec.hidden_biases[0][5] == np.float32(2.0e5)
    out = mlp_np.forward(spec, mc.make_sources(case), dtype=np.float64)
    assert all(np.isfinite(v).all() for v in out.values())
    assert mc.expected_variant(spec, case.n, "float64", "float32", True, 256, 0) == \
        f"mlp_fused_kernel<2,true,{'true' if fast else 'false'},false,false,false> epilogue=general"
    # packed order [tile][register][half]: words 0..3 are hidden features 0, 4, 1, 5
    b = spec.hidden_biases[0]
    with np.errstate(over="ignore"):
        as_double = np.array([b[0], b[4], b[1], b[5]], np.float32).view(np.float64).astype(np.float32)
    assert np.isinf(as_double).all()


def test_catalogue_limits_cut_in_the_oracle():
    """Every limited output of the catalogue reaches each of its bounds in the float64 oracle (so the device test's
    'reaches both bounds' is about the limiter, not about luck), and masked levels are exactly 0."""
    n_limited = 0
    for case in mc.CATALOGUE:
        if not any(lo is not None or hi is not None for _, _, lo, hi, _ in case.outputs):
            continue
        spec = mc.build_spec(case)
        out = mlp_np.forward(spec, mc.make_sources(case), dtype=np.float64)
        for name, nf, lo, hi, n_masked in case.outputs:
            y = out[name][:, n_masked:]
            if lo is not None:
                assert y.min() == lo, (case.name, name)
                n_limited += 1
            if hi is not None:
                assert y.max() == hi, (case.name, name)
            if n_masked:
                assert not out[name][:, :n_masked].any()
    assert n_limited >= 8


@pytest.mark.parametrize("case", mc.CATALOGUE + mc.poison_cases() + [mc.padding_case(True), mc.padding_case(False)],
                         ids=lambda c: c.name)
def test_cases_are_conditioned_for_float32(case):
    """The gate of the device tests is 1e-5 of a level's maximum over the samples.  A case is fit for it only if float32
    arithmetic can meet it at all: the float32 evaluation of the oracle must be within a quarter of that of the float64
    one at every level (a level that cancels down far below its terms, or a hidden unit that the ReLU almost always
    clips, is not).  This holds the case design to the reference's own error, not to what a kernel gives."""
    spec = mc.build_spec(case)
    src = mc.make_sources(case)
    o64, o32 = mlp_np.forward(spec, src, dtype=np.float64), mlp_np.forward(spec, src, dtype=np.float32)
    for name in o64:
        scale = np.max(np.abs(o64[name]), axis=0)
        err = np.max(np.abs(o32[name].astype(np.float64) - o64[name]), axis=0)
        worst = int(np.argmax(err / np.where(scale == 0, 1, scale)))
        assert np.all(err <= 2.5e-6 * scale), (case.name, name, worst, err[worst], scale[worst])
