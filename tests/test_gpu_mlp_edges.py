"""Every instantiation of the MLP kernels (csrc/mlp.hip) at its edges, against the float64 oracle ``oracle/mlp_np.forward``
at the per-level gate of tests/tolerances.py; everything else here is bit for bit or an exact class (NaN / +inf / -inf /
finite).  The cases and the predicted dispatch live in tests/mlp_cases.py; tests/test_host_mlp_edges.py proves without a
GPU that they select all 36 ``mlp_fused_kernel`` instantiations, both ``mlp_small_kernel`` ones and the layered path.
Every model is built with an explicit ``small_limit`` and every call asserts the kernel it ran.

No test here can fault: every array a kernel may touch is allocated with guard space around it, and a store that strays
stays inside the allocation -- a failure is a failed assertion."""
import functools

import numpy as np
import pytest
import torch

import mlp_cases as mc
from oracle import mlp_np
from tolerances import assert_close_per_level

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {"float32": torch.float32, "float64": torch.float64}


# ---- shared, computed once and left unchanged ----
@functools.lru_cache(maxsize=None)
def _spec(case):
    return mc.build_spec(case)


@functools.lru_cache(maxsize=None)
def _clean(case):
    """(sources [sample, feature], float64 oracle, float32 oracle) of a case."""
    src = mc.make_sources(case)
    return src, mlp_np.forward(_spec(case), src, dtype=np.float64), mlp_np.forward(_spec(case), src, dtype=np.float32)


def _n_cu(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def _model(case, device):
    from fv3net_amd.mlp import MlpModel

    return MlpModel(_spec(case), device=device, small_limit=case.small_limit)


def _to_device(case, src, device, layout=None):
    """[sample, feature] numpy arrays -> contiguous device arrays in the case's layout."""
    layout = layout or case.layout
    out = {}
    for k, v in src.items():
        a = torch.from_numpy(np.ascontiguousarray(v))
        # (a fresh array: the strides of a one-feature source are then those of its shape, not what a transpose left)
        t = torch.empty(a.shape if layout == "sample_feature" else a.shape[::-1], dtype=a.dtype, device=device)
        t.copy_(a if layout == "sample_feature" else a.T)
        out[k] = t
    return out


def _sf(case, t, layout=None):
    """A device output as a [sample, feature] numpy array."""
    a = t.cpu().numpy()
    return a if (layout or case.layout) == "sample_feature" else a.T


def _predict(model, case, dev_src, device, n, fast_layout=None, src_dtype=None, out_dtype=None, layout=None, out=None):
    """One call; asserts that it ran the kernel the restated dispatch predicts and returns (outputs, variant)."""
    layout = layout or case.layout
    out_dtype = out_dtype or case.out_dtype
    got = model.predict(dev_src, layout=layout, out_dtype=TORCH_DTYPE[out_dtype], out=out)
    want = mc.expected_variant(_spec(case), n, src_dtype or case.src_dtype, out_dtype,
                               (layout == "feature_sample") if fast_layout is None else fast_layout, _n_cu(device), case.small_limit)
    assert model.last_variant == want, (case.name, model.last_variant, want)
    return got, want


def _gate(case, got, truth, cpu32, rows=None, layout=None, what=""):
    assert set(got) == set(truth), (set(got), set(truth))
    for name in truth:
        g = _sf(case, got[name], layout)
        assert g.shape == truth[name].shape, (name, g.shape, truth[name].shape)
        if rows is not None:
            g, t, c = g[rows], truth[name][rows], cpu32[name][rows]
        else:
            t, c = truth[name], cpu32[name]
        assert_close_per_level(g, t, c, f"{case.name} {name} {what}")


# =====================================================================================================================
# a. every instantiation against the oracle
# =====================================================================================================================
@pytest.mark.parametrize("case", mc.CATALOGUE, ids=lambda c: c.name)
def test_every_instantiation_against_the_oracle(device, case):
    """One catalogue entry: the predicted kernel ran; every output, residual and hidden output passes the per-level gate
    (levels that are exactly 0 in the oracle are exactly 0); a residual row is exactly ``before + difference`` of the
    stored difference row in float32; a limited output stays inside [lo, hi] and reaches both bounds."""
    spec = _spec(case)
    src, truth, cpu32 = _clean(case)
    model = _model(case, device)
    dev_src = _to_device(case, src, device)
    got, variant = _predict(model, case, dev_src, device, case.n)
    _gate(case, got, truth, cpu32)
    for r in spec.residuals:
        diff = _sf(case, got[r.output])
        before = src[r.source][:, :diff.shape[1]].astype(np.float32)
        want = (before + diff.astype(np.float32)).astype(diff.dtype)
        assert np.array_equal(_sf(case, got[r.name]), want), (case.name, r.name)
    for o in spec.outputs:
        y = _sf(case, got[o.name])
        if o.mask is not None:
            assert not y[:, o.mask == 0].any(), (case.name, o.name)
            y = y[:, o.mask != 0]
        if o.min is not None:
            assert y.min() == o.min, (case.name, o.name, y.min())
        if o.max is not None:
            assert y.max() == o.max, (case.name, o.name, y.max())
    if spec.hidden_output and spec.activation == "relu":
        assert (got[spec.hidden_output] >= 0).all()


def test_hidden_output_model_refuses_float64_sources_on_the_fused_kernel(device):
    from fv3net_amd._lib import Fv3HipError

    case = mc._kind_case("hout_fast", 1)
    src, _, _ = _clean(case)
    model = _model(case, device)
    with pytest.raises(mc.VariantRefused):
        mc.expected_variant(_spec(case), case.n, "float64", "float32", True, _n_cu(device), 0)
    with pytest.raises(Fv3HipError, match="float32 sources only"):
        model.predict(_to_device(case, {k: v.astype(np.float64) for k, v in src.items()}, device))


# =====================================================================================================================
# b. a column's bits do not depend on the call
# =====================================================================================================================
@pytest.mark.parametrize("case", [mc._kind_case(kind, ht) for ht in (1, 8) for kind in mc.KINDS], ids=lambda c: c.name)
def test_column_bits_do_not_depend_on_the_call(device, case):
    """Within one variant string: the columns of the 160 / 161-sample call against a call of the first 128 (fast I/O) or
    33 (general) only, and against a call in which the partial tile's columns come first."""
    src, _, _ = _clean(case)
    model = _model(case, device)
    n = case.n
    full, variant = _predict(model, case, _to_device(case, src, device), device, n)
    full = {k: _sf(case, v).copy() for k, v in full.items()}
    xbulk = variant.split(",")[2] == "true"
    head = 128 if xbulk else 33
    part, v_head = _predict(model, case, _to_device(case, {k: v[:head] for k, v in src.items()}, device), device, head)
    assert v_head == variant
    for name in full:
        assert np.array_equal(_sf(case, part[name]), full[name][:head]), (case.name, name, "head")
    order = np.concatenate([np.arange(128, n), np.arange(128)])
    moved, v_moved = _predict(model, case, _to_device(case, {k: v[order] for k, v in src.items()}, device), device, n)
    assert v_moved == variant
    for name in full:
        assert np.array_equal(_sf(case, moved[name]), full[name][order]), (case.name, name, "partial tile first")


@pytest.mark.parametrize("name", ["side-fast-F40", "side-fast-F40-res", "side-fast64-F40", "side-fast-F70-res", "side-hout-F20"])
def test_column_bits_when_a_workgroup_walks_a_full_tile_and_then_the_partial_one(device, name):
    """``128 x n_cu + 32`` samples on the 8-tile fast-I/O kernels (plain, residual, float64 sources): one tile more than
    workgroups, so workgroup 0 takes tile 0 with the branch-free side epilogue and then the 32-sample tile ``n_cu`` with
    the general one inside the same launch; its inputs pass the ``n_samples - 4`` clamp.  The inputs repeat the 160-sample
    call's columns, so the first 128 and the last 32 columns must equal that call's bits."""
    case = next(c for c in mc.CATALOGUE if c.name == name)
    src, _, _ = _clean(case)
    model = _model(case, device)
    dev_src = _to_device(case, src, device)
    small, variant = _predict(model, case, dev_src, device, case.n)
    n_cu = _n_cu(device)
    n_big = 128 * n_cu + 32
    big_src = {k: torch.cat([v[:, :128].repeat(1, n_cu), v[:, 128:160]], dim=1).contiguous() for k, v in dev_src.items()}
    big, v_big = _predict(model, case, big_src, device, n_big)
    assert v_big == variant and variant.startswith("mlp_fused_kernel<8,") and variant.split(",")[2] == "true"
    for out_name in small:
        assert torch.equal(big[out_name][:, :128], small[out_name][:, :128]), (name, out_name, "tile 0")
        assert torch.equal(big[out_name][:, -32:], small[out_name][:, 128:160]), (name, out_name, "partial tile after a full one")
        assert torch.equal(big[out_name][:, 128 * (n_cu - 1):128 * n_cu], small[out_name][:, :128]), (name, out_name, "last full tile")


# =====================================================================================================================
# c. non-finite inputs and their neighbours
# =====================================================================================================================
@pytest.mark.parametrize("case", mc.poison_cases(), ids=lambda c: c.name)
def test_non_finite_inputs_stay_in_their_sample(device, case):
    """A clean call, then the same call with NaN, +inf and -inf in a plain feature and NaN, +inf, -inf, 0 and a negative
    value in a log feature at samples 0, 31, 32, 63, 64, 127, 128, n-4 and n-1 (mlp_cases.poisons).  Pinned:

      * every unpoisoned sample keeps the clean call's bits in every output, residual and hidden output;
      * a NaN-poisoned sample is NaN in every output (the log floor ``v < eps ? eps : v``, the ReLU ``h < 0 ? 0 : h``, the
        limiter's two compares and ``x * mask`` all keep a NaN), its residual too;
      * a sample whose log input is 0, negative or -inf takes the floor and passes the ordinary gate;
      * a +-inf-poisoned sample is not finite where the float32 oracle is not, and where the oracle holds an infinity the
        kernel gives that infinity or NaN.

    The recorded departure: padded hidden features (a width that is no multiple of 32; 64 on the layered path) carry
    zero weights, ``0 x inf`` makes them NaN, and NaN then reaches every output of that sample -- also where the oracle
    keeps an infinity or, behind the limiter or in the hidden output, a finite value.  Such cells (kernel NaN, oracle
    not NaN) are counted; they occur only in +-inf-poisoned samples, all of those samples' cells are such cells when the
    model has padded hidden features, and there is none when it has not -- padded input rows read zeros and add none.
    Measured on an MI355X (the table DEPARTURES below, asserted): width 20 -- 40 to 49 cells per case on the kernels with
    an output tile or a hidden output (all 20 + 20 output and residual cells of the four or five poisoned samples that
    the oracle does not make NaN itself, the limited head's 6, the hidden output's), 4 on the small-output kernels; the
    feature-split kernel 40; the layered path at width 288 40; width 256 -- 0 on all fourteen fused cases (K = 64, and
    K = 12 with 20 padded input rows) and on the feature-split kernel."""
    spec = _spec(case)
    clean_src, bad_src, classes = mc.poisoned_sources(case)
    model = _model(case, device)
    clean, variant = _predict(model, case, _to_device(case, clean_src, device), device, case.n)
    clean = {k: _sf(case, v).copy() for k, v in clean.items()}
    bad, v_bad = _predict(model, case, _to_device(case, bad_src, device), device, case.n)
    assert v_bad == variant
    bad = {k: _sf(case, v) for k, v in bad.items()}
    with np.errstate(invalid="ignore", over="ignore"):
        o64 = mlp_np.forward(spec, bad_src, dtype=np.float64)
        o32 = mlp_np.forward(spec, bad_src, dtype=np.float32)
    assert set(bad) == set(o64)
    nan_s = np.array([s for s, c in classes.items() if c == "nan"])
    inf_s = np.array([s for s, c in classes.items() if c == "inf"])
    floor_s = np.array([s for s, c in classes.items() if c == "floor"], dtype=int)
    untouched = np.array([s for s in range(case.n) if s not in classes])
    finite_rows = np.sort(np.concatenate([untouched, floor_s]))
    departures = 0
    cells = 0
    for name in bad:
        g = bad[name]
        assert np.array_equal(g[untouched], clean[name][untouched]), (case.name, name, "an unpoisoned sample changed")
        assert np.isnan(g[nan_s]).all(), (case.name, name, "a NaN-poisoned sample is not NaN everywhere")
        assert_close_per_level(g[finite_rows], o64[name][finite_rows], o32[name][finite_rows], f"{case.name} {name} (floored log inputs)")
        gi, oi = g[inf_s], o32[name][inf_s]
        assert not np.isfinite(gi[~np.isfinite(oi)]).any(), (case.name, name, "finite where the oracle is not")
        at_inf = np.isinf(oi)
        assert (np.isnan(gi[at_inf]) | (gi[at_inf] == oi[at_inf])).all(), (case.name, name, "another value where the oracle is +-inf")
        departures += int((np.isnan(gi) & ~np.isnan(oi)).sum())
        cells += int((~np.isnan(oi)).sum())
    assert len(floor_s) == 0 or (np.concatenate([bad[k][floor_s] != clean[k][floor_s] for k in bad], axis=1)).any(axis=1).all()
    pad_to = 64 if variant.startswith("layered") else 32
    padded_hidden = spec.width % pad_to != 0
    print(f"DEPARTURE {case.name}: {variant.split(' ')[0]}: {departures} of {cells} cells, padded hidden features: {padded_hidden}")
    assert departures == (cells if padded_hidden else 0), (case.name, departures, cells, padded_hidden)
    assert departures == DEPARTURES[case.name], (case.name, departures)


# cells that are NaN on the device and not in the float32 oracle, per case (all in +-inf-poisoned samples), as measured on
# an MI355X; equal to the number of the oracle's non-NaN cells in those samples where the model has padded hidden
# features and 0 where it has none
DEPARTURES = {
    "poison-general-ht1-normal": 46,
    "poison-fast-ht1-normal": 40,
    "poison-fast-ht1-denormal": 40,
    "poison-general64-ht1-normal": 40,
    "poison-fast64-ht1-normal": 46,
    "poison-fast64-ht1-denormal": 46,
    "poison-hout_general-ht1-normal": 48,
    "poison-hout_fast-ht1-normal": 49,
    "poison-hout_fast-ht1-denormal": 48,
    "poison-smallf-ht1-normal": 4,
    "poison-smallf-ht1-denormal": 4,
    "poison-smallf_hout-ht1-normal": 44,
    "poison-smallf_hout-ht1-denormal": 44,
    "poison-l1short-ht1-normal": 4,
    "poison-general-ht8-normal": 0,
    "poison-fast-ht8-normal": 0,
    "poison-fast-ht8-denormal": 0,
    "poison-general64-ht8-normal": 0,
    "poison-fast64-ht8-normal": 0,
    "poison-fast64-ht8-denormal": 0,
    "poison-hout_general-ht8-normal": 0,
    "poison-hout_fast-ht8-normal": 0,
    "poison-hout_fast-ht8-denormal": 0,
    "poison-smallf-ht8-normal": 0,
    "poison-smallf-ht8-denormal": 0,
    "poison-smallf_hout-ht8-normal": 0,
    "poison-smallf_hout-ht8-denormal": 0,
    "poison-l1short-ht8-normal": 0,
    "poison-small-f32-ht1-normal": 40,
    "poison-small-f64-ht8-normal": 0,
    "poison-layered-ht8-normal": 40,
}


# =====================================================================================================================
# d. no store outside the outputs
# =====================================================================================================================
PATTERN32, PATTERN64 = 0x7FC5A5A5, 0x7FF85A5A5A5A5A5A  # (quiet NaNs with a payload no kernel produces)


def _guarded(shape, dtype, device, layout):
    """(buffer, view): ``view`` has ``shape`` and sits inside ``buffer`` with guard cells on every side; feature_sample
    views keep unit sample stride, a 16-byte aligned base and a feature stride that is a multiple of 16 bytes."""
    f, n = (shape[0], shape[1]) if layout == "feature_sample" else (shape[1], shape[0])
    if layout == "feature_sample":
        big = torch.empty((f + 2, n + 64), dtype=dtype, device=device)
        view = big[1:1 + f, 32:32 + n]
    else:
        big = torch.empty((n + 2, f + 16), dtype=dtype, device=device)
        view = big[1:1 + n, 8:8 + f]
    if dtype == torch.float32:
        big.view(torch.int32).fill_(PATTERN32)
    else:
        big.view(torch.int64).fill_(PATTERN64)
    return big, view


# every instantiation kind at hidden tilings 1 and 8, and the cases whose full tile takes the branch-free side epilogue
# ("plain", "residual") with the partial tile of the same launch on the general one
GUARDED = [mc._kind_case(kind, ht) for ht in (1, 8) for kind in mc.KINDS] + \
          [c for c in mc.CATALOGUE if c.name in ("side-fast-F40", "side-fast-F70-res", "side-fast64-F20", "side-hout-F40")]


@pytest.mark.parametrize("case", GUARDED, ids=lambda c: c.name)
def test_no_store_outside_the_outputs(device, case):
    """Outputs, residual and hidden outputs as views into larger arrays filled with a bit pattern (the fast-I/O kernels
    still run: the variant is asserted): afterwards every guard cell holds the pattern bit for bit and the views hold what
    an ordinary call returned -- the 16-byte stores of 32-row tiles, the sink row of padded rows, the partial tile and the
    per-lane stores of the small-output path all stay inside their rows."""
    spec = _spec(case)
    src, _, _ = _clean(case)
    model = _model(case, device)
    dev_src = _to_device(case, src, device)
    ref, variant = _predict(model, case, dev_src, device, case.n)
    ref = {k: v.clone() for k, v in ref.items()}
    bufs, views = {}, {}
    for name, t in ref.items():
        bufs[name], views[name] = _guarded(tuple(t.shape), t.dtype, device, case.layout)
        if variant.startswith("mlp_fused") and variant.split(",")[2] == "true":  # the views keep the call on the fast path
            assert views[name].stride(1) == 1 and views[name].data_ptr() % 16 == 0 and views[name].stride(0) % 4 == 0
    ints = {torch.float32: torch.int32, torch.float64: torch.int64}
    before = {k: b.view(ints[b.dtype]).clone() for k, b in bufs.items()}
    got, v_guarded = _predict(model, case, dev_src, device, case.n, out=views)
    assert v_guarded == variant
    for name in ref:
        assert got[name].data_ptr() == views[name].data_ptr()
        assert torch.equal(views[name], ref[name]), (case.name, name, "the view differs from an ordinary call")
        after = bufs[name].view(ints[bufs[name].dtype]).clone()
        inside = torch.zeros_like(after, dtype=torch.bool)
        if case.layout == "feature_sample":
            inside[1:1 + ref[name].shape[0], 32:32 + ref[name].shape[1]] = True
        else:
            inside[1:1 + ref[name].shape[0], 8:8 + ref[name].shape[1]] = True
        assert torch.equal(after[~inside], before[name][~inside]), (case.name, name, "a guard cell was written",
                                                                     torch.nonzero((after != before[name]) & ~inside)[:8].tolist())
    assert spec.output_names == list(ref)


# =====================================================================================================================
# e. layouts that must leave the fast path
# =====================================================================================================================
def _offset_copy(t, elements=1):
    """The same values in a flat buffer at element offset ``elements``: the base is 4 (8) bytes off 16-byte alignment."""
    flat = torch.empty(t.numel() + elements, dtype=t.dtype, device=t.device)
    view = flat[elements:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0
    return view


E_CASE = "side-fast-F40-res"  # float32, 160 samples, 8-tile kernel: XBULK=true with the residual side epilogue


@pytest.mark.parametrize("how", ["source off alignment", "output off alignment", "source feature stride n + 1",
                                 "sample_feature slices of a wider array", "expanded source with sample stride 0"])
def test_layouts_that_must_leave_the_fast_path(device, how):
    """A model and a sample count that otherwise select the fast-I/O kernel: each of these layouts must run the general
    instantiation (XBULK=false in the variant string) and pass the oracle gate."""
    case = next(c for c in mc.CATALOGUE if c.name == E_CASE)
    spec = _spec(case)
    src, truth, cpu32 = _clean(case)
    model = _model(case, device)
    n = case.n
    dev_src = _to_device(case, src, device)
    _, fast_variant = _predict(model, case, dev_src, device, n)
    assert fast_variant == "mlp_fused_kernel<8,false,true,false,false,false> epilogue=residual"
    layout, out = "feature_sample", None
    if how == "source off alignment":
        dev_src["a"] = _offset_copy(dev_src["a"])
    elif how == "output off alignment":
        out = {name: torch.empty_like(t) for name, t in model.predict(dev_src).items()}
        out["y"] = _offset_copy(out["y"])
    elif how == "source feature stride n + 1":
        wide = torch.zeros((dev_src["before"].shape[0], n + 1), device=device)
        wide[:, :n] = dev_src["before"]
        dev_src["before"] = wide[:, :n]
        assert dev_src["before"].stride(0) == n + 1
    elif how == "sample_feature slices of a wider array":
        layout = "sample_feature"
        dev_src = {}
        for k, v in src.items():
            wide = torch.zeros((n, v.shape[1] + 5), device=device)
            wide[:, 2:2 + v.shape[1]] = torch.from_numpy(v).to(device)
            dev_src[k] = wide[:, 2:2 + v.shape[1]]
    else:
        # (the residual's `before` array: the network's outputs still differ from sample to sample, so that a level's
        # maximum over the samples stays the scale the gate presumes)
        src = dict(src)
        src["before"] = np.repeat(src["before"][:1], n, axis=0)
        truth, cpu32 = mlp_np.forward(spec, src, dtype=np.float64), mlp_np.forward(spec, src, dtype=np.float32)
        dev_src["before"] = torch.from_numpy(np.ascontiguousarray(src["before"][:1].T)).to(device).expand(-1, n)
        assert dev_src["before"].stride(1) == 0 and dev_src["before"].shape == (src["before"].shape[1], n)
    got, variant = _predict(model, case, dev_src, device, n, fast_layout=False, layout=layout, out=out)
    assert variant == "mlp_fused_kernel<8,false,false,false,false,false> epilogue=general"
    _gate(case, got, truth, cpu32, layout=layout, what=how)


def test_dtype_pairs_and_smallest_calls(device):
    """float64 outputs from float32 sources stay on the fast path (the general epilogue on the 8-tile kernel); a float64
    source paired with a float32 one is promoted, so the float64 instantiation runs; 32 samples are the smallest fast
    call and one sample the smallest general one."""
    case = next(c for c in mc.CATALOGUE if c.name == E_CASE)
    src, truth, cpu32 = _clean(case)
    model = _model(case, device)
    dev_src = _to_device(case, src, device)
    got, variant = _predict(model, case, dev_src, device, case.n, out_dtype="float64")
    assert variant == "mlp_fused_kernel<8,false,true,false,false,false> epilogue=general"
    assert all(t.dtype == torch.float64 for t in got.values())
    _gate(case, got, truth, cpu32, what="float64 outputs")
    mixed = dict(dev_src)
    mixed["a"] = mixed["a"].to(torch.float64)
    got, variant = _predict(model, case, mixed, device, case.n, src_dtype="float64")
    assert variant == "mlp_fused_kernel<8,true,true,false,false,false> epilogue=general"
    _gate(case, got, truth, cpu32, what="a float64 and a float32 source")
    got, variant = _predict(model, case, {k: v[:, :32].contiguous() for k, v in dev_src.items()}, device, 32)
    assert variant == "mlp_fused_kernel<8,false,true,false,false,false> epilogue=general"
    _gate(case, got, {k: v[:32] for k, v in truth.items()}, {k: v[:32] for k, v in cpu32.items()}, what="32 samples")
    # One sample: a level's maximum over one sample is no statistic the gate's "8 x the float32 evaluation" clause could
    # be applied to (that evaluation is often exact there).  Instead: the call runs the general instantiation, a
    # 161-sample call of the same instantiation passes the gate, and the lone sample has that call's bits.
    src161 = {k: np.concatenate([v, v[:1]]) for k, v in src.items()}
    ref, v161 = _predict(model, case, _to_device(case, src161, device), device, 161)
    _gate(case, ref, mlp_np.forward(_spec(case), src161, dtype=np.float64), mlp_np.forward(_spec(case), src161, dtype=np.float32),
          what="161 samples")
    got, variant = _predict(model, case, {k: v[:, :1].contiguous() for k, v in dev_src.items()}, device, 1, fast_layout=False)
    assert variant == v161 == "mlp_fused_kernel<8,false,false,false,false,false> epilogue=general"
    for name in got:
        assert torch.equal(got[name], ref[name][:, :1]), name


# =====================================================================================================================
# the padding rows of the fused kernels' input table
# =====================================================================================================================
@pytest.mark.parametrize("fast", [True, False], ids=["fast-io", "general"])
def test_padding_rows_read_zeros_whatever_the_biases_are(device, fast):
    """K = 33 leaves 31 padding rows in the input table.  They used to point at the packed bias block; with float64
    sources the kernel read its first words as doubles, and two first-layer biases of 2e5 (hidden features 4 and 5, packed
    words 1 and 3) made those doubles exceed the float range: +inf times the padding rows' zero weights was NaN in every
    output of every sample.  The rows now read zeros the model owns."""
    case = mc.padding_case(fast)
    src, truth, cpu32 = _clean(case)
    model = _model(case, device)
    got, variant = _predict(model, case, _to_device(case, src, device), device, case.n)
    assert variant == f"mlp_fused_kernel<2,true,{'true' if fast else 'false'},false,false,false> epilogue=general"
    for name, t in got.items():
        print(f"PADDING {case.name} {name}: NaN cells {int(torch.isnan(t).sum())} of {t.numel()}")
    _gate(case, got, truth, cpu32)
