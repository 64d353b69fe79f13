"""Every instantiation of the split-bf16 MLP kernel (csrc/mlp_bf16x3.hip) at its edges.  The cases, the predicted dispatch,
the tracer models and the emulation of the kernel's product live in tests/mlp3_cases.py; tests/test_host_mlp3_edges.py
proves without a GPU that the catalogue selects all 16 rows of ``kMlp3Table`` and every run-time path, and that the tracer
bound tells a kernel that drops one of the six cross products from one that keeps them.  Every call here goes through
``_run``, which asserts the kernel that ran (``last_variant == expected_variant3(...)``) and that the arrays are laid out
as the case says.

No test here can fault: every array a kernel may touch is a view into a larger allocation with guard space around it
(sources: NaN around them and in the stride padding past ``n``; outputs: a pattern around them, in the stride padding
and over the 32 rows behind them, where the padding features of a last tile would land), and ``_run`` checks after every
call that the pattern is intact and the sources unchanged.  A stray access fails an assertion.

Truth is the float64 oracle ``oracle/mlp_np.forward`` at the per-level gate of tests/tolerances.py with the split-bf16
tests' ``slack32=2e-7``; everything else is bit for bit, an exact class (NaN / not finite), or the derived tracer bound.
"""
import functools

import numpy as np
import pytest
import torch

import mlp3_cases as m3
from oracle import mlp_np
from tolerances import assert_close_per_level

pytestmark = pytest.mark.gpu

GUARD = 64                 # floats in front of every array (a multiple of 4: the 16-byte path stays reachable)
PAD = 8                    # stride padding columns past n (the stride is a multiple of 4 unless the case says otherwise)
PATTERN = -1.2345678e30    # what guards and untouched output cells hold
EXTRA_ROWS = 2             # feature rows behind the last one a model needs, in every source: read by nobody


# ---- shared, computed once and left unchanged ----
@functools.lru_cache(maxsize=None)
def _spec(case):
    return m3.build_spec(case)


@functools.lru_cache(maxsize=None)
def _clean(case):
    """(sources [sample, feature], float64 oracle, float32 oracle) of a case."""
    src = m3.make_sources(case)
    return src, mlp_np.forward(_spec(case), src, dtype=np.float64), mlp_np.forward(_spec(case), src, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _model_cached(case, device):
    from fv3net_amd.mlp import MlpModelSplitBf16

    return MlpModelSplitBf16(_spec(case), device=device)


def _n_cu(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


class _Array:
    """A [rows, n] float32 view (feature stride ``fs``) at float ``base`` of a flat allocation filled with ``fill``."""

    def __init__(self, rows, n, device, fill, offset=0, stride_extra=0, tail_rows=0):
        self.rows, self.n = rows, n
        self.fs = (n + 3) // 4 * 4 + PAD + stride_extra
        self.base = GUARD + offset
        self.buf = torch.full((self.base + (rows + tail_rows) * self.fs + GUARD,), fill, dtype=torch.float32, device=device)
        self.view = torch.as_strided(self.buf, (rows, n), (self.fs, 1), self.base)
        assert self.buf.data_ptr() % 256 == 0
        self.fill = fill

    def aligned(self, rows=None):
        """The 16-byte rule for the first ``rows`` rows as the library sees them (the stride of a single row means nothing)."""
        return self.view.data_ptr() % 16 == 0 and ((self.rows if rows is None else rows) == 1 or self.fs % 4 == 0)

    def outside_is_untouched(self):
        """Everything but the view still holds the fill (bit for bit)."""
        b = self.buf.clone()
        torch.as_strided(b, (self.rows, self.n), (self.fs, 1), self.base).fill_(self.fill)
        return bool((b.view(torch.int32) == torch.full_like(b, self.fill).view(torch.int32)).all())


def _unread_features(spec, source, nfeat):
    read = set()
    for i in spec.inputs:
        if i.source == source:
            read |= set(range(i.start, i.start + i.nfeat))
    nf_out = {o.name: o.nfeat for o in spec.outputs}
    for r in spec.residuals:
        if r.source == source:
            read |= set(range(nf_out[r.output]))
    return [f for f in range(nfeat) if f not in read]


def _sources(spec, src_np, device, misalign="", poison=True):
    """name -> _Array of the [sample, feature] numpy sources.  ``poison``: NaN in the guards, the stride padding, the rows
    behind the last feature and every feature no input or residual reads; else 0.5 there and the drawn values in the
    unread features (the clean call a poisoned one must reproduce bit for bit)."""
    fill = float("nan") if poison else 0.5
    res_src = spec.residuals[0].source if spec.residuals else None
    arrays = {}
    for name in spec.sources:
        a = np.ascontiguousarray(src_np[name].T, dtype=np.float32)
        if poison:
            a = a.copy()
            a[_unread_features(spec, name, a.shape[0])] = np.nan
        arr = _Array(a.shape[0] + EXTRA_ROWS, a.shape[1], device, fill, offset=1 if (misalign == "res_src" and name == res_src) else 0)
        arr.view[:a.shape[0]].copy_(torch.from_numpy(a))
        arr.before = arr.buf.clone()
        arrays[name] = arr
    return arrays


def _outputs(spec, n, device, misalign=""):
    names = spec.output_names
    nfeat = spec.output_nfeat()
    direct = [k for k in names if k != spec.hidden_output]
    arrays = {}
    for name in names:
        offset = 1 if ((misalign == "out_ptr" and name == direct[0]) or (misalign == "hout" and name == spec.hidden_output)) else 0
        extra = 1 if (misalign == "out_stride" and name == direct[-1]) else 0
        arrays[name] = _Array(nfeat[name], n, device, PATTERN, offset=offset, stride_extra=extra, tail_rows=32)
    return arrays


def _run(model, spec, src_np, device, misalign="", poison=True, name=""):
    """One call on guarded arrays; asserts the layout, the kernel that ran, the guards and that no source changed.
    Returns ({output: [sample, feature] device tensor}, variant)."""
    n = next(iter(src_np.values())).shape[0]
    src = _sources(spec, src_np, device, misalign, poison)
    out = _outputs(spec, n, device, misalign)
    direct = [out[k] for k in spec.output_names if k != spec.hidden_output]
    layout = m3.Layout(outputs_ok=all(a.aligned() for a in direct),
                       res_sources_ok=all(src[r.source].aligned(src[r.source].rows - EXTRA_ROWS) for r in spec.residuals),
                       hout_ok=out[spec.hidden_output].aligned() if spec.hidden_output else True)
    declared = m3.Layout(outputs_ok=misalign not in ("out_ptr", "out_stride") or not direct,
                         res_sources_ok=misalign != "res_src" or not spec.residuals, hout_ok=misalign != "hout" or not spec.hidden_output)
    assert layout == declared, (name, misalign, layout)
    got = model.predict({k: a.view[:a.rows - EXTRA_ROWS] for k, a in src.items()}, out={k: a.view for k, a in out.items()})
    want = m3.expected_variant3(spec, n, layout)
    assert model.last_variant == want, (name, model.last_variant, want)
    torch.cuda.synchronize(device)
    assert set(got) == set(spec.output_names)
    for k, a in out.items():
        assert got[k].data_ptr() == a.view.data_ptr()
        assert a.outside_is_untouched(), (name, k, "a store outside the output (guards, stride padding, rows behind it)")
    for k, a in src.items():
        assert bool((a.buf.view(torch.int32) == a.before.view(torch.int32)).all()), (name, k, "a source was written")
    return {k: a.view.T for k, a in out.items()}, want


def _np(outs):
    return {k: v.cpu().numpy() for k, v in outs.items()}


def _gate(name, got, truth, cpu32, rows=None):
    assert set(got) == set(truth)
    for k in truth:
        g, t, c = got[k], truth[k], cpu32[k]
        assert g.shape == t.shape, (name, k, g.shape, t.shape)
        if rows is not None:
            g, t, c = g[rows], t[rows], c[rows]
        assert_close_per_level(g, t, c, f"{name} {k}", slack32=2e-7)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =====================================================================================================================
# a. every catalogue case against the float64 oracle
# =====================================================================================================================
@pytest.mark.parametrize("case", m3.CATALOGUE, ids=lambda c: c.name)
def test_every_case_against_the_oracle(device, case):
    """The predicted kernel ran; every output, residual and hidden output passes the per-level gate; a residual row is
    ``before + stored difference row`` bit for bit in float32; the hidden output is >= 0."""
    spec = _spec(case)
    src, truth, cpu32 = _clean(case)
    got, variant = _run(_model_cached(case, device), spec, src, device, case.misalign, name=case.name)
    got = _np(got)
    _gate(case.name, got, truth, cpu32)
    for r in spec.residuals:
        diff = got[r.output]
        assert np.array_equal(got[r.name], src[r.source][:, :diff.shape[1]] + diff), (case.name, r.name)
    if spec.hidden_output:
        assert (got[spec.hidden_output] >= 0).all()


# =====================================================================================================================
# b. a column's bits do not depend on the call
# =====================================================================================================================
FAMILIES = ["t1-F5", "t1r-F32", "t3-F65", "t3r-F96", "t5-F129", "t5r-F160", "t13-F385", "t13r-F385", "valu4-hout", "cell-G2",
            "hout-mfma", "hout-mfma-res"]


def _slow_knob(spec):
    return "out_ptr" if spec.outputs else "hout"


@pytest.mark.parametrize("name", FAMILIES)
def test_column_bits_do_not_depend_on_the_call(device, name):
    """260 aligned samples (two tiles and a quad, the 16-byte epilogue) against: a call of the first 128; a call with the
    partial tile's columns moved to the front; the same call with one array off the 16-byte rule (the 4-byte epilogue:
    both perform the same float32 ``acc + bias`` and ``before + (acc + bias)``); and 259 samples (a ragged quad)."""
    case = m3.by_name(name)
    spec, model = _spec(case), _model_cached(case, device)
    src = m3.make_sources(case, 260)
    full, variant = _run(model, spec, src, device, name=name)
    assert m3.row(variant).endswith(",true>")
    head, v_head = _run(model, spec, {k: v[:128] for k, v in src.items()}, device, name=name)
    assert v_head == variant
    order = np.concatenate([np.arange(256, 260), np.arange(256)])
    moved, v_moved = _run(model, spec, {k: v[order] for k, v in src.items()}, device, name=name)
    assert v_moved == variant
    slow, v_slow = _run(model, spec, src, device, misalign=_slow_knob(spec), name=name)
    assert v_slow == variant.replace(",true>", ",false>")
    ragged, v_ragged = _run(model, spec, {k: v[:259] for k, v in src.items()}, device, name=name)
    assert v_ragged == v_slow
    for k in full:
        assert _same_bits(head[k], full[k][:128]), (name, k, "first 128")
        assert _same_bits(moved[k], full[k][torch.from_numpy(order).to(device)]), (name, k, "partial tile first")
        assert _same_bits(slow[k], full[k]), (name, k, "4-byte against 16-byte epilogue")
        assert _same_bits(ragged[k], full[k][:259]), (name, k, "259 samples")


@pytest.mark.parametrize("name", ["t13r-F385", "t1-F32", "t5r-F160", "hout-mfma-res", "valu4-hout", "cell-G2"])
def test_column_bits_when_the_persistent_loop_wraps(device, name):
    """``128 n_cu + 4`` samples (16-byte epilogue) and ``128 n_cu + 5`` (4-byte): one tile more than workgroups, so
    workgroup 0 walks a full tile and then the partial one, and the chunk requests of its first tile's last k-steps ask
    for the next tile's first chunks.  The inputs repeat the 260-sample call's columns: tile by tile the bits must be that
    call's."""
    case = m3.by_name(name)
    spec, model = _spec(case), _model_cached(case, device)
    src = m3.make_sources(case, 260)
    small, variant = _run(model, spec, src, device, name=name)
    n_cu = _n_cu(device)
    for extra in (4, 5):
        cols = np.concatenate([np.tile(np.arange(128), n_cu), np.arange(128, 128 + extra)])
        big, v_big = _run(model, spec, {k: v[cols] for k, v in src.items()}, device, name=name)
        assert v_big == (variant if extra == 4 else variant.replace(",true>", ",false>"))
        for k in small:
            assert _same_bits(big[k][:128], small[k][:128]), (name, k, extra, "tile 0")
            assert _same_bits(big[k][128 * (n_cu - 1):128 * n_cu], small[k][:128]), (name, k, extra, "last full tile")
            assert _same_bits(big[k][128 * n_cu:], small[k][128:128 + extra]), (name, k, extra, "partial tile behind a full one")
            assert _same_bits(big[k][:128 * n_cu].reshape(n_cu, 128, -1), small[k][:128].expand(n_cu, -1, -1)), (name, k, extra, "every tile")


# =====================================================================================================================
# c. determinism
# =====================================================================================================================
@pytest.mark.parametrize("name", ["t13r-F385", "t13-F385", "hout-mfma-res"])
def test_the_same_call_three_times(device, name):
    """A 13-tile residual case, a ``layer1=builtin`` case and a hidden output beside an output layer on the 16-byte path:
    identical bits from three calls of ``128 n_cu + 132`` samples (every workgroup takes a second tile, so every chunk
    wait of the tile loop, its wrap included, is passed with the stream behind it in flight)."""
    case = m3.by_name(name)
    spec, model = _spec(case), _model_cached(case, device)
    n = 128 * _n_cu(device) + 132
    src = m3.make_sources(case, n)
    want = {"t13r-F385": "mlp3_kernel<13,true,true>", "t13-F385": "mlp3_kernel<13,false,true>", "hout-mfma-res": "mlp3_kernel<3,true,true>"}[name]
    first, variant = _run(model, spec, src, device, name=name)
    assert m3.row(variant) == want and ("layer1=builtin" in variant) == (name != "t13r-F385")
    for again in range(2):
        other, v = _run(model, spec, src, device, name=name)
        assert v == variant
        for k in first:
            assert _same_bits(other[k], first[k]), (name, k, again)


# =====================================================================================================================
# d. nothing outside the inputs is read (stores outside the outputs: checked by _run after every call of this module)
# =====================================================================================================================
@pytest.mark.parametrize("n", [260, 259, 131, 132])
@pytest.mark.parametrize("name", ["t1-F5", "t1r-F32", "t13r-F385"])
def test_nothing_outside_the_inputs_is_read(device, name, n):
    """A clean call (0.5 around the sources, drawn values in the features nobody reads) and the same call with NaN in the
    stride padding columns, in the guards, in the unread features between and behind the ranges of a shared source and
    in the rows behind an input with fewer than 16 features left for its last k-step (``t1-F5``: a log k-step with 1
    real row and plain ones with 7, 3 and 1; ``t1r-F32``: 15 rows at the end of the array) give identical bits, for n
    ending inside a tile (260, 132), inside a quad (259, 131) and in both epilogues."""
    case = m3.by_name(name)
    spec, model = _spec(case), _model_cached(case, device)
    g = m3.geometry3(spec)
    assert min(g["ks_rows"]) < 16
    if name == "t1-F5":
        assert g["ks_rows"][:g["n_log_ks"]] == [16, 1] and sorted(g["ks_rows"][g["n_log_ks"]:]) == [1, 3, 7]
        assert _unread_features(spec, "s", 32) == [0, 1, 2, 10, 11]
    src = m3.make_sources(case, n)
    clean, variant = _run(model, spec, src, device, poison=False, name=name)
    dirty, v = _run(model, spec, src, device, poison=True, name=name)
    assert v == variant and m3.row(variant).endswith(",true>" if n % 4 == 0 else ",false>")
    for k in clean:
        assert not torch.isnan(dirty[k]).any(), (name, k)
        assert _same_bits(dirty[k], clean[k]), (name, k, n)


# =====================================================================================================================
# e. the arithmetic keeps all six products in every layer type
# =====================================================================================================================
@pytest.mark.parametrize("n", [132, 131])
@pytest.mark.parametrize("kind", m3.TRACER_KINDS)
def test_tracer_products_keep_all_six_terms(device, kind, n):
    """Tracer models (mlp3_cases.tracer): every weight matrix is a scaled permutation of positive float32 numbers with full
    24-bit mantissas, so are the inputs; std = 1, centre = 0, every bias 0.  Each output is then ONE chain of products,
    which the float64 oracle evaluates exactly, and the kernel's error per split layer is bounded by (derivation at
    ``mlp3_cases.E_SPLIT``):

      * the three bf16 pieces of an operand are exact (3 x 8 = 24 mantissa bits): nothing;
      * the three dropped cross products: mid*lo, lo*mid <= 2^-24 |w x| each (|mid| <= 2^-8, |lo| <= 2^-16 of the operand;
        the file's header quotes 2^-25, the typical size -- the bound takes the worst case), lo*lo <= 2^-32 |w x|;
      * one float32 rounding per accumulation of the six kept products, smallest first: four on partial sums below
        2^-6 |w x| (2^-30 |w x| each), one on the result (2^-24 |w x|);

    together 3.07 x 2^-24 relative per split layer; the vector-ALU output layer is one FMA per product, 2^-24.  Along a
    chain the factors (1 + e) multiply.  tests/test_host_mlp3_edges.py shows on the CPU emulation of this product that the
    bound passes with six terms and fails with any five in any layer type; it is not tuned on the kernel's output.
    Measured on an MI355X (worst |error| / bound over all outputs, printed; <= 1 passes): layer1 0.731, hidden 0.526,
    mfma-out 0.719, valu-out 0.725, the same in both epilogues.  A library whose host packing drops the lowest piece of
    every weight fails all eight cases."""
    from fv3net_amd.mlp import MlpModelSplitBf16

    tr = m3.tracer(kind, n)
    truth = mlp_np.forward(tr.spec, tr.sources, dtype=np.float64)
    model = MlpModelSplitBf16(tr.spec, device=device)
    got, variant = _run(model, tr.spec, tr.sources, device, name=f"tracer-{kind}")
    assert m3.row(variant).endswith(",true>" if n % 4 == 0 else ",false>")
    assert ("out=mfma" in variant) == (kind == "mfma-out") and "hout=1" in variant
    worst = m3.tracer_excess(tr, _np(got), truth)
    print(f"tracer {kind} n={n} {variant}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0, (kind, n, worst)


# =====================================================================================================================
# f. non-finite inputs stay in their sample
# =====================================================================================================================
@pytest.mark.parametrize("n", [164, 163])
@pytest.mark.parametrize("case", m3.poison_cases(), ids=lambda c: c.name)
def test_non_finite_inputs_stay_in_their_sample(device, case, n):
    """A clean call, then the same call with NaN, +inf, -inf in a plain feature and NaN, +inf, -inf, 0, a negative value,
    a value below, at and just above eps in a log feature (mlp3_cases.poisons), on the matrix-core output layer with and
    without a residual, the vector-ALU output layer and a hidden output alone, in both epilogues (164 / 163 samples):

      * every unpoisoned sample keeps the clean call's bits in every output, residual and hidden output;
      * a NaN-poisoned sample is NaN wherever the float64 oracle is (everywhere: the log floor ``x < eps ? eps : x`` and
        the ReLU ``v < 0 ? 0 : v`` keep a NaN, as numpy's ``maximum`` does);
      * a +-inf-poisoned sample is not finite wherever the oracle is not finite;
      * samples whose log input is 0, negative, -inf or below eps take the floor, those at and above eps do not: all of
        them pass the ordinary gate against the oracle."""
    spec, model = _spec(case), _model_cached(case, device)
    clean_src, bad_src, classes = m3.poisoned_sources(case, n)
    clean, variant = _run(model, spec, clean_src, device, name=case.name)
    bad, v_bad = _run(model, spec, bad_src, device, name=case.name)
    assert v_bad == variant and m3.row(variant).endswith(",true>" if n % 4 == 0 else ",false>")
    clean, bad = _np(clean), _np(bad)
    with np.errstate(invalid="ignore", over="ignore"):
        o64 = mlp_np.forward(spec, bad_src, dtype=np.float64)
        o32 = mlp_np.forward(spec, bad_src, dtype=np.float32)
    nan_s = np.array([s for s, c in classes.items() if c == "nan"])
    inf_s = np.array([s for s, c in classes.items() if c == "inf"])
    untouched = np.array([s for s in range(n) if s not in classes])
    finite_rows = np.array(sorted(s for s in range(n) if classes.get(s) not in ("nan", "inf")))
    assert set(bad) == set(o64)
    for k in bad:
        g = bad[k]
        assert np.array_equal(g[untouched].view(np.int32), clean[k][untouched].view(np.int32)), (case.name, k, "an unpoisoned sample changed")
        assert np.isnan(o64[k][nan_s]).all() and np.isnan(g[nan_s]).all(), (case.name, k, "a NaN-poisoned sample is not NaN everywhere")
        assert not np.isfinite(g[inf_s][~np.isfinite(o64[k][inf_s])]).any(), (case.name, k, "finite where the oracle is not")
        assert (~np.isfinite(o64[k][inf_s])).any(), (case.name, k)
        assert np.isfinite(g[finite_rows]).all()
        assert_close_per_level(g[finite_rows], o64[k][finite_rows], o32[k][finite_rows], f"{case.name} {k} (floored log inputs)", slack32=2e-7)


# =====================================================================================================================
# g. smallest calls
# =====================================================================================================================
def test_zero_samples_launch_nothing(device):
    from fv3net_amd.mlp import MlpModelSplitBf16

    case = m3.by_name("t1r-F32")
    spec = _spec(case)
    model = MlpModelSplitBf16(spec, device=device)   # (a fresh handle: nothing launched yet)
    assert model.last_variant == ""
    src = {k: torch.empty((v.shape[1], 0), device=device) for k, v in _clean(case)[0].items()}
    out = model.predict(src)
    assert model.last_variant == "" and all(v.shape[1] == 0 for v in out.values())


@pytest.mark.parametrize("name", ["t1-F5", "t13r-F385"])
def test_smallest_calls(device, name):
    """n = 1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 132 on a model that can take the 16-byte epilogue and on a residual
    model: the asserted variant flips with ``n % 4``, and every column has the bits it has in the 260-sample call (section
    b: neither the call nor the epilogue changes a column).  Outputs are passed through ``out=`` in every call of this
    module; the last call here lets the wrapper allocate them and passes a one-feature source as a transposed view."""
    case = m3.by_name(name)
    spec, model = _spec(case), _model_cached(case, device)
    src = m3.make_sources(case, 260)
    full, variant = _run(model, spec, src, device, name=name)
    for n in (1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 132):
        got, v = _run(model, spec, {k: a[:n] for k, a in src.items()}, device, name=name)
        assert v == (variant if n % 4 == 0 else variant.replace(",true>", ",false>")), (name, n, v)
        for k in full:
            assert got[k].shape[0] == n and _same_bits(got[k], full[k][:n]), (name, k, n)
    # (the one-feature source "ps" arrives as the transpose of an [n, 1] array: its only row reports a feature stride of 1,
    # which the wrapper must not hand to the library as a stride below n)
    dev_src = {k: torch.from_numpy(a[:132].copy()).to(device).T for k, a in src.items()}
    assert tuple(dev_src["ps"].shape) == (1, 132) and dev_src["ps"].stride(0) == 1
    dev_src = {k: v if v.shape[0] == 1 else v.contiguous() for k, v in dev_src.items()}
    alloc = model.predict(dev_src)
    assert model.last_variant == variant
    for k in full:
        assert _same_bits(alloc[k].T, full[k][:132]), (name, k, "outputs allocated by the wrapper")


def test_recurrent_state_pair_next_to_each_other(device):
    """The recurrent emulators (local_mlp.py) never hand the hidden output back into a source of the same call: the state
    ping-pongs between the two halves of one allocation -- the cell reads half ``cur`` as a source and writes half
    ``cur ^ 1`` as its hidden output.  Exactly that arrangement: two steps, each against the oracle's step, and the half
    that is read is left as it was.  (No aliasing of a source and an output is promised or tested.)"""
    from fv3net_amd.mlp import InputSpec, MlpModelSplitBf16, MlpSpec

    rng = np.random.default_rng(7)
    n, width, nin = 260, 256, 5
    kern = (rng.normal(0, 1, (nin + width, width)) / np.sqrt(nin + width)).astype(np.float32)
    spec = MlpSpec(inputs=[InputSpec("in", nin), InputSpec("rec", width)], hidden_kernels=[kern],
                   hidden_biases=[rng.uniform(0.05, 0.2, width).astype(np.float32)], outputs=[], out_kernel=np.zeros((width, 0), np.float32),
                   out_bias=np.zeros(0, np.float32), hidden_output="h")
    model = MlpModelSplitBf16(spec, device=device)
    states = torch.zeros((2, width, n), device=device)
    x = rng.normal(0, 1, (2, n, nin)).astype(np.float32)
    state_np = np.zeros((n, width), np.float32)
    for step in range(2):
        cur = step & 1
        kept = states[cur].clone()
        model.predict({"in": torch.from_numpy(np.ascontiguousarray(x[step].T)).to(device), "rec": states[cur]}, out={"h": states[cur ^ 1]})
        assert model.last_variant == m3.expected_variant3(spec, n)
        assert torch.equal(states[cur], kept)
        truth = mlp_np.forward(spec, {"in": x[step], "rec": state_np}, dtype=np.float64)["h"]
        cpu32 = mlp_np.forward(spec, {"in": x[step], "rec": state_np}, dtype=np.float32)["h"]
        state_np = states[cur ^ 1].cpu().numpy().T.copy()
        assert_close_per_level(state_np, truth, cpu32, f"state after step {step}", slack32=2e-7)


# =====================================================================================================================
# h. refusals on the device
# =====================================================================================================================
def test_create_refuses_what_the_restated_dispatch_refuses(device):
    from fv3net_amd._lib import Fv3HipError
    from fv3net_amd.mlp import MlpModelSplitBf16

    for kind, specs in m3.REFUSALS.items():
        for kw in specs:
            with pytest.raises(Fv3HipError, match=m3.REFUSAL_MESSAGES[kind]):
                MlpModelSplitBf16(m3.refusal_spec(**kw), device=device)
    for kw in m3.ACCEPTED:
        MlpModelSplitBf16(m3.refusal_spec(**kw), device=device)


def test_predict_refuses_rows_shorter_than_the_call(device):
    """``feature stride < n_samples`` for a source and for the hidden output (rows that overlap): refused before the
    launch."""
    from fv3net_amd._lib import Fv3HipError

    case = m3.by_name("cell-G2")
    spec, model = _spec(case), _model_cached(case, device)
    n = 64
    good = {k: torch.zeros((v.shape[1], n), device=device) for k, v in _clean(case)[0].items()}
    model.predict(good)
    before = model.last_variant
    flat = torch.zeros(16 * n, device=device)
    with pytest.raises(Fv3HipError, match=r"source 0: feature stride 63 < n_samples"):
        model.predict({**good, "a": torch.as_strided(flat, (16, n), (n - 1, 1))})
    hflat = torch.zeros(256 * n, device=device)
    with pytest.raises(Fv3HipError, match=r"hidden output: feature stride 63 < n_samples"):
        model.predict(good, out={"h": torch.as_strided(hflat, (256, n), (n - 1, 1))})
    assert model.last_variant == before and not hflat.any()


def test_model_of_one_device_refuses_a_call_on_another(device):
    from fv3net_amd import _lib

    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible")
    other = torch.device("cuda", (torch.device(device).index or 0) ^ 1)
    case = m3.by_name("cell-G2")
    model = _model_cached(case, device)
    src = {k: torch.zeros((v.shape[1], 64), device=other) for k, v in _clean(case)[0].items()}
    with pytest.raises((_lib.Fv3HipError, ValueError, RuntimeError), match="device"):
        model.predict(src)
