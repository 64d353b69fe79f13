"""The split-bf16 MLP kernel (csrc/mlp_bf16x3.hip): its dispatch restated in plain Python from the model description alone,
a catalogue of edge cases, the tracer models of the arithmetic test and a numpy emulation of the kernel's product.

``expected_variant3`` predicts the string ``fv3hip_mlp3_last_variant`` reports for a call; ``CATALOGUE`` holds small models
(width 256 is fixed; inputs and outputs as small as the edge allows, at most 700 samples) that together select all 16 rows
of ``kMlp3Table`` and every run-time path inside them.  tests/test_host_mlp3_edges.py proves that without a GPU;
tests/test_gpu_mlp3_edges.py runs every entry and asserts the prediction on every call.

A case is a model and a call (``mlp_cases.Case``: the model builder, the sources and the conditioning rules are shared
with the fp32 kernels' catalogue) plus how the call's arrays are laid out (``Case3.misalign``): every condition of the
16-byte epilogue's rule is broken by one case on its own.
"""
import dataclasses
from typing import Optional

import numpy as np

import mlp_cases as mc
from mlp_cases import FLT_MIN, VariantRefused

LDS_MAX = 160 * 1024
K_HT = 8            # hidden feature tiles (width 256)
MAX_KS1 = 64        # kMaxKs1
TILES = (1, 3, 5, 13)
PATCH_BYTES = 4 * 32 * 36 * 4   # a transposition patch per wave (rows of 36 floats)
SMALL_TABLE_BYTES = 8 * 4 * 2 * 16 * 4 + 16


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch of fv3hip_mlp3_create / fv3hip_mlp3_predict, restated
# ---------------------------------------------------------------------------------------------------------------------
def geometry3(spec):
    """What ``fv3hip_mlp3_create`` derives from a model, or ``VariantRefused`` with the library's message."""
    nh, F = len(spec.hidden_kernels), spec.n_out_features
    if spec.width != 256 or nh < 1 or spec.activation != "relu":
        raise VariantRefused("ReLU networks of hidden width 256")
    if any(o.min is not None or o.max is not None or o.mask is not None for o in spec.outputs):
        raise VariantRefused("does not implement output limits / masks")
    n_res = len(spec.residuals)
    small_out = F if (1 <= F <= 4 and n_res == 0) else 0
    has_out = 1 if (F > 0 and not small_out) else 0
    n_ot = (F + 31) // 32 if has_out else 1
    if n_ot not in TILES:
        raise VariantRefused("compiled for 1, 3, 5 or 13 output tiles of 32")
    # k-slots of layer 1: the log inputs first, every input padded to whole k-steps of 16; (input, feature) or None
    slots, ks_rows, ks_input, n_log_slots = [], [], [], 0
    for want_log in (True, False):
        for idx, i in enumerate(spec.inputs):
            is_log = i.transform == "log"
            if is_log and not (np.float32(i.eps) >= np.float32(FLT_MIN)):
                raise VariantRefused("needs log epsilons >= FLT_MIN")
            if is_log != want_log:
                continue
            slots += [(idx, f) for f in range(i.nfeat)]
            slots += [None] * (-len(slots) % 16)
            for f0 in range(0, i.nfeat, 16):
                ks_rows.append(min(16, i.nfeat - f0))
                ks_input.append((idx, f0))
        if want_log:
            n_log_slots = len(slots)
    n_ks1 = len(slots) // 16
    if n_ks1 > MAX_KS1:
        raise VariantRefused(f"at most {MAX_KS1} layer-1 k-steps")
    ch_h, ch_o = 3 * K_HT * 64, (3 * n_ot * 64 + 255) // 256 * 256   # float4 per hidden-type / output-type chunk
    n_hid_chunks = n_ks1 + 16 * (nh - 1)
    G = n_hid_chunks + (16 if has_out else 0)
    if G < 2:
        raise VariantRefused("at least two k-steps per tile")
    lds_bytes = 3 * max(ch_h, ch_o) * 16 + (nh * K_HT + n_ot) * 128 + len(slots) * 8 + n_ot * 32 * 24
    lds_fast = lds_bytes + PATCH_BYTES + n_ot * 128
    if small_out:
        lds_bytes += SMALL_TABLE_BYTES
        lds_fast += SMALL_TABLE_BYTES
    if lds_bytes > LDS_MAX:
        raise VariantRefused("bytes of LDS (> 160 KiB)")
    return dict(F=F, n_hidden=nh, small_out=small_out, has_out=has_out, n_ot=n_ot, n_res=n_res, hout=bool(spec.hidden_output),
                slots=slots, ks_rows=ks_rows, ks_input=ks_input, n_ks1=n_ks1, n_log_ks=n_log_slots // 16, G=G,
                lds_bytes=lds_bytes, lds_fast=lds_fast, padding_features=(n_ot * 32 - F) if has_out else 0)


@dataclasses.dataclass(frozen=True)
class Layout:
    """What ``fv3hip_mlp3_predict`` sees of a call's arrays, one flag per clause of its rule for the 16-byte epilogue:
    every output and residual output has a 16-byte aligned base and a feature stride that is a multiple of 4 floats; so
    has every residual *source*; so has the hidden output.  ``xwrap``: 16 feature rows of a source span 4 GiB or more."""
    outputs_ok: bool = True
    res_sources_ok: bool = True
    hout_ok: bool = True
    xwrap: bool = False


def fast_conditions(spec, n, layout: Layout):
    """The rule of ``fv3hip_mlp3_predict`` for the 16-byte epilogue, clause by clause (all must hold)."""
    g = geometry3(spec)
    return {"whole quads (n % 4 == 0)": n % 4 == 0,
            "LDS of the 16-byte layout <= 160 KiB": g["lds_fast"] <= LDS_MAX,
            "outputs aligned": layout.outputs_ok,
            "residual sources aligned": layout.res_sources_ok or not g["n_res"],
            "hidden output aligned": layout.hout_ok or not g["hout"]}


def expected_variant3(spec, n, layout: Layout = Layout()) -> str:
    """The string ``MlpModelSplitBf16.last_variant`` holds after a ``predict`` of ``n > 0`` samples."""
    g = geometry3(spec)
    fast = all(fast_conditions(spec, n, layout).values())
    out = "mfma" if g["has_out"] else (f"valu{g['small_out']}" if g["small_out"] else "none")
    layer1 = "block" if (g["n_hidden"] >= 2 or not g["has_out"]) else "builtin"
    return (f"mlp3_kernel<{g['n_ot']},{mc._flag(g['n_res'] != 0)},{mc._flag(fast)}> out={out} hout={int(g['hout'])} layer1={layer1}"
            f" ks1={g['n_ks1']}/{g['n_log_ks']} hidden={g['n_hidden']} xwrap={int(layout.xwrap)}")


ALL_ROWS = sorted(f"mlp3_kernel<{ot},{mc._flag(res)},{mc._flag(fast)}>" for ot in TILES for res in (False, True) for fast in (False, True))


def row(variant: str) -> str:
    return variant.split(" ")[0]


def facts(variant: str) -> dict:
    """The ``key=value`` facts behind the row of a variant string."""
    return dict(kv.split("=") for kv in variant.split(" ")[1:])


def smallest_refused_depth(n_ot=13, n_ks1=MAX_KS1):
    """The smallest number of hidden layers at which the tables of a model with ``n_ot`` output tiles and ``n_ks1`` layer-1
    k-steps exceed 160 KiB of LDS, from the formula: every hidden layer adds its 8 bias rows of 128 bytes."""
    ch = max(3 * K_HT * 64, (3 * n_ot * 64 + 255) // 256 * 256)
    fixed = 3 * ch * 16 + n_ot * 128 + n_ks1 * 16 * 8 + n_ot * 32 * 24
    return (LDS_MAX - fixed) // (K_HT * 128) + 1


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
MISALIGN = ("", "out_ptr", "out_stride", "res_src", "hout")


@dataclasses.dataclass(frozen=True)
class Case3:
    """A model and its call (``base``) and the one array of the call that is laid out off the 16-byte rule:
    "out_ptr": the first output starts one float past a 16-byte boundary; "out_stride": the last output (residual outputs
    included) has a feature stride that is 1 mod 4; "res_src": the first residual's source starts one float off while every
    output is aligned; "hout": the hidden output starts one float off."""
    base: mc.Case
    misalign: str = ""

    @property
    def name(self):
        return self.base.name + (f"+{self.misalign}" if self.misalign else "")

    @property
    def n(self):
        return self.base.n

    @property
    def layout(self) -> Layout:
        return Layout(outputs_ok=self.misalign not in ("out_ptr", "out_stride"), res_sources_ok=self.misalign != "res_src",
                      hout_ok=self.misalign != "hout")


def build_spec(case: Case3):
    return mc.build_spec(case.base)


def make_sources(case: Case3, n: Optional[int] = None):
    return mc.make_sources(case.base, n)


def variant_of(case: Case3, n: Optional[int] = None) -> str:
    return expected_variant3(build_spec(case), case.n if n is None else n, case.layout)


def _c3(name, n_hidden, inputs, outputs, n, misalign="", **kw):
    return Case3(mc._c("mlp3-" + name, 256, n_hidden, inputs, outputs, n, **kw), misalign)


def OUT(*heads):
    return tuple((name, nf, None, None, 0) for name, nf in heads)


def Y(F):
    return OUT(("y", F))


RES_Y = (("y_after", "before", "y"),)
EPS = 1e-8
# input sets.  A shared source "s" read through ranges that start past 0 and leave features nobody reads between them
# (10..11) and after them (32..): the plain range 3..9, the log range 12..28, the plain range 29..31 -- the log input is
# listed after a plain one and the host moves it to the front; 7 + 17 + 3 + 1 features in 1 + 2 + 1 + 1 k-steps.
IN_SHARED = (("a", "s", 7, 3, None), ("lg", "s", 17, 12, EPS), ("b", "s", 3, 29, None), ("ps", "ps", 1, 0, None))
IN_1 = (("a", "a", 1, 0, None),)                                   # one k-step with one real row
IN_15, IN_16, IN_17 = ((("a", "a", k, 0, None),) for k in (15, 16, 17))
IN_2KS = (("a", "a", 16, 0, None), ("b", "b", 5, 0, None))         # 2 k-steps, no log
IN_3KS_LOG = (("l1", "q", 20, 0, FLT_MIN), ("l2", "r", 9, 0, EPS))  # 3 k-steps, all log, eps exactly FLT_MIN and 1e-8
IN_4KS = (("p", "s", 16, 2, None), ("lg", "q", 30, 1, EPS), ("z", "z", 2, 0, None))   # 4 k-steps, log listed second
IN_64KS = (("a", "a", 1008, 0, None), ("b", "b", 1, 0, None))      # 63 + 1 = 64 k-steps (1 024 padded inputs)


def _catalogue():
    c = []
    # ---- one output tile, no residual: F = 5 and 32 (valu for F <= 4 below); both epilogues
    c.append(_c3("t1-F5", 2, IN_SHARED, Y(5), 260))
    c.append(_c3("t1-F32", 1, IN_2KS, Y(32), 132))                                 # layer1=builtin, 2 k-steps
    c.append(_c3("t1-F5-n%4", 1, IN_3KS_LOG, Y(5), 131))                           # builtin with an odd n_ks1 (tail step), all log
    c.append(_c3("t1-F32-outptr", 2, IN_1, Y(32), 132, "out_ptr"))
    # ---- one output tile with a residual: F = 1 and 32
    c.append(_c3("t1r-F1", 2, IN_17, Y(1), 260, residuals=RES_Y))
    c.append(_c3("t1r-F32", 1, IN_15, Y(32), 132, residuals=RES_Y))
    c.append(_c3("t1r-F1-ressrc", 1, IN_16, Y(1), 132, "res_src", residuals=RES_Y))
    c.append(_c3("t1r-F32-n%4", 3, IN_SHARED, Y(32), 130, residuals=RES_Y))
    # ---- three tiles: 65 and 96
    c.append(_c3("t3-F65", 1, IN_4KS, OUT(("a", 33), ("y", 32)), 260))
    c.append(_c3("t3-F96-stride", 2, IN_16, Y(96), 132, "out_stride"))
    c.append(_c3("t3r-F65", 2, IN_15, OUT(("a", 3), ("y", 62)), 260, residuals=RES_Y))
    c.append(_c3("t3r-F96-n%4", 1, IN_SHARED, Y(96), 133, residuals=RES_Y))
    c.append(_c3("t3r-F96", 1, IN_2KS, Y(96), 132, residuals=RES_Y))
    c.append(_c3("t3-F65-n%4", 2, IN_17, Y(65), 129))
    # ---- five tiles: 129 and 160
    c.append(_c3("t5-F129", 2, IN_3KS_LOG, Y(129), 260))
    c.append(_c3("t5-F160-n%4", 1, IN_16, Y(160), 135))
    c.append(_c3("t5r-F160", 1, IN_4KS, OUT(("a", 30), ("y", 130)), 260, residuals=RES_Y))   # residual rows 30..159: tiles 0..4
    c.append(_c3("t5r-F129-stride", 2, IN_16, Y(129), 132, "out_stride", residuals=RES_Y))
    # ---- thirteen tiles: 385 and 416; the residual output starts in tile 1 and spans 7 tiles, so the five-tile window
    # of `before` rows rolls twice and its first rows are dummies
    OUT13 = OUT(("a", 40), ("y", 200), ("z", 145))
    c.append(_c3("t13r-F385", 2, IN_SHARED, OUT13, 260, residuals=RES_Y))
    c.append(_c3("t13r-F416-ressrc", 1, IN_17, OUT(("a", 70), ("y", 346)), 132, "res_src", residuals=RES_Y))  # tiles 2..12
    c.append(_c3("t13-F385", 1, IN_16, Y(385), 132))
    c.append(_c3("t13-F416-n%4", 2, IN_2KS, Y(416), 134))
    # ---- the small output layer on the vector ALU: 1, 2, 3 (two heads of 1 + 2), 4 outputs; with a hidden output
    c.append(_c3("valu1", 2, IN_15, Y(1), 260))
    c.append(_c3("valu2-n%4", 1, IN_4KS, Y(2), 131))
    c.append(_c3("valu3-two-heads", 1, IN_SHARED, OUT(("p", 1), ("q", 2)), 132))
    c.append(_c3("valu4-hout", 2, IN_17, Y(4), 260, hidden_output=True))
    c.append(_c3("valu3-hout-misaligned", 1, IN_17, Y(3), 132, "hout", hidden_output=True))
    # ---- no output layer at all (a recurrent cell): both epilogues; the smallest legal stream (2 k-steps, G = 2)
    c.append(_c3("cell-G2", 1, IN_2KS, (), 260, hidden_output=True))
    c.append(_c3("cell-n%4", 1, IN_3KS_LOG, (), 131, hidden_output=True))
    c.append(_c3("cell-deep", 3, IN_17, (), 132, hidden_output=True))
    # ---- a hidden output beside an output layer on the matrix cores: both epilogues, with and without residuals
    c.append(_c3("hout-mfma", 2, IN_SHARED, Y(90), 260, hidden_output=True))
    c.append(_c3("hout-mfma-res", 1, IN_4KS, Y(70), 132, residuals=RES_Y, hidden_output=True))
    c.append(_c3("hout-mfma-res-n%4", 2, IN_16, Y(30), 129, residuals=RES_Y, hidden_output=True))
    c.append(_c3("hout-mfma-misaligned", 1, IN_15, Y(20), 132, "hout", hidden_output=True))
    # ---- 64 layer-1 k-steps; with 13 tiles and one hidden layer the 16-byte layout takes exactly 160 KiB, with two
    # hidden layers the LDS budget forces the 4-byte epilogue on an aligned call
    c.append(_c3("ks64-t1", 1, IN_64KS, Y(7), 132))
    c.append(_c3("ks64-t13-exactly-160KiB", 1, IN_64KS, Y(385), 132))
    c.append(_c3("ks64-t13-lds-forced", 2, IN_64KS, Y(385), 132, residuals=RES_Y))
    return c


CATALOGUE = _catalogue()


def by_name(name) -> Case3:
    return next(c for c in CATALOGUE if c.base.name == "mlp3-" + name)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: what fv3hip_mlp3_create turns down (the message it gives) and the nearest models it accepts
# ---------------------------------------------------------------------------------------------------------------------
def refusal_spec(F, n_in=(16,), n_hidden=1, residual=False, eps=None, width=256, activation="relu", lo=None, mask=False, hout=False):
    starts = np.concatenate([[0], np.cumsum(n_in)]).tolist()   # consecutive ranges of one source
    inputs = tuple((f"i{k}", "s", nf, starts[k], eps) for k, nf in enumerate(n_in))
    outs = ((("y", F, lo, None, 1 if mask else 0),) if F else ())
    case = mc._c("refusal", width, n_hidden, inputs, outs, 8, residuals=RES_Y if residual else (), activation=activation,
                 hidden_output=hout)
    return mc.build_spec(case)


REFUSALS = {
    "tiles": [dict(F=F) for F in (33, 64, 97, 128, 161, 384, 417)] + [dict(F=33, residual=True), dict(F=161, residual=True)],
    "k-steps": [dict(F=5, n_in=(16,) * 65), dict(F=5, n_in=(1025,))],
    "eps": [dict(F=5, eps=float(np.nextafter(np.float32(FLT_MIN), np.float32(0)))), dict(F=5, eps=0.0)],
    "width": [dict(F=5, width=64), dict(F=5, activation="linear")],
    "limits": [dict(F=5, lo=0.0), dict(F=5, mask=True)],
    "stream": [dict(F=0, hout=True), dict(F=3)],   # one k-step in all: no output layer on the matrix cores, one hidden layer
    "lds": [dict(F=385, n_in=(1024,), n_hidden=smallest_refused_depth())],
}
REFUSAL_MESSAGES = {"tiles": "1, 3, 5 or 13 output tiles", "k-steps": "at most 64 layer-1 k-steps", "eps": "log epsilons >= FLT_MIN",
                    "width": "ReLU networks of hidden width 256", "limits": "output limits / masks",
                    "stream": "at least two k-steps per tile", "lds": r"bytes of LDS \(> 160 KiB\)"}
ACCEPTED = [dict(F=F) for F in (32, 65, 96, 129, 160, 385, 416)] + [
    dict(F=5, n_in=(16,) * 64), dict(F=5, n_in=(1024,)), dict(F=5, eps=FLT_MIN), dict(F=0, hout=True, n_in=(17,)),
    dict(F=3, n_hidden=2), dict(F=385, n_in=(1024,), n_hidden=smallest_refused_depth() - 1)]


# ---------------------------------------------------------------------------------------------------------------------
# non-finite inputs (test_gpu_mlp3_edges.py, section f): one case per output path, residual or not; each runs in both
# epilogues (n and n - 1 samples)
# ---------------------------------------------------------------------------------------------------------------------
IN_POISON = (("x", "x", 12, 0, None), ("lg", "q", 9, 0, EPS))


def poison_cases():
    kw = dict(inf_path=("x", 5))
    return [_c3("poison-mfma", 2, IN_POISON, Y(20), 164, **kw),
            _c3("poison-mfma-res", 2, IN_POISON, Y(20), 164, residuals=RES_Y, **kw),
            _c3("poison-valu", 2, IN_POISON, Y(4), 164, **kw),
            _c3("poison-none-hout", 2, IN_POISON, (), 164, hidden_output=True, **kw)]


def poisons(n):
    """[(sample, source, feature, value, class)] -- "nan", "inf" (a +-inf that reaches the network), "floor" (a log input
    the floor replaces: 0, a negative value, -inf, a value below eps), "plain" (a log input exactly at and just above
    eps: nothing special may happen).  At the first and last lanes of waves, at the tile boundary and at the end."""
    return [(0, "x", 3, np.nan, "nan"), (32, "x", 5, np.inf, "inf"), (63, "x", 7, -np.inf, "inf"), (n - 1, "x", 5, np.inf, "inf"),
            (31, "q", 2, np.nan, "nan"), (127, "q", 4, np.inf, "inf"), (128, "q", 1, -np.inf, "floor"), (n - 4, "q", 0, 0.0, "floor"),
            (64, "q", 8, -3.5, "floor"), (65, "q", 3, 1e-9, "floor"), (66, "q", 3, float(np.float32(EPS)), "plain"),
            (67, "q", 3, float(np.nextafter(np.float32(EPS), np.float32(1))), "plain")]


def poisoned_sources(case: Case3, n=None):
    """(clean sources, poisoned sources, {sample: class}) of the first ``n`` samples."""
    n = case.n if n is None else n
    clean = make_sources(case, n)
    bad = {k: v.copy() for k, v in clean.items()}
    classes = {}
    for sample, src, feat, value, cls in poisons(n):
        bad[src][sample, feat] = value
        assert sample not in classes
        classes[sample] = cls
    return clean, bad, classes


# ---------------------------------------------------------------------------------------------------------------------
# the tracer models of the arithmetic test (section e) and the emulation of the kernel's product
# ---------------------------------------------------------------------------------------------------------------------
# A split layer: the six kept products are exact in float32 (8 x 8 mantissa bits) and are accumulated smallest first,
# mid*mid, hi*lo, lo*hi, hi*mid, mid*hi, hi*hi (w piece x x piece).  With |w - hi| <= 2^-8 |w| and |w - hi - mid| <= 2^-16 |w|
# (round to nearest, 8 bits a piece; the file's header quotes the typical 2^-25 for the dropped terms, the worst case of a
# mantissa just above a power of two is twice that):
#   * the pieces are exact (24 mantissa bits in three pieces of 8);
#   * the three dropped products: mid*lo, lo*mid <= 2^-24 |w x| each, lo*lo <= 2^-32 |w x|;
#   * the first four accumulations round sums that stay below 2^-6 |w x|: <= 2^-24 x 2^-6 |w x| each;
#   * the last accumulation (+ hi*hi) rounds the result once: <= 2^-24 |w x|.
# Sum: (2 + 2^-8 + 2^-4 + 1) 2^-24 < 3.07 x 2^-24 relative, per split layer.  The vector-ALU output layer is one fp32 FMA
# per product (one rounding, 2^-24); adding the zeros of the other features and a zero bias is exact.
E_SPLIT = 3.07 * 2.0 ** -24
E_VALU = 2.0 ** -24
TERMS = ("mid*mid", "hi*lo", "lo*hi", "hi*mid", "mid*hi", "hi*hi")   # the kernel's accumulation order
LAYER_TYPES = ("layer1", "hidden", "output")


@dataclasses.dataclass
class Tracer:
    name: str
    spec: object
    sources: dict     # name -> [sample, feature] float32
    bounds: dict      # output name -> relative bound per output value (the chain's layers summed, compounded)
    layer_types: tuple  # the split layer types this model's outputs pass through


def _mantissas(rng, shape):
    """Positive float32 numbers in [1, 2) with full 24-bit mantissas (the last bit set, so that all three pieces matter)."""
    m = rng.integers(0, 1 << 22, shape, dtype=np.int64) * 2 + 1
    return (1.0 + m / float(1 << 23)).astype(np.float32)


def _scaled_permutation(rng, rows, cols):
    """[rows, cols] with one non-zero per column and at most one per row (rows >= cols): a scaled partial permutation."""
    w = np.zeros((rows, cols), np.float32)
    w[rng.permutation(rows)[:cols], np.arange(cols)] = _mantissas(rng, cols)
    return w


def tracer(kind: str, n=132) -> Tracer:
    """``kind``: "layer1" (layer 1 alone in front of a valu output; the hidden output shows all 256 of its products),
    "hidden" (a hidden -> hidden layer behind it), "mfma-out" (the output layer on the matrix cores, 5 tiles),
    "valu-out" (the vector-ALU output layer).  std = 1 and centre = 0 in layer 1, every bias 0, output scale 1: every
    output is one chain of products of positive numbers, which the float64 oracle evaluates exactly (2 x 24 bits per
    product; three factors need 72 bits and are exact to 2^-53, far below the bound)."""
    from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec

    rng = np.random.default_rng({"layer1": 11, "hidden": 12, "mfma-out": 13, "valu-out": 14}[kind])
    nh = 2 if kind == "hidden" else 1
    F = 160 if kind == "mfma-out" else 4
    hk = [_scaled_permutation(rng, 256, 256) for _ in range(nh)]
    spec = MlpSpec(inputs=[InputSpec("a", 256)], hidden_kernels=hk, hidden_biases=[np.zeros(256, np.float32) for _ in range(nh)],
                   outputs=[OutputSpec("y", F)], out_kernel=_scaled_permutation(rng, 256, F), out_bias=np.zeros(F, np.float32),
                   hidden_output="h")
    spec.validate()
    e_out = E_SPLIT if kind == "mfma-out" else E_VALU
    bounds = {"h": (1 + E_SPLIT) ** nh - 1, "y": (1 + E_SPLIT) ** nh * (1 + e_out) - 1}
    types = {"layer1": ("layer1",), "hidden": ("layer1", "hidden"), "mfma-out": ("layer1", "output"), "valu-out": ("layer1",)}[kind]
    return Tracer(kind, spec, {"a": _mantissas(rng, (n, 256))}, bounds, types)


TRACER_KINDS = ("layer1", "hidden", "mfma-out", "valu-out")


def bf16_pieces(x):
    """(hi, mid, lo): three round-to-nearest-even bf16 pieces of float32 ``x`` as float32 arrays; the residuals are exact."""
    def rne(a):
        b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
        b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
        return b.astype(np.uint32).view(np.float32).reshape(np.shape(a))
    x = np.asarray(x, np.float32)
    hi = rne(x)
    r1 = (x - hi).astype(np.float32)
    mid = rne(r1)
    lo = rne((r1 - mid).astype(np.float32))
    return {"hi": hi, "mid": mid, "lo": lo}


def split_dense(x, w, drop=None):
    """[sample, in] @ [in, out] as the kernel's matrix cores compute it on a tracer model: three bf16 pieces of every
    float32 operand, the six kept terms summed in float32 in the kernel's order.  A term is the float64 contraction of two
    pieces rounded to float32 -- exact where a column of ``w`` has one non-zero (the products of 8-bit pieces are exact), which
    is all this is for.  ``drop``: a term of ``TERMS`` to leave out."""
    xp, wp = bf16_pieces(x), bf16_pieces(w)
    acc = np.zeros((x.shape[0], w.shape[1]), np.float32)
    for term in TERMS:
        if term == drop:
            continue
        wn, xn = term.split("*")
        acc = (acc + (xp[xn].astype(np.float64) @ wp[wn].astype(np.float64)).astype(np.float32)).astype(np.float32)
    return acc


def emulate_tracer(tr: Tracer, drop=None):
    """The tracer model as the kernel evaluates it (float32, every bias 0), ``drop`` = (layer type, term) or None."""
    spec = tr.spec
    g = geometry3(spec)
    h = tr.sources["a"].astype(np.float32)
    for l, kern in enumerate(spec.hidden_kernels):
        kind = "layer1" if l == 0 else "hidden"
        h = np.maximum(split_dense(h, kern, drop[1] if drop and drop[0] == kind else None), np.float32(0))
    if g["has_out"]:
        y = split_dense(h, spec.out_kernel, drop[1] if drop and drop[0] == "output" else None)
    else:  # one fp32 FMA per product, the other features add exact zeros
        y = (h.astype(np.float64) @ spec.out_kernel.astype(np.float64)).astype(np.float32)
    return {"h": h, "y": y}


def tracer_excess(tr: Tracer, got, truth):
    """max over the outputs of |got - truth| / (bound x |truth|): <= 1 passes."""
    worst = 0.0
    for name, bound in tr.bounds.items():
        t = np.asarray(truth[name], np.float64)
        g = np.asarray(got[name], np.float64)
        nz = t != 0
        assert np.array_equal(g[~nz], t[~nz]), (tr.name, name, "a value that is exactly 0 in the oracle")
        worst = max(worst, float(np.max(np.abs(g[nz] - t[nz]) / (bound * np.abs(t[nz])))))
    return worst
