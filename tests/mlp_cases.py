"""The catalogue of MLP edge cases and a pure-Python restatement of the dispatch in ``fv3hip_mlp_predict``.

``expected_variant`` predicts the string ``fv3hip_mlp_last_variant`` reports for a call; ``CATALOGUE`` holds, for every one
of the 36 instantiations of ``mlp_fused_kernel`` (9 kinds x hidden tilings 1, 2, 4, 8), both ``mlp_small_kernel``
instantiations and the layered path, a model and a call that select it.  tests/test_host_mlp_edges.py proves that the
catalogue says so (no GPU needed); tests/test_gpu_mlp_edges.py runs every entry and asserts the prediction.

Sample counts are the smallest that reach the edge: 161 on the general kernels (one full 128-sample tile and a ragged
wave), 160 on the fast-I/O kernels (one full tile and one whole wave of a partial tile).
"""
import dataclasses
from typing import Optional, Tuple

import numpy as np

from tolerances import decades

FLT_MIN = float(np.finfo(np.float32).tiny)
K_MAX = 2048          # kMaxK
TILE = 128            # kTileSamples
LDS_MAX = 160 * 1024
LAYERED_SLAB = 65536  # kLayeredSlab


class VariantRefused(Exception):
    """The entry point refuses the call (FV3HIP_EUNSUPPORTED)."""


# ---------------------------------------------------------------------------------------------------------------------
# the predicted dispatch
# ---------------------------------------------------------------------------------------------------------------------
def _flag(b):
    return "true" if b else "false"


def fused_geometry(spec):
    """What fused_geometry / pack_fused of mlp.hip derive from a model (only what the dispatch needs)."""
    K, F, width, nh = spec.n_in_features, spec.n_out_features, spec.width, len(spec.hidden_kernels)
    HT = next(v for v in (1, 2, 4, 8) if 32 * v >= width)
    hout = bool(spec.hidden_output)
    has_limits = any(o.min is not None or o.max is not None or o.mask is not None for o in spec.outputs)
    n_chunks1 = ((K + 1) // 2 + 15) // 16
    n_ktab = 32 * n_chunks1
    nt_out = (F + 31) // 32
    n_otab = 32 * ((HT if hout else 0) + nt_out)
    n_bias = nh * HT * 32 + nt_out * 32
    smallf_n = F if (1 <= F <= 4 and not has_limits and not spec.residuals) else 0
    if smallf_n:
        n_bias += HT * 32 * 4
    n_log = sum(i.nfeat for i in spec.inputs if i.transform == "log")
    n_pad = (32 - n_log % 32) % 32
    n_log_padded = n_log + n_pad if (n_log > 0 and n_log + n_pad + (K - n_log) <= n_ktab) else n_log
    ch_h, ch_o = 16 * ((HT + 3) // 4) * 64, HT * 256  # float4 per hidden-type / output-type chunk
    lds_bytes = (2 * max(ch_h, ch_o) * 16 + n_ktab * 32 + n_otab * (16 + 16 + (32 if spec.residuals else 0))
                 + ((n_bias + 3) & ~3) * 4 + (3 * 16 + 3 * 32) * 8)
    return dict(K=K, F=F, width=width, n_hidden=nh, HT=HT, hout=hout, has_limits=has_limits, n_ktab=n_ktab, nt_out=nt_out,
                smallf_n=smallf_n, n_log_chunks=(n_log_padded + 31) // 32, lds_bytes=lds_bytes,
                padded_input_rows=n_ktab - K, padded_hidden=HT * 32 - width)


def expected_variant(spec, n, src_dtype, out_dtype, fast_layout, n_cu, small_limit) -> str:
    """The string ``MlpModel.last_variant`` holds after a ``predict`` of ``n`` samples (mlp.hip, fv3hip_mlp_predict).

    ``src_dtype`` / ``out_dtype``: numpy dtypes (or their names) of the sources as the kernel sees them (a mixed pair is
    promoted to float64 by the wrapper) and of the outputs.  ``fast_layout``: every source and output has unit sample
    stride, a 16-byte aligned base and a feature stride that is a multiple of 16 bytes.  ``small_limit``: what the model
    was built with (None = the library's rule, 32 samples per compute unit; the FV3HIP_MLP_SMALL_MAX_SAMPLES override of
    the environment is not modelled)."""
    src64 = np.dtype(src_dtype) == np.float64
    out64 = np.dtype(out_dtype) == np.float64
    nh, width, K = len(spec.hidden_kernels), spec.width, spec.n_in_features
    if nh < 1 or width > 256 or K > K_MAX or spec.activation != "relu":
        if spec.hidden_output:
            raise VariantRefused("hidden-output models outside the fused kernels' range")
        return f"layered (gather, {nh + 1} x layered_dense_kernel, scatter; slabs of {LAYERED_SLAB} samples)"
    g = fused_geometry(spec)
    if g["lds_bytes"] > LDS_MAX:
        raise VariantRefused("model tables exceed the LDS")
    HT = g["HT"]
    limit = small_limit if (small_limit is not None and small_limit >= 0) else 32 * n_cu
    lds_small = (2 * 128 * 32 + 2 * HT * 32 * 32) * 4 + g["n_ktab"] * 32 + 3 * (32 + 16) * 8
    if n <= limit and g["nt_out"] + (HT if g["hout"] else 0) > 0 and lds_small <= LDS_MAX:
        return f"mlp_small_kernel<{_flag(src64)}> (32-sample workgroups, features split over 8 waves)"
    xbulk = bool(fast_layout) and n % 32 == 0 and g["lds_bytes"] + 2 * 32 * TILE * 4 <= LDS_MAX
    if g["hout"] and src64:
        raise VariantRefused("hidden-output models take float32 sources only")
    smallf = bool(g["smallf_n"]) and xbulk and not src64 and not out64
    l1short = smallf and not g["hout"] and K <= 16 and g["n_log_chunks"] == 0
    src64_v = src64 and not smallf and not g["hout"]
    side = xbulk and not smallf and HT == 8 and not g["has_limits"] and not out64 and n >= TILE
    if smallf:
        epi = "small-output"
    elif side and not spec.residuals:
        epi = "plain"
    elif side and not src64_v and not g["hout"]:
        epi = "residual"
    else:
        epi = "general"
    return (f"mlp_fused_kernel<{HT},{_flag(src64_v)},{_flag(xbulk)},{_flag(g['hout'])},{_flag(smallf)},{_flag(l1short)}>"
            f" epilogue={epi}")


# the nine instantiation kinds mlp.hip's kFusedRows compiles per hidden tiling: template flags <SRC64, XBULK, HOUT, SMALLF, L1SHORT>
KINDS = {
    "general": "false,false,false,false,false",
    "fast": "false,true,false,false,false",
    "general64": "true,false,false,false,false",
    "fast64": "true,true,false,false,false",
    "hout_general": "false,false,true,false,false",
    "hout_fast": "false,true,true,false,false",
    "smallf": "false,true,false,true,false",
    "smallf_hout": "false,true,true,true,false",
    "l1short": "false,true,false,true,true",
}
ALL_FUSED = sorted(f"mlp_fused_kernel<{ht},{flags}>" for ht in (1, 2, 4, 8) for flags in KINDS.values())
SMALL_KERNELS = ("mlp_small_kernel<false>", "mlp_small_kernel<true>")
EPILOGUES = ("plain", "residual", "general", "small-output")


def instantiation(variant: str) -> str:
    """The kernel instantiation of a variant string (without the epilogue flavour / the description in parentheses)."""
    return variant.split(" ")[0]


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    """A model and a call.  ``inputs``: (name, source, nfeat, start, log eps or None); ``outputs``: (name, nfeat, min, max,
    number of leading zero-masked levels); ``residuals``: (name, source, output)."""
    name: str
    width: int
    n_hidden: int
    inputs: Tuple[tuple, ...]
    outputs: Tuple[tuple, ...]
    n: int
    residuals: Tuple[tuple, ...] = ()
    hidden_output: bool = False
    src_dtype: str = "float32"
    out_dtype: str = "float32"
    layout: str = "feature_sample"
    small_limit: Optional[int] = 0
    activation: str = "relu"
    seed: int = 0
    # the rows of (input, feature) get few positive weights through the network, so that +inf there reaches the outputs
    # as an infinity and not only as inf - inf (see build_spec)
    inf_path: Optional[Tuple[str, int]] = None
    big_bias: bool = False  # hidden_biases[0][4] = hidden_biases[0][5] = 2e5 (the padding-row case)

    @property
    def fast_layout(self):
        """Whether the arrays ``device_sources`` / ``MlpModel.predict`` build for this case qualify for fast I/O."""
        return self.layout == "feature_sample"


def build_spec(case: Case):
    from fv3net_amd.mlp import InputSpec, MlpSpec, OutputSpec, ResidualSpec

    rng = np.random.default_rng(case.seed)
    # (a log input is normalised by the mean and spread of the logarithm of what make_sources draws for it, 10^U(-8, -2):
    # the network then sees O(1) values, as the normalisation of a trained model gives it)
    inputs = [InputSpec(source=src, nfeat=nf, start=start, transform="none" if eps is None else "log",
                        eps=0.0 if eps is None else eps,
                        center=(rng.normal(0, 1, nf) if eps is None else rng.normal(-11.5, 1, nf)).astype(np.float32),
                        scale=(rng.uniform(0.5, 2, nf) if eps is None else rng.uniform(2, 6, nf)).astype(np.float32))
              for _, src, nf, start, eps in case.inputs]
    K = sum(i.nfeat for i in inputs)
    hk, hb = [], []
    fan = K
    for _ in range(case.n_hidden):
        hk.append((rng.normal(0, 1, (fan, case.width)) / np.sqrt(fan)).astype(np.float32))  # (never exactly 0)
        hb.append(rng.normal(0, 0.1, case.width).astype(np.float32))
        fan = case.width
    outputs = []
    for name, nf, lo, hi, n_masked in case.outputs:
        limited = lo is not None or hi is not None
        mask = None
        if n_masked:
            mask = np.ones(nf, np.float32)
            mask[:n_masked] = 0
        # per-level standard deviations over 4.5 decades (the gate is per level); limited outputs: see the end
        outputs.append(OutputSpec(name=name, nfeat=nf, min=lo, max=hi, mask=mask,
                                  scale=rng.uniform(0.5, 2, nf).astype(np.float32) if limited else decades(rng, nf),
                                  center=rng.normal(0, 1, nf).astype(np.float32) * (1 if limited else decades(rng, nf, top=0.5))))
    F = sum(o.nfeat for o in outputs)
    spec = MlpSpec(inputs=inputs, hidden_kernels=hk, hidden_biases=hb, outputs=outputs,
                   out_kernel=(rng.normal(0, 1, (fan, F)) / np.sqrt(fan)).astype(np.float32),
                   out_bias=rng.normal(0, 0.1, F).astype(np.float32),
                   residuals=[ResidualSpec(name=n_, source=s, output=o) for n_, s, o in case.residuals],
                   activation=case.activation, hidden_output="h" if case.hidden_output else None)
    if case.inf_path is not None:
        # +inf in that feature: layer 1 gives +inf in hidden units 0, 1 and -inf (0 after the ReLU) in all others; the rows
        # 0, 1 of every later hidden kernel do the same; so the last hidden layer holds +inf in units 0, 1 and finite
        # values elsewhere, and an output is +-inf where its two weights agree in sign and NaN where they do not
        name, feat = case.inf_path
        k = 0
        for (iname, _, nf, _, _) in case.inputs:
            if iname == name:
                k += feat
                break
            k += nf
        hk[0][k, :] = -np.abs(hk[0][k, :])
        hk[0][k, :2] = np.abs(hk[0][k, :2])
        for kern in hk[1:]:
            kern[:2, :] = -np.abs(kern[:2, :])
            kern[:2, :2] = np.abs(kern[:2, :2])
        # (... they agree at the even output features and differ at the odd ones)
        ok = spec.out_kernel
        ok[1, 0::2] = np.abs(ok[1, 0::2]) * np.sign(ok[0, 0::2])
        ok[1, 1::2] = -np.abs(ok[1, 1::2]) * np.sign(ok[0, 1::2])
    if case.hidden_output:
        # The gate is per level, against the level's own maximum over the samples.  A hidden unit that the ReLU clips for
        # almost every sample has a maximum far below the terms it sums, and no float32 evaluation -- the float32 oracle
        # included -- is within 1e-5 of that.  Every unit of the hidden output gets the bias that centres its
        # pre-activation on the case's own inputs a little above zero: it is then clipped for a good third of the
        # samples and its maximum is of the size of its terms (tests/test_host_mlp_edges.py holds every case to this:
        # the float32 oracle itself must pass the gate's first clause four times over).
        from oracle import mlp_np

        head = MlpSpec(inputs=inputs, hidden_kernels=hk[:-1], hidden_biases=hb[:-1], outputs=[OutputSpec("p", case.width)],
                       out_kernel=hk[-1], out_bias=np.zeros(case.width, np.float32))
        pre = mlp_np.forward(head, make_sources(case), dtype=np.float64)["p"]
        hb[-1][:] = (-np.median(pre, axis=0) + rng.uniform(0.2, 1.0, case.width) * pre.std(axis=0)).astype(np.float32)
    if case.big_bias:
        # (the two units then hold about 2e5; their rows of the next kernel are scaled so that they weigh as much as the
        # other units -- a sum dominated by two constants of that size would cancel down to the levels' scales in float32)
        hb[0][4] = hb[0][5] = 2.0e5
        hk[1][4:6, :] *= np.float32(1e-5)
    if any(o.min is not None or o.max is not None for o in outputs):
        # A limited output is de-normalised so that, on the case's own inputs, every level spreads a little wider than its
        # limits: they cut on both sides at every level, yet most samples of a level stay inside, so that the level's
        # maximum error is taken over many samples and its scale -- the limit -- is the size of the values.  (Limits far
        # inside the spread leave a handful of samples per level and a scale far below the terms summed.)
        from oracle import mlp_np

        raw = MlpSpec(inputs=inputs, hidden_kernels=hk, hidden_biases=hb, outputs=[OutputSpec("p", F)],
                      out_kernel=spec.out_kernel, out_bias=spec.out_bias, activation=case.activation)
        yhat = mlp_np.forward(raw, make_sources(case), dtype=np.float64)["p"]
        f0 = 0
        for o in outputs:
            if o.min is not None and o.max is not None:
                y = yhat[:, f0:f0 + o.nfeat]
                o.scale = (0.7 * (o.max - o.min) / 2 / y.std(axis=0)).astype(np.float32)
                o.center = ((o.max + o.min) / 2 + rng.uniform(-0.1, 0.1, o.nfeat) - y.mean(axis=0) * o.scale).astype(np.float32)
            f0 += o.nfeat
    spec.validate()
    return spec


def source_shapes(case: Case):
    """source name -> (number of features, whether a log input reads it)."""
    need = {}
    for _, src, nf, start, eps in case.inputs:
        f, pos = need.get(src, (0, False))
        need[src] = (max(f, start + nf), pos or eps is not None)
    nfo = {name: nf for name, nf, *_ in case.outputs}
    for _, src, out in case.residuals:
        f, pos = need.get(src, (0, False))
        need[src] = (max(f, nfo[out]), pos)
    return need


def make_sources(case: Case, n: Optional[int] = None):
    """name -> [sample, feature] arrays of the case's source dtype (values exactly representable in float32)."""
    rng = np.random.default_rng(case.seed + 1000)
    n = case.n if n is None else n
    out = {}
    for src, (nf, positive) in source_shapes(case).items():
        a = 10.0 ** rng.uniform(-8, -2, (n, nf)) if positive else rng.normal(0, 1, (n, nf))
        out[src] = a.astype(np.float32).astype(case.src_dtype)
    return out


def _c(name, width, n_hidden, inputs, outputs, n, **kw):
    import zlib

    return Case(name=name, width=width, n_hidden=n_hidden, inputs=tuple(inputs), outputs=tuple(outputs), n=n,
                seed=zlib.crc32(name.encode()) % 100000, **kw)


# input sets: K = 58 with a clipped input (start 3) and a log view of the same source, the log block too long to be
# padded to a whole chunk (a mixed chunk); K = 42 whose 12 log rows are padded to a chunk and followed by a plain one
# (the 8-slot log chunk of the fast-I/O kernels); K = 40 plain; K = 12 clipped (the short first chunk)
IN_MIXED = (("T", "T", 19, 0, None), ("q", "q", 19, 3, None), ("logq", "q", 19, 3, 1e-8), ("ps", "ps", 1, 0, None))
IN_SHORTLOG = (("a", "a", 30, 0, None), ("lg", "b", 12, 0, 1e-8))
IN_PLAIN40 = (("a", "a", 40, 0, None),)
IN_CLIP12 = (("a", "a", 12, 2, None),)
# output sets: limits, a zero mask and a residual of a clipped source (39 features, 2 tiles); one plain head of F features
OUT_LIMITS = (("dQ1", 19, None, None, 3), ("dQ2", 19, -0.5, 0.75, 0), ("pr", 1, None, None, 0))
RES_LIMITS = (("q_after", "q", "dQ2"),)


def OUT_PLAIN(F):
    return (("y", F, None, None, 0),)


RES_PLAIN = (("y_after", "before", "y"),)


def OUT_SMALL(n_out):
    return tuple((f"y{i}", 1, None, None, 0) for i in range(n_out))


WIDTHS = {1: (20, 32), 2: (40, 64), 4: (100, 128), 8: (200, 256)}  # per hidden tiling: with and without padded features


def _kind_case(kind, ht, variant=0):
    """One case of instantiation kind ``kind`` at hidden tiling ``ht``.  The two widths of a tiling, the depth, the
    layout and the output dtype alternate over the kinds, so that each tiling sees padded and unpadded hidden features."""
    wa, wb = WIDTHS[ht]
    name = f"{kind}-ht{ht}" + (f"-v{variant}" if variant else "")
    if kind == "general":
        return _c(name, wa, 2, IN_MIXED, OUT_LIMITS, 161, residuals=RES_LIMITS, layout="sample_feature")
    if kind == "fast":
        return _c(name, wb, 2, IN_SHORTLOG, OUT_LIMITS[:2], 160)
    if kind == "general64":
        return _c(name, wb, 3, IN_SHORTLOG, OUT_PLAIN(33), 161, residuals=RES_PLAIN, src_dtype="float64", out_dtype="float64")
    if kind == "fast64":
        return _c(name, wa, 1, IN_MIXED, OUT_LIMITS, 160, residuals=RES_LIMITS, src_dtype="float64")
    if kind == "hout_general":
        return _c(name, wb, 2, IN_MIXED, OUT_PLAIN(7), 161, hidden_output=True)
    if kind == "hout_fast":
        return _c(name, wa, 2, IN_SHORTLOG, (), 160, hidden_output=True)
    if kind == "smallf":
        return _c(name, wa, 2, IN_MIXED, OUT_SMALL(3), 160)
    if kind == "smallf_hout":
        return _c(name, wb, 1, IN_PLAIN40, OUT_SMALL(4), 160, hidden_output=True)
    if kind == "l1short":
        return _c(name, wa if ht in (1, 4) else wb, 2, IN_CLIP12, OUT_SMALL(1 + ht % 3), 160)
    raise KeyError(kind)


def _catalogue():
    cases = [_kind_case(kind, ht) for ht in (1, 2, 4, 8) for kind in KINDS]
    # the 8-tile fast-I/O kernels without the small-output path: 1, 2 and 3 output tiles (the one-tile loop and both
    # parities of the accumulator swap), with and without residual outputs -- the branch-free side epilogue on the full
    # tile (float32 sources: "plain" / "residual"; float64 sources and hidden-output models take the general one with
    # residuals), the general one on the partial tile of the same launch
    for F in (20, 40, 70):
        for res in (False, True):
            tag = f"F{F}" + ("-res" if res else "")
            r = RES_PLAIN if res else ()
            w = 256 if F != 40 else 200
            cases.append(_c(f"side-fast-{tag}", w, 2, IN_PLAIN40, OUT_PLAIN(F), 160, residuals=r))
            cases.append(_c(f"side-fast64-{tag}", w, 2, IN_PLAIN40, OUT_PLAIN(F), 160, residuals=r, src_dtype="float64"))
            cases.append(_c(f"side-hout-{tag}", w, 2, IN_PLAIN40, OUT_PLAIN(F), 160, residuals=r, hidden_output=True))
    # both feature-split kernels (any count goes to them with a large limit) and the layered path (no hidden layer, a
    # hidden layer wider than 256, hidden layers without activation)
    big = 1 << 40
    cases.append(_c("small-f32", 100, 2, IN_MIXED, OUT_LIMITS, 161, residuals=RES_LIMITS, small_limit=big, hidden_output=True))
    cases.append(_c("small-f64", 40, 2, IN_SHORTLOG, OUT_PLAIN(33), 161, residuals=RES_PLAIN, small_limit=big,
                    src_dtype="float64", layout="sample_feature"))
    cases.append(_c("layered-linear-model", 58, 0, IN_MIXED, OUT_LIMITS, 161, residuals=RES_LIMITS))
    cases.append(_c("layered-wide", 288, 2, IN_SHORTLOG, OUT_PLAIN(33), 161, residuals=RES_PLAIN, src_dtype="float64"))
    cases.append(_c("layered-no-activation", 40, 2, IN_PLAIN40, OUT_PLAIN(20), 161, activation="linear", layout="sample_feature"))
    return cases


CATALOGUE = _catalogue()


# ---------------------------------------------------------------------------------------------------------------------
# non-finite inputs (test_gpu_mlp_edges.py, section c)
# ---------------------------------------------------------------------------------------------------------------------
EPS_NORMAL, EPS_DENORMAL = 1e-8, 1e-40  # >= FLT_MIN: the fast log on fast-I/O launches; denormal: logf


def poison_case(kind, ht, eps=EPS_NORMAL):
    """One plain and one log input (the short-first-chunk kernel takes no log input: plain only).  Width 20 (HT = 1) has
    padded hidden features and padded input rows; width 256 (HT = 8) has K = 64 and no padding anywhere, except the
    short-first-chunk kernel, whose K <= 16 always leaves padding rows."""
    width = {1: 20, 8: 256}[ht]
    kp, kl = (12, 9) if ht == 1 else (32, 32)
    inputs = (("x", "x", kp, 0, None), ("lg", "q", kl, 0, eps))
    name = f"poison-{kind}-ht{ht}-{'normal' if eps >= FLT_MIN else 'denormal'}"
    kw = dict(inf_path=("x", 5))
    if kind in ("general", "fast", "general64", "fast64"):
        kw.update(residuals=RES_PLAIN, src_dtype="float64" if kind.endswith("64") else "float32")
        # (a limited and partly masked head on two of the four: the limiter and the mask must keep a NaN; the other two stay
        # without, so that the 8-tile fast-I/O kernel runs its branch-free side epilogue on the poisoned full tile)
        outs = OUT_PLAIN(20) + ((("z", 6, -0.5, 0.75, 2),) if kind in ("general", "fast64") else ())
        return _c(name, width, 2, inputs, outs, 161 if kind.startswith("general") else 160, **kw)
    if kind in ("hout_general", "hout_fast"):
        return _c(name, width, 2, inputs, OUT_PLAIN(7), 161 if kind == "hout_general" else 160, hidden_output=True, **kw)
    if kind in ("smallf", "smallf_hout"):
        return _c(name, width, 2, inputs, OUT_SMALL(4), 160, hidden_output=kind == "smallf_hout", **kw)
    if kind == "l1short":
        return _c(name, width, 2, (("x", "x", 12, 0, None),), OUT_SMALL(4), 160, **kw)
    if kind in ("small-f32", "small-f64"):
        return _c(name, width, 2, inputs, OUT_PLAIN(20), 161, residuals=RES_PLAIN, small_limit=1 << 40,
                  src_dtype="float64" if kind == "small-f64" else "float32", **kw)
    if kind == "layered":
        return _c(name, 288, 2, inputs, OUT_PLAIN(20), 161, residuals=RES_PLAIN, **kw)
    raise KeyError(kind)


def poison_cases():
    cases = []
    for ht in (1, 8):
        for kind in KINDS:
            cases.append(poison_case(kind, ht))
            if KINDS[kind].split(",")[1] == "true" and kind != "l1short":  # fast I/O with a log input: the other log
                cases.append(poison_case(kind, ht, EPS_DENORMAL))
    cases += [poison_case("small-f32", 1), poison_case("small-f64", 8), poison_case("layered", 8)]
    return cases


def poisons(case: Case):
    """[(sample, source, feature, value, class)]: distinct poisons at the first and last lanes of the first waves, at
    the tile boundary and in the last vector / the last sample of the call.  ``class``: "nan", "inf" (a +-inf that reaches
    the network) or "floor" (a log input the floor replaces: 0, a negative value, -inf)."""
    n = case.n
    has_log = any(eps is not None for *_, eps in case.inputs)
    plain = [(0, "x", 3, np.nan, "nan"), (32, "x", 5, np.inf, "inf"), (63, "x", 7, -np.inf, "inf"), (n - 1, "x", 5, np.inf, "inf")]
    if not has_log:
        return plain + [(31, "x", 0, np.nan, "nan"), (127, "x", 11, -np.inf, "inf"), (128, "x", 2, np.nan, "nan"),
                        (n - 4, "x", 9, np.inf, "inf")]
    return plain + [(31, "q", 2, np.nan, "nan"), (127, "q", 4, np.inf, "inf"), (128, "q", 1, -np.inf, "floor"),
                    (n - 4, "q", 0, 0.0, "floor"), (64, "q", 8, -3.5, "floor")]


def poisoned_sources(case: Case):
    """(clean sources, poisoned sources, {sample: class})."""
    clean = make_sources(case)
    bad = {k: v.copy() for k, v in clean.items()}
    classes = {}
    for sample, src, feat, value, cls in poisons(case):
        bad[src][sample, feat] = value
        assert sample not in classes
        classes[sample] = cls
    return clean, bad, classes


# ---------------------------------------------------------------------------------------------------------------------
# the padding row (section 4): K = 33 leaves 31 padding rows in the fused kernels' input table, which used to read the
# first biases -- as doubles with float64 sources
# ---------------------------------------------------------------------------------------------------------------------
def padding_case(fast: bool):
    return _c(f"padding-bias-{'fast' if fast else 'general'}", 40, 2, (("a", "a", 33, 0, None),), OUT_PLAIN(20),
              160 if fast else 161, src_dtype="float64", big_bias=True)
