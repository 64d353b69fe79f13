"""Inputs shared by tests/test_host_precipitative.py (which pins the numpy restatement and the gates on them, on the CPU) and
tests/test_gpu_precipitative.py (which runs fv3hip_precip_closure and the predictor on them)."""
import dataclasses

import numpy as np

import precipitative_np as P
from tolerances import decades

NZS = (0, 1, 2, 79)
NS = (1, 63, 64, 65, 256, 257, 1000)            # around one wave and one 256-thread block, and several blocks
DTYPES = (("f32", "f32"), ("f32", "f64"), ("f64", "f32"), ("f64", "f64"))   # (delp, physics_precip)
LAYOUTS = ("contiguous", "transposed", "stride2", "one_thickness")
# contiguous [z, n]; the transposed view of an [n, z] array; columns [::2] of a twice as wide array (physics_precip every
# second element too); feature stride 0 -- one thickness for every level
MODES = ("precip_only", "in_place", "out_of_place")   # couple = 0; couple = 1 over the residual heads / into new arrays


@dataclasses.dataclass(frozen=True)
class Case:
    nz: int
    n: int
    delp_dtype: str
    pp_dtype: str
    layout: str
    mode: str

    @property
    def couple(self):
        return self.mode != "precip_only"

    @property
    def id(self):
        return f"nz{self.nz}-n{self.n}-{self.delp_dtype}-{self.pp_dtype}-{self.layout}-{self.mode}"


def _block(sizes, others, as_nz, shift=0):
    """Every size of ``sizes`` with every dtype pair, every layout and every mode; the other extent cycles."""
    out = []
    for a, size in enumerate(sizes):
        for slot in range(4):
            other = others[(a + slot + shift) % len(others)]
            nz, n = (size, other) if as_nz else (other, size)
            out.append(Case(nz, n, *DTYPES[slot], LAYOUTS[(slot + a) % 4], MODES[(slot + a) % 3]))
    return out


KERNEL_CASES = _block(NS, NZS, as_nz=False) + _block(NZS, NS, as_nz=True, shift=2)   # 28 + 16 launches


def kernel_inputs(case, seed=0):
    """(t_res, q_res, cp [nz, n] float32, delp [nz, n], pp [n]) of the case's dtypes.  float64 thicknesses are no float32
    values (a kernel that multiplied in double and rounded late would differ), float64 physics_precip neither."""
    rng = np.random.default_rng([seed, case.nz, case.n])
    nz, n = case.nz, case.n
    t_res = rng.normal(0, 1e-4, (nz, n)).astype(np.float32)
    q_res = rng.normal(0, 1e-7, (nz, n)).astype(np.float32)
    cp = (rng.normal(0, 1, (nz, n)) * 10.0 ** rng.uniform(-9, -6, (nz, 1))).astype(np.float32)
    delp = rng.uniform(300, 1500, (1 if case.layout == "one_thickness" else nz, n)) + 1e-9
    delp = np.broadcast_to(delp, (nz, n)).astype(np.float64 if case.delp_dtype == "f64" else np.float32)
    pp = rng.uniform(0, 1e-4, n).astype(np.float64 if case.pp_dtype == "f64" else np.float32)
    if case.delp_dtype == "f64":
        assert np.all(delp.astype(np.float32) != delp)
    if case.pp_dtype == "f64":
        assert np.all(pp.astype(np.float32) != pp)
    return t_res, q_res, cp, np.ascontiguousarray(delp), pp


def fma_precip(cp, delp, pp):
    """What a contracted multiply-add would give: each level's product is added UNROUNDED (a float32 product is exact in
    float64) and the sum rounded once per level."""
    d = np.asarray(delp).astype(np.float32).astype(np.float64)
    acc = np.zeros(cp.shape[1], np.float32)
    for k in range(cp.shape[0]):
        acc = (acc.astype(np.float64) + cp[k].astype(np.float64) * d[k]).astype(np.float32)
    return np.asarray(pp).astype(np.float32) + P.C_G * acc


FMA_CASE = Case(79, 64, "f32", "f32", "contiguous", "precip_only")

NONFINITE_NZ, NONFINITE_N, NONFINITE_LEVEL, NONFINITE_COLUMN = 5, 130, 2, 70   # the middle of the second wave
NONFINITE_CASE = Case(NONFINITE_NZ, NONFINITE_N, "f64", "f32", "contiguous", "out_of_place")
NONFINITE_ARRAYS = ("cp", "t_res", "q_res", "delp", "physics_precip")
NONFINITE_VALUES = (np.nan, np.inf, -np.inf)


def nonfinite_inputs(which, value):
    """The inputs of NONFINITE_CASE with ``value`` at one level of one column of the array ``which``.  Where the thickness
    is poisoned the column precipitation there is zero: ``inf * 0`` must give NaN."""
    t_res, q_res, cp, delp, pp = kernel_inputs(NONFINITE_CASE, seed=3)
    arrays = {"cp": cp, "t_res": t_res, "q_res": q_res, "delp": delp, "physics_precip": pp}
    a = arrays[which]
    if which == "physics_precip":
        a[NONFINITE_COLUMN] = value
    else:
        a[NONFINITE_LEVEL, NONFINITE_COLUMN] = value
    if which == "delp":
        cp[NONFINITE_LEVEL, NONFINITE_COLUMN] = 0.0
    return t_res, q_res, cp, delp, pp


def cancellation_inputs(nz=79, n=257, seed=5):
    """cp of alternating sign whose terms cancel in pairs to a part in a thousand, magnitudes over six decades."""
    rng = np.random.default_rng(seed)
    pairs = (nz + 1) // 2
    mag = 10.0 ** rng.uniform(-6, 0, (pairs, n))
    delp = np.repeat(rng.uniform(300, 1500, (pairs, n)), 2, axis=0)[:nz].astype(np.float32)
    cp = np.repeat(mag, 2, axis=0)[:nz]
    cp[1::2] *= -(1 + rng.uniform(-1e-3, 1e-3, cp[1::2].shape))
    cp[-1] *= 1e-6   # (the level without a partner)
    pp = rng.uniform(0, 1e-4, n).astype(np.float32)
    return cp.astype(np.float32), delp, pp


def cancellation_gate(precip, cp, delp, pp):
    """``|precip - truth64| <= (nz + 2) * 2**-24 * (|pp| + (1/g) * sum_k |cp[k] * delp[k]|)``: one rounded product per level,
    a sequential float32 sum of nz terms, one scaling and one add.  Returns (error, bound, terms over |integral|)."""
    nz = cp.shape[0]
    terms = np.abs(cp.astype(np.float64) * delp.astype(np.float64))
    _, _, truth = P.closure64(None, None, cp, delp, pp, couple=False)
    bound = (nz + 2) * 2.0 ** -24 * (np.abs(pp.astype(np.float64)) + terms.sum(axis=0) / P.GRAVITY)
    integral = np.abs(np.sum(cp.astype(np.float64) * delp.astype(np.float64), axis=0))
    return np.abs(np.asarray(precip, np.float64) - truth), bound, terms.sum(axis=0) / integral


# ---------------------------------------------------------------------------------------------------------------------
# the model of the parity tests: 79 + 79 + 79 + 1 -> 16 -> 16 -> 3 x 79 (the reference's defaults, depth 3)
# ---------------------------------------------------------------------------------------------------------------------
NAMES_IN = ["air_temperature", "specific_humidity", P.DELP, P.PHYS_PRECIP]
NAMES_OUT = ["dQ1", "dQ2", "total_precipitation_rate"]
PARITY_SMALL_LIMIT = 512        # samples up to which the model of the parity test runs the small kernel
PARITY_COLUMNS = (333, 777)     # one count on each side of it, neither a multiple of a tile


def state(n, nz=79, seed=1):
    """name -> [sample, feature] float64: T ~ U(200, 300), q ~ U(0, 0.02) (BASELINE config 1), delp ~ U(300, 1500),
    physics_precip ~ U(0, 1e-4)."""
    rng = np.random.default_rng([seed, n])
    return {"air_temperature": rng.uniform(200, 300, (n, nz)), "specific_humidity": rng.uniform(0, 0.02, (n, nz)),
            P.DELP: rng.uniform(300, 1500, (n, nz)), P.PHYS_PRECIP: rng.uniform(0, 1e-4, n)}


def arrays_for_spec(nz=79, width=16, depth=3, clip=None, seed=0):
    """The arguments of ``precipitative_spec_from_arrays``: weights N(0, 1/sqrt(fan_in)), normalisation fitted on a sample of
    ``state``, output scales that fall over two decades (dQ1 ~ 1e-4 K/s, dQ2 ~ 1e-7 kg/kg/s)."""
    rng = np.random.default_rng(seed)
    clip = dict(clip or {})
    sample = state(2048, nz, seed=99)
    means, stds = [], []
    for name in NAMES_IN:
        a = sample[name].reshape(2048, -1)
        a = a[:, clip[name]] if name in clip else a
        means.append(a.mean(axis=0).astype(np.float32))
        stds.append(a.std(axis=0).astype(np.float32))
    fan = sum(m.shape[0] for m in means)
    hk, hb = [], []
    for _ in range(depth - 1):
        hk.append((rng.normal(0, 1, (fan, width)) / np.sqrt(fan)).astype(np.float32))
        hb.append(rng.normal(0, 0.1, width).astype(np.float32))
        fan = width
    head_k = [(rng.normal(0, 1, (width, nz)) / np.sqrt(width)).astype(np.float32) for _ in range(3)]
    head_b = [rng.normal(0, 0.1, nz).astype(np.float32) for _ in range(3)]
    out_std = [decades(rng, nz, 2, 1e-4), decades(rng, nz, 2, 1e-7)]
    out_mean = [(rng.normal(0, 1, nz) * s).astype(np.float32) for s in out_std]
    return dict(input_variables=NAMES_IN, input_means=means, input_stds=stds, hidden_kernels=hk, hidden_biases=hb,
                head_kernels=head_k, head_biases=head_b, output_means=out_mean, output_stds=out_std, clip=clip)


PARITY_VARIANTS = {   # name -> (couple, input clip)
    "coupled": (True, None),
    "uncoupled": (False, None),
    "clipped_delp": (True, {P.DELP: slice(10, None)}),
}


def precip_gate(got, truth, cpu32, src, cp_truth):
    """The per-level 1e-5 gate carried through the linear functional: |got - truth| <= 1e-5 * (max |pp| + (1/g) sum_k
    max_i |cp_truth[i, k]| max_i |delp[i, k]|), and no worse than 8x the float32 restatement's own error + 1e-7 of that scale.
    Returns (worst error, scale, worst error of the float32 restatement)."""
    scale = np.max(np.abs(src[P.PHYS_PRECIP])) + np.sum(np.max(np.abs(cp_truth), axis=0) * np.max(np.abs(src[P.DELP]), axis=0)) / P.GRAVITY
    err = np.max(np.abs(np.asarray(got, np.float64) - truth))
    err32 = np.max(np.abs(np.asarray(cpu32, np.float64) - truth))
    return err, scale, err32


def assert_precip_gate(got, truth, cpu32, src, cp_truth, name=""):
    err, scale, err32 = precip_gate(got, truth, cpu32, src, cp_truth)
    assert err <= 1e-5 * scale, (name, err, scale)
    assert err <= 8 * err32 + 1e-7 * scale, (name, err, err32, scale)
