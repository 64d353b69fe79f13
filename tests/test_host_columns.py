"""tests/column_np.py -- the numpy references tests/test_gpu_column_edges.py holds the column kernels of csrc/vertical.hip to --
pinned on the host against oracle/coarsen_np.py and oracle/coarsen_restarts_np.py, on the inputs the GPU tests use
(tests/column_cases.py)."""
import numpy as np
import pytest

import column_cases as cases
import column_np as C
from glue_np import assert_same_bits as same_bits
from oracle import coarsen_np as onp
from oracle import coarsen_restarts_np as rnp

F32, F64 = np.float32, np.float64
nan, inf = np.nan, np.inf
PAIRS = {"ff": (F32, F32), "fd": (F32, F64), "df": (F64, F32), "dd": (F64, F64)}


def _all_cases(dtype):
    for nz in cases.NZS:
        for shape, z_axis in cases.layouts(nz):
            yield nz, shape, z_axis, cases.column_fields(dtype, shape, z_axis)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_pressure_at_interface_is_the_oracles_cumsum_and_a_nan_poisons_what_lies_below(dtype):
    for nz, shape, z_axis, f in _all_cases(dtype):
        got = C.pressure_at_interface(f["delp"], cases.TOA, z_axis)
        with np.errstate(all="ignore"):
            same_bits(got, onp.pressure_at_interface(f["delp"], cases.TOA, z_axis), err_msg=f"{shape}")
        cols = cases.as_columns(got, z_axis)
        assert cols.shape[0] == nz + 1 and (cols[0] == dtype(cases.TOA)).all()
        bad = np.isnan(cols)
        if cols.shape[1] >= 3:  # NaN at level nz // 2: interfaces nz // 2 + 1 .. nz; the infinity stays an infinity
            want = np.zeros_like(bad)
            want[nz // 2 + 1:, cases.NAN_COLUMN] = True
            np.testing.assert_array_equal(bad, want)
            assert np.isposinf(cols[nz // 2 + 1:, cases.INF_COLUMN]).all() and np.isfinite(cols[:nz // 2 + 1, cases.INF_COLUMN]).all()
        else:
            assert not bad.any()


def test_empty_and_levelless_columns():
    for dtype in (F32, F64):
        same_bits(C.pressure_at_interface(np.zeros((3, 0, 5), dtype), cases.TOA, 1), np.full((3, 1, 5), cases.TOA, dtype))
        assert C.pressure_at_interface(np.zeros((0, 4, 5), dtype), cases.TOA, 1).shape == (0, 5, 5)
        same_bits(C.column_sum(np.zeros((3, 0, 5), dtype), 1, 300.0), np.full((3, 5), 300.0, dtype))
        same_bits(C.column_sum(np.zeros((3, 0, 5), dtype), 1), np.zeros((3, 5), dtype))
        phis = np.array([0.0, 1234.5, 3e4], dtype)
        empty = np.zeros((0, 3), dtype)
        same_bits(C.hydrostatic_phis(empty, phis, empty, dtype, 0), dtype(C.GRAVITY) * (phis / dtype(C.GRAVITY)))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_column_sum_is_numpys_sum_where_numpy_adds_level_by_level(dtype):
    """Over an axis with more than one element behind it numpy adds the levels one after the other: bit for bit.  Over the
    last axis it adds in pairs: within the bound of any order of summation, ``(nz - 1) * eps * sum|x|``."""
    eps = np.finfo(dtype).eps
    for nz, shape, z_axis, f in _all_cases(dtype):
        for addend in (0.0, cases.TOA):
            got = C.column_sum(f["delp"], z_axis, addend)
            with np.errstate(all="ignore"):
                want = onp.surface_pressure_from_delp(f["delp"], addend, z_axis)
                assert want.dtype == dtype
                if int(np.prod(shape[z_axis + 1:])) > 1:  # (a single column of [nz, 1] is a contiguous row to numpy: pairs)
                    same_bits(got, want, err_msg=f"{shape}")
                    continue
                bound = (nz - 1) * eps * np.abs(f["delp"]).sum(axis=z_axis)   # (nz = 1: equality)
                finite = np.isfinite(want)
                np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
                np.testing.assert_array_equal(got[~finite & ~np.isnan(want)], want[~finite & ~np.isnan(want)])
                assert (np.abs(got[finite] - want[finite]) <= bound[finite]).all()


def test_mask_reference_known_answers():
    """The rule is a strict ``<`` and the fill is +0: written out by hand for one column per surface pressure."""
    big = np.finfo(F32).max
    #         level:   tie  above            below             nan  +inf  -inf  +0   -0
    table = {101325.0: [0, 0, 1, 0, 0, 1, 1, 1], 0.0: [0, 0, 1, 0, 0, 1, 0, 0], -0.0: [0, 0, 1, 0, 0, 1, 0, 0],
             nan: [0] * 8, inf: [0, 0, 1, 0, 0, 1, 1, 1]}
    for ps, keep in table.items():
        levels = np.array(cases._around(np.array([ps], F32))).reshape(1, 8, 1)
        p_fine = np.concatenate([np.zeros((1, 8, 1), F32), np.full((1, 1, 1), ps, F32)], axis=1)
        for w in cases.WEIGHT_SPECIALS:
            got = C.mask_weights(np.full((1, 1), w, F32), levels, p_fine, 0)
            same_bits(got.reshape(-1), np.where(np.array(keep, bool), F32(w), F32(0.0)), err_msg=f"ps={ps} w={w}")
    assert cases._around(np.array([inf], F32))[2][0] == big


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("extrapolate", [False, True])
def test_mask_references_are_the_oracles(pair, extrapolate):
    tw, tp = PAIRS[pair]
    for n_batch, nz, n_inner in cases.MASK_TABLE_SHAPES:
        w, pc, pf, off = cases.mask_case(tw, tp, n_batch, nz, n_inner, extrapolate)
        got = C.mask_weights(w, pc, pf, off)
        assert got.dtype == tw and got.shape == (n_batch, nz, n_inner) and off == (0 if extrapolate else 1)
        same_bits(got, onp.mask_weights(w, pc, pf, 1, pfull_coarse_on_fine=pc, extrapolate=extrapolate))
    for ny, nx, f in cases.COARSE_SHAPES:
        w, pc, pf, off = cases.coarse_mask_case(tw, tp, 2, 3, ny, nx, f, extrapolate)
        assert pc.shape[-2:] == (cases.coarse_extent(ny, f), cases.coarse_extent(nx, f))
        up = C.upsample_onto(pc, ny, nx, f)
        if (ny, nx, f) != (9, 12, 4):  # (12 unstaggered columns in 3 blocks: the oracle would take the 3 for a staggered dim)
            same_bits(up, onp.block_upsample(pc, f))
        else:
            same_bits(up, np.repeat(onp._upsample_axis(pc, f, -2), f, axis=-1))
        got = C.mask_weights_coarse(w, pc, pf, off, f)
        same_bits(got, onp.mask_weights(w, up, pf, 1, pfull_coarse_on_fine=up, extrapolate=extrapolate))
        ps, level = pf[:, 3][:, None], up[:, off:off + 3]
        with np.errstate(invalid="ignore"):  # ties, NaNs and both outcomes on either side of a coarse column's edge
            assert (level == ps).sum() >= 4 and np.isnan(level).any() and np.isnan(ps).any() and (level < ps).any() and (level > ps).any()


def test_mask_cases_hold_every_triple_and_w_repeat_shares_a_weight_slice():
    for n_batch, nz, n_inner in cases.MASK_TABLE_SHAPES:
        assert len(cases.mask_triples(n_batch, nz, n_inner)) == 8 * 5 * 5, (n_batch, nz, n_inner)
    w, pc, pf, off = cases.mask_case(F32, F32, 75, 3, 1, False)
    with np.errstate(invalid="ignore"):
        assert (pc[:, 1:] == pf[:, 3:]).sum() >= 20   # (ties; a NaN surface pressure ties with nothing)
    for n_inner in (8, 6):
        w, pc, pf, off = cases.mask_case(F64, F32, 6, 2, n_inner, False, w_repeat=3)
        assert w.shape == (2, n_inner)
        got = C.mask_weights(w, pc, pf, off, w_repeat=3)
        same_bits(got, C.mask_weights(np.repeat(w, 3, axis=0), pc, pf, off))
        assert not np.array_equal(got, C.mask_weights(w[np.arange(6) % 2], pc, pf, off), equal_nan=True)  # (b % 2 is not b // 3)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_blend_reference_is_the_oracles(dtype):
    for nz in cases.NZS:
        for shape, z_axis in cases.layouts(nz):
            pb, ps, p = cases.blend_case(dtype, shape, z_axis)
            got = C.blend_weights(pb, ps, p, z_axis)
            same_bits(got, onp.compute_blending_weights(pb, ps, p, z_axis), err_msg=f"{shape}")
    pb, ps, p = cases.blend_case(dtype, (79, 257), 0)
    got = C.blend_weights(pb, ps, p, 0)
    on = p == pb[None]  # p on pb: not above it, weight 1
    assert on.sum() >= 10 and (got[on] == 1).all()
    assert np.isneginf(got).any() and np.isnan(got).any() and (got == 0).any()   # x / 0, NaN operands, p on ps


def test_midpoint_log_reference_bounds_the_oracle():
    """oracle/coarsen_np.pressure_at_midpoint_log in its own dtype against the float64-log reference, inside the reference's
    conditioning bound.  Worst observed error / bound with numpy on the host: float32 0.161 for delp in U(300, 1500) and 0.122
    for the thin layers (U(1, 50) on 9e4 Pa), float64 0 for both (numpy's float64 log is the reference's own).  No level
    is skipped for its bound except 0.98 % of the thin layers (the test prints the figures: run with -s)."""
    tally = C.Tally()
    for dtype in (F32, F64):
        for thin in (False, True):
            for nz in cases.NZS:
                for shape, z_axis in cases.layouts(nz):
                    f = cases.column_fields(dtype, shape, z_axis, thin=thin)
                    want, bound = C.pressure_at_midpoint_log_f64(f["delp"], cases.TOA, z_axis)
                    with np.errstate(all="ignore"):
                        got = onp.pressure_at_midpoint_log(f["delp"], cases.TOA, z_axis)
                    assert got.dtype == dtype and want.dtype == F64
                    tally.add(f"{np.dtype(dtype).name}{' thin' if thin else ''}", got, want, bound)
                    cols = cases.as_columns(want, z_axis)
                    if cols.shape[1] >= 3:  # the NaN layer and those below it; below the infinite layer inf / inf and inf - inf
                        assert np.isnan(cols[nz // 2:, cases.NAN_COLUMN]).all() and np.isfinite(cols[:nz // 2, cases.NAN_COLUMN]).all()
                        assert np.isnan(cols[nz // 2:, cases.INF_COLUMN]).all()
    tally.check("pressure_at_midpoint_log, numpy:")
    assert tally.worst["float32"] > 0.01   # (the bound is not vacuous: float32 uses a good part of it)


def test_hydrostatic_references_bound_the_oracle():
    """oracle/coarsen_restarts_np.impose_hydrostatic_balance in its own dtype: DZ inside the bound of the float64-log
    reference (worst observed with numpy: float32 0.162, float32 thin 0.122, float64 0), and its phis equal to
    ``hydrostatic_phis`` of its own DZ bit for bit where its sum over z runs level by level (z not the last axis)."""
    tally = C.Tally()
    for dtype in (F32, F64):
        for thin in (False, True):
            for nz in cases.NZS:
                for shape, z_axis in cases.layouts(nz):
                    f = cases.column_fields(dtype, shape, z_axis, thin=thin)
                    want, bound = C.hydrostatic_dz_f64(f["t"], f["q"], f["delp"], cases.TOA, z_axis)
                    # the oracle works on [tile, z, ...]: columns as tiles
                    col = lambda a: np.ascontiguousarray(cases.as_columns(a, z_axis).T)
                    core = dict(DZ=col(f["dz"]), phis=f["phis"].reshape(-1), T=col(f["t"]), delp=col(f["delp"]))
                    with np.errstate(all="ignore"):
                        got = rnp.impose_hydrostatic_balance(core, dict(sphum=col(f["q"])), cases.TOA)
                    assert got["DZ"].dtype == dtype
                    tally.add(f"{np.dtype(dtype).name}{' thin' if thin else ''}", got["DZ"], col(want), col(bound))
    tally.check("hydrostatic DZ, numpy:")
    for dtype in (F32, F64):
        for nz in cases.NZS:
            f = cases.column_fields(dtype, (3, nz, 5, 7), 1)
            core = dict(DZ=f["dz"], phis=f["phis"], T=f["t"], delp=f["delp"])
            with np.errstate(all="ignore"):
                got = rnp.impose_hydrostatic_balance(core, dict(sphum=f["q"]), cases.TOA)
            same_bits(got["phis"], C.hydrostatic_phis(f["dz"], f["phis"], got["DZ"], dtype, 1))


def test_the_float32_quotient_of_the_gas_constants_is_not_the_references_constant():
    """The reference forms ``Rv / Rd - 1`` in Python floats and numpy rounds it once to the array's dtype.  Formed from the
    float32 constants it lies two float32 steps higher, and the virtual temperature then differs, by one to three float32 steps,
    in 1.2 % of values for specific humidities in U(0, 0.025) and in 44 % for U(0, 1)."""
    ref = F32(C.VIRTUAL_COEFFICIENT)
    quotient = F32(C.RVGAS) / F32(C.RDGAS) - F32(1)
    assert ref == F32(0.60773385) and quotient == F32(0.60773396)
    assert np.nextafter(np.nextafter(ref, F32(1)), F32(1)) == quotient
    assert F64(C.RVGAS) / F64(C.RDGAS) - F64(1) == C.VIRTUAL_COEFFICIENT   # (float64 has one value only)
    rng = np.random.default_rng(0)
    t = rng.uniform(200, 320, 200000).astype(F32)
    for q_max, lo, hi in ((0.025, 0.004, 0.03), (1.0, 0.35, 0.55)):
        q = rng.uniform(0, q_max, t.size).astype(F32)
        a, b = C.virtual_temperature(t, q), t * (F32(1) + quotient * q)
        assert a.dtype == F32 and b.dtype == F32
        share = np.mean(a != b)
        assert lo < share < hi, (q_max, share)
        # a few steps, never more: the constants differ by eps, the two products c * q round by eps / 4 each, the two sums and
        # the two final products by eps / 2 each, all relative to a factor in [1, 2)
        assert (np.abs(a.astype(F64) - b) <= 3.5 * np.finfo(F32).eps * a).all()
    # the pairs of the device's differential test can see the difference
    n = sum(cases.virtual_constant_pairs(cases.CONSTANT_PAIRS, cases.CONSTANT_NZ, q_max)[3] for q_max in cases.CONSTANT_Q_MAX)
    assert n >= 100, n


# ------------------------------------------------------------------------------------------------
# the inputs can tell a subtly wrong kernel from a right one: the slips below, played through in numpy
# ------------------------------------------------------------------------------------------------
def _differs(a, b):
    return not (np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b)))


def _mask_with_a_slip(w, p_cmp, p_fine, off, le=False, w_repeat=1, batch_for_slice=False):
    """column_np.mask_weights with ``<=`` for ``<`` / weight slice ``b`` for ``b // w_repeat`` (as far as the slices reach)."""
    nz = p_fine.shape[1] - 1
    level, ps = p_cmp[:, off:off + nz], p_fine[:, nz:nz + 1]
    slices = np.minimum(np.arange(p_fine.shape[0]), w.shape[0] - 1) if batch_for_slice else np.arange(p_fine.shape[0]) // w_repeat
    with np.errstate(invalid="ignore"):
        return np.where((level <= ps) if le else (level < ps), w[slices][:, None], w.dtype.type(0))


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("extrapolate", [False, True])
def test_mask_cases_tell_the_slips_apart(pair, extrapolate):
    tw, tp = PAIRS[pair]
    for shape in cases.MASK_TABLE_SHAPES:  # generic and rows kernel
        w, pc, pf, off = cases.mask_case(tw, tp, *shape, extrapolate)
        want = C.mask_weights(w, pc, pf, off)
        assert not _differs(_mask_with_a_slip(w, pc, pf, off), want)
        assert _differs(_mask_with_a_slip(w, pc, pf, off, le=True), want), shape
    for n_inner in (8, 6):
        w, pc, pf, off = cases.mask_case(tw, tp, 6, 2, n_inner, extrapolate, w_repeat=3)
        want = C.mask_weights(w, pc, pf, off, w_repeat=3)
        assert _differs(_mask_with_a_slip(w, pc, pf, off, batch_for_slice=True)[1], want[1])  # batch 1 must read slice 0
    for ny, nx, f in cases.COARSE_SHAPES:  # plain and quad kernel
        w, pc, pf, off = cases.coarse_mask_case(tw, tp, 2, 3, ny, nx, f, extrapolate)
        want = C.mask_weights_coarse(w, pc, pf, off, f)
        up = C.upsample_onto(pc, ny, nx, f)
        assert _differs(_mask_with_a_slip(w, up, pf, off, le=True), want), (ny, nx, f)
        x = np.arange(nx)
        first_of_quad = (x - x % 4) // f  # ``l0`` for ``l1``: every column of a quad compares the quad's first coarse column
        if nx % 4 == 0 and f >= 4 and (first_of_quad != x // f).any():
            assert (ny, nx, f) in ((12, 12, 6), (10, 20, 5))
            slipped = np.take(np.take(pc, np.arange(ny) // f, axis=-2), first_of_quad, axis=-1)
            assert _differs(_mask_with_a_slip(w, slipped, pf, off), want), (ny, nx, f)
        w, pc, pf, off = cases.coarse_mask_case(tw, tp, 4, 3, ny, nx, f, extrapolate, w_repeat=2)
        want = C.mask_weights_coarse(w, pc, pf, off, f, w_repeat=2)
        slipped = _mask_with_a_slip(w, C.upsample_onto(pc, ny, nx, f), pf, off, batch_for_slice=True)
        assert _differs(slipped[1], want[1]), (ny, nx, f)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_blend_cases_tell_a_non_strict_comparison_apart(dtype):
    """``p >= pb`` gives (ps - pb) / (ps - pb) = 1 on an ordinary tie as well: only a tie under ``ps == pb``, an infinite or a
    NaN ``ps`` shows it.  Every case with at least 255 columns holds one."""
    for nz in cases.NZS:
        for shape, z_axis in cases.layouts(nz):
            pb, ps, p = cases.blend_case(dtype, shape, z_axis)
            with np.errstate(all="ignore"):
                e = lambda a: np.expand_dims(a, z_axis)
                slipped = np.where(p >= e(pb), (e(ps) - p) / (e(ps) - e(pb)), dtype(1))
            if pb.size >= 255:
                assert _differs(slipped, C.blend_weights(pb, ps, p, z_axis)), shape
