"""The nine small column kernels of csrc/vertical.hip that both restart pipelines run around the remap, each compared directly
with a plain numpy reference (tests/column_np.py, pinned on the host by tests/test_host_columns.py) on the inputs of
tests/column_cases.py: a compared pressure ON the surface pressure and one float next to it, NaN, +-inf and +-0 in every
operand, all four (weights, pressure) dtype pairs on all four mask kernels, quads that straddle two coarse columns,
``w_repeat > 1``, operands off their 16-byte alignment, ``n_batch * nz`` on both sides of the grid's row limit, column counts
around one 256-thread block and past the 16384-block cap of the grid-stride loops.

Bit for bit (dtype, shape, NaN places, sign of zero) except for the two kernels that call ``log``.  Those are held to the
float64-log references inside a derived bound: with ``lp`` the float64 logs of the interfaces accumulated in the kernel's
dtype and ``d = lp[k + 1] - lp[k]``, the relative error of a result is at most
``eps * (3 * (|lp[k]| + |lp[k + 1]|) / |d| + R)`` -- 3 ulps for ``log`` (the OpenCL full-profile requirement, which the ROCm
device library is written to; the ROCm installation ships no accuracy table of the math functions that could state a tighter
figure, and 3 would be kept if one did) and R other roundings, 2 for the midpoint pressure and 4 for DZ.  A level whose bound
exceeds 0.5 is skipped: none for delp in U(300, 1500), 0.98 % of the layers of U(1, 50) Pa on 9e4 Pa.

The tests past the block cap call the entry points themselves on outputs filled with NaN beforehand (their references hold no
NaN there), so that a cell a kernel did not write cannot pass for a right one.

Worst observed error / bound:
  numpy on the host (tests/test_host_columns.py): midpoint float32 0.161, thin layers 0.122; DZ float32 0.162, thin 0.122;
  float64 0 (numpy's float64 log is the reference's own).
  MI355X (this module): midpoint float32 0.268, thin layers 0.284, float64 0.165, thin 0.117; DZ float32 0.267, thin 0.265,
  float64 0.163, thin 0.117; past the block cap (float32) midpoint 0.234, DZ 0.232.
The bound tests print their figures (run with -s).  A ratio above 1 is a failure to explain, not a bound to widen."""
import numpy as np
import pytest
import torch

import column_cases as cases
import column_np as C
from glue_np import assert_same_bits as same_bits

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PAIRS = {"ff": (F32, F32), "fd": (F32, F64), "df": (F64, F32), "dd": (F64, F64)}


def _to(device, x):
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x if x.flags.writeable else x.copy()).to(device)  # (the shared read-only inputs: torch wants a writable one)


def _np(t):
    return t.cpu().numpy()


def _nan_filled(device, shape, dtype):
    """An output that shows which cells a kernel wrote: NaN everywhere (for references that hold no NaN)."""
    return torch.full(shape, float("nan"), dtype=dtype, device=device)


def _no_nan(want, tail_only=False):
    """``want`` once it is sure that it holds no NaN -- ``tail_only``: none past the cells that 16384 blocks of 256 cover."""
    assert not np.isnan(want.reshape(-1)[256 * 64 * 256:] if tail_only else want).any()
    return want


def _raw(device, name, *args):
    """An entry point of the library itself on the current stream (the caller owns the output)."""
    from fv3net_amd import _lib, ops

    ops._require_device(torch.empty(1, device=device))  # (initialises the library on the device once)
    _lib.call_on(device, name, *args, ops._stream(device))


def _off_alignment(device, x):
    """``x`` as a contiguous view one element into a larger device buffer: its pointer is not on 16 bytes."""
    x = np.ascontiguousarray(x)
    buf = torch.empty(x.size + 1, dtype=torch.from_numpy(x).dtype, device=device)
    view = buf[1:].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.is_contiguous() and view.data_ptr() % 16 != 0 and buf.data_ptr() % 16 == 0
    return view


# ------------------------------------------------------------------------------------------------
# pressure_at_interface, column_sum
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", cases.NZS)
@pytest.mark.parametrize("dtype", [F32, F64])
def test_pressure_at_interface_and_column_sum(device, dtype, nz):
    """Every layout and column count, a NaN and an infinity at a middle level: the sequential sums, bit for bit."""
    from fv3net_amd import ops

    for shape, z_axis in cases.layouts(nz):
        delp = cases.column_fields(dtype, shape, z_axis)["delp"]
        d = _to(device, delp)
        got = _np(ops.pressure_at_interface(d, cases.TOA, z_axis))
        same_bits(got, C.pressure_at_interface(delp, cases.TOA, z_axis), err_msg=f"{shape}")
        if int(np.prod(shape)) // nz >= 3:
            cols = cases.as_columns(got, z_axis)
            assert np.isnan(cols[nz // 2 + 1:, cases.NAN_COLUMN]).all() and np.isnan(cols).sum() == nz - nz // 2
        for addend in (0.0, 300.0):
            same_bits(_np(ops.column_sum(d, z_axis, addend)), C.column_sum(delp, z_axis, addend), err_msg=f"{shape} + {addend}")


@pytest.mark.parametrize("dtype", [F32, F64])
def test_columns_without_levels_and_empty_extents(device, dtype):
    from fv3net_amd import ops

    tdt = torch.from_numpy(np.zeros(1, dtype)).dtype
    empty = torch.empty((3, 0, 5), dtype=tdt, device=device)
    same_bits(_np(ops.pressure_at_interface(empty, cases.TOA, 1)), np.full((3, 1, 5), cases.TOA, dtype))
    same_bits(_np(ops.column_sum(empty, 1, 300.0)), np.full((3, 5), 300.0, dtype))
    same_bits(_np(ops.column_sum(empty, 1)), np.zeros((3, 5), dtype))
    for shape in ((0, 4, 5), (3, 4, 0)):
        x = torch.empty(shape, dtype=tdt, device=device)
        assert tuple(ops.pressure_at_interface(x, cases.TOA, 1).shape) == (shape[0], 5, shape[2])
        assert tuple(ops.column_sum(x, 1, 300.0).shape) == (shape[0], shape[2])
        assert tuple(ops.pressure_at_midpoint_log(x, cases.TOA, 1).shape) == shape
    # hydrostatic balance without levels: phis = g * (phis / g), an empty DZ
    phis = np.array([[0.0, 1234.5, 3e4, -0.0, np.nan]], dtype)
    dz, phis_out = ops.hydrostatic_balance(*([torch.empty((1, 0, 5), dtype=tdt, device=device)] + [_to(device, phis)]
                                             + [torch.empty((1, 0, 5), dtype=tdt, device=device)] * 3), cases.TOA, 1)
    assert tuple(dz.shape) == (1, 0, 5)
    same_bits(_np(phis_out), C.hydrostatic_phis(np.zeros((1, 0, 5), dtype), phis, np.zeros((1, 0, 5), dtype), dtype, 1))
    same_bits(_np(phis_out)[0, :3], dtype(C.GRAVITY) * (phis[0, :3] / dtype(C.GRAVITY)))


def test_interface_and_sum_past_the_block_cap(device):
    """4194561 columns: more than the 16384 blocks of 256 threads that one pass of the grid-stride loop holds."""
    from fv3net_amd import ops

    delp = cases.past_the_cap_delp()
    d = _to(device, delp)
    nb, nz, ni = delp.shape
    out = _nan_filled(device, (nb, nz + 1, ni), d.dtype)
    _raw(device, "fv3hip_pressure_at_interface", ops._ptr(d), ops._float_code(d), nb, nz, ni, cases.TOA, ops._ptr(out))
    same_bits(_np(out), _no_nan(C.pressure_at_interface(delp, cases.TOA, 1)))
    for addend in (0.0, 300.0):
        out = _nan_filled(device, (nb, ni), d.dtype)
        _raw(device, "fv3hip_column_sum", ops._ptr(d), ops._float_code(d), nb, nz, ni, addend, ops._ptr(out))
        same_bits(_np(out), _no_nan(C.column_sum(delp, 1, addend)))


# ------------------------------------------------------------------------------------------------
# mask_weights, fine route
# ------------------------------------------------------------------------------------------------
def _mask_raw(device, w, pc, pf, off, w_repeat):
    """fv3hip_mask_weights itself on device tensors [n_batch / w_repeat, n_inner], [n_batch, cmp_levels, n_inner],
    [n_batch, nz + 1, n_inner], into an output filled with NaN."""
    from fv3net_amd import _lib, ops

    ops._require_device(w, pc, pf)
    n_batch, nz, n_inner = int(pf.shape[0]), int(pf.shape[1]) - 1, int(pf.shape[2])
    out = _nan_filled(device, (n_batch, nz, n_inner), w.dtype)
    _lib.call_on(device, "fv3hip_mask_weights", ops._ptr(w), ops._float_code(w), ops._ptr(pc), int(pc.shape[1]), off, ops._ptr(pf),
                 ops._float_code(pf), n_batch, nz, n_inner, w_repeat, ops._ptr(out), ops._stream(device))
    return out


def _mask_coarse_raw(device, w, pc, pf, off, f, w_repeat):
    """fv3hip_mask_weights_coarse itself: it raises on EUNSUPPORTED where ops.mask_weights would fall back."""
    from fv3net_amd import _lib, ops

    ops._require_device(w, pc, pf)
    n_batch, nz, ny, nx = int(pf.shape[0]), int(pf.shape[1]) - 1, int(pf.shape[2]), int(pf.shape[3])
    out = torch.empty((n_batch, nz, ny, nx), dtype=w.dtype, device=device)
    _lib.call_on(device, "fv3hip_mask_weights_coarse", ops._ptr(w), ops._float_code(w), ops._ptr(pc), int(pc.shape[1]), off,
                 ops._ptr(pf), ops._float_code(pf), n_batch, nz, ny, nx, f, w_repeat, ops._ptr(out), ops._stream(device))
    return out


@pytest.mark.parametrize("extrapolate", [False, True])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_mask_weights_specials_on_the_generic_and_the_rows_kernel(device, pair, extrapolate):
    """Every (level, surface pressure, weight) triple of the specials, in each dtype pair and both modes, at row lengths of
    the generic kernel (1, 3, 1030) and of the rows kernel (4, 1020, 1024, 1028), with nz = 3 and nz = 1."""
    from fv3net_amd import ops

    tw, tp = PAIRS[pair]
    for n_batch, nz, n_inner in cases.MASK_TABLE_SHAPES:
        w, pc, pf, off = cases.mask_case(tw, tp, n_batch, nz, n_inner, extrapolate)
        got = ops.mask_weights(_to(device, w), _to(device, pc), _to(device, pf), 1, extrapolate=extrapolate)
        same_bits(_np(got), C.mask_weights(w, pc, pf, off), err_msg=f"{(n_batch, nz, n_inner)}")


@pytest.mark.parametrize("pair", list(PAIRS))
def test_mask_weights_z_first_and_last(device, pair):
    """The wrapper's other two layouts: z first (one batch) and z last (one column per batch)."""
    from fv3net_amd import ops

    tw, tp = PAIRS[pair]
    for extrapolate in (False, True):
        w, pc, pf, off = cases.mask_case(tw, tp, 1, 3, 80, extrapolate)        # z first: [z, columns]
        got = ops.mask_weights(_to(device, w[0]), _to(device, pc[0]), _to(device, pf[0]), 0, extrapolate=extrapolate)
        same_bits(_np(got), C.mask_weights(w, pc, pf, off)[0])
        w, pc, pf, off = cases.mask_case(tw, tp, 80, 3, 1, extrapolate)        # z last: [columns, z]
        got = ops.mask_weights(_to(device, w[:, 0]), _to(device, pc[:, :, 0]), _to(device, pf[:, :, 0]), 1, extrapolate=extrapolate)
        same_bits(_np(got), C.mask_weights(w, pc, pf, off)[:, :, 0])


@pytest.mark.parametrize("pair", list(PAIRS))
def test_mask_weights_operands_off_their_alignment(device, pair):
    """Rows of whole quads whose weights, compared pressures or fine pressures start one element into a buffer: the rows
    kernel's 16-byte accesses do not apply, the dispatch takes the generic kernel, the result is the same."""
    from fv3net_amd import ops

    tw, tp = PAIRS[pair]
    for n_inner in cases.ROWS_INNER:
        n_batch = max(2, -(-cases.n_special_columns(3) // n_inner))
        w, pc, pf, off = cases.mask_case(tw, tp, n_batch, 3, n_inner, False)
        want = C.mask_weights(w, pc, pf, off)
        for which in range(3):
            ops_in = [_off_alignment(device, x) if i == which else _to(device, x) for i, x in enumerate((w, pc, pf))]
            same_bits(_np(ops.mask_weights(*ops_in, 1)), want, err_msg=f"n_inner={n_inner}, operand {which} off alignment")


@pytest.mark.parametrize("rows", [65535, 65536])
def test_mask_weights_at_the_grid_row_limit(device, rows):
    """n_batch * nz = 65535 is the last size of the rows grid, 65536 the first of the generic kernel."""
    from fv3net_amd import ops

    nz = 3 if rows % 3 == 0 else 4
    assert rows % nz == 0
    for pair in ("ff", "dd"):
        tw, tp = PAIRS[pair]
        w, pc, pf, off = cases.mask_case(tw, tp, rows // nz, nz, 4, False)
        got = ops.mask_weights(_to(device, w), _to(device, pc), _to(device, pf), 1)
        same_bits(_np(got), C.mask_weights(w, pc, pf, off))


def test_mask_weights_generic_kernel_past_the_block_cap(device):
    n_batch, nz, n_inner = cases.PAST_THE_CAP_MASK_SHAPE
    w, pc, pf, off = cases.mask_case(F32, F32, n_batch, nz, n_inner, False)
    got = _mask_raw(device, _to(device, w), _to(device, pc), _to(device, pf), off, 1)
    same_bits(_np(got), _no_nan(C.mask_weights(w, pc, pf, off), tail_only=True))


@pytest.mark.parametrize("n_inner", [8, 6])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_mask_weights_shared_weight_slices(device, pair, n_inner):
    """``w_repeat = 3`` on 6 batches through the entry point itself: batch b reads weight slice b // 3, on the rows kernel
    (n_inner = 8) and on the generic one (n_inner = 6)."""
    tw, tp = PAIRS[pair]
    for extrapolate in (False, True):
        w, pc, pf, off = cases.mask_case(tw, tp, 6, 2, n_inner, extrapolate, w_repeat=3)
        assert w.shape == (2, n_inner)
        got = _mask_raw(device, _to(device, w), _to(device, pc), _to(device, pf), off, 3)
        same_bits(_np(got), C.mask_weights(w, pc, pf, off, w_repeat=3))


# ------------------------------------------------------------------------------------------------
# mask_weights, coarse route
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extrapolate", [False, True])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_mask_weights_coarse_specials(device, pair, extrapolate):
    """The compared pressures on their own coarser grid against the upsampled reference: the plain kernel (factor < 4, a
    staggered x), quads inside one coarse column and across two at every offset, over two workgroups, under a staggered y --
    with ties and NaNs on either side of the coarse columns' edges -- then the same with weights or fine pressures off their
    alignment (the plain kernel again), and with shared weight slices through the entry point itself."""
    from fv3net_amd import ops

    tw, tp = PAIRS[pair]
    for ny, nx, f in cases.COARSE_SHAPES:
        w, pc, pf, off = cases.coarse_mask_case(tw, tp, 2, 3, ny, nx, f, extrapolate)
        want = C.mask_weights_coarse(w, pc, pf, off, f)
        d_w, d_pc, d_pf = _to(device, w), _to(device, pc), _to(device, pf)
        got = ops.mask_weights(d_w, d_pc, d_pf, 1, extrapolate=extrapolate, coarse_factor=f)
        same_bits(_np(got), want, err_msg=f"{(ny, nx, f)}")
        same_bits(_np(_mask_coarse_raw(device, d_w, d_pc, d_pf, off, f, 1)), want, err_msg=f"{(ny, nx, f)} raw")
        for which, name in ((0, "weights"), (2, "p_fine")):
            ops_in = [_off_alignment(device, x) if i == which else t for i, (x, t) in enumerate(zip((w, pc, pf), (d_w, d_pc, d_pf)))]
            got = ops.mask_weights(*ops_in, 1, extrapolate=extrapolate, coarse_factor=f)
            same_bits(_np(got), want, err_msg=f"{(ny, nx, f)} {name} off alignment")
        w2, pc2, pf2, off = cases.coarse_mask_case(tw, tp, 4, 3, ny, nx, f, extrapolate, w_repeat=2)
        assert w2.shape == (2, ny, nx)
        got = _mask_coarse_raw(device, _to(device, w2), _to(device, pc2), _to(device, pf2), off, f, 2)
        same_bits(_np(got), C.mask_weights_coarse(w2, pc2, pf2, off, f, w_repeat=2), err_msg=f"{(ny, nx, f)} w_repeat=2")


def test_mask_weights_coarse_past_the_grid_row_limit(device):
    """n_batch * nz = 65536: the entry point reports EUNSUPPORTED, the wrapper upsamples and takes the fine route."""
    from fv3net_amd import _lib, ops

    n_batch, nz, ny, nx, f = 16384, 4, 4, 4, 2
    w, pc, pf, off = cases.coarse_mask_case(F32, F32, n_batch, nz, ny, nx, f, False)
    d_w, d_pc, d_pf = _to(device, w), _to(device, pc), _to(device, pf)
    with pytest.raises(_lib.Fv3HipError) as err:
        _mask_coarse_raw(device, d_w, d_pc, d_pf, off, f, 1)
    assert err.value.code == _lib.EUNSUPPORTED
    got = ops.mask_weights(d_w, d_pc, d_pf, 1, coarse_factor=f)
    same_bits(_np(got), C.mask_weights_coarse(w, pc, pf, off, f))


# ------------------------------------------------------------------------------------------------
# blend_weights
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", cases.NZS)
@pytest.mark.parametrize("dtype", [F32, F64])
def test_blend_weights_specials(device, dtype, nz):
    """One subtraction pair and one division (the library is built with contraction off): bit for bit, with ``p`` on ``pb``
    and next to it, zero numerators and denominators, NaN and +-inf in each operand."""
    from fv3net_amd import ops

    for shape, z_axis in cases.layouts(nz):
        pb, ps, p = cases.blend_case(dtype, shape, z_axis)
        got = ops.blend_weights(_to(device, pb), _to(device, ps), _to(device, p), z_axis)
        same_bits(_np(got), C.blend_weights(pb, ps, p, z_axis), err_msg=f"{shape}")


def test_blend_weights_past_the_block_cap(device):
    from fv3net_amd import ops

    pb, ps, p = cases.blend_case(F32, cases.PAST_THE_CAP_TOTAL_SHAPE, 1)
    d_pb, d_ps, d_p = _to(device, pb), _to(device, ps), _to(device, p)
    out = _nan_filled(device, p.shape, d_p.dtype)
    _raw(device, "fv3hip_blend_weights", ops._ptr(d_pb), ops._ptr(d_ps), ops._ptr(d_p), ops._float_code(d_p), *p.shape, ops._ptr(out))
    same_bits(_np(out), _no_nan(C.blend_weights(pb, ps, p, 1), tail_only=True))


# ------------------------------------------------------------------------------------------------
# pressure_at_midpoint_log, hydrostatic_balance
# ------------------------------------------------------------------------------------------------
def _hydrostatic(device, f, z_axis):
    from fv3net_amd import ops

    dz, phis = ops.hydrostatic_balance(*(_to(device, f[k]) for k in ("dz", "phis", "t", "q", "delp")), cases.TOA, z_axis)
    return _np(dz), _np(phis)


def test_midpoint_log_and_hydrostatic_dz_inside_the_derived_bound(device):
    """Both dtypes, every layout and size, ordinary and thin layers, a NaN and an infinite layer: the NaN patterns of the
    float64-log references, their infinities, and every finite result inside the bound (module docstring).  phis is the
    kernel's two sequential sums of its own DZ, bit for bit."""
    from fv3net_amd import ops

    mid, dzt = C.Tally(), C.Tally()
    for dtype in (F32, F64):
        for thin in (False, True):
            key = f"{np.dtype(dtype).name}{' thin' if thin else ''}"
            for nz in cases.NZS:
                for shape, z_axis in cases.layouts(nz):
                    f = cases.column_fields(dtype, shape, z_axis, thin=thin)
                    got = _np(ops.pressure_at_midpoint_log(_to(device, f["delp"]), cases.TOA, z_axis))
                    assert got.dtype == dtype and got.shape == shape
                    mid.add(key, got, *C.pressure_at_midpoint_log_f64(f["delp"], cases.TOA, z_axis))
                    dz, phis = _hydrostatic(device, f, z_axis)
                    assert dz.dtype == dtype and dz.shape == shape
                    dzt.add(key, dz, *C.hydrostatic_dz_f64(f["t"], f["q"], f["delp"], cases.TOA, z_axis))
                    same_bits(phis, C.hydrostatic_phis(f["dz"], f["phis"], dz, dtype, z_axis), err_msg=f"phis {key} {shape}")
                    if int(np.prod(shape)) // nz >= 3:   # the NaN layer and those below it
                        cols = cases.as_columns(got, z_axis)
                        assert np.isnan(cols[nz // 2:, cases.NAN_COLUMN]).all() and np.isfinite(cols[:nz // 2, cases.NAN_COLUMN]).all()
    mid.check("pressure_at_midpoint_log, device:")
    dzt.check("hydrostatic DZ, device:")


def test_log_kernels_past_the_block_cap(device):
    from fv3net_amd import ops

    delp = cases.past_the_cap_delp()
    d = _to(device, delp)
    nb, nz, ni = delp.shape
    code = ops._float_code(d)
    out = _nan_filled(device, delp.shape, d.dtype)
    _raw(device, "fv3hip_pressure_at_midpoint_log", ops._ptr(d), code, nb, nz, ni, cases.TOA, ops._ptr(out))
    tally = C.Tally()   # (error_over_bound holds the result to the reference's NaN pattern: none)
    tally.add("float32", _np(out), *C.pressure_at_midpoint_log_f64(delp, cases.TOA, 1))
    tally.check("pressure_at_midpoint_log past the cap, device:")
    zeros, t, phis_in = torch.zeros_like(d), torch.full_like(d, 250.0), torch.zeros((nb, ni), dtype=d.dtype, device=device)
    dz, phis = _nan_filled(device, delp.shape, d.dtype), _nan_filled(device, (nb, ni), d.dtype)
    _raw(device, "fv3hip_hydrostatic_balance", ops._ptr(zeros), ops._ptr(phis_in), ops._ptr(t), ops._ptr(zeros), ops._ptr(d), code,
         nb, nz, ni, cases.TOA, ops._ptr(dz), ops._ptr(phis))
    dz = _np(dz)
    tally = C.Tally()
    tally.add("float32", dz, *C.hydrostatic_dz_f64(np.full_like(delp, 250.0), np.zeros_like(delp), delp, cases.TOA, 1))
    tally.check("hydrostatic DZ past the cap, device:")
    same_bits(_np(phis), _no_nan(C.hydrostatic_phis(np.zeros_like(delp), np.zeros((nb, ni), F32), dz, F32, 1)))


def test_virtual_temperature_constant_is_the_references(device):
    """``Rv / Rd - 1`` rounded once from float64, as numpy rounds the reference's Python float -- not the quotient of the
    float32 constants, two float32 steps higher.  Column pairs share their delp; the second column of a pair carries the
    first one's virtual temperature, computed by numpy with the reference's constant, as its temperature and no humidity.  A
    kernel with the reference's constant gives both the same DZ, bit for bit; with the float32 quotient, as the kernel had it
    before, 966 of the 1000 pairs of the first range (q in U(0, 1); a pair differs if one of its 8 levels does) differed on an
    MI355X."""
    n_seen = 0
    for q_max in cases.CONSTANT_Q_MAX:
        t, q, delp, n_differ = cases.virtual_constant_pairs(cases.CONSTANT_PAIRS, cases.CONSTANT_NZ, q_max)
        assert t.shape == (8, 2000) and t.dtype == F32
        n_seen += n_differ
        f = dict(t=t, q=q, delp=delp, dz=np.full_like(t, -100.0), phis=np.zeros(t.shape[1], F32))
        dz, _ = _hydrostatic(device, f, 0)
        bad = (dz[:, 0::2] != dz[:, 1::2]).any(axis=0)
        assert np.isfinite(dz).all()
        assert not bad.any(), f"q in U(0, {q_max}): {int(bad.sum())} of {bad.size} pairs differ"
    assert n_seen >= 100, n_seen   # (pairs in which the two candidate constants give different virtual temperatures)
