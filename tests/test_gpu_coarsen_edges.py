"""The kernels of csrc/coarsen.hip that the restart pipelines reach only through longer routes, each compared directly with a
plain numpy reference (tests/coarsen_edge_np.py and oracle/coarsen_np.py, pinned on the host by
tests/test_host_coarsen_edges.py) on the inputs of tests/coarsen_edge_cases.py: ``cast`` / ``cast_many``, the boundary vectors
of the cube faces and the halo pick, the centre-to-edge lines, ``repeat`` / ``block_upsample`` on both sides of the row
kernel's dispatch rule, the window average outside its fast path and the strided reductions.

Word copies and conversions are compared through integer views; the centre-to-edge lines and the reductions of small
integers bit for bit.  The weighted means have a derived gate, none measured: with ``n = by * bx``, ``u_P`` the unit
roundoff of the promoted type and ``u_W`` that of the weights' type,

    |got - want| <= 2 n u_P sum|obj w| / sum(w) + (2 n u_W + 2 u_P) |want|

(a numerator of n once-rounded products summed in any order, a denominator of n weights summed in the weights' own type, one
division; ``want`` from the float64 restatement).  A non-finite ``want`` must be met exactly.  Every test of a mean prints
its worst fraction of the gate.

Which test runs which instantiation (float32 / int32 are the 4-byte words, float64 / int64 the 8-byte ones):
  cast_kernel<Tin, Tout>, the six non-identity pairs      test_cast_rounds_like_astype[Tin-Tout]
    (<float, float> and <double, double> are never launched by ``ops.cast``: test_cast_to_the_same_dtype_is_the_tensor_itself)
  cast_many_kernel<float>, <double>                       test_cast_many_converts_every_entry, test_cast_many_writes_only_its_segments
  cube_edge_rows_kernel, halo_pick_kernel <u32>, <u64>    test_boundary_vectors_and_halo_pick_copy_words[shape-dtype]
  interp_to_outer_kernel<float>, <double>                 test_interp_tiles_to_edges_is_the_sliced_oracle, test_interp_lines_on_a_rectangle_with_explicit_halos
  upsample_kernel<u32>, <u64>                             test_repeat_on_both_sides_of_the_row_kernel (nx_out 252, 259; 258 for u32), test_block_upsample_staggered_dims
  upsample_rows_kernel<u32, 4>, <u64, 2>                  the same two tests (nx_out 256, 260, 1028, 1036; 258 for u64); <u32, 4> also test_repeat_past_65535_rows
  wavg_generic_kernel, the four (obj, weights) pairs      test_window_average_outside_the_fast_path, test_block_average_fallback_conditions
  wavg_block_kernel, four pairs x F in {2, 4, 8, 16, 32}  test_block_average_fast_path_under_the_same_gate
  block_reduce_kernel<T>, four types                      test_take_lines, test_block_reduce_over_strided_windows (sum / mean / min / max; all ops at (9, 8))
  block_rank_wave_kernel<T>, four types                   test_block_reduce_over_strided_windows (median / mode below 65 values)
The inputs that tell the likely slips apart: a missing flip -- every cube shape with n >= 2 (random words; n = 1 cannot); an
index off by one at the last edge -- step 12 of n = 12 and step 8 of nx = 8, where the outputs are the two halo edges alone,
with NaN / inf planted in the last halo cell; a dropped 49th table entry -- 49 and 97 entries to convert; a 16-byte group that
reads the wrong input cell -- (nx_in, fx) = (86, 3) on 8-byte words, (52, 5), (148, 7); a halfway case rounded away from
even -- 2^24 + 1, 2^40 + 2^16, 2^53 + 1, 1 + 2^-24 and 1.5 * 2^-149 in ``conversion_values``."""
import ctypes

import numpy as np
import pytest
import torch

import coarsen_edge_cases as cases
import coarsen_edge_np as E
from oracle import coarsen_np

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64
_TORCH = {np.dtype(F32): torch.float32, np.dtype(F64): torch.float64, np.dtype(I32): torch.int32, np.dtype(I64): torch.int64}
_name = lambda d: np.dtype(d).name


def _to(device, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------
# cast_kernel: 4 input types x 2 output types
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dtype, out_dtype", cases.CAST_PAIRS, ids=lambda d: _name(d))
def test_cast_rounds_like_astype(device, in_dtype, out_dtype):
    """Ties to even, overflow to infinity, float32 subnormals, the sign of a zero: every word equals ``astype``'s outside
    NaN, at sizes around one block and past the 16384-block cap of the grid-stride loop."""
    from fv3net_amd import ops

    for size in cases.CAST_SIZES:
        x = cases.conversion_input(in_dtype, size)
        got = ops.cast(_to(device, x), _TORCH[np.dtype(out_dtype)])
        assert got.shape == (size,) and got.is_cuda
        E.assert_same_outside_nan(_np(got), E.cast_np(x, out_dtype), err_msg=f"size {size}")
    # a transposed view converts in logical order
    x = cases.conversion_input(in_dtype, 6 * 50).reshape(6, 50)
    t = _to(device, x).t()
    assert not t.is_contiguous()
    E.assert_same_outside_nan(_np(ops.cast(t, _TORCH[np.dtype(out_dtype)])), E.cast_np(x.T, out_dtype), err_msg="transposed")


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
def test_cast_to_the_same_dtype_is_the_tensor_itself(device, dtype):
    from fv3net_amd import ops

    t = _to(device, cases.conversion_input(dtype, 7))
    assert ops.cast(t, t.dtype) is t
    assert ops.cast_many([t, t], t.dtype)[0] is t


# ------------------------------------------------------------------------------------------------
# cast_many_kernel: 2 output types, tables of 48
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("count", cases.CAST_MANY_COUNTS)
def test_cast_many_converts_every_entry(device, count, out_dtype):
    """2, 48, 49 and 97 tensors to convert against a table of 48 (one launch; one full; 48 + 1; 48 + 48 + 1), tensors already
    converted between them: mixed input types, one empty tensor, and from 48 up one long tensor whose table neighbours are
    short."""
    from fv3net_amd import ops

    arrays = cases.cast_many_tensors(count, out_dtype)
    tensors = [_to(device, a) for a in arrays]
    got = ops.cast_many(tensors, _TORCH[np.dtype(out_dtype)])
    assert len(got) == len(tensors) == count + count // 7
    for k, (a, t, g) in enumerate(zip(arrays, tensors, got)):
        if a.dtype == np.dtype(out_dtype):
            assert g is t, k
        else:
            E.assert_same_outside_nan(_np(g), E.cast_np(a, out_dtype), err_msg=f"entry {k} of {count}")


@pytest.mark.parametrize("out_dtype", [F32, F64], ids=_name)
def test_cast_many_writes_only_its_segments(device, out_dtype):
    """``fv3hip_cast_many`` called the way ``ops.cast_many`` calls it, 97 entries (tables of 48, 48 and 1), the outputs
    consecutive segments of one buffer of sentinels with gaps of three elements between them: every segment converted, every
    gap and the tail untouched."""
    from fv3net_amd import _lib, ops

    arrays = [a for a in cases.cast_many_tensors(97, out_dtype) if a.dtype != np.dtype(out_dtype)]
    assert len(arrays) == 97 and any(a.size == 0 for a in arrays)
    src = [_to(device, a) for a in arrays]
    gap, sentinel = 3, -12345.0
    starts, pos = [], gap
    for a in arrays:
        starts.append(pos)
        pos += a.size + gap
    buf = torch.full((pos + 64,), sentinel, dtype=_TORCH[np.dtype(out_dtype)], device=device)
    dst = [buf[s:s + a.size] for s, a in zip(starts, arrays)]
    n = len(src)
    _lib.call_on(device, "fv3hip_cast_many", (ctypes.c_void_p * n)(*[t.data_ptr() for t in src]),
                 (ctypes.c_int * n)(*[ops._CAST_IN[t.dtype] for t in src]), (ctypes.c_void_p * n)(*[t.data_ptr() for t in dst]),
                 ops._CAST_IN[buf.dtype], (ctypes.c_int64 * n)(*[t.numel() for t in src]), n, ops._stream(device))
    out = _np(buf)
    untouched = np.ones(out.size, bool)
    for k, (s, a) in enumerate(zip(starts, arrays)):
        E.assert_same_outside_nan(out[s:s + a.size], E.cast_np(a, out_dtype), err_msg=f"entry {k}")
        untouched[s:s + a.size] = False
    assert untouched.sum() == gap * (n + 1) + 64
    E.assert_same_words(out[untouched], np.full(int(untouched.sum()), sentinel, out_dtype))


# ------------------------------------------------------------------------------------------------
# cube_edge_rows_kernel, halo_pick_kernel: 4- and 8-byte words
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.WORD_DTYPES, ids=_name)
@pytest.mark.parametrize("shape", cases.CUBE_SHAPES, ids=str)
def test_boundary_vectors_and_halo_pick_copy_words(device, shape, dtype):
    """No, one and two middle dims, n = 1, 2, 12, all six tiles, subsets and a list out of order, both axes: NaN payloads
    and -0.0 survive, and the device pick equals the array indexing of the CPU branch."""
    from fv3net_amd import ops
    from fv3net_amd.cubedsphere.grid import halos_from_rows

    a = cases.words(shape, dtype)
    rows = ops.cube_edge_rows(_to(device, a))
    want_rows = E.edge_rows_np(a)
    E.assert_same_words(_np(rows), want_rows)
    rows_cpu = rows.cpu()
    for tiles in cases.TILE_LISTS:
        for axis in ("x", "y"):
            lo, hi = halos_from_rows(rows, tiles, axis)
            assert lo.is_cuda and hi.is_cuda
            want_lo, want_hi = E.halo_pick_np(want_rows, tiles, axis)
            cpu_lo, cpu_hi = halos_from_rows(rows_cpu, tiles, axis)
            for got, want, cpu, side in ((lo, want_lo, cpu_lo, "lo"), (hi, want_hi, cpu_hi, "hi")):
                E.assert_same_words(_np(got), want, err_msg=f"{tiles} {axis} {side}")
                E.assert_same_words(_np(got), cpu.numpy(), err_msg=f"{tiles} {axis} {side} (CPU branch)")


def test_halo_pick_refuses_entries_the_kernel_would_index_with(device):
    from fv3net_amd import ops
    from fv3net_amd.cubedsphere.grid import halos_from_rows

    rows = ops.cube_edge_rows(_to(device, cases.words((6, 5, 12, 12), F32)))
    assert 2 * 6 * 5 * 12 > 256   # (the shape above: more than one block of the pick)
    with pytest.raises(ValueError):
        ops.halo_pick(rows, [0] * 14, [0] * 14, [0] * 14)       # seven local tiles
    with pytest.raises(ValueError):
        halos_from_rows(rows, [0, 1, 2, 3, 4, 5, 0], "x")
    with pytest.raises(ValueError):
        ops.halo_pick(rows, [1, 6], [0, 0], [0, 0])             # a neighbour index of 6
    with pytest.raises(ValueError):
        ops.halo_pick(rows, [1, -1], [0, 0], [0, 0])
    with pytest.raises(ValueError):
        ops.halo_pick(rows, [1, 2], [0, 4], [0, 0])             # a row index of 4
    with pytest.raises(ValueError):
        ops.halo_pick(rows[:3], [1, 3], [0, 0], [0, 0])         # a neighbour the table does not hold
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# interp_to_outer_kernel: float and double
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("n", [1, 12])
def test_interp_tiles_to_edges_is_the_sliced_oracle(device, n, axis, dtype):
    """Every step that divides n (at 12 both outputs are halo edges), values with NaN and +-inf among them: bit for bit."""
    from fv3net_amd.cubedsphere.grid import interp_tiles_to_edges

    a = cases.float_field((6, 5, n, n), dtype, seed=n)
    with np.errstate(invalid="ignore"):   # (inf + -inf among the planted values)
        want = coarsen_np.interp_center_to_outer(a, axis)
    t = _to(device, a)
    for step in [s for s in cases.INTERP_STEPS if n % s == 0]:
        got = _np(interp_tiles_to_edges(t, axis, step=step))
        E.assert_same_outside_nan(got, want[..., ::step] if axis == "x" else want[..., ::step, :], err_msg=f"step {step}")


@pytest.mark.parametrize("dtype", [F32, F64], ids=_name)
def test_interp_lines_on_a_rectangle_with_explicit_halos(device, dtype):
    """ny = 5, nx = 8 at every step that divides the axis length; NaN, +-inf and pairs whose sum overflows in interior and in
    halo cells; 360 outputs at step 1 along x.  The restatement makes the same two roundings."""
    from fv3net_amd import ops

    x, halos = cases.interp_rect(dtype)
    t = _to(device, x)
    for axis, steps in ((0, (1, 2, 4, 8)), (1, (1, 5))):
        lo, hi = halos[axis]
        for step in steps:
            got = _np(ops.interp_center_to_outer(t, _to(device, lo), _to(device, hi), axis, step=step))
            want = E.interp_lines_np(x, lo, hi, axis, step)
            E.assert_same_outside_nan(got, want, err_msg=f"axis {axis} step {step}")
            assert np.isinf(want).any() and np.isnan(want).any()
        for bad in ((3, 0) if axis == 0 else (2, 0)):
            with pytest.raises(ValueError):
                ops.interp_center_to_outer(t, _to(device, lo), _to(device, hi), axis, step=bad)
    assert x.size // 8 * 9 > 256


# ------------------------------------------------------------------------------------------------
# upsample_kernel, upsample_rows_kernel: 4- and 8-byte words
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.WORD_DTYPES, ids=_name)
def test_repeat_on_both_sides_of_the_row_kernel(device, dtype):
    """nx_out = 252, 256, 258, 260, 1028 (and 259, 1036 for fx = 7) with fx in {1, 2, 3, 5, 7}: 16-byte groups that span two
    or three input cells; fy != fx; the identity."""
    from fv3net_amd import ops

    for nx_in, fx in cases.REPEAT_X:
        a = cases.words((2, 3, nx_in), dtype, seed=fx)
        got = ops.repeat(_to(device, a), 2, fx)
        E.assert_same_words(_np(got), E.repeat_np(a, 2, fx), err_msg=f"nx_in {nx_in} fx {fx}")
    for fy, fx in cases.REPEAT_YX:
        for nx_in in (7, 52, 64, 260):
            a = cases.words((3, 2, 3, nx_in), dtype, seed=fy)
            E.assert_same_words(_np(ops.repeat(_to(device, a), fy, fx)), E.repeat_np(a, fy, fx), err_msg=f"nx_in {nx_in} ({fy}, {fx})")
    for shape in ((2, 3, 7), (2, 3, 256)):
        a = cases.words(shape, dtype)
        E.assert_same_words(_np(ops.repeat(_to(device, a), 1, 1)), a)
        E.assert_same_words(_np(ops.block_upsample(_to(device, a), 1)), a)


@pytest.mark.parametrize("dtype", cases.WORD_DTYPES, ids=_name)
def test_block_upsample_staggered_dims(device, dtype):
    """A staggered ny on the row kernel (5 x 128, f = 2 -> 9 x 256), a staggered nx (129 -> 257: the scalar kernel), both,
    and even sizes of both kernels, against the oracle and -- where no dim is staggered -- the repeat."""
    from fv3net_amd import ops

    for shape, f in (((2, 5, 128), 2), ((2, 4, 129), 2), ((2, 5, 129), 2), ((2, 4, 128), 2), ((2, 4, 86), 3), ((3, 5, 87), 3),
                     ((2, 2, 4, 52), 5), ((2, 3, 7), 2)):
        a = cases.words(shape, dtype, seed=f)
        got = _np(ops.block_upsample(_to(device, a), f))
        E.assert_same_words(got, coarsen_np.block_upsample(a, f), err_msg=f"{shape} f {f}")
        if shape[-1] % 2 == 0 and shape[-2] % 2 == 0:
            E.assert_same_words(got, E.repeat_np(a, f, f), err_msg=f"{shape} f {f}")


def test_repeat_past_65535_rows(device):
    """65540 output rows of 256 on the row kernel, whose grid holds 65535 rows: the whole array."""
    from fv3net_amd import ops

    a = cases.words((2, 16385, 128), F32)
    got = _np(ops.repeat(_to(device, a), 2, 2))
    assert got.shape == (2, 32770, 256)
    E.assert_same_words(got, E.repeat_np(a, 2, 2))


# ------------------------------------------------------------------------------------------------
# wavg_generic_kernel (and once wavg_block_kernel): the four (obj, weights) pairs
# ------------------------------------------------------------------------------------------------
def _gate_fraction(got, obj, w, window, stride, label):
    """The worst |got - want| / gate over the finite ``want``; NaNs and infinities must sit where the restatement's do."""
    promoted = F64 if F64 in (obj.dtype.type, w.dtype.type) else F32
    assert got.dtype == np.dtype(promoted), (label, got.dtype)
    wb = w if w.ndim == obj.ndim else w.reshape(w.shape[:-2] + (1,) * (obj.ndim - w.ndim) + w.shape[-2:])
    want, mag, den, n = E.window_average_np(obj, wb, window, stride)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    finite = np.isfinite(want)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{label} (NaN pattern)")
    np.testing.assert_array_equal(got[~finite], want[~finite].astype(promoted), err_msg=f"{label} (non-finite results)")
    u_p, u_w = (2.0 ** -24 if promoted == F32 else 2.0 ** -53), (2.0 ** -24 if w.dtype == np.dtype(F32) else 2.0 ** -53)
    with np.errstate(invalid="ignore", divide="ignore"):
        gate = 2 * n * u_p * mag / den + (2 * n * u_w + 2 * u_p) * np.abs(want)
        err = np.abs(got.astype(F64) - want)
        frac = np.where(gate > 0, err / gate, np.where(err == 0, 0.0, np.inf))
    return float(frac[finite].max()) if finite.any() else 0.0


@pytest.mark.parametrize("obj_dtype, w_dtype", cases.FLOAT_PAIRS, ids=_name)
@pytest.mark.parametrize("shared", [False, True], ids=["full", "shared"])
def test_window_average_outside_the_fast_path(device, shared, obj_dtype, w_dtype):
    """Window != stride, overlap, gaps, remainders, the whole field; a NaN in obj, a NaN weight, a window of NaN weights, a
    window of zero weights, an infinity; weights of the field's shape and 2-D weights shared over the levels."""
    from fv3net_amd import ops

    worst = 0.0
    for shape, window, stride in cases.WAVG_WINDOWS:
        obj, w = cases.wavg_inputs(shape, obj_dtype, w_dtype, shared, window)
        got = _np(ops.weighted_window_average(_to(device, obj), _to(device, w), window, stride))
        frac = _gate_fraction(got, obj, w, window, stride, f"{shape} {window}/{stride}")
        assert np.isnan(got).any() and (np.isinf(got).any() or window == shape[-2:]), (shape, window, stride)
        worst = max(worst, frac)
        assert frac <= 1.0, (shape, window, stride, frac)
    print(f"window average {_name(obj_dtype)}/{_name(w_dtype)} shared={shared}: {worst:.3f} of the gate")


@pytest.mark.parametrize("obj_dtype, w_dtype", cases.FLOAT_PAIRS, ids=_name)
def test_block_average_fallback_conditions(device, obj_dtype, w_dtype):
    """``dispatch_wavg`` leaves the fast path at factor 3, factor 64, nx % VEC != 0 and for a pointer 4 (8) bytes off a 16-byte
    boundary; the last agrees with the aligned call within the gate."""
    from fv3net_amd import ops

    worst = 0.0
    for shape, factor in (((2, 3, 6, 12), 3), ((1, 2, 64, 128), 64), ((2, 3, 4, 6), 2)):
        for shared in (False, True):
            obj, w = cases.wavg_inputs(shape, obj_dtype, w_dtype, shared, (factor, factor))
            got = _np(ops.weighted_block_average(_to(device, obj), _to(device, w), factor))
            frac = _gate_fraction(got, obj, w, (factor, factor), (factor, factor), f"{shape} factor {factor}")
            worst = max(worst, frac)
            assert frac <= 1.0, (shape, factor, frac)
    shape, factor = (2, 3, 8, 16), 4
    obj, w = cases.wavg_inputs(shape, obj_dtype, w_dtype, False, (factor, factor))
    to, tw = _to(device, obj), _to(device, w)
    aligned = _np(ops.weighted_block_average(to, tw, factor))

    def shifted(t):  # the same values in a contiguous view that starts one element into its buffer
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0 and t.data_ptr() % 16 == 0
        return view

    for label, a, b in (("obj", shifted(to), tw), ("weights", to, shifted(tw)), ("both", shifted(to), shifted(tw))):
        got = _np(ops.weighted_block_average(a, b, factor))
        frac = _gate_fraction(got, obj, w, (factor, factor), (factor, factor), f"misaligned {label}")
        # against the aligned call: the same gate, centred on the aligned result's own reference
        want, mag, den, n = E.window_average_np(obj, w, (factor, factor), (factor, factor))
        finite = np.isfinite(want)
        u_p, u_w = (2.0 ** -24 if got.dtype == np.dtype(F32) else 2.0 ** -53), (2.0 ** -24 if w_dtype == F32 else 2.0 ** -53)
        gate = 2 * n * u_p * mag[finite] / den[finite] + (2 * n * u_w + 2 * u_p) * np.abs(want[finite])
        between = float((np.abs(got[finite].astype(F64) - aligned[finite].astype(F64)) / gate).max())
        worst = max(worst, frac, _gate_fraction(aligned, obj, w, (factor, factor), (factor, factor), "aligned"))
        assert frac <= 1.0 and between <= 1.0, (label, frac, between)
    print(f"block average fallbacks {_name(obj_dtype)}/{_name(w_dtype)}: {worst:.3f} of the gate")


@pytest.mark.parametrize("obj_dtype, w_dtype", cases.FLOAT_PAIRS, ids=_name)
def test_block_average_fast_path_under_the_same_gate(device, obj_dtype, w_dtype):
    """F in {2, 4, 8, 16, 32} on [2, 3, 2F, max(2F, 16)], weights of the field's shape and shared over the levels, the same
    non-finite plants."""
    from fv3net_amd import ops

    worst = 0.0
    for factor in cases.FAST_FACTORS:
        for shared in (False, True):
            obj, w = cases.wavg_inputs(cases.fast_shape(factor), obj_dtype, w_dtype, shared, (factor, factor))
            got = _np(ops.weighted_block_average(_to(device, obj), _to(device, w), factor))
            frac = _gate_fraction(got, obj, w, (factor, factor), (factor, factor), f"factor {factor} shared {shared}")
            worst = max(worst, frac)
            assert frac <= 1.0, (factor, shared, frac)
    print(f"block average fast path {_name(obj_dtype)}/{_name(w_dtype)}: {worst:.3f} of the gate")


# ------------------------------------------------------------------------------------------------
# block_reduce_kernel, block_rank_wave_kernel: 4 dtypes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.WORD_DTYPES, ids=_name)
@pytest.mark.parametrize("axis", [0, 1])
def test_take_lines(device, axis, dtype):
    """Steps 1, 4, 17 and 40 of 17 lines: the strided slice, infinities included; NaNs where the slice has them."""
    from fv3net_amd import ops

    shape = (2, 3, 5, 17) if axis == 0 else (2, 3, 17, 5)
    isfloat = np.issubdtype(np.dtype(dtype), np.floating)
    x = cases.float_field(shape, dtype) if isfloat else cases.words(shape, dtype)
    if isfloat:  # the first line, which every step keeps
        first = x[0, 0, :, 0] if axis == 0 else x[0, 0, 0, :]
        first[:3] = np.nan, np.inf, -np.inf
    t = _to(device, x)
    for step in cases.TAKE_STEPS:
        got = _np(ops.take_lines(t, step, axis))
        want = x[..., ::step] if axis == 0 else x[..., ::step, :]
        assert got.dtype == want.dtype and got.shape == want.shape, (step, got.shape, want.shape)
        assert np.array_equal(got, want, equal_nan=isfloat), step
        if isfloat:
            assert np.isnan(want).any() and np.isinf(want).any()


@pytest.mark.parametrize("dtype", cases.WORD_DTYPES, ids=_name)
@pytest.mark.parametrize("case", cases.REDUCE_WINDOWS, ids=lambda c: f"{c[1]}/{c[2]}")
def test_block_reduce_over_strided_windows(device, case, dtype):
    """Window != stride for every op and NaN policy: 72 values take the serial kernel, the other windows the wave kernel for
    median and mode.  Small integers, so sums and middle-pair means are exact and the mode has ties; NaNs sprinkled in, one
    window all NaN."""
    from fv3net_amd import ops

    shape, window, stride = case
    isfloat = np.issubdtype(np.dtype(dtype), np.floating)
    a = cases.small_integers(shape, dtype, window)
    t = _to(device, a)
    for op in cases.REDUCE_OPS if isfloat else ("sum", "min", "max", "mode"):
        for policy in (("omit", "propagate") if op == "mode" else ("propagate",) if op == "median" else ("skip", "propagate")):
            got = _np(ops.block_reduce(t, window, stride, op=op, nan_policy=policy))
            want = E.window_reduce_np(a, window, stride, op, policy)
            assert got.dtype == want.dtype
            np.testing.assert_array_equal(got, want, err_msg=f"{op} {policy}")
