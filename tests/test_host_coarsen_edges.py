"""Pins the numpy restatements of tests/coarsen_edge_np.py -- the references of tests/test_gpu_coarsen_edges.py -- against
oracle/coarsen_np.py and numpy on the inputs of tests/coarsen_edge_cases.py, and checks that the conversion cases hold what
their docstring promises.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import coarsen_edge_cases as cases
import coarsen_edge_np as E
from oracle import coarsen_np

F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64


# ------------------------------------------------------------------------------------------------
# window averages
# ------------------------------------------------------------------------------------------------
def _oracle_operands(obj, w):
    """float64 copies with the shared weights broadcast over the level dim."""
    obj = obj.astype(F64)
    w = w.astype(F64)
    return obj, (w[:, None] if w.ndim < obj.ndim else w)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("factor", [1, 2, 3, 4])
def test_window_average_is_the_block_average_at_window_equal_stride(factor, shared):
    shape = (2, 3, 12, 24)
    obj, w = cases.wavg_inputs(shape, F32, F64, shared, (factor, factor))
    o64, w64 = _oracle_operands(obj, w)
    got, mag, den, n = E.window_average_np(obj, w if not shared else w[:, None], (factor, factor), (factor, factor))
    want = coarsen_np.weighted_block_average(o64, w64, factor)
    E.assert_same_outside_nan(got, want)
    assert n == factor * factor and got.shape == (2, 3, 12 // factor, 24 // factor)
    assert np.isnan(got).any() and np.isinf(got).any()   # the planted windows are there
    np.testing.assert_array_equal(den, coarsen_np._nansum_blocks(np.broadcast_to(w64, o64.shape), factor, factor))
    np.testing.assert_array_equal(mag, coarsen_np._nansum_blocks(np.abs(o64 * w64), factor, factor))


@pytest.mark.parametrize("edge", ["x", "y"])
@pytest.mark.parametrize("factor", [2, 3, 4])
def test_window_average_is_the_edge_weighted_average(factor, edge):
    shape = (2, 3, 12, 24)
    window = (1, factor) if edge == "x" else (factor, 1)
    obj, w = cases.wavg_inputs(shape, F64, F32, False, window)
    o64, w64 = _oracle_operands(obj, w)
    got = E.window_average_np(obj, w, window, (factor, factor))[0]
    E.assert_same_outside_nan(got, coarsen_np.edge_weighted_block_average(o64, w64, factor, edge))


def test_window_average_counts_a_nan_obj_in_the_denominator():
    obj = np.array([[1.0, np.nan, 3.0, np.inf]])
    w = np.array([[1.0, 2.0, np.nan, 1.0]])
    got, mag, den, n = E.window_average_np(obj, w, (1, 2), (1, 2))
    np.testing.assert_array_equal(got, [[1.0 / 3.0, np.inf]])   # 3 * NaN and NaN are left out; inf * 1 / 1
    np.testing.assert_array_equal(den, [[3.0, 1.0]])
    np.testing.assert_array_equal(mag, [[1.0, np.inf]])
    # overlapping windows and gaps: the windows sliding_window_view makes, by hand
    a = np.arange(20.0).reshape(4, 5)
    got = E.window_average_np(a, np.ones_like(a), (2, 2), (2, 3))[0]
    np.testing.assert_array_equal(got, [[a[0:2, 0:2].mean(), a[0:2, 3:5].mean()], [a[2:4, 0:2].mean(), a[2:4, 3:5].mean()]])


# ------------------------------------------------------------------------------------------------
# boundary vectors, the pick, the lines
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("n", [1, 2, 12])
def test_lines_from_picked_rows_are_the_oracle_on_all_twelve_edges(n, axis, dtype):
    a = np.random.default_rng(n).normal(0, 2, (6, 5, n, n)).astype(dtype)
    want = coarsen_np.interp_center_to_outer(a, axis)
    lo, hi = E.halo_pick_np(E.edge_rows_np(a), range(6), axis)
    for step in [s for s in cases.INTERP_STEPS if n % s == 0]:
        got = E.interp_lines_np(a, lo, hi, 0 if axis == "x" else 1, step)
        E.assert_same_words(got, want[..., ::step] if axis == "x" else want[..., ::step, :], err_msg=f"step {step}")
    # the two halo edges of every tile differ from a tile padded with itself: all 12 edges are in play
    if n > 1:
        own = E.interp_lines_np(a, a[..., :, -1] if axis == "x" else a[..., -1, :], a[..., :, 0] if axis == "x" else a[..., 0, :],
                                0 if axis == "x" else 1)
        first, last = (np.s_[..., :, 0], np.s_[..., :, -1]) if axis == "x" else (np.s_[..., 0, :], np.s_[..., -1, :])
        for t in range(6):
            assert not np.array_equal(own[t][first[1:]], want[t][first[1:]]) and not np.array_equal(own[t][last[1:]], want[t][last[1:]])


@pytest.mark.parametrize("dtype", cases.WORD_DTYPES)
@pytest.mark.parametrize("shape", cases.CUBE_SHAPES)
def test_halo_pick_is_the_cpu_branch_of_halos_from_rows(shape, dtype):
    import torch

    from fv3net_amd.cubedsphere.grid import halos_from_rows

    a = cases.words(shape, dtype)
    rows = E.edge_rows_np(a)
    assert rows.shape == (6, 4) + shape[1:-2] + shape[-1:]
    for tiles in cases.TILE_LISTS:
        for axis in ("x", "y"):
            lo, hi = E.halo_pick_np(rows, tiles, axis)
            t_lo, t_hi = halos_from_rows(torch.from_numpy(rows), tiles, axis)
            E.assert_same_words(lo, t_lo.numpy(), err_msg=f"{tiles} {axis} lo")
            E.assert_same_words(hi, t_hi.numpy(), err_msg=f"{tiles} {axis} hi")


def test_edge_rows_by_hand():
    a = np.arange(6 * 9).reshape(6, 3, 3)
    rows = E.edge_rows_np(a)
    np.testing.assert_array_equal(rows[1], [[9, 12, 15], [11, 14, 17], [9, 10, 11], [15, 16, 17]])
    # tile 0 along x: left neighbour 4 through its y axis (last row, reversed), right neighbour 1 through x (first column)
    lo, hi = E.halo_pick_np(rows, [0], "x")
    np.testing.assert_array_equal(lo[0], a[4][-1, ::-1])
    np.testing.assert_array_equal(hi[0], a[1][:, 0])


# ------------------------------------------------------------------------------------------------
# strided reductions, repeat
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", cases.WORD_DTYPES)
@pytest.mark.parametrize("factor", [2, 3])
def test_window_reduce_is_block_coarsen_at_window_equal_stride(factor, dtype):
    a = cases.small_integers((2, 3, 6, 12), dtype, (factor, factor))
    isfloat = np.issubdtype(np.dtype(dtype), np.floating)
    for op in cases.REDUCE_OPS if isfloat else ("sum", "min", "max", "mode"):
        got = E.window_reduce_np(a, (factor, factor), (factor, factor), op, "propagate" if op == "mode" else "skip")
        assert got.dtype == np.dtype(dtype)
        np.testing.assert_array_equal(got, coarsen_np.block_coarsen(a, factor, op), err_msg=op)
    if isfloat:
        np.testing.assert_array_equal(E.window_reduce_np(a, (factor, factor), (factor, factor), "mode", "omit"),
                                      coarsen_np.block_mode(a, factor, "omit"))
        # 'propagate' is numpy's plain reduction
        b = coarsen_np._blocks(a, factor, factor)
        for op, fn in (("sum", np.sum), ("mean", np.mean), ("min", np.min), ("max", np.max)):
            np.testing.assert_array_equal(E.window_reduce_np(a, (factor, factor), (factor, factor), op, "propagate"), fn(b, axis=(-3, -1)))
        assert np.isnan(E.window_reduce_np(a, (factor, factor), (factor, factor), "min", "skip")).any()   # the all-NaN window


def test_window_reduce_strided_by_hand():
    a = np.arange(20.0).reshape(4, 5)
    np.testing.assert_array_equal(E.window_reduce_np(a, (1, 1), (1, 2), "max", "propagate"), a[:, ::2])
    np.testing.assert_array_equal(E.window_reduce_np(a, (2, 2), (2, 3), "sum"), [[12.0, 24.0], [52.0, 64.0]])
    np.testing.assert_array_equal(E.window_reduce_np(a, (3, 2), (1, 1), "median")[0], a[1, :4] + 0.5)


def test_repeat_by_hand():
    a = np.array([[1, 2], [3, 4]])
    np.testing.assert_array_equal(E.repeat_np(a, 2, 3), [[1, 1, 1, 2, 2, 2]] * 2 + [[3, 3, 3, 4, 4, 4]] * 2)
    np.testing.assert_array_equal(E.repeat_np(a, 2, 2), coarsen_np.block_upsample(a, 2))


# ------------------------------------------------------------------------------------------------
# the conversion cases hold what their docstring promises
# ------------------------------------------------------------------------------------------------
def _exact(v):
    return Fraction(int(v)) if isinstance(v, (np.integer, int)) else Fraction(float(v))


def _ties_to_even(values, out_dtype):
    """The finite values that lie exactly half way between two neighbouring numbers of ``out_dtype`` (infinity standing in for
    the number after the largest), with whether ``astype`` went to the even one."""
    out = E.cast_np(values, out_dtype)
    bits = E.int_view(out)
    inf = out_dtype(np.inf)
    found = []
    for v, r, b in zip(values, out, bits):
        if not isinstance(v, np.integer) and not np.isfinite(v):
            continue
        x = _exact(v)
        if np.isinf(r):  # the neighbours are FLT_MAX and the 2^128 that infinity stands for
            fmax = Fraction(float(np.finfo(out_dtype).max))
            step = Fraction(2) ** (np.finfo(out_dtype).maxexp - np.finfo(out_dtype).nmant - 1)
            if abs(x) - fmax == step / 2:
                found.append((v, True))
            continue
        if _exact(r) == x:
            continue
        with np.errstate(over="ignore"):
            other = np.nextafter(r, inf if x > _exact(r) else -inf)
        if np.isfinite(other) and abs(x - _exact(r)) == abs(x - _exact(other)):
            found.append((v, int(b) & 1 == 0))
    return found


@pytest.mark.parametrize("in_dtype, out_dtype", [(I32, F32), (I64, F32), (I64, F64), (F64, F32)])
def test_conversion_cases_hold_ties_to_even(in_dtype, out_dtype):
    ties = _ties_to_even(cases.conversion_values(in_dtype), out_dtype)
    assert len(ties) >= 4, ties
    assert all(even for _, even in ties), ties   # numpy's astype rounds half to even: it is the reference


def test_conversion_cases_hold_the_promised_values():
    v64, v32 = cases.conversion_values(F64), cases.conversion_values(F32)
    with np.errstate(over="ignore"):
        r = v64.astype(F32)
    fi = np.finfo(F32)
    assert (np.isinf(r) & np.isfinite(v64)).sum() >= 4                       # float64 -> float32 overflow, both signs
    assert r[v64 == F64(fi.max) + 2.0 ** 103][0] == np.inf                   # the halfway point goes to infinity ...
    assert r[v64 == np.nextafter(F64(fi.max) + 2.0 ** 103, 0)][0] == fi.max  # ... the double below it does not
    sub = (r != 0) & (np.abs(r) < fi.tiny)
    assert sub.sum() >= 8 and (sub & (v64 != r.astype(F64))).sum() >= 4      # subnormal float32 results, some of them rounded
    assert ((r == 0) & (v64 != 0)).sum() >= 4 and (np.signbit(r) & (r == 0) & (v64 != 0)).any()   # underflow to +-0
    for v in (v64, v32):
        assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
        assert ((v == 0) & np.signbit(v)).any() and ((v == 0) & ~np.signbit(v)).any()
    assert ((v32 != 0) & (np.abs(v32) < fi.tiny)).sum() >= 4 and (v32 == fi.max).any()
    i32, i64 = cases.conversion_values(I32), cases.conversion_values(I64)
    for want, have in (([2 ** 24 - 1, 2 ** 24 + 1, 2 ** 24 + 3, np.iinfo(I32).min, np.iinfo(I32).max], i32),
                       ([2 ** 24 + 1, 2 ** 53 - 1, 2 ** 53 + 1, 2 ** 53 + 3, np.iinfo(I64).min, np.iinfo(I64).max,
                         2 ** 40 + 2 ** 16 - 1, 2 ** 40 + 2 ** 16, 2 ** 40 + 2 ** 16 + 1], i64)):
        assert set(want) <= set(have.tolist())
    for dtype in cases.WORD_DTYPES:
        assert cases.conversion_values(dtype).dtype == np.dtype(dtype) and cases.conversion_values(dtype).size >= 300


def test_cast_many_cases():
    for count in cases.CAST_MANY_COUNTS:
        for out_dtype in (F32, F64):
            ts = cases.cast_many_tensors(count, out_dtype)
            todo = [t for t in ts if t.dtype != np.dtype(out_dtype)]
            assert len(todo) == count and len(ts) == count + count // 7   # the table entries, and those already converted
            assert {t.size for t in todo} >= {1, 257} and (count == 2 or todo[2].size == 0)
            assert {t.dtype for t in todo} == {np.dtype(d) for d in cases.WORD_DTYPES} - {np.dtype(out_dtype)} or count == 2
            assert (max(t.size for t in ts) == cases.CAST_MANY_LONG) == (count >= 48)
            if count >= 48:
                assert todo[count - 2].size == cases.CAST_MANY_LONG and todo[count - 3].size <= 1000 and todo[count - 1].size <= 1000


def test_words_hold_nan_payloads_and_negative_zero():
    for dtype in (F32, F64):
        a = cases.words((6, 5, 12, 12), dtype)
        assert np.isnan(a).any() and ((a == 0) & np.signbit(a)).any()
        assert len(set(E.int_view(a[np.isnan(a)]).tolist())) > 1   # more than one NaN payload
