"""The checkers of ``tests/test_gpu_conv_edges.py`` (``conv_cases.assert_close_with_non_finite``, ``assert_close_pooled``) held
to the float32 CPU chain against the float64 oracle: they pass on the reference arithmetic itself, and fail on a cleared NaN
and on one finite value moved by 1e-4 of its level's scale (ten times the gate).  No GPU.

Float32 CPU chain against float64, worst per-level error / scale of the cases the device tests use (run with ``-s``):
the shape sweep 1.8e-7 ... 6.6e-7 over the seven networks, the small cubes 0.9e-7 ... 8.1e-7, the non-finite cases'
finite part 2.1e-7 ... 3.7e-7 -- at most 0.08 of the gate of 1e-5.
"""
import numpy as np
import pytest

import conv_cases


def _heads(spec):
    return [(o.name, o.nfeat) for o in spec.outputs]


@pytest.mark.parametrize("value", list(conv_cases.NON_FINITE))
@pytest.mark.parametrize("activation", conv_cases.ACTIVATION_NAMES)
def test_float32_chain_passes_the_non_finite_checker(activation, value):
    """The class map of the float32 chain equals the float64 oracle's in all nine combinations -- condition (a) is exact --
    and the oracle's count of non-finite pixels is what the receptive fields say: the 5 x 5 outputs around the interior hit
    plus the one output that sees the halo corner, 26 of 360; none for tanh of an infinity (tanh(+-Inf) = +-1), whose
    outputs still differ from the clean run's."""
    spec, (clean, planted) = conv_cases.non_finite_case(activation, conv_cases.NON_FINITE[value])
    nx, ny = conv_cases.NON_FINITE_EXTENT
    want = 0 if (activation == "tanh" and value != "nan") else 26
    inside = conv_cases.footprint_mask(spec, nx, ny)
    assert int(inside.sum()) == 25
    for name, nf in _heads(spec):
        truth, cpu32 = planted[2][name], planted[3][name]
        assert truth.shape == (2, nx, ny, nf)
        n_bad = conv_cases.assert_close_with_non_finite(cpu32, truth, cpu32, name=f"{activation} {value} {name}")
        assert n_bad == want, (name, n_bad)
        changed = np.any(truth != clean[2][name], axis=-1)   # (NaN != x is True: the non-finite pixels count as changed)
        touched = np.zeros((2, nx, ny), bool)
        touched[0][inside] = True
        touched[1, 0, 0] = True
        np.testing.assert_array_equal(changed, touched)
        if want:
            np.testing.assert_array_equal(~np.isfinite(truth).all(axis=-1), touched)
        t0, c0 = (np.where(np.isfinite(truth), a, 0) for a in (truth, cpu32))
        print(f"{activation} {value} {name}: float32 chain, worst finite error / scale "
              f"{np.max(np.abs(c0 - t0) / np.max(np.abs(t0), axis=(0, 1, 2))):.2e}, non-finite pixels {n_bad}")


def _planted_relu_nan():
    spec, (_, planted) = conv_cases.non_finite_case("relu", np.nan)
    return planted[2]["dQ1"], planted[3]["dQ1"]


def test_checker_fails_on_a_cleared_nan():
    """What ``v > 0 ? v : 0`` does to a NaN: one NaN of the result replaced by 0."""
    truth, cpu32 = _planted_relu_nan()
    got = cpu32.copy()
    where = tuple(np.argwhere(np.isnan(got))[0])
    got[where] = 0.0
    with pytest.raises(AssertionError, match="differ in class"):
        conv_cases.assert_close_with_non_finite(got, truth, cpu32, name="cleared")
    # ... and a NaN where the oracle is finite, or an infinity of the other sign, is as wrong
    got = cpu32.copy()
    got[1, 5, 5, 0] = np.nan
    with pytest.raises(AssertionError, match="differ in class"):
        conv_cases.assert_close_with_non_finite(got, truth, cpu32, name="spurious")
    truth, cpu32 = truth.copy(), cpu32.copy()
    truth[1, 5, 5, 0], cpu32[1, 5, 5, 0] = np.inf, np.inf
    got = cpu32.copy()
    got[1, 5, 5, 0] = -np.inf
    with pytest.raises(AssertionError, match="differ in class"):
        conv_cases.assert_close_with_non_finite(got, truth, cpu32, name="sign")


def test_checker_fails_on_a_moved_finite_value():
    """One finite value moved by 1e-4 of its level's scale (ten times the gate) next to the non-finite ones."""
    truth, cpu32 = _planted_relu_nan()
    level = truth.shape[-1] - 1   # the smallest level: 4.5 decades below the first
    scale = np.max(np.abs(np.where(np.isfinite(truth[..., level]), truth[..., level], 0)))
    got = cpu32.copy()
    assert np.isfinite(got[1, 7, 3, level])
    got[1, 7, 3, level] += 1e-4 * scale
    with pytest.raises(AssertionError, match=f"level {level}"):
        conv_cases.assert_close_with_non_finite(got, truth, cpu32, name="moved")


def test_checker_caps_the_non_finite_share():
    truth, cpu32 = _planted_relu_nan()
    truth, cpu32 = truth.copy(), cpu32.copy()
    truth[0, :3], cpu32[0, :3] = np.nan, np.nan   # 27 + 26 pixels of 360
    with pytest.raises(AssertionError, match="nothing left to judge"):
        conv_cases.assert_close_with_non_finite(cpu32, truth, cpu32, name="cap")


@pytest.mark.parametrize("name", list(conv_cases.EDGE_NETWORKS))
def test_float32_chain_passes_the_pooled_gate_of_the_shape_sweep(name):
    spec, parts = conv_cases.sweep_case(name)
    h = spec.halos_required
    assert sum(2 * nx * ny for nx, ny in conv_cases.EDGE_EXTENTS) == 3876
    for head, nf in _heads(spec):
        for (nx, ny), fields, truth, cpu32 in parts:
            assert truth[head].shape == cpu32[head].shape == (2, nx, ny, nf)
            assert all(v.shape[:3] == (2, nx + 2 * h, ny + 2 * h) for v in fields.values())
        worst = conv_cases.assert_close_pooled([(ext, c[head], t[head], c[head]) for ext, _, t, c in parts], f"{name} {head}")
        print(f"{name} {head}: float32 chain, worst per-level error / scale {worst:.2e}")
        assert worst <= 0.1 * 1e-5


@pytest.mark.parametrize("name", list(conv_cases.CUBE_NETWORKS))
def test_float32_chain_passes_the_pooled_gate_of_the_small_cubes(name):
    spec, parts = conv_cases.cube_case(name)
    for head, nf in _heads(spec):
        worst = conv_cases.assert_close_pooled([(f"n = {n}", c[head], t[head], c[head]) for n, _, t, c in parts], f"{name} {head}")
        print(f"{name} {head}: float32 chain, worst per-level error / scale {worst:.2e}")
        assert worst <= 0.1 * 1e-5


def test_pooled_gate_names_the_extent_of_the_worst_error():
    spec, parts = conv_cases.sweep_case("k5_c7_f5")
    entries = [(ext, c["dQ1"].copy(), t["dQ1"], c["dQ1"]) for ext, _, t, c in parts]
    scale = max(np.max(np.abs(t["dQ1"][..., 0])) for _, _, t, _ in parts)
    entries[5][1][1, 16, 14, 0] += 1e-4 * scale   # the last pixel of the 17 x 15 field
    with pytest.raises(AssertionError, match=r"in part \(17, 15\).*level 0"):
        conv_cases.assert_close_pooled(entries, "moved")
    # the scale is the pooled one: the same 1 x 1 field passes in the pool and has a (much smaller) scale of its own
    one = parts[0]
    assert np.max(np.abs(one[2]["dQ1"][..., 0])) < scale


def test_references_are_shared_and_read_only():
    a, b = conv_cases.sweep_case("k1"), conv_cases.sweep_case("k1")
    assert a is b
    with pytest.raises(ValueError):
        a[1][0][2]["dQ1"][0, 0, 0, 0] = 1.0
