"""The reservoir edge tests' own checker and inputs, on the CPU: the checker fails on what it must catch, the restatement
alone stays well inside the gate at every increment shape the device tests use, and the non-finite cases are what they
claim to be (tests/reservoir_cases.py; the device side is tests/test_gpu_reservoir_edges.py)."""
import numpy as np
import pytest

import reservoir_cases as C


def test_checker_catches_a_moved_value_and_a_cleared_nan():
    rng = np.random.RandomState(0)
    want = rng.uniform(-1, 1, (6, 41))
    want[2, 7], want[4, 0], want[5, 40] = np.nan, np.inf, -np.inf
    assert C.check(want.copy(), want, C.STATE_GATE) == 0.0
    near = want.copy()
    near[0, 0] += 0.5e-13
    assert 0.4 < C.check(near, want, C.STATE_GATE) <= 0.51
    moved = want.copy()
    moved[3, 9] += 2e-13
    moved[3, 11] -= 3e-13
    with pytest.raises(AssertionError, match=r"2 of 246 elements are outside the gate; first at \(3, 9\)"):
        C.check(moved, want, C.STATE_GATE, "moved")
    cleared = want.copy()
    cleared[2, 7] = 0.0
    with pytest.raises(AssertionError, match=r"1 of 246 elements differ in class.*first at \(2, 7\): got 0 .*want 3"):
        C.check(cleared, want, C.STATE_GATE, "cleared")
    for at, value in (((4, 0), -np.inf), ((5, 40), np.nan), ((1, 1), np.nan)):
        other = want.copy()
        other[at] = value
        with pytest.raises(AssertionError, match="differ in class"):
            C.check(other, want, C.STATE_GATE)
    # float32 outputs: one ulp passes, two do not; a float64 answer where float32 is due is refused
    w32 = rng.randn(4, 5, 2).astype(np.float32)
    C.check_outputs([np.nextafter(w32, np.float32(np.inf))], [w32])
    with pytest.raises(AssertionError, match="outside the gate"):
        C.check_outputs([np.nextafter(np.nextafter(w32, np.float32(np.inf)), np.float32(np.inf))], [w32])
    with pytest.raises(AssertionError):
        C.check_outputs([w32.astype(np.float64)], [w32])


def test_checker_catches_a_transposed_layout():
    """A (2, 3) layout cut or merged as (3, 2), on a 6 x 6 rank that both layouts divide."""
    rng = np.random.RandomState(1)
    m = C.make_model(rng, (2, 3), (3, 2), overlap=1, in_sizes=(2, 1), out_sizes=(2, 1))
    assert m["rank"] == (6, 6)
    arrays = C.make_arrays(rng, (2, 1), C.ov_extent(m))
    state = rng.uniform(-1, 1, (6, 41))
    with pytest.raises(AssertionError, match="outside the gate"):
        C.check(C.increment(dict(m, layout=(3, 2)), state, arrays), C.increment(m, state, arrays), C.STATE_GATE)
    with pytest.raises(AssertionError, match="outside the gate"):
        C.check_outputs(C.predict(dict(m, layout=(3, 2)), state), C.predict(m, state))


@pytest.mark.parametrize("transformer, mask", [("do-nothing", "f32"), ("scale-f32", "none"), ("scale-f32", "f32"),
                                               ("scale-none", "f32")])
@pytest.mark.parametrize("hybrid", [False, True])
def test_a_missing_float32_rounding_is_far_outside_the_gate(transformer, mask, hybrid):
    """The restatement with the float32 masks widened to float64 (no rounding of the product) differs from the real one by
    much more than the gate, so the device's dtype matrix can fail."""
    m, state, x, h = C.dtype_case("f32", transformer, mask, hybrid)
    wide = dict(m)
    side = "hybrid" if hybrid else "input"
    wide[side] = dict(m[side])
    if wide[side].get("mask") is not None:
        wide[side]["mask"] = wide[side]["mask"].astype(np.float64)
    key = "hybrid_mask" if hybrid else "input_mask"
    if m[key] is not None:
        wide[key] = m[key].astype(np.float64)
    if hybrid:
        want, other = C.predict(m, state, h), C.predict(wide, state, h)
        for w, o in zip(want, other):
            assert np.abs(w - o).max() > 1e3 * C.output_gate(w)
        with pytest.raises(AssertionError, match="outside the gate"):
            C.check_outputs(other, want)
    else:
        want, other = C.increment(m, state, x), C.increment(wide, state, x)
        assert np.abs(want - other).max() > 1e3 * C.STATE_GATE
        with pytest.raises(AssertionError, match="outside the gate"):
            C.check(other, want, C.STATE_GATE)


def test_restatement_follows_numpys_promotion():
    """The masked input's dtype is what numpy gives it: float32 only when every factor is."""
    for sources in C.SOURCES:
        for transformer, (kind, tf_mask) in C.TRANSFORMERS.items():
            for mask, mask_dtype in C.MASKS.items():
                m, state, x, _ = C.dtype_case(sources, transformer, mask, False)
                u = C.masked_input(m, x)
                enc32 = (kind == "scale-spatial" and tf_mask is not np.float64) or (kind == "do-nothing" and sources == "f32")
                want = np.float32 if enc32 and mask_dtype is not np.float64 else np.float64
                assert u.dtype == want, (sources, transformer, mask, u.dtype)


def _increment_shapes():
    for layout in C.LAYOUTS:
        for overlap in (0, 1):
            yield f"layout{layout}-overlap{overlap}", lambda l=layout, o=overlap: C.cached(C.layout_case, l, o)[:3]
    for size in C.STATE_SIZES:
        yield f"state{size}", lambda s=size: C.cached(C.state_size_case, s)
    for name in C.MULTI_STEP:
        yield name, lambda n=name: C.cached(C.multi_step_case, n)
    for sources in C.SOURCES:
        for transformer in C.TRANSFORMERS:
            for mask in C.MASKS:
                yield f"dtype-{sources}-{transformer}-{mask}", lambda a=(sources, transformer, mask): C.dtype_case(*a, False)[:3]
    for name in C.sparse_cases():
        yield f"sparse-{name}", lambda n=name: C.sparse_cases()[n][:3]


@pytest.mark.parametrize("name, build", list(_increment_shapes()), ids=[n for n, _ in _increment_shapes()])
def test_restatement_alone_stays_inside_a_quarter_of_the_gate(name, build):
    """The pre-activation summed in a permuted order of the inputs and of the state agrees with the restatement's own within
    0.25 of the state gate (tanh only shrinks a difference): the reference's own error leaves the gate meaningful."""
    m, state, x = build()
    u = np.asarray(C.masked_input(m, x), np.float64)
    finite_u, finite_s = np.where(np.isfinite(u), u, 0.0), np.where(np.isfinite(state), state, 0.0)
    rng = np.random.RandomState(5)
    w_in, w_res = C.dense_of(m["w_in"]), C.dense_of(m["w_res"])
    a = finite_u @ w_in.T + finite_s @ w_res.T
    p, q = rng.permutation(u.shape[1]), rng.permutation(state.shape[1])
    b = finite_u[:, p] @ w_in[:, p].T + finite_s[:, q] @ w_res[:, q].T
    b2 = finite_u[:, p[::-1]] @ w_in[:, p[::-1]].T + finite_s[:, q[::-1]] @ w_res[:, q[::-1]].T
    worst = max(np.abs(a - b).max(), np.abs(a - b2).max())
    assert worst <= 0.25 * C.STATE_GATE, (name, worst)


def test_stored_product_is_scipys():
    """``product(.., "stored")`` against scipy's csc product, the reference's own (reservoir.py), class for class."""
    sp = pytest.importorskip("scipy.sparse")
    cases = [(m, C.masked_input(m, planted)) for m, _, _, planted in C.input_cases().values()]
    cases += [(v[0], C.masked_input(v[0], v[2])) for v in C.sparse_cases().values()]
    m, _, x = C.dense_difference_case()
    cases.append((m, C.masked_input(m, x)))
    for m, u in cases:
        indptr, idx, val, shape = m["w_in"]
        w = sp.csc_matrix(sp.csr_matrix((val, idx, indptr), shape=shape))
        with np.errstate(invalid="ignore", over="ignore"):
            want = u @ w.T
        C.check(C.product(u, m["w_in"], "stored"), want, 0.25 * C.STATE_GATE)
    for m, state, _ in C.state_cases().values():
        indptr, idx, val, shape = m["w_res"]
        w = sp.csc_matrix(sp.csr_matrix((val, idx, indptr), shape=shape))
        with np.errstate(invalid="ignore", over="ignore"):
            want = state @ w.T
        C.check(C.product(state, m["w_res"], "stored"), want, 0.25 * C.STATE_GATE)


def test_summed_duplicates_are_scipys():
    sp = pytest.importorskip("scipy.sparse")
    coo, summed = C.coo_with_duplicates(np.random.RandomState(3), 41, 32, 0.7, 0.05, 60)
    ref = sp.coo_matrix((coo["data"], (coo["row"], coo["col"])), shape=(41, 32)).tocsr()
    assert coo["data"].size == summed[2].size + 60
    np.testing.assert_allclose(C.dense_of(summed), ref.toarray(), rtol=0, atol=1e-17)
    np.testing.assert_array_equal(C.stored_of(summed), ref.toarray() != 0)


def _pinned(pre, new, name):
    bad = ~np.isfinite(pre)
    assert bad.any(), (name, "no non-finite entry reaches the state's pre-activation")
    assert np.isfinite(new).sum() * 2 >= new.size, (name, "less than half of the new state is finite")


def test_non_finite_cases_are_what_they_claim():
    """Per case: at least one non-finite entry in the pre-activation (an infinite one leaves tanh as exactly +-1, a NaN as
    NaN), and at least half of the new state finite, so that the finite gate still judges something."""
    x, y = C.NF_SHARED_CELL
    for name, (m, state, clean, planted) in C.input_cases().items():
        a, b = C.pre_activation(m, state, planted)
        new = C.increment(m, state, planted)
        _pinned(a + b, new, name)
        u = C.masked_input(m, planted)
        hit = np.nonzero(~np.isfinite(u).all(axis=1))[0]
        if name.startswith("overlap") or name.endswith("zero-on-nan"):
            assert tuple(hit) == C.NF_SHARED_BY, (name, hit)
        if name.startswith("corner"):
            assert tuple(hit) == (0,), (name, hit)
        if "inf" in name and "meets" not in name:
            assert np.isfinite(new).all() and (np.abs(new) == 1.0).sum() == 41 * len(hit), name
        # the fully stored W_in makes the two semantics agree
        np.testing.assert_array_equal(C.classes(new), C.classes(C.increment(m, state, planted, "dense")))
    meet = C.increment(*[C.input_cases()["inf-meets-inf"][i] for i in (0, 1, 3)])
    assert np.isnan(meet[0]).any() and (np.abs(meet[0]) == 1.0).any() and np.isfinite(meet[1:]).all()
    zero = C.masked_input(*[C.input_cases()["zero-denominator"][i] for i in (0, 3)])
    assert np.isnan(zero).any() and np.isinf(zero).any()
    far = C.masked_input(*[C.input_cases()["beyond-float32"][i] for i in (0, 3)])
    assert np.isposinf(far).any() and np.isneginf(far).any() and not np.isnan(far).any()
    for name, (m, state, arrays) in C.state_cases().items():
        a, b = C.pre_activation(m, state, arrays)
        new = C.increment(m, state, arrays)
        _pinned(a + b, new, name)
        assert np.isfinite(np.delete(new, 1 if name != "inf-meets-inf" else (1, 7), axis=0)).all(), name
        assert 0 < (~np.isfinite(b[1])).sum() < 41, (name, "W_res must carry the value to some rows, not to all")
    meet = C.increment(*C.state_cases()["inf-meets-inf"])
    assert np.isnan(meet[1]).any() and (meet[7] == 1.0).any() and (meet[7] == -1.0).any()


def test_dense_difference_is_pinned():
    """Finding recorded in DESIGN section 12: with 90 % of W_in stored, scipy's product and a dense product disagree on which
    state rows a NaN input reaches."""
    m, state, arrays = C.dense_difference_case()
    stored, dense = C.increment(m, state, arrays, "stored"), C.increment(m, state, arrays, "dense")
    assert np.isnan(dense).all()  # the cell lies in all four subdomains
    assert 0 < np.isnan(stored).sum() < dense.size
    assert (C.classes(stored) != C.classes(dense)).any()
    with pytest.raises(AssertionError, match="differ in class"):
        C.check(dense, stored, C.STATE_GATE)
    column_stored = C.stored_of(m["w_in"])
    u = C.masked_input(m, arrays)
    for s in range(4):
        k = np.nonzero(np.isnan(u[s]))[0]
        assert k.size == 1
        np.testing.assert_array_equal(np.isnan(stored[s]), column_stored[:, k[0]])


def test_sparse_cases_are_what_they_claim():
    cases = C.sparse_cases()
    m = cases["empty-rows"][0]
    assert (np.diff(m["w_in"][0]) == 0).sum() >= 3 and (np.diff(m["w_res"][0]) == 0).sum() >= 4
    assert cases["empty-w-in"][0]["w_in"][0][-1] == 0
    m, state, x = cases["stored-zeros"][:3]
    assert (m["w_in"][2] == 0).sum() > 50 and (m["w_res"][2] == 0).sum() > 20
    # a stored zero meets the NaN input: stored semantics differ from a product that skips zeros
    u = C.masked_input(m, x)
    s, k = np.argwhere(np.isnan(u))[0]
    zero_there = C.stored_of(m["w_in"])[:, k] & (C.dense_of(m["w_in"])[:, k] == 0)
    assert zero_there.any() and np.isnan(C.product(u, m["w_in"], "stored")[s][zero_there]).all()
    coo = cases["coo-duplicates"][3]
    pairs = coo["row"].astype(np.int64) * 32 + coo["col"]
    assert pairs.size - np.unique(pairs).size == 60
    m = cases["unsorted-columns"][0]
    indptr, idx = m["w_in"][0], m["w_in"][1]
    assert any((np.diff(idx[indptr[i]:indptr[i + 1]]) < 0).any() for i in range(41))
    assert cases["just-below-half"][0]["w_in"][0][-1] * 2 == 41 * 32 - 2
    assert cases["just-at-half"][0]["w_in"][0][-1] * 2 == 41 * 32
    assert cases["just-above-half"][0]["w_in"][0][-1] * 2 == 41 * 32 + 2


def test_readout_cases_are_what_they_claim():
    for name, (layout, sub, size, hybrid_sizes, out_sizes) in C.READOUTS.items():
        m, state, h = C.readout_case(name, False, "do-nothing")
        n_h = sub[0] * sub[1] * sum(hybrid_sizes) if hybrid_sizes else 0
        assert name == f"S{size}_H{n_h}"
        assert m["coefficients"].shape == (layout[0] * layout[1], size + n_h, sub[0] * sub[1] * sum(out_sizes))
    assert {C.readout_case(n, False, "do-nothing")[0]["coefficients"].shape[2] for n in C.READOUTS} >= {1, 9, 18}
