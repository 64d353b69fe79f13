"""The reservoir kernels at their edges on the MI355X, against the restatement (tests/reservoir_cases.py, whose checker and
inputs tests/test_oracle_reservoir.py pins on the CPU): every slice plan of the dense input product and of the readout,
non-square layouts and partial subdomain groups, the dtype rules of sources and masks, non-finite inputs and states, sparse
structure, a captured graph's replays and the state's bookkeeping across the parity of the double buffer.

Every test that depends on the launch plan asserts through ``ReservoirModel.plan()`` that its shape reaches the path it was
chosen for.  Gates: the state within 1e-13, float64 outputs within 1e-12 * max|y|, float32 outputs
within one ulp; each test prints the fraction of its gate that it used.
"""
import numpy as np
import pytest
import torch

from fv3net_amd import fit
from fv3net_amd.graphs import GraphedCall
from fv3net_amd.reservoir import WIN_AUTO, WIN_CSR, WIN_DENSE, SparseMatrix

import reservoir_cases as C

pytestmark = pytest.mark.gpu

STORAGES = {"dense": WIN_DENSE, "csr": WIN_CSR}


def _note(section, name, ratio):
    print(f"gate fraction [{section}] {name}: {ratio:.3g}")


def _device(arrays, views=None):
    """Device tensors of the arrays; ``views``: per variable "plain", "transposed" or "strided" device views."""
    out = []
    for v, a in enumerate(arrays):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        view = views[v] if views else "plain"
        if view == "transposed":
            t = t.permute(2, 1, 0).contiguous().permute(2, 1, 0)
        elif view == "strided":
            big = torch.zeros((a.shape[0], 2 * a.shape[1], a.shape[2] + 1), dtype=t.dtype, device="cuda")
            big[:, ::2, :a.shape[2]] = t
            t = big[:, ::2, :a.shape[2]]
        out.append(t)
    return out


def _predict(model, hybrid):
    return model.predict(hybrid) if hybrid is not None else model.predict()


def _kpad(m):
    return -(-C.n_in_of(m) // 64) * 64


# ---------------------------------------------------------------------------------------------
# plan shapes of the increment
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("layout", list(C.LAYOUTS), ids=lambda l: f"{l[0]}x{l[1]}")
def test_layouts_and_partial_groups(layout, overlap):
    """2, 3, 6, 9, 12, 33 and 36 subdomains in non-square layouts of 2 x 3 cells: every subdomain count per wave, partial
    groups, x and y told apart in the cut (increment, hybrid inputs) and in the merge (predict); three input variables of
    different z sizes."""
    m, state, x, h = C.cached(C.layout_case, layout, overlap)
    want = C.cached(_layout_reference, layout, overlap)
    for name, storage in STORAGES.items():
        model = C.package_model(m, state=state, storage=storage)
        plan = model._model().plan()
        assert plan["dense"] == (storage == WIN_DENSE)
        if storage == WIN_DENSE:
            assert plan["in_sb"] == C.LAYOUTS[layout], plan
            assert plan["ldw"] == 42 and plan["in_chunk"] == 64
        model.increment_state(x)
        _note("layouts", f"{layout} overlap {overlap} {name} state", C.check(model.get_state(), want[0], C.STATE_GATE, name))
        model.set_state(want[0])
        _note("layouts", f"{layout} overlap {overlap} {name} outputs", C.check_outputs(model.predict(h), want[1], name))


def _layout_reference(layout, overlap):
    m, state, x, h = C.cached(C.layout_case, layout, overlap)
    new = C.increment(m, state, x)
    return new, C.predict(m, new, h)


@pytest.mark.parametrize("size", C.STATE_SIZES)
def test_state_sizes(size):
    """State sizes around the 128 rows of a wave: the clamped lanes past the last pair of rows, the odd row's padding, a
    second block that is almost empty; three subdomains in a group of four."""
    m, state, x = C.cached(C.state_size_case, size)
    want = C.increment(m, state, x)
    for name, storage in STORAGES.items():
        model = C.package_model(m, state=state, storage=storage)
        plan = model._model().plan()
        if storage == WIN_DENSE:
            assert plan["dense"] == 1 and plan["in_sb"] == 4 and plan["ldw"] == size + size % 2, plan
        model.increment_state(x)
        _note("state sizes", f"{size} {name}", C.check(model.get_state(), want, C.STATE_GATE, name))


@pytest.mark.parametrize("name", list(C.MULTI_STEP))
def test_multi_step_slices(name):
    """Slices of more than one 64-row LDS step (the production path): the prefetched W_in rows carried across a step, the
    clamp at a slice's end, and a last slice shorter than the others."""
    m, state, x = C.cached(C.multi_step_case, name)
    want = C.cached(_multi_step_reference, name)
    for label, storage in STORAGES.items():
        model = C.package_model(m, state=state, storage=storage)
        plan = model._model().plan()
        if storage == WIN_DENSE:
            assert plan["dense"] == 1 and plan["in_sb"] == 32, plan
            if name == "chunk192_short_last":
                assert plan["in_chunk"] >= 192 and _kpad(m) % plan["in_chunk"] != 0, plan
            else:
                assert plan["in_chunk"] == 128 and _kpad(m) % plan["in_chunk"] == 0, plan
            assert (plan["in_split"] - 1) * plan["in_chunk"] < _kpad(m) <= plan["in_split"] * plan["in_chunk"], plan
        else:
            assert plan["dense"] == 0
        model.increment_state(x)
        _note("multi-step slices", f"{name} {label}", C.check(model.get_state(), want, C.STATE_GATE, label))


def _multi_step_reference(name):
    m, state, x = C.cached(C.multi_step_case, name)
    return C.increment(m, state, x)


# ---------------------------------------------------------------------------------------------
# readout
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("out_kind", ["do-nothing", "scale-spatial"])
@pytest.mark.parametrize("square", [False, True], ids=["plain", "square"])
@pytest.mark.parametrize("name", list(C.READOUTS))
def test_readout_tails(name, square, out_kind):
    """The readout's tails: one output, an odd count, the state / hybrid boundary inside a step and inside a group of eight
    rows, a last slice of one row, both square modes (subdomains for the pure models, elements for the hybrid ones), z sizes
    that differ per variable in the hybrid and output transformers."""
    m, state, h = C.readout_case(name, square, out_kind)
    model = C.package_model(m, state=state)
    plan = model._model().plan()
    rows = m["coefficients"].shape[1]
    assert plan["out_chunk"] == 64 and plan["out_split"] == -(-rows // 64), plan
    assert plan["ldc"] == m["coefficients"].shape[2] + m["coefficients"].shape[2] % 2
    if name == "S33_H96":
        assert plan["out_split"] == 3 and rows - 2 * plan["out_chunk"] == 1
    _note("readout", f"{name} {square} {out_kind}", C.check_outputs(_predict(model, h), C.predict(m, state, h), name))


def test_readout_slices_of_two_steps():
    """n_out 8192 and J = 8200 on one subdomain: readout slices of 128 rows, the last one 8 rows long.  No increment: the
    state comes with the model, W_in and W_res are empty."""
    m, state = C.long_readout_case()
    model = C.package_model(m, state=state)
    plan = model._model().plan()
    assert plan["dense"] == 0, plan
    assert plan["out_chunk"] >= 128 and (plan["out_split"] - 1) * plan["out_chunk"] < 8200 < plan["out_split"] * plan["out_chunk"]
    _note("readout", "two-step slices", C.check_outputs(model.predict(), C.predict(m, state), "long readout"))


# ---------------------------------------------------------------------------------------------
# dtypes
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("transformer", list(C.TRANSFORMERS))
@pytest.mark.parametrize("sources", C.SOURCES)
def test_dtype_matrix_of_the_inputs(sources, transformer):
    """float32 / float64 / mixed sources (one plain, one transposed view, one strided view) x the transformer and its mask
    dtype x the input mask's dtype, against numpy's own promotion.  A wrong float32 rounding is five orders of magnitude
    above the state gate."""
    for mask in C.MASKS:
        m, state, x, _ = C.dtype_case(sources, transformer, mask, False)
        want = C.increment(m, state, x)
        model = C.package_model(m, state=state)
        assert model._model().plan()["dense"] == 1
        model.increment_state(_device(x, C.VIEWS))
        _note("dtypes", f"inputs {sources} {transformer} {mask}", C.check(model.get_state(), want, C.STATE_GATE, mask))
        model.set_state(state)
        model.increment_state(x)  # host views
        C.check(model.get_state(), want, C.STATE_GATE, f"{mask} from the host")


@pytest.mark.parametrize("transformer", list(C.TRANSFORMERS))
@pytest.mark.parametrize("sources", C.SOURCES)
def test_dtype_matrix_of_the_hybrid_inputs(sources, transformer):
    for mask in C.MASKS:
        m, state, _, h = C.dtype_case(sources, transformer, mask, True)
        model = C.package_model(m, state=state)
        got = [t.cpu().numpy() for t in model.predict(_device(h, C.VIEWS))]
        _note("dtypes", f"hybrid {sources} {transformer} {mask}", C.check_outputs(got, C.predict(m, state, h), mask))


# ---------------------------------------------------------------------------------------------
# non-finite values
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(C.input_cases()))
def test_non_finite_inputs(name):
    """NaN, +Inf and -Inf in the inputs: the class of every state entry and the finite part against scipy's stored-entry
    product, for CSR and for dense storage of a fully stored W_in; the subdomains that hold no non-finite input are
    bit-identical to the clean run (no atomics)."""
    m, state, clean, planted = C.input_cases()[name]
    want = C.increment(m, state, planted, "stored")
    u_clean, u_planted = C.masked_input(m, clean), C.masked_input(m, planted)
    untouched = [s for s in range(12) if np.isfinite(u_planted[s]).all() and np.array_equal(u_clean[s], u_planted[s])]
    assert 6 <= len(untouched) <= 12
    for label, storage in STORAGES.items():
        model = C.package_model(m, state=state, storage=storage)
        model.increment_state(planted)
        got = model.get_state()
        _note("non-finite", f"{name} {label}", C.check(got, want, C.STATE_GATE, f"{name} {label}"))
        model.set_state(state)
        model.increment_state(clean)
        np.testing.assert_array_equal(got[untouched], model.get_state()[untouched])


@pytest.mark.parametrize("value", list(C.NON_FINITE))
def test_non_finite_hybrid_input(value):
    rng = np.random.RandomState(17)
    m = C.nf_model(rng)
    state = rng.uniform(-1, 1, (12, 41))
    clean = C.make_arrays(rng, (1, 1), m["rank"])
    planted = [a.copy() for a in clean]
    planted[1][3, 4, 0] = C.NON_FINITE[value]  # subdomain 1 + 3 * 1 = 4
    model = C.package_model(m, state=state)
    got = model.predict(planted)
    want = C.predict(m, state, planted)
    _note("non-finite", f"hybrid {value}", C.check_outputs(got, want, value))
    ok = np.ones(m["rank"], bool)
    ok[2:4, 3:6] = False
    for g, w, c in zip(got, want, model.predict(clean)):
        assert not np.isfinite(w[~ok]).any() and np.isfinite(w[ok]).all()
        np.testing.assert_array_equal(g[ok], c[ok])


@pytest.mark.parametrize("name", list(C.state_cases()))
def test_non_finite_state(name):
    """NaN, +Inf and -Inf in the state itself (set_state): W_res carries them to the rows with a stored weight only; an
    infinite pre-activation is exactly +-1 after tanh; +Inf meeting -Inf is NaN."""
    m, state, x = C.state_cases()[name]
    want = C.increment(m, state, x)
    for label, storage in STORAGES.items():
        model = C.package_model(m, storage=storage)
        model.set_state(state)
        np.testing.assert_array_equal(model.get_state(), state)
        model.increment_state(x)
        _note("non-finite", f"state {name} {label}", C.check(model.get_state(), want, C.STATE_GATE, f"{name} {label}"))


@pytest.mark.parametrize("out_kind", ["do-nothing", "scale-spatial"])
def test_predict_from_a_state_with_one_nan_subdomain(out_kind):
    """One NaN in the state of subdomain 5: only its outputs are non-finite, the others are bit-identical to the clean
    state's.  Intercepts of +-1e39 in subdomain 3 overflow the float32 decode to +-Inf as numpy's cast does."""
    rng = np.random.RandomState(23)
    m = C.nf_model(rng, out_kind=out_kind)
    m["intercepts"][3] = 1.0e39 * np.where(np.arange(m["intercepts"].shape[1]) % 2, -1.0, 1.0)
    clean = rng.uniform(-1, 1, (12, 41))
    state = clean.copy()
    state[5, 17] = np.nan
    h = C.make_arrays(rng, (1, 1), m["rank"])
    model = C.package_model(m, state=state)
    got = model.predict(h)
    want = C.predict(m, state, h)
    _note("non-finite", f"predict {out_kind}", C.check_outputs(got, want, out_kind))
    block = np.zeros(m["rank"], bool)
    block[4:6, 3:6] = True  # subdomain 5 = x block 2, y block 1
    model.set_state(clean)
    for g, w, c in zip(got, want, model.predict(h)):
        assert np.isnan(w[block]).all() and not np.isnan(w[~block]).any()
        np.testing.assert_array_equal(g[~block], c[~block])
        if out_kind == "scale-spatial":
            assert np.isposinf(w).any() and np.isneginf(w).any() and w.dtype == np.float32
        else:
            assert np.isfinite(w[~block]).all() and np.abs(w[~block]).max() > 1e38


def test_dense_storage_spreads_a_nan_input_over_the_subdomain():
    """The deliberate difference of DESIGN.md section 12: with part of W_in unstored, dense storage computes the dense
    product (NaN times a padded zero is NaN), CSR storage computes scipy's; AUTO is dense here."""
    m, state, x = C.dense_difference_case()
    stored, dense = C.increment(m, state, x, "stored"), C.increment(m, state, x, "dense")
    assert (C.classes(stored) != C.classes(dense)).any()
    for storage, want in ((WIN_CSR, stored), (WIN_DENSE, dense), (WIN_AUTO, dense)):
        model = C.package_model(m, state=state, storage=storage)
        assert model._model().plan()["dense"] == (storage != WIN_CSR)
        model.increment_state(x)
        _note("non-finite", f"dense difference, storage {storage}", C.check(model.get_state(), want, C.STATE_GATE, str(storage)))


# ---------------------------------------------------------------------------------------------
# sparse structure
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(C.sparse_cases()))
def test_sparse_structure(name):
    """Empty rows, an empty W_in, stored zeros, COO duplicates, unsorted columns, and AUTO on either side of half the entries
    stored.  CSR storage against the stored-entry product, dense storage against the dense product (they differ only where
    a non-finite input meets an unstored entry)."""
    m, state, x, coo, auto_dense = C.sparse_cases()[name]
    wants = {WIN_CSR: C.increment(m, state, x, "stored"), WIN_DENSE: C.increment(m, state, x, "dense")}
    assert np.isfinite(wants[WIN_CSR]).any()
    results = {}
    for storage in (WIN_CSR, WIN_DENSE, WIN_AUTO):
        w_in = SparseMatrix("coo", (41, 32), coo) if coo is not None else None
        model = C.package_model(m, state=state, storage=storage, w_in=w_in)
        dense = model._model().plan()["dense"]
        if storage == WIN_AUTO:
            if auto_dense is not None:
                assert dense == auto_dense, (name, dense)
        else:
            assert dense == (storage == WIN_DENSE)
        model.increment_state(x)
        results[storage] = model.get_state()
        _note("sparse", f"{name} storage {storage}",
              C.check(results[storage], wants[WIN_DENSE if dense else WIN_CSR], C.STATE_GATE, f"{name} {storage}"))
    if np.isfinite(wants[WIN_DENSE]).all():
        C.check(results[WIN_DENSE], results[WIN_CSR], 2 * C.STATE_GATE, "dense against CSR")


# ---------------------------------------------------------------------------------------------
# graph replay and the state across the parity of its double buffer
# ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("hybrid, warmup, storage", [(False, 2, WIN_DENSE), (True, 1, WIN_CSR), (True, 2, WIN_DENSE)],
                         ids=["pure-even", "hybrid-odd", "hybrid-even"])
def test_graph_replay_steps_like_eager(hybrid, warmup, storage):
    """One increment + predict captured by ``GraphedCall`` (at an even or an odd parity of the state's double buffer) and
    replayed three times, new data copied into the captured inputs before each: the state and the outputs after every
    replay are bit-identical to an eager model's, and eager steps continue from the last replay."""
    rng = np.random.RandomState(31)
    m = C.make_model(rng, (2, 3), (2, 3), overlap=1, state_size=41, in_sizes=(2, 1), out_sizes=(1, 2),
                     hybrid_sizes=(1, 2) if hybrid else None, input_mask=np.float64, square=True)
    state0 = rng.uniform(-1, 1, (6, 41))
    series = [(C.make_arrays(rng, (2, 1), C.ov_extent(m)), C.make_arrays(rng, (1, 2), m["rank"]) if hybrid else None)
              for _ in range(5)]
    graphed = C.package_model(m, state=state0, storage=storage)._model()
    eager = C.package_model(m, state=state0, storage=storage)._model()
    x = _device(series[0][0])
    h = _device(series[0][1]) if hybrid else None

    def step():
        graphed.increment(x)
        return graphed.predict(h)

    call = GraphedCall(step, warmup=warmup)
    graphed.set_state(state0)  # the warm-up steps moved it
    state = state0
    for t in range(1, 4):
        for held, new in zip(x + (h or []), _device(series[t][0]) + (_device(series[t][1]) if hybrid else [])):
            held.copy_(new)
        outs = call.replay()
        eager.increment(_device(series[t][0]))
        expect = eager.predict(_device(series[t][1]) if hybrid else None)
        assert torch.equal(graphed.get_state(), eager.get_state()), f"state after replay {t}"
        for o, e in zip(outs, expect):
            assert torch.equal(o, e), f"outputs after replay {t}"
        state = C.increment(m, state, series[t][0])
    C.check(graphed.get_state().cpu().numpy(), state, 3 * C.STATE_GATE, "three replays against the restatement")
    C.check_outputs([o.cpu().numpy() for o in outs], C.predict(m, state, series[3][1]), "outputs of the last replay")
    for model in (graphed, eager):
        model.increment(_device(series[4][0]))
    assert torch.equal(graphed.get_state(), eager.get_state())
    for o, e in zip(graphed.predict(_device(series[4][1]) if hybrid else None),
                    eager.predict(_device(series[4][1]) if hybrid else None)):
        assert torch.equal(o, e)
    C.check(graphed.get_state().cpu().numpy(), C.increment(m, state, series[4][0]), 4 * C.STATE_GATE, "eager after replay")


@pytest.mark.parametrize("increments", [1, 2], ids=["odd", "even"])
def test_state_bookkeeping_across_parity(increments):
    """get_state, get_model_from_subdomain, set_state and reset_state after an odd and an even number of increments (the
    state is double-buffered; each of them must see the current half)."""
    rng = np.random.RandomState(37)
    m = C.make_model(rng, (3, 2), (2, 3), overlap=1, state_size=41, in_sizes=(1, 2), out_sizes=(2,), input_mask=np.float64)
    state = rng.uniform(-1, 1, (6, 41))
    series = [C.make_arrays(rng, (1, 2), C.ov_extent(m)) for _ in range(4)]
    model = C.package_model(m, state=state)
    for t in range(increments):
        model.increment_state(series[t])
        state = C.increment(m, state, series[t])
    got = model.get_state()
    C.check(got, state, increments * C.STATE_GATE, "get_state")
    full = model.predict()
    C.check_outputs(full, C.predict(m, state), "predict")
    for i, sub in enumerate(fit.split_multi_subdomain_model(model)):
        np.testing.assert_array_equal(sub.get_state()[0], got[i])
        x0, y0 = (i % 3) * 2, (i // 3) * 3
        np.testing.assert_array_equal(sub.predict()[0], full[0][x0:x0 + 2, y0:y0 + 3])
    # set_state at this parity, a step, reset_state at the other parity, a step
    other = rng.uniform(-1, 1, (6, 41))
    model.set_state(other)
    np.testing.assert_array_equal(model.get_state(), other)
    model.increment_state(series[2])
    C.check(model.get_state(), C.increment(m, other, series[2]), C.STATE_GATE, "after set_state")
    model.reset_state()
    np.testing.assert_array_equal(model.get_state(), np.zeros((6, 41)))
    C.check_outputs(model.predict(), C.predict(m, np.zeros((6, 41))), "predict after reset_state")
    model.increment_state(series[3])
    C.check(model.get_state(), C.increment(m, np.zeros((6, 41)), series[3]), C.STATE_GATE, "after reset_state")
