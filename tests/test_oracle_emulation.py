"""The post-processing oracle against the reference's own known answers
(external/emulation/tests/test_zhao_carr.py:15-147, test_mask.py:7-47, _regtest_outputs/*.out)."""
import numpy as np
import pytest

from oracle import emulation_np as E


def test_limit_net_condensation_known_answer():
    qv = np.array([[1, 1, 1], [0, 0, 0]], dtype=np.float64)
    qc = np.array([[0, 0, 0], [1, 1, 0]], dtype=np.float64)
    net = np.array([[1.5, 0.5, 0], [-1.5, -0.5, 0]], dtype=np.float64)
    res = E.limit_net_condensation({E.CLOUD_IN: qc, E.QV_IN: qv}, net)
    np.testing.assert_array_equal(res, np.array([[1, 0.5, 0], [-1, -0.5, 0]]))


def test_ice_water_flag_known_answers():
    iw = E.ice_water_flag(np.array([[10, 0, -10, -15, -16]]), np.array([[0, 0, 0, 1, 0]]))
    np.testing.assert_array_equal(iw, np.array([[0, 0, 0.0, 1.0, 1.0]]))
    iw = E.ice_water_flag(np.array([[-14, -16]]), np.array([[0, 0]]))
    np.testing.assert_array_equal(iw, np.array([[0, 1.0]]))


def test_regtest_scalars():
    assert E.latent_heat_phase_dependent(0.5) == 2666790.0
    assert np.array(10.0) / E.RHO_WATER == 0.01
    assert np.array(2.0) * np.array(1.0) / E.GRAVITY == 0.20394324259558566


def test_strict_precip_scan_known_answer():
    c, v, total = E.strict_precip_scan(np.array([[1.0], [-2.0], [3.0]]), np.array([[4.0], [-1.0], [2.0]]))
    np.testing.assert_equal(c, [[1.0], [0.0], [3.0]])
    np.testing.assert_equal(v, [[2.0], [0.0], [2.0]])
    np.testing.assert_equal(total, np.zeros_like(total))


def _states():
    shp = (5, 10)
    state = {E.CLOUD_G: np.ones(shp) * 4, E.QV_G: np.ones(shp), E.T_G: np.ones(shp) * 10, E.DELP: np.ones(shp)}
    emulator = {E.CLOUD_P: np.ones(shp) * 2, E.QV_P: np.ones(shp) * 2}
    return state, emulator


def test_enforce_conservative_precpd_properties():
    state, emulator = _states()
    res = E.enforce_conservative_precpd(state, emulator)
    assert E.PRECIP in res and E.T_P in res
    dummy = -1 * np.ones_like(state[E.QV_G])
    res = E.enforce_conservative_precpd(state, {E.CLOUD_P: dummy * -10, E.QV_P: dummy, E.T_P: dummy, E.PRECIP: dummy})
    for v in res.values():
        assert not np.any(v == -1)
    assert not np.any(res[E.CLOUD_P] == 10)


def test_simple_conservative_overwrites_precip():
    state, emulator = _states()
    res = E.conservative_precip_simple(state, emulator)
    res[E.PRECIP] = -1 * np.ones_like(res[E.PRECIP])
    assert not np.any(E.conservative_precip_simple(state, res)[E.PRECIP] == -1)


def test_range_mask_known_answers():
    assert E.range_mask({"foo": 0.5}, "foo", 0, 1) == {"foo": 0.5}
    assert E.range_mask({"foo": 1.5}, "foo", 0, 1) == {"foo": 1.0}
    assert E.range_mask({"foo": -1.5}, "foo", 0, 1) == {"foo": 0}


@pytest.mark.parametrize("start, stop", [(2, 3), (2, 5), (None, 2), (None, None)])
def test_level_mask_known_answers(start, stop):
    ones = np.ones((4, 2))
    zeros = ones * 0
    res = E.level_mask({"foo": zeros}, {"foo": ones}, "foo", start, stop)
    sl = slice(start, stop)
    np.testing.assert_array_equal(res["foo"][sl], zeros[sl])
    assert np.sum(res["foo"]) == res["foo"].size - zeros[sl].size
    res = E.level_mask({}, {"foo": ones}, "foo", 0, 2, fill_value=0.5)
    np.testing.assert_array_equal(0.5, res["foo"][:2])
    a = ones * 1.1
    res = E.level_mask({"a": a}, {"foo": ones}, "foo", 0, 2, fill_value="a")
    np.testing.assert_array_equal(a[:2], res["foo"][:2])


# ---------------------------------------------------------------------------------------------------------
# the checker at numpy's edges (what tests/test_gpu_emulation_edges.py holds the device to)
# ---------------------------------------------------------------------------------------------------------
def test_precpd_nan_hand_example():
    """A NaN cloud after precpd in the middle level of three: np.maximum / np.minimum carry it into that level's cloud,
    into humidity and temperature from there down (the scan runs from the last level to the first) and into the column's
    precipitation; the level above it stays finite."""
    z = np.zeros((3, 1))
    state = {E.CLOUD_G: z, E.QV_G: z, E.T_G: z, E.DELP: np.full_like(z, E.GRAVITY)}
    emulator = {E.CLOUD_P: -np.array([[1.0], [np.nan], [3.0]]), E.QV_P: np.array([[4.0], [1.0], [2.0]])}
    with np.errstate(invalid="ignore"):
        res = E.enforce_conservative_precpd(state, emulator)
    assert np.isnan(res[E.CLOUD_P]).ravel().tolist() == [False, True, False]
    np.testing.assert_allclose(res[E.CLOUD_P][[0, 2], 0], [-1.0, -3.0], rtol=1e-15)
    for key in (E.QV_P, E.T_P):
        assert np.isnan(res[key]).ravel().tolist() == [True, True, False], key
    np.testing.assert_allclose(res[E.QV_P][2, 0], 2.0, rtol=1e-15)
    assert np.isnan(res[E.PRECIP]).tolist() == [True]


def test_classify_nan_logits_and_ties():
    """``logits == np.max(logits, axis=0)``: a NaN among a column's classes leaves no class hot, wherever it sits; every
    tied maximum is hot."""
    nan = np.nan
    with np.errstate(invalid="ignore"):
        hot = lambda column: [bool(E.classify(np.array(column, dtype=np.float64)[:, None])[name][0]) for name in E.CLASSES]  # noqa: E731
        assert hot([0, nan, 1, 0.5]) == [False] * 4      # a kernel that skips the NaN makes class 2 hot
        assert hot([nan, 0.3, 1, 0.5]) == [False] * 4
        assert hot([0.1, 0.3, nan, 0.5]) == [False] * 4
        assert hot([0.1, 0.3, 0.2, nan]) == [False] * 4
        assert hot([nan] * 4) == [False] * 4
    assert hot([1.0, 1.0, 0.2, 0.5]) == [True, True, False, False]
    assert hot([0.1, 0.7, 0.2, 0.7]) == [False, True, False, True]
    assert hot([0.25] * 4) == [True] * 4
    assert hot([0.0, -0.0, 0.0, -0.0]) == [True] * 4
    assert hot([-np.inf] * 4) == [True] * 4
    assert hot([0.1, 0.3, 0.9, 0.5]) == [False, False, True, False]


def test_limit_net_condensation_nan_operands():
    """np.where drops a NaN net condensation (both branches take the 0), np.maximum / np.minimum propagate a NaN in the
    available liquid or vapour."""
    one = np.ones((1, 1))
    state = {E.CLOUD_IN: one, E.QV_IN: one}
    assert E.limit_net_condensation(state, one * np.nan)[0, 0] == 0.0
    for key in (E.CLOUD_IN, E.QV_IN):
        for net in (0.5, -0.5, 0.0):
            with np.errstate(invalid="ignore"):
                assert np.isnan(E.limit_net_condensation({**state, key: one * np.nan}, one * net)[0, 0]), (key, net)
    # ... and so does the update built on it: NaN humidity in, NaN cloud / humidity / temperature out
    with np.errstate(invalid="ignore"):
        res = E.update_with_net_condensation(one * 1.5, {**state, E.QV_IN: one * np.nan, E.T_IN: one * 280.0}, {})
    assert all(np.isnan(res[k][0, 0]) for k in (E.CLOUD_G, E.QV_G, E.T_G))


def _float32_against_float64(st, em, label, skip_at_bound=False):
    """Worst error of the oracle on float32 operands against the oracle on the same values in float64, as a fraction of
    the gate of ``emulation_cases.check`` (float32 figures), per family of outputs."""
    import emulation_cases as C

    up = lambda d: {k: v.astype(np.float64) for k, v in d.items()}  # noqa: E731
    s64, e64 = up(st), up(em)
    worst = {}

    def gate(family, r32, r64, rtol, atol=0.0, operand=None, keep=None):
        r32 = np.asarray(r32)
        if keep is not None:
            r32, r64 = r32[keep], r64[keep]
            operand = None if operand is None else np.broadcast_to(operand, keep.shape)[keep]
        w, _ = C.check(r32.astype(np.float64), r64, f"{label}: {family}", rtol, atol, operand)
        worst[family] = max(worst.get(family, 0.0), w)

    with np.errstate(all="ignore"):
        for mode in C.GSCOND_MODES:
            for phase in (False, True):
                a = E.update_with_net_condensation(E.gscond_cloud_choice(st, em, mode), st, em, phase_dependent=phase)
                b = E.update_with_net_condensation(E.gscond_cloud_choice(s64, e64, mode), s64, e64, phase_dependent=phase)
                for k, op in C.GSCOND_OPERAND.items():
                    gate("gscond", a[k], b[k], 2e-6, operand=s64[op])
        for ckey, qkey in ((E.CLOUD_G, E.QV_G), (E.CLOUD_P, E.QV_P)):
            # (a cloud exactly at float32(bound) is below 1e-4 as a float64 and not below it as a float32: a decision that
            # belongs to the dtype, not a rounding error -- the threshold draws put six clouds there)
            keep = em[ckey] != np.float32(1e-4) if skip_at_bound else None
            a, b = E.squash(em[ckey], em[qkey], 1e-4), E.squash(e64[ckey], e64[qkey], 1e-4)
            gate("squash", a[0], b[0], 2e-6, keep=keep)
            gate("squash", a[1], b[1], 2e-6, operand=e64[qkey], keep=keep)
        a, b = E.infer_gscond_cloud_from_conservation(st, em), E.infer_gscond_cloud_from_conservation(s64, e64)
        gate("inferred cloud", a[E.CLOUD_G], b[E.CLOUD_G], 2e-6, operand=s64[E.CLOUD_IN])
        a, b = E.enforce_conservative_precpd(st, em), E.enforce_conservative_precpd(s64, e64)
        for k in (E.CLOUD_P, E.QV_P, E.T_P, E.PRECIP):
            gate("strict scan", a[k], b[k], 5e-5, 1e-9, s64[C.PRECPD_OPERAND[k]] if k in C.PRECPD_OPERAND else None)
        a, b = E.conservative_precip_simple(st, em), E.conservative_precip_simple(s64, e64)
        gate("simple budget", a[E.PRECIP], b[E.PRECIP], 2e-6, operand=C.column_mass(s64))
    return worst


def test_float32_oracle_stays_inside_the_gate():
    """The gate of the device tests is met by the reference arithmetic itself: float32 against float64 evaluation of the
    oracle on the ordinary, non-finite and threshold draws of ``emulation_cases`` (``check`` asserts it, non-finite
    positions included; run with ``-s`` for the figures quoted in ``test_gpu_emulation_edges.py``)."""
    import emulation_cases as C

    st, em = C.draw(21, sdt=np.float32, edt=np.float32)
    worst = {}
    draws = [("ordinary", st, em, False)]
    rng = np.random.default_rng(22)
    for name, value in C.NON_FINITE.items():
        draws.append((name, {k: C.poke(v, rng, value) for k, v in st.items()}, {k: C.poke(v, rng, value) for k, v in em.items()}, False))
    draws.append(("thresholds",) + C.at_thresholds(st, em, seed=42) + (True,))
    for label, s, e, at_bound in draws:
        for family, w in _float32_against_float64(s, e, label, at_bound).items():
            worst[family] = max(worst.get(family, 0.0), w)
    print("float32 oracle against float64 oracle, worst error / gate:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0
