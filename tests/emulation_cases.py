"""Draws, edge-case builders and the gate shared by the Zhao-Carr post-processing tests (``test_gpu_emulation*.py`` on the
device, ``test_oracle_emulation.py`` on the host).  Everything here is numpy; truth is ``oracle/emulation_np.py``.

The gate (``check``): the set of NaN, +Inf and -Inf outputs equals the oracle's position for position, and every finite
output lies within ``rtol * max(|oracle|, |operand|) + atol`` of the oracle, where ``operand`` is the state field the
correction was added to.  The edge draws hold exact cancellations (a squashed cloud of 0 gives ``cloud_g - cloud_g``, a net
condensation limited to ``-cloud_in`` gives ``cloud_in - cloud_in``), so ``|oracle|`` alone is no scale for the rounding
of the sum.  ``rtol`` is 1e-12 where the arithmetic is float64 and 2e-6 where it is float32; the all-float32 strict
precipitation scan has 5e-5 relative with 1e-9 absolute, since the reference accumulates that one in float64."""
import numpy as np

from oracle import emulation_np as E

GRID_CAP = 16384 * 256   # threads of the capped grid of the grid-stride kernels
SCAN_SEGMENTS = 256      # per-thread segments of a row in the phase-dependent flag scan
NON_FINITE = {"nan": np.nan, "posinf": np.inf, "neginf": -np.inf}
GSCOND_OPERAND = {E.CLOUD_G: E.CLOUD_IN, E.QV_G: E.QV_IN, E.T_G: E.T_IN}
PRECPD_OPERAND = {E.CLOUD_P: E.CLOUD_G, E.QV_P: E.QV_G, E.T_P: E.T_G}
GSCOND_MODES = ["none", "fortran_vanishes", "fortran_identical", "class_zero_cloud", "class_zero_tend"]


def state(rng, n0=79, n1=257, dt=np.float64):
    t = rng.uniform(230, 300, (n0, n1))
    qv = 10 ** rng.uniform(-6, -2, (n0, n1))
    qc = np.where(rng.random((n0, n1)) < 0.5, 0.0, 10 ** rng.uniform(-9, -3, (n0, n1)))
    state = {E.T_IN: t, E.QV_IN: qv, E.CLOUD_IN: qc, E.DELP: rng.uniform(300, 1500, (n0, n1))}
    dq = rng.normal(0, 2e-4, (n0, n1))
    state[E.CLOUD_G] = np.where(rng.random((n0, n1)) < 0.3, qc, np.maximum(qc + dq, 0))
    state[E.QV_G] = qv - (state[E.CLOUD_G] - qc)
    state[E.T_G] = t + 2.5e6 / 1004.6 * (state[E.CLOUD_G] - qc)
    return {k: v.astype(dt) for k, v in state.items()}


def emulator(rng, state, dt=np.float32):
    sh = state[E.T_IN].shape
    em = {
        E.CLOUD_G: state[E.CLOUD_IN] + rng.normal(0, 3e-4, sh),
        E.QV_G: state[E.QV_IN] + rng.normal(0, 3e-4, sh),
        E.T_G: state[E.T_IN] + rng.normal(0, 1, sh),
        E.CLOUD_P: state[E.CLOUD_G] + rng.normal(0, 3e-4, sh),
        E.QV_P: state[E.QV_G] + rng.normal(0, 3e-4, sh),
        E.T_P: state[E.T_G] + rng.normal(0, 1, sh),
        E.PRECIP: rng.uniform(0, 1e-3, sh[1]),
        "gscond_classes": rng.normal(0, 1, (4,) + sh),
        "precpd_classes": rng.normal(0, 1, (4,) + sh),
    }
    return {k: v.astype(dt) for k, v in em.items()}


def draw(seed, n0=79, n1=257, sdt=np.float64, edt=np.float32, adt=None):
    """An ordinary (state, emulator) pair; ``adt`` is the dtype of the auxiliary operands (the Fortran scheme's cloud for the
    two state masks, the class logits for the classifier masks), the emulator's by default."""
    rng = np.random.default_rng(seed)
    st = state(rng, n0, n1, sdt)
    em = emulator(rng, st, edt)
    if adt is not None:
        st[E.CLOUD_G] = st[E.CLOUD_G].astype(adt)
        em["gscond_classes"] = em["gscond_classes"].astype(adt)
        em["precpd_classes"] = em["precpd_classes"].astype(adt)
    return st, em


def poke(a, rng, value, count=7):
    """A copy of ``a`` with ``value`` at ``count`` scattered elements."""
    out = np.array(a, copy=True)
    flat = out.reshape(-1)
    flat[rng.choice(flat.size, size=min(count, flat.size), replace=False)] = value
    return out


def neighbours(x, dt):
    """``x`` rounded to ``dt`` with the representable number below and above it."""
    v = np.dtype(dt).type(x)
    return np.array([np.nextafter(v, dt(-np.inf)), v, np.nextafter(v, dt(np.inf))], dtype=dt)


def scatter(a, rng, values, each=5):
    """``each`` scattered elements of ``a`` (in place) set to every one of ``values``; returns the flat positions."""
    flat = a.reshape(-1)
    pos = rng.choice(flat.size, size=min(each * len(values), flat.size), replace=False)
    flat[pos] = np.resize(np.asarray(values, dtype=a.dtype), pos.size)
    return pos


def at_thresholds(st, em, seed, bound=1e-4):
    """(state, emulator) with scattered operands exactly at each comparison of the gscond / precpd kernels:
    emulator cloud == the squash bound (and its neighbours, in the emulator's dtype); Fortran cloud == 1e-15 (and neighbours);
    Fortran cloud == input cloud; net condensation == available vapour, == -available liquid, and one step beyond each;
    precipitation source == 0 and sink == 0 (after-precpd field == after-gscond field)."""
    rng = np.random.default_rng(seed)
    st = {k: np.array(v, copy=True) for k, v in st.items()}
    em = {k: np.array(v, copy=True) for k, v in em.items()}
    for key in (E.CLOUD_G, E.CLOUD_P):
        scatter(em[key], rng, neighbours(bound, em[key].dtype.type), each=6)
    scatter(st[E.CLOUD_G], rng, neighbours(1e-15, st[E.CLOUD_G].dtype.type), each=6)
    pos = rng.choice(st[E.CLOUD_IN].size, 40, replace=False)
    st[E.CLOUD_G].reshape(-1)[pos] = st[E.CLOUD_IN].reshape(-1)[pos]
    # net == available vapour: no liquid, emulator cloud == humidity (values that every dtype here holds exactly)
    pos = rng.choice(st[E.CLOUD_IN].size, 60, replace=False)
    qv = (10 ** rng.uniform(-5, -2, pos.size)).astype(np.float32)
    st[E.CLOUD_IN].reshape(-1)[pos] = 0
    st[E.QV_IN].reshape(-1)[pos] = qv
    em[E.CLOUD_G].reshape(-1)[pos] = np.where(np.arange(pos.size) % 3 == 0, qv,
                                              np.where(np.arange(pos.size) % 3 == 1, np.nextafter(qv, np.float32(1)),
                                                       np.nextafter(qv, np.float32(0))))
    # net == -available liquid: emulator cloud 0 and -0, and a cloud just below zero
    pos = rng.choice(st[E.CLOUD_IN].size, 60, replace=False)
    st[E.CLOUD_IN].reshape(-1)[pos] = (10 ** rng.uniform(-7, -3, pos.size)).astype(np.float32)
    em[E.CLOUD_G].reshape(-1)[pos] = np.resize(np.array([0.0, -0.0, -1e-30, 1e-30], dtype=np.float32), pos.size)
    # precipitation source / sink exactly zero
    for ekey, skey in ((E.CLOUD_P, E.CLOUD_G), (E.QV_P, E.QV_G)):
        pos = rng.choice(st[skey].size, 60, replace=False)
        v = st[skey].reshape(-1)[pos].astype(np.float32)
        st[skey].reshape(-1)[pos] = v
        em[ekey].reshape(-1)[pos] = v
    return st, em


def threshold_temperatures(shape, seed, dt=np.float32):
    """Temperatures drawn from ``dt(273.16)``, ``dt(258.16)`` and their two neighbours each (the flag scan's two
    comparisons), with a cold element here and there so that there is a flag to carry."""
    rng = np.random.default_rng(seed)
    values = np.concatenate([neighbours(273.16, dt), neighbours(258.16, dt)])
    t = values[rng.integers(0, values.size, shape)]
    return np.where(rng.random(shape) < 0.05, dt(250.0), t).astype(dt)


def scan_rows(n1, seed, dt=np.float64):
    """(temperature, cloud, labels) rows of length ``n1`` whose flags stress the chain of the 256 scan segments.  The scan
    runs from the END of a row; segment ``j`` covers ``[n1 - (j + 1) seg, n1 - j seg)`` with ``seg = ceil(n1 / 256)``."""
    rng = np.random.default_rng(seed)
    seg = -(-n1 // SCAN_SEGMENTS)
    carry_t, cold, warm = 265.0, 250.0, 280.0
    rows_t, rows_c, labels = [], [], []

    def add(t, c, label):
        rows_t.append(t)
        rows_c.append(c)
        labels.append(label)

    t = np.full(n1, carry_t)
    t[-1] = cold
    add(t, np.full(n1, 1e-5), "all carry, last cold: the flag crosses every segment")
    for j in (1, 2, 128, 255) if n1 > 4 else (1,):
        border = n1 - j * seg
        for off in (-1, 0, 1):
            p = border + off
            if not 0 <= p < n1 - 1:
                continue
            t2 = t.copy()
            t2[p] = warm
            add(t2, np.full(n1, 1e-5), f"one warm element at segment border {j} {off:+d}")
    t3 = t.copy()
    c3 = neighbours(1e-20, dt)[rng.integers(0, 3, n1)].astype(np.float64)
    add(t3, c3, "cloud at 1e-20 and its neighbours")
    c4 = np.full(n1, 1e-5)
    c4[rng.integers(0, n1, max(1, n1 // 500))] = neighbours(1e-20, dt)[1]
    add(t3, c4, "a few clouds exactly at 1e-20")
    t5 = np.where(rng.random(n1) < 0.01, cold, rng.uniform(258.2, 273.1, n1))
    t5[rng.integers(0, n1, max(1, n1 // 300))] = warm
    add(t5, np.where(rng.random(n1) < 0.98, 1e-5, 0.0), "random runs")
    return np.array(rows_t, dtype=dt), np.array(rows_c, dtype=dt), labels


def logit_edge_columns(dt=np.float32):
    """[4, n] class logits: a NaN in class 0, in a middle class, in each asked-for class (zero_cloud = 2,
    zero_tendency = 3, and the positive / negative pair 0, 1), in all classes; exact ties between two and between all
    classes; infinities; and ordinary columns around them."""
    nan, inf = np.nan, np.inf
    cols = [
        [0.0, nan, 1.0, 0.5],      # the issue's example: nothing is hot
        [nan, 0.3, 1.0, 0.5],      # class 0
        [0.1, nan, 0.2, 0.5],      # a middle class
        [0.1, 0.3, nan, 0.5],      # the asked-for class (zero_cloud)
        [0.1, 0.3, 0.2, nan],      # the asked-for class (zero_tendency), last
        [nan, nan, nan, nan],
        [nan, 0.3, nan, 0.5],
        [1.0, 1.0, 0.2, 0.5],      # ties between two
        [0.1, 0.3, 0.7, 0.7],
        [0.7, 0.3, 0.7, 0.5],
        [0.25, 0.25, 0.25, 0.25],  # ties between all
        [0.0, -0.0, 0.0, -0.0],
        [inf, 0.3, inf, 0.5],
        [-inf, -inf, -inf, -inf],
        [inf, nan, 0.2, 0.5],
        [0.1, 0.3, 0.2, 0.5],
        [0.9, 0.3, 0.2, 0.5],
        [0.1, 0.3, 0.9, 0.5],
    ]
    return np.array(cols, dtype=dt).T.copy()


def logits_with_edges(shape, seed, dt=np.float32):
    """[4, *shape] ordinary logits with the edge columns of ``logit_edge_columns`` scattered over the plane."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    logits = rng.normal(0, 1, (4, n)).astype(dt)
    edges = logit_edge_columns(dt)
    pos = rng.choice(n, size=min(n, 6 * edges.shape[1]), replace=False)
    logits[:, pos] = edges[:, np.arange(pos.size) % edges.shape[1]]
    return logits.reshape((4,) + tuple(shape))


def rtol_of(*dtypes):
    """The gate's relative figure for arithmetic in the numpy promotion of ``dtypes``."""
    return 1e-12 if np.result_type(*dtypes) == np.float64 else 2e-6


def check(res, ref, name, rtol, atol=0.0, operand=None):
    """The gate of the module docstring, every element included.  Prints the worst error as a fraction of the gate and the
    number of elements that are not identical to the oracle's (NaN == NaN, -0 == 0); returns both."""
    res, ref = np.asarray(res), np.asarray(ref)
    assert res.shape == ref.shape, f"{name}: shape {res.shape} != {ref.shape}"
    assert res.dtype == ref.dtype, f"{name}: dtype {res.dtype} != {ref.dtype}"
    for what, pick in (("NaN", np.isnan), ("+Inf", np.isposinf), ("-Inf", np.isneginf)):
        a, b = pick(res), pick(ref)
        assert np.array_equal(a, b), (f"{name}: {what} at {int(a.sum())} outputs, the oracle has {int(b.sum())}; "
                                      f"first difference at {tuple(np.argwhere(a != b)[0])}")
    fin = np.isfinite(ref)
    scale = np.abs(ref.astype(np.float64))
    if operand is not None:
        op = np.broadcast_to(np.asarray(operand, dtype=np.float64), ref.shape)
        scale = np.maximum(scale, np.where(np.isfinite(op), np.abs(op), 0.0))
    err = np.abs(res.astype(np.float64)[fin] - ref.astype(np.float64)[fin])
    gate = rtol * scale[fin] + atol
    different = int(np.sum(~((res == ref) | (np.isnan(res) & np.isnan(ref)))))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / gate)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{name} [{res.dtype}]: worst error / gate = {worst:.3g}, not identical to the oracle: {different} of {res.size}")
    assert worst <= 1.0, (f"{name}: error {worst:.3g} x the gate (rtol {rtol:g}, atol {atol:g}) at finite element "
                          f"{int(np.argmax(ratio))}; {int(np.sum(ratio > 1))} outside")
    return worst, different


def precpd_gate(st, em):
    """(rtol, atol) of the strict scan: the all-float32 call is the one the reference accumulates in float64."""
    if np.result_type(*(st[k] for k in (E.CLOUD_G, E.QV_G, E.T_G, E.DELP)), em[E.CLOUD_P], em[E.QV_P]) == np.float32:
        return 5e-5, 1e-9
    return 1e-12, 0.0


def column_mass(st):
    """The water column before precpd as ``conservative_precip_simple`` forms it [m of liquid water]: the operand of its
    ``before - after``."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sum((st[E.QV_G] + st[E.CLOUD_G]).astype(np.float64) * st[E.DELP] / E.GRAVITY, axis=0) / E.RHO_WATER
