"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of ``fv3hip_train_precip_loss_grad`` (csrc/mlp_train.hip, DESIGN.md
section 25) -- the loss behind the closure of the precipitative model and its gradient with respect to the raw head outputs --
and of a whole training step, with the bounds the tests hold the float32 kernels to.  Nothing here is chosen by hand: every
bound counts the float32 operations of the stated evaluation order at ``U = 2^-24`` each (first order), doubled as
``train_np.dot_bound`` doubles (slack for the casts of this float64 reference).

With ``x^`` the raw head outputs, ``f_i = 2 inv_i w_i`` and M1 = |t^ s1| + |c1| + couple |c_heat| (|cp^ s2| + |c2|) (M2 alike):

    t, q, cp        one product, one sum:                     2 U (|x^ s| + |c|)
    dq1, dq2        + one product, one sum:                   4 U M
    e1, e2          + one difference:                         5 U (M + |T|)
    g1, g2          + three products (the 2 is exact):        8 U (M + |T|) |f|
    precip          the predictor's figure plus the error cp carries into the integral:
                    (nz + 2) U (|pp| + |c_g| sum |cp delp|) + |c_g| sum e_cp |delp|
    e3, g3          (E_precip + 4 U (|precip| + |T3|)) |f3|
    dt^, dq^        g s + r: e_g |s| + 2 U |g s| + 4 U |r|,   r = (l1 sign + 2 l2 x) / n: three roundings and the sum's
    dcp^            ((c_heat g1 + g2) + (c_g delp) g3) s2:
                    |s2| (|c_heat| e_g1 + e_g2 + |c_g delp| e_g3 + 4 U (|c_heat g1| + |g2| + |c_g delp g3|))

``e_yhat`` (the bound the forward pass puts on ``yhat``) is carried through the same expressions, which are linear in ``yhat``
but for ``sign``: a ``t^`` within its bound of zero may take either sign, so ``2 l1 / n`` is added there.
"""
import numpy as np

from precipitative_np import C_G, C_HEAT
from train_np import U, _contract, _f64, rows


def _gather(a, idx, rows_total, fill):
    """Rows ``idx`` of a resident array; a row outside ``[0, rows_total)`` reads as ``fill``."""
    a = _f64(a)
    if idx is None:
        return a
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < rows_total)
    out = a[np.where(ok, idx, 0)]
    out = out.copy()
    out[~ok] = fill
    return out


def weights(n, nz):
    """(w12, w3) as the entry point forms them: float32 of 1 / (n nz) and of 1 / n."""
    return np.float32(1.0 / (float(n) * float(nz))), np.float32(1.0 / float(n))


def loss_grad(yhat, scale1, center1, scale2, center2, inv1, inv2, inv3, delp, pp, t1, t2, t3, idx=None, couple=True, has_dead=False,
              l1=0.0, l2=0.0, e_yhat=None):
    """``(dY, loss, dY bound, loss bound, predictions)`` for ``yhat [n, 3 nz + has_dead]`` laid out ``t | q | dead | cp``;
    ``predictions`` is ``{"dq1", "dq2", "precip"}`` in float64.  ``l1`` / ``l2`` are taken as their float32 values."""
    yhat = _f64(yhat)
    n = yhat.shape[0]
    nz = (yhat.shape[1] - int(has_dead)) // 3
    assert yhat.shape[1] == 3 * nz + int(has_dead)
    s1, c1, s2, c2, inv1, inv2 = (_f64(np.asarray(v, np.float32)) for v in (scale1, center1, scale2, center2, inv1, inv2))
    inv3, l1, l2 = float(np.float32(inv3)), float(np.float32(l1)), float(np.float32(l2))
    total = _f64(delp).shape[0]
    d = _gather(delp, idx, total, 0.0)[:n]
    p0 = _gather(pp, idx, total, 0.0)[:n]
    T1, T2, T3 = (_gather(a, idx, total, np.nan)[:n] for a in (t1, t2, t3))
    w12, w3 = (float(w) for w in weights(n, nz))
    ch, cg = float(C_HEAT), float(C_G)

    def cpl(v):   # a term that exists only under coupling (not 0 * v: a NaN there must not leak into the uncoupled graph)
        return v if couple else 0.0

    cp0 = 2 * nz + int(has_dead)
    th, qh, xh = yhat[:, :nz], yhat[:, nz:2 * nz], yhat[:, cp0:]
    ey = np.zeros_like(yhat) if e_yhat is None else _f64(e_yhat)
    e_th, e_qh, e_xh = ey[:, :nz], ey[:, nz:2 * nz], ey[:, cp0:]
    reg = l1 != 0.0 or l2 != 0.0

    def r(x):
        return (l1 * np.sign(x) + 2 * l2 * x) / n if reg else np.zeros_like(x)

    def r_abs(x):
        return (l1 * np.abs(np.sign(x)) + 2 * l2 * np.abs(x)) / n if reg else np.zeros_like(x)

    def r_in(x, e):   # what an error e of x does to r(x)
        return (2 * l2 * e + np.where(np.abs(x) <= e, 2 * l1, 0.0)) / n if reg else np.zeros_like(x)

    with np.errstate(invalid="ignore", over="ignore"):
        t, q, cp = th * s1 + c1, qh * s2 + c2, xh * s2 + c2
        dq1, dq2 = t + cpl(ch * cp), q + cpl(cp)
        precip = p0 + cg * np.sum(cp * d, axis=1)
        e1, e2, e3 = dq1 - T1, dq2 - T2, precip - T3
        f1, f2, f3 = 2 * inv1 * w12, 2 * inv2 * w12, 2 * inv3 * w3
        g1, g2, g3 = e1 * f1, e2 * f2, e3 * f3
        dy = np.zeros_like(yhat)
        dy[:, :nz] = g1 * s1 + r(th)
        dy[:, nz:2 * nz] = g2 * s2 + r(qh)
        dy[:, cp0:] = (cpl(ch * g1 + g2) + (cg * d) * g3[:, None]) * s2
        loss = float(np.sum(e1 * e1 * inv1 * w12) + np.sum(e2 * e2 * inv2 * w12) + np.sum(e3 * e3 * inv3 * w3))
        if has_dead:
            dead = yhat[:, 2 * nz]
            dy[:, 2 * nz] = r(dead)
        if reg:
            heads = yhat[:, :cp0]
            loss += float((l1 * np.sum(np.abs(heads)) + l2 * np.sum(heads * heads)) / n)

        # ---- bounds: the float32 roundings of the evaluation, then the error of yhat carried through ----
        m_cp = np.abs(xh * s2) + np.abs(c2)
        m1 = np.abs(th * s1) + np.abs(c1) + cpl(abs(ch) * m_cp)
        m2 = np.abs(qh * s2) + np.abs(c2) + cpl(m_cp)
        in_cp = e_xh * np.abs(s2)
        in_dq1, in_dq2 = e_th * np.abs(s1) + cpl(abs(ch) * in_cp), e_qh * np.abs(s2) + cpl(in_cp)
        a1, a2 = m1 + np.abs(T1), m2 + np.abs(T2)
        e_e1, e_e2 = 5 * U * a1 + in_dq1, 5 * U * a2 + in_dq2
        e_g1, e_g2 = (8 * U * a1 + in_dq1) * np.abs(f1), (8 * U * a2 + in_dq2) * np.abs(f2)
        e_precip = (nz + 2) * U * (np.abs(p0) + abs(cg) * np.sum(np.abs(cp * d), axis=1)) + \
            abs(cg) * np.sum((2 * U * m_cp + in_cp) * np.abs(d), axis=1)
        a3 = np.abs(precip) + np.abs(T3)
        e_e3 = e_precip + U * a3
        e_g3 = (e_precip + 4 * U * a3) * abs(f3)
        bound = np.zeros_like(yhat)
        bound[:, :nz] = e_g1 * np.abs(s1) + 2 * U * np.abs(g1 * s1) + 4 * U * r_abs(th) + r_in(th, e_th)
        bound[:, nz:2 * nz] = e_g2 * np.abs(s2) + 2 * U * np.abs(g2 * s2) + 4 * U * r_abs(qh) + r_in(qh, e_qh)
        cgd = np.abs(cg * d)
        bound[:, cp0:] = np.abs(s2) * (cpl(abs(ch) * e_g1 + e_g2) + cgd * e_g3[:, None] +
                                       4 * U * (cpl(np.abs(ch * g1) + np.abs(g2)) + cgd * np.abs(g3)[:, None]))
        if has_dead:
            bound[:, 2 * nz] = 4 * U * r_abs(dead) + r_in(dead, ey[:, 2 * nz])
        bound = 2.0 * bound + 1e-37
        loss_bound = float(np.sum((2 * np.abs(e1) * 2 * e_e1 + 4 * e_e1 ** 2) * inv1 * w12) +
                           np.sum((2 * np.abs(e2) * 2 * e_e2 + 4 * e_e2 ** 2) * inv2 * w12) +
                           np.sum((2 * np.abs(e3) * 2 * e_e3 + 4 * e_e3 ** 2) * inv3 * w3))
        if reg:
            e_heads = ey[:, :cp0]
            loss_bound += float(np.sum(l1 * e_heads + l2 * (2 * np.abs(heads) * e_heads + e_heads ** 2)) / n)
        loss_bound += 1e-14 * abs(loss)
    return dy, loss, bound, loss_bound, {"dq1": dq1, "dq2": dq2, "precip": precip}


def loss_grad32(yhat, scale1, center1, scale2, center2, inv1, inv2, inv3, delp, pp, t1, t2, t3, couple=True, has_dead=False, l1=0.0,
                l2=0.0, drop_integral_term=False):
    """The same evaluation in float32 numpy in the stated order (no row table): ``(dY, loss)``.  ``drop_integral_term`` leaves
    ``(c_g delp) g3`` out of ``dcp^`` -- the mistake the bound has to catch."""
    f = np.float32
    yhat = np.asarray(yhat, f)
    n = yhat.shape[0]
    nz = (yhat.shape[1] - int(has_dead)) // 3
    s1, c1, s2, c2, inv1, inv2, d, p0, T1, T2, T3 = (np.asarray(v, f) for v in (scale1, center1, scale2, center2, inv1, inv2, delp, pp,
                                                                                  t1, t2, t3))
    inv3, l1, l2, nf = f(inv3), f(l1), f(l2), f(n)
    w12, w3 = weights(n, nz)
    cp0 = 2 * nz + int(has_dead)
    th, qh, xh = yhat[:, :nz], yhat[:, nz:2 * nz], yhat[:, cp0:]
    t, q, cp = th * s1 + c1, qh * s2 + c2, xh * s2 + c2
    dq1, dq2 = (t + C_HEAT * cp, q + cp) if couple else (t, q)
    acc = np.zeros(n, f)
    for k in range(nz):
        acc = acc + cp[:, k] * d[:, k]
    precip = p0 + C_G * acc
    e1, e2, e3 = dq1 - T1, dq2 - T2, precip - T3
    g1, g2, g3 = f(2) * e1 * inv1 * w12, f(2) * e2 * inv2 * w12, f(2) * e3 * inv3 * w3
    reg = l1 != 0 or l2 != 0

    def r(x):
        return (l1 * np.sign(x) + f(2) * l2 * x) / nf

    dy = np.zeros_like(yhat)
    dy[:, :nz] = g1 * s1 + r(th) if reg else g1 * s1
    dy[:, nz:2 * nz] = g2 * s2 + r(qh) if reg else g2 * s2
    first = C_HEAT * g1 + g2 if couple else np.zeros_like(g1)
    dy[:, cp0:] = (first if drop_integral_term else first + (C_G * d) * g3[:, None]) * s2
    if has_dead and reg:
        dy[:, 2 * nz] = r(yhat[:, 2 * nz])
    assert dy.dtype == f
    e1, e2, e3, heads = (_f64(v) for v in (e1, e2, e3, yhat[:, :cp0]))
    loss = float(np.sum(e1 * e1 * _f64(inv1) * float(w12)) + np.sum(e2 * e2 * _f64(inv2) * float(w12)) +
                 np.sum(e3 * e3 * float(inv3) * float(w3)))
    if reg:
        loss += float((float(l1) * np.sum(np.abs(heads)) + float(l2) * np.sum(heads * heads)) / n)
    return dy, loss


def step(kernels, biases, xin, delp, pp, targets, loss, idx, relu=True):
    """Gradients of one minibatch of the precipitative network, as ``train_np.step``: ``(grads, bounds, loss_value, loss_bound)``,
    per layer ``(dW, db)`` and the bound of each.  ``loss``: an object with scale1, center1, scale2, center2, inv_cstd2_1,
    inv_cstd2_2, inv_cstd2_3, couple, has_dead, l1 and l2; ``targets``: (dQ1, dQ2, total_precipitation_rate)."""
    x = rows(xin, idx)
    n = x.shape[0]
    last = len(kernels) - 1
    acts, errs, pres = [x], [np.zeros_like(x)], []
    for l, (w, b) in enumerate(zip(kernels, biases)):
        w, b = _f64(w), _f64(b)
        pre = acts[-1] @ w + b
        e = _contract(acts[-1], errs[-1], w, np.zeros_like(w), w.shape[0] + 1, np.abs(b))
        pres.append((pre, e))
        acts.append(np.maximum(pre, 0) if (relu and l < last) else pre)
        errs.append(e)
    t1, t2, t3 = targets
    dh, value, e_dh, loss_bound, _ = loss_grad(acts[-1], loss.scale1, loss.center1, loss.scale2, loss.center2, loss.inv_cstd2_1,
                                               loss.inv_cstd2_2, loss.inv_cstd2_3, delp, np.reshape(pp, -1), t1, t2, np.reshape(t3, -1),
                                               idx=idx, couple=loss.couple, has_dead=loss.has_dead, l1=loss.l1, l2=loss.l2,
                                               e_yhat=errs[-1])
    grads, bounds = [None] * (last + 1), [None] * (last + 1)
    for l in range(last, -1, -1):
        a, ea, w = acts[l], errs[l], _f64(kernels[l])
        dw, db = a.T @ dh, dh.sum(axis=0)
        e_dw = _contract(a.T, ea.T, dh, e_dh, n)
        e_db = e_dh.sum(axis=0) + 2.0 * n * U * (np.abs(dh) + e_dh).sum(axis=0)
        grads[l], bounds[l] = (dw, db), (e_dw + 1e-37, e_db + 1e-37)
        if l > 0:
            da = dh @ w.T
            e_da = _contract(dh, e_dh, w.T, np.zeros_like(w.T), w.shape[1])
            if relu:
                pre, e_pre = pres[l - 1]
                mask = pre > 0
                unsure = np.abs(pre) <= e_pre
                e_da = np.where(unsure, np.abs(da) + e_da, np.where(mask, e_da, 0.0))
                da = np.where(mask, da, 0.0)
            dh, e_dh = da, e_da
    return grads, bounds, value, loss_bound


def compose_jacobians(head_jac, head_bound, cp, e_cp, delp, couple):
    """``train_np.predict_jacobians``' output for the three heads with the closure applied (float64), and the bounds carried
    through it: ``(jacobians, bounds)`` for dQ1, dQ2 and total_precipitation_rate.  ``cp`` / ``e_cp``: the column-precipitation
    head's value at the profile and its bound."""
    ch, cg = float(C_HEAT), float(C_G)
    d = np.atleast_1d(np.asarray(delp)).astype(np.float32).astype(np.float64)
    out = {"dQ1": {}, "dQ2": {}, "total_precipitation_rate": {}}
    bnd = {"dQ1": {}, "dQ2": {}, "total_precipitation_rate": {}}
    for src, jc in head_jac["q_tendency_due_to_precip"].items():
        bc = head_bound["q_tendency_due_to_precip"][src]
        jt, jq = head_jac["dQ1"][src], head_jac["dQ2"][src]
        bt, bq = head_bound["dQ1"][src], head_bound["dQ2"][src]
        out["dQ1"][src], bnd["dQ1"][src] = (jt + ch * jc, bt + abs(ch) * bc) if couple else (jt, bt)
        out["dQ2"][src], bnd["dQ2"][src] = (jq + jc, bq + bc) if couple else (jq, bq)
        row, brow = cg * (d[None, :] @ jc), abs(cg) * (np.abs(d)[None, :] @ bc)
        if src == "pressure_thickness_of_atmospheric_layer":
            row, brow = row + cg * np.asarray(cp)[None, :], brow + abs(cg) * np.asarray(e_cp)[None, :]
        elif src == "physics_precip":
            row = row + 1.0
        out["total_precipitation_rate"][src], bnd["total_precipitation_rate"][src] = row, brow
    return out, bnd

