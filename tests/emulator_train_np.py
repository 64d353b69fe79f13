"""TEST INFRASTRUCTURE ONLY: numpy restatement of ``fv3hip_train_emulator_loss_grad`` (csrc/mlp_train.hip)
-- the multi-variable loss of the microphysics emulators and its gradient with respect to the raw head outputs -- in float64
(``loss_grad``) and in float32 in the stated order (``loss_grad32``), and of a whole training step (``step``), with the gates the
tests hold the float32 kernels to.  No gate is chosen by hand: each counts the float32 operations of the stated evaluation order
at ``U = 2^-24`` each (first order, the second-order terms of carried errors kept), doubled as ``train_np.dot_bound`` doubles
(slack for the casts of this float64 reference).  ``expf`` and ``logf`` count 3 ulp each, the figure DESIGN section 4.4 uses for
the device's ``log``.

The heads are ``fv3net_amd.ops.EmulatorHead`` descriptors holding numpy arrays.  ``wgrad = float32(weight / count)`` is taken at
its float32 value, as the entry point forms it; a metric term (``is_loss`` false) is reported and adds nothing to ``dY``.  With ``M = |y s| + |c|`` (``|y|`` for an unscaled head) and ``e_y`` the bound the
forward pass puts on ``yhat``:

    MSE   p = y s + c      one product, one sum              e_p = 2 U M + e_y |s|            (unscaled: e_p = e_y)
          d = p - T        one difference                    e_d = e_p + U (M + |T|)
          d d inv          two products                      (2 |d| e_d + e_d^2) inv + 2 U d^2 inv          (value, per element)
          g = 2 d inv w    two rounded products (2 d exact)  e_g = (e_d + 2 U (|d| + e_d)) 2 inv w
          a = B + p        one sum                           e_a = e_p + U (|B| + M)
          e = a - A        one difference                    e_e = e_a + U (|B| + M + |A|);  its value and g as for d
          g_d + g_a        one sum, where both terms exist   + U (|g_d| + |g_a| + e_gd + e_ga)
          dy = g s         one product                       e_g |s| + U (|g| + e_g) |s|
    CE    u_c = x_c - mx   one difference (mx is one of x)   e_u = U |u_c| + 2 e_y
          expf(u_c)        3 ulp and the argument's error    e_c = exp(u_c) (3 U + e_u)
          s                C - 1 sums                        e_s = (C - 1) U s + sum e_c
          lse = mx + logf  3 ulp, one sum                    e_l = e_y + 3 U |log s| + e_s / s + U |lse|
          t_c (lse - x_c)  one difference, one product       |t_c| (e_l + e_y + U |lse - x_c|) + U |t_c (lse - x_c)|   (value)
          st               C - 1 sums                        e_st = (C - 1) U sum |t_c|
          q = expf(x - lse)                                  e_q = q (3 U + U |x_c - lse| + e_l + e_y)
          (q st - t_c) w   product, difference, product      (e_q |st| + q e_st + U q |st| + U (q |st| + |t_c|)) w + U |dy|
"""
import numpy as np

from train_np import U, _contract, _f64, rows

VARIANTS = (None, "drop_after_grad", "count_n", "st_one")   # the mistakes the gates have to catch


def n_slots(heads):
    return sum((h.slot is not None) + (h.slot_after is not None) for h in heads)


def _gather(a, idx, fill, n):
    a = _f64(a)
    if idx is None:
        return a[:n]
    idx = np.asarray(idx)[:n]
    ok = (idx >= 0) & (idx < a.shape[0])
    out = a[np.where(ok, idx, 0)].copy()
    out[~ok] = fill
    return out


def _count(h, n, levels, variant=None):
    if h.kind == "mse":
        return n if variant == "count_n" else n * h.ncol
    return n if h.single_level else n * levels


EXACT_WGRAD = False   # True: wgrad = weight / count unrounded, for the comparison with autograd of a torch.mean


def _wgrad(weight, is_loss, count):
    if not is_loss:
        return 0.0
    w = float(weight) / float(count)
    return w if EXACT_WGRAD else float(np.float32(w))


def _tables(h, levels, dtype):
    nt = h.ncol if h.kind == "mse" else levels

    def tab(v):
        return None if v is None else np.broadcast_to(np.asarray(v, np.float32), (nt,)).astype(dtype)

    return tab(h.scale), tab(h.center), tab(h.inv), tab(h.inv_after)


def _finish(heads, sums, counts):
    """values[slot] = sum * wval; loss = the loss slots' weight * value in slot order."""
    ns = n_slots(heads)
    values = np.zeros(ns)
    weight, is_loss = np.zeros(ns), np.zeros(ns, bool)
    for h in heads:
        for slot, w, il in ((h.slot, h.weight, h.is_loss), (h.slot_after, h.weight_after, h.is_loss_after)):
            if slot is not None:
                values[slot] = sums[slot] * (1.0 / counts[slot])
                weight[slot], is_loss[slot] = float(w), bool(il)
    loss = 0.0
    for s in range(ns):
        if is_loss[s]:
            loss += weight[s] * values[s]
    return values, loss, weight, is_loss


def loss_grad(yhat, heads, levels=1, idx=None, e_yhat=None, variant=None):
    """Float64: ``(dY, values, loss, dY bound, value bounds, loss bound)`` for ``yhat [n * levels, F]``.  ``variant`` evaluates
    one of the mistakes of ``VARIANTS`` instead (no bounds meant)."""
    yhat = _f64(yhat)
    L = int(levels)
    n = yhat.shape[0] // L
    ey = np.zeros_like(yhat) if e_yhat is None else _f64(e_yhat)
    dy, bound = np.zeros_like(yhat), np.zeros_like(yhat)
    ns = n_slots(heads)
    sums, counts, vb = np.zeros(ns), np.ones(ns), np.zeros(ns)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for h in heads:
            cols = slice(h.col0, h.col0 + h.ncol)
            count = _count(h, n, L, variant)
            if h.kind == "xent":
                C = h.ncol
                x, e_x = yhat[:, cols].reshape(n, L, C), ey[:, cols].reshape(n, L, C)
                e1 = e_x.max(axis=-1, keepdims=True)
                t = _gather(h.target, idx, np.nan, n).reshape(n, L, C)
                w = _wgrad(h.weight, h.is_loss, count)
                mx = x.max(axis=-1, keepdims=True)
                u = x - mx
                ex = np.exp(u)
                s = ex.sum(axis=-1, keepdims=True)
                lse = mx + np.log(s)
                st = np.ones_like(s) if variant == "st_one" else t.sum(axis=-1, keepdims=True)
                term = t * (lse - x)
                q = np.exp(x - lse)
                g = (q * st - t) * w if h.is_loss else np.zeros_like(x)
                e_u = U * np.abs(u) + 2 * e1
                e_c = ex * (3 * U + e_u)
                e_s = (C - 1) * U * s + e_c.sum(axis=-1, keepdims=True)
                e_l = e1 + 3 * U * np.abs(np.log(s)) + e_s / s + U * np.abs(lse)
                e_term = np.abs(t) * (e_l + e1 + U * np.abs(lse - x)) + U * np.abs(term)
                e_st = (C - 1) * U * np.abs(t).sum(axis=-1, keepdims=True)
                e_q = q * (3 * U + U * np.abs(x - lse) + e_l + e1)
                e_g = (e_q * np.abs(st) + q * e_st + U * q * np.abs(st) + U * (q * np.abs(st) + np.abs(t))) * w + U * np.abs(g)
                if not h.is_loss:
                    e_g = np.zeros_like(x)
                dy[:, cols], bound[:, cols] = g.reshape(n * L, C), e_g.reshape(n * L, C)
                sums[h.slot], counts[h.slot], vb[h.slot] = term.sum(), count, e_term.sum() / count
                continue
            scale, center, inv, inv_a = _tables(h, L, np.float64)
            shape = (n, h.ncol) if h.kind == "mse" else (n, L)
            y, e_y = yhat[:, cols].reshape(shape), ey[:, cols].reshape(shape)
            if h.single_level:
                y, e_y = y[:, :1], e_y[:, :1]
                scale, center, inv, inv_a = (None if v is None else v[:1] for v in (scale, center, inv, inv_a))
            if scale is None:
                p, M, e_p = y, np.abs(y), e_y
            else:
                p, M = y * scale + center, np.abs(y * scale) + np.abs(center)
                e_p = 2 * U * M + e_y * np.abs(scale)
            g, e_g, nterms = np.zeros_like(p), np.zeros_like(p), 0
            if h.slot is not None:
                T = _gather(h.target, idx, np.nan, n).reshape(p.shape)
                w = _wgrad(h.weight, h.is_loss, count)
                d = p - T
                e_d = e_p + U * (M + np.abs(T))
                sums[h.slot], counts[h.slot] = np.sum(d * d * inv), count
                vb[h.slot] = np.sum((2 * np.abs(d) * e_d + e_d ** 2) * inv + 2 * U * d * d * inv) / count
                if h.is_loss:   # (a metric term adds nothing to dY, not even a NaN)
                    gd = 2 * d * inv * w
                    g, e_g, nterms = gd, (e_d + 2 * U * (np.abs(d) + e_d)) * 2 * inv * w, 1
            if h.slot_after is not None:
                B = _gather(h.before, idx, 0.0, n).reshape(p.shape)
                A = _gather(h.target_after, idx, np.nan, n).reshape(p.shape)
                w = _wgrad(h.weight_after, h.is_loss_after, count)
                e = (B + p) - A
                e_e = e_p + U * (np.abs(B) + M) + U * (np.abs(B) + M + np.abs(A))
                sums[h.slot_after], counts[h.slot_after] = np.sum(e * e * inv_a), count
                vb[h.slot_after] = np.sum((2 * np.abs(e) * e_e + e_e ** 2) * inv_a + 2 * U * e * e * inv_a) / count
                if variant != "drop_after_grad" and h.is_loss_after:
                    ga = 2 * e * inv_a * w
                    e_ga = (e_e + 2 * U * (np.abs(e) + e_e)) * 2 * inv_a * w
                    if nterms:
                        e_g = e_g + e_ga + U * (np.abs(g) + np.abs(ga) + e_g + e_ga)
                        g = g + ga
                    else:
                        g, e_g = ga, e_ga
            if scale is not None:
                e_g = e_g * np.abs(scale) + U * (np.abs(g) + e_g) * np.abs(scale)
                g = g * scale
            if h.single_level:
                full, efull = np.zeros((n, L)), np.zeros((n, L))
                full[:, :1], efull[:, :1] = g, e_g
                g, e_g = full, efull
            dy[:, cols], bound[:, cols] = g.reshape(-1, h.ncol), e_g.reshape(-1, h.ncol)
    values, loss, weight, is_loss = _finish(heads, sums, counts)
    vb = 2.0 * vb + 1e-14 * np.abs(values) + 1e-37
    loss_bound = float(np.sum(np.where(is_loss, weight * vb, 0.0)))
    return dy, values, loss, 2.0 * bound + 1e-37, vb, loss_bound


def loss_grad32(yhat, heads, levels=1, idx=None, variant=None):
    """The same evaluation in float32 numpy in the stated order, values as float64 sums of the float32 terms:
    ``(dY float32, values, loss)``.  ``expf`` / ``logf`` are numpy's float32 ones."""
    f = np.float32
    yhat = np.asarray(yhat, f)
    L = int(levels)
    n = yhat.shape[0] // L
    dy = np.zeros_like(yhat)
    ns = n_slots(heads)
    sums, counts = np.zeros(ns), np.ones(ns)

    def gather(a, fill):
        return _gather(a, idx, fill, n).astype(f)

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for h in heads:
            cols = slice(h.col0, h.col0 + h.ncol)
            count = _count(h, n, L, variant)
            if h.kind == "xent":
                C = h.ncol
                x = yhat[:, cols].reshape(n, L, C)
                t = gather(h.target, np.nan).reshape(n, L, C)
                w = f(_wgrad(h.weight, h.is_loss, count))
                mx = x.max(axis=-1)
                s, st = np.zeros((n, L), f), np.zeros((n, L), f)
                for c in range(C):
                    s = s + np.exp(x[..., c] - mx)
                    st = st + t[..., c]
                if variant == "st_one":
                    st = np.ones_like(st)
                lse = mx + np.log(s)
                total = 0.0
                g = np.zeros_like(x)
                for c in range(C):
                    total += float(np.sum(_f64(t[..., c] * (lse - x[..., c]))))
                    if h.is_loss:
                        g[..., c] = (np.exp(x[..., c] - lse) * st - t[..., c]) * w
                assert g.dtype == f
                dy[:, cols] = g.reshape(n * L, C)
                sums[h.slot], counts[h.slot] = total, count
                continue
            scale, center, inv, inv_a = _tables(h, L, f)
            shape = (n, h.ncol) if h.kind == "mse" else (n, L)
            y = yhat[:, cols].reshape(shape)
            if h.single_level:
                y = y[:, :1]
                scale, center, inv, inv_a = (None if v is None else v[:1] for v in (scale, center, inv, inv_a))
            p = y if scale is None else y * scale + center
            g = np.zeros_like(p)
            if h.slot is not None:
                d = p - gather(h.target, np.nan).reshape(p.shape)
                sums[h.slot], counts[h.slot] = float(np.sum(_f64(d * d * inv))), count
                if h.is_loss:
                    g = f(2) * d * inv * f(_wgrad(h.weight, h.is_loss, count))
            if h.slot_after is not None:
                a = gather(h.before, 0.0).reshape(p.shape) + p
                e = a - gather(h.target_after, np.nan).reshape(p.shape)
                sums[h.slot_after], counts[h.slot_after] = float(np.sum(_f64(e * e * inv_a))), count
                if variant != "drop_after_grad" and h.is_loss_after:
                    g = g + f(2) * e * inv_a * f(_wgrad(h.weight_after, h.is_loss_after, count))
            if scale is not None:
                g = g * scale
            assert g.dtype == f
            if h.single_level:
                full = np.zeros((n, L), f)
                full[:, :1] = g
                g = full
            dy[:, cols] = g.reshape(-1, h.ncol)
    values, loss, _, _ = _finish(heads, sums, counts)
    return dy, values, loss


def step(kernels, biases, xin, heads, levels, idx, relu=True, variant=None):
    """Gradients of one minibatch of the emulator network, as ``train_np.step``: ``(grads, bounds, values, loss, loss_bound, value_bounds)``,
    per layer ``(dW, db)`` and the bound of each.  ``xin [rows * levels, K]``; ``idx`` the batch rows."""
    idx = np.asarray(idx)
    L = int(levels)
    net = (idx[:, None] * L + np.arange(L)[None, :]).reshape(-1)
    x = rows(xin, net)
    m = x.shape[0]
    last = len(kernels) - 1
    acts, errs, pres = [x], [np.zeros_like(x)], []
    for l, (w, b) in enumerate(zip(kernels, biases)):
        w, b = _f64(w), _f64(b)
        pre = acts[-1] @ w + b
        e = _contract(acts[-1], errs[-1], w, np.zeros_like(w), w.shape[0] + 1, np.abs(b))
        pres.append((pre, e))
        acts.append(np.maximum(pre, 0) if (relu and l < last) else pre)
        errs.append(e)
    dh, values, loss, e_dh, value_bounds, loss_bound = loss_grad(acts[-1], heads, L, idx=idx, e_yhat=errs[-1], variant=variant)
    grads, bounds = [None] * (last + 1), [None] * (last + 1)
    for l in range(last, -1, -1):
        a, ea, w = acts[l], errs[l], _f64(kernels[l])
        dw, db = a.T @ dh, dh.sum(axis=0)
        e_dw = _contract(a.T, ea.T, dh, e_dh, m)
        e_db = e_dh.sum(axis=0) + 2.0 * m * U * (np.abs(dh) + e_dh).sum(axis=0)
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
    return grads, bounds, values, loss, loss_bound, value_bounds
