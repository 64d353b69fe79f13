"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of what csrc/mlp_train.hip computes -- the three GEMM forms, the loss
and its gradient, torch's Adam, a full training step and the Jacobian through the predict graph -- together with the
absolute-product sums ``sum |a_i| |b_i|`` of every contraction, from which the tests derive their bounds:

    a float32 dot product of length n in any summation order:  |got - exact| <= n 2^-24 sum |a_i| |b_i|  (to first order)

The tests use twice that (slack for the cast of the float64 reference), with n + 1 where a bias is added.  ``step`` and
``jacobian_raw`` carry such bounds through the layers: an input known to within E adds ``E @ |W|``; where a ReLU mask or a
limit is decided by a value closer to its threshold than that value's bound, the whole term counts as error.
"""
import numpy as np

U = 2.0 ** -24


def _f64(a):
    return np.asarray(a, np.float64)


def rows(a, idx=None):
    return _f64(a) if idx is None else _f64(a)[np.asarray(idx)]


# ---- the three GEMM forms: (result, absolute-product sums) ---------------------------------------------------------------
def linear_forward(a, w, b=None, idx=None, relu=False):
    a, w = rows(a, idx), _f64(w)
    b = np.zeros(w.shape[1]) if b is None else _f64(b)
    h = a @ w + b
    mag = np.abs(a) @ np.abs(w) + np.abs(b)
    return (np.maximum(h, 0) if relu else h), mag


def linear_backward_data(dh, w, p=None, shared_p=False):
    dh, w = _f64(dh), _f64(w)
    da = dh @ w.T
    mag = np.abs(dh) @ np.abs(w).T
    if p is not None:
        mask = (_f64(p)[0:1] if shared_p else _f64(p)) > 0
        da, mag = np.where(mask, da, 0.0), np.where(mask, mag, 0.0)
    return da, mag


def linear_backward_weight(a, dh, idx=None):
    a, dh = rows(a, idx), _f64(dh)
    return a.T @ dh, dh.sum(axis=0), np.abs(a).T @ np.abs(dh), np.abs(dh).sum(axis=0)


def dot_bound(n, mag):
    """The tests' bound for a contraction of length ``n`` (bias counted by the caller)."""
    return 2.0 * n * U * mag + 1e-37


# ---- loss ----------------------------------------------------------------------------------------------------------------
def mse_grad(yhat, scale, center, inv_cstd2, lo, hi, keep, wnorm, targets, idx=None):
    """(dY, loss, bound): the gradient of ``sum_j keep_j wnorm_j inv_cstd2_j (clamp(p, lo, hi) - t)^2`` with ``p = yhat scale +
    center`` with respect to ``yhat`` (torch.clamp's gradient: 1 for lo <= p <= hi), the loss, and the elementwise bound
    ``8 U (|yhat scale| + |center| + |t|) |2 inv_cstd2 scale wnorm|``."""
    yhat, t = _f64(yhat), rows(targets, idx)
    scale, center, inv, lo, hi, keep, wnorm = (_f64(v) for v in (scale, center, inv_cstd2, lo, hi, keep, wnorm))
    p = yhat * scale + center
    pc = np.clip(p, lo, hi)
    kept = keep != 0
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(kept, pc - t, 0.0)
        factor = np.where(kept, 2.0 * inv * scale * wnorm, 0.0)
        inside = (p >= lo) & (p <= hi)
        dy = np.where(inside & kept, d * factor, 0.0)
        loss = float(np.sum(np.where(kept, d * d * inv * wnorm, 0.0)))
        bound = 8.0 * U * (np.abs(yhat * scale) + np.abs(center) + np.abs(np.where(kept, t, 0.0))) * np.abs(factor)
    return dy, loss, bound


# ---- torch.optim.Adam (defaults: no weight decay, no amsgrad) ----------------------------------------------------------------
def adam(p, g, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """One update at step ``t`` (1-based); returns the new (p, m, v)."""
    p, g, m, v = (_f64(x) for x in (p, g, m, v))
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - beta2 ** t) + eps
    return p - (lr / (1 - beta1 ** t)) * m / denom, m, v


# ---- a full step with bounds carried through the layers ------------------------------------------------------------------------
def _contract(a, ea, b, eb, n, extra=0.0):
    """|computed - exact| of a length-n float32 contraction of operands known to within ea, eb."""
    return ea @ np.abs(b) + np.abs(a) @ eb + ea @ eb + 2.0 * n * U * ((np.abs(a) + ea) @ (np.abs(b) + eb) + extra)


def step(kernels, biases, xin, targets, loss, idx, relu=True):
    """Gradients of one minibatch.  ``loss``: an object with scale, center, inv_cstd2, lo, hi, keep and ``wnorm(n)``.  Returns
    ``(grads, bounds, loss_value, loss_bound)``: per layer ``(dW, db)`` and the bound of each; the loss is a float64 sum of
    squared float32 differences d, each known to within e_d: its bound is the sum of ``(2 |d| e_d + e_d^2) inv_cstd2 wnorm``."""
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
    wn = loss.wnorm(n)
    dy, value, bound = mse_grad(acts[-1], loss.scale, loss.center, loss.inv_cstd2, loss.lo, loss.hi, loss.keep, wn, targets, idx)
    scale, center = _f64(loss.scale), _f64(loss.center)
    factor = np.where(_f64(loss.keep) != 0, 2.0 * _f64(loss.inv_cstd2) * scale * _f64(wn), 0.0)
    ep = errs[-1] * np.abs(scale) + 4 * U * (np.abs(acts[-1] * scale) + np.abs(center))
    e_dy = bound + ep * np.abs(factor)
    p = acts[-1] * scale + center
    for edge in (_f64(loss.lo), _f64(loss.hi)):
        with np.errstate(invalid="ignore"):
            near = np.abs(p - edge) <= ep
        d_full = np.abs((np.clip(p, _f64(loss.lo), _f64(loss.hi)) - rows(targets, idx)) * factor)
        e_dy = np.where(near & (_f64(loss.keep) != 0), e_dy + d_full + ep * np.abs(factor), e_dy)
    t = rows(targets, idx)
    kept = _f64(loss.keep) != 0
    with np.errstate(invalid="ignore"):
        pc = np.clip(p, _f64(loss.lo), _f64(loss.hi))
        d = np.where(kept, np.abs(pc - t), 0.0)
        e_d = np.where(kept, ep + 2 * U * (np.abs(pc) + np.abs(t)), 0.0)
    loss_bound = float(np.sum((2 * d * e_d + e_d * e_d) * _f64(loss.inv_cstd2) * _f64(wn))) + 1e-14 * abs(value)
    grads, bounds = [None] * (last + 1), [None] * (last + 1)
    dh, e_dh = dy, e_dy
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


def jacobian_raw(kernels, biases, x_row, relu=True):
    """(J, bound, yhat, yhat bound): d yhat / d x at one row, float64, with the composed bound of the float32 kernels."""
    x = _f64(x_row).reshape(1, -1)
    last = len(kernels) - 1
    a, e = x, 2 * U * np.abs(x)   # (the caller's row may have been normalised in float32)
    pres = []
    for l, (w, b) in enumerate(zip(kernels, biases)):
        w, b = _f64(w), _f64(b)
        pre = a @ w + b
        e = _contract(a, e, w, np.zeros_like(w), w.shape[0] + 1, np.abs(b))
        pres.append((pre, e))
        a = np.maximum(pre, 0) if (relu and l < last) else pre
    yhat, e_y = a[0], e[0]
    f = kernels[-1].shape[1]
    dh, e_dh = np.eye(f), np.zeros((f, f))
    for l in range(last, -1, -1):
        w = _f64(kernels[l])
        da = dh @ w.T
        e_da = _contract(dh, e_dh, w.T, np.zeros_like(w.T), w.shape[1])
        if l > 0 and relu:
            pre, e_pre = pres[l - 1]
            unsure = np.abs(pre) <= e_pre
            e_da = np.where(unsure, np.abs(da) + e_da, np.where(pre > 0, e_da, 0.0))
            da = np.where(pre > 0, da, 0.0)
        dh, e_dh = da, e_da
    return dh, e_dh + 1e-37, yhat, e_y


# ---- the Jacobian through the predict graph ------------------------------------------------------------------------------------
def _per_feature(v, n, fill):
    return np.full(n, fill, np.float64) if v is None else np.broadcast_to(_f64(np.asarray(v, np.float32)), (n,))


def predict_jacobians(spec, profiles, relu=True):
    """``{output: {source: [nfeat_out, len(profile)]}}`` of an MlpSpec-shaped predict graph (oracle/mlp_np.forward) at one
    profile per source, float64, with the matching bounds as a second dict.  The profile is cast to float32 first, as the
    predictor casts its inputs.  Bounds inclusive at the limits, as in training."""
    prof = {name: np.atleast_1d(np.asarray(p)).astype(np.float32).astype(np.float64) for name, p in profiles.items()}
    cols, slopes = [], []
    for i in spec.inputs:
        x = prof[i.source][i.start:i.start + i.nfeat]
        slope = np.ones(i.nfeat)
        if i.transform == "log":
            eps = float(np.float32(i.eps))
            with np.errstate(divide="ignore"):
                slope = np.where(x > eps, 1.0 / x, 0.0)
            x = np.log(np.maximum(x, eps))
        center, scale = _per_feature(i.center, i.nfeat, 0.0), _per_feature(i.scale, i.nfeat, 1.0)
        cols.append((x - center) / scale)
        slopes.append(slope / scale)
    x_row = np.concatenate(cols)
    kernels = list(spec.hidden_kernels) + [spec.out_kernel]
    biases = list(spec.hidden_biases) + [spec.out_bias]
    jac, e_jac, yhat, _ = jacobian_raw(kernels, biases, x_row.astype(np.float32), relu=relu and getattr(spec, "activation", "relu") == "relu")
    out, bounds = {}, {}
    f0 = 0
    for o in spec.outputs:
        sl = slice(f0, f0 + o.nfeat)
        f0 += o.nfeat
        scale, center = _per_feature(o.scale, o.nfeat, 1.0), _per_feature(o.center, o.nfeat, 0.0)
        p = yhat[sl] * scale + center
        factor = scale.copy()
        if o.min is not None:
            factor = np.where(p >= float(np.float32(o.min)), factor, 0.0)
        if o.max is not None:
            factor = np.where(p <= float(np.float32(o.max)), factor, 0.0)
        if o.mask is not None:
            factor = np.where(np.asarray(o.mask) != 0, factor, 0.0)
        out[o.name] = {name: np.zeros((o.nfeat, p_.shape[0])) for name, p_ in prof.items() if any(i.source == name for i in spec.inputs)}
        bounds[o.name] = {name: np.zeros_like(v) for name, v in out[o.name].items()}
        c0 = 0
        for i, slope in zip(spec.inputs, slopes):
            cs = slice(i.start, i.start + i.nfeat)
            out[o.name][i.source][:, cs] += jac[sl, c0:c0 + i.nfeat] * slope[None, :] * factor[:, None]
            # the device Jacobian is float32 (one more rounding); the host factors are applied in float64
            bounds[o.name][i.source][:, cs] += (e_jac[sl, c0:c0 + i.nfeat] + U * np.abs(jac[sl, c0:c0 + i.nfeat])) * \
                np.abs(slope[None, :] * factor[:, None]) * (1 + 8 * U) + 1e-37
            c0 += i.nfeat
    return out, bounds


def nondimensionalize(jacobians, std_factors):
    """The reference's formula (keras/jacobian.py, nondimensionalize_jacobians): columns times std(input), rows times
    ``1.0 / std(output)``, the factors in the dtype ``np.std`` gave them."""
    return {o: {i: np.multiply(np.multiply(j, std_factors[i].reshape(1, -1)), 1.0 / std_factors[o].reshape(-1, 1)) for i, j in per.items()}
            for o, per in jacobians.items()}
