"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of what csrc/conv_train.hip and fv3net_amd/conv_train.py compute -- the
"valid" convolution in its three orientations, the transpose-invariance constraint, the data preparation of
``fit.train_convolutional_model`` and one whole training step -- together with the absolute-product sums ``sum |a_i| |b_i|`` of
every contraction, from which the tests derive their bounds exactly as tests/train_np.py does (``dot_bound``, ``_contract``).

Every contraction is written as a matrix product over ``patches``: the ``k x k`` windows of ``[s, X, Y, c]`` laid out
``[s, X - k + 1, Y - k + 1, (a, b, c)]``, the order in which a Keras kernel ``[k, k, c, f]`` reshapes to ``[(a, b, c), f]``.  The
adjoint with respect to the input is the same product on the gradient padded by ``k - 1`` zeros with the kernel flipped.
Arrays are ``[sample, x, y, channel]``; nothing here imports ``fv3net_amd``.
"""
import numpy as np

import conv_np
import train_np as T

U = T.U


def _f64(a):
    return np.asarray(a, np.float64)


def samples(a, idx=None):
    """The batch ``a[idx]``; an index outside the table reads as a sample of zeros."""
    a = _f64(a)
    if idx is None:
        return a
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < a.shape[0])
    out = np.zeros((len(idx),) + a.shape[1:])
    out[ok] = a[idx[ok]]
    return out


def patches(x, k):
    s, X, Y, c = x.shape
    ox, oy = X - k + 1, Y - k + 1
    return np.concatenate([x[:, a:a + ox, b:b + oy, :] for a in range(k) for b in range(k)], axis=-1)


def _flipped(w):
    """``[k, k, c, f]`` -> the matrix ``[(a', b', f), c]`` of the adjoint: w[k - 1 - a', k - 1 - b', c, f]."""
    k, _, c, f = w.shape
    return w[::-1, ::-1].transpose(0, 1, 3, 2).reshape(k * k * f, c)


def _padded(dh, k):
    return np.pad(dh, ((0, 0), (k - 1, k - 1), (k - 1, k - 1), (0, 0)))


# ---- the three forms: (result, absolute-product sums) -----------------------------------------------------------------------
def conv_forward(a, w, b=None, idx=None, relu=False):
    a, w = samples(a, idx), _f64(w)
    k, f = w.shape[0], w.shape[3]
    b = np.zeros(f) if b is None else _f64(b)
    p, wm = patches(a, k), w.reshape(-1, f)
    h = p @ wm + b
    mag = np.abs(p) @ np.abs(wm) + np.abs(b)
    return (np.where(h < 0, 0.0, h) if relu else h), mag


def conv_backward_data(dh, w, p=None):
    dh, w = _f64(dh), _f64(w)
    k = w.shape[0]
    dp, wf = patches(_padded(dh, k), k), _flipped(w)
    da, mag = dp @ wf, np.abs(dp) @ np.abs(wf)
    if p is not None:
        mask = _f64(p) > 0
        da, mag = np.where(mask, da, 0.0), np.where(mask, mag, 0.0)
    return da, mag


def conv_backward_weight(a, dh, k, idx=None):
    a, dh = samples(a, idx), _f64(dh)
    c, f = a.shape[3], dh.shape[3]
    p, d = patches(a, k).reshape(-1, k * k * c), dh.reshape(-1, f)
    return ((p.T @ d).reshape(k, k, c, f), d.sum(axis=0), (np.abs(p).T @ np.abs(d)).reshape(k, k, c, f), np.abs(d).sum(axis=0))


def constrain(w):
    """TransposeInvariant in the dtype of ``w`` (float32 in: the bits of the device's and of torch's result)."""
    w = np.asarray(w)
    return (w.dtype.type(0.5) * (w + w.transpose(1, 0, 2, 3))).astype(w.dtype)


# ---- data preparation ---------------------------------------------------------------------------------------------------------
def prepare(inputs, outputs, n_halo, nfit):
    """``inputs`` / ``outputs``: lists of ``[sample, tile, x, y, z]`` float32 arrays.  Returns a dict: ``X`` the padded inputs
    folded to ``[sample * tile, x + 2 h, y + 2 h, z]``, ``y`` the folded outputs, mean / std per feature of the first ``nfit``
    folded samples (float64, halo cells and zero corners included), and ``xin`` = (X - mean) / (std + 1e-7) concatenated."""
    def fold(a):
        return a.reshape((-1,) + a.shape[2:])

    def pad(a):   # conv_np.append_halos takes [6, ..., x, y]
        return np.asarray(conv_np.append_halos(a.transpose(1, 0, 4, 2, 3), n_halo)).transpose(1, 0, 3, 4, 2)

    X = [fold(pad(np.asarray(a, np.float32))) for a in inputs]
    y = [fold(np.asarray(a, np.float32)) for a in outputs]
    flat = lambda a: _f64(a[:nfit]).reshape(-1, a.shape[-1])
    out = {"X": X, "y": y,
           "x_mean": [flat(a).mean(axis=0) for a in X], "x_std": [flat(a).std(axis=0) for a in X],
           "y_mean": [flat(a).mean(axis=0) for a in y], "y_std": [flat(a).std(axis=0) for a in y]}
    eps = float(np.float32(1e-7))
    out["xin"] = np.concatenate([(_f64(a) - m) / (s + eps) for a, m, s in zip(X, out["x_mean"], out["x_std"])], axis=-1)
    return out


# ---- a whole step with bounds carried through the layers ---------------------------------------------------------------------
def _as_rows(a):
    return a.reshape(-1, a.shape[-1])


def step(hidden_kernels, hidden_biases, out_kernel, out_bias, xin, targets, loss, idx, relu=True):
    """Gradients of the batch of tile-samples ``idx``.  ``targets`` is ``[samples * nx * ny, F_out]``; ``loss`` an object with
    scale, center, inv_cstd2, lo, hi, keep and ``wnorm(rows)``.  Returns ``(grads, bounds, loss_value, loss_bound)``: per hidden
    layer and then for the heads ``(dW, db)`` and the bound of each, composed as ``train_np.step`` composes them (an element
    whose ReLU mask is decided within its own bound counts in full)."""
    x = samples(xin, idx)
    n_hidden = len(hidden_kernels)
    acts, errs, pres = [x], [np.zeros_like(x)], []
    for w, b in zip(hidden_kernels, hidden_biases):
        w, b = _f64(w), _f64(b)
        k, f = w.shape[0], w.shape[3]
        p, ep, wm = patches(acts[-1], k), patches(errs[-1], k), w.reshape(-1, f)
        pre = p @ wm + b
        e = T._contract(_as_rows(p), _as_rows(ep), wm, np.zeros_like(wm), wm.shape[0] + 1, np.abs(b)).reshape(pre.shape)
        pres.append((pre, e))
        acts.append(np.where(pre < 0, 0.0, pre) if relu else pre)
        errs.append(e)
    n, nx, ny, filters = acts[-1].shape
    n_pix = nx * ny
    rows = (np.asarray(idx)[:, None] * n_pix + np.arange(n_pix)[None, :]).reshape(-1)
    last, e_last = _as_rows(acts[-1]), _as_rows(errs[-1])
    wo, bo = _f64(out_kernel), _f64(out_bias)
    yhat = last @ wo + bo
    e_y = T._contract(last, e_last, wo, np.zeros_like(wo), filters + 1, np.abs(bo))

    # the loss and its gradient: train_np.step's composition
    wn = loss.wnorm(rows.shape[0])
    dy, value, bound = T.mse_grad(yhat, loss.scale, loss.center, loss.inv_cstd2, loss.lo, loss.hi, loss.keep, wn, targets, rows)
    scale, center, keep = _f64(loss.scale), _f64(loss.center), _f64(loss.keep) != 0
    lo, hi, inv = _f64(loss.lo), _f64(loss.hi), _f64(loss.inv_cstd2)
    factor = np.where(keep, 2.0 * inv * scale * _f64(wn), 0.0)
    ep = e_y * np.abs(scale) + 4 * U * (np.abs(yhat * scale) + np.abs(center))
    e_dy = bound + ep * np.abs(factor)
    p = yhat * scale + center
    t = T.rows(targets, rows)
    for edge in (lo, hi):
        with np.errstate(invalid="ignore"):
            near = np.abs(p - edge) <= ep
        d_full = np.abs((np.clip(p, lo, hi) - t) * factor)
        e_dy = np.where(near & keep, e_dy + d_full + ep * np.abs(factor), e_dy)
    with np.errstate(invalid="ignore"):
        pc = np.clip(p, lo, hi)
        d = np.where(keep, np.abs(pc - t), 0.0)
        e_d = np.where(keep, ep + 2 * U * (np.abs(pc) + np.abs(t)), 0.0)
    loss_bound = float(np.sum((2 * d * e_d + e_d * e_d) * inv * _f64(wn))) + 1e-14 * abs(value)

    def masked(da, e_da, layer):   # through the ReLU that produced acts[layer + 1]
        if not relu:
            return da, e_da
        pre, e_pre = pres[layer]
        pre, e_pre = pre.reshape(da.shape), e_pre.reshape(da.shape)
        unsure = np.abs(pre) <= e_pre
        return np.where(pre > 0, da, 0.0), np.where(unsure, np.abs(da) + e_da, np.where(pre > 0, e_da, 0.0))

    grads, bounds = [None] * (n_hidden + 1), [None] * (n_hidden + 1)
    n_rows = rows.shape[0]
    grads[-1] = (last.T @ dy, dy.sum(axis=0))
    bounds[-1] = (T._contract(last.T, e_last.T, dy, e_dy, n_rows) + 1e-37,
                  e_dy.sum(axis=0) + 2.0 * n_rows * U * (np.abs(dy) + e_dy).sum(axis=0) + 1e-37)
    da = dy @ wo.T
    e_da = T._contract(dy, e_dy, wo.T, np.zeros_like(wo.T), wo.shape[1])
    da, e_da = masked(da, e_da, n_hidden - 1)
    dh, e_dh = da.reshape(acts[-1].shape), e_da.reshape(acts[-1].shape)
    for l in range(n_hidden - 1, -1, -1):
        w = _f64(hidden_kernels[l])
        k, c, f = w.shape[0], w.shape[2], w.shape[3]
        pa, pe = _as_rows(patches(acts[l], k)), _as_rows(patches(errs[l], k))
        d2, e2 = _as_rows(dh), _as_rows(e_dh)
        m = d2.shape[0]
        grads[l] = ((pa.T @ d2).reshape(k, k, c, f), d2.sum(axis=0))
        bounds[l] = (T._contract(pa.T, pe.T, d2, e2, m).reshape(k, k, c, f) + 1e-37,
                     e2.sum(axis=0) + 2.0 * m * U * (np.abs(d2) + e2).sum(axis=0) + 1e-37)
        if l > 0:
            dp, de, wf = patches(_padded(dh, k), k), patches(_padded(e_dh, k), k), _flipped(w)
            da = dp @ wf
            e_da = T._contract(_as_rows(dp), _as_rows(de), wf, np.zeros_like(wf), k * k * f).reshape(da.shape)
            dh, e_dh = masked(da, e_da, l - 1)
    return grads, bounds, value, loss_bound


def update(params, grads, m, v, t, lr=1e-3, constrained=()):
    """``train_np.adam`` on every array of ``params`` (lists alike), then ``constrain`` on the arrays whose position is in
    ``constrained`` -- the order of ``ConvTrainer.step``.  Returns the new (params, m, v)."""
    out = [T.adam(p, g, mm, vv, t, lr=lr) for p, g, mm, vv in zip(params, grads, m, v)]
    new_p = [constrain(o[0]) if i in constrained else o[0] for i, o in enumerate(out)]
    return new_p, [o[1] for o in out], [o[2] for o in out]


# ---- the tiny training problem shared by the host and the GPU tests -----------------------------------------------------------
TINY_INPUTS, TINY_OUTPUTS = ["field", "surface"], ["tendency", "flux"]


def tiny_cube(n_samples=3, n=8, seed=7):
    """name -> float32 ``[sample, tile, x, y, z]`` (``surface`` and ``flux``: ``[sample, tile, x, y]``): six ``n`` x ``n`` tiles,
    two inputs of 4 and 1 levels, two outputs of 3 and 1 levels that are a fixed function of the inputs."""
    rng = np.random.default_rng(seed)
    field = (280 + 20 * rng.normal(0, 1, (n_samples, 6, n, n, 4))).astype(np.float32)
    surface = rng.uniform(0, 1, (n_samples, 6, n, n)).astype(np.float32)
    x = np.concatenate([(field - 280) / 20, surface[..., None] - 0.5], axis=-1)
    hidden = np.tanh(x @ rng.normal(0, 1, (5, 6)))
    y = hidden @ rng.normal(0, 1, (6, 4))
    return {"field": field, "surface": surface, "tendency": (1e-3 * y[..., :3] + 2e-3).astype(np.float32),
            "flux": (50 * y[..., 3] - 10).astype(np.float32)}


def evaluate_loss(spec, cube, inputs=TINY_INPUTS, outputs=TINY_OUTPUTS, nfit=30):
    """The training loss of a ConvSpec-shaped ``spec`` on the whole ``cube``: per output the mean of
    ``((prediction - target) / std)^2`` with the float32 std of the first ``nfit`` tile-samples, added up."""
    five = lambda a: a if a.ndim == 5 else a[..., None]
    prep = prepare([five(cube[v]) for v in inputs], [five(cube[v]) for v in outputs], conv_np.halos_required(
        int(np.shape(spec.hidden_kernels[0])[0]), len(spec.hidden_kernels) + 1), nfit)
    pred = conv_np.forward(spec, dict(zip(inputs, prep["X"])))
    total = 0.0
    for name, y in zip(outputs, prep["y"]):
        std = np.std(y[:nfit].reshape(-1, y.shape[-1]), axis=0, dtype=np.float32).astype(np.float64)
        total += float(np.mean(((pred[name] - _f64(y)) / std) ** 2))
    return total
