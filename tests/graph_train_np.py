"""TEST INFRASTRUCTURE ONLY: float64 numpy restatement of what csrc/graph_train.hip computes -- the five backward entries of the
graph U-Net's layers and torch's AdamW -- with the absolute-product sums from which the tests derive their bounds, and the whole
network's multistep gradient (``network_gradients``) with those bounds carried through the layers as tests/train_np.py and
tests/conv_train_np.py carry them:

    a float32 contraction of length n in any order:  |got - exact| <= 2 n 2^-24 sum |a_i| |b_i|            
    mean5 (four sums, one division, the cast of the reference):  six roundings on mean5(|x|)
    tanh' = 1 - p^2 times v: four roundings on |v| (1 + p^2)
    an element whose mask (or tanh') is decided by a stored activation within that activation's own bound counts in full

Arrays are ``[S, 6, n, n, c]``; weights ``[c_in, c_out]`` (up: ``[c_in, 2, 2, c_out]``).
"""
import numpy as np

U = 2.0 ** -24
TINY = 1e-37


def _f64(a):
    return np.asarray(a, np.float64)


_TABLES = {}


def table(n):
    """``[6 n n, 5]`` cell ids (self, x-low, x-high, y-low, y-high across the seams): ``fit.graph.neighbour_table``."""
    if n not in _TABLES:
        from fv3net_amd.fit.graph import neighbour_table

        _TABLES[n] = neighbour_table(n).numpy().copy()
    return _TABLES[n]


def sum5(x):
    """The five-cell sum, in the kernel's order (((self + x-low) + x-high) + y-low) + y-high; any dtype."""
    x = np.asarray(x)
    S, _, n, _, c = x.shape
    g = x.reshape(S, 6 * n * n, c)[:, table(n)]   # [S, N, 5, c]
    return ((((g[:, :, 0] + g[:, :, 1]) + g[:, :, 2]) + g[:, :, 3]) + g[:, :, 4]).reshape(x.shape)


def mean5(x):
    return sum5(_f64(x)) / 5.0


def act_grad(p, act):
    """act'(.) from the stored output ``p``: relu [p > 0] (a NaN masks), tanh 1 - p^2, linear 1."""
    p = _f64(p)
    if act == "relu":
        with np.errstate(invalid="ignore"):
            return (p > 0).astype(np.float64)
    if act == "tanh":
        return 1.0 - p * p
    return np.ones_like(p)


def _mask(v, p, act):
    """(v act'(p), the rounding bound of that product): the tanh mask is four roundings on |v| (1 + p^2)."""
    if p is None or act == "linear":
        return v, np.zeros_like(v)
    extra = 4 * U * np.abs(v) * (1 + _f64(p) ** 2) if act == "tanh" else np.zeros_like(v)
    return v * act_grad(p, act), extra


def _mm(a, w):
    """[S, 6, n, n, c] @ [c, o]"""
    return a @ w


# ---- the five backward entries: (results ..., gates ...) ---------------------------------------------------------------------
def sage_backward_data(dh, w_self, w_neigh, p=None, act="linear"):
    """(dX, gate): dX = (dH W_self^T + mean5(dH) W_neigh^T) act'(P); one contraction of length 2 c_out."""
    dh, ws, wn = _f64(dh), _f64(w_self), _f64(w_neigh)
    with np.errstate(invalid="ignore"):
        v = _mm(dh, ws.T) + _mm(mean5(dh), wn.T)
        m5 = mean5(np.abs(dh))
        mag = _mm(np.abs(dh), np.abs(ws).T) + _mm(m5, np.abs(wn).T)
        gate = 2.0 * (2 * ws.shape[1]) * U * mag + 6 * U * _mm(m5, np.abs(wn).T)
        out, extra = _mask(v, p, act)
        if p is not None and act != "linear":
            gate = gate * np.abs(act_grad(p, act)) + extra
    return out, gate + TINY


def sage_backward_weight(x, g):
    """(dW_self, dW_neigh, db, gate_self, gate_neigh, gate_b): contractions over the S 6 n^2 cells."""
    x, g = _f64(x), _f64(g)
    cells = x.shape[0] * 6 * x.shape[2] ** 2
    xf, gf = x.reshape(cells, -1), g.reshape(cells, -1)
    mf, amf = mean5(x).reshape(cells, -1), mean5(np.abs(x)).reshape(cells, -1)
    with np.errstate(invalid="ignore"):
        dws, dwn, db = xf.T @ gf, mf.T @ gf, gf.sum(axis=0)
        gs = 2.0 * cells * U * (np.abs(xf).T @ np.abs(gf))
        gn = (2.0 * cells + 6) * U * (amf.T @ np.abs(gf))
        gb = 2.0 * cells * U * np.abs(gf).sum(axis=0)
    return dws, dwn, db, gs + TINY, gn + TINY, gb + TINY


def _fine(dcat):
    """[S, 6, 2n, 2n, co] -> [S, 6, n, n, 2, 2, co] (di, dj after the coarse cell)"""
    S, _, n2, _, co = dcat.shape
    n = n2 // 2
    return dcat.reshape(S, 6, n, 2, n, 2, co).transpose(0, 1, 2, 4, 3, 5, 6)


def up2_backward_data(dcat, w, p=None, act="linear"):
    """(dLow, gate): dLow[i][j][ci] = sum_{di,dj,co} dCat[2i+di][2j+dj][co] w[ci][di][dj][co], masked; length 4 c_out."""
    f, w = _fine(_f64(dcat)), _f64(w)
    with np.errstate(invalid="ignore"):
        v = np.einsum("stijabo,cabo->stijc", f, w)
        mag = np.einsum("stijabo,cabo->stijc", np.abs(f), np.abs(w))
        gate = 2.0 * (4 * w.shape[3]) * U * mag
        out, extra = _mask(v, p, act)
        if p is not None and act != "linear":
            gate = gate * np.abs(act_grad(p, act)) + extra
    return out, gate + TINY


def up2_backward_weight(low, dcat):
    """(dW, db, gate_w, gate_b): dW[ci][di][dj][co] = sum low[i][j][ci] dCat[2i+di][2j+dj][co]; db = sum dCat."""
    low, f = _f64(low), _fine(_f64(dcat))
    cells = low.shape[0] * 6 * low.shape[2] ** 2
    with np.errstate(invalid="ignore"):
        dw = np.einsum("stijc,stijabo->cabo", low, f)
        db = f.sum(axis=(0, 1, 2, 3, 4, 5))
        gw = 2.0 * cells * U * np.einsum("stijc,stijabo->cabo", np.abs(low), np.abs(f))
        gb = 2.0 * (cells + 4) * U * np.abs(f).sum(axis=(0, 1, 2, 3, 4, 5))
    return dw, db, gw + TINY, gb + TINY


def pool2_backward(dst, dpool, p=None, act="linear"):
    """(result, gate): (dst + 0.25 dPool[x/2][y/2]) act'(P): one sum (0.25 x is exact), then the mask."""
    dst, dpool = _f64(dst), _f64(dpool)
    spread = 0.25 * np.repeat(np.repeat(dpool, 2, axis=2), 2, axis=3)
    with np.errstate(invalid="ignore"):
        v = dst + spread
        gate = 2 * U * (np.abs(dst) + np.abs(spread))
        out, extra = _mask(v, p, act)
        if p is not None and act != "linear":
            gate = gate * np.abs(act_grad(p, act)) + extra
    return out, gate + TINY


# ---- torch.optim.AdamW (defaults: decoupled decay, no amsgrad) ---------------------------------------------------------------
def adamw(p, g, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2):
    """One update at step ``t`` (1-based) in float64; returns the new (p, m, v)."""
    p, g, m, v = (_f64(x) for x in (p, g, m, v))
    p = p * (1 - lr * weight_decay)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - beta2 ** t) + eps
    return p - (lr / (1 - beta1 ** t)) * m / denom, m, v


def adamw_f32(p, g, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2):
    """The same update rounded as torch's CPU kernels round it on float32 tensors (_single_tensor_adam): the decay is one
    product with the float32 scalar; exp_avg.lerp_(grad, 1 - beta1) is fma(w, g - m, m) for w < 0.5 (taken here in float64,
    where the product is exact, and rounded once); exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2) is
    v beta2 + ((1 - beta2) g) g; denom = sqrt(v) / bc2_sqrt + eps; p += (-step_size m) / denom."""
    f = np.float32
    p, g, m, v = (np.asarray(x, f) for x in (p, g, m, v))
    p = p * f(1 - lr * weight_decay)
    m = (np.float64(f(1 - beta1)) * (g - m).astype(np.float64) + m.astype(np.float64)).astype(f)
    v = v * f(beta2) + (f(1 - beta2) * g) * g
    step_size, bc2_sqrt = f(lr / (1 - beta1 ** t)), f(np.sqrt(1 - beta2 ** t))
    denom = np.sqrt(v) / bc2_sqrt + f(eps)
    return p - (step_size * m) / denom, m, v


# ---- the whole network with bounds carried through the layers ------------------------------------------------------------------
def _contract(a, ea, b, eb, n, extra=0.0):
    """|computed - exact| of a length-n float32 contraction of operands known to within ea, eb (``a @ b``)."""
    return ea @ np.abs(b) + np.abs(a) @ eb + ea @ eb + 2.0 * n * U * ((np.abs(a) + ea) @ (np.abs(b) + eb) + extra)


def _apply(pre, e, act):
    if act == "relu":
        return np.maximum(pre, 0), e
    if act == "tanh":
        y = np.tanh(pre)
        return y, e + 4 * U * np.abs(y) + TINY   # (tanh is 1-Lipschitz; tanhf within a few ulp)
    return pre, e


def sage_forward(x, ex, layer, act):
    """(output, its bound) of one SAGE layer on an input known to within ``ex``."""
    ws, wn, b = (_f64(a) for a in layer)
    c = ws.shape[0]
    m, em = mean5(x), mean5(ex) + 6 * U * mean5(np.abs(x))
    pre = x @ ws + m @ wn + b
    e = (ex @ np.abs(ws) + em @ np.abs(wn)
         + 2.0 * (2 * c + 1) * U * ((np.abs(x) + ex) @ np.abs(ws) + (np.abs(m) + em) @ np.abs(wn) + np.abs(b)))
    return _apply(pre, e, act)


def _grad_mask(v, ev, stored, e_stored, act):
    """v act'(stored) with the bound: an element whose act' is decided within the stored value's own bound counts in full."""
    if act == "linear":
        return v, ev
    if act == "relu":
        mask = stored > 0
        unsure = np.abs(stored) <= e_stored
        return np.where(mask, v, 0.0), np.where(unsure, np.abs(v) + ev, np.where(mask, ev, 0.0))
    d = 1.0 - stored * stored
    ed = 2 * np.abs(stored) * e_stored + e_stored ** 2
    return v * d, ev * (np.abs(d) + ed) + np.abs(v) * ed + 4 * U * (np.abs(v) + ev) * (1 + stored ** 2)


def _sage_bwd(x, ex, g, eg, layer, want_data):
    """(dWs, dWn, db, their bounds, dX, its bound) of one SAGE layer with input x and masked output gradient g."""
    ws, wn, _ = (_f64(a) for a in layer)
    cells = x.shape[0] * 6 * x.shape[2] ** 2
    xf, exf, gf, egf = (a.reshape(cells, -1) for a in (x, ex, g, eg))
    m, em = mean5(x).reshape(cells, -1), (mean5(ex) + 6 * U * mean5(np.abs(x))).reshape(cells, -1)
    grads = (xf.T @ gf, m.T @ gf, gf.sum(axis=0))
    bounds = (_contract(xf.T, exf.T, gf, egf, cells), _contract(m.T, em.T, gf, egf, cells),
              egf.sum(axis=0) + 2.0 * cells * U * (np.abs(gf) + egf).sum(axis=0))
    if not want_data:
        return grads, bounds, None, None
    co = ws.shape[1]
    mg, emg = mean5(g), mean5(eg) + 6 * U * mean5(np.abs(g))
    dx = g @ ws.T + mg @ wn.T
    edx = (eg @ np.abs(ws).T + emg @ np.abs(wn).T
           + 2.0 * (2 * co) * U * ((np.abs(g) + eg) @ np.abs(ws).T + (np.abs(mg) + emg) @ np.abs(wn).T))
    return grads, bounds, dx, edx


def network_gradients(layers, depth, min_filters, activation, batch, multistep):
    """``layers``: name -> (w_self, w_neigh, bias) | (weight, bias); ``batch`` ``[S, T, 6, n, n, F]``.  The gradient of the mean
    over the steps of the MSE of the state rolled out from time 0 (training_loop.py:136-148).  Returns ``(loss, grads, bounds,
    d_input, d_input_bound)`` with ``grads[name]`` a tuple like the layer's."""
    batch = _f64(batch)
    S, _, _, n, _, F = batch.shape
    from fv3net_amd.graph import layer_plan

    plan = layer_plan(depth, F, min_filters)
    act = activation
    zero = np.zeros_like
    steps = []
    state, e_state = batch[:, 0], zero(batch[:, 0])
    loss = 0.0
    for k in range(multistep):
        rec = {"in": (state, e_state)}
        x, ex = sage_forward(state, e_state, layers["first"], act)
        rec["first"] = (x, ex)
        for lev in range(depth):
            t, et = sage_forward(x, ex, layers[f"L{lev}.conv1a"], act)
            b, eb = sage_forward(t, et, layers[f"L{lev}.conv1b"], act)
            rec[f"L{lev}.x"], rec[f"L{lev}.t1"], rec[f"L{lev}.before"] = (x, ex), (t, et), (b, eb)
            nk = b.shape[2]
            pool = lambda a: a.reshape(S, 6, nk // 2, 2, nk // 2, 2, -1)
            sub = pool(b)
            x = (((sub[:, :, :, 0, :, 0] + sub[:, :, :, 0, :, 1]) + sub[:, :, :, 1, :, 0]) + sub[:, :, :, 1, :, 1]) * 0.25
            ex = pool(eb).mean(axis=(3, 5)) + 3 * U * pool(np.abs(b)).mean(axis=(3, 5))
        t, et = sage_forward(x, ex, layers["bottom.a"], act)
        low, elow = sage_forward(t, et, layers["bottom.b"], act)
        rec["bottom.x"], rec["bottom.t"] = (x, ex), (t, et)
        for lev in reversed(range(depth)):
            w, bias = (_f64(a) for a in layers[f"L{lev}.up"])
            ci = w.shape[0]
            up = np.einsum("stijc,cabo->stiajbo", low, w) + bias
            eup = (np.einsum("stijc,cabo->stiajbo", elow, np.abs(w))
                   + 2.0 * (ci + 1) * U * (np.einsum("stijc,cabo->stiajbo", np.abs(low) + elow, np.abs(w)) + np.abs(bias)))
            nk = 2 * low.shape[2]
            up, eup = up.reshape(S, 6, nk, nk, -1), eup.reshape(S, 6, nk, nk, -1)
            rec[f"L{lev}.low"] = (low, elow)
            b, eb = rec[f"L{lev}.before"]
            cat, ecat = np.concatenate([b, up], axis=-1), np.concatenate([eb, eup], axis=-1)
            t, et = sage_forward(cat, ecat, layers[f"L{lev}.conv2a"], act)
            low, elow = sage_forward(t, et, layers[f"L{lev}.conv2b"], act)
            rec[f"L{lev}.cat"], rec[f"L{lev}.t2"] = (cat, ecat), (t, et)
        rec["low0"] = (low, elow)
        y, ey = sage_forward(low, elow, layers["last"], "linear")
        rec["y"] = (y, ey)
        loss += float(np.mean((y - batch[:, k + 1]) ** 2)) / multistep
        steps.append(rec)
        state, e_state = y, ey

    wnorm = 1.0 / (S * 6 * n * n * F * multistep)
    grads = {name: None for name, *_ in plan}
    bounds = {name: None for name, *_ in plan}

    def add(name, g, b):
        if grads[name] is None:
            grads[name], bounds[name] = list(g), list(b)
        else:   # old + new, one more rounding
            for i in range(len(g)):
                grads[name][i] = grads[name][i] + g[i]
                bounds[name][i] = bounds[name][i] + b[i] + U * np.abs(grads[name][i])

    d_state, e_d_state = None, None
    for k in reversed(range(multistep)):
        rec = steps[k]
        y, ey = rec["y"]
        tgt = batch[:, k + 1]
        g = 2.0 * (y - tgt) * wnorm
        eg = 2.0 * wnorm * (ey + 2 * U * (np.abs(y) + np.abs(tgt))) + 4 * U * np.abs(g)
        if d_state is not None:
            g = g + d_state
            eg = eg + e_d_state + U * np.abs(g)
        (x, ex) = rec["low0"]
        gr, bd, dx, edx = _sage_bwd(x, ex, g, eg, layers["last"], True)
        add("last", gr, bd)
        g, eg = _grad_mask(dx, edx, x, ex, act)
        for lev in range(depth):
            (t, et), (cat, ecat) = rec[f"L{lev}.t2"], rec[f"L{lev}.cat"]
            gr, bd, dx, edx = _sage_bwd(t, et, g, eg, layers[f"L{lev}.conv2b"], True)
            add(f"L{lev}.conv2b", gr, bd)
            g, eg = _grad_mask(dx, edx, t, et, act)
            gr, bd, dcat, edcat = _sage_bwd(cat, ecat, g, eg, layers[f"L{lev}.conv2a"], True)
            add(f"L{lev}.conv2a", gr, bd)
            rec[f"L{lev}.dcat"] = (dcat, edcat)
            half = dcat.shape[-1] // 2
            gup, egup = dcat[..., half:], edcat[..., half:]
            (low, elow) = rec[f"L{lev}.low"]
            w = _f64(layers[f"L{lev}.up"][0])
            cells = low.shape[0] * 6 * low.shape[2] ** 2
            f, ef = _fine(gup), _fine(egup)
            dw = np.einsum("stijc,stijabo->cabo", low, f)
            edw = (np.einsum("stijc,stijabo->cabo", elow, np.abs(f)) + np.einsum("stijc,stijabo->cabo", np.abs(low) + elow, ef)
                   + 2.0 * cells * U * np.einsum("stijc,stijabo->cabo", np.abs(low) + elow, np.abs(f) + ef))
            db = f.sum(axis=(0, 1, 2, 3, 4, 5))
            edb = ef.sum(axis=(0, 1, 2, 3, 4, 5)) + 2.0 * (cells + 4) * U * (np.abs(f) + ef).sum(axis=(0, 1, 2, 3, 4, 5))
            add(f"L{lev}.up", (dw, db), (edw, edb))
            dlow = np.einsum("stijabo,cabo->stijc", f, w)
            edlow = (np.einsum("stijabo,cabo->stijc", ef, np.abs(w))
                     + 2.0 * (4 * w.shape[3]) * U * np.einsum("stijabo,cabo->stijc", np.abs(f) + ef, np.abs(w)))
            g, eg = _grad_mask(dlow, edlow, low, elow, act)
        (t, et), (x, ex) = rec["bottom.t"], rec["bottom.x"]
        gr, bd, dx, edx = _sage_bwd(t, et, g, eg, layers["bottom.b"], True)
        add("bottom.b", gr, bd)
        g, eg = _grad_mask(dx, edx, t, et, act)
        gr, bd, dpool, edpool = _sage_bwd(x, ex, g, eg, layers["bottom.a"], True)
        add("bottom.a", gr, bd)
        for lev in reversed(range(depth)):
            (dcat, edcat), (b, eb) = rec[f"L{lev}.dcat"], rec[f"L{lev}.before"]
            half = dcat.shape[-1] // 2
            spread = lambda a: 0.25 * np.repeat(np.repeat(a, 2, axis=2), 2, axis=3)
            v = dcat[..., :half] + spread(dpool)
            ev = edcat[..., :half] + spread(edpool) + 2 * U * (np.abs(dcat[..., :half]) + np.abs(spread(dpool)))
            g, eg = _grad_mask(v, ev, b, eb, act)
            (t, et), (x, ex) = rec[f"L{lev}.t1"], rec[f"L{lev}.x"]
            gr, bd, dx, edx = _sage_bwd(t, et, g, eg, layers[f"L{lev}.conv1b"], True)
            add(f"L{lev}.conv1b", gr, bd)
            g, eg = _grad_mask(dx, edx, t, et, act)
            gr, bd, dpool, edpool = _sage_bwd(x, ex, g, eg, layers[f"L{lev}.conv1a"], True)
            add(f"L{lev}.conv1a", gr, bd)
        (x, ex), (s_in, e_in) = rec["first"], rec["in"]
        g, eg = _grad_mask(dpool, edpool, x, ex, act)
        gr, bd, d_state, e_d_state = _sage_bwd(s_in, e_in, g, eg, layers["first"], True)
        add("first", gr, bd)
    grads = {k: tuple(v) for k, v in grads.items()}
    bounds = {k: tuple(b + TINY for b in v) for k, v in bounds.items()}
    return loss, grads, bounds, d_state, e_d_state + TINY
