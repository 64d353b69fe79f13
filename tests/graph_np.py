"""Float64 numpy oracle of the graph U-Net autoregressor, written from the description of the reference
(external/fv3fit/fv3fit/pytorch/graph/graph_builder.py:12-49, graph/unet.py, pytorch/predict.py:136-387), for the tests only.

The graph: every cell has an edge from itself and from the four cells that the one-cell halo of ``append_halos`` shows around
it, so a "mean" aggregation over in-edges is ``(self + x-low + x-high + y-low + y-high) / 5``.  All arrays are
``[sample, tile, x, y, channel]``; ``spec`` is a ``fv3net_amd.graph.GraphUNetSpec`` (plain arrays).
"""
import numpy as np

import conv_np

ACTIVATIONS = conv_np.ACTIVATIONS


def neighbour_table(n):
    """``[6 n n, 5]`` ids: self, x-low, x-high, y-low, y-high, read off the padded id field as graph_builder.py does."""
    ids = np.arange(6 * n * n).reshape(6, n, n)
    p = conv_np.append_halos(ids, 1)
    return np.stack([ids, p[:, :-2, 1:-1], p[:, 2:, 1:-1], p[:, 1:-1, :-2], p[:, 1:-1, 2:]], axis=-1).reshape(-1, 5)


def edges(n):
    """(destination, source) of the 5 N edges."""
    table = neighbour_table(n)
    return np.repeat(table[:, 0], 5), table.reshape(-1)


def gather5(h):
    """``[S, 6, n, n, c]`` -> ``[S, 6, n, n, 5, c]``: every cell with its neighbours."""
    S, _, n, _, c = h.shape
    return h.reshape(S, -1, c)[:, neighbour_table(n)].reshape(S, 6, n, n, 5, c)


def mean5(h):
    g = gather5(h)
    return ((((g[..., 0, :] + g[..., 1, :]) + g[..., 2, :]) + g[..., 3, :]) + g[..., 4, :]) / 5


def sage(h, w_self, w_neigh, bias, activation="linear", neigh_first=False):
    """``act(h W_self + mean5(h) W_neigh + b)``; ``neigh_first``: ``W_neigh`` before the mean, as dgl does for c_in > c_out."""
    h = np.asarray(h, np.float64)
    w_self, w_neigh = np.asarray(w_self, np.float64), np.asarray(w_neigh, np.float64)
    with np.errstate(invalid="ignore"):   # (Inf - Inf and Inf * 0 are NaN on purpose in the non-finite tests)
        neigh = mean5(h @ w_neigh) if neigh_first else mean5(h) @ w_neigh
        return ACTIVATIONS[activation](h @ w_self + neigh + (0 if bias is None else np.asarray(bias, np.float64)))


def pool2(h):
    S, _, n, _, c = h.shape
    return np.asarray(h, np.float64).reshape(S, 6, n // 2, 2, n // 2, 2, c).mean(axis=(3, 5))


def up2(h, weight, bias):
    """``weight`` [c_in, 2, 2, c_out]: out[2i + di, 2j + dj] = bias + h[i, j] @ weight[:, di, dj]."""
    h, weight = np.asarray(h, np.float64), np.asarray(weight, np.float64)
    S, _, n, _, _ = h.shape
    out = np.empty((S, 6, 2 * n, 2 * n, weight.shape[-1]))
    for di in range(2):
        for dj in range(2):
            out[:, :, di::2, dj::2] = h @ weight[:, di, dj] + np.asarray(bias, np.float64)
    return out


def forward(spec, state):
    """One step on the normalised state ``[S, 6, n, n, F]``."""
    L, act = spec.layers, spec.activation
    run = lambda name, h, a=act: sage(h, L[name].w_self, L[name].w_neigh, L[name].bias, a)

    def unet(k, h):
        before = run(f"L{k}.conv1b", run(f"L{k}.conv1a", h))
        low = pool2(before)
        low = run("bottom.b", run("bottom.a", low)) if k == spec.depth - 1 else unet(k + 1, low)
        cat = np.concatenate([before, up2(low, L[f"L{k}.up"].weight, L[f"L{k}.up"].bias)], axis=-1)
        return run(f"L{k}.conv2b", run(f"L{k}.conv2a", cat))

    return run("last", unet(0, run("first", np.asarray(state, np.float64))), "linear")


def rollout(spec, state, timesteps, step=None):
    """``[S, 6, n, n, F]`` -> ``[S, timesteps + 1, ...]``; every step starts from the float32 value of the one before, as the
    reference's float32 output array makes it (predict.py:210-217)."""
    step = step or (lambda s: forward(spec, s))
    out = [np.asarray(state, np.float32)]
    for _ in range(timesteps):
        out.append(np.asarray(step(out[-1]), np.float32))
    return np.stack(out, axis=1)


def n_windows(n_times, timesteps):
    return (n_times - 1) // timesteps


def pack(spec, arrays, timesteps):
    """name -> ``[time, tile, x, y(, z)]`` -> float32 ``[window, timesteps + 1, tile, x, y, F]``: normalised in float64, windows
    that share their end points, trailing times dropped."""
    cols = []
    for v in spec.variables:
        a = np.asarray(arrays[v.name], np.float64)
        a = (a - (v.mean if a.ndim == 5 else v.mean[0])) / (v.std if a.ndim == 5 else v.std[0])
        cols.append(a if a.ndim == 5 else a[..., None])
    data = np.concatenate(cols, axis=-1)
    nw = n_windows(data.shape[0], timesteps)
    return np.stack([data[w * timesteps:w * timesteps + timesteps + 1] for w in range(nw)]).astype(np.float32)


def unpack(spec, state):
    """float32 ``[..., F]`` -> name -> float64 ``x * std + mean`` (a one-feature variable without its ``z`` axis)."""
    out, f = {}, 0
    for v in spec.variables:
        x = np.asarray(state[..., f:f + v.nfeat], np.float32).astype(np.float64)
        out[v.name] = (x * v.std + v.mean) if v.nfeat > 1 else (x[..., 0] * v.std[0] + v.mean[0])
        f += v.nfeat
    return out


def predict(spec, arrays, timesteps, step=None):
    """``(predicted, reference)`` as name -> ``[window, time, tile, x, y(, z)]``."""
    packed = pack(spec, arrays, timesteps)
    return unpack(spec, rollout(spec, packed[:, 0], timesteps, step)), unpack(spec, packed)
