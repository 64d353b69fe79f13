"""Specs, inputs and CPU evaluations of the FMR tests: weights drawn as N(0, 1 / fan_in), the state as N(0, 1).

The float64 truth of a rollout is ``RecurrentGeneratorTwin`` converted with ``.double()`` (the ``xyz`` tables too; the clock's
sin and cos stay the float32 values, as in the reference); the float32 chain is the same twin as it is.  A single context
convolution is torch's ``conv2d`` on the ``append_halos_tensor``-padded or zero-padded concatenation of the transformed source,
the per-cell context and the uniform context.
"""
import numpy as np
import torch

import cyclegan_cases as cc

F = torch.nn.functional
ORDER = ("time", "tile", "x", "y", "z")


def grid_xyz(nx):
    return cc.synthetic_grid(nx)[1]


def make_generator(rng, channels, nx, n_convolutions, n_resnet, max_filters, step_type="resnet", samples_per_day=4, kernel_size=3,
                   bias=True, features=True):
    from fv3net_amd.cyclegan import weight_shape
    from fv3net_amd.fmr import RecurrentGeneratorSpec, layer_plan

    weights, biases = {}, {}
    for name, kind, ci, co, k, _ in layer_plan(channels, n_convolutions, n_resnet, kernel_size, max_filters, step_type, features, samples_per_day):
        taps = 4 if kind == "transposed" else k * k
        weights[name] = (rng.normal(0, 1, weight_shape(kind, ci, co, k)) / np.sqrt(ci * taps)).astype(np.float32)
        biases[name] = rng.normal(0, 0.1, co).astype(np.float32)
    geo = lambda: rng.normal(0, 0.3, (6, channels, nx, nx)).astype(np.float32)
    return RecurrentGeneratorSpec(channels, nx, weights, biases, n_convolutions, n_resnet, kernel_size, 4, max_filters, step_type,
                                  samples_per_day, geo() if bias else None, geo() if bias else None,
                                  grid_xyz(nx) if features else None, grid_xyz(nx >> n_convolutions) if features else None)


def make_spec(rng, variables, nx, n_convolutions, n_resnet, max_filters, convolution_type="halo_conv2d", **flags):
    """``variables``: name -> feature count.  Scalers as a temperature-like and a humidity-like field."""
    from fv3net_amd.fmr import FullModelReplacementSpec

    gen = make_generator(rng, sum(variables.values()), nx, n_convolutions, n_resnet, max_filters, **flags)
    scalers = {name: (rng.normal(0, 10, nf), rng.uniform(0.5, 2, nf) * 10.0 ** rng.integers(-3, 2)) for name, nf in variables.items()}
    return FullModelReplacementSpec(gen, list(variables.items()), scalers, convolution_type)


def make_dataset(rng, spec, n_times, dtype=np.float64, order=ORDER):
    """name -> (dims, array) of raw fields stored in the dim order ``order`` (a one-feature variable has no ``z``)."""
    n, out = spec.generator.nx, {}
    for name, nf in spec.variables:
        mean, std = spec.scalers[name]
        a = rng.normal(0, 1, (n_times, 6, n, n, nf)) * std + mean
        dims = list(order)
        if nf == 1:
            a, dims = a[..., 0], [d for d in order if d != "z"]
        canon = [d for d in ORDER if d in dims]
        out[name] = (tuple(dims), np.ascontiguousarray(np.transpose(a.astype(dtype), [canon.index(d) for d in dims])))
    return out


def pack(spec, arrays):
    """numpy's normalisation: ``float32((x - mean) / std)`` in float64, ``[time, 6, n, n, F]``."""
    cols = []
    for name, nf in spec.variables:
        a = np.asarray(arrays[name], np.float64)
        mean, std = spec.scalers[name]
        cols.append(((a if a.ndim == 5 else a[..., None]) - mean) / std)
    return np.concatenate(cols, axis=-1).astype(np.float32)


def windows(packed, timesteps):
    """predict.py:326-352 written by hand: ``[time, ...]`` -> ``[window, timesteps + 1, ...]``, window w from time w * timesteps."""
    n = (packed.shape[0] - 1) // timesteps
    return np.stack([packed[w * timesteps:w * timesteps + timesteps + 1] for w in range(n)])


def unpack(spec, state):
    """``float64(state) * std + mean`` per variable (no ``z`` for a one-feature variable)."""
    out, f0 = {}, 0
    for name, nf in spec.variables:
        mean, std = spec.scalers[name]
        a = np.asarray(state[..., f0:f0 + nf], np.float64) * std + mean
        out[name] = a[..., 0] if nf == 1 else a
        f0 += nf
    return out


def twin_of(generator, convolution_type, dtype=torch.float32):
    from fv3net_amd.fit.fmr import recurrent_twin_from_spec

    return recurrent_twin_from_spec(generator, convolution_type, dtype)


def twin_forward(generator, convolution_type, state, ntime, dtype=torch.float32):
    """The plain-torch twin on the CPU: ``state`` ``[S, 6, n, n, C]`` float32 (numpy) -> ``[S, ntime, 6, n, n, C]``."""
    x = torch.from_numpy(np.ascontiguousarray(state)).to(dtype).permute(0, 1, 4, 2, 3)
    with torch.no_grad():
        return twin_of(generator, convolution_type, dtype)(x, ntime).permute(0, 1, 2, 4, 5, 3).contiguous().numpy()


def time_channel(a):
    """``[S, time, 6, n, n, C]`` -> ``[S 6 n n, time C]``: one "level" per (time, channel), so that every time is gated on its own."""
    a = np.asarray(a)
    return np.ascontiguousarray(np.moveaxis(a, 1, -2)).reshape(-1, a.shape[1] * a.shape[-1])


def ratio_per_time(got, truth):
    """Per time the worst channel's max error over the channel's scale at that time."""
    g, t = time_channel(np.asarray(got, np.float64)), time_channel(np.asarray(truth, np.float64))
    scale = np.max(np.abs(t), axis=0)
    r = np.max(np.abs(g - t), axis=0) / np.where(scale == 0, 1, scale)
    return r.reshape(truth.shape[1], truth.shape[-1]).max(axis=1)


# -- the context convolution ----------------------------------------------------------------------
def torch_context_layer(k, halo, x, w, w_ctx, bias, ctx_cell=None, ctx_uniform=None, transform=None):
    """``x`` ``[S, 6, n, n, c]``; ``w`` ``[c_out, c, k, k]`` and ``w_ctx`` ``[c_out, c_cell + c_uni, k, k]`` in torch's layout;
    ``ctx_cell`` ``[6, n, n, c_cell]``, ``ctx_uniform`` ``[c_uni]``; ``transform`` as in ``cyclegan_cases.torch_layer``, applied to
    the source channels only, before concatenation and padding.  Returns ``[S, 6, n, n, c_out]``."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    if transform is not None:
        mean, rstd, cell_bias, relu = transform
        t = (t - torch.from_numpy(mean)[:, :, None, None]) * torch.from_numpy(rstd)[:, :, None, None]
        if cell_bias is not None:
            t = t + torch.from_numpy(cell_bias)
        if relu:
            t = torch.relu(t)
    S, _, n, _, c = t.shape
    parts = [t]
    if ctx_cell is not None:
        parts.append(torch.from_numpy(np.ascontiguousarray(ctx_cell)).expand(S, 6, n, n, -1))
    if ctx_uniform is not None:
        parts.append(torch.from_numpy(np.ascontiguousarray(ctx_uniform)).expand(S, 6, n, n, -1))
    t = torch.cat(parts, dim=-1)
    h = (k - 1) // 2
    p = cc.pad(t.permute(0, 1, 4, 2, 3), h, halo).reshape(S * 6, t.shape[-1], n + 2 * h, n + 2 * h)
    weight = torch.from_numpy(np.concatenate([w] + ([w_ctx] if w_ctx is not None else []), axis=1))
    y = F.conv2d(p, weight, None if bias is None else torch.from_numpy(bias))
    return y.reshape(S, 6, -1, n, n).permute(0, 1, 3, 4, 2).contiguous().numpy()


def device_context_layer(device, k, halo, x, w, w_ctx, bias, ctx_cell=None, ctx_uniform=None, transform=None, kind="regular",
                         src_off=0, src_width=None, out_bias=None, src_gap=0, dst_gap=0, dst_off=0, dst_width=None):
    """One ``fv3hip_cyclegan_conv_context`` launch; the result goes to a buffer filled with the sentinel -7.  Returns it (numpy).
    ``dst_off`` / ``dst_width`` and ``src_gap`` / ``dst_gap`` as in ``cyclegan_cases.device_layer``: with a ``dst_gap`` the whole
    flat buffer is returned."""
    from fv3net_amd import _lib
    from fv3net_amd.cyclegan import KINDS
    from fv3net_amd.ops import _stream

    S, _, n, _, c = x.shape
    c_out = w.shape[0]
    n_out = {"regular": n, "strided": n // 2, "transposed": 2 * n}[kind]
    wide, src_ld, src_ss = cc.gapped(x, src_off, src_width, src_gap)
    flat, dst_ld, dst_ss = cc.gapped(np.full((S, 6, n_out, n_out, c_out), cc.SENTINEL, np.float32), dst_off, dst_width, dst_gap, fill=cc.SENTINEL)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
    src, dst = up(wide), up(flat)
    mean, rstd, cell_bias, relu = transform or (None, None, None, False)
    held = [up(a) for a in (mean, rstd, cell_bias, bias, ctx_cell, ctx_uniform, out_bias)]
    wk, wc = up(np.asarray(w).transpose(2, 3, 1, 0)), None if w_ctx is None else up(np.asarray(w_ctx).transpose(2, 3, 1, 0))
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.call_on(device, "fv3hip_cyclegan_conv_context", src.data_ptr(), src_ld, src_off, src_ss if src_gap else 0, ptr(held[0]),
                 ptr(held[1]), ptr(held[2]), int(relu), wk.data_ptr(), ptr(held[3]), ptr(held[6]), dst.data_ptr(), dst_ld, dst_off,
                 dst_ss if dst_gap else 0, S, n, c, c_out, KINDS[kind], k, _lib.CYCLEGAN_HALO_CUBE if halo else _lib.CYCLEGAN_HALO_ZEROS,
                 ptr(held[4]), 0 if ctx_cell is None else ctx_cell.shape[-1], ptr(held[5]), 0 if ctx_uniform is None else ctx_uniform.shape[-1],
                 ptr(wc), _stream(device))
    torch.cuda.synchronize(device)
    out = dst.cpu().numpy()
    return out if dst_gap else out.reshape(S, 6, n_out, n_out, dst_ld)
