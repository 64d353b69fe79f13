"""CPU references and launch helpers of the CycleGAN training-layer tests.

The reference of every convolution case is torch's autograd on the CPU through ``append_halos_tensor`` (or zero ``F.pad``), then
``F.conv2d`` / ``F.conv_transpose2d`` + crop, as ``cyclegan_cases.torch_layer`` evaluates the layer forwards."""
import os

import numpy as np
import torch

import cyclegan_cases as cc
from fv3net_amd.fit import cyclegan_train as ct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cyclegan_train_reference.npz")

F = torch.nn.functional

KIND_CASES = [("regular", 3), ("regular", 5), ("regular", 7), ("strided", 3), ("strided", 4), ("transposed", 4)]


def out_edge(kind, n):
    return {"regular": n, "strided": n // 2, "transposed": 2 * n}[kind]


def torch_weight_shape(kind, c_in, c_out, k):
    return (c_in, c_out, k, k) if kind == "transposed" else (c_out, c_in, k, k)


def kernel_weight(kind, w):
    """torch's layout -> the kernels' (``[k][k][c_in][c_out]``, or the parity split of the transposed kind)."""
    from fv3net_amd.cyclegan import split_transposed_weight

    w = np.asarray(w)
    return np.ascontiguousarray(split_transposed_weight(w) if kind == "transposed" else w.transpose(2, 3, 1, 0))


def torch_forward(kind, k, halo, t, w, b):
    """``t`` ``[S, 6, n, n, c]`` tensor -> ``[S, 6, n_out, n_out, c_out]`` tensor, differentiable."""
    S, _, n, _, c = t.shape
    h = 1 if kind != "regular" else (k - 1) // 2
    p = cc.pad(t.permute(0, 1, 4, 2, 3), h, halo).reshape(S * 6, c, n + 2 * h, n + 2 * h)
    if kind == "transposed":
        y = F.conv_transpose2d(p, w, b, stride=2)[..., 3:-3, 3:-3]
    else:
        y = F.conv2d(p, w, b, stride=2 if kind == "strided" else 1)
    return y.reshape(S, 6, y.shape[1], y.shape[2], y.shape[3]).permute(0, 1, 3, 4, 2)


def torch_backward(kind, k, halo, x, w, dy, dtype=torch.float64):
    """Autograd on the CPU: (y, dx, dw in the kernels' layout, db) as numpy arrays of ``dtype``."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_()
    wt = torch.from_numpy(np.ascontiguousarray(w)).to(dtype).requires_grad_()
    c_out = w.shape[1] if kind == "transposed" else w.shape[0]
    b = torch.zeros(c_out, dtype=dtype, requires_grad=True)
    y = torch_forward(kind, k, halo, t, wt, b)
    y.backward(torch.from_numpy(np.ascontiguousarray(dy)).to(dtype))
    return y.detach().numpy(), t.grad.numpy(), kernel_weight(kind, wt.grad.numpy()), b.grad.numpy()


def torch_abs_bound(kind, k, halo, x, w, dy):
    """Per element of (dx, dw, db): the sum of |a| |b| over the element's own terms -- the same adjoint on absolute values."""
    _, dx, dw, db = torch_backward(kind, k, halo, np.abs(x), np.abs(w), np.abs(dy))
    return dx, dw, db


def _slice(device, a, off, width, fill):
    """``a`` ``[S, 6, n, n, c]`` at channel ``off`` of rows ``width`` wide on the device -> (tensor, _Slice)."""
    from fv3net_amd.cube import _Slice

    buf, ld, _ = cc.gapped(a, off, width, fill=fill)
    t = torch.from_numpy(buf).to(device)
    return t, _Slice(t, ld, off)


def device_forward(device, kind, k, halo, x, w, bias=None, src_off=0, src_width=None):
    """``ops.cyclegan_train_conv`` -> ``[S, 6, n_out, n_out, c_out]`` numpy."""
    from fv3net_amd import ops

    S, _, n, _, c_in = x.shape
    wk = torch.from_numpy(kernel_weight(kind, w)).to(device)
    c_out = wk.shape[-1]
    _, xs = _slice(device, x, src_off, src_width, np.nan)
    n_out = out_edge(kind, n)
    yt, ys = _slice(device, np.full((S, 6, n_out, n_out, c_out), cc.SENTINEL, np.float32), 0, None, cc.SENTINEL)
    b = None if bias is None else torch.from_numpy(bias).to(device)
    ops.cyclegan_train_conv(xs, wk, b, ys, S, n, c_in, c_out, kind, k, halo)
    torch.cuda.synchronize(device)
    return yt.cpu().numpy().reshape(S, 6, n_out, n_out, c_out)


def device_backward(device, kind, k, halo, x, w, dy, x_off=0, x_width=None, dy_off=0, dy_width=None, dx_off=0, dx_width=None):
    """``ops.cyclegan_train_backward_data`` and ``_backward_weight`` -> (dx buffer ``[S, 6, n, n, ld]``, dw, db) numpy; the
    sources sit in NaN-filled buffers, the results in sentinel-filled ones."""
    from fv3net_amd import ops

    S, _, n, _, c_in = x.shape
    wk = torch.from_numpy(kernel_weight(kind, w)).to(device)
    c_out = wk.shape[-1]
    _, xs = _slice(device, x, x_off, x_width, np.nan)
    _, gs = _slice(device, dy, dy_off, dy_width, np.nan)
    dxt, dxs = _slice(device, np.full(x.shape, cc.SENTINEL, np.float32), dx_off, dx_width, cc.SENTINEL)
    ws = torch.full((max(1, ops.cyclegan_train_backward_data_workspace_floats(S, n, c_in, kind, k, halo)),), np.nan, device=device)
    ops.cyclegan_train_backward_data(gs, wk, dxs, S, n, c_in, c_out, kind, k, halo, ws)
    dw, db = torch.full_like(wk, cc.SENTINEL), torch.full((c_out,), cc.SENTINEL, device=device)
    ws2 = torch.full((ops.cyclegan_train_backward_weight_workspace_floats(S, n, c_in, c_out, kind, k),), np.nan, device=device)
    ops.cyclegan_train_backward_weight(xs, gs, dw, db, S, n, c_in, c_out, kind, k, halo, ws2)
    torch.cuda.synchronize(device)
    return dxt.cpu().numpy().reshape(S, 6, n, n, dxs.ld), dw.cpu().numpy(), db.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# -- the trainer's configuration and batches ----------------------------------------------------------
def fixture_config(**changes):
    """The network configuration of the reference fixture (tests/golden/make_cyclegan_train_golden.py)."""
    fields = dict(optimizer=dict(name="Adam", kwargs=dict(lr=2e-4)), generator=dict(n_convolutions=2, n_resnet=2, max_filters=12),
                  discriminator=dict(n_convolutions=2, max_filters=8, strided_kernel_size=3, use_geographic_embedded_bias=True),
                  convolution_type="halo_conv2d", identity_loss=dict(loss_type="mae"), cycle_loss=dict(loss_type="mae"),
                  gan_loss=dict(loss_type="mse"), identity_weight=0.5, cycle_weight=10.0, generator_weight=1.0, discriminator_weight=1.0)
    fields.update(changes)
    return ct.CycleGANNetworkConfig(**fields)


def training_batches(n_batches=3, samples=2, seed=0):
    """Pairs (mapping_a, mapping_b) of raw fields at nx = 12: a 2-level and a 1-level variable, one time per sample."""
    rng = np.random.default_rng(seed)

    def mapping():
        return {"time": (1.7e9 + 977 + 3600.0 * rng.integers(0, 48, (samples, 1))).astype(np.float32).astype(np.float64),
                "air_temperature": 250 + 10 * rng.normal(0, 1, (samples, 1, 6, 12, 12, 2)),
                "surface_pressure": 1e5 + 1e3 * rng.normal(0, 1, (samples, 1, 6, 12, 12))}

    return [(mapping(), mapping()) for _ in range(n_batches)]


def training_hyperparameters(**training):
    return ct.CycleGANHyperparameters(["air_temperature", "surface_pressure"], network=fixture_config(),
                                       training=dict(n_epoch=1, samples_per_batch=2, **training))
