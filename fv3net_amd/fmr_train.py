"""Training layers of the FMR recurrent generator on the MI355X: the convolution with context channels under
autograd and ``HipRecurrentGenerator``, built from it and from the CycleGAN training layers (``cyclegan_train``: the cube
convolution, the instance norm, their conventions).

A layer that reads context channels -- x, y, z of every cell, and sin / cos of the clock in the step layers -- holds its
parameter as the source rows ``weight`` ``[k, k, c_in, c_out]`` and the context rows ``weight_ctx``
``[k, k, c_cell + c_uni, c_out]``, as ``fv3hip_cyclegan_conv_context`` reads them; torch's layout concatenates the two along
``c_in``.  The context is never stored with the activations and has no gradient: backward-data is the plain layer's on the
source rows, backward-weight is ``fv3hip_cyclegan_train_backward_weight_context``.  There is no fallback: the modules need the GPU.
"""
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from .cube import _Slice
from .cyclegan import CONVOLUTION_TYPES, check_convolution_type
from .cyclegan_train import CubeConv, _check_activation, instance_norm_act, kernel_weight, torch_weight
from .fmr import RecurrentGeneratorSpec, clock_table

nn = torch.nn


class _ContextConvFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, w_ctx, b, ctx_cell, ctx_uniform, k, halo):
        c_in, c_out = int(w.shape[-2]), int(w.shape[-1])
        x = _check_activation(x, c_in, "the input of a context convolution")
        S, n = int(x.shape[0]), int(x.shape[2])
        y = torch.empty((S, 6, n, n, c_out), dtype=torch.float32, device=x.device)
        if S:
            ops.cyclegan_train_conv_context(_Slice(x, c_in), w, w_ctx, b, ctx_cell, ctx_uniform, _Slice(y, c_out), S, n, c_in, c_out, k, halo)
        ctx.save_for_backward(x, w, ctx_cell, ctx_uniform)
        ctx.geometry = (k, halo, tuple(w_ctx.shape))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, ctx_cell, ctx_uniform = ctx.saved_tensors
        k, halo, ctx_shape = ctx.geometry
        c_in, c_out = int(w.shape[-2]), int(w.shape[-1])
        S, n = int(x.shape[0]), int(x.shape[2])
        c_cell, c_uni = 0 if ctx_cell is None else int(ctx_cell.shape[-1]), 0 if ctx_uniform is None else int(ctx_uniform.numel())
        dy = dy.contiguous()
        new = (lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)) if S else \
            (lambda *shape: torch.zeros(shape, dtype=torch.float32, device=x.device))
        dx = dw = dw_ctx = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if S:
                floats = ops.cyclegan_train_backward_data_workspace_floats(S, n, c_in, "regular", k, halo)
                ops.cyclegan_train_backward_data(_Slice(dy, c_out), w, _Slice(dx, c_in), S, n, c_in, c_out, "regular", k, halo,
                                                 new(floats) if floats else None)
        if any(ctx.needs_input_grad[1:4]):
            dw, dw_ctx, db = new(*w.shape), new(*ctx_shape), new(c_out)
            if S:
                floats = ops.cyclegan_train_backward_weight_context_workspace_floats(S, n, c_in, c_cell, c_uni, c_out, k)
                ops.cyclegan_train_backward_weight_context(_Slice(x, c_in), _Slice(dy, c_out), ctx_cell, ctx_uniform, dw, dw_ctx, db, S, n,
                                                           c_in, c_out, k, halo, new(floats))
        return dx, dw, dw_ctx, db, None, None, None, None


def context_conv(x, weight, weight_ctx, bias, ctx_cell: Optional[torch.Tensor], ctx_uniform: Optional[torch.Tensor], k: int, halo: bool):
    """The regular cube convolution of ``x || ctx_cell || ctx_uniform`` under autograd; ``x`` un-padded ``[S, 6, n, n, c_in]``,
    ``ctx_cell`` ``[6, n, n, c_cell]`` and ``ctx_uniform`` ``[c_uni]`` (either None), the weights in the kernels' layout."""
    return _ContextConvFunction.apply(x, weight, weight_ctx, bias, ctx_cell, ctx_uniform, int(k), bool(halo))


class ContextConv(nn.Module):
    """One regular convolution over the cube whose last ``c_ctx`` input channels are context channels."""

    def __init__(self, c_in: int, c_ctx: int, c_out: int, k: int, convolution_type: str = "halo_conv2d"):
        super().__init__()
        check_convolution_type(convolution_type)
        if c_ctx < 1:
            raise ValueError("a context convolution needs at least one context channel; without one it is a CubeConv")
        self.k, self.halo = int(k), CONVOLUTION_TYPES[convolution_type] == _lib.CYCLEGAN_HALO_CUBE
        self.weight = nn.Parameter(torch.zeros((self.k, self.k, c_in, c_out)))
        self.weight_ctx = nn.Parameter(torch.zeros((self.k, self.k, c_ctx, c_out)))
        self.bias = nn.Parameter(torch.zeros(c_out))

    def load_torch(self, weight, bias):
        """Parameters in ``Conv2d``'s layout ``[c_out, c_in + c_ctx, k, k]``, the context channels last."""
        w = kernel_weight("regular", np.asarray(weight, np.float32))
        c_in = int(self.weight.shape[2])
        with torch.no_grad():
            self.weight.copy_(torch.from_numpy(np.ascontiguousarray(w[:, :, :c_in])))
            self.weight_ctx.copy_(torch.from_numpy(np.ascontiguousarray(w[:, :, c_in:])))
            self.bias.copy_(torch.from_numpy(np.asarray(bias, np.float32)))

    def torch_arrays(self):
        w = np.concatenate([self.weight.detach().cpu().numpy(), self.weight_ctx.detach().cpu().numpy()], axis=2)
        return torch_weight("regular", w), self.bias.detach().cpu().numpy().copy()

    def forward(self, x, ctx_cell=None, ctx_uniform=None):
        return context_conv(x, self.weight, self.weight_ctx, self.bias, ctx_cell, ctx_uniform, self.k, self.halo)


class HipRecurrentGenerator(nn.Module):
    """``RecurrentGeneratorTwin`` on the training kernels: the layers of ``fmr.layer_plan`` in order, activations channel-last.
    ``forward(state, ntime)``: ``state`` ``[S, 6, n, n, C]`` float32 -> ``[S, ntime, 6, n, n, C]``, bit for bit
    ``RecurrentGeneratorModel.forward`` on the same parameters.

    The ``ntime - 1`` steps run first and keep their latents (step ``i`` reads the clock at ``i - 1``, forwards and backwards);
    then all times are decoded in one batched call over ``ntime * S`` samples, time-major, so that every decoder layer has one
    forward and one weight-gradient launch whatever ``ntime``.  The result is the ``[S, ntime, ...]`` view of that
    ``[ntime, S, ...]`` tensor: its states are contiguous, its window stride is the smaller one."""

    def __init__(self, spec: RecurrentGeneratorSpec, convolution_type: str = "halo_conv2d"):
        super().__init__()
        spec.validate()
        self.convolution_type = convolution_type
        c_cell, c_uni = spec.context_channels
        self.convs = nn.ModuleDict()
        for name, kind, ci, co, k, _ in spec.plan:
            n_ctx = c_cell if name == "first" else c_cell + c_uni if name.endswith(".a") else 0
            conv = ContextConv(ci - n_ctx, n_ctx, co, k, convolution_type) if n_ctx else CubeConv(ci, co, kind, k, convolution_type)
            conv.load_torch(spec.weights[name], spec.biases[name])
            self.convs[name.replace(".", "_")] = conv
        last = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).transpose(0, 2, 3, 1)))   # noqa: E731
        self.input_bias = nn.Parameter(last(spec.input_bias)) if spec.use_geographic_bias else None
        self.output_bias = nn.Parameter(last(spec.output_bias)) if spec.use_geographic_bias else None
        self.use_geographic_features = spec.use_geographic_features
        if self.use_geographic_features:
            self.register_buffer("xyz", last(spec.xyz), persistent=False)
            self.register_buffer("xyz_bottom", last(spec.xyz_bottom), persistent=False)
        self.samples_per_day = spec.samples_per_day
        if self.samples_per_day is not None:
            self.register_buffer("clock", torch.from_numpy(clock_table(self.samples_per_day)), persistent=False)
        self.n_convolutions, self.step_type, self.step_stems = spec.n_convolutions, spec.step_type, list(spec.step_stems)
        self._spec_fields = dict(channels=spec.channels, nx=spec.nx, n_convolutions=spec.n_convolutions, n_resnet=spec.n_resnet,
                                 kernel_size=spec.kernel_size, strided_kernel_size=spec.strided_kernel_size,
                                 max_filters=spec.max_filters, step_type=spec.step_type, samples_per_day=spec.samples_per_day)

    def _context(self, name, x, ctx_cell=None, ctx_uniform=None):
        conv = self.convs[name]
        return conv(x, ctx_cell, ctx_uniform) if isinstance(conv, ContextConv) else conv(x)

    def encode(self, state):
        x = state if self.input_bias is None else state + self.input_bias
        x = instance_norm_act(self._context("first", x, self.xyz if self.use_geographic_features else None), None, 0.0)
        for level in range(self.n_convolutions):
            x = instance_norm_act(self.convs[f"down{level}"](x), None, 0.0)
        return x

    def step(self, x, i: int):
        """Step ``i`` (1-based) of the latent: the clock is at ``(i - 1) % samples_per_day``."""
        cell = self.xyz_bottom if self.use_geographic_features else None
        uniform = None if self.samples_per_day is None else self.clock[(int(i) - 1) % self.samples_per_day]
        for stem in self.step_stems:
            y = instance_norm_act(self._context(f"{stem}_a", x, cell, uniform), None, 0.0)
            if self.step_type == "resnet":
                x = instance_norm_act(self.convs[f"{stem}_b"](y), None, 1.0) + x
            else:
                x = instance_norm_act(self.convs[f"{stem}_b"](y), None, 0.0)
        return x

    def decode(self, x):
        for level in reversed(range(self.n_convolutions)):
            x = instance_norm_act(self.convs[f"up{level}"](x), None, 0.0)
        x = self.convs["last"](x)
        return x if self.output_bias is None else x + self.output_bias

    def forward(self, state, ntime: int):
        ntime = int(ntime)
        if ntime < 1:
            raise ValueError(f"ntime must be at least 1, got {ntime}")
        S = int(state.shape[0])
        latents = [self.encode(state)]
        for i in range(1, ntime):
            latents.append(self.step(latents[-1], i))
        out = self.decode(torch.cat(latents, dim=0) if ntime > 1 else latents[0])
        return out.view(ntime, S, *out.shape[1:]).transpose(0, 1)

    def to_spec(self) -> RecurrentGeneratorSpec:
        """The parameters as they stand, in torch's layout."""
        weights, biases = {}, {}
        for key, conv in self.convs.items():
            name = key.replace("_", ".")
            weights[name], biases[name] = conv.torch_arrays()
        first = lambda p: None if p is None else np.ascontiguousarray(p.detach().cpu().numpy().transpose(0, 3, 1, 2))   # noqa: E731
        geo = self.use_geographic_features
        return RecurrentGeneratorSpec(weights=weights, biases=biases, input_bias=first(self.input_bias), output_bias=first(self.output_bias),
                                      xyz=first(self.xyz) if geo else None, xyz_bottom=first(self.xyz_bottom) if geo else None,
                                      **self._spec_fields)
