"""Training layers of the CycleGAN on the MI355X: ``torch.autograd.Function``s over the
``fv3hip_cyclegan_train_*`` kernels and the modules built from them.

Activations are channel-last float32 ``[sample, 6, n, n, channel]`` without halos: the kernels resolve the cube seams themselves,
forwards and in both adjoints.  Parameters live in the kernels' weight layout (``[k][k][c_in][c_out]``, the transposed kind as
its parity split ``[px][py][a][b][c_in][c_out]``) and are converted to and from torch's layout only when a network is created
from a spec or exported to one; ``torch.optim``'s updates are element-wise, so training in this layout is exact.  PyTorch does
the plumbing: the residual and geographic-bias adds, the slice that is the adjoint of the feature concatenation, the leaky ReLU
of slope 0.2 on an un-activated output, the losses and the optimisers.  There is no fallback: the modules need the GPU.
"""
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from .cube import _Slice
from .cyclegan import (CONVOLUTION_TYPES, INSTANCE_NORM_EPS, GeneratorSpec, check_convolution_type, split_transposed_weight,
                       weight_shape)

nn = torch.nn


def merge_transposed_weight(w: np.ndarray) -> np.ndarray:
    """The inverse of ``split_transposed_weight``: ``[px, py, a, b, c_in, c_out]`` -> ``ConvTranspose2d``'s ``[c_in, c_out, 4, 4]``."""
    w = np.asarray(w)
    tap = lambda p, a: 1 + 2 * a if p == 0 else 2 * a   # noqa: E731
    out = np.empty(w.shape[4:] + (4, 4), w.dtype)
    for px in range(2):
        for py in range(2):
            for a in range(2):
                for b in range(2):
                    out[:, :, tap(px, a), tap(py, b)] = w[px, py, a, b]
    return out


def kernel_weight(kind: str, w) -> np.ndarray:
    """torch's layout -> the kernels'."""
    w = np.asarray(w)
    return np.ascontiguousarray(split_transposed_weight(w) if kind == "transposed" else w.transpose(2, 3, 1, 0))


def torch_weight(kind: str, w) -> np.ndarray:
    """The kernels' layout -> torch's."""
    w = np.asarray(w)
    return np.ascontiguousarray(merge_transposed_weight(w) if kind == "transposed" else w.transpose(3, 2, 0, 1))


def _out_edge(kind: str, n: int) -> int:
    return {"regular": n, "strided": n // 2, "transposed": 2 * n}[kind]


def _check_activation(x: torch.Tensor, channels: int, what: str) -> torch.Tensor:
    if x.dim() != 5 or x.shape[1] != 6 or x.shape[2] != x.shape[3] or x.shape[4] != channels:
        raise ValueError(f"{what} must be [sample, 6, n, n, {channels}], got {tuple(x.shape)}")
    if x.dtype != torch.float32 or not x.is_cuda:
        raise TypeError(f"{what} must be a float32 tensor on the GPU (there is no CPU fallback), got {x.dtype} on {x.device}")
    return x.contiguous()


class _CubeConvFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, kind, k, halo):
        c_in, c_out = int(w.shape[-2]), int(w.shape[-1])
        x = _check_activation(x, c_in, "the input of a cube convolution")
        S, n = int(x.shape[0]), int(x.shape[2])
        n_out = _out_edge(kind, n)
        y = torch.empty((S, 6, n_out, n_out, c_out), dtype=torch.float32, device=x.device)
        ops.cyclegan_train_conv(_Slice(x, c_in), w, b, _Slice(y, c_out), S, n, c_in, c_out, kind, k, halo)
        ctx.save_for_backward(x, w)
        ctx.geometry = (kind, k, halo, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        kind, k, halo, has_bias = ctx.geometry
        c_in, c_out = int(w.shape[-2]), int(w.shape[-1])
        S, n = int(x.shape[0]), int(x.shape[2])
        dy = dy.contiguous()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)   # noqa: E731
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if S:
                floats = ops.cyclegan_train_backward_data_workspace_floats(S, n, c_in, kind, k, halo)
                ops.cyclegan_train_backward_data(_Slice(dy, c_out), w, _Slice(dx, c_in), S, n, c_in, c_out, kind, k, halo,
                                                 new(floats) if floats else None)
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            dw, db = torch.zeros_like(w) if not S else torch.empty_like(w), None
            if has_bias:
                db = torch.zeros(c_out, device=x.device) if not S else new(c_out)
            if S:
                ops.cyclegan_train_backward_weight(_Slice(x, c_in), _Slice(dy, c_out), dw, db, S, n, c_in, c_out, kind, k, halo,
                                                   new(ops.cyclegan_train_backward_weight_workspace_floats(S, n, c_in, c_out, kind, k)))
        return dx, dw, db, None, None, None


def cube_conv(x, weight, bias, kind: str, k: int, halo: bool):
    """The cube convolution under autograd; ``x`` un-padded ``[S, 6, n, n, c_in]``, ``weight`` in the kernels' layout."""
    return _CubeConvFunction.apply(x, weight, bias, kind, int(k), bool(halo))


class _NormActFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, slope, relu_in_kernel):
        c = int(x.shape[-1])
        x = _check_activation(x, c, "the input of an instance norm")
        S, n = int(x.shape[0]), int(x.shape[2])
        st = torch.empty((2, S, 6, c), dtype=torch.float32, device=x.device)
        y = torch.empty_like(x)
        if S:
            stream = ops._stream(x.device)
            _lib.call_on(x.device, "fv3hip_cyclegan_stats", x.data_ptr(), c, 0, 0, st[0].data_ptr(), st[1].data_ptr(), S, n, c,
                         INSTANCE_NORM_EPS, stream)
            _lib.call_on(x.device, "fv3hip_cyclegan_apply", x.data_ptr(), c, 0, 0, st[0].data_ptr(), st[1].data_ptr(),
                         None if bias is None else bias.data_ptr(), int(relu_in_kernel), None, 1, 0, 0, y.data_ptr(), c, 0, 0, S, n, c,
                         stream)
        ctx.save_for_backward(x, st, bias)
        ctx.slope = float(slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, st, bias = ctx.saved_tensors
        c, S, n = int(x.shape[-1]), int(x.shape[0]), int(x.shape[2])
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dbias = None
        if bias is not None and ctx.needs_input_grad[1]:
            dbias = torch.zeros_like(bias) if not S else torch.empty_like(bias)
        if S:
            ops.cyclegan_train_norm_backward(_Slice(dy, c), _Slice(x, c), st[0], st[1], bias, ctx.slope, _Slice(dx, c), dbias, S, n, c)
        return dx, dbias, None, None


def instance_norm_act(x, bias: Optional[torch.Tensor] = None, slope: float = 0.0):
    """``act(instance_norm(x) + bias)`` under autograd: ``act`` a leaky ReLU of ``slope`` (0: ReLU, 1: none); ``bias``
    ``[6, n, n, c]`` or None.  Slopes 0 and 1 are ``fv3hip_cyclegan_stats`` + ``_apply`` as at predict time; any other slope is
    torch's ``leaky_relu`` on the un-activated output: its backward applies the mask (taken from that same float32
    pre-activation) and the kernel then runs with slope 1.  The kernel's own branch for a slope strictly between 0 and 1 is
    reached through ``ops.cyclegan_train_norm_backward`` only, not by the networks."""
    slope = float(slope)
    if slope in (0.0, 1.0):
        return _NormActFunction.apply(x, bias, slope, slope == 0.0)
    return torch.nn.functional.leaky_relu(_NormActFunction.apply(x, bias, 1.0, False), slope)


class CubeConv(nn.Module):
    """One convolution over the cube: ``weight`` in the kernels' layout, ``bias`` ``[c_out]``."""

    def __init__(self, c_in: int, c_out: int, kind: str, k: int, convolution_type: str = "halo_conv2d"):
        super().__init__()
        check_convolution_type(convolution_type)
        self.kind, self.k, self.halo = kind, int(k), CONVOLUTION_TYPES[convolution_type] == _lib.CYCLEGAN_HALO_CUBE
        shape = (2, 2, 2, 2, c_in, c_out) if kind == "transposed" else (self.k, self.k, c_in, c_out)
        self.weight, self.bias = nn.Parameter(torch.zeros(shape)), nn.Parameter(torch.zeros(c_out))

    def load_torch(self, weight, bias):
        """Parameters in torch's layout (``Conv2d`` / ``ConvTranspose2d``)."""
        with torch.no_grad():
            self.weight.copy_(torch.from_numpy(kernel_weight(self.kind, np.asarray(weight, np.float32))))
            self.bias.copy_(torch.from_numpy(np.asarray(bias, np.float32)))

    def torch_arrays(self):
        return (torch_weight(self.kind, self.weight.detach().cpu().numpy()), self.bias.detach().cpu().numpy().copy())

    def forward(self, x):
        return cube_conv(x, self.weight, self.bias, self.kind, self.k, self.halo)


class _InputFeatures(torch.autograd.Function):
    """``fv3hip_cyclegan_input`` forwards (the state, then sin / cos of the local time and x, y, z); a slice backwards."""

    @staticmethod
    def forward(ctx, state, lon, xyz, theta):
        S, n, c = int(state.shape[0]), int(state.shape[2]), int(state.shape[-1])
        state = state.contiguous()
        out = torch.empty((S, 6, n, n, c + 5), dtype=torch.float32, device=state.device)
        if S:
            _lib.call_on(state.device, "fv3hip_cyclegan_input", state.data_ptr(), c, 0, 0, None, lon.data_ptr(), xyz.data_ptr(),
                         theta.data_ptr(), out.data_ptr(), c + 5, 0, 0, S, n, c, ops._stream(state.device))
        ctx.channels = c
        return out

    @staticmethod
    def backward(ctx, d):
        return d[..., :ctx.channels].contiguous(), None, None, None


class HipGenerator(nn.Module):
    """``GeneratorTwin`` on the training kernels: the same layers in the same order, activations channel-last.
    ``forward(theta, state)``: ``theta`` ``[S]`` float32 radians (``theta_from_seconds``; ignored without geographic
    features), ``state`` ``[S, 6, n, n, C]``.  Bit for bit ``GeneratorModel.forward`` on the same parameters: the apply pass
    and that model's loader transform are the same float32 expression."""

    def __init__(self, spec: GeneratorSpec, convolution_type: str = "halo_conv2d"):
        super().__init__()
        spec.validate()
        self.meta, _ = spec.to_arrays()
        self.convolution_type = convolution_type
        self.convs = nn.ModuleDict()
        for name, kind, ci, co, k, _ in spec.plan:
            conv = CubeConv(ci, co, kind, k, convolution_type)
            conv.load_torch(spec.weights[name], spec.biases[name])
            self.convs[name.replace(".", "_")] = conv
        last = lambda a: nn.Parameter(torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).transpose(0, 2, 3, 1))))   # noqa: E731
        self.input_bias = last(spec.input_bias) if spec.use_geographic_bias else None
        self.output_bias = last(spec.output_bias) if spec.use_geographic_bias else None
        self.embedded_bias = last(spec.embedded_bias) if spec.use_geographic_embedded_bias else None
        self.n_convolutions, self.n_resnet = spec.n_convolutions, spec.n_resnet
        self.use_geographic_features = spec.use_geographic_features
        if self.use_geographic_features:
            self.register_buffer("lon", torch.from_numpy(np.ascontiguousarray(spec.lon, np.float32)), persistent=False)
            self.register_buffer("xyz", torch.from_numpy(np.ascontiguousarray(np.asarray(spec.xyz, np.float32).transpose(0, 2, 3, 1))),
                                 persistent=False)
        self._spec_fields = dict(channels=spec.channels, nx=spec.nx, n_convolutions=spec.n_convolutions, n_resnet=spec.n_resnet,
                                 kernel_size=spec.kernel_size, strided_kernel_size=spec.strided_kernel_size, max_filters=spec.max_filters)

    def forward(self, theta, state):
        x = state if self.input_bias is None else state + self.input_bias
        if self.use_geographic_features:
            x = _InputFeatures.apply(x, self.lon, self.xyz, theta.to(torch.float32).contiguous())
        x = instance_norm_act(self.convs["first"](x), self.embedded_bias, 0.0)
        for level in range(self.n_convolutions):
            x = instance_norm_act(self.convs[f"down{level}"](x), None, 0.0)
        for j in range(self.n_resnet):
            y = instance_norm_act(self.convs[f"res{j}_a"](x), None, 0.0)
            x = instance_norm_act(self.convs[f"res{j}_b"](y), None, 1.0) + x
        for level in reversed(range(self.n_convolutions)):
            x = instance_norm_act(self.convs[f"up{level}"](x), None, 0.0)
        x = self.convs["last"](x)
        return x if self.output_bias is None else x + self.output_bias

    def to_spec(self) -> GeneratorSpec:
        """The parameters as they stand, in torch's layout."""
        weights, biases = {}, {}
        for key, conv in self.convs.items():
            name = key.replace("_", ".")
            weights[name], biases[name] = conv.torch_arrays()
        first = lambda p: None if p is None else np.ascontiguousarray(p.detach().cpu().numpy().transpose(0, 3, 1, 2))   # noqa: E731
        lon = self.lon.cpu().numpy().copy() if self.use_geographic_features else None
        xyz = np.ascontiguousarray(self.xyz.cpu().numpy().transpose(0, 3, 1, 2)) if self.use_geographic_features else None
        return GeneratorSpec(weights=weights, biases=biases, input_bias=first(self.input_bias), output_bias=first(self.output_bias),
                             embedded_bias=first(self.embedded_bias), lon=lon, xyz=xyz, **self._spec_fields)


def check_weight_layout(kind: str, c_in: int, c_out: int, k: int):
    """The two layouts hold the same numbers: a round trip through both is the identity (used by the tests)."""
    w = np.arange(np.prod(weight_shape(kind, c_in, c_out, k)), dtype=np.float32).reshape(weight_shape(kind, c_in, c_out, k))
    return np.array_equal(torch_weight(kind, kernel_weight(kind, w)), w)
