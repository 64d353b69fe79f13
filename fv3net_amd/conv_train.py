"""Training state of the convolutional network on the device (csrc/conv_train.hip).

``ConvTrainer`` mirrors ``train.DenseTrainer``: it owns every tensor the stateless ``fv3hip_train_conv_*`` and
``fv3hip_train_*`` entry points work on -- one flat float32 parameter buffer (per hidden layer the kernel ``[k][k][c_in][f]``,
Keras layout, followed by its bias; then the heads as one concatenated ``[filters][sum F_out]`` layer and its bias), the
gradient and Adam moment buffers of the same layout, the device-resident step counter, the activation buffers of the largest
batch, the chunk workspaces of the weight gradients, the resident normalised, halo-padded inputs
``[samples, nx + 2 h, ny + 2 h, C]`` and the targets ``[samples * nx * ny, sum F_out]``.  PyTorch supplies memory and the stream
only.
"""
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .train import MseLoss
from .train_state import DeviceMseLoss, FlatParameters, capture_step, check_batch, split_heads, upload


class ConvTrainer:
    """``hidden_kernels[l]`` is ``[k, k, c_in, f]``, each followed by ReLU (``relu=False``: by nothing); ``out_kernel`` is the
    1 x 1 heads ``[filters, sum F_out]``.  A batch is a set of tile-samples (rows of ``xin``)."""

    def __init__(self, hidden_kernels: Sequence[np.ndarray], hidden_biases: Sequence[np.ndarray], out_kernel: np.ndarray,
                 out_bias: np.ndarray, xin: np.ndarray, targets: np.ndarray, loss: MseLoss, device="cuda", max_batch: int = 1,
                 learning_rate: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, relu: bool = True,
                 transpose_invariant: bool = True):
        self.device = dev = torch.device(device)
        ops._require_device(torch.empty(1, device=dev))
        if len(hidden_kernels) != len(hidden_biases) or not hidden_kernels:
            raise ValueError("one bias per hidden kernel, at least one hidden layer")
        self.conv_shapes = [tuple(int(v) for v in np.shape(w)) for w in hidden_kernels]
        k = self.conv_shapes[0][0]
        c_in = int(np.shape(xin)[3])
        for (a, b, c, f), bias in zip(self.conv_shapes, hidden_biases):
            if (a, b, c) != (k, k, c_in) or tuple(np.shape(bias)) != (f,):
                raise ValueError("layer shapes do not chain")
            c_in = f
        self.k, self.filters = k, c_in
        self.head_shape = tuple(int(v) for v in np.shape(out_kernel))
        if len(self.head_shape) != 2 or self.head_shape[0] != c_in or tuple(np.shape(out_bias)) != (self.head_shape[1],):
            raise ValueError("the heads must be [filters, F_out] with a bias [F_out]")
        self.f_out = self.head_shape[1]
        self.relu, self.transpose_invariant = bool(relu), bool(transpose_invariant)
        self.lr, self.betas, self.eps = float(learning_rate), (float(betas[0]), float(betas[1])), float(eps)
        self.max_batch = int(max_batch)

        n_hidden = len(self.conv_shapes)
        self.n_samples, X, Y, _ = (int(v) for v in np.shape(xin))
        self.extents = [(X - l * (k - 1), Y - l * (k - 1)) for l in range(n_hidden + 1)]   # of the input and of every hidden layer
        self.nx, self.ny = self.extents[-1]
        if self.nx < 1 or self.ny < 1:
            raise ValueError(f"inputs of {X} x {Y} cells do not hold the halo of {n_hidden} layers of {k} x {k} kernels")
        self.n_pix = self.nx * self.ny
        if tuple(np.shape(targets)) != (self.n_samples * self.n_pix, self.f_out):
            raise ValueError(f"targets are {np.shape(targets)}, expected {(self.n_samples * self.n_pix, self.f_out)}")

        layers = list(zip(list(hidden_kernels) + [out_kernel], list(hidden_biases) + [out_bias]))
        pairs = [pair for l, (w, b) in enumerate(layers) for pair in ((("w", l), w), (("b", l), b))]   # kernel, then its bias
        flat = self._flat = FlatParameters(pairs, dev)
        self.params, self.grads, self.m, self.v, self.step_count = flat.params, flat.grads, flat.m, flat.v, flat.step_count
        p, g = flat.views(flat.params), flat.views(flat.grads)
        self.w, self.b = [p["w", l] for l in range(len(layers))], [p["b", l] for l in range(len(layers))]
        self.dw, self.db = [g["w", l] for l in range(len(layers))], [g["b", l] for l in range(len(layers))]

        B = self.max_batch
        self._h = [torch.zeros((B, ex, ey, s[3]), dtype=torch.float32, device=dev)
                   for (ex, ey), s in zip(self.extents[1:], self.conv_shapes)]
        self._dh = [torch.zeros_like(h) for h in self._h]
        self._y = torch.zeros((B * self.n_pix, self.f_out), dtype=torch.float32, device=dev)
        self._dy = torch.zeros_like(self._y)
        ws = max([ops.train_conv_backward_weight_workspace_floats(B, ex, ey, s[0], s[2], s[3])
                  for (ex, ey), s in zip(self.extents[:-1], self.conv_shapes)] +
                 [ops.train_backward_weight_workspace_floats(B * self.n_pix, self.filters, self.f_out)])
        self._ws = torch.zeros(ws, dtype=torch.float32, device=dev) if ws else None
        self._loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self._loss_ws = torch.zeros(ops.train_loss_workspace_doubles(), dtype=torch.float64, device=dev)
        # the batch's rows of the targets: idx[s] * n_pix + p
        self._pix = torch.arange(self.n_pix, dtype=torch.int64, device=dev).unsqueeze(0)
        self._first = torch.zeros(B, dtype=torch.int64, device=dev)
        self._rows = torch.zeros(B * self.n_pix, dtype=torch.int64, device=dev)

        self.xin, self.targets = upload(xin, dev), upload(targets, dev)
        self._mse = DeviceMseLoss(loss, dev)

    # -- one optimiser step ------------------------------------------------------------------
    def step(self, idx: torch.Tensor) -> None:
        """One Adam step on the tile-samples ``idx`` (int64, on the device), then the kernel constraint on every hidden kernel
        (Keras applies a ``kernel_constraint`` after the update); the loss stays on the device."""
        self.backward(idx)
        self._flat.adam(self.lr, self.betas, self.eps)
        if self.transpose_invariant and self.k > 1:   # (on a 1 x 1 kernel, the heads included, it is the identity)
            for w in self.w[:-1]:
                ops.train_conv_constrain(w)

    def backward(self, idx: torch.Tensor) -> None:
        """Forward, loss and the gradient of every parameter for the tile-samples ``idx``, into ``self.grads``."""
        n = check_batch(int(idx.shape[0]), self.max_batch, "tile-samples")
        rows_n = n * self.n_pix
        n_hidden = len(self.conv_shapes)
        a, table = self.xin, idx
        for l in range(n_hidden):
            ops.train_conv_forward(a, self.w[l], self.b[l], self._h[l][:n], idx=table, relu=self.relu)
            a, table = self._h[l][:n], None
        last = self._h[-1][:n].view(rows_n, self.filters)
        dlast = self._dh[-1][:n].view(rows_n, self.filters)
        y, dy = self._y[:rows_n], self._dy[:rows_n]
        ops.train_linear_forward(last, self.w[-1], self.b[-1], y)
        torch.mul(idx, self.n_pix, out=self._first[:n])
        rows = self._rows[:rows_n]
        torch.add(self._first[:n].unsqueeze(1), self._pix, out=rows.view(n, self.n_pix))
        self._mse.grad(y, self.targets, dy, self._loss, self._loss_ws, rows)
        ops.train_linear_backward_weight(last, dy, self.dw[-1], self.db[-1], workspace=self._ws)
        ops.train_linear_backward_data(dy, self.w[-1], last if self.relu else None, dlast)
        for l in range(n_hidden - 1, -1, -1):
            if l == 0:
                ops.train_conv_backward_weight(self.xin, self._dh[0][:n], self.dw[0], self.db[0], idx=idx, workspace=self._ws)
            else:
                ops.train_conv_backward_weight(self._h[l - 1][:n], self._dh[l][:n], self.dw[l], self.db[l], workspace=self._ws)
                ops.train_conv_backward_data(self._dh[l][:n], self.w[l], self._h[l - 1][:n] if self.relu else None, self._dh[l - 1][:n])

    def capture(self, idx: torch.Tensor) -> "torch.cuda.CUDAGraph":
        """``train_state.capture_step``: a HIP graph of ``step(idx)``, after one eager step that counts as a step."""
        return capture_step(self, idx)

    def loss(self) -> float:
        """The loss of the last step's batch (before its update), read back."""
        return float(self._loss.cpu()[0])

    # -- reading the state back ----------------------------------------------------------------
    def _host(self, buffer: torch.Tensor, head_sizes: Optional[Sequence[int]]):
        host = self._flat.to_host(buffer)
        layers = range(len(self.w))
        return split_heads([host["w", l] for l in layers], [host["b", l] for l in layers], self.f_out, head_sizes)

    def parameters(self, head_sizes: Optional[Sequence[int]] = None):
        """``(hidden_kernels, hidden_biases, output_kernels, output_biases)`` as numpy arrays, the order
        ``fit.conv_spec_from_arrays`` takes them in; the concatenated head layer is cut into ``head_sizes``."""
        return self._host(self.params, head_sizes)

    def gradients(self, head_sizes: Optional[Sequence[int]] = None):
        """The gradient buffer in the layout of ``parameters``."""
        return self._host(self.grads, head_sizes)
