"""What the device trainers (``train.DenseTrainer``, ``conv_train.ConvTrainer``, ``graph_train.GraphTrainer``) share: the flat
parameter store and its offsets, the capture of a step as a HIP graph, the upload idiom, the cut of the concatenated head layer,
the device side of an ``MseLoss`` and the batch-size check (DESIGN.md sections 21, 23 and 24).
"""
from typing import Dict, Hashable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops


def upload(array, device) -> torch.Tensor:
    """``array`` as a contiguous float32 tensor on ``device``."""
    return torch.from_numpy(np.ascontiguousarray(array, np.float32)).to(device)


class FlatParameters:
    """One flat float32 parameter buffer holding ``arrays`` (``(key, array)`` pairs) one after the other in their order, the
    gradient buffer and the two moment buffers of the same layout (zero) and the int64 step counter, all on ``device``."""

    def __init__(self, arrays: Sequence[Tuple[Hashable, np.ndarray]], device):
        self.layout: Dict[Hashable, Tuple[int, Tuple[int, ...]]] = {}   # key -> (offset, shape)
        off = 0
        for key, a in arrays:
            if key in self.layout:
                raise ValueError(f"parameter {key!r} is given twice")
            self.layout[key] = (off, tuple(int(v) for v in np.shape(a)))
            off += int(np.prod(np.shape(a), dtype=np.int64))
        self.size = off
        self.params = torch.from_numpy(np.concatenate([np.asarray(a, np.float32).reshape(-1) for _, a in arrays])).to(device)
        self.grads, self.m, self.v = (torch.zeros_like(self.params) for _ in range(3))
        self.step_count = torch.zeros(1, dtype=torch.int64, device=device)

    def views(self, buffer: torch.Tensor) -> Dict[Hashable, torch.Tensor]:
        """key -> the key's part of ``buffer`` (one of the four flat buffers) in its shape; a view, not a copy."""
        return {key: buffer[off:off + int(np.prod(shape, dtype=np.int64))].view(shape) for key, (off, shape) in self.layout.items()}

    def to_host(self, buffer: torch.Tensor) -> Dict[Hashable, np.ndarray]:
        """key -> a numpy copy of the key's part of ``buffer``, in the order of construction: one read-back."""
        host = buffer.cpu().numpy()
        return {key: host[off:off + int(np.prod(shape, dtype=np.int64))].reshape(shape).copy() for key, (off, shape) in self.layout.items()}

    def adam(self, lr: float, betas: Tuple[float, float], eps: float) -> None:
        ops.train_adam(self.params, self.grads, self.m, self.v, self.step_count, lr, betas[0], betas[1], eps)

    def adamw(self, lr: float, betas: Tuple[float, float], eps: float, weight_decay: float) -> None:
        ops.train_adamw(self.params, self.grads, self.m, self.v, self.step_count, lr, betas[0], betas[1], eps, weight_decay)


def capture_step(trainer, idx: torch.Tensor) -> "torch.cuda.CUDAGraph":
    """A HIP graph of ``trainer.step(idx)`` reading the row numbers from ``idx``'s memory: refill ``idx`` in place and
    ``replay()``.  One eager step is taken first (on a side stream, as torch asks) so that nothing is initialised under capture;
    it counts as a step."""
    side = torch.cuda.Stream(trainer.device)
    side.wait_stream(torch.cuda.current_stream(trainer.device))
    with torch.cuda.stream(side):
        trainer.step(idx)
    torch.cuda.current_stream(trainer.device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        trainer.step(idx)
    return graph


def check_batch(n: int, max_batch: int, what: str = "rows") -> int:
    """``n`` if a batch of ``n`` fits buffers made for ``max_batch``."""
    if not 1 <= n <= max_batch:
        raise ValueError(f"a batch of {n} {what} does not fit the buffers of {max_batch}")
    return n


def split_heads(kernels: List[np.ndarray], biases: List[np.ndarray], f_out: int, head_sizes: Optional[Sequence[int]]):
    """``(hidden_kernels, hidden_biases, output_kernels, output_biases)``: the last layer, the concatenated heads
    ``[..., f_out]``, cut along its columns into ``head_sizes`` (None: one head)."""
    if head_sizes is None:
        head_sizes = [f_out]
    if sum(head_sizes) != f_out:
        raise ValueError(f"head sizes {list(head_sizes)} do not add up to {f_out} output features")
    cuts = np.cumsum([0] + list(head_sizes))
    out_k = [kernels[-1][:, a:b].copy() for a, b in zip(cuts[:-1], cuts[1:])]
    out_b = [biases[-1][a:b].copy() for a, b in zip(cuts[:-1], cuts[1:])]
    return kernels[:-1], biases[:-1], out_k, out_b


class DeviceMseLoss:
    """The per-feature arrays of a ``train.MseLoss`` on the device and its ``wnorm`` per batch size, uploaded when a size is
    first seen (the eager step before a capture sees it)."""

    def __init__(self, loss, device):
        self.loss, self.device = loss, device
        self.arrays = tuple(upload(getattr(loss, name), device) for name in ("scale", "center", "inv_cstd2", "lo", "hi", "keep"))
        self._wnorm: Dict[int, torch.Tensor] = {}

    def grad(self, yhat: torch.Tensor, targets: torch.Tensor, dy: torch.Tensor, loss: torch.Tensor, loss_workspace: torch.Tensor,
             idx: torch.Tensor) -> None:
        """``ops.train_mse_grad`` on the ``yhat.shape[0]`` rows ``idx`` of ``targets``."""
        n = int(yhat.shape[0])
        wn = self._wnorm.get(n)
        if wn is None:
            wn = self._wnorm[n] = torch.from_numpy(self.loss.wnorm(n)).to(self.device)
        ops.train_mse_grad(yhat, *self.arrays, wn, targets, dy, loss, loss_workspace, idx=idx)
