"""What the networks on the six faces of the cubed sphere share on the host: the channel slice of a device buffer, the shape
check of a cube, the device of a model, and the scalers that pack state variables into the normalised state and back
(``fv3hip_graph_pack`` / ``fv3hip_graph_unpack``).  Used by graph.py, cyclegan.py and fmr.py."""
import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .ops import _require_device, _stream


class _Slice:
    """A channel slice of a channel-last device buffer ``[S][6][n][n][ld]`` (``stride``: elements between samples)."""

    def __init__(self, tensor: torch.Tensor, ld: int, off: int = 0, stride: int = 0):
        self.tensor, self.ptr, self.ld, self.off, self.stride = tensor, tensor.data_ptr(), int(ld), int(off), int(stride)


def check_cube_shape(shape: Sequence[int], what: str = "state"):
    """``[..., tile, x, y, feature]``: six square tiles."""
    if len(shape) < 4:
        raise ValueError(f"{what} must be [..., tile, x, y, feature], got shape {tuple(shape)}")
    if shape[-4] != 6:
        raise ValueError(f"{what} must hold the six tiles of the cube, got {shape[-4]} tiles")
    if shape[-3] != shape[-2]:
        raise ValueError(f"cube tiles are square, got {shape[-3]} x {shape[-2]}")


def cuda_device(device, who: str) -> torch.device:
    """``device`` as a 'cuda' device with its index; ``who``: the class that asks."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who} needs a 'cuda' (ROCm) device; there is no CPU fallback")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class StatePacker:
    """The ``StandardScaler`` of every state variable on one device: ``variables`` ``(name, feature count)`` in the network's
    channel order, ``mean`` and ``std`` float64 ``[F]`` over all of them."""

    def __init__(self, variables: Sequence[Tuple[str, int]], mean: np.ndarray, std: np.ndarray, device: torch.device):
        self.variables = [(str(name), int(nfeat)) for name, nfeat in variables]
        self.n_features = sum(nfeat for _, nfeat in self.variables)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(device)
        self._mean, self._std = up(mean), up(std)
        self._nfeat = (ctypes.c_int * len(self.variables))(*[nfeat for _, nfeat in self.variables])

    def pack(self, sources: Sequence[torch.Tensor], n_windows: Optional[int], n_times: int, step: int) -> torch.Tensor:
        """``sources[v]``: a ``[time, tile, x, y, level]`` view (any strides, float32 or float64) of state variable v ->
        float32 ``[n_windows, n_times, 6, n, n, F]``, ``(x - mean) / std`` in float64, window w from times ``w * step ...``
        (``n_windows`` ``None``: as many as there are times)."""
        if len(sources) != len(self.variables):
            raise ValueError(f"{len(self.variables)} sources are needed, got {len(sources)}")
        dev = _require_device(*sources)
        for (name, nfeat), t in zip(self.variables, sources):
            if t.dim() != 5 or t.shape[-1] != nfeat:
                raise ValueError(f"variable {name!r} must be [time, tile, x, y, {nfeat}], got shape {tuple(t.shape)}")
            check_cube_shape(t.shape[:-1] + (0,), f"variable {name!r}")
            if tuple(t.shape[:4]) != tuple(sources[0].shape[:4]):
                raise ValueError("the state variables differ in their time, tile, x or y extent")
            if t.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"variable {name!r} must be float32 or float64, got {t.dtype}")
        T, n, k = int(sources[0].shape[0]), int(sources[0].shape[2]), len(sources)
        if n_windows is None:
            n_windows = T
        if step < 1 or n_windows < 0 or n_windows * step + n_times - step > T:   # the last window ends at its n_times
            raise ValueError(f"{n_windows} windows of {step} steps do not fit {T} times")
        state = torch.empty((n_windows, n_times, 6, n, n, self.n_features), dtype=torch.float32, device=dev)
        _lib.call_on(dev, "fv3hip_graph_pack", (ctypes.c_void_p * k)(*[t.data_ptr() for t in sources]),
                     (ctypes.c_int * k)(*[_lib.F64 if t.dtype == torch.float64 else _lib.F32 for t in sources]),
                     (ctypes.c_int64 * (5 * k))(*[s for t in sources for s in t.stride()]), k, self._nfeat, self._mean.data_ptr(),
                     self._std.data_ptr(), n_windows, n_times, step, n, state.data_ptr(), _stream(dev))
        return state

    def unpack(self, state: torch.Tensor) -> List[torch.Tensor]:
        """Normalised float32 ``[..., 6, n, n, F]`` -> per variable float64 ``[..., 6, n, n, nfeat]``, ``float64(x) * std + mean``."""
        check_cube_shape(state.shape)
        if state.dtype != torch.float32 or state.shape[-1] != self.n_features:
            raise ValueError(f"the state must be float32 with {self.n_features} features")
        dev = _require_device(state)
        state = state.contiguous()
        lead, n = tuple(state.shape[:-1]), int(state.shape[-2])
        outs = [torch.empty(lead + (nfeat,), dtype=torch.float64, device=dev) for _, nfeat in self.variables]
        rows = int(np.prod(lead[:-3])) if lead[:-3] else 1
        _lib.call_on(dev, "fv3hip_graph_unpack", state.data_ptr(), rows, n, len(outs), self._nfeat, self._mean.data_ptr(),
                     self._std.data_ptr(), (ctypes.c_void_p * len(outs))(*[t.data_ptr() for t in outs]), _stream(dev))
        return outs
