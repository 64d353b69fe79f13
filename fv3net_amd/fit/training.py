"""What the ``train_*`` functions share: the choice of backend and device, the minibatch sequence that both backends of a model
see, the weights of torch ``Linear`` layers in the Keras layout and the strict reading of a configuration mapping.
"""
import dataclasses
from typing import Dict, Iterator, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch


def check_backend(backend: Optional[str], allow: Sequence[str] = ("torch", "hip")) -> str:
    """``backend`` if it is one of ``allow``; ``None`` is ``"torch"``."""
    if backend is not None and backend not in allow:
        raise ValueError(f"backend must be None, {' or '.join(repr(a) for a in allow)}, got {backend!r}")
    return backend or "torch"


def resolve_backend(backend: Optional[str], device, allow: Sequence[str] = ("torch", "hip")) -> Tuple[str, torch.device]:
    """``(backend, device)`` of a training function: ``check_backend``; ``device=None`` is ``"cuda"`` where there is one, else
    ``"cpu"``; ``"hip"`` anywhere but on a GPU is refused, since the kernels have no CPU path."""
    backend = check_backend(backend, allow)
    dev = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
    if backend == "hip" and dev.type != "cuda":
        from .. import ops

        ops._require_device(torch.empty(0, device=dev))   # raises
    return backend, dev


def epoch_minibatches(n: int, batch_size: int, epochs: int, seed: int, device) -> Iterator[List[torch.Tensor]]:
    """Per epoch the list of its minibatches: one ``torch.randperm(n)`` from a generator seeded once with ``seed``, moved to
    ``device`` and cut into ``batch_size`` rows.  Both backends of a model draw from this, so they see the same rows in the same
    order."""
    g = torch.Generator().manual_seed(seed)
    for _ in range(epochs):
        perm = torch.randperm(n, generator=g).to(device)
        yield [perm[i:i + batch_size] for i in range(0, n, batch_size)]


def linear_arrays(layers: Sequence[torch.nn.Linear]) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """``(kernels, biases)`` of torch ``Linear`` layers as fresh numpy arrays, the kernels in the Keras layout ``[in][out]``."""
    return ([m.weight.detach().cpu().numpy().T.copy() for m in layers], [m.bias.detach().cpu().numpy().copy() for m in layers])


def strict_fields(cls, d: Optional[Mapping], what: str) -> Dict:
    """``d`` as the keyword arguments of the dataclass ``cls``; a key that is none of its fields is refused."""
    d = dict(d or {})
    unknown = set(d) - {f.name for f in dataclasses.fields(cls)}
    if unknown:
        raise ValueError(f"{what} has no fields {sorted(unknown)}")
    return d
