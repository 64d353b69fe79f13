"""Training state of the graph U-Net on the device (csrc/graph_train.hip).

``GraphTrainer`` mirrors ``conv_train.ConvTrainer``: it owns every tensor the stateless ``fv3hip_graph_*`` and ``fv3hip_train_*``
entry points work on -- one flat float32 parameter buffer (per layer of ``layer_plan``, in its order, ``w_self``, ``w_neigh``,
``bias`` or ``weight``, ``bias``: the layout of ``GraphUNetSpec``), the gradient and moment buffers of the same layout, the
device-resident step counter, every activation buffer of every rollout step for the largest batch (the levels' cat buffers
included: the transposed convolution writes their second half), one set of gradient buffers, the chunk workspace of the weight
gradients, the staged batch and the resident normalised samples ``[sample, time, 6, n, n, F]``.  PyTorch supplies memory, the
stream and the gather of the batch's samples into the staging buffer (``fv3hip_graph_sage`` addresses its samples by a stride,
not by an index); everything else of a step is a launch of this project's kernels on one stream, one after the other.
"""
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from .cube import _Slice
from .graph import ACTIVATIONS, GraphUNetSpec, SageLayer, UpLayer
from .train_state import FlatParameters, capture_step, check_batch

_FIELDS = {"sage": ("w_self", "w_neigh", "bias"), "up": ("weight", "bias")}


class GraphTrainer:
    """``spec``: the initial network (and the scalers, which training leaves alone); ``samples``: the normalised training set
    ``[sample, time, 6, n, n, F]`` with at least ``multistep + 1`` times.  The loss is the mean over the rollout steps of the
    MSE against the sample's later times (training_loop.py:136-148)."""

    def __init__(self, spec: GraphUNetSpec, samples, multistep: int = 1, max_batch: int = 1, device="cuda",
                 optimizer: str = "AdamW", lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: Optional[float] = None):
        self.device = dev = torch.device(device)
        ops._require_device(torch.empty(1, device=dev))
        if optimizer not in ("AdamW", "Adam"):
            raise NotImplementedError(f"optimizer {optimizer!r} is not built; supported: 'AdamW', 'Adam'")
        self.optimizer = optimizer
        self.weight_decay = float((1e-2 if optimizer == "AdamW" else 0.0) if weight_decay is None else weight_decay)
        if optimizer == "Adam" and self.weight_decay != 0.0:
            raise NotImplementedError("Adam with weight_decay (an L2 term in the gradient) is not built; use 'AdamW'")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        spec.validate()
        self._spec = spec
        self.depth, self.m, self.F = int(spec.depth), int(spec.min_filters), int(spec.n_features)
        self._act_code = ACTIVATIONS[spec.activation]
        self.K, self.B = int(multistep), int(max_batch)
        samples = torch.as_tensor(samples)
        if samples.dim() != 6 or samples.shape[2] != 6 or samples.shape[3] != samples.shape[4] or samples.shape[5] != self.F:
            raise ValueError(f"samples must be [sample, time, 6, n, n, {self.F}], got {tuple(samples.shape)}")
        if self.K < 1 or samples.shape[1] < self.K + 1:
            raise ValueError(f"samples of {samples.shape[1]} times do not hold {self.K} steps")
        if self.B < 1 or self.B * 6 > 65535:
            raise ValueError(f"max_batch must be in [1, 10922], got {self.B}")
        self.n = n = int(samples.shape[3])
        spec.check_grid(n)
        self.samples = samples.to(device=dev, dtype=torch.float32).contiguous()
        self.T = int(self.samples.shape[1])
        self.cells = 6 * n * n
        if self.B * self.cells > 1 << 24:
            raise ValueError(f"a batch of {self.B} cubes of {n} x {n} cells exceeds the loss kernel's 2^24 rows")

        # parameters, gradients, moments: one flat buffer each, per-layer views in the order of layer_plan
        self.plan = spec.plan
        self._fields = {name: _FIELDS[kind] for name, kind, *_ in self.plan}
        flat = self._flat = FlatParameters([((name, f), getattr(spec.layers[name], f)) for name, fields in self._fields.items() for f in fields],
                                           dev)
        self.params, self.grads, self.mom, self.var, self.step_count = flat.params, flat.grads, flat.m, flat.v, flat.step_count
        p, g = flat.views(flat.params), flat.views(flat.grads)
        self.w: Dict[str, Dict[str, torch.Tensor]] = {name: {f: p[name, f] for f in fields} for name, fields in self._fields.items()}
        self.dw: Dict[str, Dict[str, torch.Tensor]] = {name: {f: g[name, f] for f in fields} for name, fields in self._fields.items()}

        # activations of every rollout step and one set of gradients, named alike
        B, m, F = self.B, self.m, self.F
        shapes = {"x0": (n, m), "y": (n, F)}
        ws = [ops.graph_sage_backward_weight_workspace_floats(B, n, F, m), ops.graph_sage_backward_weight_workspace_floats(B, n, 2 * m, F)]
        for k in range(self.depth + 1):
            c, nk = m * 2 ** k, n >> k
            if k < self.depth:
                shapes.update({f"t1.{k}": (nk, 2 * c), f"cat.{k}": (nk, 4 * c), f"pool.{k}": (nk // 2, 2 * c), f"t2.{k}": (nk, 2 * c),
                               f"low.{k}": (nk, 2 * c)})
                ws += [ops.graph_sage_backward_weight_workspace_floats(B, nk, 4 * c, 2 * c),
                       ops.graph_up2_backward_weight_workspace_floats(B, nk // 2, 4 * c, 2 * c)]
            else:
                shapes.update({"t.b": (nk, 2 * c), "low.b": (nk, 2 * c)})
                ws.append(ops.graph_sage_backward_weight_workspace_floats(B, nk, 2 * c, 2 * c))
        new = lambda: {key: _Slice(torch.zeros((B, 6, e, e, c), dtype=torch.float32, device=dev), c) for key, (e, c) in shapes.items()}
        self._act = [new() for _ in range(self.K)]
        self._d = new()
        self._ws = torch.zeros(max(max(ws), 1), dtype=torch.float32, device=dev)
        self._batch = torch.zeros((B, self.T) + tuple(self.samples.shape[2:]), dtype=torch.float32, device=dev)

        # the loss: rows = cells, scale 1, center 0, no limits, every feature kept; the targets of step k are the staged batch's
        # time k + 1, found through a row table that depends on k only
        one, zero = torch.ones(F, device=dev), torch.zeros(F, device=dev)
        self._loss_vecs = (one, zero, one, torch.full((F,), -np.inf, device=dev), torch.full((F,), np.inf, device=dev), one)
        self._wnorm: Dict[int, torch.Tensor] = {}
        cell = torch.arange(self.cells, dtype=torch.int64, device=dev).unsqueeze(0)
        first = torch.arange(B, dtype=torch.int64, device=dev).unsqueeze(1) * self.T
        self._rows = [((first + (k + 1)) * self.cells + cell).reshape(-1) for k in range(self.K)]
        self._loss = torch.zeros(self.K, dtype=torch.float64, device=dev)
        self._loss_ws = torch.zeros(ops.train_loss_workspace_doubles(), dtype=torch.float64, device=dev)

    # -- layers ----------------------------------------------------------------------------------
    def _sage(self, name, src: _Slice, dst: _Slice, dst_off, S, n, c_in, c_out, act):
        w = self.w[name]
        _lib.call_on(self.device, "fv3hip_graph_sage", src.ptr, src.ld, src.off, src.stride, w["w_self"].data_ptr(),
                     w["w_neigh"].data_ptr(), w["bias"].data_ptr(), dst.ptr, dst.ld, dst_off, dst.stride, S, n, c_in, c_out, act,
                     ops._stream(self.device))

    def _state_in(self, k: int) -> _Slice:
        """What step k reads: the staged batch's time 0, then the step before's output."""
        if k:
            return self._act[k - 1]["y"]
        return _Slice(self._batch[:, 0], self.F, 0, self.T * self.cells * self.F)

    def _forward(self, k: int, S: int) -> None:
        A, act, st, dev = self._act[k], self._act_code, ops._stream(self.device), self.device
        n, m, F = self.n, self.m, self.F
        self._sage("first", self._state_in(k), A["x0"], 0, S, n, F, m, act)
        x = A["x0"]
        for lev in range(self.depth):
            c, nk = m * 2 ** lev, n >> lev
            self._sage(f"L{lev}.conv1a", x, A[f"t1.{lev}"], 0, S, nk, c, 2 * c, act)
            self._sage(f"L{lev}.conv1b", A[f"t1.{lev}"], A[f"cat.{lev}"], 0, S, nk, 2 * c, 2 * c, act)
            x = A[f"pool.{lev}"]
            _lib.call_on(dev, "fv3hip_graph_pool2", A[f"cat.{lev}"].ptr, 4 * c, 0, x.ptr, x.ld, 0, S, nk, 2 * c, st)
        c, nk = m * 2 ** self.depth, n >> self.depth
        self._sage("bottom.a", x, A["t.b"], 0, S, nk, c, 2 * c, act)
        self._sage("bottom.b", A["t.b"], A["low.b"], 0, S, nk, 2 * c, 2 * c, act)
        low = A["low.b"]
        for lev in reversed(range(self.depth)):
            c, nk = m * 2 ** lev, n >> lev
            cat, w = A[f"cat.{lev}"], self.w[f"L{lev}.up"]
            _lib.call_on(dev, "fv3hip_graph_up2", low.ptr, low.ld, 0, w["weight"].data_ptr(), w["bias"].data_ptr(), cat.ptr, cat.ld,
                         2 * c, S, nk // 2, 4 * c, 2 * c, st)
            self._sage(f"L{lev}.conv2a", cat, A[f"t2.{lev}"], 0, S, nk, 4 * c, 2 * c, act)
            self._sage(f"L{lev}.conv2b", A[f"t2.{lev}"], A[f"low.{lev}"], 0, S, nk, 2 * c, 2 * c, act)
            low = A[f"low.{lev}"]
        self._sage("last", low, A["y"], 0, S, n, 2 * m, F, _lib.ACT_LINEAR)

    def _sage_backward(self, name, x: _Slice, g: _Slice, p: Optional[_Slice], dst: Optional[_Slice], S, n, c_in, c_out, more: bool):
        """The weight gradients of layer ``name`` (input ``x``, masked output gradient ``g``; ``more``: added to those of the
        later rollout steps) and, with ``dst``, its data gradient masked by act' of ``p``."""
        w, dw = self.w[name], self.dw[name]
        ops.graph_sage_backward_weight(x, g, dw["w_self"], dw["w_neigh"], dw["bias"], S, n, c_in, c_out, workspace=self._ws,
                                       accumulate=more)
        if dst is not None:
            ops.graph_sage_backward_data(g, w["w_self"], w["w_neigh"], p, self._act_code, dst, S, n, c_in, c_out)

    def _backward_step(self, k: int, S: int) -> None:
        A, D, act = self._act[k], self._d, self._act_code
        n, m, F, K = self.n, self.m, self.F, self.K
        more = k < K - 1
        rows = S * self.cells
        wn = self._wnorm.get(S)
        if wn is None:
            wn = self._wnorm[S] = torch.full((F,), 1.0 / (rows * F * K), dtype=torch.float32, device=self.device)
        scale, center, inv, lo, hi, keep = self._loss_vecs
        ops.train_mse_grad(A["y"].tensor.view(-1, F)[:rows], scale, center, inv, lo, hi, keep, wn, self._batch.view(-1, F),
                           D["y"].tensor.view(-1, F)[:rows], self._loss[k:k + 1], self._loss_ws, idx=self._rows[k][:rows])
        if more:   # step k + 1's gradient into the state (D["x0"] still holds its masked gradient of `first`), added to the loss's
            w = self.w["first"]
            ops.graph_sage_backward_data(D["x0"], w["w_self"], w["w_neigh"], None, _lib.ACT_LINEAR, D["y"], S, n, F, m, accumulate=True)
        low = f"low.{0}" if self.depth else "low.b"
        self._sage_backward("last", A[low], D["y"], A[low], D[low], S, n, 2 * m, F, more)
        for lev in range(self.depth):
            c, nk = m * 2 ** lev, n >> lev
            t2, cat, below = f"t2.{lev}", f"cat.{lev}", (f"low.{lev + 1}" if lev + 1 < self.depth else "low.b")
            self._sage_backward(f"L{lev}.conv2b", A[t2], D[f"low.{lev}"], A[t2], D[t2], S, nk, 2 * c, 2 * c, more)
            self._sage_backward(f"L{lev}.conv2a", A[cat], D[t2], None, D[cat], S, nk, 4 * c, 2 * c, more)   # raw: masked with the pool's part
            dup = _Slice(D[cat].tensor, 4 * c, 2 * c)
            dwu = self.dw[f"L{lev}.up"]
            ops.graph_up2_backward_weight(A[below], dup, dwu["weight"], dwu["bias"], S, nk // 2, 4 * c, 2 * c, self._ws, accumulate=more)
            ops.graph_up2_backward_data(dup, self.w[f"L{lev}.up"]["weight"], A[below], act, D[below], S, nk // 2, 4 * c, 2 * c)
        c, nk = m * 2 ** self.depth, n >> self.depth
        x = f"pool.{self.depth - 1}" if self.depth else "x0"
        self._sage_backward("bottom.b", A["t.b"], D["low.b"], A["t.b"], D["t.b"], S, nk, 2 * c, 2 * c, more)
        self._sage_backward("bottom.a", A[x], D["t.b"], None if self.depth else A[x], D[x], S, nk, c, 2 * c, more)
        for lev in reversed(range(self.depth)):
            c, nk = m * 2 ** lev, n >> lev
            t1, cat = f"t1.{lev}", f"cat.{lev}"
            before, dbefore = _Slice(A[cat].tensor, 4 * c, 0), _Slice(D[cat].tensor, 4 * c, 0)
            ops.graph_pool2_backward(D[f"pool.{lev}"], before, act, dbefore, S, nk, 2 * c)
            x = f"pool.{lev - 1}" if lev else "x0"
            self._sage_backward(f"L{lev}.conv1b", A[t1], dbefore, A[t1], D[t1], S, nk, 2 * c, 2 * c, more)
            self._sage_backward(f"L{lev}.conv1a", A[x], D[t1], None if lev else A[x], D[x], S, nk, c, 2 * c, more)
        self._sage_backward("first", self._state_in(k), D["x0"], None, None, S, n, F, m, more)   # (its data gradient: at step k - 1)

    # -- one optimiser step ------------------------------------------------------------------------
    def _check(self, idx: torch.Tensor) -> int:
        ops._require_device(idx)
        if idx.dtype != torch.int64 or idx.dim() != 1:
            raise TypeError("idx must be a 1-D int64 tensor of sample numbers")
        return check_batch(int(idx.shape[0]), self.B, "samples")

    def backward(self, idx: torch.Tensor) -> None:
        """The rollout from the samples ``idx`` (int64, on the device), the loss of every step and the gradient of every
        parameter, into ``self.grads``."""
        S = self._check(idx)
        torch.index_select(self.samples, 0, idx, out=self._batch[:S])
        for k in range(self.K):
            self._forward(k, S)
        for k in reversed(range(self.K)):
            self._backward_step(k, S)

    def step(self, idx: torch.Tensor) -> None:
        """One optimiser step on the samples ``idx``; the loss stays on the device."""
        self.backward(idx)
        if self.optimizer == "AdamW":
            self._flat.adamw(self.lr, self.betas, self.eps, self.weight_decay)
        else:
            self._flat.adam(self.lr, self.betas, self.eps)

    def capture(self, idx: torch.Tensor) -> "torch.cuda.CUDAGraph":
        """``train_state.capture_step``: a HIP graph of ``step(idx)``, after one eager step that counts as a step."""
        return capture_step(self, idx)

    def loss(self) -> float:
        """The loss of the last step's batch (before its update), read back: the rollout steps' parts added in order."""
        return float(self._loss.cpu().numpy().sum())

    def validation_loss(self, samples) -> float:
        """The loss of ``samples`` ``[sample, time, 6, n, n, F]`` (normalised) under the current parameters, as one batch would
        give it: forwards and the loss kernel only, in batches of ``max_batch``."""
        samples = torch.as_tensor(samples).to(device=self.device, dtype=torch.float32)
        if tuple(samples.shape[1:]) != tuple(self.samples.shape[1:]):
            raise ValueError(f"validation samples are {tuple(samples.shape)}, the training set {tuple(self.samples.shape)}")
        V, F = int(samples.shape[0]), self.F
        scale, center, inv, lo, hi, keep = self._loss_vecs
        wn = torch.full((F,), 1.0 / (V * self.cells * F * self.K), dtype=torch.float32, device=self.device)
        total = torch.zeros((), dtype=torch.float64, device=self.device)
        for i in range(0, V, self.B):
            S = min(self.B, V - i)
            rows = S * self.cells
            self._batch[:S].copy_(samples[i:i + S])
            for k in range(self.K):
                self._forward(k, S)
                ops.train_mse_grad(self._act[k]["y"].tensor.view(-1, F)[:rows], scale, center, inv, lo, hi, keep, wn,
                                   self._batch.view(-1, F), self._d["y"].tensor.view(-1, F)[:rows], self._loss[k:k + 1], self._loss_ws,
                                   idx=self._rows[k][:rows])
            total += self._loss.sum()
        return float(total.cpu())

    # -- reading the state back ----------------------------------------------------------------------
    def _host(self, buffer: torch.Tensor) -> Dict[str, Tuple[np.ndarray, ...]]:
        host = self._flat.to_host(buffer)
        return {name: tuple(host[name, f] for f in fields) for name, fields in self._fields.items()}

    def parameters(self) -> Dict[str, Tuple[np.ndarray, ...]]:
        """``layer_plan`` name -> ``(w_self, w_neigh, bias)`` or ``(weight, bias)`` as numpy arrays."""
        return self._host(self.params)

    def gradients(self) -> Dict[str, Tuple[np.ndarray, ...]]:
        """The gradient buffer in the layout of ``parameters``."""
        return self._host(self.grads)

    def spec(self) -> GraphUNetSpec:
        """The network as it stands, with the scalers it was given."""
        s = self._spec
        layers = {name: (SageLayer if len(arrays) == 3 else UpLayer)(*arrays) for name, arrays in self.parameters().items()}
        return GraphUNetSpec(s.variables, s.depth, s.min_filters, s.activation, layers)
