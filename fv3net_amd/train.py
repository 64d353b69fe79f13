"""Training state of the dense column network on the device, and its Jacobian (csrc/mlp_train.hip);
``PrecipitativeTrainer`` is the same state with the loss behind the precipitative closure (section 25), ``EmulatorTrainer`` with the
multi-variable loss of the microphysics emulators (section 26).

``DenseTrainer`` owns every tensor the stateless ``fv3hip_train_*`` entry points work on: one flat float32 parameter buffer
(per layer the kernel ``[in][out]`` followed by its bias; the heads are one concatenated layer, as ``MlpSpec.out_kernel`` is),
the gradient and Adam moment buffers of the same layout, the device-resident step counter, the activation buffers of the
largest batch, the chunk workspace of the weight gradient, and -- for training -- the resident normalised inputs and the
targets.  PyTorch supplies memory and the stream only.
"""
import dataclasses
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .train_state import DeviceMseLoss, FlatParameters, capture_step, check_batch, split_heads, upload


@dataclasses.dataclass
class MseLoss:
    """Per-feature arrays ``[F_out]`` of the loss of ``fit.train_dense_model``: sum over the outputs of
    ``mean(((clamp(yhat * scale + center, lo, hi) - t) / cstd) ** 2)`` over the kept (not clipped away) features."""

    scale: np.ndarray
    center: np.ndarray
    inv_cstd2: np.ndarray
    lo: np.ndarray        # -inf: no lower limit
    hi: np.ndarray        # +inf: no upper limit
    keep: np.ndarray      # 0 / 1
    kept: np.ndarray      # kept features of the feature's output

    def wnorm(self, n: int) -> np.ndarray:
        return (1.0 / (float(n) * np.maximum(np.asarray(self.kept, np.float64), 1.0))).astype(np.float32)


class DenseTrainer:
    """``kernels[l]`` is ``[in][out]``; every layer but the last is followed by ReLU (``relu=False``: by nothing)."""

    def __init__(self, kernels: Sequence[np.ndarray], biases: Sequence[np.ndarray], device="cuda", xin: Optional[np.ndarray] = None,
                 targets: Optional[np.ndarray] = None, loss: Optional[MseLoss] = None, max_batch: int = 512,
                 learning_rate: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, relu: bool = True):
        self.device = torch.device(device)
        ops._require_device(torch.empty(1, device=self.device))
        if len(kernels) != len(biases) or not kernels:
            raise ValueError("one bias per kernel, at least one layer")
        self.shapes = [(int(k.shape[0]), int(k.shape[1])) for k in kernels]
        for l, ((_, o), b) in enumerate(zip(self.shapes, biases)):
            if tuple(np.shape(b)) != (o,) or (l + 1 < len(self.shapes) and self.shapes[l + 1][0] != o):
                raise ValueError("layer shapes do not chain")
        self.relu = bool(relu)
        self.lr, self.betas, self.eps = float(learning_rate), (float(betas[0]), float(betas[1])), float(eps)
        self.max_batch = int(max_batch)
        dev = self.device

        pairs = [pair for l, (k, b) in enumerate(zip(kernels, biases)) for pair in ((("w", l), k), (("b", l), b))]   # kernel, then its bias
        flat = self._flat = FlatParameters(pairs, dev)
        self.params, self.grads, self.m, self.v, self.step_count = flat.params, flat.grads, flat.m, flat.v, flat.step_count
        layers = range(len(self.shapes))
        p, g = flat.views(flat.params), flat.views(flat.grads)
        self.w, self.b = [p["w", l] for l in layers], [p["b", l] for l in layers]
        self.dw, self.db = [g["w", l] for l in layers], [g["b", l] for l in layers]

        self.k_in, self.f_out = self.shapes[0][0], self.shapes[-1][1]
        self._h = [torch.zeros((self.max_batch, o), dtype=torch.float32, device=dev) for _, o in self.shapes]
        self._dh = [torch.zeros((self.max_batch, o), dtype=torch.float32, device=dev) for _, o in self.shapes]
        ws = max(ops.train_backward_weight_workspace_floats(self.max_batch, k, o) for k, o in self.shapes)
        self._ws = torch.zeros(ws, dtype=torch.float32, device=dev) if ws else None
        self._loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self._loss_ws = torch.zeros(ops.train_loss_workspace_doubles(), dtype=torch.float64, device=dev)

        self.xin = self.targets = None
        self._mse: Optional[DeviceMseLoss] = None
        if xin is not None:
            if targets is None or loss is None:
                raise ValueError("training needs xin, targets and loss together")
            self.xin, self.targets = upload(xin, dev), upload(targets, dev)
            if self.xin.shape[1] != self.k_in or self.targets.shape[1] != self.f_out or self.xin.shape[0] != self.targets.shape[0]:
                raise ValueError("xin / targets do not match the network")
            self._mse = DeviceMseLoss(loss, dev)
        self._jac = None

    @classmethod
    def from_spec(cls, spec, device="cuda") -> "DenseTrainer":
        """The network of an ``MlpSpec`` (no training data: for ``jacobian``)."""
        return cls(list(spec.hidden_kernels) + [spec.out_kernel], list(spec.hidden_biases) + [spec.out_bias], device=device, max_batch=1,
                   relu=spec.activation == "relu")

    # -- one optimiser step ------------------------------------------------------------------
    def _forward(self, a: torch.Tensor, idx: Optional[torch.Tensor], n: int):
        last = len(self.shapes) - 1
        for l in range(last + 1):
            ops.train_linear_forward(a, self.w[l], self.b[l], self._h[l][:n], idx=idx, relu=self.relu and l < last)
            a, idx = self._h[l][:n], None

    def step(self, idx: torch.Tensor) -> None:
        """One Adam step on the minibatch ``idx`` (int64 row numbers, on the device); the loss stays on the device."""
        if self.xin is None:
            raise RuntimeError("this trainer holds no training data")
        check_batch(int(idx.shape[0]), self.max_batch)
        self.backward(idx)
        self._flat.adam(self.lr, self.betas, self.eps)

    def backward(self, idx: torch.Tensor) -> None:
        """Forward, loss and the gradient of every parameter for the minibatch ``idx``, into ``self.grads``."""
        n = int(idx.shape[0])
        last = len(self.shapes) - 1
        self._forward(self.xin, idx, n)
        self._loss_grad(idx, n)
        for l in range(last, -1, -1):
            if l == 0:
                ops.train_linear_backward_weight(self.xin, self._dh[0][:n], self.dw[0], self.db[0], idx=idx, workspace=self._ws)
            else:
                ops.train_linear_backward_weight(self._h[l - 1][:n], self._dh[l][:n], self.dw[l], self.db[l], workspace=self._ws)
                ops.train_linear_backward_data(self._dh[l][:n], self.w[l], self._h[l - 1][:n] if self.relu else None, self._dh[l - 1][:n])

    def _loss_grad(self, idx: torch.Tensor, n: int) -> None:
        """The loss stage: from the head layer's output ``_h[-1][:n]`` to its gradient ``_dh[-1][:n]`` and ``_loss``."""
        self._mse.grad(self._h[-1][:n], self.targets, self._dh[-1][:n], self._loss, self._loss_ws, idx)

    def capture(self, idx: torch.Tensor) -> "torch.cuda.CUDAGraph":
        """``train_state.capture_step``: a HIP graph of ``step(idx)``, after one eager step that counts as a step."""
        return capture_step(self, idx)

    def loss(self) -> float:
        """The loss of the last step's minibatch (before its update), read back."""
        return float(self._loss.cpu()[0])

    # -- reading the state back ----------------------------------------------------------------
    def _host(self, buffer: torch.Tensor, head_sizes: Optional[Sequence[int]]):
        host = self._flat.to_host(buffer)
        layers = range(len(self.shapes))
        return split_heads([host["w", l] for l in layers], [host["b", l] for l in layers], self.f_out, head_sizes)

    def parameters(self, head_sizes: Optional[Sequence[int]] = None):
        """``(hidden_kernels, hidden_biases, output_kernels, output_biases)`` as numpy arrays, the order ``fit.spec_from_arrays``
        takes them in; the concatenated head layer is cut into ``head_sizes``."""
        return self._host(self.params, head_sizes)

    def gradients(self, head_sizes: Optional[Sequence[int]] = None):
        """The gradient buffer in the layout of ``parameters``."""
        return self._host(self.grads, head_sizes)

    # -- Jacobian --------------------------------------------------------------------------------
    def jacobian(self, x_row) -> Tuple[np.ndarray, np.ndarray]:
        """``(J, yhat)``: ``J[f][k]`` = d yhat[f] / d x[k] of the raw head outputs at the normalised input row ``x_row`` -- one
        forward pass of one row, then backward-data on ``F_out`` one-hot cotangent rows that share its activations."""
        dev, f, last = self.device, self.f_out, len(self.shapes) - 1
        x = torch.as_tensor(np.asarray(x_row, np.float32).reshape(1, self.k_in)).to(dev)
        if self._jac is None:
            self._jac = ([torch.zeros((1, o), dtype=torch.float32, device=dev) for _, o in self.shapes],
                         [torch.zeros((f, k), dtype=torch.float32, device=dev) for k, _ in self.shapes],
                         torch.eye(f, dtype=torch.float32, device=dev))
        acts, cots, eye = self._jac
        a = x
        for l in range(last + 1):
            ops.train_linear_forward(a, self.w[l], self.b[l], acts[l], relu=self.relu and l < last)
            a = acts[l]
        dh = eye
        for l in range(last, -1, -1):
            p = acts[l - 1] if (l > 0 and self.relu) else None
            ops.train_linear_backward_data(dh, self.w[l], p, cots[l], shared_p=True)
            dh = cots[l]
        return cots[0].cpu().numpy(), acts[last].cpu().numpy()[0]


@dataclasses.dataclass
class PrecipLoss:
    """What ``fv3hip_train_precip_loss_grad`` takes besides the data: the de-normalisation of dQ1 (``1``) and of dQ2 and the column
    precipitation (``2``), ``1 / max(std, 1e-12) ** 2`` of the three targets, the coupling and the activity regulariser."""

    scale1: np.ndarray
    center1: np.ndarray
    scale2: np.ndarray
    center2: np.ndarray
    inv_cstd2_1: np.ndarray
    inv_cstd2_2: np.ndarray
    inv_cstd2_3: float
    couple: bool = True
    has_dead: bool = False
    l1: float = 0.0
    l2: float = 0.0


class PrecipitativeTrainer(DenseTrainer):
    """The dense trainer with the loss behind the precipitative closure.  The head layer is
    ``[ dQ1 (nz) | dQ2 (nz) | dead (1, with loss.has_dead) | column precipitation (nz) ]``; besides the normalised inputs the
    trainer holds the raw ``delp [rows, nz]``, ``physics_precip [rows]`` and the targets ``dQ1``, ``dQ2`` ``[rows, nz]`` and
    ``total_precipitation_rate [rows]``."""

    def __init__(self, kernels: Sequence[np.ndarray], biases: Sequence[np.ndarray], device="cuda", *, xin: np.ndarray, delp: np.ndarray,
                 physics_precip: np.ndarray, targets: Sequence[np.ndarray], loss: PrecipLoss, max_batch: int = 512,
                 learning_rate: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8):
        super().__init__(kernels, biases, device=device, max_batch=max_batch, learning_rate=learning_rate, betas=betas, eps=eps)
        dev = self.device
        nz = int(np.shape(loss.scale1)[0])
        if self.f_out != 3 * nz + int(bool(loss.has_dead)):
            raise ValueError(f"the head layer has {self.f_out} features, the loss {nz} levels (has_dead={bool(loss.has_dead)})")
        self.nz, self.precip_loss = nz, loss
        self.xin = upload(xin, dev)
        rows = int(self.xin.shape[0])
        t1, t2, t3 = targets
        # dQ1 and dQ2 side by side in one array: one row stride for both
        self.targets = upload(np.concatenate([t1, t2], axis=1), dev)
        self.t3 = upload(np.reshape(t3, -1), dev)
        self.delp = upload(delp, dev)
        self.physics_precip = upload(np.reshape(physics_precip, -1), dev)
        if self.xin.shape[1] != self.k_in or tuple(self.targets.shape) != (rows, 2 * nz) or tuple(self.delp.shape) != (rows, nz) or \
                self.t3.shape[0] != rows or self.physics_precip.shape[0] != rows:
            raise ValueError("xin, delp, physics_precip and the targets do not match the network or each other")
        self._loss_arrays = {name: upload(getattr(loss, name), dev)
                             for name in ("scale1", "center1", "scale2", "center2", "inv_cstd2_1", "inv_cstd2_2")}

    def _loss_grad(self, idx: torch.Tensor, n: int) -> None:
        la, pl, nz = self._loss_arrays, self.precip_loss, self.nz
        ops.train_precip_loss_grad(self._h[-1][:n], la["scale1"], la["center1"], la["scale2"], la["center2"], la["inv_cstd2_1"],
                                   la["inv_cstd2_2"], pl.inv_cstd2_3, self.delp, self.physics_precip, self.targets[:, :nz],
                                   self.targets[:, nz:], self.t3, self._dh[-1][:n], self._loss, self._loss_ws, idx=idx, couple=pl.couple,
                                   has_dead=pl.has_dead, l1=pl.l1, l2=pl.l2)


class EmulatorTrainer(DenseTrainer):
    """The dense trainer with the multi-variable loss of the microphysics emulators (``ops.train_emulator_loss_grad``, DESIGN.md
    section 26).  ``heads``: ``ops.EmulatorHead`` descriptors holding numpy arrays (uploaded here); ``slot_names[s]`` names the
    variable of slot ``s``.  ``levels = 1``: the "dense" / "linear" architectures, ``xin [rows, K]``.  ``levels = nz``:
    "dense-local", ``xin [rows * nz, n_inputs]`` (row ``r * nz + z``); the inherited GEMMs then run on ``n * nz`` network rows
    whose row table ``idx * nz + arange(nz)`` is written into a preallocated buffer, and ``max_batch`` still counts batch rows.

    Every ``step`` / ``backward`` / ``evaluate`` adds its loss and values into a device accumulator; ``epoch_means`` reads and
    clears it.  The number of calls is counted on the host: after replaying a captured step pass ``epoch_means(steps=...)``."""

    def __init__(self, kernels: Sequence[np.ndarray], biases: Sequence[np.ndarray], device="cuda", *, xin: np.ndarray, heads: Sequence,
                 slot_names: Sequence[str], levels: int = 1, max_batch: int = 512, learning_rate: float = 1e-3,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-7, relu: bool = True):
        self.levels, self.batch_cap = int(levels), int(max_batch)
        super().__init__(kernels, biases, device=device, max_batch=self.batch_cap * self.levels, learning_rate=learning_rate, betas=betas,
                         eps=eps, relu=relu)
        dev = self.device
        self.xin = upload(xin, dev)
        if self.xin.dim() != 2 or self.xin.shape[1] != self.k_in or self.xin.shape[0] % self.levels:
            raise ValueError(f"xin {tuple(self.xin.shape)} does not match {self.k_in} inputs and {self.levels} levels")
        self.rows = int(self.xin.shape[0]) // self.levels

        def up(a):
            return None if a is None else upload(a, dev)

        arrays = ("scale", "center", "target", "inv", "before", "target_after", "inv_after")
        self.heads = [dataclasses.replace(h, **{k: up(getattr(h, k)) for k in arrays}) for h in heads]
        self.table = ops.EmulatorHeadTable(self.heads, self.levels)
        if self.table.f != self.f_out or (self.table.rows is not None and self.table.rows != self.rows):
            raise ValueError(f"the heads cover {self.table.f} features of {self.table.rows} rows, the network has {self.f_out} "
                             f"and {self.rows}")
        self.slot_names = list(slot_names)
        if len(self.slot_names) != self.table.n_slots:
            raise ValueError(f"{len(self.slot_names)} slot names for {self.table.n_slots} slots")
        ns = self.table.n_slots
        self._values = torch.zeros(max(ns, 1), dtype=torch.float64, device=dev)
        self._accum = torch.zeros(1 + ns, dtype=torch.float64, device=dev)
        self._accum_calls = 0
        self._emu_ws = torch.zeros(ops.train_emulator_loss_workspace_doubles(), dtype=torch.float64, device=dev)
        self._batch_idx: Optional[torch.Tensor] = None
        if self.levels > 1:
            self._level = torch.arange(self.levels, dtype=torch.int64, device=dev)
            self._row0 = torch.zeros(self.batch_cap, dtype=torch.int64, device=dev)
            self._net_idx = torch.zeros(self.batch_cap * self.levels, dtype=torch.int64, device=dev)

    def _network_rows(self, idx: torch.Tensor) -> torch.Tensor:
        n = check_batch(int(idx.shape[0]), self.batch_cap)
        if self.levels == 1:
            return idx
        net = self._net_idx[:n * self.levels]
        torch.mul(idx, self.levels, out=self._row0[:n])
        torch.add(self._row0[:n].unsqueeze(1), self._level, out=net.view(n, self.levels))
        return net

    def backward(self, idx: torch.Tensor) -> None:
        self._batch_idx = idx
        super().backward(self._network_rows(idx))

    def _loss_grad(self, net_idx: torch.Tensor, m: int) -> None:
        ops.train_emulator_loss_grad(self._h[-1][:m], self.table, self._dh[-1][:m], self._values, self._loss, self._emu_ws,
                                     idx=self._batch_idx, accum=self._accum)
        self._accum_calls += 1

    def loss_stage(self, idx: torch.Tensor):
        """The loss launch alone on the head layer's output that the last ``step`` / ``backward`` / ``evaluate`` of a batch of
        this size left: ``(yhat, dY)``, views of the trainer's buffers ``[n * levels, F]``; ``loss`` and ``values`` are updated
        (and the accumulator: it counts as a call)."""
        m = int(idx.shape[0]) * self.levels
        self._batch_idx = idx
        self._loss_grad(None, m)
        return self._h[-1][:m], self._dh[-1][:m]

    def evaluate(self, idx: torch.Tensor, accumulate: bool = True) -> None:
        """Forward and loss only on the rows ``idx``: no gradient is written, no parameter or moment touched."""
        net = self._network_rows(idx)
        m = int(net.shape[0])
        self._forward(self.xin, net, m)
        ops.train_emulator_loss_grad(self._h[-1][:m], self.table, None, self._values, self._loss, self._emu_ws, idx=idx,
                                     accum=self._accum if accumulate else None)
        self._accum_calls += int(accumulate)

    def values(self) -> Dict[str, float]:
        """The per-variable values of the last call, read back."""
        host = self._values.cpu().numpy()
        return {name: float(host[s]) for s, name in enumerate(self.slot_names)}

    def epoch_means(self, steps: Optional[int] = None) -> Dict[str, float]:
        """``{"loss": ..., name: ...}``: the accumulator divided by the calls since it was last cleared; clears it."""
        calls = self._accum_calls if steps is None else int(steps)
        host = self._accum.cpu().numpy() / max(calls, 1)
        self._accum.zero_()
        self._accum_calls = 0
        return {"loss": float(host[0]), **{name: float(host[1 + s]) for s, name in enumerate(self.slot_names)}}


def predict_graph_jacobians(spec, profiles: Mapping[str, np.ndarray], device="cuda", trainer: Optional[DenseTrainer] = None,
                            values: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, Dict[str, np.ndarray]]:
    """``{output: {source: d output / d source}}`` of an ``MlpSpec``'s predict graph at one profile per source (``[nfeat]``,
    cast to float32 as ``predict`` casts): input clip, ``log(max(x, eps))`` where the spec asks for it, normalisation, network,
    de-normalisation, limits and masked levels.  Each array is ``[nfeat_out][len(profile)]`` in float64; columns of levels
    that no input reads, rows of masked levels and rows of outputs outside a limit (bounds inclusive) are exactly 0.  Residual
    outputs and the hidden output are left out.  ``values`` (a dict) receives each output's de-normalised float32 value at the
    profile, before limits and masks."""
    trainer = trainer or DenseTrainer.from_spec(spec, device)
    prof = {name: np.atleast_1d(np.asarray(profiles[name])).astype(np.float32) for name in dict.fromkeys(i.source for i in spec.inputs)}
    cols, slopes = [], []
    for i in spec.inputs:
        x = prof[i.source][i.start:i.start + i.nfeat]
        if x.shape[0] != i.nfeat:
            raise ValueError(f"{i.source!r} has {prof[i.source].shape[0]} features, the model reads [{i.start}, {i.start + i.nfeat})")
        slope = np.ones(i.nfeat, np.float64)
        if i.transform == "log":
            eps = np.float32(i.eps)
            with np.errstate(divide="ignore"):
                slope = np.where(x > eps, 1.0 / x.astype(np.float64), 0.0)
            x = np.log(np.maximum(x, eps))
        center = np.zeros(i.nfeat, np.float32) if i.center is None else np.broadcast_to(np.asarray(i.center, np.float32), (i.nfeat,))
        scale = np.ones(i.nfeat, np.float32) if i.scale is None else np.broadcast_to(np.asarray(i.scale, np.float32), (i.nfeat,))
        cols.append((x - center) / scale)
        slopes.append(slope / scale.astype(np.float64))
    jac, yhat = trainer.jacobian(np.concatenate(cols))
    jac = jac.astype(np.float64)

    out: Dict[str, Dict[str, np.ndarray]] = {}
    f0 = 0
    for o in spec.outputs:
        rows = jac[f0:f0 + o.nfeat]
        y = yhat[f0:f0 + o.nfeat]
        f0 += o.nfeat
        scale = np.ones(o.nfeat, np.float32) if o.scale is None else np.broadcast_to(np.asarray(o.scale, np.float32), (o.nfeat,))
        center = np.zeros(o.nfeat, np.float32) if o.center is None else np.broadcast_to(np.asarray(o.center, np.float32), (o.nfeat,))
        p = y * scale + center
        if values is not None:
            values[o.name] = p
        factor = scale.astype(np.float64)
        if o.min is not None:
            factor = np.where(p >= np.float32(o.min), factor, 0.0)
        if o.max is not None:
            factor = np.where(p <= np.float32(o.max), factor, 0.0)
        if o.mask is not None:
            factor = np.where(np.asarray(o.mask) != 0, factor, 0.0)
        per_source = {name: np.zeros((o.nfeat, p_.shape[0]), np.float64) for name, p_ in prof.items()}
        c0 = 0
        for i, slope in zip(spec.inputs, slopes):
            block = rows[:, c0:c0 + i.nfeat] * slope[None, :]
            block = np.where(factor[:, None] != 0, block * factor[:, None], 0.0)
            per_source[i.source][:, i.start:i.start + i.nfeat] += block
            c0 += i.nfeat
        out[o.name] = per_source
    return out
