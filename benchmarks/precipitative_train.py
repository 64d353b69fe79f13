"""One training step of the precipitative column network: ``fv3net_amd.train.PrecipitativeTrainer.step`` eager
and as a replayed HIP graph, next to the torch backend's step (``torch.nn.Linear``, autograd, ``torch.optim.Adam``: what
``fit.train_precipitative_model(backend="torch")`` runs) on the same device, the same resident data and the same minibatch, in
alternating windows of one run, timed with device events after warm-up.

  b512    79 + 79 + 79 + 1 -> 16 -> 16 -> 3 x 79 (the reference's defaults), batch 512
  b8192   the same, batch 8192

and the loss launch alone (``ops.train_precip_loss_grad``: the kernel and the one-block loss reduction) next to the same loss and
gradient as a PyTorch autograd expression on the raw head outputs, at both batches.  One JSON line per configuration.

    python3 benchmarks/precipitative_train.py [--configs b512,b8192] [--windows N] [--steps K] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.dense_train import alternating  # noqa: E402
from fv3net_amd import ops  # noqa: E402
from fv3net_amd.train import PrecipitativeTrainer, PrecipLoss  # noqa: E402

NZ, WIDTH = 79, 16
CONFIGS = {"b512": 512, "b8192": 8192}
N_ROWS = 16384
C_HEAT, C_G = float(np.float32(-2.5e6 / 1004.6)), float(np.float32(-1.0 / 9.80665))


def build(batch, dev, rng):
    sizes = (3 * NZ + 1, WIDTH, WIDTH, 3 * NZ)
    kernels = [(rng.normal(0, 1, (i, o)) / np.sqrt(i)).astype(np.float32) for i, o in zip(sizes[:-1], sizes[1:])]
    biases = [np.zeros(o, np.float32) for o in sizes[1:]]
    xin = rng.normal(0, 1, (N_ROWS, sizes[0])).astype(np.float32)
    delp = rng.uniform(300, 1500, (N_ROWS, NZ)).astype(np.float32)
    pp = rng.uniform(0, 1e-4, N_ROWS).astype(np.float32)
    std1, std2, std3 = np.full(NZ, 1e-4, np.float32), np.full(NZ, 1e-7, np.float32), np.float32(3e-5)
    targets = [rng.normal(0, 1, (N_ROWS, NZ)).astype(np.float32) * std1, rng.normal(0, 1, (N_ROWS, NZ)).astype(np.float32) * std2,
               (pp + rng.normal(0, 1, N_ROWS) * std3).astype(np.float32)]
    zero = np.zeros(NZ, np.float32)
    loss = PrecipLoss(scale1=std1, center1=zero, scale2=std2, center2=zero, inv_cstd2_1=(1 / std1.astype(np.float64) ** 2).astype(np.float32),
                      inv_cstd2_2=(1 / std2.astype(np.float64) ** 2).astype(np.float32), inv_cstd2_3=float(np.float32(1 / float(std3) ** 2)))
    trainer = PrecipitativeTrainer(kernels, biases, device=dev, xin=xin, delp=delp, physics_precip=pp, targets=targets, loss=loss,
                                   max_batch=batch)

    layers = []
    for l, (k, b) in enumerate(zip(kernels, biases)):
        lin = torch.nn.Linear(k.shape[0], k.shape[1])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(k.T.copy()))
            lin.bias.copy_(torch.from_numpy(b))
        layers += [lin] + ([torch.nn.ReLU()] if l < len(kernels) - 1 else [])
    net = torch.nn.Sequential(*layers).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    s1, s2 = torch.from_numpy(std1).to(dev), torch.from_numpy(std2).to(dev)
    t1, t2, t3 = trainer.targets[:, :NZ], trainer.targets[:, NZ:], trainer.t3

    def loss_expression(raw, idx):
        """The loss of the torch backend's loop on the raw head outputs ``[n, 3 NZ]`` (coupled, no regulariser)."""
        col_precip = raw[:, 2 * NZ:] * s2
        t_tend = raw[:, :NZ] * s1 + C_HEAT * col_precip
        q_tend = raw[:, NZ:2 * NZ] * s2 + col_precip
        precip = trainer.physics_precip[idx] + C_G * torch.sum(col_precip * trainer.delp[idx], dim=1)
        return torch.mean(((t_tend - t1[idx]) / s1) ** 2) + torch.mean(((q_tend - t2[idx]) / s2) ** 2) + \
            torch.mean(((precip - t3[idx]) / float(std3)) ** 2)

    def torch_step(idx):
        out = loss_expression(net(trainer.xin[idx]), idx)
        opt.zero_grad()
        out.backward()
        opt.step()

    return trainer, torch_step, loss_expression


def run(name, windows, steps, dev):
    batch = CONFIGS[name]
    rng = np.random.default_rng(0)
    trainer, torch_step, loss_expression = build(batch, dev, rng)
    idx = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(0))[:batch].to(dev)
    graph = trainer.capture(idx)
    eager, replay, library = alternating([lambda: trainer.step(idx), graph.replay, lambda: torch_step(idx)], windows, steps)
    result = {"config": name, "sizes": [3 * NZ + 1, WIDTH, WIDTH, 3 * NZ], "batch": batch, "hip_eager": eager, "hip_graph": replay,
              "torch": library, "hip_eager_over_torch": eager["median_ms"] / library["median_ms"],
              "hip_graph_over_torch": replay["median_ms"] / library["median_ms"], "loss_after": trainer.loss()}

    # the loss launch alone, on the head outputs the last step left
    raw = trainer._h[-1][:batch].clone().requires_grad_(True)

    def hip_loss():
        trainer._loss_grad(idx, batch)

    def torch_loss():
        raw.grad = None
        loss_expression(raw, idx).backward()

    stage, stage_torch = alternating([hip_loss, torch_loss], windows, steps)
    torch_loss()
    hip_loss()
    torch.cuda.synchronize()
    scale = float(raw.grad.abs().max())
    result.update({"loss_launch_hip": stage, "loss_launch_torch_autograd": stage_torch,
                   "loss_launch_hip_over_torch": stage["median_ms"] / stage_torch["median_ms"],
                   "loss_launch_max_difference_over_max_gradient": float((trainer._dh[-1][:batch] - raw.grad).abs().max()) / scale})
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="b512,b8192")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/precipitative_train.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    ops._require_device(torch.empty(1, device=dev))
    lines = [run(name, args.windows, args.steps, dev) for name in args.configs.split(",") if name]
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
