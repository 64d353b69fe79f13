"""One training step of the dense column network: ``fv3net_amd.train.DenseTrainer.step`` eager and as a
replayed HIP graph, next to the torch backend's step (``torch.nn.Linear``, autograd, ``torch.optim.Adam``: what
``fit.train_dense_model(backend="torch")`` runs) on the same device, the same resident data and the same minibatch, in
alternating windows of one run, timed with device events after warm-up.

  a       the C48 plumbing configuration, 159 -> 8 -> 8 -> 158, batch 512
  b512    the Zhao-Carr shape, 711 -> 256 -> 256 -> 396, batch 512
  b8192   the same, batch 8192

and ``HipDenseModel.jacobians`` (what ``input_sensitivity`` computes on the device, with its host work and copies) at the
Zhao-Carr shape, timed with a host clock around a synchronised call.

FLOP per step: 6 n sum(in * out) (forward, backward weight, backward data: 2 n in out each) less the first layer's backward
data, which nobody needs.  The TFLOP/s are whole-step figures (launch gaps, the loss and Adam included), not a kernel's share
of peak; the fraction is of the 157.3 TFLOP/s float32 matrix peak.  One JSON line per configuration.

    python3 benchmarks/dense_train.py [--configs a,b512,b8192] [--windows N] [--steps K]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fv3net_amd import fit  # noqa: E402
from fv3net_amd.train import DenseTrainer, MseLoss  # noqa: E402

FP32_MATRIX_TFLOPS = 157.3
CONFIGS = {"a": ((159, 8, 8, 158), 512), "b512": ((711, 256, 256, 396), 512), "b8192": ((711, 256, 256, 396), 8192)}
N_ROWS = 16384


def step_flop(sizes, n):
    pairs = list(zip(sizes[:-1], sizes[1:]))
    return 6 * n * sum(i * o for i, o in pairs) - 2 * n * pairs[0][0] * pairs[0][1]


def window_ms(fn, count):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(count):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / count


def alternating(fns, windows, count, warmup=3):
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            times[i].append(window_ms(fn, count))
    return [{"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))} for t in times]


def build(sizes, batch, dev, rng):
    kernels = [(rng.normal(0, 1, (i, o)) / np.sqrt(i)).astype(np.float32) for i, o in zip(sizes[:-1], sizes[1:])]
    biases = [np.zeros(o, np.float32) for o in sizes[1:]]
    xin, targets = rng.normal(0, 1, (N_ROWS, sizes[0])).astype(np.float32), rng.normal(0, 1, (N_ROWS, sizes[-1])).astype(np.float32)
    f = sizes[-1]
    one = np.ones(f, np.float32)
    loss = MseLoss(scale=one, center=0 * one, inv_cstd2=one, lo=np.full(f, -np.inf, np.float32), hi=np.full(f, np.inf, np.float32),
                   keep=one, kept=np.full(f, float(f)))
    trainer = DenseTrainer(kernels, biases, device=dev, xin=xin, targets=targets, loss=loss, max_batch=batch)

    layers = []
    for l, (k, b) in enumerate(zip(kernels, biases)):
        lin = torch.nn.Linear(k.shape[0], k.shape[1])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(k.T.copy()))
            lin.bias.copy_(torch.from_numpy(b))
        layers += [lin] + ([torch.nn.ReLU()] if l < len(kernels) - 1 else [])
    net = torch.nn.Sequential(*layers).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    x_t, t_t = trainer.xin, trainer.targets

    def torch_step(idx):
        pred = net(x_t[idx])   # (scale 1, center 0, no limits: the loss of train_dense_model with one output)
        out = torch.mean((pred - t_t[idx]) ** 2)
        opt.zero_grad()
        out.backward()
        opt.step()

    return trainer, torch_step, kernels, biases


def run(name, windows, steps, dev):
    sizes, batch = CONFIGS[name]
    rng = np.random.default_rng(0)
    trainer, torch_step, kernels, biases = build(sizes, batch, dev, rng)
    idx = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(0))[:batch].to(dev)
    graph = trainer.capture(idx)
    eager, replay, library = alternating([lambda: trainer.step(idx), graph.replay, lambda: torch_step(idx)], windows, steps)
    flop = step_flop(sizes, batch)
    result = {"config": name, "sizes": list(sizes), "batch": batch, "flop_per_step": flop, "hip_eager": eager, "hip_graph": replay,
              "torch": library}
    for key in ("hip_eager", "hip_graph", "torch"):
        result[key]["tflops"] = flop / (result[key]["median_ms"] * 1e-3) / 1e12
        result[key]["fraction_of_fp32_matrix_peak"] = result[key]["tflops"] / FP32_MATRIX_TFLOPS
    result["hip_eager_over_torch"] = eager["median_ms"] / library["median_ms"]
    result["hip_graph_over_torch"] = replay["median_ms"] / library["median_ms"]
    result["loss_after"] = trainer.loss()
    return result


def run_sensitivity(windows, dev):
    sizes = CONFIGS["b512"][0]
    rng = np.random.default_rng(1)
    kernels = [(rng.normal(0, 1, (i, o)) / np.sqrt(i)).astype(np.float32) for i, o in zip(sizes[:-1], sizes[1:])]
    spec = fit.spec_from_arrays(["x"], [np.zeros(sizes[0], np.float32)], [np.ones(sizes[0], np.float32)], kernels[:-1],
                                [np.zeros(k.shape[1], np.float32) for k in kernels[:-1]], ["y"], [kernels[-1]],
                                [np.zeros(sizes[-1], np.float32)], [np.zeros(sizes[-1], np.float32)], [np.ones(sizes[-1], np.float32)])
    model = fit.HipDenseModel(["x"], ["y"], spec)
    profile = {"x": rng.normal(0, 1, sizes[0]).astype(np.float32)}
    for _ in range(3):
        model.jacobians(profile)
    times = []
    for _ in range(windows * 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.jacobians(profile)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    flop = 2 * sizes[-1] * sum(i * o for i, o in zip(sizes[:-1], sizes[1:]))
    return {"config": "input_sensitivity_b", "sizes": list(sizes), "median_ms": float(np.median(times)), "min_ms": float(min(times)),
            "max_ms": float(max(times)), "backward_flop": flop}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="a,b512,b8192")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/dense_train.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    lines = [run(name, args.windows, args.steps, dev) for name in args.configs.split(",") if name]
    lines.append(run_sensitivity(args.windows, dev))
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
