"""One training step of the convolutional network: ``fv3net_amd.conv_train.ConvTrainer.step`` eager and as a
replayed HIP graph, next to the torch twin's step (``torch.nn.functional.conv2d``, autograd, ``torch.optim.Adam``, the
constraint after the update: what ``fit.train_convolutional_model(backend="torch")`` runs) on the same device, the same resident
data and the same tile-samples, in alternating windows of one run, timed with device events after warm-up.

The C48 default network: 159 -> 32 -> 32 -> 79 + 79 with 3 x 3 kernels on 48 x 48 tiles with a halo of 2 (52 x 52 cells in),
batches of 1, 6 and 16 tile-samples out of 24 resident ones.

FLOP per step: per hidden layer 2 P k k C F for the forward, the same for the weight gradient and -- not for the first layer,
whose input gradient nobody needs -- for the data gradient, P the layer's output pixels; the heads 6 P 32 158.  The TFLOP/s
are whole-step figures (launch gaps, the loss, Adam and the constraint included), not a kernel's share of peak; the fraction is
of the 157.3 TFLOP/s float32 matrix peak.  One JSON line per batch size.

    python3 benchmarks/conv_train.py [--batches 1,6,16] [--windows N] [--steps K] [--out profiles/conv_train.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fv3net_amd.conv_train import ConvTrainer  # noqa: E402
from fv3net_amd.train import MseLoss  # noqa: E402

FP32_MATRIX_TFLOPS = 157.3
N_TILE, K, CHANNELS, FILTERS, HEADS = 48, 3, 159, 32, (79, 79)
N_RESIDENT = 24


def step_flop(n):
    flop, c, ext = 0, CHANNELS, N_TILE + 2 * (K - 1)
    for layer in range(2):
        ext -= K - 1
        flop += (2 if layer == 0 else 3) * 2 * n * ext * ext * K * K * c * FILTERS
        c = FILTERS
    return flop + 6 * n * N_TILE * N_TILE * FILTERS * sum(HEADS)


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


def build(batch, dev, rng):
    ext = N_TILE + 2 * (K - 1)
    f_out = sum(HEADS)
    shapes = [(K, K, CHANNELS, FILTERS), (K, K, FILTERS, FILTERS)]
    kernels = [(rng.normal(0, 1, s) / np.sqrt(K * K * s[2])).astype(np.float32) for s in shapes]
    biases = [np.zeros(FILTERS, np.float32) for _ in shapes]
    out_k, out_b = (rng.normal(0, 1, (FILTERS, f_out)) / np.sqrt(FILTERS)).astype(np.float32), np.zeros(f_out, np.float32)
    xin = rng.normal(0, 1, (N_RESIDENT, ext, ext, CHANNELS)).astype(np.float32)
    targets = rng.normal(0, 1, (N_RESIDENT * N_TILE * N_TILE, f_out)).astype(np.float32)
    one = np.ones(f_out, np.float32)
    loss = MseLoss(scale=one, center=0 * one, inv_cstd2=one, lo=np.full(f_out, -np.inf, np.float32), hi=np.full(f_out, np.inf, np.float32),
                   keep=one, kept=np.concatenate([np.full(h, float(h)) for h in HEADS]))
    trainer = ConvTrainer(kernels, biases, out_k, out_b, xin, targets, loss, device=dev, max_batch=batch)

    F = torch.nn.functional
    tw = [torch.from_numpy(np.ascontiguousarray(w.transpose(3, 2, 0, 1))).to(dev).requires_grad_() for w in kernels]
    tb = [torch.from_numpy(b.copy()).to(dev).requires_grad_() for b in biases]
    cuts = np.cumsum([0] + list(HEADS))
    hw = [torch.from_numpy(np.ascontiguousarray(out_k[:, a:b].T[:, :, None, None])).to(dev).requires_grad_() for a, b in zip(cuts[:-1], cuts[1:])]
    hb = [torch.from_numpy(out_b[a:b].copy()).to(dev).requires_grad_() for a, b in zip(cuts[:-1], cuts[1:])]
    opt = torch.optim.Adam(tw + tb + hw + hb, lr=1e-3)
    x_t = trainer.xin.permute(0, 3, 1, 2)
    t_t = [trainer.targets.view(N_RESIDENT, N_TILE, N_TILE, f_out)[..., a:b] for a, b in zip(cuts[:-1], cuts[1:])]

    def torch_step(idx):   # (scale 1, center 0: the loop body of fit.conv._train_conv_torch)
        a = x_t[idx]
        for w, b in zip(tw, tb):
            a = torch.relu(F.conv2d(a, w, b))
        out = 0.0
        for w, b, t in zip(hw, hb, t_t):
            out = out + torch.mean((F.conv2d(a, w, b).permute(0, 2, 3, 1) - t[idx]) ** 2)
        opt.zero_grad()
        out.backward()
        opt.step()
        with torch.no_grad():
            for w in tw:
                w.copy_(0.5 * (w + w.transpose(2, 3)))

    return trainer, torch_step


def run(batch, windows, steps, dev):
    rng = np.random.default_rng(0)
    trainer, torch_step = build(batch, dev, rng)
    idx = torch.randperm(N_RESIDENT, generator=torch.Generator().manual_seed(0))[:batch].to(dev)
    graph = trainer.capture(idx)
    eager, replay, library = alternating([lambda: trainer.step(idx), graph.replay, lambda: torch_step(idx)], windows, steps)
    flop = step_flop(batch)
    result = {"config": f"c48_batch{batch}", "network": [CHANNELS, FILTERS, FILTERS, list(HEADS)], "kernel_size": K, "batch": batch,
              "flop_per_step": flop, "hip_eager": eager, "hip_graph": replay, "torch": library}
    for key in ("hip_eager", "hip_graph", "torch"):
        result[key]["tflops"] = flop / (result[key]["median_ms"] * 1e-3) / 1e12
        result[key]["fraction_of_fp32_matrix_peak"] = result[key]["tflops"] / FP32_MATRIX_TFLOPS
    result["hip_eager_over_torch"] = eager["median_ms"] / library["median_ms"]
    result["hip_graph_over_torch"] = replay["median_ms"] / library["median_ms"]
    result["loss_after"] = trainer.loss()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,6,16")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/conv_train.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    lines = []
    for batch in (int(b) for b in args.batches.split(",") if b):
        lines.append(run(batch, args.windows, args.steps, dev))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
