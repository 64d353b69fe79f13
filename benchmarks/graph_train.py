"""One training step of the graph U-Net: ``fv3net_amd.graph_train.GraphTrainer.step`` eager and as a
replayed HIP graph, next to the torch twin's step (``GraphUNetTwin``: an index gather, a mean and ``nn.Linear``; autograd;
``torch.optim.AdamW`` -- what ``fit.train_graph_model(backend="torch")`` runs) on the same device, the same resident samples and
the same batch, in alternating windows of one run, timed with device events after warm-up.

The state is section 16's: T + q (79 levels each) and two surface fields, 160 features, multistep 1.  Configurations: the
reference's defaults at C48 (min_filters 4, depth 1, batch 1); G1 (C48, min_filters 64, depth 2) at batch 1 and 8; G3 (C384,
min_filters 32, depth 3, batch 1).

FLOP per step: three times the forward's (``GraphUNetSpec.flops_per_node``: the forward, the data gradient and the weight
gradient are the same contraction) less the data gradient of ``first``, which nobody needs.  The TFLOP/s are whole-step
figures (launch gaps, the loss, the staging of the batch and AdamW included), not a kernel's share of peak; the fraction is of
the 157.3 TFLOP/s float32 matrix peak.  ``launches`` counts the kernels of one step: every entry point is one, except the loss,
AdamW and a weight gradient of more than one chunk (two each), plus torch's gather of the batch.  One JSON line per
configuration.

    python3 benchmarks/graph_train.py [--configs defaults,G1_b1,G1_b8,G3] [--windows N] [--out profiles/graph_train.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.conv_train import alternating  # noqa: E402
from benchmarks.graph_rollout import make_spec  # noqa: E402
from fv3net_amd import _lib  # noqa: E402
from fv3net_amd.fit.graph import _multistep_loss, twin_from_spec  # noqa: E402
from fv3net_amd.graph_train import GraphTrainer  # noqa: E402

FP32_MATRIX_TFLOPS = 157.3
# name -> (n, min_filters, depth, batch, resident samples, steps per window)
CONFIGS = {"defaults": (48, 4, 1, 1, 8, 40), "G1_b1": (48, 64, 2, 1, 8, 20), "G1_b8": (48, 64, 2, 8, 16, 5), "G3": (384, 32, 3, 1, 2, 3)}
TWO_LAUNCHES = ("fv3hip_train_mse_grad", "fv3hip_train_adamw", "fv3hip_graph_up2_backward_weight", "fv3hip_graph_sage_backward_weight")


def step_flop(spec, n, batch):
    cells = batch * 6 * n * n
    return (3.0 * spec.flops_per_node() - 4.0 * spec.n_features * spec.min_filters) * cells


def count_launches(trainer, idx):
    """The kernels of one eager step (every weight gradient here has more than one chunk)."""
    calls, real = [], _lib.call_on

    def counting(where, name, *args):
        calls.append(name)
        return real(where, name, *args)

    _lib.call_on = counting
    try:
        trainer.step(idx)
    finally:
        _lib.call_on = real
    return 1 + sum(2 if name in TWO_LAUNCHES else 1 for name in calls)


def run(name, windows, dev):
    n, m, depth, batch, resident, steps = CONFIGS[name]
    rng = np.random.default_rng(0)
    spec = make_spec(rng, depth, m)
    gen = torch.Generator(device=dev).manual_seed(0)
    samples = torch.randn((resident, 2, 6, n, n, spec.n_features), device=dev, generator=gen)
    trainer = GraphTrainer(spec, samples, multistep=1, max_batch=batch, device=dev, lr=1e-4)
    twin = twin_from_spec(spec, device=dev).train()
    opt = torch.optim.AdamW(twin.parameters(), lr=1e-4)
    idx = torch.randperm(resident, generator=torch.Generator().manual_seed(0))[:batch].to(dev)

    def torch_step():   # (the loop body of fit.train_graph_model, backend "torch")
        opt.zero_grad()
        _multistep_loss(twin, trainer.samples[idx], 1).backward()
        opt.step()

    launches = count_launches(trainer, idx)
    graph = trainer.capture(idx)
    eager, replay, library = alternating([lambda: trainer.step(idx), graph.replay, torch_step], windows, steps)
    flop = step_flop(spec, n, batch)
    result = {"config": name, "n": n, "features": spec.n_features, "min_filters": m, "depth": depth, "batch": batch,
              "flop_per_step": flop, "launches": launches, "hip_eager": eager, "hip_graph": replay, "torch": library}
    for key in ("hip_eager", "hip_graph", "torch"):
        result[key]["tflops"] = flop / (result[key]["median_ms"] * 1e-3) / 1e12
        result[key]["fraction_of_fp32_matrix_peak"] = result[key]["tflops"] / FP32_MATRIX_TFLOPS
    result["hip_eager_over_torch"] = eager["median_ms"] / library["median_ms"]
    result["hip_graph_over_torch"] = replay["median_ms"] / library["median_ms"]
    result["loss_after"] = trainer.loss()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/graph_train.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    lines = []
    for name in (c for c in args.configs.split(",") if c):
        lines.append(run(name, args.windows, dev))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
