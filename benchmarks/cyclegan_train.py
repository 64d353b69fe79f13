"""One CycleGAN ``train_on_batch`` at the reference's production configuration (projects/cyclegan/0K_to_8K/training.yaml: C48,
two 2-D variables, generator n_convolutions 2 / n_resnet 6 / max_filters 256 with 4 x 4 strided layers, discriminator 3 strided
levels / max_filters 256 with 3 x 3 strided layers, ``halo_conv2d``) at batch 1 and batch 4: ``backend="hip"`` (the training
kernels of DESIGN section 27) against ``backend="torch"`` (the twins under autograd) on the same device in the same run.

Times are per step: HIP events after warm-up, the median of five windows of back-to-back steps, minimum and maximum beside it.
``ratio`` is hip / torch: below 1 the HIP step is the faster one.  Also the three new kernels alone on the 256 -> 256 3 x 3
layer at 12 x 12 (the bottom level), one sample.  One JSON line per workload; all of them go to profiles/cyclegan_train.json.

    python3 benchmarks/cyclegan_train.py [--steps K] [--warmup W] [--batches 1,4]
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cyclegan_cases  # noqa: E402
from fv3net_amd import fit, ops  # noqa: E402
from fv3net_amd.cube import _Slice  # noqa: E402

NX, CHANNELS = 48, 2


def timed(fn, steps, warmup, repeats=5):
    """(median, min, max) ms per call over ``repeats`` windows of ``steps`` back-to-back calls between two HIP events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(steps):
            fn()
        stop.record()
        stop.synchronize()
        windows.append(start.elapsed_time(stop) / steps)
    windows.sort()
    return windows[len(windows) // 2], windows[0], windows[-1]


def production_config():
    return fit.CycleGANNetworkConfig(
        optimizer=dict(name="Adam", kwargs=dict(lr=2e-4)), generator=dict(n_convolutions=2, n_resnet=6, max_filters=256, strided_kernel_size=4),
        discriminator=dict(n_convolutions=3, max_filters=256, strided_kernel_size=3), convolution_type="halo_conv2d",
        identity_loss=dict(loss_type="mae"), cycle_loss=dict(loss_type="mae"), gan_loss=dict(loss_type="mse"), cycle_weight=10.0)


def step_times(device, batch, steps, warmup):
    lon, xyz = cyclegan_cases.synthetic_grid(NX)
    rng = np.random.default_rng(0)
    seconds = lambda: torch.from_numpy((1.7e9 + 3600.0 * rng.integers(0, 48, (batch, 1))).astype(np.float32).astype(np.float64))   # noqa: E731
    state = lambda: torch.from_numpy(rng.normal(0, 1, (batch, 1, 6, CHANNELS, NX, NX)).astype(np.float32)).to(device)          # noqa: E731
    a, b = (seconds(), state()), (seconds(), state())
    out = {"workload": f"train_on_batch_b{batch}", "batch": batch}
    for backend in ("hip", "torch"):
        random.seed(0)
        # (the torch baseline pads with the batched gathers: the tile-by-tile pad that reproduces the reference's bits is slower)
        trainer = production_config().build(CHANNELS, NX, batch, lon, xyz, seed=0, backend=backend, device=device,
                                            reference_order_gradients=False)
        med, lo, hi = timed(lambda: trainer.train_on_batch(a, b), steps, warmup)
        out[f"{backend}_ms"], out[f"{backend}_ms_min"], out[f"{backend}_ms_max"] = med, lo, hi
        del trainer
        torch.cuda.empty_cache()
    out["ratio"] = out["hip_ms"] / out["torch_ms"]
    return out


def kernel_times(device, steps, warmup):
    """The three new kernels alone: 256 -> 256, 3 x 3, 12 x 12 faces, one sample, cube halos."""
    S, n, c, kind, k = 1, 12, 256, "regular", 3
    new = lambda *shape: torch.randn(shape, device=device)   # noqa: E731
    x, dy, w, dx, dw, db = new(S, 6, n, n, c), new(S, 6, n, n, c), new(k, k, c, c), new(S, 6, n, n, c), new(k, k, c, c), new(c)
    pad = new(ops.cyclegan_train_backward_data_workspace_floats(S, n, c, kind, k, True))
    ws = new(ops.cyclegan_train_backward_weight_workspace_floats(S, n, c, c, kind, k))
    st = torch.empty((2, S, 6, c), device=device)
    st[0], st[1] = 0.0, 1.0
    cases = {
        "backward_data": lambda: ops.cyclegan_train_backward_data(_Slice(dy, c), w, _Slice(dx, c), S, n, c, c, kind, k, True, pad),
        "backward_weight": lambda: ops.cyclegan_train_backward_weight(_Slice(x, c), _Slice(dy, c), dw, db, S, n, c, c, kind, k, True, ws),
        "norm_backward": lambda: ops.cyclegan_train_norm_backward(_Slice(dy, c), _Slice(x, c), st[0], st[1], None, 0.0, _Slice(dx, c), None, S, n, c),
        "forward": lambda: ops.cyclegan_train_conv(_Slice(x, c), w, db, _Slice(dx, c), S, n, c, c, kind, k, True),
    }
    flops = 2.0 * 9 * c * c * S * 6 * n * n
    out = {"workload": "kernels_256x256_3x3_n12", "gemm_gflop": flops / 1e9}
    for name, fn in cases.items():
        med, lo, hi = timed(fn, steps, warmup)
        out[f"{name}_ms"], out[f"{name}_ms_min"], out[f"{name}_ms_max"] = med, lo, hi
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--steps", type=int, default=3)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--batches", default="1,4")
    args = parser.parse_args()
    device = torch.device("cuda:0")
    results = [kernel_times(device, 50, 10)]
    print(json.dumps(results[-1]), flush=True)
    for batch in (int(b) for b in args.batches.split(",")):
        results.append(step_times(device, batch, args.steps, args.warmup))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "cyclegan_train.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
