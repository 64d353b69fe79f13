"""One FMR ``train_on_batch`` at the reference's production configuration (projects/fmr/training.yaml: C48, four 2-D variables,
generator n_convolutions 2 / n_resnet 6 / max_filters 256 with ``samples_per_day`` 4 and geographic features, discriminator 3
strided 4 x 4 levels / max_filters 256, ``halo_conv2d``, windows of 4 times, mae identity and mse target and GAN losses with
weights 10 / 10 / 1 / 1) at batch 1 and batch 4: ``backend="hip"`` against ``backend="torch"`` (the twins
under autograd) on the same device in the same run.

Times are per step: HIP events after warm-up, the median of five windows of back-to-back steps, minimum and maximum beside it.
``ratio`` is hip / torch: below 1 the HIP step is the faster one.  Also, alone:

  * the weight gradient of the 261 -> 256 3 x 3 step layer at 12 x 12, one sample: the new entry point (256 source rows + 5
    context rows) against the existing one on 256 channels (the K rows predict 261 / 256) and against the existing one on a
    materialised 261-channel concatenation;
  * the loss launch on one production window against the same loss and gradient as a PyTorch autograd expression.

One JSON line per workload; all of them go to profiles/fmr_train.json.

    python3 benchmarks/fmr_train.py [--steps K] [--warmup W] [--batches 1,4]
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
import fmr_cases  # noqa: E402
from cyclegan_train import timed  # noqa: E402
from fv3net_amd import fit, ops  # noqa: E402
from fv3net_amd.cube import _Slice  # noqa: E402

NX, CHANNELS, NTIME = 48, 4, 4


def production_config():
    adam = dict(name="Adam", kwargs=dict(lr=2e-4))
    return fit.FMRNetworkConfig(
        generator_optimizer=adam, discriminator_optimizer=adam,
        generator=dict(n_convolutions=2, n_resnet=6, max_filters=256, strided_kernel_size=4, use_geographic_bias=False, samples_per_day=4),
        discriminator=dict(n_convolutions=3, max_filters=256, strided_kernel_size=4), convolution_type="halo_conv2d",
        identity_loss=dict(loss_type="mae"), target_loss=dict(loss_type="mse"), gan_loss=dict(loss_type="mse"), identity_weight=10.0,
        target_weight=10.0)


def step_times(device, batch, steps, warmup):
    rng = np.random.default_rng(0)
    real = torch.from_numpy(rng.normal(0, 1, (batch, NTIME, 6, CHANNELS, NX, NX)).astype(np.float32)).to(device)
    out = {"workload": f"train_on_batch_b{batch}", "batch": batch, "ntime": NTIME}
    for backend in ("hip", "torch"):
        random.seed(0)
        # (the torch baseline pads with the batched gathers: the tile-by-tile pad that reproduces the reference's bits is slower)
        trainer = production_config().build(CHANNELS, NX, batch, fmr_cases.grid_xyz(NX), fmr_cases.grid_xyz(NX >> 2), seed=0, backend=backend,
                                            device=device, reference_order_gradients=False)
        med, lo, hi = timed(lambda: trainer.train_on_batch(real), steps, warmup)
        out[f"{backend}_ms"], out[f"{backend}_ms_min"], out[f"{backend}_ms_max"] = med, lo, hi
        del trainer
        torch.cuda.empty_cache()
    out["ratio"] = out["hip_ms"] / out["torch_ms"]
    return out


def weight_gradient_times(device, steps, warmup):
    S, n, c, k, c_cell, c_uni = 1, 12, 256, 3, 3, 2
    new = lambda *shape: torch.randn(shape, device=device)   # noqa: E731
    x, dy, dw, db, dw_ctx = new(S, 6, n, n, c), new(S, 6, n, n, c), new(k, k, c, c), new(c), new(k, k, c_cell + c_uni, c)
    cell, uni = new(6, n, n, c_cell), new(c_uni)
    wide = torch.cat([x, cell[None].expand(S, -1, -1, -1, -1), uni.expand(S, 6, n, n, -1)], dim=-1).contiguous()
    dw_wide = new(k, k, c + c_cell + c_uni, c)
    ws = new(ops.cyclegan_train_backward_weight_context_workspace_floats(S, n, c, c_cell, c_uni, c, k))
    cases = {
        "context": lambda: ops.cyclegan_train_backward_weight_context(_Slice(x, c), _Slice(dy, c), cell, uni, dw, dw_ctx, db, S, n, c, c, k,
                                                                      True, ws),
        "plain_256": lambda: ops.cyclegan_train_backward_weight(_Slice(x, c), _Slice(dy, c), dw, db, S, n, c, c, "regular", k, True, ws),
        "plain_261_materialised": lambda: ops.cyclegan_train_backward_weight(_Slice(wide, c + 5), _Slice(dy, c), dw_wide, db, S, n, c + 5, c,
                                                                             "regular", k, True, ws),
    }
    out = {"workload": "backward_weight_261x256_3x3_n12", "k_rows_ratio": (c + 5) / c}
    for name, fn in cases.items():
        med, lo, hi = timed(fn, steps, warmup)
        out[f"{name}_ms"], out[f"{name}_ms_min"], out[f"{name}_ms_max"] = med, lo, hi
    return out


def loss_times(device, steps, warmup):
    """One production window, time-major ``fake`` as the trainer hands it over."""
    W, shape = 1, (NTIME, 1, 6, NX, NX, CHANNELS)
    fake, dgan, dfake = (torch.randn(shape, device=device).transpose(0, 1) for _ in range(3))
    real = torch.randn((W, NTIME, 6, NX, NX, CHANNELS), device=device)
    values, ws = torch.empty(2, dtype=torch.float64, device=device), torch.empty(1 << 12, dtype=torch.float64, device=device)

    def kernel():
        ops.fmr_loss_grad(fake, real, dgan, dfake, "mae", 10.0, "mse", 10.0, values, ws)

    def autograd():
        leaf = fake.detach().requires_grad_()
        loss = 10.0 * torch.nn.functional.l1_loss(leaf[:, 0], real[:, 0]) + 10.0 * torch.nn.functional.mse_loss(leaf[:, 1:], real[:, 1:])
        return torch.autograd.grad(loss, leaf)[0] + dgan

    out = {"workload": "window_loss_c48_4x4", "elements": int(real.numel())}
    for name, fn in (("kernel", kernel), ("autograd", autograd)):
        med, lo, hi = timed(fn, steps, warmup)
        out[f"{name}_ms"], out[f"{name}_ms_min"], out[f"{name}_ms_max"] = med, lo, hi
    out["ratio"] = out["kernel_ms"] / out["autograd_ms"]
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--steps", type=int, default=3)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--batches", default="1,4")
    args = parser.parse_args()
    device = torch.device("cuda:0")
    results = [weight_gradient_times(device, 50, 10), loss_times(device, 50, 10)]
    for r in results:
        print(json.dumps(r), flush=True)
    for batch in (int(b) for b in args.batches.split(",")):
        results.append(step_times(device, batch, args.steps, args.warmup))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "fmr_train.json"), "w") as f:
        json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
