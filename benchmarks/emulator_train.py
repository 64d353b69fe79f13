"""One training step of the microphysics emulators: ``fv3net_amd.train.EmulatorTrainer.step`` eager and as a
replayed HIP graph, next to the torch backend's step (torch expressions, autograd, ``torch.optim.Adam``: what
``fit.train_transformed_model(backend="torch")`` runs) on the same device, the same resident data and the same minibatch, in
alternating windows of one run, timed with device events after warm-up.

  zc_b512      the Zhao-Carr configuration of projects/microphysics/train/dense.yaml: 9 x 79 inputs -> 256 -> 256 -> 1 + 5 x 79, six
               loss and five metric variables (the ``after`` fields of the five Differences), batch 512
  zc_b8192     the same, batch 8192
  classifier   the gscond classifier of gscond-classifier.yaml: 13 inputs, dense-local, 256 x 2, 4 channels, batch 512 columns x
               79 levels

and the loss launch alone (``ops.train_emulator_loss_grad``: the kernel and its finish kernel) next to the same loss and gradient
as a PyTorch autograd expression on the same head outputs.  The data is synthetic; the shapes are the configurations'.  One JSON
line per configuration.

    python3 benchmarks/emulator_train.py [--configs zc_b512,zc_b8192,classifier] [--windows N] [--steps K] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.dense_train import alternating  # noqa: E402
from fv3net_amd import fit, ops  # noqa: E402
from fv3net_amd.fit import emulator_train as fe  # noqa: E402

NZ = 79
CONFIGS = {"zc_b512": ("dense", 512, 16384), "zc_b8192": ("dense", 8192, 16384), "classifier": ("dense-local", 512, 2048)}
LOGS = [("log_cloud_input", "cloud_water_mixing_ratio_input", 1e-10), ("log_humidity_input", "specific_humidity_input", 1e-8),
        ("log_humidity_after_last_gscond", "specific_humidity_after_last_gscond", 1e-8)]
DIFFERENCES = [("temperature_gscond_difference", "air_temperature_input", "air_temperature_after_gscond"),
               ("humidity_gscond_difference", "specific_humidity_input", "specific_humidity_after_gscond"),
               ("cloud_precpd_difference", "cloud_water_mixing_ratio_input", "cloud_water_mixing_ratio_after_precpd"),
               ("temperature_precpd_difference", "air_temperature_input", "air_temperature_after_precpd"),
               ("humidity_precpd_difference", "specific_humidity_input", "specific_humidity_after_precpd")]
INPUTS = ["air_temperature_input", "specific_humidity_input", "cloud_water_mixing_ratio_input", "log_cloud_input", "log_humidity_input",
          "pressure_thickness_of_atmospheric_layer", "air_temperature_after_last_gscond", "specific_humidity_after_last_gscond",
          "log_humidity_after_last_gscond"]


def config(arch, batch):
    transforms = [{"to": to, "source": src, "transform": {"epsilon": eps}} for to, src, eps in LOGS]
    model = {"architecture": {"name": arch, "kwargs": {"width": 256, "depth": 2}}, "input_variables": list(INPUTS),
             "normalize_default": {"center": "per_feature", "scale": "all"}}
    if arch == "dense":
        transforms += [{"to": to, "before": b, "after": a} for to, b, a in DIFFERENCES]
        outs = ["total_precipitation"] + [d[0] for d in DIFFERENCES]
        model["direct_out_variables"] = outs
        loss = {"loss_variables": outs, "metric_variables": [d[2] for d in DIFFERENCES]}
    else:
        model["input_variables"] += ["air_pressure", "surface_air_pressure", "surface_air_pressure_after_last_gscond", "relative_humidity"]
        model["architecture"]["output_channels"] = {"gscond_classes": 4}
        model["unscaled_outputs"] = ["gscond_classes"]
        loss = {"logit_variables": ["gscond_classes"], "weights": {"gscond_classes": 1.0}}
    loss["optimizer"] = {"name": "Adam", "kwargs": {"learning_rate": 1e-4}}
    return {"batch_size": batch, "epochs": 1, "tensor_transform": transforms, "loss": loss, "model": model, "use_wandb": False}


def state(rows, rng):
    f32 = np.float32
    z = np.linspace(0, 1, NZ)
    t = (220 + 70 * z + rng.normal(0, 5, (rows, NZ))).astype(f32)
    q = (1e-3 * np.exp(3 * z) * rng.uniform(0.2, 1.5, (rows, NZ))).astype(f32)
    qc = np.where(rng.uniform(size=(rows, NZ)) < 0.4, 0.0, 1e-4 * rng.uniform(0, 1, (rows, NZ))).astype(f32)
    s = {"air_temperature_input": t, "specific_humidity_input": q, "cloud_water_mixing_ratio_input": qc,
         "pressure_thickness_of_atmospheric_layer": (1000 + 200 * rng.uniform(-1, 1, (rows, NZ))).astype(f32),
         "air_temperature_after_last_gscond": (t + rng.normal(0, 0.1, t.shape)).astype(f32),
         "specific_humidity_after_last_gscond": (q * rng.uniform(0.9, 1.1, q.shape)).astype(f32),
         "air_pressure": (1e5 * (0.01 + z) * rng.uniform(0.97, 1.03, (rows, 1))).astype(f32), "surface_air_pressure": (1e5 + 2e3 * rng.normal(0, 1, rows)).astype(f32),
         "surface_air_pressure_after_last_gscond": (1e5 + 2e3 * rng.normal(0, 1, rows)).astype(f32),
         "relative_humidity": rng.uniform(0, 1.1, (rows, NZ)).astype(f32),
         "total_precipitation": rng.uniform(0, 1e-3, rows).astype(f32),
         "gscond_classes": np.eye(4, dtype=f32)[rng.integers(0, 4, (rows, NZ))]}
    for _, before, after in DIFFERENCES:
        scale = 0.5 if "temperature" in before else 1e-5
        s[after] = (s[before] + scale * rng.normal(0, 1, (rows, NZ))).astype(f32)
    return s


def build(name, dev, rng):
    arch, batch, rows = CONFIGS[name]
    hp = fit.TransformedParameters.from_dict(config(arch, batch))
    prep = fe._prepare(hp, [state(rows, rng)], None)
    trainer = fe.emulator_trainer(hp, prep, dev)
    L = prep.levels
    ws = [torch.from_numpy(k.copy()).to(dev).requires_grad_() for k in prep.kernels]
    bs = [torch.from_numpy(b.copy()).to(dev).requires_grad_() for b in prep.biases]
    opt = torch.optim.Adam(ws + bs, lr=prep.adam["learning_rate"], eps=prep.adam["epsilon"])
    xin3 = trainer.xin.view(-1, L, trainer.xin.shape[1])
    heads = trainer.heads   # the device tensors the kernel reads

    def loss_expression(raw, idx):
        return fe.emulator_loss_torch(raw, heads, idx, L)[0]

    def torch_step(idx):
        h = xin3[idx].reshape(-1, xin3.shape[2])
        for l, (w, b) in enumerate(zip(ws, bs)):
            h = h @ w + b
            if l + 1 < len(ws):
                h = torch.relu(h)
        out = loss_expression(h, idx)
        opt.zero_grad()
        out.backward()
        opt.step()

    return prep, trainer, torch_step, loss_expression


def run(name, windows, steps, dev):
    arch, batch, rows = CONFIGS[name]
    rng = np.random.default_rng(0)
    prep, trainer, torch_step, loss_expression = build(name, dev, rng)
    idx = torch.randperm(rows, generator=torch.Generator().manual_seed(0))[:batch].to(dev)
    graph = trainer.capture(idx)
    eager, replay, library = alternating([lambda: trainer.step(idx), graph.replay, lambda: torch_step(idx)], windows, steps)
    sizes = [k.shape[0] for k in prep.kernels] + [prep.kernels[-1].shape[1]]
    result = {"config": name, "architecture": arch, "sizes": sizes, "batch": batch, "levels": prep.levels, "heads": len(prep.heads),
              "slots": len(prep.slot_names), "hip_eager": eager, "hip_graph": replay, "torch": library,
              "hip_eager_over_torch": eager["median_ms"] / library["median_ms"],
              "hip_graph_over_torch": replay["median_ms"] / library["median_ms"], "loss_after": trainer.loss()}

    # the loss launch alone, on the head outputs the last step left
    raw = trainer.loss_stage(idx)[0].clone().requires_grad_(True)

    def hip_loss():
        trainer.loss_stage(idx)

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
                   "loss_launch_max_difference_over_max_gradient": float((trainer.loss_stage(idx)[1] - raw.grad).abs().max()) / scale})
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="zc_b512,zc_b8192,classifier")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("benchmarks/emulator_train.py needs a GPU: a CPU run gives no time")
    dev = torch.device("cuda:0")
    ops._require_device(torch.empty(1, device=dev))
    lines = [run(name, args.windows, args.steps, dev) for name in args.configs.split(",") if name]
    for line in lines:
        for key in ("loss_after", "loss_launch_max_difference_over_max_gradient"):
            if not np.isfinite(line[key]):
                raise SystemExit(f"{line['config']}: {key} is {line[key]}: the benchmark's data or the step is broken")
        print(json.dumps(line, allow_nan=False), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(line, allow_nan=False) + "\n" for line in lines)


if __name__ == "__main__":
    main()
