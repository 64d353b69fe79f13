"""Cycle stamps of mlp_fused_kernel on bench.py's own model at full size (build.sh first).

usage: run.py PHASE [--lib-dir DIR] [--out FILE.json]
  PHASE is the per-slot phase the library was built for (MLP_STAMP_PHASE in mlp.hip):
    0 / 2  layer-1 chunks by the flavour of the input tile they prepare (plain / fast log)
    3      the 8-slot layer-1 chunk behind a log block whose last chunk is at most half full
    4      the 13-slot first plain chunk, where the plain block's partial chunk is its first
    10     hidden chunks        20  output chunks
One process per phase (the library is chosen when it is loaded); both epilogue flavours, plain and residual, run in it.
Prints, and merges into FILE.json under "phase_<PHASE>", per flavour: the per-phase cycle sums per tile (st_acc[0..3]:
layer 1, hidden, output, last epilogue) and the per-slot means sl_acc[0..15] / sl_acc[16] with the chunk count.
A whole table:  for p in 0 2 3 4 10 20; do timeout -k 10 120 python benchmarks/mlp_stamps/run.py $p --out t.json || break; done
"""
import argparse
import ctypes
import json
import os
import sys

here = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("phase", type=int)
ap.add_argument("--lib-dir", default=os.path.join(here, "build"))
ap.add_argument("--out")
args = ap.parse_args()
os.environ["FV3HIP_LIBRARY"] = os.path.join(os.path.abspath(args.lib_dir), f"libfv3hip_stamps_{args.phase}.so")
sys.path.insert(0, os.path.join(here, "..", ".."))

import numpy as np
import torch

import bench
from fv3net_amd import _lib, ops
from fv3net_amd.mlp import MlpModel

dev = torch.device("cuda:0")
lib = _lib.load()
lib.fv3hip_diag_set_mlp_stamps.argtypes = [ctypes.c_void_p]
N = 6 * 384 * 384
src = bench.zc_inputs_device(dev, N, seed=1)
n_cu = int(ops.device_info()["compute_units"])
grid = min(N // 128, n_cu)
tiles = N / 128 / grid  # tiles per workgroup
result = {"columns": N, "workgroups": grid, "tiles_per_workgroup": tiles}
for flavour, residuals in (("plain", False), ("residual", True)):
    model = MlpModel(bench.zc_spec(0, residuals=residuals), device=dev)
    lib.fv3hip_diag_set_mlp_stamps(None)
    for _ in range(6):
        model.predict(src)
    torch.cuda.synchronize()
    t = ops.HipTimer()
    t.start(dev)
    for _ in range(5):
        model.predict(src)
    t.stop(dev)
    ms = t.elapsed_ms() / 5
    stamps = torch.zeros((grid * 4, 32), dtype=torch.int64, device=dev)
    lib.fv3hip_diag_set_mlp_stamps(ctypes.c_void_p(stamps.data_ptr()))
    model.predict(src)
    torch.cuda.synchronize()
    lib.fv3hip_diag_set_mlp_stamps(None)
    s = stamps.cpu().numpy().astype(np.float64)
    per_tile = (s[:, :4].mean(0) / tiles).round(1).tolist()
    chunks = s[:, 24].mean()
    slots = (s[:, 8:24].sum(0) / max(s[:, 24].sum(), 1.0)).round(1).tolist()
    entry = {
        "variant": model.last_variant,
        "stamped_build_ms": round(ms, 4),
        "cycles_per_tile": dict(zip(("layer1", "hidden", "output", "last_epilogue"), per_tile)),
        "cycles_per_tile_sum": round(sum(per_tile), 1),
        "chunks_per_tile": round(chunks / tiles, 3),
        "slot_cycles_mean": slots,
        "chunk_cycles_mean": round(sum(slots), 1),
    }
    result[flavour] = entry
    print(flavour, json.dumps(entry))
    del model
if args.out:
    table = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            table = json.load(f)
    table[f"phase_{args.phase}"] = result
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
