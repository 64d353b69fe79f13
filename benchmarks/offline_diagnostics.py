"""Offline diagnostics on the device against copying the predictions to the host.

One run, at C384 with 79 levels in float32 -- dQ1 and dQ2 (3-D) and two 2-D variables, prediction and target resident on the
device -- times and prints as one JSON line:

  (a) ``OfflineDiagnostics.update`` of one snapshot: the whole call (host clock around a device synchronise, median of
      ``--steps`` after ``--warmup``) and, from one more update with device events around every ``ops`` call, its split by call;
  (b) copying the same prediction arrays to pinned host memory (what ``fit.SnapshotStream`` does with every output);
  (c) the streaming read rate of benchmarks/hbm_bandwidth.py (``torch.sum`` over a large float32 array).

The feature has a point where (a) < (b); the line says whether that holds.  Every ``group_sums`` pass is listed with the
fraction of (c) it reaches on its algorithmic bytes -- one read of ``a`` and ``b`` (559 MB for a 3-D float32 variable);
recorded, not gated.

    python benchmarks/offline_diagnostics.py [--steps 5] [--warmup 2] [--c 384] [--nz 79]
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fv3net_amd import ops  # noqa: E402
from fv3net_amd.diagnostics import OfflineDiagnostics, offline  # noqa: E402
from fv3net_amd.xr_compat import DataArray, Dataset  # noqa: E402

TIMED_OPS = ("group_plan", "group_sums", "interpolate_2d", "pressure_at_midpoint_log", "histogram_counts", "histogram2d_counts", "ew",
             "column_sum")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--c", type=int, default=384)
    ap.add_argument("--nz", type=int, default=79)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup not negative")
    if not torch.cuda.is_available():
        raise SystemExit("this benchmark needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    n, nz = args.c, args.nz
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *shape: torch.rand(shape, device=dev, generator=gen)  # noqa: E731

    rng = np.random.default_rng(0)
    horizontal = ["tile", "y", "x"]
    grid = Dataset({
        "lat": DataArray(np.degrees(np.arcsin(rng.uniform(-1, 1, (6, n, n)))), dims=horizontal),
        "lon": DataArray(rng.uniform(0, 360, (6, n, n)), dims=horizontal),
        "area": DataArray(rng.uniform(0.5, 1.5, (6, n, n)).astype(np.float32), dims=horizontal),
        "land_sea_mask": DataArray(rng.choice([0.0, 1.0, 2.0], size=(6, n, n), p=[0.6, 0.3, 0.1]), dims=horizontal),
    })
    diags = OfflineDiagnostics(grid)
    d3, d2 = ["time", "z"] + horizontal, ["time"] + horizontal
    when = {"time": [datetime.datetime(2016, 8, 1, 3)]}
    target = Dataset({"dQ1": DataArray(rand(1, nz, 6, n, n) - 0.5, dims=d3), "dQ2": DataArray(rand(1, nz, 6, n, n) - 0.5, dims=d3),
                      "Q2": DataArray(rand(1, nz, 6, n, n) - 0.5, dims=d3),
                      "water_vapor_path": DataArray(80 * rand(1, 6, n, n), dims=d2),
                      "column_integrated_Q2": DataArray(100 * rand(1, 6, n, n) - 80, dims=d2)}, coords=when)
    names = ["dQ1", "dQ2", "water_vapor_path", "column_integrated_Q2"]
    prediction = Dataset({k: DataArray(target[k].data + 0.1 * rand(*target[k].shape), dims=target[k].dims) for k in names}, coords=when)
    delp = DataArray(100000.0 / nz * (0.5 + rand(1, nz, 6, n, n)), dims=d3)

    def timed_update():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        diags.update(prediction, target, delp)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(args.warmup):
        timed_update()
    update_ms = [timed_update() for _ in range(args.steps)]

    # (a) split by call: one more update with device events around every ops call (the events add host time: the sum of the
    # parts is device time, the whole above is what a user waits for)
    records = []
    originals = {name: getattr(ops, name) for name in TIMED_OPS}

    def wrap(name, fn):
        def timed(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            records.append((name, a, e0, e1))
            return out
        return timed

    for name, fn in originals.items():
        setattr(ops, name, wrap(name, fn))
    try:
        diags.update(prediction, target, delp)
        torch.cuda.synchronize(dev)
    finally:
        for name, fn in originals.items():
            setattr(ops, name, fn)
    by_call, passes = {}, []
    for name, a, e0, e1 in records:
        ms = e0.elapsed_time(e1)
        by_call[name] = by_call.get(name, 0.0) + ms
        if name == "group_sums":
            field, plan = a[0], a[3]
            nbytes = 2 * field.numel() * field.element_size()
            passes.append({"levels": int(field.shape[1]), "dtype": str(field.dtype).replace("torch.", ""), "groups": plan.n_groups,
                           "weighted": a[2] is not None, "ms": round(ms, 4), "algorithmic_MB": round(nbytes / 1e6, 1),
                           "GBps": round(nbytes / ms / 1e6, 1)})

    # (b) the same prediction arrays to pinned host memory
    src = [prediction[k].data for k in names]
    pinned = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in src]

    def copy_out():
        for p, t in zip(pinned, src):
            p.copy_(t, non_blocking=True)

    def timed_events(fn, reps):
        fn()
        torch.cuda.synchronize(dev)
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            out.append(e0.elapsed_time(e1))
        return out

    copy_ms = timed_events(copy_out, args.steps)
    copy_bytes = sum(t.numel() * t.element_size() for t in src)

    # (c) streaming read rate, as benchmarks/hbm_bandwidth.py measures it
    big = torch.rand((6, nz, 4 * n, n), device=dev)
    read_ms = statistics.median(timed_events(lambda: big.sum(), 10))
    read_gbps = big.numel() * 4 / read_ms / 1e6
    for p in passes:
        p["fraction_of_read_rate"] = round(p["GBps"] / read_gbps, 3)

    a_ms, b_ms = statistics.median(update_ms), statistics.median(copy_ms)
    print(json.dumps({
        "benchmark": "offline_diagnostics", "grid": f"C{n}", "levels": nz, "dtype": "float32", "variables": names,
        "update_ms": round(a_ms, 3), "update_ms_all": [round(v, 3) for v in update_ms],
        "update_device_ms_by_call": {k: round(v, 3) for k, v in sorted(by_call.items(), key=lambda kv: -kv[1])},
        "group_sums_passes": passes,
        "copy_to_pinned_host_ms": round(b_ms, 3), "copy_to_pinned_host_ms_all": [round(v, 3) for v in copy_ms],
        "copy_GBps": round(copy_bytes / b_ms / 1e6, 1), "copy_MB": round(copy_bytes / 1e6, 1),
        "streaming_read_GBps": round(read_gbps, 1),
        "update_faster_than_copy": bool(a_ms < b_ms),
        "outputs": len(list(diags.compute())), "diagnostic_names": len(offline.DIAGNOSTIC_NAMES),
    }))


if __name__ == "__main__":
    main()
