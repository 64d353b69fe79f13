"""The precipitative predictor (fit.HipPrecipitativeModel) on three column counts, state resident on the
device: the network launch, the closure launch (fv3hip_precip_closure) and the whole ``predict``, next to the same closure
written as a PyTorch-ROCm expression on the same arrays in the same run.

  network   T, q, delp (79 levels each) + physics_precip -> 16 -> 16 -> 3 x 79 (the reference's defaults, depth 3)
  columns   C48 (13 824), one C384 tile (147 456), the C384 cube (884 736)
  state     float64 and float32

Every figure is the median over ``--windows`` windows of ``--steps`` calls between two device events, after ``--warmup`` calls,
with the lowest and highest window beside it.  Two kinds of window: "eager" is a Python loop of calls (what a caller sees; for
small column counts it is bound by the host's enqueue rate, not by the kernels) and "graph" is a captured chain of the same
launches replayed without Python between them (what the device needs per launch, kernel boundary included).  The closure's
bytes are the algorithmic ones, nz * n * (3*4 + 2*4 + sizeof(delp)) + n * (sizeof(pp) + 4) with coupling, over the graph time.
One JSON line per (columns, dtype).

    python3 benchmarks/precipitative_predict.py [--steps K] [--warmup W] [--windows N] [--columns 13824,147456]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fv3net_amd import fit, ops  # noqa: E402
from fv3net_amd.fit.precipitative import CPD, DELP_NAME, GRAVITY, LV, PHYS_PRECIP_NAME  # noqa: E402
from fv3net_amd.graphs import GraphedCall  # noqa: E402
from fv3net_amd.xr_compat import DataArray, Dataset  # noqa: E402

NZ, WIDTH = 79, 16
HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.29   # HBM3E spec; measured float4 copy (MI355X_MICROARCH "HBM3E peak BW")
NAMES_IN = ["air_temperature", "specific_humidity", DELP_NAME, PHYS_PRECIP_NAME]
NAMES_OUT = ["dQ1", "dQ2", "total_precipitation_rate"]


def build_model(rng):
    nfeat = [NZ, NZ, NZ, 1]
    fan, hk, hb = sum(nfeat), [], []
    for _ in range(2):
        hk.append((rng.normal(0, 1, (fan, WIDTH)) / np.sqrt(fan)).astype(np.float32))
        hb.append(rng.normal(0, 0.1, WIDTH).astype(np.float32))
        fan = WIDTH
    centers = [np.full(NZ, 250.0), np.full(NZ, 0.01), np.full(NZ, 900.0), np.full(1, 5e-5)]
    scales = [np.full(NZ, 29.0), np.full(NZ, 0.0058), np.full(NZ, 346.0), np.full(1, 2.9e-5)]
    spec = fit.precipitative_spec_from_arrays(
        NAMES_IN, centers, scales, hk, hb,
        [(rng.normal(0, 1, (WIDTH, NZ)) / np.sqrt(WIDTH)).astype(np.float32) for _ in range(3)],
        [rng.normal(0, 0.1, NZ).astype(np.float32) for _ in range(3)],
        [np.zeros(NZ), np.zeros(NZ)], [np.full(NZ, 1e-4), np.full(NZ, 1e-7)])
    return fit.HipPrecipitativeModel(NAMES_IN, NAMES_OUT, spec)


def windows_ms(run_window, calls_per_window, windows):
    """(median, min, max) milliseconds per call over ``windows`` windows, each between two device events."""
    per_call = []
    for _ in range(windows):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run_window()
        stop.record()
        stop.synchronize()
        per_call.append(start.elapsed_time(stop) / calls_per_window)
    return [round(x, 5) for x in (statistics.median(per_call), min(per_call), max(per_call))]


def time_both(fn, steps, warmup, windows, chain):
    """``fn`` timed as an eager loop of ``steps`` calls and as a captured chain of ``chain`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()

    def loop():
        for _ in range(steps):
            fn()

    eager = windows_ms(loop, steps, windows)

    def chained():
        for _ in range(chain):
            fn()

    call = GraphedCall(chained, warmup=1)
    call.replay()
    torch.cuda.synchronize()
    graph = windows_ms(call.replay, chain, windows)
    del call
    return {"eager_ms": eager, "graph_ms": graph}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--columns", default="13824,147456,884736")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    model = build_model(rng)
    c_heat, c_g = float(np.float32(-LV / CPD)), float(np.float32(-1.0 / GRAVITY))
    for n in [int(c) for c in args.columns.split(",")]:
        chain = max(4, min(50, 4_000_000 // n))   # (a captured chain holds every call's new arrays)
        for dtype in (torch.float64, torch.float32):
            gen = torch.Generator(device=dev).manual_seed(n)
            uniform = lambda lo, hi, *shape: (torch.rand(*shape, generator=gen, device=dev, dtype=torch.float64) * (hi - lo) + lo).to(dtype)
            state = {"air_temperature": uniform(200, 300, NZ, n), "specific_humidity": uniform(0, 0.02, NZ, n),
                     DELP_NAME: uniform(300, 1500, NZ, n), PHYS_PRECIP_NAME: uniform(0, 1e-4, n)}
            ds = Dataset({k: DataArray(v, dims=["z", "x"] if v.dim() == 2 else ["x"]) for k, v in state.items()})
            sources = {k: (v if v.dim() == 2 else v.unsqueeze(0)) for k, v in state.items()}
            delp, pp = state[DELP_NAME], state[PHYS_PRECIP_NAME]
            heads = model.model.predict(sources, layout="feature_sample")
            network_variant = model.model.last_variant
            t_res, q_res, cp = (heads[k] for k in ("dQ1", "dQ2", "q_tendency_due_to_precip"))

            def torch_closure():
                dq1 = torch.add(t_res, cp, alpha=c_heat)
                dq2 = torch.add(q_res, cp)
                integral = torch.mul(cp, delp.to(torch.float32)).sum(dim=0)
                return dq1, dq2, torch.add(pp.to(torch.float32), integral, alpha=c_g)

            # the two closures agree (the torch sum has its own order: close, not bitwise)
            ours = ops.precip_closure(t_res, q_res, cp, delp, pp, couple=True, in_place=False)
            theirs = torch_closure()
            for a, b, name in zip(ours, theirs, NAMES_OUT):
                scale = float(b.abs().max())
                assert float((a - b).abs().max()) <= 1e-5 * scale, (name, float((a - b).abs().max()), scale)

            row = {"columns": n, "state_dtype": str(dtype).replace("torch.", ""), "network_variant": network_variant,
                   "steps": args.steps, "windows": args.windows, "graph_chain": chain}
            row["network"] = time_both(lambda: model.model.predict(sources, layout="feature_sample", out=heads), args.steps,
                                       args.warmup, args.windows, chain)
            # out of place, so that the heads keep their values over the repeats (the same bytes move as in place)
            row["closure"] = time_both(lambda: ops.precip_closure(t_res, q_res, cp, delp, pp, couple=True, in_place=False),
                                       args.steps, args.warmup, args.windows, chain)
            row["closure_in_torch"] = time_both(torch_closure, args.steps, args.warmup, args.windows, chain)
            row["predict"] = time_both(lambda: model.predict(ds), args.steps, args.warmup, args.windows, max(4, chain // 4))
            size = delp.element_size()
            nbytes = NZ * n * (3 * 4 + 2 * 4 + size) + n * (size + 4)
            ms = row["closure"]["graph_ms"][0]
            row["closure_bytes"] = nbytes
            row["closure_TB_per_s"] = round(nbytes / ms / 1e9, 3)
            row["closure_share_of_hbm_peak"] = round(nbytes / ms / 1e9 / HBM_PEAK_TBS, 3)
            row["closure_share_of_hbm_copy_rate"] = round(nbytes / ms / 1e9 / HBM_COPY_TBS, 3)
            row["closure_over_network"] = round(ms / row["network"]["graph_ms"][0], 3)
            row["closure_over_torch"] = round(ms / row["closure_in_torch"]["graph_ms"][0], 3)
            row["columns_per_s_predict_graph"] = round(n / row["predict"]["graph_ms"][0] * 1e3)
            print(json.dumps(row), flush=True)
            del state, ds, sources, heads, t_res, q_res, cp, ours, theirs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
