"""Graph U-Net autoregressor rollouts (fv3hip_graph_sage / _pool2 / _up2 through ``GraphModel``), timed with HIP events after
warm-up, next to the plain-torch twin (``fit.graph.GraphUNetTwin``: an index gather, a mean and ``nn.Linear`` per layer) on the
same device in the same run, and the float32 twin on the CPU.  dgl exists on neither side.

  G1  the C48 cube, T + q (79 levels each) + two surface fields = 160 features, min_filters 64, depth 2: an 8-step rollout of
      1 and of 8 windows
  G2  the same state with the reference's defaults (min_filters 4, depth 1): the 8-step rollout eager and as a GraphedCall replay
  G3  the C384 cube, min_filters 32, depth 3: one step

Times are per step: the median of five windows of back-to-back calls (minimum and maximum beside it).  Beside them the derived
floors: flops_per_node x nodes over the fp32 matrix peak, and the bytes of state in, state out and every intermediate written
and read once over the HBM peak.  One JSON line per workload; all of them are also written to profiles/graph_rollout.json.
``--quick NAME`` runs the HIP path of one workload only (for profiler runs).

    python3 benchmarks/graph_rollout.py [--quick G1] [--steps K] [--warmup W]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fv3net_amd.fit.graph import twin_from_spec  # noqa: E402
from fv3net_amd.graph import GraphModel, GraphUNetSpec, GraphVariable, SageLayer, UpLayer, layer_plan  # noqa: E402
from fv3net_amd.graphs import GraphedCall  # noqa: E402

FP32_MATRIX_PEAK_TFLOPS = 157.3   # MI355X, v_mfma_f32_32x32x2_f32: 256 FLOP / clk / CU x 256 CUs x 2.4 GHz
HBM_PEAK_TBS = 8.0                # HBM3E spec (MI355X_MICROARCH "HBM3E peak BW"; a float4 copy reaches 6.29)
VARIABLES = {"T": 79, "q": 79, "ps": 1, "ts": 1}


def make_spec(rng, depth, min_filters):
    vs = [GraphVariable(name, nf, rng.normal(0, 10, nf), rng.uniform(0.5, 2, nf)) for name, nf in VARIABLES.items()]
    layers = {}
    for name, kind, ci, co, _ in layer_plan(depth, sum(VARIABLES.values()), min_filters):
        if kind == "sage":
            draw = lambda: (rng.normal(0, 1, (ci, co)) / np.sqrt(2 * ci)).astype(np.float32)
            layers[name] = SageLayer(draw(), draw(), rng.normal(0, 0.1, co).astype(np.float32))
        else:
            layers[name] = UpLayer((rng.normal(0, 1, (ci, 2, 2, co)) / np.sqrt(ci)).astype(np.float32), rng.normal(0, 0.1, co).astype(np.float32))
    return GraphUNetSpec(vs, depth, min_filters, "relu", layers)


def floor_bytes_per_node(spec):
    """float32 bytes per full-resolution cell of one step: the state read and written, and every intermediate (layer outputs,
    the pooled arrays) written once and read once."""
    F = spec.n_features
    total = 2.0 * F
    for name, kind, ci, co, k in spec.plan:
        if name != "last":
            total += 2.0 * co / 4.0 ** k
    for k in range(spec.depth):   # the pooled copy of conv1's output, at level k + 1
        total += 2.0 * 2 * spec.min_filters * 2 ** k / 4.0 ** (k + 1)
    return 4.0 * total


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


def auto_steps(fn, asked):
    if asked > 0:
        return asked
    return max(3, min(500, int(200.0 / timed(fn, 2, 1, repeats=1)[0])))   # windows of about 0.2 s


def twin_rollout(twin, state, timesteps):
    out = torch.empty((state.shape[0], timesteps + 1) + tuple(state.shape[1:]), dtype=state.dtype, device=state.device)
    out[:, 0] = state
    with torch.no_grad():
        for i in range(timesteps):
            out[:, i + 1] = twin(out[:, i])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="calls per timed window (0: enough for about 0.2 s)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", default=None, help="G1, G2 or G3: the HIP path of that workload only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_rollout.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    gen = torch.Generator(device=dev).manual_seed(0)
    # (workload, n, depth, min_filters, windows, timesteps, replay too)
    plans = [("G1_c48_m64_d2_1window", 48, 2, 64, 1, 8, False), ("G1_c48_m64_d2_8windows", 48, 2, 64, 8, 8, False),
             ("G2_c48_m4_d1_defaults", 48, 1, 4, 1, 8, True), ("G3_c384_m32_d3_one_step", 384, 3, 32, 1, 1, False)]
    if args.quick:
        plans = [p for p in plans if p[0].startswith(args.quick)][:1]
    rows = []
    for name, n, depth, m, windows, timesteps, replay in plans:
        spec = make_spec(rng, depth, m)
        model = GraphModel(spec, device=dev)
        state = torch.randn((windows, 6, n, n, spec.n_features), device=dev, generator=gen)
        nodes = windows * 6 * n * n
        call = lambda: model.rollout(state, timesteps)
        steps = auto_steps(call, args.steps)
        ms, ms_min, ms_max = (t / timesteps for t in timed(call, steps, args.warmup))
        row = {"workload": name, "nodes": nodes, "features": spec.n_features, "min_filters": m, "depth": depth, "timesteps": timesteps,
               "launches_per_step": len(spec.plan) + depth, "flop_per_node": spec.flops_per_node(), "calls_per_window": steps,
               "hip_ms_per_step": round(ms, 4), "hip_ms_per_step_min_max_of_5_windows": [round(ms_min, 4), round(ms_max, 4)],
               "hip_tflops": round(nodes * spec.flops_per_node() / ms / 1e9, 2),
               "floor_ms_fp32_matrix_peak": round(nodes * spec.flops_per_node() / FP32_MATRIX_PEAK_TFLOPS / 1e9, 4),
               "floor_bytes_per_node": floor_bytes_per_node(spec),
               "floor_ms_hbm_peak": round(nodes * floor_bytes_per_node(spec) / HBM_PEAK_TBS / 1e9, 4)}
        if replay:
            graphed = GraphedCall(call, device=dev)
            r, r_min, r_max = (t / timesteps for t in timed(graphed.replay, steps, args.warmup))
            row["hip_replay_ms_per_step"] = round(r, 4)
            row["hip_replay_ms_per_step_min_max_of_5_windows"] = [round(r_min, 4), round(r_max, 4)]
            del graphed
        if not args.quick:
            twin = twin_from_spec(spec, torch.float32, dev)
            tcall = lambda: twin_rollout(twin, state, timesteps)
            t, t_min, t_max = (v / timesteps for v in timed(tcall, auto_steps(tcall, args.steps), args.warmup))
            row["torch_twin_ms_per_step"] = round(t, 4)
            row["torch_twin_ms_per_step_min_max_of_5_windows"] = [round(t_min, 4), round(t_max, 4)]
            row["hip_over_torch_twin"] = round(ms / t, 3)
            if replay:
                row["hip_replay_over_torch_twin_eager"] = round(row["hip_replay_ms_per_step"] / t, 3)
            got, want = model.step(state[:1]), twin(state[:1]).detach()
            row["max_abs_difference_to_twin_one_step"] = float((got - want).abs().max())
            del twin, got, want
            cpu = twin_from_spec(spec, torch.float32, "cpu")
            x = state[:1].cpu()
            with torch.no_grad():
                cpu(x)
                t0 = time.perf_counter()
                cpu(x)
            row["torch_cpu_f32_ms_per_step_one_window"] = round((time.perf_counter() - t0) * 1e3, 1)
        del model, state
        torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if not args.quick:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
