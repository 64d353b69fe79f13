"""The FMR recurrent generator at the reference's production configuration (projects/fmr/training.yaml: C48 faces, four 2-D
state variables, n_convolutions 2, n_resnet 6, max_filters 256, halo_conv2d, samples_per_day 4; evaluate.py rolls out 16 times),
timed with HIP events after warm-up.

(a) ``step_layer``: the first convolution of a ResNet block alone, 256 + 5 -> 256, 3 x 3, 12 x 12 faces, 1 and 100 samples,
    through ``fv3hip_cyclegan_conv_context``; beside it, in the same run, the same launch without context (the existing kernel;
    the K rows predict 147 / 144) and ``fv3hip_cyclegan_conv`` on a materialised 261-channel concatenation (its scalar loader).
(b) ``rollout``: ``RecurrentGeneratorModel.forward`` on a resident state, 16 times, 1 and 8 windows; beside it the plain-torch
    twin (``fit.RecurrentGeneratorTwin``) on the same device in the same run and, for one window, the float32 twin on the CPU.
    ``by_part_ms``: one rollout with a HIP event pair around every launch, summed per part (encode, step, decode) and per layer
    kind; ``sum_of_launches_ms`` against ``hip_forward_ms`` shows how much of the eager wall time the kernels fill.

Times are per call: the median of five windows of back-to-back calls (minimum and maximum beside it).  TFLOP/s are algorithmic
and exact fp32 (2 x taps x c_in x c_out per output cell, context channels included).  One JSON line per row; all of them are
also written to profiles/fmr_rollout.json.

    python3 benchmarks/fmr_rollout.py [--steps K] [--warmup W] [--only step_layer|rollout]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))
import fmr_cases  # noqa: E402
from cyclegan_predict import FP32_MATRIX_PEAK_TFLOPS, auto_steps, timed  # noqa: E402
from fv3net_amd import _lib, fit  # noqa: E402
from fv3net_amd.fit.fmr import recurrent_twin_from_spec  # noqa: E402
from fv3net_amd.ops import _stream  # noqa: E402

NX, N_CONVOLUTIONS, N_RESNET, MAX_FILTERS, SAMPLES_PER_DAY, NTIME = 48, 2, 6, 256, 4, 16
VARIABLES = {"h500": 1, "PRATEsfc": 1, "TMPsfc": 1, "PRESsfc": 1}


def span(times):
    ms, lo, hi = times
    return {"ms": round(ms, 4), "ms_min_max_of_5_windows": [round(lo, 4), round(hi, 4)]}


def step_layer(dev, S, args):
    rng = np.random.default_rng(0)
    n, c, c_out, k, c_cell, c_uni = NX >> N_CONVOLUTIONS, MAX_FILTERS, MAX_FILTERS, 3, 3, 2
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    x = up(rng.normal(0, 1, (S, 6, n, n, c)))
    cell, uni = up(fmr_cases.grid_xyz(n).transpose(0, 2, 3, 1)), up([0.0, 1.0])
    w, w_ctx, bias = up(rng.normal(0, 0.02, (k, k, c, c_out))), up(rng.normal(0, 0.02, (k, k, c_cell + c_uni, c_out))), up(rng.normal(0, 0.1, c_out))
    cat = torch.cat([x, cell.expand(S, 6, n, n, c_cell), uni.expand(S, 6, n, n, c_uni)], dim=-1).contiguous()
    w_cat = torch.cat([w, w_ctx], dim=2).contiguous()
    dst = torch.empty((S, 6, n, n, c_out), dtype=torch.float32, device=dev)
    stream = _stream(dev)

    def context():
        _lib.call_on(dev, "fv3hip_cyclegan_conv_context", x.data_ptr(), c, 0, 0, None, None, None, 0, w.data_ptr(), bias.data_ptr(), None,
                     dst.data_ptr(), c_out, 0, 0, S, n, c, c_out, _lib.CYCLEGAN_CONV_REGULAR, k, _lib.CYCLEGAN_HALO_CUBE, cell.data_ptr(),
                     c_cell, uni.data_ptr(), c_uni, w_ctx.data_ptr(), stream)

    def plain(src=x, ld=c, ci=c, weights=w):
        _lib.call_on(dev, "fv3hip_cyclegan_conv", src.data_ptr(), ld, 0, 0, None, None, None, 0, weights.data_ptr(), bias.data_ptr(), None,
                     dst.data_ptr(), c_out, 0, 0, S, n, ci, c_out, _lib.CYCLEGAN_CONV_REGULAR, k, _lib.CYCLEGAN_HALO_CUBE, stream)

    concatenated = lambda: plain(cat, c + c_cell + c_uni, c + c_cell + c_uni, w_cat)
    context()
    with_context = dst.clone()
    concatenated()
    steps = auto_steps(context, args.steps)
    t_ctx, t_plain, t_cat = (timed(fn, steps, args.warmup) for fn in (context, plain, concatenated))
    flop = 2.0 * k * k * (c + c_cell + c_uni) * c_out * S * 6 * n * n
    return {"workload": f"step_layer_s{S}", "samples": S, "face": n, "c_in": c, "context": [c_cell, c_uni], "c_out": c_out, "k": k,
            "calls_per_window": steps, "context_entry": span(t_ctx),
            "context_entry_tflops": round(flop / t_ctx[0] / 1e9, 2),
            "no_context_existing_kernel": span(t_plain), "context_over_no_context": round(t_ctx[0] / t_plain[0], 4),
            "k_rows_predict": round(147 / 144, 4),
            "existing_entry_on_261_channel_concatenation": span(t_cat),
            "context_over_concatenation": round(t_ctx[0] / t_cat[0], 4),
            "max_abs_difference_context_vs_concatenation": float((with_context - dst).abs().max())}


def by_part(model, state, ntime):
    """One rollout with an event pair around every launch: ms per part and per layer kind, and their sum."""
    spans, part = [], ["encode"]

    def wrap(name, kind_of):
        inner = getattr(model, name)

        def outer(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            result = inner(*a, **kw)
            e1.record()
            spans.append((part[0], kind_of(a), e0, e1))
            return result

        setattr(model, name, outer)

    def mark(name, label):
        inner = getattr(model, name)

        def outer(*a, **kw):
            part[0] = label
            return inner(*a, **kw)

        setattr(model, name, outer)

    kinds = {"fi": "conv7x7", "la": "conv7x7", "do": "strided4x4", "re": "step3x3", "st": "step3x3", "up": "transposed4x4"}
    wrap("_conv", lambda a: kinds[a[0][:2]] + ("+context" if a[0].endswith(".a") else ""))
    wrap("_stats", lambda a: "statistics")
    wrap("_apply", lambda a: "apply")
    for name, label in (("_encode_chunk", "encode"), ("_step_chunk", "step"), ("_decode_chunk", "decode")):
        mark(name, label)
    try:
        model.forward(state, ntime)
        torch.cuda.synchronize()
    finally:
        for name in ("_conv", "_stats", "_apply", "_encode_chunk", "_step_chunk", "_decode_chunk"):
            delattr(model, name)
    parts, kinds_ms = {}, {}
    for p, kind, e0, e1 in spans:
        ms = e0.elapsed_time(e1)
        parts[p] = parts.get(p, 0.0) + ms
        kinds_ms[kind] = kinds_ms.get(kind, 0.0) + ms
    rnd = lambda d: {k: round(v, 4) for k, v in sorted(d.items())}
    return rnd(parts), rnd(kinds_ms), len(spans), round(sum(parts.values()), 4)


def rollout(dev, windows, args):
    rng = np.random.default_rng(0)
    spec = fmr_cases.make_spec(rng, VARIABLES, NX, N_CONVOLUTIONS, N_RESNET, MAX_FILTERS, samples_per_day=SAMPLES_PER_DAY)
    predictor = fit.HipFullModelReplacement(spec.state_variables, spec)
    model = predictor.model.generator
    state = torch.from_numpy(rng.normal(0, 1, (windows, 6, NX, NX, spec.n_features)).astype(np.float32)).to(dev)
    g = spec.generator
    flop = (g.flops_encode() + g.flops_decode() + (NTIME - 1) * g.flops_per_step()) * windows
    forward = lambda: model.forward(state, NTIME)
    steps = auto_steps(forward, args.steps)
    t_hip = timed(forward, steps, args.warmup)
    parts, kinds, launches, total = by_part(model, state, NTIME)
    row = {"workload": f"rollout_w{windows}", "nx": NX, "windows": windows, "ntime": NTIME, "channels": spec.n_features,
           "n_convolutions": N_CONVOLUTIONS, "n_resnet": N_RESNET, "max_filters": MAX_FILTERS, "samples_per_day": SAMPLES_PER_DAY,
           "gflop_per_window": round(flop / windows / 1e9, 3), "calls_per_window": steps, "chunk": model.chunk_size(windows),
           "workspace_mib_per_window": round(model.workspace_bytes_per_sample() / 2 ** 20, 2),
           "hip_forward_ms": round(t_hip[0], 4), "hip_forward_ms_min_max_of_5_windows": [round(t_hip[1], 4), round(t_hip[2], 4)],
           "hip_forward_tflops": round(flop / t_hip[0] / 1e9, 2),
           "hip_forward_fraction_of_fp32_matrix_peak": round(flop / t_hip[0] / 1e9 / FP32_MATRIX_PEAK_TFLOPS, 4),
           "launches": launches, "sum_of_launches_ms": total, "sum_of_launches_over_forward": round(total / t_hip[0], 3),
           "by_part_ms": parts, "by_kind_ms": kinds}
    twin = recurrent_twin_from_spec(g, spec.convolution_type, torch.float32, dev)
    x = state.permute(0, 1, 4, 2, 3).contiguous()

    def tcall():
        with torch.no_grad():
            return twin(x, NTIME)

    t_twin = timed(tcall, auto_steps(tcall, args.steps), args.warmup)
    row["torch_twin_forward_ms"] = round(t_twin[0], 4)
    row["torch_twin_forward_ms_min_max_of_5_windows"] = [round(t_twin[1], 4), round(t_twin[2], 4)]
    row["hip_over_torch_twin"] = round(t_hip[0] / t_twin[0], 3)
    got, want = forward(), tcall().permute(0, 1, 2, 4, 5, 3)
    row["max_abs_difference_to_twin_per_time"] = [float(v) for v in (got - want).abs().amax(dim=(0, 2, 3, 4, 5)).cpu()]
    del twin, got, want
    if windows == 1:
        cpu = recurrent_twin_from_spec(g, spec.convolution_type, torch.float32, "cpu")
        xc = x.cpu()
        with torch.no_grad():
            cpu(xc, 2)
            t0 = time.perf_counter()
            cpu(xc, NTIME)
        row["torch_cpu_f32_forward_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="calls per timed window (0: enough for about 0.2 s)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, choices=("step_layer", "rollout"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fmr_rollout.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.load()
    rows = []
    jobs = [(step_layer, S) for S in (1, 100) if args.only != "rollout"] + [(rollout, w) for w in (1, 8) if args.only != "step_layer"]
    for fn, size in jobs:
        rows.append(fn(dev, size, args))
        torch.cuda.empty_cache()
        print(json.dumps(rows[-1]), flush=True)
    if args.only is None:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(dev), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
