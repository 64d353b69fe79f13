"""Convolutional predict (fv3hip_conv_predict) on three workloads, timed with HIP events after warm-up, next to the same graph
through PyTorch-ROCm's ``conv2d`` on the same device in the same run and the float32 ``torch`` CPU chain.

  W1  the C384 cube resident: 6 x 384 x 384 = 884 736 pixels, T + q (79 levels each) + cos-zenith = 159 channels, the
      reference's defaults (32 filters, depth 3, 3 x 3 kernels, relu), dQ1 + dQ2 (79 levels each); float32 and float64 sources
  W2  one 48 x 48 rank with its halo strips supplied (the prognostic-run call of a six-rank C48 run)
  W3  the C48 cube resident

The HIP time covers the whole call on the fields as the model holds them ([tile, z, y, x]): halos, normalisation, all layers.
The library comparison is timed on an input that was padded and normalised beforehand ([tile, C, x + 2h, y + 2h]), its
``conv2d`` chain in the default and in the ``channels_last`` memory format, the faster taken.  Times are the median of five windows of back-to-back calls (about 0.2 s each; minimum and maximum beside it).  One JSON line per workload;
``--quick`` times the HIP path of W1 (float32) only (for profiler runs).

    python3 benchmarks/conv_predict.py [--quick] [--steps K] [--warmup W]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fv3net_amd.conv import ConvInput, ConvModel, ConvOutput, ConvSpec  # noqa: E402

NZ = 79
FP32_MATRIX_PEAK_TFLOPS = 157.3  # MI355X, v_mfma_f32_32x32x2_f32: 256 FLOP / clk / CU x 256 CUs x 2.4 GHz


def default_spec(rng, filters=32, depth=3, k=3):
    inputs = [ConvInput("T", NZ, rng.normal(250, 30, NZ).astype(np.float32), rng.uniform(2, 20, NZ).astype(np.float32)),
              ConvInput("q", NZ, rng.uniform(0, 1e-2, NZ).astype(np.float32), rng.uniform(1e-6, 1e-3, NZ).astype(np.float32)),
              ConvInput("cos_zenith", 1, np.float32([0.2]), np.float32([0.3]))]
    c_in, kernels, biases = 2 * NZ + 1, [], []
    for _ in range(depth - 1):
        kernels.append((rng.normal(0, 1, (k, k, c_in, filters)) / np.sqrt(k * k * c_in)).astype(np.float32))
        biases.append(rng.normal(0, 0.1, filters).astype(np.float32))
        c_in = filters
    outputs = [ConvOutput(name, NZ, (rng.normal(0, 1, (filters, NZ)) / np.sqrt(filters)).astype(np.float32),
                          rng.normal(0, 0.1, NZ).astype(np.float32), rng.uniform(1e-8, 1e-4, NZ).astype(np.float32),
                          rng.normal(0, 1e-6, NZ).astype(np.float32)) for name in ("dQ1", "dQ2")]
    return ConvSpec(inputs, kernels, biases, outputs, activation="relu")


def fields(spec, lead, n, dtype, dev, gen):
    """name -> [*lead, z, y, x] on the device, drawn around each channel's own mean and spread."""
    out = {}
    for i in spec.inputs:
        a = torch.randn(tuple(lead) + (i.nfeat, n, n), device=dev, dtype=torch.float32, generator=gen)
        a = a * torch.from_numpy(i.scale).to(dev)[:, None, None] + torch.from_numpy(i.center).to(dev)[:, None, None]
        out[i.source] = a.to(dtype)
    return out


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


def torch_graph(spec, dev):
    ws = [torch.from_numpy(w).permute(3, 2, 0, 1).contiguous().to(dev) for w in spec.hidden_kernels]
    bs = [torch.from_numpy(b).to(dev) for b in spec.hidden_biases]
    hw = torch.cat([torch.from_numpy(o.kernel) for o in spec.outputs], dim=1).t()[:, :, None, None].contiguous().to(dev)
    hb = torch.cat([torch.from_numpy(o.bias) for o in spec.outputs]).to(dev)
    hs = torch.cat([torch.from_numpy(o.scale) for o in spec.outputs]).to(dev)[None, :, None, None]
    hc = torch.cat([torch.from_numpy(o.center) for o in spec.outputs]).to(dev)[None, :, None, None]

    def run(x):
        for w, b in zip(ws, bs):
            x = torch.relu(torch.nn.functional.conv2d(x, w, b))
        return torch.nn.functional.conv2d(x, hw, hb) * hs + hc

    return run, (ws, hw)


def library_times(spec, samples, n, dev, steps, warmup, gen):
    """ms of the conv2d chain on a padded, normalised input, per memory format; an error text where the library refuses."""
    h = spec.halos_required
    out = {}
    for fmt_name, fmt in (("default", torch.contiguous_format), ("channels_last", torch.channels_last)):
        try:
            run, (ws, hw) = torch_graph(spec, dev)
            if fmt is torch.channels_last:
                for w in ws + [hw]:
                    w.data = w.data.contiguous(memory_format=fmt)
            x = torch.randn((samples, spec.n_in_channels, n + 2 * h, n + 2 * h), device=dev, generator=gen).contiguous(memory_format=fmt)
            with torch.no_grad():
                out[fmt_name] = round(timed(lambda: run(x), steps, warmup)[0], 4)
            del x
        except Exception as err:  # noqa: BLE001  (recorded, not hidden: the comparison then rests on the CPU chain)
            out[fmt_name] = f"failed: {type(err).__name__}: {str(err)[:200]}"
        torch.cuda.empty_cache()
    return out


def cpu_time(spec, samples, n):
    h = spec.halos_required
    run, _ = torch_graph(spec, torch.device("cpu"))
    x = torch.randn((samples, spec.n_in_channels, n + 2 * h, n + 2 * h))
    with torch.no_grad():
        run(x[:1])
        t0 = time.perf_counter()
        run(x)
    return round((time.perf_counter() - t0) * 1e3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="calls per timed window (0: enough for about 0.2 s)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    gen = torch.Generator(device=dev).manual_seed(0)
    spec = default_spec(rng)
    model = ConvModel(spec, device=dev)
    h = spec.halos_required
    plans = [("W1_c384_cube_f32", 6, 384, torch.float32, "cube"), ("W1_c384_cube_f64", 6, 384, torch.float64, "cube"),
             ("W2_c48_rank_strips", 1, 48, torch.float32, "strips"), ("W3_c48_cube", 6, 48, torch.float32, "cube")]
    if args.quick:
        plans = plans[:1]
    for name, samples, n, dtype, halo in plans:
        src = fields(spec, (samples,), n, dtype, dev, gen)
        strips = None
        if halo == "strips":
            strips = torch.randn((samples, 4, h, spec.n_in_channels, n), device=dev, generator=gen)
        call = lambda: model.predict(src, halo=halo, strips=strips)
        steps = args.steps
        if steps <= 0:  # windows of about 0.2 s, so that neither the clock ramp nor the scheduler is what gets measured
            steps = max(10, min(2000, int(200.0 / timed(call, 3, 2, repeats=1)[0])))
        with torch.no_grad():
            ms, ms_min, ms_max = timed(call, steps, args.warmup)
        t0 = time.perf_counter()   # the host side of a call: what it costs to enqueue, with the device left behind
        for _ in range(steps):
            call()
        host_ms = (time.perf_counter() - t0) * 1e3 / steps
        torch.cuda.synchronize()
        pixels = samples * n * n
        tflops = pixels * spec.flops_per_pixel / ms / 1e9
        row = {"workload": name, "pixels": pixels, "channels_in": spec.n_in_channels, "filters": spec.filters, "depth": spec.depth,
               "kernel_size": spec.kernel_size, "source_dtype": str(dtype).split(".")[-1], "halo": halo,
               "flop_per_pixel": spec.flops_per_pixel, "steps_per_window": steps, "hip_ms": round(ms, 4), "host_enqueue_ms": round(host_ms, 4),
               "hip_ms_min_max_of_5_windows": [round(ms_min, 4), round(ms_max, 4)], "hip_tflops_whole_call": round(tflops, 2),
               # the whole call -- depth + 1 launches and the host side of predict -- not one kernel's share of the peak
               "whole_call_fraction_of_fp32_matrix_peak": round(tflops / FP32_MATRIX_PEAK_TFLOPS, 3)}
        del src
        torch.cuda.empty_cache()
        if not args.quick:
            lib = library_times(spec, samples, n, dev, steps, args.warmup, gen)
            row["pytorch_rocm_ms"] = lib
            ok = [v for v in lib.values() if not isinstance(v, str)]
            if ok:
                row["hip_over_pytorch_rocm"] = round(ms / min(ok), 3)
            row["torch_cpu_f32_ms"] = cpu_time(spec, samples, n)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
