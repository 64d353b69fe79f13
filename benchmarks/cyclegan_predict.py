"""CycleGAN generator at the reference's production configuration (projects/cyclegan/c48_to_c384 and 0K_to_8K: C48 faces,
n_convolutions 2, n_resnet 6, max_filters 256, halo_conv2d; one and two 2-D state variables) through ``GeneratorModel.forward``
and ``HipCycleGAN.predict`` from device-resident arrays, timed with HIP events after warm-up, next to the plain-torch twin
(``fit.GeneratorTwin``: ``nn.Conv2d`` / ``nn.ConvTranspose2d`` / ``nn.InstanceNorm2d`` on ``append_halos_tensor``-padded input)
on the same device in the same run, and the float32 twin on the CPU.

Batches of 1 and of 100 samples.  Times are per call: the median of five windows of back-to-back calls (minimum and maximum
beside it).  TFLOP/s are algorithmic and exact fp32: per sample the sum over the layers of 2 x taps x c_in x c_out x 6 n_l^2
(``GeneratorSpec.flops_per_sample``; a transposed layer counts the 4 taps every output cell reads).  ``by_kind_ms`` is one
forward pass with a HIP event around every launch, summed per layer kind.  One JSON line per workload; all of them are also
written to profiles/cyclegan_predict.json.  ``--quick NAME`` runs the HIP path of one workload only (for profiler runs).

    python3 benchmarks/cyclegan_predict.py [--quick one_var_b100] [--steps K] [--warmup W]
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
import cyclegan_cases  # noqa: E402
from fv3net_amd import fit  # noqa: E402
from fv3net_amd.cyclegan import theta_from_seconds  # noqa: E402
from fv3net_amd.fit.cyclegan import twin_from_spec  # noqa: E402
from fv3net_amd.xr_compat import DataArray, Dataset  # noqa: E402

FP32_MATRIX_PEAK_TFLOPS = 157.3   # MI355X, v_mfma_f32_32x32x2_f32: 256 FLOP / clk / CU x 256 CUs x 2.4 GHz
NX, N_CONVOLUTIONS, N_RESNET, MAX_FILTERS = 48, 2, 6, 256


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
    return max(2, min(200, int(200.0 / timed(fn, 1, 1, repeats=1)[0])))   # windows of about 0.2 s


def by_kind(model, state, theta):
    """One forward pass with an event pair around every launch: ms per layer kind."""
    spans = []

    def wrap(name, kind_of):
        inner = getattr(model, name)

        def outer(*args, **kwargs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            result = inner(*args, **kwargs)
            b.record()
            spans.append((kind_of(args), a, b))
            return result

        setattr(model, name, outer)

    conv_kind = lambda args: {"fi": "conv7x7", "la": "conv7x7", "do": "strided4x4", "re": "resnet3x3", "up": "transposed4x4"}[args[0][:2]]
    wrap("_conv", conv_kind)
    wrap("_stats", lambda args: "statistics")
    wrap("_apply", lambda args: "apply")
    try:
        model.forward(state, theta)
        torch.cuda.synchronize()
    finally:
        for name in ("_conv", "_stats", "_apply"):
            delattr(model, name)
    out = {}
    for kind, a, b in spans:
        out[kind] = out.get(kind, 0.0) + a.elapsed_time(b)
    return {k: round(v, 4) for k, v in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="calls per timed window (0: enough for about 0.2 s)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", default=None, help="the HIP path of that workload only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cyclegan_predict.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    plans = [(f"{label}_b{batch}", variables, batch) for label, variables in (("one_var", {"h500": 1}), ("two_vars", {"h500": 1, "PRATEsfc": 1}))
             for batch in (1, 100)]
    if args.quick:
        plans = [p for p in plans if p[0] == args.quick][:1]
    rows = []
    for name, variables, batch in plans:
        rng = np.random.default_rng(0)
        spec = cyclegan_cases.make_spec(rng, variables, NX, N_CONVOLUTIONS, N_RESNET, MAX_FILTERS)
        predictor = fit.HipCycleGAN(spec.state_variables, spec)
        data, seconds = cyclegan_cases.make_dataset(rng, spec, batch, np.float32)
        X = Dataset({k: DataArray(torch.from_numpy(a).to(dev), dims=dims) for k, (dims, a) in data.items()})
        X["time"] = DataArray(seconds, dims=("time",))
        model = predictor.model.generator()
        state = predictor.model.pack([X[k].data.unsqueeze(-1) for k in variables], "a")
        theta = torch.from_numpy(theta_from_seconds(seconds.astype(np.float32))).to(dev)
        flop = spec.generator_a_to_b.flops_per_sample() * batch
        forward = lambda: model.forward(state, theta)
        steps = auto_steps(forward, args.steps)
        ms, ms_min, ms_max = timed(forward, steps, args.warmup)
        predict = lambda: predictor.predict(X)
        p, p_min, p_max = timed(predict, steps, args.warmup)
        row = {"workload": name, "nx": NX, "batch": batch, "channels": spec.n_features, "n_convolutions": N_CONVOLUTIONS,
               "n_resnet": N_RESNET, "max_filters": MAX_FILTERS, "gflop_per_sample": round(flop / batch / 1e9, 3), "calls_per_window": steps,
               "chunk": model.chunk_size(batch), "workspace_mib_per_sample": round(model.workspace_bytes_per_sample() / 2 ** 20, 2),
               "hip_forward_ms": round(ms, 4), "hip_forward_ms_min_max_of_5_windows": [round(ms_min, 4), round(ms_max, 4)],
               "hip_forward_tflops": round(flop / ms / 1e9, 2),
               "hip_forward_fraction_of_fp32_matrix_peak": round(flop / ms / 1e9 / FP32_MATRIX_PEAK_TFLOPS, 3),
               "hip_predict_ms": round(p, 4), "hip_predict_ms_min_max_of_5_windows": [round(p_min, 4), round(p_max, 4)],
               "by_kind_ms": by_kind(model, state, theta)}
        if not args.quick:
            twin = twin_from_spec(spec.generator_a_to_b, spec.convolution_type, torch.float32, dev)
            x = state.permute(0, 1, 4, 2, 3).contiguous()
            secs = torch.from_numpy(seconds.astype(np.float32)).to(dev)

            def tcall():
                with torch.no_grad():
                    return twin(secs, x)

            t, t_min, t_max = timed(tcall, auto_steps(tcall, args.steps), args.warmup)
            row["torch_twin_forward_ms"] = round(t, 4)
            row["torch_twin_forward_ms_min_max_of_5_windows"] = [round(t_min, 4), round(t_max, 4)]
            row["torch_twin_forward_tflops"] = round(flop / t / 1e9, 2)
            row["hip_over_torch_twin"] = round(ms / t, 3)
            got, want = model.forward(state[:1], theta[:1]), tcall()[:1].permute(0, 1, 3, 4, 2)
            row["max_abs_difference_to_twin"] = float((got - want).abs().max())
            del twin, got, want, x
            if batch == 1:
                cpu = twin_from_spec(spec.generator_a_to_b, spec.convolution_type, torch.float32, "cpu")
                xc, sc = state.permute(0, 1, 4, 2, 3).cpu(), torch.from_numpy(seconds.astype(np.float32))
                with torch.no_grad():
                    cpu(sc, xc)
                    t0 = time.perf_counter()
                    cpu(sc, xc)
                row["torch_cpu_f32_forward_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        del model, predictor, state, X
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
