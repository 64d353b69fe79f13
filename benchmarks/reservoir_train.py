"""Reservoir training per batch of 100 time steps on the workloads of benchmarks/reservoir_step.py (R1, R2,
R3 of section 12): the series stepping (fv3hip_reservoir_train_series), the Gram update (fv3hip_gram_update) and the ridge
solve (torch.linalg.solve per subdomain), timed with HIP events after warm-up, next to

  (a) the numpy restatement in the same process (one scipy/numpy increment per time step, X1.T @ X1 and X1.T @ Y per
      subdomain, np.linalg.solve), and
  (b) torch.baddbmm in float64 (rocBLAS) on the same resident X and Y, for the Gram update alone, in alternating windows of
      the same run.  (b) is given the series with the bias column already appended and laid out [subdomain, time, feature];
      building that copy is not timed.

The update's TFLOP/s counts the full products, 2 T J1^2 + 2 T J1 n_out per subdomain, although the kernel computes only the
tiles of A on or above the diagonal; the fraction is of the vendor's 78.6 TFLOP/s float64 figure.  Its bytes are the
accumulators read (the upper tiles of A, and B) and written (all of A, and B).  One JSON line per workload.

    python3 benchmarks/reservoir_train.py [--workloads R1,R2,R3] [--windows N] [--updates K] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reservoir_step import FP64_TFLOPS, N_VAR, STREAM_TBS, build  # noqa: E402

from fv3net_amd.fit import BatchLinearRegressor, BatchLinearRegressorHyperparameters  # noqa: E402
from fv3net_amd.reservoir import GramAccumulator  # noqa: E402

N_TIMES = 100
L2 = 1.0


def window_ms(fn, count):
    """``count`` back-to-back calls between two events: ms per call."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(count):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / count


def alternating(fns, windows, count, warmup=2):
    """Median and range of ms per call of each function, measured in alternating windows."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            times[i].append(window_ms(fn, count))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in times]


def numpy_parts(w, inputs, X, Y, series_steps):
    """(series ms per batch, Gram ms per batch, solve ms for every subdomain) of the numpy restatement; the series is
    timed over ``series_steps`` steps and the solve on one subdomain, both scaled."""
    import scipy.sparse as sp

    S, ns, lx, sub, tile = w["S"], w["ns"], w["layout"][0], w["sub"], w["tile"]
    w_in = sp.csr_matrix((w["w_in"][2], w["w_in"][1], w["w_in"][0]), shape=(S, w["n_in"])).tocsc()
    w_res = sp.csr_matrix((w["w_res"][2], w["w_res"][1], w["w_res"][0]), shape=(S, S)).tocsc()
    c_in, s_in = w["tin"].center, w["tin"].scale
    x = [t.cpu().numpy() for t in inputs]
    state = np.zeros((ns, S))
    t0 = time.perf_counter()
    for t in range(series_steps):
        stacked = np.concatenate([a[t].reshape(-1) for a in x]).astype(np.float32)
        enc = (stacked - c_in) / (s_in + np.float32(1e-7))
        enc = np.concatenate([p.reshape(tile, tile, 1) for p in np.split(enc, N_VAR)], axis=-1)
        u = np.stack([enc[(s % lx) * sub:(s % lx + 1) * sub, (s // lx) * sub:(s // lx + 1) * sub].reshape(-1)
                      for s in range(ns)])
        state = np.tanh(u @ w_in.T + state @ w_res.T)
    series_ms = (time.perf_counter() - t0) * 1e3 * N_TIMES / series_steps
    Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
    A = np.zeros((S + 1, S + 1))
    B = np.zeros((S + 1, Yh.shape[2]))
    t0 = time.perf_counter()
    for s in range(ns):  # one pair of sums reused: the timing is the products and the additions
        x1 = np.concatenate([Xh[:, s], np.ones((N_TIMES, 1))], axis=1)
        A = np.add(A, np.dot(x1.T, x1))
        B = np.add(B, np.dot(x1.T, Yh[:, s]))
    gram_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    np.linalg.solve(A + L2 * np.identity(S + 1), B)
    solve_ms = (time.perf_counter() - t0) * 1e3 * ns
    return series_ms, gram_ms, solve_ms


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--workloads", default="R1,R2,R3")
    p.add_argument("--windows", type=int, default=5, help="alternating timing windows per measurement")
    p.add_argument("--updates", type=int, default=0, help="calls per window (0: enough for about 0.2 s of work)")
    p.add_argument("--no-cpu", action="store_true", help="skip the numpy restatement")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path to time")
    dev = torch.device("cuda")
    for name in args.workloads.split(","):
        w = build(name, np.random.default_rng(0))
        m, S, ns, n_out, tile = w["model"], w["S"], w["ns"], w["n_out"], w["tile"]
        J1 = S + 1
        inputs = [torch.randn(N_TIMES, tile, tile, 1, dtype=torch.float32, device=dev) for _ in range(N_VAR)]
        targets = [torch.randn(N_TIMES, tile, tile, 1, dtype=torch.float32, device=dev)]
        m.reset_state()
        X, Y = m.train_series(inputs), m.encode_targets(targets)
        per_window = lambda ms: args.updates or max(3, int(200.0 / max(ms, 1e-3)))  # noqa: E731

        # series stepping (states and packing) and the target encoding
        rough = window_ms(lambda: m.train_series(inputs), 1)
        (series, targets_ms) = alternating([lambda: m.train_series(inputs), lambda: m.encode_targets(targets)],
                                           args.windows, per_window(rough))

        # Gram update against rocBLAS on the same resident series
        acc = GramAccumulator(ns, S, n_out, add_bias=True, device=dev)
        X1 = torch.cat([X, torch.ones((N_TIMES, ns, 1), dtype=torch.float64, device=dev)], dim=2).permute(1, 0, 2).contiguous()
        Ys = Y.permute(1, 0, 2).contiguous()
        X1t = X1.transpose(1, 2)
        A2 = torch.zeros((ns, J1, J1), dtype=torch.float64, device=dev)
        B2 = torch.zeros((ns, J1, n_out), dtype=torch.float64, device=dev)

        def ours():
            acc.update(X, Y)

        def rocblas():
            torch.baddbmm(A2, X1t, X1, out=A2)
            torch.baddbmm(B2, X1t, Ys, out=B2)

        ours()
        rocblas()
        a_ours, b_ours = acc.get(0)
        diff_a = float((a_ours - A2[0]).abs().max() / A2[0].abs().max())
        diff_b = float((b_ours - B2[0]).abs().max() / B2[0].abs().max())
        del a_ours, b_ours
        rough = window_ms(ours, 1)
        gram, blas = alternating([ours, rocblas], args.windows, per_window(rough))
        flop = ns * (2.0 * N_TIMES * J1 * J1 + 2.0 * N_TIMES * J1 * n_out)
        nt = -(-J1 // 64)
        upper = min(nt * (nt + 1) // 2 * 64 * 64, J1 * J1)
        bytes_moved = ns * 8.0 * (upper + J1 * J1 + 2 * J1 * n_out)
        del A2, B2, X1, X1t, Ys
        torch.cuda.empty_cache()

        # the solve: the public regressor over the same accumulated sums' shapes
        lr = BatchLinearRegressor(BatchLinearRegressorHyperparameters(l2=L2), device=dev)
        lr.batch_update(X, Y)
        lr.get_weights()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lr.get_weights()
        torch.cuda.synchronize()
        solve_ms = (time.perf_counter() - t0) * 1e3
        res = {
            "workload": name, "tile": tile, "layout": list(w["layout"]), "state_size": S, "n_out": n_out, "n_times": N_TIMES,
            "accumulator_bytes": int(ns * 8 * (J1 * J1 + J1 * n_out)),
            "series_ms": round(series[0], 3), "series_ms_range": [round(series[1], 3), round(series[2], 3)],
            "encode_targets_ms": round(targets_ms[0], 3),
            "gram_ms": round(gram[0], 3), "gram_ms_range": [round(gram[1], 3), round(gram[2], 3)],
            "baddbmm_ms": round(blas[0], 3), "baddbmm_ms_range": [round(blas[1], 3), round(blas[2], 3)],
            "gram_over_baddbmm": round(gram[0] / blas[0], 3),
            "gram_tflops": round(flop / (gram[0] * 1e-3) / 1e12, 2),
            "gram_frac_fp64": round(flop / (gram[0] * 1e-3) / 1e12 / FP64_TFLOPS, 3),
            "gram_tbs": round(bytes_moved / (gram[0] * 1e-3) / 1e12, 3),
            "gram_frac_stream": [round(bytes_moved / (gram[0] * 1e-3) / 1e12 / r, 3) for r in STREAM_TBS],
            "gram_vs_baddbmm_max_rel_diff": [diff_a, diff_b],
            "solve_ms": round(solve_ms, 2),
        }
        if not args.no_cpu:
            steps = N_TIMES if S * ns <= 100000 else 10
            s_ms, g_ms, v_ms = numpy_parts(w, inputs, X, Y, steps)
            res.update({"numpy_series_ms": round(s_ms, 1), "numpy_series_steps_timed": steps, "numpy_gram_ms": round(g_ms, 1),
                        "numpy_solve_ms": round(v_ms, 1), "numpy_solve_subdomains_timed": 1,
                        "speedup_series": round(s_ms / series[0], 1), "speedup_gram": round(g_ms / gram[0], 1),
                        "speedup_solve": round(v_ms / solve_ms, 1)})
        print(json.dumps(res), flush=True)
        del w, m, acc, lr, X, Y
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
