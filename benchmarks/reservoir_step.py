"""One reservoir step (fv3hip_reservoir_increment, fv3hip_reservoir_predict) on three workloads, timed with HIP events after
warm-up, next to a numpy/scipy restatement of the reference's step in the same process.

  R1  the production SST config (projects/reservoir/train/training-config.yaml): one C48 tile per rank, 2x2 layout,
      overlap 0, state 1000, 4 input variables with z = 1, adjacency sparsity 0.999, input coupling sparsity 0.001,
      scale-spatial-concat-z transformers, 1 output variable (SST)
  R2  the sweep's largest (sweep/tile-train-sweep.yaml): R1 with state 5000 and a 4x4 layout
  R3  a scaling point: one C384 tile, 8x8 layout, state 5000 (W_in 369 MB, C 5.9 GB: past the 256 MiB Infinity Cache)

Each step is timed back to back, so R1 and R2 (18-92 MB) are read from the Infinity Cache; R3 from HBM.  The weights are
random (the cost depends on shapes only).  One JSON line per workload.

    python3 benchmarks/reservoir_step.py [--workloads R1,R2,R3] [--steps K] [--warmup W] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fv3net_amd.reservoir import (RankXYDivider, ReservoirModel, ScaleSpatialConcatZTransformer,  # noqa: E402
                                  SparseMatrix)

STREAM_TBS = (6.0, 6.3)    # measured HBM streaming rate (MI355X_MICROARCH: float4 copy 6.29 TB/s, 1.2 GB sweep 6.0-6.1)
FP64_TFLOPS = 78.6         # vendor float64 figure (not measured on this card)

WORKLOADS = {
    "R1": dict(tile=48, layout=(2, 2), state=1000),
    "R2": dict(tile=48, layout=(4, 4), state=5000),
    "R3": dict(tile=384, layout=(8, 8), state=5000),
}
N_VAR, W_RES_SPARSITY, W_IN_SPARSITY = 4, 0.999, 0.001


def random_csr(rng, m, n, density, lo, hi):
    """Rows of a random sparse matrix; dense enough ones as a full pattern (as scipy.sparse.random with that density)."""
    if density >= 0.99:
        idx = np.tile(np.arange(n, dtype=np.int32), m)
        keep = rng.random(m * n) < density
        counts = keep.reshape(m, n).sum(axis=1)
        indptr = np.zeros(m + 1, np.int64)
        np.cumsum(counts, out=indptr[1:])
        return indptr, idx[keep], rng.uniform(lo, hi, int(keep.sum()))
    nnz = int(round(m * n * density))
    flat = np.unique(rng.choice(m * n, nnz, replace=False))
    rows, cols = np.divmod(flat, n)
    indptr = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=m), out=indptr[1:])
    return indptr, cols.astype(np.int32), rng.uniform(lo, hi, flat.size)


def build(name, rng):
    w = WORKLOADS[name]
    tile, (lx, ly), S = w["tile"], w["layout"], w["state"]
    ns = lx * ly
    sub = tile // lx
    n_in = sub * sub * N_VAR
    n_out = sub * sub
    divider = RankXYDivider((lx, ly), 0, rank_extent=(tile, tile), z_feature_size=N_VAR)
    tin = ScaleSpatialConcatZTransformer(rng.standard_normal(N_VAR * tile * tile).astype(np.float32),
                                         rng.uniform(0.5, 2, N_VAR * tile * tile).astype(np.float32), (tile, tile, 1), N_VAR)
    tout = ScaleSpatialConcatZTransformer(rng.standard_normal(tile * tile).astype(np.float32),
                                          rng.uniform(0.5, 2, tile * tile).astype(np.float32), (tile, tile, 1), 1)
    w_in = random_csr(rng, S, n_in, 1.0 - W_IN_SPARSITY, -0.1, 0.1)
    w_res = random_csr(rng, S, S, 1.0 - W_RES_SPARSITY, 0.0, 1.0)
    w_res = (w_res[0], w_res[1], w_res[2] * (0.99 / max(1.0, S * (1.0 - W_RES_SPARSITY) * 0.5)))
    coef = rng.standard_normal((ns, S, n_out)) * (1.0 / np.sqrt(S))
    bias = rng.standard_normal((ns, n_out))
    model = ReservoirModel(divider, tin, tout, SparseMatrix.from_csr(*w_in, (S, n_in)),
                           SparseMatrix.from_csr(*w_res, (S, S)), coef, bias)
    inputs = [torch.randn(tile, tile, 1, dtype=torch.float32, device="cuda") for _ in range(N_VAR)]
    return dict(model=model, inputs=inputs, w_in=w_in, w_res=w_res, coef=coef, bias=bias, tin=tin, tout=tout, ns=ns,
                S=S, n_in=n_in, n_out=n_out, layout=(lx, ly), tile=tile, sub=sub)


def gpu_time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / steps  # us


def numpy_step(w):
    """The reference's increment_state and predict in numpy/scipy (reservoir.py:68-82, readout.py:98-99, transformer.py)."""
    import scipy.sparse as sp
    S, ns, lx, sub, tile = w["S"], w["ns"], w["layout"][0], w["sub"], w["tile"]
    w_in = sp.csr_matrix((w["w_in"][2], w["w_in"][1], w["w_in"][0]), shape=(S, w["n_in"])).tocsc()
    w_res = sp.csr_matrix((w["w_res"][2], w["w_res"][1], w["w_res"][0]), shape=(S, S)).tocsc()
    x = [t.cpu().numpy() for t in w["inputs"]]
    c_in, s_in = w["tin"].center, w["tin"].scale
    c_out, s_out = w["tout"].center, w["tout"].scale
    state = np.zeros((ns, S))

    def step():
        nonlocal state
        stacked = np.concatenate([a.reshape(-1) for a in x]).astype(np.float32)
        enc = (stacked - c_in) / (s_in + np.float32(1e-7))
        enc = np.concatenate([p.reshape(tile, tile, 1) for p in np.split(enc, N_VAR)], axis=-1)
        u = np.stack([enc[(s % lx) * sub:(s % lx + 1) * sub, (s // lx) * sub:(s // lx + 1) * sub].reshape(-1)
                      for s in range(ns)])
        state = np.tanh(u @ w_in.T + state @ w_res.T)
        y = np.einsum("...ij,ijk->...ik", state, w["coef"]) + w["bias"]
        merged = np.empty((tile, tile, 1))
        for s in range(ns):
            merged[(s % lx) * sub:(s % lx + 1) * sub, (s // lx) * sub:(s // lx + 1) * sub] = y[s].reshape(sub, sub, 1)
        return (merged.reshape(-1).astype(np.float32) * s_out + c_out).reshape(tile, tile, 1)

    step()
    t0 = time.perf_counter()
    n = 3
    for _ in range(n):
        step()
    return (time.perf_counter() - t0) * 1e6 / n


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--workloads", default="R1,R2,R3")
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--no-cpu", action="store_true", help="skip the numpy/scipy restatement")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU path to time")
    for name in args.workloads.split(","):
        rng = np.random.default_rng(0)
        w = build(name, rng)
        m = w["model"]
        t_inc = gpu_time(lambda: m.increment(w["inputs"]), args.steps, args.warmup)
        t_pred = gpu_time(lambda: m.predict(), args.steps, args.warmup)
        t_step = gpu_time(lambda: (m.increment(w["inputs"]), m.predict()), args.steps, args.warmup)
        S, ns, n_in, n_out = w["S"], w["ns"], w["n_in"], w["n_out"]
        win_bytes = ((n_in + 63) // 64 * 64) * ((S + 1) // 2 * 2) * 8  # dense, column-major (density 0.999)
        wres_bytes = w["w_res"][2].size * 12 + (S + 1) * 8
        c_bytes = ns * S * ((n_out + 1) // 2 * 2) * 8
        inc_flop, read_flop = 2.0 * ns * S * n_in, 2.0 * ns * S * n_out
        inc_tbs = (win_bytes + wres_bytes) / (t_inc * 1e-6) / 1e12
        read_tbs = c_bytes / (t_pred * 1e-6) / 1e12
        res = {
            "workload": name, "tile": w["tile"], "layout": list(w["layout"]), "state_size": S, "input_size": n_in,
            "n_out": n_out, "cache_state": "HBM (past the Infinity Cache)" if c_bytes > (256 << 20) else
            "Infinity Cache (back to back)",
            "increment_us": round(t_inc, 2), "predict_us": round(t_pred, 2), "step_us": round(t_step, 2),
            "w_in_bytes": win_bytes, "w_res_bytes": wres_bytes, "c_bytes": c_bytes,
            "increment_tbs": round(inc_tbs, 3), "increment_tflops": round(inc_flop / (t_inc * 1e-6) / 1e12, 2),
            "increment_frac_stream": [round(inc_tbs / r, 3) for r in STREAM_TBS],
            "increment_frac_fp64": round(inc_flop / (t_inc * 1e-6) / 1e12 / FP64_TFLOPS, 3),
            "predict_tbs": round(read_tbs, 3), "predict_frac_stream": [round(read_tbs / r, 3) for r in STREAM_TBS],
        }
        if not args.no_cpu:
            t_cpu = numpy_step(w)
            res["numpy_step_us"] = round(t_cpu, 1)
            res["speedup_step"] = round(t_cpu / t_step, 1)
        print(json.dumps(res), flush=True)
        del w, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
