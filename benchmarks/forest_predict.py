"""Random-forest predict (fv3hip_forest_predict) on three workloads, timed with HIP events after warm-up, next to sklearn's
own predict on a trained forest of the same tree count, depth and outputs.

  W1  C48: 13 824 columns, T and q (79 levels each) + 2 scalars = 160 features, dQ1 + dQ2 = 158 outputs, 100 trees, depth 13
  W2  one C384 tile: 147 456 columns, the W1 forest
  W3  the integration shape (tests/end_to_end_integration/argo.yaml): 1 tree, depth 13, dQ1 only (79 outputs), C48

The timed forests are complete trees synthesised as arrays (the cost depends on shape, not on training); thresholds are drawn
from the inputs' values.  One JSON line per workload; `--quick` times W1 only and skips sklearn (for profiler runs).

    python3 benchmarks/forest_predict.py [--quick] [--steps K] [--warmup W]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fv3net_amd.forest import ForestInput, ForestModel, ForestOutput, ForestSpec  # noqa: E402

NZ = 79
HBM_ROW_GATHER_TBS = (5.5, 6.0)    # ~1.2-KB rows from HBM into registers (MI355X_MICROARCH, "Indexed rows")
MALL_ROW_GATHER_TBS = (7.4, 8.6)   # rows of a table that fits the 256 MiB Infinity Cache


def complete_forest(n_trees, depth, n_feat, n_out, inputs, rng):
    """Complete binary trees in sklearn's numbering (depth-first, children after their parent)."""
    n_nodes = 2 ** (depth + 1) - 1
    left, right, leaf = np.full(n_nodes, -1, np.int32), np.full(n_nodes, -1, np.int32), np.zeros(n_nodes, bool)
    nxt = [1]

    def build(i, d):
        if d == depth:
            leaf[i] = True
            return
        left[i] = nxt[0]; nxt[0] += 1
        build(left[i], d + 1)
        right[i] = nxt[0]; nxt[0] += 1
        build(right[i], d + 1)

    build(0, 0)
    n_leaves = int(leaf.sum())
    feats, thrs, rows = [], [], []
    for t in range(n_trees):
        f = rng.integers(0, n_feat, n_nodes).astype(np.int32)
        f[leaf] = -2
        pick = inputs[rng.integers(0, inputs.shape[0], n_nodes), np.maximum(f, 0)]
        thrs.append(np.where(leaf, -2.0, pick).astype(np.float32))
        feats.append(f)
        r = np.full(n_nodes, -1, np.int32)
        r[leaf] = t * n_leaves + np.arange(n_leaves, dtype=np.int32)
        rows.append(r)
    trees = {
        "node_offset": np.arange(n_trees + 1, dtype=np.int64) * n_nodes,
        "children_left": np.tile(left, n_trees), "children_right": np.tile(right, n_trees),
        "feature": np.concatenate(feats), "threshold": np.concatenate(thrs),
        "missing_go_to_left": np.ones(n_nodes * n_trees, np.uint8), "leaf_row": np.concatenate(rows),
        "leaf_values": rng.normal(size=(n_trees * n_leaves, n_out)),
    }
    return trees


def workload(name, n_cols, n_trees, depth, outputs, rng, dev, trees=None):
    scalars = 2 if outputs == ("dQ1", "dQ2") else 1
    n_feat = 2 * NZ + scalars
    n_out = NZ * len(outputs)
    x = rng.normal(size=(n_cols, n_feat)).astype(np.float32)
    if trees is None:
        trees = complete_forest(n_trees, depth, n_feat, n_out, x[:4096], rng)
    inputs = [ForestInput("T", NZ), ForestInput("q", NZ)] + [ForestInput(f"s{i}", 1) for i in range(scalars)]
    spec = ForestSpec(inputs, [ForestOutput(o, NZ) for o in outputs], trees, rng.normal(size=n_out), rng.uniform(0.5, 2, n_out))
    xt = torch.from_numpy(np.ascontiguousarray(x.T)).to(dev)  # [feature, column], the model's native [z, ...] layout
    src = {"T": xt[:NZ], "q": xt[NZ:2 * NZ]}
    for i in range(scalars):
        src[f"s{i}"] = xt[2 * NZ + i]
    return spec, src, x, trees


def time_gpu(model, src, steps, warmup):
    for _ in range(warmup):
        model.predict(src)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        model.predict(src)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / steps


_TRAINED = {}


def sklearn_baseline(n_trees, depth, n_feat, n_out, X, reps, rng):
    """sklearn predict in this process on a trained forest of the same T, depth and n_out (n_jobs=None, the reference's
    path, and n_jobs=16).  Training: 16 jobs, 16 features per split (the predict cost does not depend on it)."""
    from sklearn.ensemble import RandomForestRegressor

    key = (n_trees, depth, n_feat, n_out)
    if key not in _TRAINED:
        n_train = max(4 * 2 ** depth, 2048)
        Xt = rng.normal(size=(n_train, n_feat)).astype(np.float32)
        w = rng.normal(size=(n_feat, n_out))
        yt = np.tanh(Xt @ w / np.sqrt(n_feat)) + 0.1 * rng.normal(size=(n_train, n_out))
        t0 = time.perf_counter()
        forest = RandomForestRegressor(n_estimators=n_trees, max_depth=depth, max_features=min(16, n_feat), n_jobs=16,
                                       random_state=0).fit(Xt, yt)
        _TRAINED[key] = (forest, time.perf_counter() - t0)
    forest, train_s = _TRAINED[key]
    out = {"train_s": round(train_s, 1), "trained_depth_mean": float(np.mean([e.get_depth() for e in forest.estimators_]))}
    for jobs in (None, 16):
        forest.set_params(n_jobs=jobs)
        forest.predict(X[:256])
        t0 = time.perf_counter()
        for _ in range(reps):
            forest.predict(X)
        out[f"ms_n_jobs_{jobs}"] = round((time.perf_counter() - t0) / reps * 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    plans = [("W1", 13824, 100, 13, ("dQ1", "dQ2"), 2), ("W2", 147456, 100, 13, ("dQ1", "dQ2"), 1),
             ("W3", 13824, 1, 13, ("dQ1",), 3)]
    if args.quick:
        plans = plans[:1]
    trees = None
    for name, n_cols, n_trees, depth, outputs, reps in plans:
        spec, src, x, trees_w = workload(name, n_cols, n_trees, depth, outputs, rng, dev,
                                         trees=trees if name == "W2" else None)
        if name == "W1":
            trees = trees_w
        model = ForestModel(spec, device=dev)
        ms = time_gpu(model, src, args.steps, args.warmup)
        n_out = spec.n_out_features
        gathered = n_cols * n_trees * n_out * 8
        row = {
            "workload": name, "columns": n_cols, "trees": n_trees, "depth": depth, "features": spec.n_in_features,
            "outputs": n_out, "ms": round(ms, 4), "columns_per_s": round(n_cols / ms * 1e3),
            "leaf_table_MB": round(spec.leaf_table_bytes / 1e6, 1), "gathered_leaf_GB": round(gathered / 1e9, 3),
            "gathered_TB_per_s": round(gathered / ms / 1e9, 3),
            "row_gather_reference_TB_per_s": MALL_ROW_GATHER_TBS if spec.leaf_table_bytes <= 256 << 20 else HBM_ROW_GATHER_TBS,
        }
        if not args.quick:
            sk = sklearn_baseline(n_trees, depth, spec.n_in_features, n_out, x, reps, rng)
            row["sklearn"] = sk
            row["speedup_vs_sklearn_n_jobs_None"] = round(sk["ms_n_jobs_None"] / ms, 1)
        print(json.dumps(row), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
