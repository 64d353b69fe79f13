"""Growing random-forest trees on the device: ``forest_train.ForestTrainer.grow`` on resident synthetic
C48-like data -- 160 inputs, 158 outputs, depth 13, bootstrap -- next to sklearn's ``RandomForestRegressor.fit`` of the same
number of trees on the same arrays in the same run, at ``n_jobs=1`` and at 16 (the CPU allowance of a GPU job).

  c48    n = 13 824   (one C48 time step)
  c384   n = 147 456  (the rows of one C384 tile)

Per configuration, one JSON line: device milliseconds per tree (HIP events around whole ``grow`` calls, the per-level readback
and the host's renumbering included, after one warm-up tree), sklearn's seconds per tree at both job counts, and for the scan
launches (``ft_scan_kernel`` + ``ft_best_kernel``, timed with events in a second pass that runs every level's phases as
separate calls) their share of the tree's time and their rate in algorithmic bytes -- in-bag positions x F x O x 8 per level
that searches for splits -- to set beside the ~5 TB/s at which ``forest_sum_kernel`` gathers rows of the same length.  The
one-off presort and upload (``ForestTrainer(...)``) is reported separately.

    python3 benchmarks/forest_train.py [--configs c48,c384] [--trees N] [--sklearn-trees N] [--skip-sklearn]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fv3net_amd import forest_train  # noqa: E402

CONFIGS = {"c48": 13824, "c384": 147456}
N_IN, N_OUT, DEPTH = 160, 158, 13


def synthetic(n, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, N_IN)).astype(np.float32)
    w = rng.normal(size=(N_IN, N_OUT)) / np.sqrt(N_IN)
    y = np.tanh(X.astype(np.float64) @ w) + 0.1 * rng.normal(size=(n, N_OUT))
    return X, (y - y.mean(axis=0)) / y.std(axis=0)


def device_trees(trainer, n, seeds, scan_events=None):
    """Milliseconds per tree over ``seeds`` (device events around the whole calls)."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    nodes, scan_bytes = 0, 0
    for seed in seeds:
        tree = trainer._grow(forest_train.bootstrap_counts(seed, n, n), DEPTH, 2, 1, scan_events=scan_events)
        nodes += tree["feature"].shape[0]
        scan_bytes += trainer.scan_bytes
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / len(seeds), nodes / len(seeds), scan_bytes / len(seeds)


def sklearn_seconds_per_tree(X, y, trees, jobs):
    from sklearn.ensemble import RandomForestRegressor

    t0 = time.perf_counter()
    RandomForestRegressor(n_estimators=trees, max_depth=DEPTH, random_state=0, n_jobs=jobs).fit(X, y)
    return (time.perf_counter() - t0) / trees


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c48,c384")
    ap.add_argument("--trees", type=int, default=4, help="device trees timed per configuration")
    ap.add_argument("--sklearn-trees", type=int, default=0, help="0: 16 for 16 jobs; for one job 4 at c48 and 1 at c384")
    ap.add_argument("--skip-sklearn", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    for name in args.configs.split(","):
        n = CONFIGS[name]
        X, y = synthetic(n)
        t0 = time.perf_counter()
        trainer = forest_train.ForestTrainer(X, y, device=dev)
        torch.cuda.synchronize()
        setup_s = time.perf_counter() - t0
        seeds = forest_train.tree_seeds(0, args.trees + 1)
        device_trees(trainer, n, seeds[:1])  # warm-up: sizes the per-node buffers
        ms, nodes, scan_bytes = device_trees(trainer, n, seeds[1:])
        events = []
        ms_split, _, _ = device_trees(trainer, n, seeds[1:], scan_events=events)
        scan_ms = sum(a.elapsed_time(b) for a, b in events) / args.trees
        out = {"config": name, "n": n, "inputs": N_IN, "outputs": N_OUT, "max_depth": DEPTH, "trees_timed": args.trees,
               "setup_s": round(setup_s, 3), "device_ms_per_tree": round(ms, 2), "nodes_per_tree": round(nodes, 1),
               "levels": trainer.levels, "scan_ms_per_tree": round(scan_ms, 2), "scan_share": round(scan_ms / ms_split, 3),
               "device_ms_per_tree_phases_split": round(ms_split, 2), "scan_algorithmic_GB_per_tree": round(scan_bytes / 1e9, 2),
               "scan_algorithmic_TB_per_s": round(scan_bytes / (scan_ms * 1e-3) / 1e12, 3), "forest_sum_kernel_TB_per_s": 5.0}
        if not args.skip_sklearn:
            many = args.sklearn_trees or 16
            one = args.sklearn_trees or (4 if n <= 20000 else 1)
            out["sklearn_trees_16_jobs"], out["sklearn_trees_1_job"] = many, one
            out["sklearn_s_per_tree_16_jobs"] = round(sklearn_seconds_per_tree(X, y, many, 16), 3)
            out["sklearn_s_per_tree_1_job"] = round(sklearn_seconds_per_tree(X, y, one, 1), 3)
            out["speedup_vs_16_jobs"] = round(out["sklearn_s_per_tree_16_jobs"] / (ms * 1e-3), 2)
            out["speedup_vs_1_job"] = round(out["sklearn_s_per_tree_1_job"] / (ms * 1e-3), 2)
        print(json.dumps(out), flush=True)
        del trainer
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
