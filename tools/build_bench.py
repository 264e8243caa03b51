#!/usr/bin/env python3
"""Tree-build microbench: time the `bag+build` phase of fit().

Usage: python tools/build_bench.py [--rows 2000000] [--features 32]
       [--max-samples 1000000] [--trees 64] [--dtype bf16]
       [--kind standard|extended] [--extension-level L]
       [--threads-sweep 128,256,512]

Fits one estimator on a resident [N, d] CUDA matrix and reports the phase
fit() times as `bag+build`, split into the host-side draws
(cpu_engine.sample_bags + feature_subsets) and the rest, which is the tree
build itself with its uploads and downloads: the HIP builders on a GPU route,
`X.float().cpu()` plus the CPU oracle where fit() falls back to it. The tool
only uses the public estimators, so it runs unchanged on older commits.

--threads-sweep re-times one launch of the large-bag binding alone (the
first chunk of the same bags, outputs left on the device) at the given block
sizes, on commits that have the large-bag builders.

Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--max-samples", type=int, default=1_000_000)
    ap.add_argument("--trees", type=int, default=64)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--kind", choices=["standard", "extended"],
                    default="standard")
    ap.add_argument("--extension-level", type=int, default=None)
    ap.add_argument("--threads-sweep", default="")
    args = ap.parse_args()

    from isolation_forest_amd import ExtendedIsolationForest, IsolationForest
    from isolation_forest_amd.core import cpu_engine
    from isolation_forest_amd.ops import gpu_engine, load_extension

    load_extension()
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16,
             "fp32": torch.float32}[args.dtype]
    X = torch.empty((args.rows, args.features), device=dev, dtype=dtype)
    step = max(1, min(args.rows, 64_000_000))
    for lo in range(0, args.rows, step):
        hi = min(args.rows, lo + step)
        X[lo:hi] = torch.randn((hi - lo, args.features), device=dev,
                               generator=g).to(dtype)
    torch.cuda.synchronize()

    # time the host-side draws inside fit() and keep what they returned
    draws = {"s": 0.0}
    kept = {}

    def timed(name):
        fn = getattr(cpu_engine, name)

        def wrapper(*a, **kw):
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            draws["s"] += time.perf_counter() - t0
            kept[name] = out
            return out

        setattr(cpu_engine, name, wrapper)

    timed("sample_bags")
    timed("feature_subsets")

    cls = ExtendedIsolationForest if args.kind == "extended" else IsolationForest
    kw = {}
    if args.kind == "extended" and args.extension_level is not None:
        kw["extensionLevel"] = args.extension_level
    est = cls(numEstimators=args.trees, maxSamples=float(args.max_samples),
              randomSeed=3, **kw)
    os.environ["IFA_TIMING_SYNC"] = "1"
    t0 = time.perf_counter()
    model = est.fit(X)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    phase_s = float(model.fit_metrics["bag+build"])
    n = int(model.forest.num_samples)
    large = hasattr(gpu_engine, "build_forest_large")
    if n <= 16384:
        route = "gpu-lds"
    else:
        route = "gpu-large" if large else "cpu-oracle"
    out = {
        "tool": "build_bench", "kind": args.kind,
        "ext_level": (getattr(model.forest, "extension_level", None)
                      if args.kind == "extended" else None),
        "rows": args.rows, "features": args.features, "max_samples": n,
        "trees": args.trees, "dtype": args.dtype, "route": route,
        "fit_s": round(t_fit, 4),
        "bag_build_s": round(phase_s, 4),
        "host_draws_s": round(draws["s"], 4),
        "build_s": round(phase_s - draws["s"], 4),
        "build_ms_per_tree": round((phase_s - draws["s"]) * 1e3 / args.trees, 3),
        "draws_ms_per_tree": round(draws["s"] * 1e3 / args.trees, 3),
        "nodes_per_tree": round(float(model.forest.node_count.mean()), 1),
        "height_limit": int(math.ceil(math.log2(max(n, 2)))),
    }

    if args.threads_sweep and large and n > 16384:
        # one launch of the binding, outputs left on the device
        import numpy as np

        ext = load_extension()
        rp = model._resolved
        H = out["height_limit"]
        extended = args.kind == "extended"
        nnz = min(rp.extension_level + 1, rp.num_features) if extended else 1
        max_nodes = 2 ** (H + 1) - 1 if extended else 2 * n - 1
        per_tree = 16 * n + (28 + (8 * nnz if extended else 0)) * max_nodes
        Tk = gpu_engine._large_chunk_trees(args.trees, per_tree, None)
        bag_t = torch.from_numpy(
            np.ascontiguousarray(kept["sample_bags"][:Tk])).to(dev)
        fs_t = torch.from_numpy(np.ascontiguousarray(
            kept["feature_subsets"][:Tk], dtype=np.int32)).to(dev)
        lut = gpu_engine._leaf_lut(n, X.device)
        sweep = {}
        for th in [int(v) for v in args.threads_sweep.split(",")]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if extended:
                res = ext.build_extended_forest_large(
                    X, bag_t, fs_t, 3, 0, lut, nnz, max_nodes, H, th)
            else:
                res = ext.build_forest_large(
                    X, bag_t, fs_t, 3, 0, lut, max_nodes, H, th)
            torch.cuda.synchronize()
            sweep[str(th)] = round((time.perf_counter() - t0) * 1e3, 3)
            del res
        out["sweep_trees_per_launch"] = Tk
        out["sweep_launch_ms"] = sweep

    print(json.dumps(out))


if __name__ == "__main__":
    main()
