#!/usr/bin/env python3
"""Attribution microbench: time feature_contributions() and score() on the
same resident matrix in one process.

Usage: python tools/explain_bench.py [--rows 5000000] [--features 32]
       [--trees 1000] [--dtype bf16] [--reps 5] [--warmup 2] [--extended]
       [--layout row|pitched|feature] [--copy-first] [--method path|shap]

--method is feature_contributions' own: "path" (default) times the
path-length decomposition, "shap" the exact TreeSHAP kernel (standard
forests only; expect orders of magnitude below "path", it visits every
leaf of every tree).

--layout and --copy-first are those of tools/score_bench.py: the matrix as
packed rows, as the first d columns of a matrix 8 columns wider, or as a
[d, N] buffer seen through .T; --copy-first times .contiguous() plus the
call, not the call on the view.

Both calls are warmed up, every repetition is bracketed by device
synchronises, the two calls alternate (same process, same matrix, same
model) and the MEDIAN repetition is reported. Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, X):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(X)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--max-samples", type=int, default=256)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--extended", action="store_true")
    ap.add_argument("--extension-level", type=int, default=None)
    ap.add_argument("--layout", choices=["row", "pitched", "feature"],
                    default="row")
    ap.add_argument("--copy-first", action="store_true")
    ap.add_argument("--method", choices=["path", "shap"], default="path")
    args = ap.parse_args()
    if args.method == "shap" and args.extended:
        raise SystemExit("--method shap is defined for standard forests only")

    from isolation_forest_amd import ExtendedIsolationForest, IsolationForest
    from isolation_forest_amd.ops import load_extension

    load_extension()
    if not torch.cuda.is_available():
        raise SystemExit("explain_bench needs a GPU; it has no CPU fallback")
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16,
             "fp32": torch.float32}[args.dtype]
    X = torch.randn((args.rows, args.features), device=dev,
                    generator=g).to(dtype)
    if args.layout == "pitched":
        wide = torch.empty((args.rows, args.features + 8), device=dev,
                           dtype=dtype)
        wide[:, :args.features] = X
        X = wide[:, :args.features]
    elif args.layout == "feature":
        X = X.T.contiguous().T

    cls = ExtendedIsolationForest if args.extended else IsolationForest
    kw = {}
    if args.extended and args.extension_level is not None:
        kw["extensionLevel"] = args.extension_level
    model = cls(numEstimators=args.trees, maxSamples=float(args.max_samples),
                randomSeed=3, **kw).fit(X)

    def rows(x):
        return x.contiguous() if args.copy_first else x

    def explain(x):
        return model.feature_contributions(rows(x), method=args.method)

    def score(x):
        return model.score(rows(x))

    for _ in range(args.warmup):
        explain(X)
        score(X)
    t_explain, t_score = [], []
    for _ in range(args.reps):
        dt, contrib = timed(explain, X)
        t_explain.append(dt)
        dt, scores = timed(score, X)
        t_score.append(dt)
    te = statistics.median(t_explain)
    ts = statistics.median(t_score)
    print(json.dumps({
        "kernel": ("explain_extended" if args.extended
                   else "shap" if args.method == "shap" else "explain"),
        "method": args.method,
        "ext_level": args.extension_level if args.extended else None,
        "rows": args.rows, "features": args.features, "trees": args.trees,
        "max_samples": args.max_samples, "dtype": args.dtype,
        "layout": args.layout, "copy_first": args.copy_first,
        "reps": args.reps, "warmup": args.warmup,
        "explain_ms_median": round(te * 1e3, 3),
        "explain_ms_all": [round(t * 1e3, 3) for t in t_explain],
        "explain_rows_per_s": round(args.rows / te),
        "score_ms_median": round(ts * 1e3, 3),
        "score_ms_all": [round(t * 1e3, 3) for t in t_score],
        "score_rows_per_s": round(args.rows / ts),
        "explain_over_score_time": round(te / ts, 3),
        "expected_path_length": model.expected_path_length,
        "sample_contributions": [
            round(float(v), 6) for v in contrib[0, :4].float().cpu()],
        "sample_scores": [round(float(v), 6) for v in scores[:4].float().cpu()],
    }))


if __name__ == "__main__":
    main()
