#!/usr/bin/env python3
"""Large-bag attribution microbench: `model.feature_contributions` of a
standard forest past the 15-bit node ids on the deep explain route, at its
default stage and with each IFA_EXPLAIN_DEEP_STAGE of --stages (2:
practically every record from global memory; a trailing g: accumulators in
the output, IFA_EXPLAIN_FORCE_GLOBAL_ACC=1), and with IFA_EXPLAIN_DEEP=0
(the CPU oracle behind a host copy), alternated inside one process.

Usage: python tools/explain_deep_bench.py [--rows 5000000] [--features 32]
       [--max-samples 65536] [--trees 100] [--dtype bf16] [--repeats 5]
       [--calls 3] [--cpu-rows 20000] [--stages 2] [--out FILE]
       [--extended [--extension-level L]]

--extended fits an ExtendedIsolationForest instead and times the deep EIF
route (explain_extended_deep) the same way.

Fits one IsolationForest on a resident [N, d] CUDA matrix (contamination 0),
explains once per variant to make and cache the packs and tables (timed as
`first_call_s`), then times `--repeats` windows per variant, each ending in a
device synchronise, alternating the variants. The GPU variants run `--calls`
calls a window on all rows; the CPU path runs one call on the first
`--cpu-rows` rows (`--cpu-rows 0` leaves it out) and is also reported per
million rows. The results of the variants are compared bit for bit on the
CPU rows. Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"deep": {"IFA_EXPLAIN_DEEP": "1"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--max-samples", type=int, default=65536)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3,
                    help="GPU explain calls per timed window")
    ap.add_argument("--cpu-rows", type=int, default=20000)
    ap.add_argument("--stages", default="2",
                    help="forced stages to time beside the default, a,b,...; "
                         "a trailing g (1024g, or g alone for the default "
                         "stage) adds IFA_EXPLAIN_FORCE_GLOBAL_ACC=1")
    ap.add_argument("--extended", action="store_true",
                    help="an ExtendedIsolationForest (explain_extended_deep)")
    ap.add_argument("--extension-level", type=int, default=None,
                    help="with --extended; default: fully extended")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    for st in filter(None, args.stages.split(",")):
        env = {"IFA_EXPLAIN_DEEP": "1"}
        if st.endswith("g"):
            env["IFA_EXPLAIN_FORCE_GLOBAL_ACC"] = "1"
        if st.rstrip("g"):
            env["IFA_EXPLAIN_DEEP_STAGE"] = str(int(st.rstrip("g")))
        VARIANTS[f"deep_stage{st}"] = env
    VARIANTS["cpu"] = {"IFA_EXPLAIN_DEEP": "0"}

    from isolation_forest_amd import ExtendedIsolationForest, IsolationForest
    from isolation_forest_amd.ops import gpu_engine, load_extension

    load_extension()
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16,
             "fp32": torch.float32}[args.dtype]
    X = torch.randn((args.rows, args.features), device=dev,
                    generator=g).to(dtype)
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    kw = dict(numEstimators=args.trees, maxSamples=float(args.max_samples),
              randomSeed=3)
    if args.extended and args.extension_level is not None:
        kw["extensionLevel"] = args.extension_level
    model = (ExtendedIsolationForest if args.extended
             else IsolationForest)(**kw).fit(X)
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    forest = model.forest
    print(f"fit {t_fit:.1f}s, nodes/tree max {int(forest.node_count.max())}",
          file=sys.stderr, flush=True)
    names = [v for v in VARIANTS if v != "cpu" or args.cpu_rows > 0]
    n_cpu = min(args.cpu_rows, args.rows) if args.cpu_rows > 0 else 20000
    rows_of = {v: X[:n_cpu] if v == "cpu" else X for v in names}

    def explain(variant, calls=1):
        """seconds per call over a window of `calls` synchronised at its end"""
        os.environ.pop("IFA_EXPLAIN_DEEP_STAGE", None)
        os.environ.pop("IFA_EXPLAIN_FORCE_GLOBAL_ACC", None)
        os.environ.update(VARIANTS[variant])
        want = "cpu" if variant == "cpu" else "deep"
        assert gpu_engine.large_explain_route(
            forest, args.features, dtype) == want, variant
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(calls):
            c = model.feature_contributions(rows_of[variant])
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / calls, c

    first, head, times = {}, {}, {v: [] for v in names}
    for v in names:
        first[v], c = explain(v)
        head[v] = c[:n_cpu].view(torch.int32).clone()
        del c
        print(f"{v}: first call {first[v]:.2f}s", file=sys.stderr, flush=True)
    same = all(bool(torch.equal(head[names[0]], head[v])) for v in names[1:])
    del head
    for _ in range(args.repeats):
        for v in names:
            dt, _ = explain(v, 1 if v == "cpu" else args.calls)
            times[v].append(dt)
            print(f"{v}: {dt * 1e3:.1f} ms", file=sys.stderr, flush=True)

    def stats(v, rows):
        med = statistics.median(v)
        return {"rows": rows, "ms": [round(x * 1e3, 2) for x in v],
                "median_ms": round(med * 1e3, 2),
                "spread_ms": round((max(v) - min(v)) * 1e3, 2),
                "median_ms_per_million_rows": round(med * 1e9 / rows, 2),
                "spread_ms_per_million_rows": round(
                    (max(v) - min(v)) * 1e9 / rows, 2)}

    rec_bytes = {
        "/".join(map(str, key[2])): sum(
            a.numel() * a.element_size()
            for a in (aos, extra.get("payload")) if a is not None)
        for key, (aos, _, extra) in model._gpu_forest_cache.items()}
    out = {
        "tool": "explain_deep_bench", "rows": args.rows,
        "extended": args.extended,
        "hyperplane_width": int(getattr(forest, "nnz", 1)),
        "features": args.features, "max_samples": int(forest.num_samples),
        "trees": int(forest.num_trees), "dtype": args.dtype,
        "calls_per_window": args.calls, "fit_s": round(t_fit, 2),
        "nodes_per_tree_max": int(forest.node_count.max()),
        "nodes_per_tree_mean": round(float(forest.node_count.mean()), 1),
        "array_width": int(forest.feature.shape[1]),
        "bitwise_equal_on_cpu_rows": same,
        "first_call_s": {k: round(v, 3) for k, v in first.items()},
        "record_bytes": rec_bytes,
    }
    for v in names:
        out[v] = stats(times[v], int(rows_of[v].shape[0]))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
