#!/usr/bin/env python3
"""Large-bag TreeSHAP microbench: `model.shap_values` of a standard forest
past the 15-bit node ids, at several row counts, three ways, alternated
inside one process:

  deep  the entry-parallel kernel (shap_forest_deep_kernel)
  row   IFA_SHAP_DEEP_SPLIT=row: shap_forest_kernel, one row per thread, its
        table read from global memory (only when max_m <= 16)
  cpu   IFA_SHAP_DEEP=0: the CPU oracle, one call on --cpu-rows rows,
        reported per row and SCALED to each row count (labelled as such)

Usage: python tools/shap_deep_bench.py [--rows 256,1000,10000,100000]
       [--fit-rows 200000] [--features 32] [--max-samples 65536]
       [--trees 100] [--dtype bf16] [--repeats 3] [--calls 3]
       [--cpu-rows 8] [--out FILE]

Fits one IsolationForest on a resident CUDA matrix, makes the packs with one
call per variant (timed as `first_call_s`), then for every row count warms
each GPU variant once and times `--repeats` windows of `--calls` calls, each
window ending in a device synchronise, alternating the variants. The three
results are compared bit for bit on the CPU rows. Prints one JSON line (and
writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"deep": {}, "row": {"IFA_SHAP_DEEP_SPLIT": "row"},
            "cpu": {"IFA_SHAP_DEEP": "0"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="256,1000,10000,100000")
    ap.add_argument("--fit-rows", type=int, default=200_000)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--max-samples", type=int, default=65536)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3,
                    help="GPU calls per timed window")
    ap.add_argument("--cpu-rows", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    row_counts = [int(r) for r in args.rows.split(",")]

    from isolation_forest_amd import IsolationForest
    from isolation_forest_amd.core import cpu_engine
    from isolation_forest_amd.ops import gpu_engine, load_extension

    ext = load_extension()
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16,
             "fp32": torch.float32}[args.dtype]
    n_all = max(args.fit_rows, max(row_counts))
    X = torch.randn((n_all, args.features), device=dev, generator=g).to(dtype)
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    model = IsolationForest(
        numEstimators=args.trees, maxSamples=float(args.max_samples),
        randomSeed=3).fit(X[:args.fit_rows])
    torch.cuda.synchronize()
    t_fit = time.perf_counter() - t0
    forest = model.forest
    t0 = time.perf_counter()
    tabs = cpu_engine.shap_tables(forest)
    t_tabs = time.perf_counter() - t0
    max_m = int(tabs["max_m"])
    kind = gpu_engine._row_kind(dtype)
    cfg = ext.shap_deep_cfg(kind, args.features, max_m)
    print(f"fit {t_fit:.1f}s, tables {t_tabs:.1f}s, leaves "
          f"{len(tabs['leaf_L'])}, max_m {max_m}, cfg {cfg}",
          file=sys.stderr, flush=True)
    assert gpu_engine.large_shap_route(forest, args.features, dtype) == "deep"
    names = ["deep"] + (["row"] if max_m <= 16 else [])

    def shap(variant, rows, calls=1):
        """seconds per call over a window of `calls` synchronised at its end"""
        for env in VARIANTS.values():
            for k in env:
                os.environ.pop(k, None)
        os.environ.update(VARIANTS[variant])
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(calls):
            c = model.shap_values(rows)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / calls, c

    n_cpu = max(1, args.cpu_rows)
    first, head = {}, {}
    for v in names:
        first[v], c = shap(v, X[:n_cpu])
        head[v] = c.view(torch.int32).clone()
        print(f"{v}: first call {first[v]:.2f}s", file=sys.stderr, flush=True)
    cpu_s = None
    if args.cpu_rows > 0:
        cpu_s, c = shap("cpu", X[:n_cpu])
        head["cpu"] = c.view(torch.int32).clone()
        print(f"cpu: {n_cpu} rows {cpu_s:.2f}s", file=sys.stderr, flush=True)
    same = all(bool(torch.equal(head["deep"], h)) for h in head.values())

    def stats(v):
        med = statistics.median(v)
        return {"ms": [round(x * 1e3, 2) for x in v],
                "median_ms": round(med * 1e3, 2),
                "spread_ms": round((max(v) - min(v)) * 1e3, 2)}

    per_n = {}
    for n in row_counts:
        rows = X[:n]
        times = {v: [] for v in names}
        for v in names:
            shap(v, rows)  # warm this shape
        for _ in range(args.repeats):
            for v in names:
                dt, _ = shap(v, rows, args.calls)
                times[v].append(dt)
                print(f"N={n} {v}: {dt * 1e3:.1f} ms", file=sys.stderr,
                      flush=True)
        per_n[str(n)] = {v: stats(times[v]) for v in names}
        if cpu_s is not None:
            per_n[str(n)]["cpu_scaled_from_%d_rows_ms" % n_cpu] = round(
                cpu_s / n_cpu * n * 1e3, 1)

    out = {
        "tool": "shap_deep_bench", "features": args.features,
        "max_samples": int(forest.num_samples), "trees": int(forest.num_trees),
        "dtype": args.dtype, "calls_per_window": args.calls,
        "fit_s": round(t_fit, 2), "shap_tables_s": round(t_tabs, 2),
        "leaves": int(len(tabs["leaf_L"])), "entries": int(len(tabs["ent_z"])),
        "max_m": max_m,
        "cfg_G_acc_lds_keys_lds": [int(cfg[0]), bool(cfg[1]), bool(cfg[2])],
        "nodes_per_tree_max": int(forest.node_count.max()),
        "array_width": int(forest.feature.shape[1]),
        "bitwise_equal_on_cpu_rows": same,
        "first_call_s": {k: round(v, 3) for k, v in first.items()},
        "cpu_rows": n_cpu if cpu_s is not None else 0,
        "cpu_s": None if cpu_s is None else round(cpu_s, 3),
        "table_bytes": {
            "/".join(map(str, key[2])): aos.numel() * aos.element_size()
            for key, (aos, _, _) in model._gpu_forest_cache.items()},
        "rows": per_n,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
