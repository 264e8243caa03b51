#!/usr/bin/env python3
"""Large-bag scoring microbench: `model.score` of a standard forest past the
15-bit node ids, on the default route and with IFA_SCORE_DEEP=0 (the wide
int4 kernel), alternated inside one process.

Usage: python tools/score_deep_bench.py [--rows 5000000] [--features 32]
       [--max-samples 65536] [--trees 100] [--dtype bf16] [--repeats 5]
       [--extended [--extension-level L] [--phases 4,2,1]] [--out FILE]

--extended scores an ExtendedIsolationForest instead (fully extended unless
--extension-level says otherwise); --phases adds one deep route per listed
IFA_EIF_DEEP_PHASE value to the alternation, each with the stage that phase
leaves room for.

Fits one IsolationForest on a resident [N, d] CUDA matrix (contamination 0,
so fit() itself scores nothing), scores once per route to make and cache the
packs (timed as `first_call_s`: host pack, upload, reorder, one score), then
times `--repeats` windows of `--calls` calls per route, each window ending
in a device synchronise, alternating the two routes. The
outputs of the two routes are compared bit for bit. Reports the device bytes
of each route's records. Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--max-samples", type=int, default=65536)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp32"], default="bf16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10,
                    help="score calls per timed window")
    ap.add_argument("--extended", action="store_true")
    ap.add_argument("--extension-level", type=int, default=None)
    ap.add_argument("--phases", default="",
                    help="--extended: forced trees per phase to time as well")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

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

    def score(route, calls=1):
        """seconds per call over a window of `calls` synchronised at its end"""
        os.environ["IFA_SCORE_DEEP"] = "0" if route == "wide" else "1"
        os.environ.pop("IFA_EIF_DEEP_PHASE", None)
        if route.startswith("deep_ph"):
            os.environ["IFA_EIF_DEEP_PHASE"] = route[len("deep_ph"):]
        assert gpu_engine.large_score_route(
            forest, args.features, dtype) == route[:4], route
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(calls):
            s = model.score(X)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / calls, s

    routes = ["deep", "wide"] + [f"deep_ph{p}" for p in
                                 args.phases.split(",") if p]
    first, outs, times = {}, {}, {r: [] for r in routes}
    cfgs = {}
    for route in routes:
        first[route], outs[route] = score(route)
        if args.extended and route != "wide":
            cfgs[route] = list(load_extension().score_eif_deep_cfg(
                gpu_engine._row_kind(dtype), args.features, forest.nnz))
        print(f"{route}: first call {first[route]:.2f}s", file=sys.stderr,
              flush=True)
    same = all(bool(torch.equal(o.view(torch.int32),
                                outs["wide"].view(torch.int32)))
               for o in outs.values())
    del outs
    for _ in range(args.repeats):
        for route in routes:
            dt, _ = score(route, args.calls)
            times[route].append(dt)
            print(f"{route}: {dt * 1e3:.1f} ms", file=sys.stderr, flush=True)

    rec_bytes = {}
    for key, (aos, _, extra) in model._gpu_forest_cache.items():
        name = key[2] if isinstance(key[2], str) else "_".join(
            str(k) for k in key[2] if isinstance(k, (str, int)))
        # extended packs: the hyperplane entries travel beside the records
        rec_bytes[name if args.extended else key[2][0]] = sum(
            a.numel() * a.element_size()
            for a in (aos, *(extra.get(k) for k in ("hyper", "hidx", "hw")))
            if a is not None)
    n, T = int(forest.num_samples), int(forest.num_trees)

    def stats(v):
        return {"ms": [round(x * 1e3, 2) for x in v],
                "median_ms": round(statistics.median(v) * 1e3, 2),
                "spread_ms": round((max(v) - min(v)) * 1e3, 2)}

    out = {
        "tool": "score_deep_bench", "rows": args.rows,
        "features": args.features, "max_samples": n, "trees": T,
        "dtype": args.dtype, "calls_per_window": args.calls,
        "fit_s": round(t_fit, 2),
        "nodes_per_tree_max": int(forest.node_count.max()),
        "nodes_per_tree_mean": round(float(forest.node_count.mean()), 1),
        "array_width": int(forest.feature.shape[1]),
        "bitwise_equal": same,
        "first_call_s": {k: round(v, 3) for k, v in first.items()},
        **{r: stats(times[r]) for r in routes},
        "speedup_median": round(statistics.median(times["wide"])
                                / statistics.median(times["deep"]), 2),
        "record_bytes": rec_bytes,
        **({"extended": True, "nnz": int(forest.nnz),
            "rpt_phase_stage": cfgs} if args.extended else {}),
        "record_bytes_formula": {"deep_8_M_Tpad": None,
                                 "wide_32_n_T": 32 * n * T},
    }
    deep_key = [k for k in model._gpu_forest_cache if k[2][0] == "deep"]
    if deep_key:
        aos = model._gpu_forest_cache[deep_key[0]][0]
        out["record_bytes_formula"]["deep_8_M_Tpad"] = (
            8 * aos.shape[1] * aos.shape[0])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
