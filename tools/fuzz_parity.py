#!/usr/bin/env python3
"""Differential GPU<->CPU fuzzer.

Random configurations of (rows, features, subsampling, tree count,
extension level, row dtype f32/bf16/fp16, row layout packed/pitched/
feature-major, bootstrap, data pathologies):
build on the GPU and on the CPU oracle (which sees the upcast matrix), demand BITWISE forest equality; score on both, demand
the routing contract (bitwise for standard/sparse walks, knife-edge
tolerance for reassociated dense dots). Exits non-zero on the first
divergence with a repro line.

    python tools/fuzz_parity.py [--iters 30] [--seed 0]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.ops import gpu_engine
from isolation_forest_amd.utils.params import ResolvedParams


def _knife_edge_explained(forest, x_row: np.ndarray) -> bool:
    """True when at least one internal node on the row's oracle walk (any
    tree) sits within reassociation error of its offset — i.e. the dense
    kernels' reordered float32 dot could legitimately flip the branch.
    A kernel BUG (wrong weights/indexing) flips rows at large margins and
    stays unexplained."""
    eps = 1.1920929e-07
    nnz = forest.nnz
    for t in range(forest.num_trees):
        cur = 0
        while forest.feature[t, cur] >= 0:
            idx = forest.hyper_idx[t, cur, :nnz]
            w = forest.hyper_w[t, cur, :nnz]
            terms = (w * x_row[idx]).astype(np.float32)
            dot = np.float32(0.0)
            for v in terms:
                dot = np.float32(dot + v)
            off = float(forest.value[t, cur])
            bound = (8.0 * max(nnz, 4) * eps
                     * (float(np.abs(terms).sum()) + abs(off)))
            if abs(float(dot) - off) <= bound:
                return True
            cur = cur + 1 if float(dot) < off else int(forest.right[t, cur])
    return False


def one_case(rs: np.random.RandomState, it: int) -> str:
    rows = int(rs.randint(300, 20000))
    d = int(rs.choice([1, 2, 3, 5, 8, 13, 16, 31, 32, 47, 64, 100, 128,
                       200, 600]))
    n = int(rs.choice([2, 4, 16, 64, 128, 256, 512, 1024, 4096]))
    n = min(n, rows)
    k = int(rs.randint(1, d + 1))
    T = int(rs.choice([1, 2, 3, 7, 8, 16, 33]))
    seed = int(rs.randint(1, 2**30))
    extended = bool(rs.randint(0, 2))
    rowdt = ("f32", "bf16", "f16")[int(rs.randint(0, 3))]
    bf16 = rowdt == "bf16"
    half = rowdt != "f32"  # 2-byte rows: bf16 or fp16
    # drawn from a stream of its own (keyed by the case's seed), so the
    # configurations of every --seed are the ones they were before layouts
    layout = ("row", "pitched", "feature")[
        int(np.random.RandomState(seed).randint(0, 3))]
    bootstrap = bool(rs.randint(0, 2))
    patho = rs.choice(["normal", "const_col", "dups", "big", "tiny"])

    X = rs.normal(size=(rows, d)).astype(np.float32)
    if patho == "const_col":
        X[:, rs.randint(0, d)] = float(rs.normal())
    elif patho == "dups":
        X = X[rs.randint(0, max(rows // 7, 1), size=rows)]
    elif patho == "big":
        # fp16 tops out at 65504: stay in range (inf rows would make the
        # build's min/max scan degenerate, which is not what this draws for)
        X *= 1e4 if rowdt == "f16" else 1e20
    elif patho == "tiny":
        # fp16: mostly subnormals (|x| < 2^-14), multiples of 2^-24
        X *= 1e-5 if rowdt == "f16" else 1e-20
    desc = (f"it={it} rows={rows} d={d} n={n} k={k} T={T} seed={seed} "
            f"ext={extended} dtype={rowdt} layout={layout} boot={bootstrap} "
            f"patho={patho}")

    Xt = torch.from_numpy(X).to("cuda")
    if half:
        Xt = Xt.to(torch.bfloat16 if bf16 else torch.float16)
        X = Xt.float().cpu().numpy()  # exact upcast: what the kernels see
    # the same values behind other strides, over a NaN-filled buffer (a read
    # outside the view would change a walk); consumed in place
    if layout == "pitched":
        wide = torch.full((rows + 2, d + 7), float("nan"), dtype=Xt.dtype,
                          device="cuda")
        wide[1:rows + 1, 3:3 + d] = Xt
        Xt = wide[1:rows + 1, 3:3 + d]
    elif layout == "feature":
        tall = torch.full((d + 2, rows + 5), float("nan"), dtype=Xt.dtype,
                          device="cuda")
        tall[1:d + 1, 2:rows + 2] = Xt.T
        Xt = tall[1:d + 1, 2:rows + 2].T
    assert gpu_engine._row_layout(Xt) == (
        "feature" if layout == "feature" and d > 1 else "row")

    bag = cpu_engine.sample_bags(rows, T, n, seed=seed, bootstrap=bootstrap)
    fs = cpu_engine.feature_subsets(d, k, T, seed=seed)

    if not extended:
        cpu_f = cpu_engine.build_forest(X, bag, fs, seed, n, k, d)
        rp = ResolvedParams(num_samples=n, num_features=k, total_rows=rows,
                            total_features=d)
        gpu_f = gpu_engine.build_forest(Xt, bag, fs, seed, rp)
        for name in ["node_count", "feature", "right", "num_instances"]:
            if not np.array_equal(getattr(gpu_f, name), getattr(cpu_f, name)):
                return f"FOREST MISMATCH {name}: {desc}"
        if not np.array_equal(gpu_f.value.view(np.int32),
                              cpu_f.value.view(np.int32)):
            return f"FOREST MISMATCH value: {desc}"
        cpu_ps = cpu_engine.path_lengths(cpu_f, X)

        class Shell:
            forest = gpu_f
            _gpu_forest_cache = {}
        gpu_ps = gpu_engine.score_forest(Shell(), Xt, finalize=False)
        if not np.array_equal(gpu_ps.cpu().numpy().view(np.int32),
                              cpu_ps.view(np.int32)):
            return f"SCORE MISMATCH standard (bitwise): {desc}"
    else:
        ext_level = int(rs.randint(0, k))
        desc += f" ext_level={ext_level}"
        cpu_f = cpu_engine.build_extended_forest(X, bag, fs, seed, n, k, d,
                                                 ext_level)
        rp = ResolvedParams(num_samples=n, num_features=k, total_rows=rows,
                            total_features=d, extension_level=ext_level)
        gpu_f = gpu_engine.build_extended_forest(Xt, bag, fs, seed, rp)
        for name in ["node_count", "feature", "right", "num_instances",
                     "hyper_idx"]:
            if not np.array_equal(getattr(gpu_f, name), getattr(cpu_f, name)):
                return f"EIF FOREST MISMATCH {name}: {desc}"
        for name in ["value", "hyper_w"]:
            if not np.array_equal(getattr(gpu_f, name).view(np.int32),
                                  getattr(cpu_f, name).view(np.int32)):
                return f"EIF FOREST MISMATCH {name}: {desc}"
        if not np.array_equal(gpu_f.offset64, cpu_f.offset64):
            return f"EIF FOREST MISMATCH offset64: {desc}"
        cpu_ps = cpu_engine.path_lengths_extended(cpu_f, X)

        class Shell:
            forest = gpu_f
            _gpu_forest_cache = {}
        gpu_ps = gpu_engine.score_extended_forest(Shell(), Xt, finalize=False)
        diff = np.abs(gpu_ps.cpu().numpy() - cpu_ps)
        # mirror the routing to know the numeric contract: sparse v2 and the
        # general kernel keep strict j-order (bitwise); dense reassociates
        nnz = min(ext_level + 1, k)
        mn = gpu_f.feature.shape[1]
        elem = 2 if half else 4
        dpad_s = d
        while (dpad_s % 4 != 2) if half else (dpad_s % 2 != 1):
            dpad_s += 1
        sparse_route = (nnz <= 5
                        and mn * (12 + nnz * 8) + 2 * 256 * dpad_s * elem
                        <= 150 * 1024)
        if d <= 8:
            D = 8
        elif d <= 16:
            D = 16
        elif d <= 32:
            D = 32
        elif d <= 64:
            D = 64
        else:
            D = 128
        # v3 (bf16 rows only) packs bf16 weights; f32 and fp16 rows take v2
        d_cap = 128 if bf16 else 64
        wbytes = (D // 8 + 1) * 16 if bf16 else (D // 4 + 1) * 16
        dense_route = (not sparse_route and d <= d_cap
                       and (nnz == d or nnz >= 6)
                       and mn * 12 + 16 + mn * wbytes <= 160 * 1024)
        old_dense_route = (not sparse_route and not dense_route
                           and nnz == d and d % 4 == 0 and mn * 8 <= 120 * 1024)
        if dense_route or old_dense_route:
            if bf16 and dense_route:
                # v3 route: weights staged as bf16 (RNE) — oracle must use
                # the same rounded weights; remaining diffs are
                # reassociation-level only (PARITY.md EIF bf16 contract)
                from isolation_forest_amd.utils.det_math import bf16_round

                import copy as _copy
                f_b = _copy.copy(cpu_f)
                f_b.hyper_w = bf16_round(cpu_f.hyper_w)
                cpu_ps_b = cpu_engine.path_lengths_extended(f_b, X)
                diff = np.abs(gpu_ps.cpu().numpy() - cpu_ps_b)
                cpu_ps = cpu_ps_b
            scale = max(1.0, float(np.abs(cpu_ps).max()))
            bad = np.nonzero(diff > 1e-3 * scale)[0]
            frac = len(bad) / max(len(diff), 1)
            # every flip must be an EXPLAINED knife edge (reassociation
            # scale) on the oracle walk — duplicate-heavy data amplifies
            # the flip FRACTION arbitrarily (every copy of a knife-edge
            # row flips together) but never the margin; an indexing bug
            # flips rows at large margins and fails here
            # duplicate-heavy data can legitimately flip MOST rows: a
            # pure-duplicate segment's offset is EXACTLY the class's own
            # projection (every intercept has lo == hi), so the whole
            # class sits on an exact f64 tie that f32 rounding resolves
            # either way. No fraction ceiling therefore — instead a
            # STRIDED sample across all flipped rows must each be
            # individually margin-explained (a systematic inversion flips
            # rows at large margins and fails).
            oracle_f = f_b if (bf16 and dense_route) else cpu_f
            step_ = max(1, len(bad) // 80)
            for r in bad[::step_][:80]:
                if not _knife_edge_explained(oracle_f, X[r]):
                    return (f"UNEXPLAINED dense mismatch row {int(r)} "
                            f"(diff {float(diff[r]):.5f}, "
                            f"{frac:.4f} rows off): {desc}")
        else:  # sparse v2 or general strict-order kernel: bitwise
            if not np.array_equal(gpu_ps.cpu().numpy().view(np.int32),
                                  cpu_ps.view(np.int32)):
                return f"SCORE MISMATCH EIF strict-order (bitwise): {desc}"
    return ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from isolation_forest_amd.ops import load_extension

    load_extension()
    rs = np.random.RandomState(args.seed)
    for it in range(args.iters):
        msg = one_case(rs, it)
        if msg:
            print(msg)
            sys.exit(1)
    print(f"fuzz: {args.iters} random configurations, all parity checks "
          "passed")


if __name__ == "__main__":
    main()
