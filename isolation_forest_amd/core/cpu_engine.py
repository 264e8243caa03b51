"""CPU reference engine (numpy) — the correctness oracle for the HIP kernels.

Implements the exact algorithm semantics of the reference:

* iTree construction, Liu et al. Algorithm 2 — height limit ceil(log2(n)),
  constant-feature retry, uniform split in [min, max)
  (IsolationTree.scala:53-183),
* Extended iTree construction, Hariri et al. Alg. 2 — Gaussian hyperplane,
  L2-normalized, sparse over min(extensionLevel+1, dim) coordinates, no
  retry on degenerate splits (empty side => zero-instance leaf)
  (ExtendedIsolationTree.scala:112-270),
* path-length scoring with leaf adjustment c(numInstances)
  (IsolationTreeBase.scala:15, IsolationTree.scala:196-230),
* bagging semantics: uniform subsample without replacement (bootstrap=False,
  the composition of Binomial thinning + shuffle/slice in
  BaggedPoint.scala:114-178 + SharedTrainLogic.scala:287) or with
  replacement (bootstrap=True, Poisson bagging).

Randomness is the counter-based Philox scheme of utils/rng.py, NOT the
reference's java Random streams: we match *semantics* (the same
distributions at every decision point), not Scala RNG bit-streams — see
SURVEY.md §7 "Hard parts" #1. Self-determinism is bitwise: the same seed
yields the same forest on CPU and GPU, at any world size, because every
draw is keyed by (seed, purpose, treeId, nodeId/slot, attempt).

PRECISION CONTRACT (kept identical in ops/hip/forest_kernels.hip):
* features are float32 (core/Utils.scala:11),
* node min/max scans are float32,
* the split point / hyperplane offset is computed in float64 and then
  ROUNDED TO FLOAT32; the float32 value is what both construction-time
  partitioning and scoring compare against (the reference keeps float64 —
  we round so CPU/GPU/ONNX all agree bitwise; Avro persists the exact
  float32 value widened to double),
* EIF hyperplane dots accumulate in float32 in ascending-index order with
  un-fused multiply-add (matches the HIP kernel's __fmul_rn/__fadd_rn),
* per-row path length = int depth + float32 c(leaf count); the sum over
  trees accumulates float32 in tree order; the final score is
  2^(-mean/c(n)) in float64, cast to float32.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

from ..utils import det_math, rng
from ..utils.math import avg_path_length
from .forest import (
    ExtendedForest,
    Forest,
    empty_extended_forest,
    empty_forest,
)

# ---------------------------------------------------------------------------
# Bagging (reference: BaggedPoint.scala + SharedTrainLogic.scala:287)
# ---------------------------------------------------------------------------


def sample_bags(
    total_rows: int,
    num_trees: int,
    num_samples: int,
    seed: int,
    bootstrap: bool,
    tree_id_offset: int = 0,
    row_offset: int = 0,
) -> np.ndarray:
    """Sample per-tree bags of row indices, shape [num_trees, num_samples].

    ``tree_id_offset`` keys the draws by GLOBAL tree id so a tree-sharded
    multi-GPU run draws the identical forest as a single-GPU run.
    ``row_offset`` maps local row indices to global ones under row sharding
    (draws are over the local shard only; bags are iid samples of the local
    rows, statistically equivalent to the reference's partition-local
    bagging, BaggedPoint.scala:161-178).
    """
    T, n = num_trees, num_samples
    tree_ids = (np.arange(T, dtype=np.uint32) + np.uint32(tree_id_offset))[:, None]
    slots = np.arange(n, dtype=np.uint32)[None, :]
    if bootstrap:
        idx = rng.randint_below(seed, rng.P_BAG, tree_ids, slots, total_rows)
        return idx + row_offset

    if num_samples > total_rows:
        raise ValueError("cannot sample more rows than the dataset holds")

    if num_samples * 2 > total_rows:
        # dense regime: a full random permutation per tree (argsort of
        # per-(tree,row) Philox keys; ties broken stably by row id), take the
        # first n. O(T*N log N), only used when N < 2n.
        row_ids = np.arange(total_rows, dtype=np.uint32)[None, :]
        keys = rng.u32(
            seed, rng.P_BAG, tree_ids, row_ids, attempt=np.uint32(0xFFFF)
        )
        perm = np.argsort(keys, axis=1, kind="stable")
        return perm[:, :n].astype(np.int64) + row_offset

    # Sparse regime (n <= N/2): iterative collision-resolution with
    # deterministic "smallest slot wins" arbitration; expected O(1) rounds.
    idx = rng.randint_below(seed, rng.P_BAG, tree_ids, slots, total_rows)
    slot_mat = np.broadcast_to(np.arange(n, dtype=np.int64)[None, :], (T, n))
    attempt = 0
    while True:
        # per tree: among slots sharing a value, the smallest slot id wins;
        # the rest redraw with attempt+1 (deterministic, order-independent).
        order = np.lexsort((slot_mat, idx), axis=-1)  # by value, then slot
        sorted_vals = np.take_along_axis(idx, order, axis=1)
        dup = np.zeros((T, n), dtype=bool)
        dup[:, 1:] = sorted_vals[:, 1:] == sorted_vals[:, :-1]
        loser = np.zeros((T, n), dtype=bool)
        np.put_along_axis(loser, order, dup, axis=1)
        if not loser.any():
            return idx + row_offset
        attempt += 1
        if attempt > 256:
            raise RuntimeError("bag sampling failed to converge (internal bug)")
        fresh = rng.randint_below(
            seed, rng.P_BAG, tree_ids, slots, total_rows, attempt=np.uint32(attempt)
        )
        idx = np.where(loser, fresh, idx)


def feature_subsets(
    total_features: int, num_features: int, num_trees: int, seed: int,
    tree_id_offset: int = 0,
) -> np.ndarray:
    """Per-tree sorted feature subsets [num_trees, num_features] (global ids).

    Reference: shuffle(0..d-1).take(numFeatures).sorted
    (SharedTrainLogic.scala:300-304). A uniform random permutation is drawn
    as the argsort of per-(tree, feature) Philox keys.
    """
    T, d, k = num_trees, total_features, num_features
    tree_ids = (np.arange(T, dtype=np.uint32) + np.uint32(tree_id_offset))[:, None]
    feats = np.arange(d, dtype=np.uint32)[None, :]
    keys = rng.u32(seed, rng.P_FEATSUB, tree_ids, feats)
    perm = np.argsort(keys, axis=1, kind="stable")
    subset = np.sort(perm[:, :k], axis=1)
    return subset.astype(np.int32)


# ---------------------------------------------------------------------------
# Standard iTree construction (reference: IsolationTree.scala:83-183)
# ---------------------------------------------------------------------------


def _split_feature(
    bag: np.ndarray, seg: np.ndarray, features: np.ndarray, seed: int,
    tree_id: int, node_id: int, featsel_row: np.ndarray = None,
) -> Tuple[int, float, float]:
    """Draw a split feature with constant-feature retry.

    Fisher-Yates over the tree's feature subset; first feature whose values
    in this node are non-constant wins (IsolationTree.scala:124-150).
    Returns (feature, min, max) or (-1, 0, 0) when every feature is constant.
    ``featsel_row`` optionally supplies the node's precomputed Fisher-Yates
    offsets (featsel_table; bitwise-identical draws, vectorized Philox).
    """
    avail = features.copy()
    k = len(avail)
    for j in range(k):
        if featsel_row is not None:
            t = j + int(featsel_row[j])
        else:
            t = j + int(
                rng.randint_below(
                    seed, rng.P_FEATSEL, np.uint32(tree_id),
                    np.uint32(node_id), k - j, attempt=np.uint32(j),
                )
            )
        avail[j], avail[t] = avail[t], avail[j]
        f = int(avail[j])
        col = bag[seg, f]
        fmin = np.float32(col.min())
        fmax = np.float32(col.max())
        if fmin < fmax:
            return f, float(fmin), float(fmax)
    return -1, 0.0, 0.0


def draw_tables(seed: int, tree_ids: np.ndarray, max_nodes: int, k: int):
    """Vectorized per-(tree, node) Philox draws for the standard build.

    Bitwise-identical to the per-node scalar calls build_tree would
    otherwise make (same keys/purposes; rng.py is broadcast-capable) —
    one batched Philox evaluation replaces ~2*nodes scalar ones, the
    dominant cost of the CPU oracle build (profiled 80%).
    Returns (usplit [T, mn] float64, featsel [T, mn, k] int64)."""
    T = len(tree_ids)
    tg = tree_ids.astype(np.uint32)[:, None]
    ng = np.arange(max_nodes, dtype=np.uint32)[None, :]
    usplit = rng.uniform(seed, rng.P_SPLIT, tg, ng)
    featsel = np.empty((T, max_nodes, k), dtype=np.int64)
    for j in range(k):
        featsel[:, :, j] = rng.randint_below(
            seed, rng.P_FEATSEL, tg, ng, k - j, attempt=np.uint32(j))
    return usplit, featsel


def _split_value32(fmin: float, fmax: float, u: float) -> np.float32:
    """float64 split draw rounded to float32, bumped off the left edge."""
    s64 = fmin + u * (fmax - fmin)
    s32 = np.float32(s64)
    if not (np.float32(fmin) < s32):
        s32 = np.nextafter(np.float32(fmin), np.float32(np.inf), dtype=np.float32)
    return s32


def build_tree(
    bag: np.ndarray,  # [n, d_total] float32 (full-width rows; subset via indices)
    features: np.ndarray,  # sorted int32 global feature ids for this tree
    seed: int,
    tree_id: int,
    out_feature: np.ndarray,
    out_value: np.ndarray,
    out_right: np.ndarray,
    out_count: np.ndarray,
    out_value64: np.ndarray = None,
    usplit_row: np.ndarray = None,   # [max_nodes] precomputed split uniforms
    featsel_tab: np.ndarray = None,  # [max_nodes, k] precomputed FY offsets
    leaf_lut: np.ndarray = None,     # [n+1] precomputed c(m) float32
) -> int:
    """Build one iTree into pre-order SoA rows; returns node count."""
    n = bag.shape[0]
    height_limit = int(math.ceil(math.log2(max(n, 2))))
    rows = np.arange(n, dtype=np.int64)

    next_id = 0
    # stack entries: (segment_rows, height, patch_parent) — patch_parent is the
    # node whose `right` field points to the node this entry will emit (-1 root/left)
    stack = [(rows, 0, -1)]
    while stack:
        seg, height, patch = stack.pop()
        node = next_id
        next_id += 1
        if patch >= 0:
            out_right[patch] = node
        m = len(seg)
        if m <= 1 or height >= height_limit:
            out_feature[node] = Forest.LEAF
            out_value[node] = (leaf_lut[m] if leaf_lut is not None
                               else avg_path_length(m))
            out_count[node] = m
            continue
        f, fmin, fmax = _split_feature(
            bag, seg, features, seed, tree_id, node,
            featsel_tab[node] if featsel_tab is not None else None)
        if f < 0:
            out_feature[node] = Forest.LEAF
            out_value[node] = (leaf_lut[m] if leaf_lut is not None
                               else avg_path_length(m))
            out_count[node] = m
            continue
        u = (float(usplit_row[node]) if usplit_row is not None
             else float(rng.uniform(seed, rng.P_SPLIT, np.uint32(tree_id),
                                    np.uint32(node))))
        s32 = _split_value32(fmin, fmax, u)
        mask = bag[seg, f] < s32
        left = seg[mask]
        right = seg[~mask]
        out_feature[node] = f
        out_value[node] = s32
        if out_value64 is not None:
            out_value64[node] = float(s32)
        out_count[node] = -1
        # pre-order: left child = node+1 (immediately next); push right first
        stack.append((right, height + 1, node))
        stack.append((left, height + 1, -1))
    return next_id


def build_forest(
    X: np.ndarray,  # [N, d] float32
    bag_idx: np.ndarray,  # [T, n] int64
    feat_sub: np.ndarray,  # [T, k] int32
    seed: int,
    num_samples: int,
    num_features: int,
    total_num_features: int,
    tree_id_offset: int = 0,
) -> Forest:
    T, n = bag_idx.shape
    max_nodes = 2 * n - 1 if n >= 1 else 1
    forest = empty_forest(T, max_nodes, num_samples, num_features, total_num_features)
    k = feat_sub.shape[1]
    leaf_lut = avg_path_length(np.arange(n + 1)).astype(np.float32)
    # chunk the draw tables so memory stays bounded at large tree counts
    # (featsel is [chunk, max_nodes, k] int64)
    chunk = max(1, min(T, int(64e6 // max(max_nodes * k, 1)) or 1))
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        tree_ids = np.arange(t0, t1, dtype=np.int64) + tree_id_offset
        usplit, featsel = draw_tables(seed, tree_ids, max_nodes, k)
        for t in range(t0, t1):
            bag = X[bag_idx[t]]
            nc = build_tree(
                bag,
                feat_sub[t],
                seed,
                t + tree_id_offset,
                forest.feature[t],
                forest.value[t],
                forest.right[t],
                forest.num_instances[t],
                forest.value64[t],
                usplit_row=usplit[t - t0],
                featsel_tab=featsel[t - t0],
                leaf_lut=leaf_lut,
            )
            forest.node_count[t] = nc
    return forest


# ---------------------------------------------------------------------------
# Extended iTree construction (reference: ExtendedIsolationTree.scala:112-270)
# ---------------------------------------------------------------------------


def _gaussian(seed: int, tree_id: int, counter: int) -> float:
    u1, u2 = rng.uniform2(seed, rng.P_EIF_NORMAL, np.uint32(tree_id), np.uint32(counter))
    # Box-Muller with bitwise-deterministic log/cos (utils/det_math.py):
    # the HIP device implementation produces identical doubles.
    return float(det_math.det_gaussian(u1, u2))


def draw_tables_extended(seed: int, tree_ids: np.ndarray, max_nodes: int,
                         k: int, nnz: int):
    """Vectorized per-(tree, node, slot) Philox draws for the EIF build —
    bitwise-identical counters to the per-node calls in _draw_hyperplane
    (same purposes/keys, rng.py broadcasts). Returns
    (fy [T,mn,nnz] int64, w32 [T,mn,nnz] float32 unnormalized gaussians,
    uint [T,mn,nnz] float64 intercept uniforms)."""
    tg = tree_ids.astype(np.uint32)[:, None, None]
    ng = np.arange(max_nodes, dtype=np.int64)[None, :, None]
    jarr = np.arange(nnz, dtype=np.int64)[None, None, :]
    fy = rng.randint_below(
        seed, rng.P_EIF_COORD, tg, ng.astype(np.uint32),
        (k - jarr), attempt=jarr.astype(np.uint32),
    )
    slot = (ng * 4096 + jarr).astype(np.uint32)
    u1, u2 = rng.uniform2(seed, rng.P_EIF_NORMAL, tg, slot)
    w32 = det_math.det_gaussian(u1, u2).astype(np.float32)
    uint = rng.uniform(seed, rng.P_EIF_INTERCEPT, tg, slot).astype(np.float64)
    return fy, w32, uint


def _draw_hyperplane(
    bag: np.ndarray, seg: np.ndarray, features: np.ndarray, nnz: int,
    seed: int, tree_id: int, node_id: int, tabs=None,
):
    """Returns (idx[nnz] int32 ascending, w[nnz] float32, offset64, offset32)
    or None when the weight vector has zero norm (theoretical leaf case,
    ExtendedIsolationTree.scala:183-184)."""
    k = len(features)
    avail = features.copy()
    if tabs is not None:
        fy = tabs[0][node_id]
        w = tabs[1][node_id].copy()
    else:
        jarr = np.arange(nnz, dtype=np.uint32)
        # batched Philox draws — identical counters (and therefore bitwise-
        # identical values) to per-j scalar calls, ~5x faster per node
        fy = rng.randint_below(
            seed, rng.P_EIF_COORD, np.uint32(tree_id), np.uint32(node_id),
            (k - jarr.astype(np.int64)), attempt=jarr,
        )
    for j in range(nnz):
        t = j + int(fy[j])
        avail[j], avail[t] = avail[t], avail[j]
    coords = np.array(sorted(int(c) for c in avail[:nnz]), dtype=np.int32)

    if tabs is None:
        # weights drawn AFTER sorting, keyed by slot j over sorted coords
        base = node_id * 4096  # nnz-slot stride; nnz <= 4096 by construction
        u1, u2 = rng.uniform2(
            seed, rng.P_EIF_NORMAL, np.uint32(tree_id),
            np.uint32(base) + jarr,
        )
        w = det_math.det_gaussian(u1, u2).astype(np.float32)
    # L2 normalize in float32, sequential accumulation
    acc = np.float32(0.0)
    for j in range(nnz):
        acc = np.float32(acc + np.float32(w[j] * w[j]))
    if acc <= np.float32(0.0):
        return None
    norm = np.float32(np.sqrt(acc))
    w = (w / norm).astype(np.float32)

    # intercepts per sorted coordinate; offset in float64
    sub = bag[np.ix_(seg, coords)]
    mn = sub.min(axis=0).astype(np.float32).astype(np.float64)
    mx = sub.max(axis=0).astype(np.float32).astype(np.float64)
    if tabs is not None:
        u = tabs[2][node_id]
    else:
        u = rng.uniform(
            seed, rng.P_EIF_INTERCEPT, np.uint32(tree_id),
            np.uint32(base) + jarr,
        ).astype(np.float64)
    intercepts = mn + u * (mx - mn)
    off64 = 0.0
    for j in range(nnz):
        off64 += float(w[j]) * float(intercepts[j])
    return coords, w, off64, np.float32(off64)


def _dot32(bag: np.ndarray, seg: np.ndarray, coords: np.ndarray, w: np.ndarray):
    """Sequential float32 dot in ascending-index order (no FMA)."""
    acc = np.zeros(len(seg), dtype=np.float32)
    for j in range(len(coords)):
        prod = (w[j] * bag[seg, coords[j]]).astype(np.float32)
        acc = (acc + prod).astype(np.float32)
    return acc


def build_extended_tree(
    bag: np.ndarray,
    features: np.ndarray,
    nnz: int,
    seed: int,
    tree_id: int,
    fr: ExtendedForest,
    t: int,
    tabs=None,
    leaf_lut: np.ndarray = None,
) -> int:
    n = bag.shape[0]
    height_limit = int(math.ceil(math.log2(max(n, 2))))
    rows = np.arange(n, dtype=np.int64)
    next_id = 0
    stack = [(rows, 0, -1)]
    while stack:
        seg, height, patch = stack.pop()
        node = next_id
        next_id += 1
        if patch >= 0:
            fr.right[t, patch] = node
        m = len(seg)
        if m <= 1 or height >= height_limit:
            fr.feature[t, node] = ExtendedForest.LEAF
            fr.value[t, node] = (leaf_lut[m] if leaf_lut is not None
                                 else avg_path_length(m))
            fr.num_instances[t, node] = m
            continue
        hp = _draw_hyperplane(bag, seg, features, nnz, seed, tree_id, node,
                              tabs=tabs)
        if hp is None:
            fr.feature[t, node] = ExtendedForest.LEAF
            fr.value[t, node] = (leaf_lut[m] if leaf_lut is not None
                                 else avg_path_length(m))
            fr.num_instances[t, node] = m
            continue
        coords, w, off64, off32 = hp
        dots = _dot32(bag, seg, coords, w)
        mask = dots < off32
        left = seg[mask]
        right = seg[~mask]
        # NO retry on degenerate splits: empty side becomes a 0-instance leaf
        fr.feature[t, node] = nnz
        fr.value[t, node] = off32
        fr.offset64[t, node] = off64
        fr.hyper_idx[t, node, :nnz] = coords
        fr.hyper_w[t, node, :nnz] = w
        fr.num_instances[t, node] = -1
        stack.append((right, height + 1, node))
        stack.append((left, height + 1, -1))
    return next_id


def build_extended_forest(
    X: np.ndarray,
    bag_idx: np.ndarray,
    feat_sub: np.ndarray,
    seed: int,
    num_samples: int,
    num_features: int,
    total_num_features: int,
    extension_level: int,
    tree_id_offset: int = 0,
) -> ExtendedForest:
    T, n = bag_idx.shape
    height_limit = int(math.ceil(math.log2(max(n, 2))))
    max_nodes = 2 ** (height_limit + 1) - 1
    nnz = min(extension_level + 1, num_features)
    fr = empty_extended_forest(
        T, max_nodes, nnz, num_samples, num_features, total_num_features,
        extension_level,
    )
    k = feat_sub.shape[1]
    leaf_lut = avg_path_length(np.arange(n + 1)).astype(np.float32)
    chunk = max(1, min(T, int(32e6 // max(max_nodes * max(nnz, 1), 1)) or 1))
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        tree_ids = np.arange(t0, t1, dtype=np.int64) + tree_id_offset
        fy_t, w_t, u_t = draw_tables_extended(seed, tree_ids, max_nodes, k,
                                              nnz)
        for t in range(t0, t1):
            bag = X[bag_idx[t]]
            fr.node_count[t] = build_extended_tree(
                bag, feat_sub[t], nnz, seed, t + tree_id_offset, fr, t,
                tabs=(fy_t[t - t0], w_t[t - t0], u_t[t - t0]),
                leaf_lut=leaf_lut,
            )
    return fr


# ---------------------------------------------------------------------------
# Scoring (reference: IsolationTree.scala:196-230, IsolationForestModel.scala:116-151)
# ---------------------------------------------------------------------------


def path_lengths(forest: Forest, X: np.ndarray) -> np.ndarray:
    """Sum of per-tree path lengths for each row, float32 [N].

    Accumulates over trees in tree order with float32 adds, matching the
    HIP traversal kernel bit-for-bit. Dispatches to a vectorized
    fixed-trip walk (mask-free; ~6x) that is bitwise-identical to the
    masked reference walk below (tests/test_cpu_engine.py pins both
    against each other); set IFA_CPU_WALK_REF=1 to force the reference.
    """
    import os as _os

    if _os.environ.get("IFA_CPU_WALK_REF") != "1":
        return _path_lengths_fast(forest, X)
    return _path_lengths_ref(forest, X)


def _path_lengths_fast(forest: Forest, X: np.ndarray) -> np.ndarray:
    """Vectorized fixed-trip walk (the v4 kernel's structure in numpy):
    leaves self-loop, depth is folded into f32 leaf values at pack time,
    splits compare x(f32, promoted) < value64 — identical semantics and
    f32 accumulation order to _path_lengths_ref, with no per-iteration
    masking or nonzero() calls."""
    N = X.shape[0]
    T, mn = forest.feature.shape
    feat = forest.feature
    internal = feat >= 0
    leaf = feat == Forest.LEAF
    right = forest.right.astype(np.int64)
    v64_all = (forest.value64 if getattr(forest, "value64", None) is not None
               else forest.value.astype(np.float64))
    # pack: feature (sentinel column d at leaves/pads), self-loop rights,
    # -inf thresholds at leaves (the +inf sentinel column compares false),
    # depth-folded f32 leaf values
    from ..ops.gpu_engine import _node_depths

    depth = _node_depths(feat, forest.right)
    d = X.shape[1]
    ids = np.broadcast_to(np.arange(mn, dtype=np.int64)[None, :], (T, mn))
    fcol = np.where(internal, feat.astype(np.int64), d)
    nxt_r = np.where(internal, right, ids)
    thr = np.where(internal, v64_all, -np.inf)
    leafval = np.where(
        leaf, depth.astype(np.float32) + forest.value.astype(np.float32),
        np.float32(0.0)).astype(np.float32)
    max_depth = int(depth[internal | leaf].max()) if (internal | leaf).any() else 0

    Xa = np.concatenate(
        [X, np.full((N, 1), np.inf, dtype=X.dtype)], axis=1)
    rows = np.arange(N)
    total = np.zeros(N, dtype=np.float32)
    for t in range(T):
        cur = np.zeros(N, dtype=np.int64)
        f_t, r_t, thr_t = fcol[t], nxt_r[t], thr[t]
        for _ in range(max_depth):
            f = f_t[cur]
            go_left = Xa[rows, f] < thr_t[cur]
            cur = np.where(go_left, cur + 1, r_t[cur])
        total = (total + leafval[t][cur]).astype(np.float32)
    return total


def _path_lengths_ref(forest: Forest, X: np.ndarray) -> np.ndarray:
    """Masked reference walk (kept verbatim as the differential anchor)."""
    N = X.shape[0]
    total = np.zeros(N, dtype=np.float32)
    # splits compare in FLOAT64 against the exact persisted values, matching
    # the reference's Float-promoted-to-Double compare
    # (IsolationTree.scala:213-229): x < splitValue with splitValue a Double.
    # For our own forests value64 is exactly the f32 split, so this is
    # bitwise-identical to an f32 compare; for loaded foreign models it
    # removes the knife-edge flips f32 rounding produced.
    v64_all = (forest.value64 if getattr(forest, "value64", None) is not None
               else forest.value.astype(np.float64))
    for t in range(forest.num_trees):
        feat = forest.feature[t]
        val = forest.value[t]
        v64 = v64_all[t]
        right = forest.right[t]
        cur = np.zeros(N, dtype=np.int64)
        depth = np.zeros(N, dtype=np.int32)
        active = feat[cur] >= 0
        while active.any():
            f = feat[cur[active]]
            x = X[np.nonzero(active)[0], f]
            go_left = x < v64[cur[active]]
            nxt = np.where(go_left, cur[active] + 1, right[cur[active]])
            cur[active] = nxt
            depth[active] += 1
            active2 = np.zeros(N, dtype=bool)
            active2[np.nonzero(active)[0]] = feat[nxt] >= 0
            active = active2
        leaf_term = val[cur]  # precomputed c(numInstances)
        total = (total + (depth.astype(np.float32) + leaf_term)).astype(np.float32)
    return total


def path_lengths_extended(fr: ExtendedForest, X: np.ndarray) -> np.ndarray:
    N = X.shape[0]
    total = np.zeros(N, dtype=np.float32)
    nnz = fr.nnz
    for t in range(fr.num_trees):
        feat = fr.feature[t]
        val = fr.value[t]
        right = fr.right[t]
        hidx = fr.hyper_idx[t]
        hw = fr.hyper_w[t]
        cur = np.zeros(N, dtype=np.int64)
        depth = np.zeros(N, dtype=np.int32)
        active = feat[cur] >= 0
        while active.any():
            rows = np.nonzero(active)[0]
            nodes = cur[rows]
            acc = np.zeros(len(rows), dtype=np.float32)
            for j in range(nnz):
                c = hidx[nodes, j]
                wj = hw[nodes, j]
                prod = (wj * X[rows, c]).astype(np.float32)
                acc = (acc + prod).astype(np.float32)
            go_left = acc < val[nodes]
            nxt = np.where(go_left, nodes + 1, right[nodes])
            cur[rows] = nxt
            depth[rows] += 1
            active2 = np.zeros(N, dtype=bool)
            active2[rows] = feat[nxt] >= 0
            active = active2
        leaf_term = val[cur]
        total = (total + (depth.astype(np.float32) + leaf_term)).astype(np.float32)
    return total


def scores_from_path_sums(path_sum: np.ndarray, num_trees: int, num_samples: int):
    """score = 2^(-(mean path length)/c(n)), float32.

    Reference formula: IsolationForestModel.scala:135-138."""
    mean32 = (path_sum / np.float32(num_trees)).astype(np.float32)
    c = np.float32(avg_path_length(num_samples))
    return np.exp2(-(mean32.astype(np.float64) / float(c))).astype(np.float32)


def score_forest(forest: Forest, X: np.ndarray) -> np.ndarray:
    ps = path_lengths(forest, X)
    return scores_from_path_sums(ps, forest.num_trees, forest.num_samples)


def score_extended_forest(fr: ExtendedForest, X: np.ndarray) -> np.ndarray:
    ps = path_lengths_extended(fr, X)
    return scores_from_path_sums(ps, fr.num_trees, fr.num_samples)


# ---------------------------------------------------------------------------
# Per-feature score attribution (path-length decomposition, Saabas style).
# No analogue in the reference; the contract is docs/DESIGN.md §8. These
# functions are the oracle for the explain_* HIP kernels (bitwise).
# ---------------------------------------------------------------------------


def _leaf_path_values(forest) -> np.ndarray:
    """f32(depth) + f32(value) per node — the leaf term of the v4 pack and
    _path_lengths_fast (only meaningful at leaves)."""
    from ..ops.gpu_engine import _node_depths

    depth = _node_depths(forest.feature, forest.right)
    return (depth.astype(np.float32)
            + forest.value.astype(np.float32)).astype(np.float32)


def node_expectations(forest) -> Tuple[np.ndarray, np.ndarray]:
    """Expected path length E[v] (float64) of a training row below every
    node, and the instance count n[v] (int64) it is weighted by.

    Leaf: E = f64(f32(depth) + f32(value)), n = num_instances. Internal:
    n = n_l + n_r, E = (n_l*E_l + n_r*E_r)/n, or the plain mean of the two
    children when n == 0 (EIF zero-instance leaves). Internal nodes carry
    num_instances = -1, so counts always come from the leaves. One reverse
    pre-order sweep suffices because left = id+1 and right > id. Works on
    Forest and ExtendedForest; pad nodes stay 0."""
    feat = forest.feature
    T, mn = feat.shape
    leaf = feat == Forest.LEAF
    E = np.where(leaf, _leaf_path_values(forest).astype(np.float64), 0.0)
    n = np.where(leaf, forest.num_instances.astype(np.int64), 0)
    right = forest.right.astype(np.int64)
    for v in range(mn - 2, -1, -1):
        ts = np.nonzero(feat[:, v] >= 0)[0]
        if not len(ts):
            continue
        r = right[ts, v]
        nl, nr = n[ts, v + 1], n[ts, r]
        el, er = E[ts, v + 1], E[ts, r]
        nv = nl + nr
        safe = np.where(nv > 0, nv, 1).astype(np.float64)
        E[ts, v] = np.where(nv > 0, (nl * el + nr * er) / safe,
                            (el + er) / 2.0)
        n[ts, v] = nv
    return E, n


def edge_deltas(forest, E: np.ndarray = None):
    """(delta_left, delta_right) float64 [T, mn]: E[child] - E[v] for the
    two edges leaving every internal node, 0 at leaves and pads. Callers
    round ONCE to float32 (after the EIF share multiply, if any)."""
    if E is None:
        E, _ = node_expectations(forest)
    T, mn = forest.feature.shape
    internal = forest.feature >= 0
    ti = np.broadcast_to(np.arange(T, dtype=np.int64)[:, None], (T, mn))
    ids = np.broadcast_to(np.arange(mn, dtype=np.int64)[None, :], (T, mn))
    lid = np.where(internal, ids + 1, ids)
    rid = np.where(internal, forest.right.astype(np.int64), ids)
    dl = np.where(internal, E[ti, lid] - E, 0.0)
    dr = np.where(internal, E[ti, rid] - E, 0.0)
    return dl, dr


def explain_tables(forest):
    """Cached per-forest attribution tables (forests are immutable):
    ``bias`` = f32(mean_t E[root_t]) and float32 edge deltas. Standard:
    ``dl``/``dr`` [T, mn]. Extended: [T, mn, nnz] — the node's delta shared
    over its k = feature[t, v] hyperplane coordinates in proportion to
    w_j^2 (float64 from the f32 weights; equal shares when the sum is 0 or
    non-finite), each share rounded once; slots j >= k hold +0.0.

    The cache lives on the forest object and assumes what the models'
    device pack caches assume too: a forest's arrays are not edited once it
    has been scored or explained (core/forest.py). leaf_values_from_counts()
    drops it; any other in-place edit must call
    forest.invalidate_derived()."""
    tabs = getattr(forest, "_explain_tables", None)
    if tabs is not None:
        return tabs
    E, _ = node_expectations(forest)
    dl64, dr64 = edge_deltas(forest, E)
    bias = (np.float32(E[:, 0].mean()) if forest.num_trees
            else np.float32(0.0))
    if isinstance(forest, ExtendedForest):
        nnz = forest.nnz
        k = np.where(forest.feature >= 0, forest.feature, 0).astype(np.int64)
        used = np.arange(nnz, dtype=np.int64)[None, None, :] < k[:, :, None]
        w = forest.hyper_w.astype(np.float64)
        sq = np.where(used, w * w, 0.0)
        tot = np.zeros(k.shape, dtype=np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            for j in range(nnz):  # ascending j, like every other EIF sum
                tot = tot + sq[:, :, j]
        ok = np.isfinite(tot) & (tot > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(
                ok[:, :, None], sq / np.where(ok, tot, 1.0)[:, :, None],
                1.0 / np.maximum(k, 1)[:, :, None].astype(np.float64))
        share = np.where(used, share, 0.0)
        dl = (dl64[:, :, None] * share).astype(np.float32)
        dr = (dr64[:, :, None] * share).astype(np.float32)
        dl[~used] = 0.0
        dr[~used] = 0.0
    else:
        dl = dl64.astype(np.float32)
        dr = dr64.astype(np.float32)
    tabs = {"bias": bias, "dl": np.ascontiguousarray(dl),
            "dr": np.ascontiguousarray(dr)}
    forest._explain_tables = tabs
    return tabs


def expected_path_length(forest) -> np.float32:
    """The attribution bias: f32(mean over trees of E[root])."""
    return explain_tables(forest)["bias"]


def _finalize_contributions(acc: np.ndarray, num_trees: int, finalize: bool):
    if not finalize:
        return acc
    return (acc / np.float32(num_trees)).astype(np.float32)


def feature_contributions(forest: Forest, X: np.ndarray,
                          finalize: bool = True) -> np.ndarray:
    """Per-feature path-length contributions, float32 [N, d].

    The fixed-trip walk of _path_lengths_fast with one more thing carried
    along: a row visiting internal node v (split feature f) adds the taken
    edge's f32 delta to acc[row, f]. acc is float32, added in tree order
    and root-to-leaf within a tree (the explain_forest kernel's order).
    finalize=True returns f32(acc / f32(T)); with expected_path_length the
    row sums reproduce the mean path length. Negative = the feature
    shortened the path (more anomalous)."""
    X = np.asarray(X)
    N, d = X.shape
    T, mn = forest.feature.shape
    feat = forest.feature
    internal = feat >= 0
    live = internal | (feat == Forest.LEAF)
    right = forest.right.astype(np.int64)
    v64_all = (forest.value64 if getattr(forest, "value64", None) is not None
               else forest.value.astype(np.float64))
    tabs = explain_tables(forest)
    from ..ops.gpu_engine import _node_depths

    depth = _node_depths(feat, forest.right)
    max_depth = int(depth[live].max()) if live.any() else 0
    ids = np.broadcast_to(np.arange(mn, dtype=np.int64)[None, :], (T, mn))
    fcol = np.where(internal, feat.astype(np.int64), d)
    nxt_r = np.where(internal, right, ids)
    thr = np.where(internal, v64_all, -np.inf)

    Xa = np.concatenate([X, np.full((N, 1), np.inf, dtype=X.dtype)], axis=1)
    rows = np.arange(N)
    acc = np.zeros((N, d + 1), dtype=np.float32)  # column d: leaf self-loops
    for t in range(T):
        cur = np.zeros(N, dtype=np.int64)
        f_t, r_t, thr_t = fcol[t], nxt_r[t], thr[t]
        dl_t, dr_t = tabs["dl"][t], tabs["dr"][t]
        for _ in range(max_depth):
            f = f_t[cur]
            go_left = Xa[rows, f] < thr_t[cur]
            delta = np.where(go_left, dl_t[cur], dr_t[cur])
            acc[rows, f] = acc[rows, f] + delta  # one f32 add per row
            cur = np.where(go_left, cur + 1, r_t[cur])
    return _finalize_contributions(
        np.ascontiguousarray(acc[:, :d]), T, finalize)


def feature_contributions_extended(fr: ExtendedForest, X: np.ndarray,
                                   finalize: bool = True) -> np.ndarray:
    """EIF contributions, float32 [N, d]: the path_lengths_extended walk
    (strict j-order f32 dot < value) adding, per visited node, the taken
    edge's per-coordinate shares to acc[row, hyper_idx[j]] in ascending j
    over the node's k coordinates."""
    X = np.asarray(X)
    N, d = X.shape
    nnz = fr.nnz
    tabs = explain_tables(fr)
    acc = np.zeros((N, d), dtype=np.float32)
    for t in range(fr.num_trees):
        feat = fr.feature[t]
        val = fr.value[t]
        right = fr.right[t]
        hidx = fr.hyper_idx[t]
        hw = fr.hyper_w[t]
        dl_t, dr_t = tabs["dl"][t], tabs["dr"][t]
        cur = np.zeros(N, dtype=np.int64)
        active = feat[cur] >= 0
        while active.any():
            rows = np.nonzero(active)[0]
            nodes = cur[rows]
            dot = np.zeros(len(rows), dtype=np.float32)
            with np.errstate(over="ignore", invalid="ignore"):
                for j in range(nnz):  # inf/NaN cells: NaN compares false
                    c = hidx[nodes, j]
                    prod = (hw[nodes, j] * X[rows, c]).astype(np.float32)
                    dot = (dot + prod).astype(np.float32)
            go_left = dot < val[nodes]
            k = feat[nodes]
            for j in range(nnz):
                m = j < k
                rj, nj = rows[m], nodes[m]
                c = hidx[nj, j]
                delta = np.where(go_left[m], dl_t[nj, j], dr_t[nj, j])
                acc[rj, c] = acc[rj, c] + delta
            nxt = np.where(go_left, nodes + 1, right[nodes])
            cur[rows] = nxt
            active2 = np.zeros(N, dtype=bool)
            active2[rows] = feat[nxt] >= 0
            active = active2
    return _finalize_contributions(acc, fr.num_trees, finalize)


# ---------------------------------------------------------------------------
# Exact TreeSHAP for standard forests (path-dependent, leaf-path form). No
# analogue in the reference; the contract is docs/DESIGN.md §9. These
# functions are the oracle for shap_forest_kernel (bitwise).
# ---------------------------------------------------------------------------

SHAP_MAX_PATH_FEATURES = 16  # the kernel's c[] holds 17 doubles


def shap_weights(max_m: int = SHAP_MAX_PATH_FEATURES) -> np.ndarray:
    """w[m][k] = k! (m-1-k)! / m!, float64 [max_m + 1, max_m] (row 0 and
    the cells k >= m are 0): the Shapley weight of a coalition of k of the
    other m - 1 path features. The kernel's table is the default [17, 16];
    each cell is the correctly rounded quotient of two exact integers."""
    w = np.zeros((max_m + 1, max_m), dtype=np.float64)
    for m in range(1, max_m + 1):
        for k in range(m):
            w[m, k] = (math.factorial(k) * math.factorial(m - 1 - k)
                       / math.factorial(m))
    return w


def shap_tables(forest: Forest):
    """Cached leaf-path tables of a standard forest, float64,
    shared by shap_values and the GPU pack. Flat arrays, leaves in (tree,
    ascending node id) order, entries in order of first appearance on the
    root-to-leaf path, path nodes in path order within their entry:

    ``tree_leaf_off`` [T+1], ``leaf_L`` f64, ``leaf_node``, ``leaf_ent_off``
    [leaves+1], ``ent_feat`` int32, ``ent_z`` f64, ``ent_pn_off``
    [entries+1], ``pn_tree``/``pn_node`` (the internal nodes an entry
    merges) and ``pn_left`` (True: the path turns left there), plus
    ``max_m`` and ``root_sum`` = sum_t E[root_t] (float64).

    Dropped by forest.invalidate_derived(), like explain_tables."""
    tabs = getattr(forest, "_shap_tables", None)
    if tabs is not None:
        return tabs
    if isinstance(forest, ExtendedForest):
        raise ValueError("SHAP values are defined for standard forests only")
    E, n = node_expectations(forest)
    Lall = _leaf_path_values(forest).astype(np.float64)
    feat_all, right_all = forest.feature, forest.right
    T = forest.num_trees
    tree_leaf_off = [0]
    leaf_L, leaf_node, leaf_ent_off = [], [], [0]
    ent_feat, ent_z, ent_pn_off = [], [], [0]
    pn_tree, pn_node, pn_left = [], [], []
    for t in range(T):
        feat = feat_all[t].tolist()
        right = right_all[t].tolist()
        nt = n[t].tolist()
        # depth-first walk. In a pre-order layout (right[v] past the whole
        # left subtree: every forest built here) it meets the leaves in id
        # order; the sort below makes the order the contract's for any
        # layout with left = id + 1.
        found = []  # (leaf id, merged entries)
        path = []  # (node, went_left)
        stack = [(0, 0)]  # (node, path length on arrival)
        while stack:
            v, plen = stack.pop()
            del path[plen:]
            f = feat[v]
            if f >= 0:
                stack.append((right[v], plen + 1))
                stack.append((v + 1, plen + 1))
                path.append([v, True])
                continue
            if f != Forest.LEAF:
                continue  # pad (never reached from a well-formed root)
            # `path` holds the ancestors; the turn taken at each is known
            # from the next node on the path (left child = id + 1)
            nodes = [pv for pv, _ in path]
            nxt = nodes[1:] + [v]
            slot = {}
            groups = []
            for pv, child in zip(nodes, nxt):
                fv = feat[pv]
                ratio = (float(nt[child]) / float(nt[pv])) if nt[pv] > 0 \
                    else 0.5
                k = slot.get(fv)
                if k is None:
                    slot[fv] = len(groups)
                    groups.append([fv, ratio, [(pv, child == pv + 1)]])
                else:
                    g = groups[k]
                    g[1] = g[1] * ratio
                    g[2].append((pv, child == pv + 1))
            found.append((v, groups))
        found.sort(key=lambda leaf: leaf[0])
        for v, groups in found:
            leaf_L.append(Lall[t, v])
            leaf_node.append(v)
            for fv, z, pns in groups:
                ent_feat.append(fv)
                ent_z.append(z)
                for pv, left in pns:
                    pn_tree.append(t)
                    pn_node.append(pv)
                    pn_left.append(left)
                ent_pn_off.append(len(pn_node))
            leaf_ent_off.append(len(ent_feat))
        tree_leaf_off.append(len(leaf_L))
    leaf_ent_off = np.asarray(leaf_ent_off, dtype=np.int64)
    leaf_m = np.diff(leaf_ent_off)
    tabs = {
        "tree_leaf_off": np.asarray(tree_leaf_off, dtype=np.int64),
        "leaf_L": np.asarray(leaf_L, dtype=np.float64),
        "leaf_node": np.asarray(leaf_node, dtype=np.int64),
        "leaf_ent_off": leaf_ent_off,
        "leaf_m": leaf_m,
        "ent_feat": np.asarray(ent_feat, dtype=np.int32),
        "ent_z": np.asarray(ent_z, dtype=np.float64),
        "ent_pn_off": np.asarray(ent_pn_off, dtype=np.int64),
        "pn_tree": np.asarray(pn_tree, dtype=np.int64),
        "pn_node": np.asarray(pn_node, dtype=np.int64),
        "pn_left": np.asarray(pn_left, dtype=bool),
        "max_m": int(leaf_m.max(initial=0)),
        "root_sum": float(E[:, 0].sum()) if T else 0.0,
    }
    forest._shap_tables = tabs
    return tabs


def _shap_leaf_terms(o: np.ndarray, z: np.ndarray, L: np.ndarray,
                     w: np.ndarray) -> np.ndarray:
    """The §9 inner loop for G leaves that all merge m features: o bool
    [N, G, m], z f64 [G, m], L f64 [G] -> the terms (L*(o_a - z_a))*W,
    f64 [N, G, m]. Every operation is one separately rounded float64
    numpy ufunc, in the contract's order."""
    N, G, m = o.shape
    out = np.empty((N, G, m), dtype=np.float64)
    of = o.astype(np.float64)
    for a in range(m):
        c = np.zeros((m + 1, N, G), dtype=np.float64)
        c[0] = 1.0
        cnt = 0
        for b in range(m):
            if b == a:
                continue
            ob = o[:, :, b]
            zb = z[None, :, b]
            for k in range(cnt, -1, -1):
                c[k + 1] = np.where(ob, c[k + 1] + c[k], c[k + 1])
                c[k] = c[k] * zb
            cnt += 1
        W = np.zeros((N, G), dtype=np.float64)
        for k in range(m):
            W = W + c[k] * w[m][k]
        out[:, :, a] = (L[None, :] * (of[:, :, a] - z[None, :, a])) * W
    return out


def shap_raw_sums(forest: Forest, X: np.ndarray) -> np.ndarray:
    """float64 [N, d]: the unrounded accumulators of shap_values (the sums
    over trees, before the division by T and the float32 rounding)."""
    X = np.asarray(X)
    N, d = X.shape
    tabs = shap_tables(forest)
    fmax = int(tabs["ent_feat"].max(initial=-1))
    if fmax >= d:
        raise ValueError(
            f"the forest splits on feature {fmax} but rows have {d} columns")
    w = shap_weights(max(tabs["max_m"], SHAP_MAX_PATH_FEATURES))
    v64_all = (forest.value64 if getattr(forest, "value64", None) is not None
               else forest.value.astype(np.float64))
    X64 = X.astype(np.float64)
    acc = np.zeros((N, d), dtype=np.float64)
    leaf_ent_off, leaf_m = tabs["leaf_ent_off"], tabs["leaf_m"]
    ent_feat, ent_z = tabs["ent_feat"], tabs["ent_z"]
    ent_pn_off = tabs["ent_pn_off"]
    n_leaves = len(tabs["leaf_L"])
    # leaves in chunks that bound the [N, entries] temporaries
    chunk = max(1, int(4e6 // max(N * max(tabs["max_m"], 1), 1)))
    for l0 in range(0, n_leaves, chunk):
        l1 = min(n_leaves, l0 + chunk)
        e0, e1 = int(leaf_ent_off[l0]), int(leaf_ent_off[l1])
        if e1 == e0:
            continue  # single-leaf trees carry no entry
        p0, p1 = int(ent_pn_off[e0]), int(ent_pn_off[e1])
        pt, pv = tabs["pn_tree"][p0:p1], tabs["pn_node"][p0:p1]
        # the engine's own decision: f64(x) < value64, NaN goes right
        goes_left = X64[:, forest.feature[pt, pv]] < v64_all[pt, pv][None, :]
        agree = goes_left == tabs["pn_left"][p0:p1][None, :]
        o_ent = np.logical_and.reduceat(agree, ent_pn_off[e0:e1] - p0, axis=1)
        terms = np.empty((N, e1 - e0), dtype=np.float64)
        ms = leaf_m[l0:l1]
        for m in np.unique(ms):
            if m == 0:
                continue
            ls = np.nonzero(ms == m)[0] + l0
            cols = (leaf_ent_off[ls][:, None] - e0
                    + np.arange(m, dtype=np.int64)[None, :])  # [G, m]
            tm = _shap_leaf_terms(o_ent[:, cols], ent_z[cols + e0],
                                  tabs["leaf_L"][ls], w)
            terms[:, cols.reshape(-1)] = tm.reshape(N, -1)
        # the adds, in the contract's order: tree, leaf, entry
        for e in range(e0, e1):
            f = ent_feat[e]
            acc[:, f] = acc[:, f] + terms[:, e - e0]
    return acc


def shap_values(forest: Forest, X: np.ndarray,
                finalize: bool = True) -> np.ndarray:
    """Exact path-dependent TreeSHAP values, float32 [N, d]:
    the Shapley values of the game sum_t v_t(S), where v_t descends tree t
    taking the row's branch at splits on features in S and the
    cover-weighted average of both children elsewhere. finalize=True
    returns f32(acc / f64(T)), else f32(acc); with expected_path_length
    the row sums reproduce the mean path length. Negative = more
    anomalous, as in feature_contributions."""
    acc = shap_raw_sums(forest, X)
    if finalize:
        acc = acc / np.float64(forest.num_trees)
    return acc.astype(np.float32)
