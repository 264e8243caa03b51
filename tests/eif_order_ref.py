"""Order-exact numpy references for the extended-forest (EIF) scoring
kernels, and mirrors of the staging choices their binding makes. No GPU.

The dense EIF kernels reassociate the hyperplane dot into four chains, so
they differ from cpu_engine.path_lengths_extended on rows that sit within
rounding of a hyperplane. They are still deterministic IEEE code:

  score_extended_dense_kernel   chain j % 4, ascending j, mul then add
  score_extended_dense_v2       chain j % 4, ascending j, fused multiply-add
                                over weights zero-padded to D columns

and both combine the chains as (a0 + a1) + (a2 + a3). walk_chain4 repeats
exactly that, so the kernels can be held to it bit for bit, knife edges
included. plant_knife_edges makes the rows on which the orders disagree.

Used by tests/test_eif_variants_ref.py (CPU) and
tests/test_eif_variants_gpu.py.
"""

import numpy as np

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.core.forest import ExtendedForest
from isolation_forest_amd.utils.det_math import bf16_round
from isolation_forest_amd.utils.math import avg_path_length

_TWO128 = 2.0 ** 128

# ---------------------------------------------------------------------------
# float32 fused multiply-add
# ---------------------------------------------------------------------------


def fma32(a, b, c, stats=None):
    """round_f32(a * b + c) with one rounding, elementwise on f32 arrays.

    The f64 product of two f32 values is exact (48 <= 53 bits). s = p + c is
    rounded to f64, and TwoSum gives its exact error e. Rounding s to f32
    can only differ from rounding the exact sum when s lies exactly halfway
    between two f32 values and e != 0 (53 >= 24 + 2 bits): the tie then
    breaks towards e. Denormal results are kept (numpy casts round into the
    denormal range correctly). inf and NaN follow IEEE through the f64 ops;
    their e is NaN, which takes no correction. `stats`, a dict, counts the
    corrections taken under "ties"."""
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        r = s.astype(np.float32)
        rd = r.astype(np.float64)
        # an f64 sum past the largest f32 rounds to inf; seen from s the
        # value above FLT_MAX on the f32 grid is 2^128
        over = np.isinf(rd) & np.isfinite(s)
        rd = np.where(over, np.sign(s) * _TWO128, rd)
        lo32 = np.nextafter(r, np.float32(-np.inf))
        hi32 = np.nextafter(r, np.float32(np.inf))
        lo = lo32.astype(np.float64)
        hi = hi32.astype(np.float64)
        fix_dn = (s < rd) & (s - lo == rd - s) & (e < 0)
        fix_up = (s > rd) & (s - rd == hi - s) & (e > 0)
    out = np.where(fix_dn, lo32, np.where(fix_up, hi32, r)).astype(np.float32)
    if stats is not None:
        stats["ties"] = stats.get("ties", 0) + int(fix_dn.sum() + fix_up.sum())
    return out


# ---------------------------------------------------------------------------
# the oracle's walk with a chosen dot
# ---------------------------------------------------------------------------

MODES = ("strict", "muladd", "fma")


def _f32(x):
    return x.astype(np.float32)


def _dot_strict(hidx, hw, Xr):
    """cpu_engine.path_lengths_extended: sparse terms, one accumulator."""
    acc = np.zeros(len(Xr), dtype=np.float32)
    rows = np.arange(len(Xr))
    for j in range(hidx.shape[1]):
        acc = _f32(acc + _f32(hw[:, j] * Xr[rows, hidx[:, j]]))
    return acc


def _dot_chain4(hidx, hw, Xr, fused, D):
    d = Xr.shape[1]
    W = np.zeros((len(Xr), D), dtype=np.float32)
    np.put_along_axis(W, hidx.astype(np.int64), hw, axis=1)
    zero = np.zeros(len(Xr), dtype=np.float32)
    a = [zero.copy() for _ in range(4)]
    for j in range(D):
        w = W[:, j]
        x = Xr[:, j] if j < d else zero  # rows are zero-padded to D too
        if fused:
            a[j % 4] = fma32(w, x, a[j % 4])
        else:
            a[j % 4] = _f32(a[j % 4] + _f32(w * x))
    return _f32(_f32(a[0] + a[1]) + _f32(a[2] + a[3]))


def walk_chain4(forest, X, mode, D=None, trace=None):
    """Path sums f32 [N] of `forest` over f32 rows X, walking as
    cpu_engine.path_lengths_extended does, with the dot of `mode`:

      "strict"  the oracle's own: sparse terms in stored order, one f32
                accumulator (bitwise path_lengths_extended; this is the
                check that the walker is right)
      "muladd"  weights densified by hyper_idx and zero-padded to D (default
                d); four f32 accumulators, term j into chain j % 4 in
                ascending j, product rounded and then added
      "fma"     the same chains with fma32

    The chains combine as f32(f32(a0 + a1) + f32(a2 + a3)); a row goes left
    when dot < offset. Each tree adds f32(depth) + leaf in tree order, in
    f32. `trace`, a dict, receives "max_node": the largest node id visited.
    """
    assert mode in MODES, mode
    X = np.ascontiguousarray(X, dtype=np.float32)
    N, d = X.shape
    D = d if D is None else D
    assert D >= d
    total = np.zeros(N, dtype=np.float32)
    max_node = 0
    with np.errstate(all="ignore"):
        for t in range(forest.num_trees):
            feat, val = forest.feature[t], forest.value[t]
            right = forest.right[t]
            hidx, hw = forest.hyper_idx[t], forest.hyper_w[t]
            cur = np.zeros(N, dtype=np.int64)
            depth = np.zeros(N, dtype=np.int32)
            while True:
                rows = np.nonzero(feat[cur] >= 0)[0]
                if len(rows) == 0:
                    break
                nodes = cur[rows]
                if mode == "strict":
                    dot = _dot_strict(hidx[nodes], hw[nodes], X[rows])
                else:
                    dot = _dot_chain4(hidx[nodes], hw[nodes], X[rows],
                                      mode == "fma", D)
                cur[rows] = np.where(dot < val[nodes], nodes + 1,
                                     right[nodes])
                depth[rows] += 1
            max_node = max(max_node, int(cur.max()))
            total = _f32(total + _f32(depth.astype(np.float32) + val[cur]))
    if trace is not None:
        trace["max_node"] = max_node
    return total


# ---------------------------------------------------------------------------
# rows and forests
# ---------------------------------------------------------------------------

KINDS = ("f32", "bf16", "f16")
ELEM = {"f32": 4, "bf16": 2, "f16": 2}


def round_rows(X, kind):
    """f32 values exact in the row dtype `kind`."""
    X = np.asarray(X, dtype=np.float32)
    if kind == "bf16":
        return bf16_round(X)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return X.astype(np.float16).astype(np.float32)
    assert kind == "f32", kind
    return X


def plant_knife_edges(forest, X, rs, frac, kind="f32"):
    """Copy of X in which a fraction `frac` of the rows lies on a hyperplane
    of their own walk: pick a tree and a node on the row's f64 walk, move the
    row along the node's weight vector until its f64 dot equals the offset,
    and round to the row dtype. In f32 the row then sits within a rounding
    of the plane, where the summation order decides the branch. A 16-bit
    grid is 2^15 times coarser than the f32 dot, so a rounded bf16 / fp16
    row lands clear of the plane. There the move leaves out the three
    coordinates with the heaviest weights, and these are then set one after
    another to (what is still missing) / weight, rounded: each takes the
    distance down by the grid's relative step (2^-8, 2^-11), and three of
    them bring it below the f32 rounding of the dot."""
    X = np.array(X, dtype=np.float32)
    for r in range(len(X)):
        if rs.rand() > frac:
            continue
        t = rs.randint(forest.num_trees)
        cur, path = 0, []
        while forest.feature[t, cur] >= 0:
            idx = forest.hyper_idx[t, cur]
            w = forest.hyper_w[t, cur].astype(np.float64)
            dot = float(w @ X[r, idx].astype(np.float64))
            path.append(cur)
            cur = (cur + 1 if dot < forest.value[t, cur]
                   else int(forest.right[t, cur]))
        node = path[rs.randint(len(path))]
        idx = forest.hyper_idx[t, node]
        w = forest.hyper_w[t, node].astype(np.float64)
        x = X[r, idx].astype(np.float64)
        off = float(forest.value[t, node])
        # 16-bit rows: the three heaviest coordinates are kept back to take
        # up what rounding leaves (below)
        held = (np.argsort(-np.abs(w))[:3]
                if kind != "f32" and len(w) >= 5 else np.zeros(0, np.int64))
        free = np.ones(len(w), dtype=bool)
        free[held] = False
        x[held] = 0.0
        wf = np.where(free, w, 0.0)
        x = round_rows((x + (off - float(w @ x)) * wf / float(wf @ wf))
                       .astype(np.float32), kind).astype(np.float64)
        for k in held:
            x[k] = round_rows(np.float32((off - float(w @ x)) / w[k]), kind)
        X[r, idx] = x.astype(np.float32)
    return X


def trained_extended_forest(n, d, T, ext, seed=17):
    """CPU-built EIF on f32 Gaussian rows (max(4000, n + 100) of them)."""
    rows = max(4000, n + 100)
    X = np.random.RandomState(1000 + d).normal(size=(rows, d)).astype(
        np.float32)
    bag = cpu_engine.sample_bags(rows, T, n, seed=seed, bootstrap=False)
    fs = cpu_engine.feature_subsets(d, d, T, seed=seed)
    return cpu_engine.build_extended_forest(X, bag, fs, seed, n, d, d, ext)


def complete_extended_forest(height, nnz, d, T, seed):
    """Synthetic pre-order COMPLETE binary forest: 2^(height+1) - 1 nodes
    per tree, every slot live. Internal nodes carry a random unit hyperplane
    on nnz sorted coordinates with offset 0, so a Gaussian row halves at
    every level and node ids up to the last one are visited (an all-zero
    row goes right everywhere and ends on it). Leaf l of a tree has the
    value l * 2^-height: distinct, and exact in every f32 sum the walk
    makes, so a path sum names the leaves that were reached."""
    rs = np.random.RandomState(seed)
    mn = 2 ** (height + 1) - 1
    feature = np.empty(mn, dtype=np.int32)
    right = np.full(mn, -1, dtype=np.int32)
    stack = [(0, height)]  # (node id, height of its subtree)
    while stack:
        i, h = stack.pop()
        if h == 0:
            feature[i] = ExtendedForest.LEAF
            continue
        feature[i] = nnz
        right[i] = i + 2 ** h  # past the left subtree's 2^h - 1 nodes
        stack.append((i + 1, h - 1))
        stack.append((int(right[i]), h - 1))
    internal = feature >= 0
    leaf_rank = np.cumsum(~internal) - 1
    value1 = np.where(internal, 0.0, leaf_rank * 2.0 ** -height).astype(
        np.float32)

    fr_feature = np.tile(feature, (T, 1))
    hidx = np.zeros((T, mn, nnz), dtype=np.int32)
    hw = np.zeros((T, mn, nnz), dtype=np.float32)
    n_int = int(internal.sum())
    for t in range(T):
        keys = rs.random_sample((n_int, d))
        hidx[t, internal] = np.sort(np.argsort(keys, axis=1)[:, :nnz],
                                    axis=1).astype(np.int32)
        w = rs.normal(size=(n_int, nnz))
        w /= np.sqrt((w * w).sum(axis=1, keepdims=True))
        hw[t, internal] = w.astype(np.float32)
    return ExtendedForest(
        feature=fr_feature,
        value=np.tile(value1, (T, 1)),
        right=np.tile(right, (T, 1)),
        num_instances=np.tile(np.where(internal, -1, 1).astype(np.int64),
                              (T, 1)),
        node_count=np.full(T, mn, dtype=np.int32),
        hyper_idx=hidx,
        hyper_w=hw,
        offset64=np.zeros((T, mn), dtype=np.float64),
        num_samples=2 ** height,
        num_features=d,
        total_num_features=d,
        extension_level=nnz - 1,
    )


def c_norm(forest):
    return float(avg_path_length(forest.num_samples))


# ---------------------------------------------------------------------------
# mirrors of the score_extended_forest binding's instantiation predicates
# ---------------------------------------------------------------------------


def max_nodes_for(n):
    """Node slots per tree of a forest built with bag size n:
    2^(h+1) - 1 with h = ceil(log2 n), not 2n - 1."""
    h = int(np.ceil(np.log2(max(n, 2))))
    return 2 ** (h + 1) - 1


def takes_old_dense(d, max_nodes, nnz):
    """The binding's first branch: the old dense kernel, else the general
    one."""
    return nnz == d and d % 4 == 0 and max_nodes * 8 <= 120 * 1024


def old_dense_variant(d, max_nodes, elem):
    """(rows_lds, wlds) of score_extended_dense_kernel<XT, ROWS_LDS, WLDS>
    (mirror of the binding's LDS budget, elem = bytes per row element)."""
    node_bytes = max_nodes * 8
    dpad = d + 4  # d % 4 == 0 here: one float4 of padding
    drow_bytes = 256 * dpad * elem
    w_bytes = max_nodes * d * 4
    wlds = node_bytes + w_bytes + drow_bytes <= 152 * 1024
    rows_lds = node_bytes + (w_bytes if wlds else 0) + drow_bytes <= 152 * 1024
    return rows_lds, wlds


def general_variant(d, max_nodes, nnz, elem):
    """(rows_lds, hyper_lds, nodes_lds) of score_extended_forest_kernel<XT,
    ROWS_LDS, HYPER_LDS, NODES_LDS> (mirror of the binding's LDS budget)."""
    pad = 16 // elem
    row_bytes = 256 * (d + pad) * elem
    node_bytes = max_nodes * 8
    nodes_lds = node_bytes <= 120 * 1024
    nb = node_bytes if nodes_lds else 0
    hyper_bytes = max_nodes * nnz * 8
    hyper_lds = nb + hyper_bytes <= 96 * 1024
    rows_lds = nb + (hyper_bytes if hyper_lds else 0) + row_bytes <= 144 * 1024
    return rows_lds, hyper_lds, nodes_lds


def sparse_v2_declines(d, max_nodes, nnz, elem):
    """True when the router's sparse v2 LDS check sends an nnz <= 5 forest
    on to the general binding."""
    dpad = d
    while (dpad % 4 != 2) if elem == 2 else (dpad % 2 != 1):
        dpad += 1
    return max_nodes * (12 + nnz * 8) + 2 * 256 * dpad * elem > 150 * 1024
