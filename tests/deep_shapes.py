"""Forests and rows for the deep routes (ops/hip/deep_kernels.hip,
shap_forest_deep_kernel): the shapes at which the 20-bit link records, the
barrier phases and the key tile can go wrong. Pure numpy, no GPU.

Every forest has node arrays wider than 32767, so it leaves the packed
formats. The extended makers return the hyperplane twin of the standard
forest: nnz = 2 ascending coordinates with weight 1.0 on the split feature
and 0.0 on its neighbour, the threshold as offset, so that the strict dot of
a finite row is the cell itself.

  trie(H, d)               one complete tree of height H, 2^(H+1) - 1 nodes
  ragged(big)              nine trees from one record to thousands, spines
                           of depth 40 among them
  sliced(forest, T)        the first T trees
  knife_rows(forest, ...)  rows that sit on, and one step beside, thresholds
                           their own walk reaches; signed zeros, denormals,
                           the largest finite values, NaN and infinities
  foreign64(forest)        float64 splits strictly between two f32 values

Used by tests/test_deep_shapes_ref.py (CPU), which asserts that each of them
reaches what it was made for, and tests/test_deep_shapes_gpu.py.
"""

import dataclasses
import functools

import numpy as np
import torch

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.core.forest import (
    ExtendedForest, Forest, empty_extended_forest, empty_forest)

KINDS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
N_BAG = 16385  # one past the packed formats' bag
MIN_WIDTH = 2 * N_BAG - 1  # the node arrays of such a bag
SPINE_DEPTH = 40
SPINE_FEATURES = 8


# ---------------------------------------------------------------------------
# single trees: dicts of pre-order arrays, one entry a node
# ---------------------------------------------------------------------------


def _tree(feature, value, right, count):
    return {"feature": np.asarray(feature, dtype=np.int32),
            "value": np.asarray(value, dtype=np.float32),
            "right": np.asarray(right, dtype=np.int32),
            "num_instances": np.asarray(count, dtype=np.int64)}


def leaf_tree(count=7):
    return _tree([Forest.LEAF], [0.0], [-1], [count])


def stump_tree(feature, value):
    return _tree([feature, Forest.LEAF, Forest.LEAF], [value, 0.0, 0.0],
                 [2, -1, -1], [-1, 3, 5])


def spine_values(depth):
    """Thresholds of a spine: sixteenths in (-1, 1), exact in bf16 and fp16,
    none repeated on one feature's turns."""
    return ((np.arange(depth) * 7) % 31 - 15).astype(np.float32) / 16


def right_spine_tree(depth=SPINE_DEPTH, nfeat=SPINE_FEATURES):
    """Node 2i splits on feature i % nfeat; its left child 2i + 1 is a leaf,
    its right child node 2i + 2 (the `chain` of tests/test_shap_deep_gpu.py)."""
    m = 2 * depth + 1
    feature = np.full(m, Forest.LEAF, dtype=np.int32)
    feature[0:2 * depth:2] = np.arange(depth) % nfeat
    value = np.zeros(m, dtype=np.float32)
    value[0:2 * depth:2] = spine_values(depth)
    right = np.full(m, -1, dtype=np.int32)
    right[0:2 * depth:2] = np.arange(2, 2 * depth + 2, 2)
    count = np.where(feature == Forest.LEAF, 1 + np.arange(m) % 5, -1)
    return _tree(feature, value, right, count)


def left_spine_tree(depth=SPINE_DEPTH, nfeat=SPINE_FEATURES):
    """Nodes 0 .. depth - 1 split on feature i % nfeat, each the left child
    of the one before; node depth is the deepest leaf and the right leaves
    follow from the bottom up."""
    m = 2 * depth + 1
    feature = np.full(m, Forest.LEAF, dtype=np.int32)
    feature[:depth] = np.arange(depth) % nfeat
    value = np.zeros(m, dtype=np.float32)
    value[:depth] = -spine_values(depth)
    right = np.full(m, -1, dtype=np.int32)
    right[:depth] = 2 * depth - np.arange(depth)
    count = np.where(feature == Forest.LEAF, 1 + np.arange(m) % 3, -1)
    return _tree(feature, value, right, count)


def trie_tree(H, d):
    """A complete tree of height H in pre-order. The node at depth k splits
    on feature k % d at the midpoint of the cell of [0, 1)^d it covers; leaf
    counts vary with the leaf's ordinal."""
    m = 2 ** (H + 1) - 1
    feature = np.full(m, Forest.LEAF, dtype=np.int32)
    value = np.zeros(m, dtype=np.float32)
    right = np.full(m, -1, dtype=np.int32)
    idx = np.zeros(1, dtype=np.int64)
    lo = np.zeros((1, d), dtype=np.float64)
    for k in range(H):
        f = k % d
        half = 0.5 ** (k // d + 1)  # the cell has been halved k // d times
        feature[idx] = f
        value[idx] = lo[:, f] + half  # dyadic: exact in every row kind
        right[idx] = idx + 2 ** (H - k)
        hi = lo.copy()
        hi[:, f] += half
        idx = np.concatenate([idx + 1, idx + 2 ** (H - k)])
        lo = np.concatenate([lo, hi])
    leaves = np.sort(idx)
    count = np.full(m, -1, dtype=np.int64)
    count[leaves] = 1 + np.arange(len(leaves)) % 1009
    return _tree(feature, value, right, count)


def tree_of(forest, t):
    """Tree t of a forest as a dict of its live nodes (extended: with the
    hyperplanes)."""
    n = int(forest.node_count[t])
    out = {k: getattr(forest, k)[t, :n].copy()
           for k in ("feature", "value", "right", "num_instances")}
    if isinstance(forest, ExtendedForest):
        out["hyper_idx"] = forest.hyper_idx[t, :n].copy()
        out["hyper_w"] = forest.hyper_w[t, :n].copy()
    return out


def _twin(tree, d):
    """The hyperplane twin of a standard tree (see the module docstring)."""
    if "hyper_idx" in tree:
        return tree
    f = tree["feature"]
    internal = f >= 0
    first = np.where(f + 1 < d, f, f - 1)  # the pair (f, f + 1) or (f - 1, f)
    hidx = np.zeros((len(f), 2), dtype=np.int32)
    hw = np.zeros((len(f), 2), dtype=np.float32)
    hidx[internal, 0] = first[internal]
    hidx[internal, 1] = first[internal] + 1
    hw[internal, 0] = (f == first)[internal]
    hw[internal, 1] = (f != first)[internal]
    out = dict(tree)
    out["feature"] = np.where(internal, 2, f).astype(np.int32)
    out["hyper_idx"], out["hyper_w"] = hidx, hw
    return out


def assemble(trees, d, num_samples, extended=False, width=MIN_WIDTH):
    """A forest of these trees in arrays `width` columns wide (wider where a
    tree needs it); leaf values come from the counts."""
    width = max([width] + [len(t["feature"]) for t in trees])
    T = len(trees)
    if extended:
        trees = [_twin(t, d) for t in trees]
        forest = empty_extended_forest(T, width, 2, num_samples, d, d, 1)
    else:
        forest = empty_forest(T, width, num_samples, d, d)
    for t, tree in enumerate(trees):
        n = len(tree["feature"])
        forest.node_count[t] = n
        for name, a in tree.items():
            getattr(forest, name)[t, :n] = a
    forest.leaf_values_from_counts()
    if extended:
        forest.offset64[:] = forest.value
    else:
        forest.value64[:] = forest.value
    return forest


# ---------------------------------------------------------------------------
# the forests
# ---------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def built(d, extended=False, T=5, k=None):
    """cpu_engine's forest over 20000 Gaussian rows of d columns at n = 16385
    (the forest of tests/test_score_deep_gpu.py at d = 6), each tree over k
    of the columns (all by default); extended ones at extensionLevel 1.
    Shared and read-only."""
    k = d if k is None else min(k, d)
    X = np.random.RandomState(5).standard_normal((20000, d)).astype(np.float32)
    bag = cpu_engine.sample_bags(20000, T, N_BAG, seed=31, bootstrap=False)
    fs = cpu_engine.feature_subsets(d, k, T, seed=31)
    if extended:
        return cpu_engine.build_extended_forest(X, bag, fs, 31, N_BAG, k, d, 1)
    return cpu_engine.build_forest(X, bag, fs, 31, N_BAG, k, d)


def trie(H, d, extended=False):
    """One complete tree of height H: 2^(H+1) - 1 nodes, 2^20 - 1 at
    H = 19, the largest odd count under the deep records' cap."""
    tree = trie_tree(H, d)
    n = int(tree["num_instances"][tree["feature"] == Forest.LEAF].sum())
    return assemble([tree], d, n, extended)


def ragged(big, extended=False):
    """Nine trees, three barrier phases of four with three pad trees, sizes
    mixed inside every phase. `big` is a built forest of the same kind with
    at least three trees at n = 16385 over SPINE_FEATURES columns; the
    hand-made trees of an extended forest are hyperplane twins."""
    assert isinstance(big, ExtendedForest) == extended
    d = SPINE_FEATURES
    assert big.total_num_features == d and big.num_trees >= 3
    assert not extended or big.nnz == 2
    trees = [
        leaf_tree(), tree_of(big, 0), right_spine_tree(), trie_tree(12, d),
        stump_tree(3, 0.25), left_spine_tree(), tree_of(big, 1), leaf_tree(2),
        tree_of(big, 2),
    ]
    return assemble(trees, d, big.num_samples, extended,
                    width=big.feature.shape[1])


def sliced(forest, T):
    """The first T trees as a forest of their own."""
    fields = {}
    for f in dataclasses.fields(forest):
        v = getattr(forest, f.name)
        fields[f.name] = v[:T].copy() if isinstance(v, np.ndarray) else v
    return type(forest)(**fields)


def foreign64(forest):
    """A copy whose float64 split sits strictly between the f32 split and
    its upper f32 neighbour on every other internal node, as a model trained
    in float64 elsewhere has them: x < value64 then also takes x == value
    to the left."""
    out = sliced(forest, forest.num_trees)
    internal = np.argwhere(out.feature >= 0)[::2]
    t, v = internal[:, 0], internal[:, 1]
    lo = out.value[t, v]
    up = np.nextafter(lo, np.float32(np.inf))
    out.value64[t, v] = (lo.astype(np.float64) + up.astype(np.float64)) / 2
    assert ((lo < out.value64[t, v]) & (out.value64[t, v] < up)).all()
    out.invalidate_derived()
    return out


# ---------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------


def widen(Xk):
    """The f32 values a device matrix of Xk's kind holds: the oracle's input."""
    return Xk.float().numpy()


def to_kind(X, kind):
    return torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(
        KINDS[kind])


def round_kind(v, kind):
    """f32 values rounded (RNE) to the kind and widened back."""
    return widen(to_kind(np.atleast_1d(v), kind))


def step_kind(v, kind, up):
    """The next value of the kind above (or below) v, for v of that kind."""
    v = np.atleast_1d(np.asarray(v, dtype=np.float32))
    toward = np.float32(np.inf if up else -np.inf)
    if kind == "f32":
        return np.nextafter(v, toward)
    if kind == "f16":
        return np.nextafter(v.astype(np.float16),
                            np.float16(toward)).astype(np.float32)
    # bf16: the upper half of the f32 word; step its magnitude-ordered integer
    b = v.view(np.uint32).astype(np.int64)
    o = np.where(b & 0x80000000, -(b & 0x7FFFFFFF), b) >> 16
    o = o + (1 if up else -1)
    b = np.where(o < 0, 0x80000000 | ((-o) << 16), o << 16)
    return b.astype(np.uint32).view(np.float32)


def special_cells(kind):
    """+0.0 and -0.0, the smallest and largest denormal and the largest
    finite value of the kind in both signs, NaN and both infinities."""
    if kind == "f32":
        mag = np.array([1, 0x007FFFFF, 0x7F7FFFFF], np.uint32).view(np.float32)
    elif kind == "bf16":
        mag = (np.array([1, 0x007F, 0x7F7F], np.uint32) << 16).view(np.float32)
    else:
        mag = np.array([1, 0x03FF, 0x7BFF], np.uint16).view(
            np.float16).astype(np.float32)
    return np.concatenate([np.float32([0.0, -0.0]), mag, -mag,
                           np.float32([np.nan, np.inf, -np.inf])])


def trie_rows(kind, d, n=2000, seed=3):
    """n rows of the kind, uniform in [-0.1, 1.1)^d: row 0 lies above every
    threshold of a trie and row 1 below every one."""
    X = np.random.RandomState(seed).uniform(-0.1, 1.1, (n, d))
    X[0], X[1] = 1.05, -0.05
    return to_kind(X, kind)


def walk(forest, X, t):
    """The oracle's walk of tree t: int64 [N, depth + 1] node ids, -1 past a
    row's leaf. Standard: x < value64; extended: the strict f32 dot < value."""
    N = X.shape[0]
    feat, right = forest.feature[t], forest.right[t]
    extended = isinstance(forest, ExtendedForest)
    thr = (forest.value[t] if extended or forest.value64 is None
           else forest.value64[t])
    cur = np.zeros(N, dtype=np.int64)
    steps = [cur.copy()]
    active = feat[cur] >= 0
    while active.any():
        rows = np.nonzero(active)[0]
        nodes = cur[rows]
        with np.errstate(all="ignore"):
            if extended:
                x = np.zeros(len(rows), dtype=np.float32)
                for j in range(forest.nnz):
                    x = x + forest.hyper_w[t, nodes, j] * X[
                        rows, forest.hyper_idx[t, nodes, j]]
            else:
                x = X[rows, feat[nodes]]
            left = x < thr[nodes]
        cur[rows] = np.where(left, nodes + 1, right[nodes])
        col = np.full(N, -1, dtype=np.int64)
        col[rows] = cur[rows]
        steps.append(col)
        active = np.zeros(N, dtype=bool)
        active[rows] = feat[cur[rows]] >= 0
    return np.stack(steps, axis=1)


def split_cell(forest, t, v):
    """The column a node compares alone, or -1: the split feature, or the
    coordinate of a hyperplane whose other weights are all zero."""
    if not isinstance(forest, ExtendedForest):
        return int(forest.feature[t, v])
    k = int(forest.feature[t, v])
    w = forest.hyper_w[t, v, :k]
    if (w != 0).sum() != 1 or w[w != 0][0] != 1.0:
        return -1
    return int(forest.hyper_idx[t, v, :k][w != 0][0])


def _touched(forest, t, v):
    """The columns that move a node's decision."""
    if not isinstance(forest, ExtendedForest):
        return {int(forest.feature[t, v])}
    k = int(forest.feature[t, v])
    return {int(c) for c, w in zip(forest.hyper_idx[t, v, :k],
                                   forest.hyper_w[t, v, :k]) if w != 0}


N_SPECIAL_ROWS = 22
N_RUNNER_ROWS = 4


def knife_rows(forest, kind, n, d=None, seed=11):
    """(rows of the kind on the host, planted): n Gaussian rows of d columns
    (the forest's own width by default) with planted cells. Row i < n - 26
    walks tree i % T; at a node of that walk whose column no earlier node of
    it reads, the cell becomes the threshold rounded to the kind (i % 3 == 0),
    the next value of the kind below that (1) or above it (2), so the row
    still reaches the node and is decided there by one step of its own
    type. `planted` lists (row, tree, node, column) of these. Four rows
    are +3.0 or -3.0 throughout, beyond every hand-made threshold: they run
    the spines to their ends. The last 22 rows carry special_cells(kind),
    each twice, one a row."""
    d = forest.total_num_features if d is None else d
    rs = np.random.RandomState(seed)
    X = round_kind(rs.standard_normal((n, d)).astype(np.float32).ravel(),
                   kind).reshape(n, d)
    T = forest.num_trees
    body = max(n - N_SPECIAL_ROWS - N_RUNNER_ROWS, 0)
    thr = forest.value
    planted = []
    for t in range(T):
        rows = np.arange(t, body, T)
        if not len(rows):
            continue
        paths = walk(forest, X[rows], t)
        for i, path in zip(rows, paths):
            seen, spots = set(), []
            for v in path[path >= 0]:
                if forest.feature[t, v] < 0:
                    break
                c = split_cell(forest, t, v)
                if c >= 0 and c not in seen:
                    spots.append((int(v), c))
                seen |= _touched(forest, t, v)
            if not spots:
                continue
            v, c = spots[rs.randint(len(spots))]
            cell = round_kind(thr[t, v], kind)
            if i % 3:
                cell = step_kind(cell, kind, up=i % 3 == 2)
            X[i, c] = cell[0]
            planted.append((int(i), t, v, c))
    for j in range(body, max(n - N_SPECIAL_ROWS, 0)):
        X[j] = 3.0 if j % 2 else -3.0
    cells = special_cells(kind)
    for j in range(min(N_SPECIAL_ROWS, n)):
        X[n - 1 - j, (3 * j) % d] = cells[j % len(cells)]
    Xk = to_kind(X, kind)
    held = widen(Xk)  # every planted value is one of the kind: kept exactly
    assert np.array_equal(np.isnan(held), np.isnan(X))
    assert np.array_equal(held.view(np.int32)[~np.isnan(X)],
                          X.view(np.int32)[~np.isnan(X)])
    return Xk, planted
