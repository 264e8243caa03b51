"""Heap node records of the 16-bit standard scoring walk (score_forest_heap,
forest_kernels.hip), checked without a GPU: a numpy reference of the layout
v4_heap_order writes, and a numpy walk of it, against the strict-order CPU
engine. tests/test_score_heap_gpu.py compares the kernels with the same
reference word for word.

Layout (uint32 [Tpad][2^(H+1)], root at slot 1, children of c at 2c, 2c+1):
internal = thr16 << 16 | feature * slab_bytes; a leaf above level H passes
through to the right (low half = the sentinel slab, high half 0) down to
level H, which holds the f32 bits of depth + c(m); every other slot is 0.
"""

import numpy as np
import pytest

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.ops import gpu_engine


def round_rows(X, kind):
    """f32 values exact in the row dtype."""
    import torch

    if kind == "bf16":
        return torch.from_numpy(np.array(X)).to(torch.bfloat16).float().numpy()
    with np.errstate(over="ignore"):
        return np.asarray(X).astype(np.float16).astype(np.float32)


def row_keys(X, kind):
    """u16 keys [N, d + 1] of rows exact in `kind`, with the all-ones
    sentinel column the tile appends (device key16 / key16_f16)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if kind == "bf16":
        bits = (X.view(np.uint32) >> 16).astype(np.uint32)
        nan_above = 0x7F80
    else:
        with np.errstate(over="ignore"):
            bits = X.astype(np.float16).view(np.uint16).astype(np.uint32)
        nan_above = 0x7C00
    m = bits & 0x7FFF
    k = np.where(bits & 0x8000, 0x7FFF - m, 0x8000 + m).astype(np.uint32)
    k[m == 0] = 0x8000
    k[m > nan_above] = 0xFFFF
    return np.concatenate(
        [k, np.full((len(X), 1), 0xFFFF, dtype=np.uint32)], axis=1)


def heap_reference(packed, H, slab_bytes):
    """The heap records of pre-order v4 records [Tpad, mn, 2]."""
    Tpad = packed.shape[0]
    out = np.zeros((Tpad, 2 << H), dtype=np.uint32)
    for t in range(Tpad):
        meta = packed[t, :, 0]
        w1 = packed[t, :, 1].view(np.uint32)
        feat = (meta & 0xFFF).astype(np.int64)
        link = (meta >> 12) & 0x7FFF
        todo = [(0, 1, 0)]  # (pre-order node, slot, level)
        while todo:
            node, c, k = todo.pop()
            if k == H:
                assert link[node] == node, "tree deeper than H"
                out[t, c] = w1[node]
            elif link[node] == node:  # leaf above level H: pass right
                out[t, c] = feat[node] * slab_bytes
                todo.append((node, 2 * c + 1, k + 1))
            else:
                out[t, c] = (int(w1[node]) & 0xFFFF0000) | \
                    int(feat[node] * slab_bytes)
                todo.append((node + 1, 2 * c, k + 1))
                todo.append((int(link[node]), 2 * c + 1, k + 1))
    return out


def heap_walk(heap, keys, H, slab_bytes, num_trees):
    """Path sums of key rows over heap records: the kernel's visit, f32 adds
    in tree order."""
    rows = np.arange(len(keys))
    ps = np.zeros(len(keys), dtype=np.float32)
    for t in range(num_trees):
        cur = np.ones(len(keys), dtype=np.int64)
        for _ in range(H):
            rec = heap[t][cur]
            key = keys[rows, (rec & 0xFFFF) // slab_bytes]
            cur = 2 * cur + (key >= (rec >> 16))
        assert (cur >= (1 << H)).all() and (cur < (2 << H)).all()
        ps = (ps + heap[t][cur].view(np.float32)).astype(np.float32)
    return ps


def make_forest(d, n, T, kind, constant=False, seed=17):
    rows = max(1000, n + 100)
    if constant:
        X = np.full((rows, d), 1.5, dtype=np.float32)
    else:
        X = round_rows(np.random.RandomState(1000 + d)
                       .standard_normal((rows, d)).astype(np.float32), kind)
    bag = cpu_engine.sample_bags(rows, T, n, seed=seed, bootstrap=False)
    fs = cpu_engine.feature_subsets(d, d, T, seed=seed)
    return cpu_engine.build_forest(X, bag, fs, seed, n, d, d)


def split_rows(forest, N, d, kind):
    """Rows made of the forest's own split values rounded into the row
    dtype: where the rounding is exact the compare meets equality, which
    must go right."""
    internal = forest.feature >= 0
    vals = gpu_engine._split_thresholds32(forest)[internal]
    if len(vals) == 0:
        vals = np.array([1.5], dtype=np.float32)
    return round_rows(np.resize(vals.astype(np.float32), (N, d)), kind)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("n", [2, 3, 8, 64, 256, 300])
def test_reference_walk_matches_cpu_engine(n, kind):
    d, T = 5, 9
    forest = make_forest(d, n, T, kind)
    packed, ncount, H = gpu_engine._nodes_packed_v4(forest, d, kind)
    assert H == max(int(np.ceil(np.log2(n))), 1)
    slab = 1024
    heap = heap_reference(packed, H, slab)
    assert heap.shape == (16, 2 << H)
    rs = np.random.RandomState(n)
    X = round_rows(rs.standard_normal((700, d)).astype(np.float32), kind)
    X[:50] = split_rows(forest, 50, d, kind)
    X[50, :] = np.nan
    X[51, :] = np.inf
    X[52, :] = -np.inf
    X[53, :] = [0.0, -0.0, 1e20, -1e20, 1e-20][:d]
    got = heap_walk(heap, row_keys(X, kind), H, slab, T)
    with np.errstate(all="ignore"):
        want = cpu_engine.path_lengths(forest, X)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_reference_single_leaf_and_padding_trees():
    d, kind = 5, "bf16"
    forest = make_forest(d, 64, 9, kind, constant=True)
    packed, ncount, H = gpu_engine._nodes_packed_v4(forest, d, kind)
    assert (ncount == 1).all() and H == 1
    slab = 1024
    heap = heap_reference(packed, H, slab)
    # root passes through the sentinel slab to slot 3; slot 2 never reached
    assert (heap[:, 1] == d * slab).all()
    assert (heap[:, 2] == 0).all() and (heap[:, 0] == 0).all()
    np.testing.assert_array_equal(heap[:, 3], packed[:, 0, 1].view(np.uint32))
    assert (heap[9:, 3] == 0).all()  # padding trees end in 0.0f
    X = round_rows(np.random.RandomState(1).standard_normal((100, d))
                   .astype(np.float32), kind)
    got = heap_walk(heap, row_keys(X, kind), H, slab, 9)
    want = cpu_engine.path_lengths(forest, X)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
