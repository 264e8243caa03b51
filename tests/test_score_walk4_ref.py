"""The four-instruction visit of score_forest_heap (forest_kernels.hip),
checked without a GPU.

The kernel tracks the complemented slot n = ~cur and stages every tree
reversed in LDS (word c of the global tree at word slots-1-c of its window),
so that the record of cur sits at tree_end + n with n read as a negative
int. With x = key - thr16 in 32 bits, bit 31 of x is `key < thr16`, and
cur' = 2*cur + (key >= thr16) becomes n' = (n << 1) | (x >> 31) mod 2^32.
Here: the identity itself, and a numpy walk of a reversed copy of the
reference heap layout against the strict-order CPU engine (bitwise).
"""

import numpy as np
import pytest

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.ops import gpu_engine
from tests.test_score_heap_ref import (
    heap_reference,
    heap_walk,
    make_forest,
    round_rows,
    row_keys,
    split_rows,
)

_EDGES = [0, 1, 2, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF]


def test_identity():
    rs = np.random.RandomState(4)
    pairs = [(k, t) for k in _EDGES for t in _EDGES]
    pairs += [tuple(p) for p in rs.randint(0, 0x10000, size=(400, 2))]
    # equal and neighbouring random pairs too: the >= edge
    pairs += [(int(v), int(v)) for v in rs.randint(0, 0x10000, size=50)]
    pairs += [(int(v), int(v) + 1) for v in rs.randint(0, 0xFFFF, size=50)]
    pairs += [(int(v) + 1, int(v)) for v in rs.randint(0, 0xFFFF, size=50)]
    k = np.array([p[0] for p in pairs], dtype=np.uint32)[:, None]
    t = np.array([p[1] for p in pairs], dtype=np.uint32)[:, None]
    c = np.arange(0, (1 << 13) + 1, dtype=np.uint32)[None, :]
    want = ~(2 * c + (k >= t).astype(np.uint32))
    x = k - t  # wraps mod 2^32
    got = ((~c) << np.uint32(1)) | (x >> np.uint32(31))
    assert want.dtype == np.uint32 and got.dtype == np.uint32
    assert x.dtype == np.uint32 and (x[k < t] >> 31 == 1).all()
    np.testing.assert_array_equal(got, want)


def walk4(heap, keys, H, slab_bytes, num_trees):
    """The kernel's walk: reversed trees, complemented slot, subtract and
    funnel shift, f32 adds in tree order."""
    slots = 2 << H
    rev = np.ascontiguousarray(heap[:, ::-1])  # word c -> word slots-1-c
    rows = np.arange(len(keys))
    ps = np.zeros(len(keys), dtype=np.float32)
    for t in range(num_trees):
        tree = rev[t]
        n = np.full(len(keys), 0xFFFFFFFE, dtype=np.uint32)  # ~1
        for _ in range(H):
            at = slots + n.view(np.int32).astype(np.int64)  # tree_end + n
            assert (at >= 0).all() and (at < slots - 1).all()
            rec = tree[at]
            key = keys[rows, (rec & 0xFFFF) // slab_bytes].astype(np.uint32)
            x = key - (rec >> np.uint32(16))
            n = (n << np.uint32(1)) | (x >> np.uint32(31))
        cur = ~n
        assert (cur >= (1 << H)).all() and (cur < (2 << H)).all()
        at = slots + n.view(np.int32).astype(np.int64)
        ps = (ps + tree[at].view(np.float32)).astype(np.float32)
    return ps


def _rows_for(forest, d, kind, seed):
    rs = np.random.RandomState(seed)
    X = round_rows(rs.standard_normal((700, d)).astype(np.float32), kind)
    X[:50] = split_rows(forest, 50, d, kind)
    X[50, :] = np.nan
    X[51, :] = np.inf
    X[52, :] = -np.inf
    X[53, :] = [0.0, -0.0, 1e20, -1e20, 1e-20][:d]
    return X


_FORESTS = {}


def _case(n, kind, constant=False):
    key = (n, kind, constant)
    if key not in _FORESTS:
        d, T = 5, 9
        if constant == "column":
            rows = max(1000, n + 100)
            X = round_rows(np.random.RandomState(1000 + d)
                           .standard_normal((rows, d)).astype(np.float32),
                           kind)
            X[:, 0] = 2.5
            bag = cpu_engine.sample_bags(rows, T, n, seed=17,
                                         bootstrap=False)
            fs = cpu_engine.feature_subsets(d, d, T, seed=17)
            forest = cpu_engine.build_forest(X, bag, fs, 17, n, d, d)
        else:
            forest = make_forest(d, n, T, kind, constant=bool(constant))
        _FORESTS[key] = forest
    return _FORESTS[key]


# n = 2, 3, 256, 4096 give H = 1, 2, 8, 12
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("n", [2, 3, 256, 4096])
def test_reversed_walk_matches_cpu_engine(n, kind):
    d, T = 5, 9
    forest = _case(n, kind)
    packed, ncount, H = gpu_engine._nodes_packed_v4(forest, d, kind)
    assert H == {2: 1, 3: 2, 256: 8, 4096: 12}[n]
    slab = 1024
    heap = heap_reference(packed, H, slab)
    X = _rows_for(forest, d, kind, n)
    keys = row_keys(X, kind)
    got = walk4(heap, keys, H, slab, T)
    with np.errstate(all="ignore"):
        want = cpu_engine.path_lengths(forest, X)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # and the direct form of the same records
    direct = heap_walk(heap, keys, H, slab, T)
    assert np.array_equal(got.view(np.int32), direct.view(np.int32))


@pytest.mark.parametrize("shape", ["single-leaf", "column"])
def test_reversed_walk_pass_through(shape):
    """Leaves above level H: pass-through records (threshold 0, sentinel
    key 0xFFFF), where 0xFFFF - 0 is not negative and the walk goes right."""
    d, T, kind = 5, 9, "bf16"
    if shape == "single-leaf":
        forest = _case(64, kind, constant=True)
    else:
        forest = _case(256, kind, constant="column")
    packed, ncount, H = gpu_engine._nodes_packed_v4(forest, d, kind)
    if shape == "single-leaf":
        assert (ncount == 1).all() and H == 1
    else:
        depth = gpu_engine._node_depths(forest.feature, forest.right)
        assert depth[forest.feature == -1].min() <= 3 and H == 8
    slab = 1024
    heap = heap_reference(packed, H, slab)
    # pass-through records exist: sentinel slab, threshold 0
    assert (heap[:T, 1:1 << H] == d * slab).any()
    X = _rows_for(forest, d, kind, 7)
    got = walk4(heap, row_keys(X, kind), H, slab, T)
    with np.errstate(all="ignore"):
        want = cpu_engine.path_lengths(forest, X)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
