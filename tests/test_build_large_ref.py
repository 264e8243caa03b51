"""The case table of the large-bag GPU build tests, checked without a GPU.

tests/test_build_large_gpu.py builds every case below with
build_forest_large_kernel / build_extended_forest_large_kernel (bags of more
than 16384 rows: 32-bit row ids in global memory, one multi-wave block per
tree) and compares the result bitwise with the CPU oracle. As in
tests/test_build_shapes_ref.py, what a case is there for is a property of
the oracle's forest and is asserted here, on the oracle alone: node ids past
the int16 range, row positions past the uint16 range, a retry loop that runs
dry, empty sides, a Philox key with a non-zero high word.

Every case has T = 2. large_case(id) returns ``(X, bag, fs, seed, args)``,
cpu_large(id) the oracle's forest for it; both are computed once and handed
out read-only.
"""

import functools

import numpy as np
import pytest

from isolation_forest_amd.core.forest import Forest
from isolation_forest_amd.ops.gpu_engine import _node_depths
from tests.test_build_shapes_ref import (
    BIG_OFFSET,
    EXT_FIELDS,
    FIELDS,
    _case,
    _normal,
    build_extended,
    build_standard,
    height_limit,
    same_forest,
)

LDS_CAP = 16384
L1_N = LDS_CAP + 1
HIGH_SEED = (1 << 40) + 3  # Philox key word k1 = 256


def _l1_rows():
    """Gaussian rows, column 2 held constant."""
    X = _normal(20000, 4, 401)
    X[:, 2] = np.float32(-1.5)
    return X


def _binary(N, d, seed):
    return np.random.RandomState(seed).randint(0, 2, size=(N, d)).astype(
        np.float32)


def _table():
    tab = {}
    tab["L1"] = lambda: _case(_l1_rows(), L1_N, 2, 41)
    tab["L2"] = lambda: _case(_binary(40001, 15, 402), 40000, 2, 42,
                              bootstrap=True)
    tab["L3"] = lambda: _case(_binary(70001, 16, 403), 70000, 2, 43,
                              bootstrap=True)
    tab["L3-ext"] = lambda: _case(_binary(70001, 16, 403), 70000, 2, 43,
                                  bootstrap=True, level=1)
    tab["L4"] = lambda: _case(_l1_rows(), L1_N, 2, HIGH_SEED,
                              offset=BIG_OFFSET)
    tab["X1-full"] = lambda: _case(_l1_rows(), L1_N, 2, 44, level=3)
    tab["X1-nnz2k3"] = lambda: _case(_l1_rows(), L1_N, 2, 45, k=3, level=1)
    return tab


_TABLE = _table()
LARGE_IDS = list(_TABLE)
STANDARD_LARGE_IDS = ["L1", "L2", "L3", "L4"]
EXTENDED_LARGE_IDS = ["L3-ext", "X1-full", "X1-nnz2k3"]


def is_extended(cid):
    return cid in EXTENDED_LARGE_IDS


@functools.lru_cache(maxsize=None)
def large_case(cid):
    return _TABLE[cid]()


@functools.lru_cache(maxsize=None)
def cpu_large(cid):
    build = build_extended if is_extended(cid) else build_standard
    forest = build(large_case(cid))
    for name in EXT_FIELDS if is_extended(cid) else FIELDS:
        getattr(forest, name).setflags(write=False)
    return forest


def _live(forest):
    cols = np.arange(forest.feature.shape[1])[None, :]
    return cols < forest.node_count[:, None]


def _leaves(forest):
    return _live(forest) & (forest.feature == Forest.LEAF)


def _internal(forest):
    return _live(forest) & (forest.feature >= 0)


def test_the_table_is_the_issue_s():
    assert sorted(LARGE_IDS) == sorted(STANDARD_LARGE_IDS + EXTENDED_LARGE_IDS)


@pytest.mark.parametrize("cid", LARGE_IDS)
def test_case_is_well_formed(cid):
    X, bag, fs, seed, a = large_case(cid)
    forest = cpu_large(cid)
    n, T = a["n"], a["T"]
    assert T == 2 and n > LDS_CAP
    assert X.dtype == np.float32 and X.shape == (a["N"], a["d"])
    assert bag.shape == (T, n) and bag.min() >= 0 and bag.max() < a["N"]
    assert fs.shape == (T, a["k"])
    H = height_limit(n)
    if is_extended(cid):
        nnz = min(a["extension_level"] + 1, a["k"])
        assert forest.feature.shape == (T, 2 ** (H + 1) - 1)
        assert forest.hyper_idx.shape == (T, 2 ** (H + 1) - 1, nnz)
    else:
        assert forest.feature.shape == (T, 2 * n - 1)
    assert forest.feature.shape[1] > 32767  # past the one-wave kernels
    assert (forest.feature[~_live(forest)] == Forest.PAD).all()
    depth = _node_depths(forest.feature, forest.right)
    assert depth[_live(forest)].max() <= H
    counts = np.where(_leaves(forest), forest.num_instances, 0)
    np.testing.assert_array_equal(counts.sum(axis=1), np.full(T, n))


def test_l1_is_the_first_size_past_the_cap():
    X, bag, fs, seed, a = large_case("L1")
    assert a["n"] == 16385 and a["N"] == 20000 and a["d"] == 4
    assert (X[:, 2] == X[0, 2]).all()
    f = cpu_large("L1")
    # the constant column never splits; the others all do
    assert set(np.unique(f.feature[_internal(f)])) == {0, 1, 3}
    # several waves' worth of rows, and not a multiple of a wave or a block
    assert a["n"] % 64 == 1 and a["n"] % 256 == 1
    # Gaussian columns run into the height limit with fat leaves
    depth = _node_depths(f.feature, f.right)
    at_limit = _leaves(f) & (depth == height_limit(a["n"]))
    assert (at_limit & (f.num_instances > 1)).any()


def test_l2_node_ids_leave_int16_and_the_retry_runs_dry():
    X, bag, fs, seed, a = large_case("L2")
    assert (a["n"], a["N"], a["d"]) == (40000, 40001, 15) and a["bootstrap"]
    assert set(np.unique(X)) == {0.0, 1.0}
    f = cpu_large("L2")
    assert f.node_count.max() > 32767
    # a right-child link past int16 too
    assert f.right.max() > 32767
    # 2^15 distinct rows at most: segments of equal rows have every feature
    # constant and end as leaves of several rows above the height limit
    depth = _node_depths(f.feature, f.right)
    dry = _leaves(f) & (f.num_instances > 1) & (depth < height_limit(40000))
    assert dry.any()
    for row in bag:
        assert len(np.unique(row)) < len(row)


@pytest.mark.parametrize("cid", ["L3", "L3-ext"])
def test_l3_row_positions_leave_uint16(cid):
    X, bag, fs, seed, a = large_case(cid)
    assert (a["n"], a["N"], a["d"]) == (70000, 70001, 16) and a["bootstrap"]
    assert a["n"] > 65536
    assert set(np.unique(X)) == {0.0, 1.0}
    f = cpu_large(cid)
    assert f.node_count.max() > 32767
    # some split has its boundary past position 65535: the leaves' sizes in
    # pre-order are the segment lengths from position 0 upward
    for t in range(a["T"]):
        sizes = f.num_instances[t][_leaves(f)[t]]
        ends = np.cumsum(sizes)
        assert ((ends > 65535) & (ends < a["n"])).any()
    if cid == "L3-ext":
        assert a["extension_level"] == 1 and f.nnz == 2


def test_l4_seed_and_offset_matter():
    case = large_case("L4")
    X, bag, fs, seed, a = case
    assert seed >> 32 != 0 and a["tree_id_offset"] == BIG_OFFSET == 100000
    np.testing.assert_array_equal(X, large_case("L1")[0])
    f = cpu_large("L4")
    assert not same_forest(f, build_standard(case, seed=seed & 0xFFFFFFFF),
                           FIELDS)
    assert not same_forest(f, build_standard(case, tree_id_offset=0), FIELDS)


@pytest.mark.parametrize("cid", ["X1-full", "X1-nnz2k3"])
def test_extended_l1_has_empty_sides(cid):
    X, bag, fs, seed, a = large_case(cid)
    f = cpu_large(cid)
    assert a["n"] == 16385
    if cid == "X1-full":
        assert a["k"] == 4 == a["d"] and f.nnz == 4
    else:
        assert a["k"] == 3 < a["d"] == 4 and f.nnz == 2
        inner = _internal(f)
        for t in range(a["T"]):
            assert np.isin(f.hyper_idx[t][inner[t]], fs[t]).all()
    assert (_leaves(f) & (f.num_instances == 0)).any()
    assert (np.diff(f.hyper_idx[_internal(f)], axis=1) > 0).all()
