"""The case table of the GPU build-parity tests, checked without a GPU.

tests/test_build_shapes_gpu.py builds every case below with
build_forest_kernel / build_extended_forest_kernel and compares the result
bitwise with the CPU oracle. A case is only worth its GPU time while it
still reaches the code it was chosen for: a bag with duplicated rows, a
retry loop that runs dry, a Fisher-Yates target past lane 63, a Philox key
with a non-zero high word. Those are properties of the oracle's forest, so
they are asserted here, on the oracle alone: a case that stops exercising
its mechanism (a changed sampler, another seed) fails in this file instead
of passing silently on the GPU.

Cases are addressed by id. standard_case(id) / extended_case(id) return
``(X, bag, fs, seed, args)``; cpu_standard(id) / cpu_extended(id) the
oracle's forest for it. Everything is computed once and handed out
read-only.
"""

import functools
import math

import numpy as np
import pytest

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.core.forest import Forest
from isolation_forest_amd.ops.gpu_engine import _node_depths
from isolation_forest_amd.utils.det_math import bf16_round

# 64-bit seeds: the Philox key word k1 = seed >> 32 is 1, 256 and 2^31 - 1
SEEDS64 = {"2p32": 1 << 32, "2p40p3": (1 << 40) + 3, "2p63m1": (1 << 63) - 1}
S1_N = [2, 3, 63, 64, 65, 100, 257, 1000]
E1_N = [2, 3, 65, 100, 257]
E1_LEVELS = [0, 2, 5]
BIG_OFFSET = 100000


def _normal(N, d, seed):
    return np.random.RandomState(seed).normal(size=(N, d)).astype(np.float32)


def _constant_columns():
    """S4: d = 8 with columns 1..6 held at 3.0; only 0 and 7 can split."""
    X = _normal(600, 8, 104)
    X[:, 1:7] = np.float32(3.0)
    return X


def round_rows16(X, kind):
    """f32 rows rounded (RNE) to bf16 or fp16 and widened back exactly: what
    a 16-bit device matrix holds, as the oracle has to see it."""
    if kind == "bf16":
        return bf16_round(X).astype(np.float32)
    assert kind == "f16"
    return X.astype(np.float16).astype(np.float32)


def _case(X, n, T, seed, k=None, bootstrap=False, level=None, offset=0):
    N, d = X.shape
    k = d if k is None else k
    bag = cpu_engine.sample_bags(N, T, n, seed=seed, bootstrap=bootstrap,
                                 tree_id_offset=offset)
    fs = cpu_engine.feature_subsets(d, k, T, seed=seed, tree_id_offset=offset)
    args = {"n": n, "d": d, "k": k, "T": T, "N": N, "bootstrap": bootstrap,
            "tree_id_offset": offset, "extension_level": level}
    for a in (X, bag, fs):
        a.setflags(write=False)
    return X, bag, fs, seed, args


def _standard_table():
    tab = {}
    for n in S1_N:
        tab[f"S1-n{n}"] = lambda n=n: _case(_normal(3000, 5, 101), n, 4, 11)
    for n in (16383, 16384):
        tab[f"S2-n{n}"] = lambda n=n: _case(_normal(20000, 4, 102), n, 2, 12)
    tab["S3"] = lambda: _case(_normal(400, 5, 103), 257, 4, 13,
                              bootstrap=True)
    tab["S4a"] = lambda: _case(_constant_columns(), 65, 4, 14, k=8)
    tab["S4b"] = lambda: _case(_constant_columns(), 65, 4, 14, k=3)
    for k in (100, 130):
        tab[f"S5-k{k}"] = lambda k=k: _case(_normal(600, 130, 105), 100, 3,
                                            15, k=k)
    for name, seed in SEEDS64.items():
        tab[f"S6-{name}"] = lambda seed=seed: _case(_normal(3000, 4, 106),
                                                    64, 2, seed)
    tab["S7"] = lambda: _case(_normal(400, 5, 107), 65, 7, 17, bootstrap=True)
    tab["S7-offset"] = lambda: _case(_normal(400, 5, 107), 65, 3, 17,
                                     bootstrap=True, offset=BIG_OFFSET)
    tab["S8"] = lambda: _case(_normal(3000, 3, 108), 16, 300, 18)
    for kind in ("bf16", "f16"):
        tab[f"S9-n65-{kind}"] = lambda kind=kind: _case(
            round_rows16(_normal(3000, 5, 101), kind), 65, 4, 11)
        tab[f"S9-boot-{kind}"] = lambda kind=kind: _case(
            round_rows16(_normal(400, 5, 103), kind), 257, 4, 13,
            bootstrap=True)
    return tab


def _extended_table():
    tab = {}
    for n in E1_N:
        for lv in E1_LEVELS:
            tab[f"E1-n{n}-L{lv}"] = lambda n=n, lv=lv: _case(
                _normal(3000, 6, 201), n, 4, 21, level=lv)
    for n in (16383, 16384):
        tab[f"E2-n{n}"] = lambda n=n: _case(_normal(20000, 4, 202), n, 2, 22,
                                            level=1)
    for lv in (64, 129):
        tab[f"E3-L{lv}"] = lambda lv=lv: _case(_normal(600, 130, 203), 100, 3,
                                               23, level=lv)
    tab["E4"] = lambda: _case(_normal(400, 6, 204), 257, 4, 24,
                              bootstrap=True, level=5)
    tab["E5"] = lambda: _case(_normal(3000, 8, 205), 100, 4, 25, k=5, level=7)
    for name, seed in SEEDS64.items():
        tab[f"E6-{name}"] = lambda seed=seed: _case(_normal(3000, 6, 206),
                                                    64, 2, seed, level=2)
    tab["E6-shards"] = lambda: _case(_normal(400, 6, 207), 65, 7, 27,
                                     bootstrap=True, level=2)
    tab["E6-offset"] = lambda: _case(_normal(400, 6, 207), 65, 3, 27,
                                     bootstrap=True, level=2,
                                     offset=BIG_OFFSET)
    return tab


_STANDARD = _standard_table()
_EXTENDED = _extended_table()
STANDARD_IDS = list(_STANDARD)
EXTENDED_IDS = list(_EXTENDED)
# cases whose GPU forest is also packed on the device and scored
CHAIN_STANDARD_IDS = ["S1-n65", "S4b", "S5-k130"]
CHAIN_EXTENDED_IDS = ["E1-n65-L5"]
# (whole case, [(first tree, end tree)]): tree shards of a multi-rank fit
SHARDS = [(0, 3), (3, 7)]


@functools.lru_cache(maxsize=None)
def standard_case(cid):
    return _STANDARD[cid]()


@functools.lru_cache(maxsize=None)
def extended_case(cid):
    return _EXTENDED[cid]()


def shard_of(case, lo, hi):
    """Trees [lo, hi) of a case as a rank of a tree-sharded fit holds them:
    its rows of the bags and subsets, and tree_id_offset = lo."""
    X, bag, fs, seed, args = case
    assert args["tree_id_offset"] == 0
    args = dict(args, T=hi - lo, tree_id_offset=lo)
    return X, bag[lo:hi], fs[lo:hi], seed, args


def build_standard(case, seed=None, tree_id_offset=None):
    X, bag, fs, case_seed, a = case
    return cpu_engine.build_forest(
        X, bag, fs, case_seed if seed is None else seed, a["n"], a["k"],
        a["d"],
        tree_id_offset=(a["tree_id_offset"] if tree_id_offset is None
                        else tree_id_offset))


def build_extended(case, seed=None, tree_id_offset=None):
    X, bag, fs, case_seed, a = case
    return cpu_engine.build_extended_forest(
        X, bag, fs, case_seed if seed is None else seed, a["n"], a["k"],
        a["d"], a["extension_level"],
        tree_id_offset=(a["tree_id_offset"] if tree_id_offset is None
                        else tree_id_offset))


@functools.lru_cache(maxsize=None)
def cpu_standard(cid):
    return build_standard(standard_case(cid))


@functools.lru_cache(maxsize=None)
def cpu_extended(cid):
    return build_extended(extended_case(cid))


FIELDS = ["node_count", "feature", "right", "num_instances", "value"]
EXT_FIELDS = FIELDS + ["hyper_idx", "hyper_w", "offset64"]


def field_bits(a):
    """Arrays as integers, so float fields compare bit for bit."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.int32)
    if a.dtype == np.float64:
        return a.view(np.int64)
    return a


def same_forest(f, g, fields):
    return all(np.array_equal(field_bits(getattr(f, name)),
                              field_bits(getattr(g, name)))
               for name in fields)


def tree_slice(forest, lo, hi, fields):
    return {name: getattr(forest, name)[lo:hi] for name in fields}


def height_limit(n):
    return int(math.ceil(math.log2(max(n, 2))))


def _live(forest):
    cols = np.arange(forest.feature.shape[1])[None, :]
    return cols < forest.node_count[:, None]


def _leaves(forest):
    return _live(forest) & (forest.feature == Forest.LEAF)


def _internal(forest):
    return _live(forest) & (forest.feature >= 0)


def _fields_of(cid):
    return FIELDS if cid in _STANDARD else EXT_FIELDS


def _any_case(cid):
    return standard_case(cid) if cid in _STANDARD else extended_case(cid)


def _any_forest(cid):
    return cpu_standard(cid) if cid in _STANDARD else cpu_extended(cid)


# ---------------------------------------------------------------------------
# every case: the shapes the table states, and a well-formed oracle forest
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("cid", STANDARD_IDS + EXTENDED_IDS)
def test_case_is_well_formed(cid):
    X, bag, fs, seed, a = _any_case(cid)
    forest = _any_forest(cid)
    n, T = a["n"], a["T"]
    assert X.dtype == np.float32 and X.shape == (a["N"], a["d"])
    assert bag.shape == (T, n) and bag.min() >= 0 and bag.max() < a["N"]
    assert fs.shape == (T, a["k"])
    assert (np.diff(fs, axis=1) > 0).all()  # sorted, distinct
    assert 2 <= n <= 16384 and 2 <= T <= 7 or cid == "S8"
    H = height_limit(n)
    if cid in _STANDARD:
        assert forest.feature.shape == (T, 2 * n - 1)
    else:
        nnz = min(a["extension_level"] + 1, a["k"])
        assert forest.feature.shape == (T, 2 ** (H + 1) - 1)
        assert forest.hyper_idx.shape == (T, 2 ** (H + 1) - 1, nnz)
    assert forest.feature.shape[1] <= 32767  # int16 patch ids
    assert (forest.node_count >= 1).all()
    assert (forest.feature[~_live(forest)] == Forest.PAD).all()
    depth = _node_depths(forest.feature, forest.right)
    assert depth[_live(forest)].max() <= H
    # every bag row lands in exactly one leaf
    counts = np.where(_leaves(forest), forest.num_instances, 0)
    np.testing.assert_array_equal(counts.sum(axis=1), np.full(T, n))


def test_s1_height_limits_and_wave_remainders():
    assert [height_limit(n) for n in (2, 3)] == [1, 2]
    assert sorted(n % 64 for n in S1_N) == sorted(
        [2, 3, 63, 0, 1, 36, 1, 40])
    assert {n % 2 for n in S1_N} == {0, 1} == {n % 2 for n in E1_N}
    # nnz of both parities against odd n (coords/wf/stack alignment)
    assert {min(lv + 1, 6) % 2 for lv in E1_LEVELS} == {0, 1}
    for n in S1_N:
        f = cpu_standard(f"S1-n{n}")
        depth = _node_depths(f.feature, f.right)
        # the tree fills its height: the limit itself is reached for small n
        if n <= 3:
            assert depth[_live(f)].max() == height_limit(n)


def test_s2_e2_sit_on_the_cap():
    assert cpu_standard("S2-n16384").feature.shape[1] == 32767
    assert cpu_standard("S2-n16383").feature.shape[1] == 32765
    assert cpu_extended("E2-n16384").feature.shape[1] == 32767
    assert cpu_extended("E2-n16383").feature.shape[1] == 32767
    # the root segment ends at 16384 and the trees run into the height limit
    # (uniform cuts of Gaussian columns are lopsided: a few thousand nodes,
    # most rows left in leaves at depth 14)
    for f, bag in ((cpu_standard("S2-n16384"), standard_case("S2-n16384")[1]),
                   (cpu_extended("E2-n16384"), extended_case("E2-n16384")[1])):
        assert bag.shape == (2, 16384)
        depth = _node_depths(f.feature, f.right)
        at_limit = _leaves(f) & (depth == 14)
        assert (at_limit & (f.num_instances > 1)).any()
        assert (f.node_count > 1024).all()


@pytest.mark.parametrize("cid", ["S3", "E4", "S7", "E6-shards",
                                 "S9-boot-bf16", "S9-boot-f16"])
def test_bootstrap_bags_repeat_rows(cid):
    _, bag, _, _, a = _any_case(cid)
    assert a["bootstrap"]
    for row in bag:
        assert len(np.unique(row)) < len(row)


@pytest.mark.parametrize("cid", ["S3", "S9-boot-bf16", "S9-boot-f16"])
def test_s3_duplicates_end_in_leaves_above_the_height_limit(cid):
    f = cpu_standard(cid)
    depth = _node_depths(f.feature, f.right)
    H = height_limit(257)
    early = _leaves(f) & (f.num_instances > 1) & (depth < H)
    assert early.any()


def test_e4_has_empty_sides():
    f = cpu_extended("E4")
    assert (_leaves(f) & (f.num_instances == 0)).any()
    # and the duplicates survive to leaves of several rows
    assert (_leaves(f) & (f.num_instances > 1)).any()


def test_s4a_retry_finds_the_two_live_columns():
    X, _, fs, _, a = standard_case("S4a")
    assert a["k"] == 8 and (X[:, 1:7] == 3.0).all()
    f = cpu_standard("S4a")
    assert set(np.unique(f.feature[_internal(f)])) == {0, 7}
    # six of eight candidates are constant: some node must have drawn one
    # first (the chance that none of >= 64 nodes did is (1/4)^64)
    assert _internal(f).sum() >= 64


def test_s4b_retry_runs_dry():
    X, _, fs, _, a = standard_case("S4b")
    assert a["k"] == 3
    f = cpu_standard("S4b")
    depth = _node_depths(f.feature, f.right)
    dry = _leaves(f) & (f.num_instances > 1) & (depth < height_limit(65))
    assert dry.any()
    # a subset of constant columns only: the root itself is such a leaf
    constant_only = [t for t in range(a["T"])
                     if not ({0, 7} & set(fs[t].tolist()))]
    assert constant_only
    for t in constant_only:
        assert f.node_count[t] == 1 and f.num_instances[t, 0] == 65
    # and a tree that does split, so both outcomes are in one forest
    assert (f.node_count > 1).any()
    assert set(np.unique(f.feature[_internal(f)])) <= {0, 7}


@pytest.mark.parametrize("k", [100, 130])
def test_s5_splits_past_lane_63(k):
    _, _, fs, _, a = standard_case(f"S5-k{k}")
    assert a["k"] == k and a["d"] == 130
    f = cpu_standard(f"S5-k{k}")
    hit = 0
    for t in range(a["T"]):
        feats = f.feature[t][_internal(f)[t]]
        pos = np.searchsorted(fs[t], feats)
        assert (fs[t][pos] == feats).all()
        hit += int((pos >= 64).sum())
    assert hit > 0


@pytest.mark.parametrize("lv", [64, 129])
def test_e3_wide_hyperplanes(lv):
    f = cpu_extended(f"E3-L{lv}")
    nnz = lv + 1
    assert f.nnz == nnz and nnz > 64
    inner = _internal(f)
    assert inner.sum() >= 3
    assert (f.feature[inner] == nnz).all()
    assert (f.hyper_w[inner][:, 64:] != 0).any()
    assert (f.hyper_w[inner][:, 64:] != 0).all(axis=1).any()
    assert (np.diff(f.hyper_idx[inner], axis=1) > 0).all()
    # nodes >= 1 draw Philox counters node * 4096 + j with j >= 64
    assert np.nonzero(inner)[1].max() >= 1


def test_e5_subspace_clamps_nnz():
    _, _, fs, _, a = extended_case("E5")
    f = cpu_extended("E5")
    assert a["k"] == 5 < a["d"] == 8 and f.nnz == 5
    inner = _internal(f)
    for t in range(a["T"]):
        # every hyperplane is the whole subspace of its tree
        assert (f.hyper_idx[t][inner[t]] == fs[t][None, :]).all()
    assert len({tuple(r) for r in fs.tolist()}) > 1


@pytest.mark.parametrize("cid", [f"S6-{s}" for s in SEEDS64]
                         + [f"E6-{s}" for s in SEEDS64])
def test_high_seed_word_matters(cid):
    case = _any_case(cid)
    seed = case[3]
    assert seed >> 32 != 0 and 0 <= seed < 1 << 63
    build = build_standard if cid in _STANDARD else build_extended
    low_only = build(case, seed=seed & 0xFFFFFFFF)
    assert not same_forest(_any_forest(cid), low_only, _fields_of(cid))
    # and the low word: a kernel that keyed on seed >> 32 alone
    high_only = build(case, seed=seed & ~0xFFFFFFFF)
    if seed & 0xFFFFFFFF:
        assert not same_forest(_any_forest(cid), high_only, _fields_of(cid))


@pytest.mark.parametrize("cid", ["S7", "E6-shards"])
def test_shards_with_offsets_make_the_whole_forest(cid):
    case = _any_case(cid)
    whole = _any_forest(cid)
    fields = _fields_of(cid)
    build = build_standard if cid in _STANDARD else build_extended
    X, bag, fs, seed, a = case
    for lo, hi in SHARDS:
        sh = shard_of(case, lo, hi)
        # a rank draws exactly these bags and subsets for its trees
        np.testing.assert_array_equal(
            cpu_engine.sample_bags(a["N"], hi - lo, a["n"], seed=seed,
                                   bootstrap=True, tree_id_offset=lo), sh[1])
        np.testing.assert_array_equal(
            cpu_engine.feature_subsets(a["d"], a["k"], hi - lo, seed,
                                       tree_id_offset=lo), sh[2])
        part = build(sh)
        for name, want in tree_slice(whole, lo, hi, fields).items():
            np.testing.assert_array_equal(
                field_bits(getattr(part, name)), field_bits(want),
                err_msg=f"{cid} trees [{lo}, {hi}) {name}")
        if lo:
            wrong = build(sh, tree_id_offset=0)
            assert not all(
                np.array_equal(field_bits(getattr(wrong, name)),
                               field_bits(want))
                for name, want in tree_slice(whole, lo, hi, fields).items())


@pytest.mark.parametrize("cid", ["S7-offset", "E6-offset"])
def test_large_offset_matters(cid):
    case = _any_case(cid)
    assert case[4]["tree_id_offset"] == BIG_OFFSET
    build = build_standard if cid in _STANDARD else build_extended
    assert not same_forest(_any_forest(cid), build(case, tree_id_offset=0),
                           _fields_of(cid))


def test_s8_has_more_trees_than_compute_units():
    a = standard_case("S8")[4]
    assert a["T"] == 300 > 256  # an MI355X has 256 CUs
    f = cpu_standard("S8")
    assert len({f.feature[t].tobytes() + f.value[t].tobytes()
                for t in range(300)}) == 300


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_s9_rows_are_16_bit_and_change_the_forest(kind):
    for cid, f32_cid in ((f"S9-n65-{kind}", "S1-n65"),
                         (f"S9-boot-{kind}", "S3")):
        X = standard_case(cid)[0]
        X32 = standard_case(f32_cid)[0]
        np.testing.assert_array_equal(round_rows16(X, kind), X)
        assert (X != X32).any()
        np.testing.assert_array_equal(standard_case(cid)[1],
                                      standard_case(f32_cid)[1])
        assert not same_forest(cpu_standard(cid), cpu_standard(f32_cid),
                               FIELDS)


def test_chain_cases_have_odd_max_nodes_and_padding():
    """The device packers must mask the raw outputs past node_count; that
    only shows where such columns exist."""
    for cid in CHAIN_STANDARD_IDS + CHAIN_EXTENDED_IDS:
        f = _any_forest(cid)
        assert f.feature.shape[1] % 2 == 1
        assert (~_live(f)).any(), cid
