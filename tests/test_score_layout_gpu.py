"""GPU tests (MI355X) for the LDS layout of the standard scoring walk
(score_forest_v4): the feature-major key tile and the level-order node
records (v4_level_order).

The tile pairs two rows of a block in one 32-bit word for 16-bit keys (rows
tid and tid+256 under RPT=2, rows tid and tid+128 under RPT=1), so the
seams of that pairing — rows 127/128 and 255/256 — together with row 0 and
the last row carry the float edge cells (+-0, +-inf, NaN, the smallest
subnormal, the largest finite value): a swapped half or a wrong slab shows
there. Row counts cover one block or less, a tail block and the second
grid-stride tile of one block; feature counts cover every (RPT, ILP,
ROWS_LDS) instantiation the binding's selector can pick.

Oracle: the strict-order CPU engine, bitwise on path sums and scores, as in
the standard-scoring parity tests of tests/test_gpu.py.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.ops import gpu_engine  # noqa: E402
from tests.test_gpu_edges import (  # noqa: E402
    MAX_BLOCKS,
    Shell,
    _assert_bitwise,
    _routed,
)

KINDS = ["bf16", "f16", "f32"]
SEAMS = (0, 127, 128, 255, 256)  # plus the last row


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


# ---------------------------------------------------------------------------
# data: values exact in the row dtype, kept as their f32 widening
# ---------------------------------------------------------------------------


def _round(X, kind):
    if kind == "bf16":
        return torch.from_numpy(X).to(torch.bfloat16).float().numpy()
    if kind == "f16":
        with np.errstate(over="ignore"):
            return X.astype(np.float16).astype(np.float32)
    return X


def _edge_values(kind, nan=True):
    """+-0, +-inf, NaN, +-smallest subnormal, +-largest finite."""
    if kind == "bf16":
        sub, big = (np.array([0x00010000, 0x7F7F0000], dtype=np.uint32)
                    .view(np.float32))
    elif kind == "f16":
        sub, big = np.float32(2.0 ** -24), np.float32(65504.0)
    else:
        sub, big = (np.array([0x00000001, 0x7F7FFFFF], dtype=np.uint32)
                    .view(np.float32))
    v = [0.0, -0.0, np.inf, -np.inf, sub, -sub, big, -big]
    if nan:
        v.append(np.nan)
    v = np.array(v, dtype=np.float32)
    w = _round(v, kind)  # exact in the row dtype (a NaN stays some NaN)
    ok = ~np.isnan(v)
    assert np.array_equal(w[ok].view(np.int32), v[ok].view(np.int32))
    assert np.isnan(w[~ok]).all()
    return v


def _rows(N, d, kind, seed, nan=True):
    """Gaussian rows with every cell of the seam rows an edge value."""
    def make():
        rs = np.random.RandomState(seed)
        X = _round(rs.standard_normal((N, d)).astype(np.float32), kind)
        vals = _edge_values(kind, nan)
        for k, r in enumerate(sorted({r for r in SEAMS if r < N} | {N - 1})):
            X[r] = vals[(np.arange(d) + k) % len(vals)]
        X.setflags(write=False)
        return X
    return _memo(("rows", N, d, kind, seed, nan), make)


def _to_dev(X, kind, dev):
    t = torch.from_numpy(np.array(X))
    if kind == "bf16":
        t = t.to(torch.bfloat16)  # exact: X is already rounded
    elif kind == "f16":
        t = t.to(torch.float16)
    return t.to(dev)


def _forest(d, n, T, kind, constant=False, ext=None, seed=17):
    def make():
        rows = max(1000, n + 100)
        if constant:
            X = np.full((rows, d), 1.5, dtype=np.float32)
        else:
            X = _round(np.random.RandomState(1000 + d)
                       .standard_normal((rows, d)).astype(np.float32), kind)
        bag = cpu_engine.sample_bags(rows, T, n, seed=seed, bootstrap=False)
        fs = cpu_engine.feature_subsets(d, d, T, seed=seed)
        if ext is not None:
            return cpu_engine.build_extended_forest(X, bag, fs, seed, n, d, d,
                                                    ext)
        return cpu_engine.build_forest(X, bag, fs, seed, n, d, d)
    return _memo(("forest", d, n, T, kind, constant, ext, seed), make)


def _oracle(forest, X):
    def make():
        with np.errstate(all="ignore"):
            if hasattr(forest, "hyper_w"):
                ps = cpu_engine.path_lengths_extended(forest, X)
            else:
                ps = cpu_engine.path_lengths(forest, X)
        return forest, X, ps  # keeps both alive, so the ids stay unique
    return _memo(("oracle", id(forest), id(X)), make)[2]


# ---------------------------------------------------------------------------
# the instantiation the score_forest binding picks (mirror of its selector:
# tile = (d + 1) slabs of rpt*256 keys, no padding)
# ---------------------------------------------------------------------------


def _route(d, mn, kind):
    elem = 4 if kind == "f32" else 2
    slabs = d + 1
    nodes_lds = 2 * mn * 8 + 256 * slabs * elem <= 150 * 1024
    best = None
    for rpt, ilp in ((2, 4), (1, 4), (2, 2), (1, 2)):
        lds = (ilp * mn * 8 if nodes_lds else 0) + rpt * 256 * slabs * elem
        if lds > 150 * 1024:
            continue
        cand = (min(160 * 1024 // lds, 3), rpt * ilp)
        if best is None or cand > best[0]:
            best = (cand, rpt, ilp)
    if best is None:
        return {"rpt": 1, "ilp": 4, "rows_lds": False, "nodes_lds": nodes_lds}
    return {"rpt": best[1], "ilp": best[2], "rows_lds": True,
            "nodes_lds": nodes_lds}


def _check(dev, forest, X, kind, what):
    got = gpu_engine.score_forest(Shell(forest), _to_dev(X, kind, dev),
                                  finalize=False)
    _assert_bitwise(got.cpu().numpy(), _oracle(forest, X), what)


# ---------------------------------------------------------------------------
# row counts
# ---------------------------------------------------------------------------


class TestRowCounts:
    @pytest.mark.parametrize("kind", KINDS)
    @pytest.mark.parametrize("N", [1, 255, 256, 257, 511, 513, 1000])
    def test_small(self, dev, N, kind):
        d = 5
        forest = _forest(d, 64, 9, kind)
        cfg = _route(d, forest.feature.shape[1], kind)
        assert cfg == {"rpt": 2, "ilp": 4, "rows_lds": True,
                       "nodes_lds": True}
        _check(dev, forest, _rows(N, d, kind, 2000 + N), kind,
               f"{kind} N={N}")

    def test_second_tile_of_a_block(self, dev):
        """More than 8192 blocks of 512 rows: block 0 re-stages a second
        tile in its grid-stride loop, and that tile is a tail."""
        d, kind = 2, "bf16"
        forest = _forest(d, 8, 8, kind)
        assert _route(d, forest.feature.shape[1], kind)["rpt"] == 2
        N = MAX_BLOCKS * 512 + 513
        _check(dev, forest, _rows(N, d, kind, 77), kind, "second tile")


# ---------------------------------------------------------------------------
# feature counts and routes
# ---------------------------------------------------------------------------

# (rpt, ilp, rows_lds) at max_nodes = 511, by the selector's arithmetic:
# 16-bit keys hold 3 blocks/CU at (2, 4) up to d = 36; d = 37 and 64 drop to
# RPT=1, d = 128 needs ILP=2 for a second block, d = 300 exceeds LDS alone.
# f32 keys reach the same switches at about half the width.
_EXPECT = {
    2: {1: (2, 4, True), 2: (2, 4, True), 31: (2, 4, True),
        32: (2, 4, True), 33: (2, 4, True), 37: (1, 4, True),
        64: (1, 4, True), 128: (1, 2, True), 300: (1, 4, False)},
    4: {1: (2, 4, True), 2: (2, 4, True), 31: (1, 4, True),
        32: (1, 4, True), 33: (1, 4, True), 37: (1, 2, True),
        64: (1, 2, True), 128: (1, 4, True), 300: (1, 4, False)},
}


class TestFeatureCounts:
    @pytest.mark.parametrize("kind", KINDS)
    @pytest.mark.parametrize("d", [1, 2, 31, 32, 33, 37, 64, 128, 300])
    def test_bitwise(self, dev, d, kind):
        forest = _forest(d, 256, 8, kind)
        assert forest.feature.shape[1] == 511
        cfg = _route(d, 511, kind)
        assert (cfg["rpt"], cfg["ilp"], cfg["rows_lds"]) == \
            _EXPECT[4 if kind == "f32" else 2][d]
        _check(dev, forest, _rows(1000, d, kind, 3000 + d), kind,
               f"{kind} d={d} {cfg}")

    def test_unaligned_rows(self, dev):
        """A view whose rows start off 16-byte alignment is made contiguous
        by the engine; a contiguous d = 8 tensor at an odd element offset of
        its storage is not, and must take the element-wise staging."""
        d, kind = 8, "bf16"
        forest = _forest(d, 64, 8, kind)
        X = _rows(1000, d, kind, 91)
        flat = torch.empty(1000 * d + 1, dtype=torch.bfloat16, device=dev)
        Xt = flat[1:].view(1000, d)
        Xt.copy_(_to_dev(X, kind, dev))
        assert Xt.is_contiguous() and Xt.data_ptr() % 16 != 0
        got = gpu_engine.score_forest(Shell(forest), Xt, finalize=False)
        _assert_bitwise(got.cpu().numpy(), _oracle(forest, X), "unaligned X")


# ---------------------------------------------------------------------------
# forests
# ---------------------------------------------------------------------------


class TestForests:
    @pytest.mark.parametrize("kind", ["bf16", "f32"])
    @pytest.mark.parametrize("T", [1, 7, 8, 9])
    def test_tree_counts(self, dev, T, kind):
        d = 5
        _check(dev, _forest(d, 64, T, kind), _rows(1000, d, kind, 41), kind,
               f"{kind} T={T}")

    @pytest.mark.parametrize("kind", ["bf16", "f32"])
    @pytest.mark.parametrize("n", [2, 3])
    def test_tiny_trees(self, dev, n, kind):
        d = 5
        forest = _forest(d, n, 9, kind)
        assert forest.feature.shape[1] == 2 * n - 1
        _check(dev, forest, _rows(1000, d, kind, 41), kind, f"{kind} n={n}")

    @pytest.mark.parametrize("kind", KINDS)
    def test_single_leaf_trees(self, dev, kind):
        d = 5
        forest = _forest(d, 64, 9, kind, constant=True)
        assert (np.asarray(forest.node_count) == 1).all()
        _check(dev, forest, _rows(1000, d, kind, 41), kind,
               f"{kind} constant data")

    @pytest.mark.parametrize("kind", KINDS)
    def test_flagship_shape_and_scores(self, dev, kind):
        """maxSamples = 256, d = 32, and the finalized score."""
        d = 32
        forest = _forest(d, 256, 8, kind)
        X = _rows(1000, d, kind, 3000 + d)
        got = gpu_engine.score_forest(Shell(forest), _to_dev(X, kind, dev),
                                      finalize=True)
        want = cpu_engine.scores_from_path_sums(
            _oracle(forest, X), forest.num_trees, forest.num_samples)
        _assert_bitwise(got.cpu().numpy(), want, f"{kind} scores")

    @pytest.mark.parametrize("kind,d,nodes_lds,ilp", [
        ("bf16", 5, True, 2),    # two 8191-node trees fit next to the tile
        ("f32", 32, False, 4),   # they do not: nodes walked from L2
    ])
    def test_deep_trees(self, dev, kind, d, nodes_lds, ilp):
        forest = _forest(d, 4096, 8, kind)
        cfg = _route(d, forest.feature.shape[1], kind)
        assert cfg["nodes_lds"] == nodes_lds and cfg["ilp"] == ilp
        assert cfg["rows_lds"]
        _check(dev, forest, _rows(1000, d, kind, 43), kind,
               f"{kind} n=4096 {cfg}")

    @pytest.mark.parametrize("kind", KINDS)
    def test_eif_extension_level_0(self, dev, kind):
        """The ext-0 mirrored pack rides the same v4 walk (NaN rows take
        another route, so none are planted)."""
        d = 5
        forest = _forest(d, 64, 9, kind, ext=0)
        X = _rows(1000, d, kind, 45, nan=False)
        out, _ = _routed(gpu_engine.score_extended_forest, Shell(forest),
                         _to_dev(X, kind, dev), "score_forest")
        _assert_bitwise(out.cpu().numpy(), _oracle(forest, X),
                        f"{kind} eif ext-0")


# ---------------------------------------------------------------------------
# level-order node records
# ---------------------------------------------------------------------------


def _fields(nodes):
    meta = nodes[..., 0]
    return meta & 0xFFF, (meta >> 12) & 0x7FFF, nodes[..., 1]


def _walk(tree, trips, keys, level_order):
    """Leaf reached from the root by every key row, with the walk's own step
    rule: pre-order `x < t ? cur + 1 : link`, level order `link - (x < t)`."""
    feat, link, w1 = _fields(tree)
    cur = np.zeros(len(keys), dtype=np.int64)
    rows = np.arange(len(keys))
    for _ in range(trips):
        lt = keys[rows, feat[cur]] < w1[cur].view(np.uint32)
        cur = link[cur] - lt if level_order else np.where(lt, cur + 1,
                                                          link[cur])
    return cur


class TestLevelOrder:
    @pytest.mark.parametrize("case", ["std", "tiny2", "tiny3", "single-leaf",
                                      "deep", "eif0"])
    def test_structure(self, dev, case):
        from isolation_forest_amd.ops import load_extension

        d, kind = 5, "f32"
        if case == "eif0":
            packed, ncount, trips = gpu_engine._eif0_packed_v4(
                _forest(d, 64, 9, kind, ext=0), d, kind)
        else:
            n = {"std": 64, "tiny2": 2, "tiny3": 3, "single-leaf": 64,
                 "deep": 1024}[case]
            packed, ncount, trips = gpu_engine._nodes_packed_v4(
                _forest(d, n, 9, kind, constant=case == "single-leaf"), d,
                kind)
        assert packed.shape[0] == 16  # 9 trees + 7 padding trees
        out = load_extension().v4_level_order(
            torch.from_numpy(packed).to(dev),
            torch.from_numpy(ncount).to(dev)).cpu().numpy()
        assert out.shape == packed.shape and out.dtype == packed.dtype

        rs = np.random.RandomState(5)
        keys = rs.randint(0, 2 ** 32, size=(300, d + 1), dtype=np.uint64) \
            .astype(np.uint32)
        keys[:, d] = 0xFFFFFFFF  # the leaf sentinel column
        for t in range(packed.shape[0]):
            n = int(ncount[t])
            pre, lvl = packed[t], out[t]
            # dead tail (and with it a padding tree's) preserved
            np.testing.assert_array_equal(lvl[n:], pre[n:])
            if t >= 9:
                assert n == 1
            feat, link, w1 = _fields(lvl[:n])
            leaf = feat == d
            idx = np.arange(n)
            # leaves self-loop; internal links point past the root
            np.testing.assert_array_equal(link[leaf], idx[leaf])
            assert ((link[~leaf] >= 2) & (link[~leaf] <= n - 1)).all()
            # every node but the root is the child of exactly one node, the
            # two children of a node adjacent (left = link - 1)
            kids = np.sort(np.concatenate([link[~leaf] - 1, link[~leaf]]))
            np.testing.assert_array_equal(kids, idx[1:])
            # depth never falls along the new index
            depth = np.zeros(n, dtype=np.int64)
            for i in idx[~leaf]:
                assert link[i] > i + 1 or i == 0
                depth[link[i] - 1] = depth[link[i]] = depth[i] + 1
            assert (np.diff(depth) >= 0).all()
            assert depth.max(initial=0) <= trips
            # the same records apart from the link field
            pf, _, pw = _fields(pre[:n])
            np.testing.assert_array_equal(
                np.sort(feat.astype(np.int64) << 32 | w1.view(np.uint32)),
                np.sort(pf.astype(np.int64) << 32 | pw.view(np.uint32)))
            # both walks end on the same leaf payload
            a = _walk(pre, trips, keys, False)
            b = _walk(lvl, trips, keys, True)
            assert (pre[a, 0] & 0xFFF == d).all()
            np.testing.assert_array_equal(lvl[b], _relinked(pre[a], b))


def _relinked(recs, new_index):
    """Leaf records with the link field set to the given indices."""
    r = recs.copy()
    r[:, 0] = (r[:, 0] & 0xFFF) | (new_index.astype(np.int32) << 12)
    return r
