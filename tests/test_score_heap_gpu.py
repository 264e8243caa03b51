"""GPU tests (MI355X) for the heap node records of the 16-bit standard
scoring walk: v4_heap_order (the converter) and score_forest_heap (the walk),
reached through gpu_engine.score_forest / score_extended_forest.

A heap record is 4 bytes (16-bit key threshold | byte offset of the
feature's slab in the key tile), children are implicit (2c, 2c+1), leaves
above the height limit pass through the sentinel slab to level H. What can
go wrong is the converter's placement, the 16-bit compare (equality goes
right, NaN goes right), the slab offset bound, the fixed-size tree stage and
the route choice, so: every case first asserts the route the extension's
score_route reports, scores are compared bitwise with the strict-order CPU
engine, and the converter's output is compared word for word with the numpy
reference of tests/test_score_heap_ref.py.
"""

import os

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
from tests.test_score_heap_ref import (  # noqa: E402
    heap_reference,
    round_rows,
    row_keys,
    split_rows,
)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def _ext():
    from isolation_forest_amd.ops import load_extension

    return load_extension()


_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _forest(d, n, T, kind, constant=False, ext=None, seed=17):
    def make():
        rows = max(1000, n + 100)
        if constant == "all":
            X = np.full((rows, d), 1.5, dtype=np.float32)
        else:
            X = round_rows(np.random.RandomState(1000 + d)
                           .standard_normal((rows, d)).astype(np.float32),
                           "f16" if kind == "f16" else "bf16")
            if constant == "column":
                X[:, 0] = 2.5
        bag = cpu_engine.sample_bags(rows, T, n, seed=seed, bootstrap=False)
        fs = cpu_engine.feature_subsets(d, d, T, seed=seed)
        if ext is not None:
            return cpu_engine.build_extended_forest(X, bag, fs, seed, n, d, d,
                                                    ext)
        return cpu_engine.build_forest(X, bag, fs, seed, n, d, d)
    return _memo(("forest", d, n, T, kind, constant, ext, seed), make)


def _rows(N, d, kind, seed):
    def make():
        X = np.random.RandomState(seed).standard_normal((N, d)) \
            .astype(np.float32)
        X = X if kind == "f32" else round_rows(X, kind)
        X.setflags(write=False)
        return X
    return _memo(("rows", N, d, kind, seed), make)


def _oracle(forest, X):
    def make():
        with np.errstate(all="ignore"):
            if hasattr(forest, "hyper_w"):
                ps = cpu_engine.path_lengths_extended(forest, X)
            else:
                ps = cpu_engine.path_lengths(forest, X)
        return forest, X, ps  # keeps both alive, so the ids stay unique
    return _memo(("oracle", id(forest), id(X)), make)[2]


def _to_dev(X, kind, dev):
    t = torch.from_numpy(np.array(X))
    if kind == "bf16":
        t = t.to(torch.bfloat16)  # exact: X is already rounded
    elif kind == "f16":
        t = t.to(torch.float16)
    return t.to(dev)


def _height(forest):
    """The pack's max_depth (>= 1), which the engine passes as the height."""
    return _memo(("height", id(forest)), lambda: gpu_engine._nodes_packed_v4(
        forest, forest.feature.max(initial=0) + 1, "bf16")[2])


def _route(forest, d, kind, layout="packed", height=None):
    h = _height(forest) if height is None else height
    return _ext().score_route(kind, d, forest.feature.shape[1], h, layout)


def _check(dev, forest, X, kind, what, route="heap"):
    """Assert the route, score, compare bitwise; also that the pack holds
    heap records exactly when the route is the heap."""
    d = X.shape[1]
    assert _route(forest, d, kind) == route, what
    shell = Shell(forest)
    got = gpu_engine.score_forest(shell, _to_dev(X, kind, dev),
                                  finalize=False)
    (_, _, extra), = shell._gpu_forest_cache.values()
    assert (extra["heap"] is not None) == (route == "heap"), what
    _assert_bitwise(got.cpu().numpy(), _oracle(forest, X), what)


# ---------------------------------------------------------------------------
# row counts
# ---------------------------------------------------------------------------


class TestRowCounts:
    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    @pytest.mark.parametrize("N", [1, 255, 256, 257, 511, 513, 1000])
    def test_small(self, dev, N, kind):
        d = 5
        _check(dev, _forest(d, 64, 9, kind), _rows(N, d, kind, 2000 + N),
               kind, f"{kind} N={N}")

    def test_second_tile_of_a_block(self, dev):
        """More than 8192 blocks of 512 rows: block 0 stages a second tile
        in its grid-stride loop, and that tile is a tail."""
        d, kind = 2, "bf16"
        N = MAX_BLOCKS * 512 + 513
        _check(dev, _forest(d, 8, 8, kind), _rows(N, d, kind, 77), kind,
               "second tile")


# ---------------------------------------------------------------------------
# heights, tree counts
# ---------------------------------------------------------------------------


class TestForests:
    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    @pytest.mark.parametrize("n", [2, 3, 8, 64, 256, 300])
    def test_heights(self, dev, n, kind):
        """256 is the flagship's H = 8; 300 gives H = 9, whose 1024-slot
        heap is larger than max_nodes = 599."""
        d = 5
        forest = _forest(d, n, 9, kind)
        H = _height(forest)
        assert H == max(int(np.ceil(np.log2(n))), 1)
        if n == 300:
            assert forest.feature.shape[1] == 599 and (2 << H) == 1024
        _check(dev, forest, _rows(1000, d, kind, 41), kind, f"{kind} n={n}")

    def test_too_deep_falls_back(self, dev):
        """n = 16384 gives H = 14: four trees of 2^15 slots do not fit the
        LDS budget (and the pre-order records do not either), so the route
        is the v4 walk over nodes in global memory."""
        d, kind = 5, "bf16"
        forest = _forest(d, 16384, 8, kind)
        assert _height(forest) == 14
        _check(dev, forest, _rows(1000, d, kind, 43), kind, "n=16384",
               route="v4_global_nodes")

    def test_deepest_heap(self, dev):
        """n = 4096, H = 12: 4 x 32 KB of heap records, the deepest forest
        of ours that stays on the route."""
        d, kind = 5, "bf16"
        forest = _forest(d, 4096, 8, kind)
        assert _height(forest) == 12
        _check(dev, forest, _rows(1000, d, kind, 43), kind, "n=4096")

    @pytest.mark.parametrize("T", [1, 7, 8, 9, 12])
    def test_tree_counts(self, dev, T):
        d, kind = 5, "bf16"
        _check(dev, _forest(d, 64, T, kind), _rows(1000, d, kind, 41), kind,
               f"T={T}")

    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    def test_flagship_shape_and_scores(self, dev, kind):
        """maxSamples = 256, d = 32, and the finalized score."""
        d = 32
        forest = _forest(d, 256, 8, kind)
        assert _route(forest, d, kind) == "heap"
        X = _rows(1000, d, kind, 3000 + d)
        got = gpu_engine.score_forest(Shell(forest), _to_dev(X, kind, dev),
                                      finalize=True)
        want = cpu_engine.scores_from_path_sums(
            _oracle(forest, X), forest.num_trees, forest.num_samples)
        _assert_bitwise(got.cpu().numpy(), want, f"{kind} scores")


# ---------------------------------------------------------------------------
# feature counts and the slab-offset bound
# ---------------------------------------------------------------------------

# (d + 1) * rpt * 256 * 2 <= 65536 for some rpt in {2, 1}: true up to
# d = 127 (rpt = 1, last slab offset 127 * 512 = 0xFE00), false from d = 128
# on. rpt = 2 is possible up to d = 63.
_SIDE = {1: "heap", 2: "heap", 32: "heap", 33: "heap", 37: "heap",
         63: "heap", 64: "heap", 127: "heap", 128: "v4"}


class TestFeatureCounts:
    @pytest.mark.parametrize("d", sorted(_SIDE))
    def test_offset_bound(self, dev, d):
        kind = "bf16"
        assert ((d + 1) * 256 * 2 <= 65536) == (_SIDE[d] == "heap")
        forest = _forest(d, 256, 8, kind)
        assert forest.feature.shape[1] == 511
        _check(dev, forest, _rows(1000, d, kind, 3000 + d), kind,
               f"d={d}", route=_SIDE[d])

    def test_last_feature_is_used(self, dev):
        """At d = 127 the last feature's slab sits at 0xFC00 and the
        sentinel slab at 0xFE00: the forest must split on it."""
        forest = _forest(127, 256, 8, "bf16")
        assert (forest.feature == 126).any()


# ---------------------------------------------------------------------------
# shapes of trees and of values
# ---------------------------------------------------------------------------


class TestShapes:
    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    def test_all_constant_data(self, dev, kind):
        """Every root is a leaf: H = 1 and the pass-through is the root."""
        d = 5
        forest = _forest(d, 64, 9, kind, constant="all")
        assert (np.asarray(forest.node_count) == 1).all()
        _check(dev, forest, _rows(1000, d, kind, 41), kind, "constant data")

    def test_constant_column_and_shallow_leaves(self, dev):
        """Leaves far above the height limit: the pass-through chain runs
        most of the height."""
        d, kind = 5, "bf16"
        forest = _forest(d, 256, 9, kind, constant="column")
        assert not (forest.feature == 0).any()
        depth = gpu_engine._node_depths(forest.feature, forest.right)
        leaf = forest.feature == -1
        assert depth[leaf].min() <= 3 and _height(forest) == 8
        _check(dev, forest, _rows(1000, d, kind, 41), kind,
               "constant column")

    def test_duplicated_rows(self, dev):
        d, kind = 5, "bf16"
        forest = _forest(d, 64, 9, kind)
        X = np.repeat(_rows(100, d, kind, 5), 10, axis=0)
        _check(dev, forest, X, kind, "duplicated rows")

    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    def test_rows_on_split_values(self, dev, kind):
        """Split values rounded into the row dtype: equality must go
        right (x < t goes left)."""
        d = 5
        forest = _forest(d, 256, 9, kind)
        X = split_rows(forest, 1000, d, kind)
        internal = forest.feature >= 0
        splits = np.resize(
            gpu_engine._split_thresholds32(forest)[internal], X.shape)
        # a split value that rounds up (or is exact) gives the row the
        # threshold's own key: the compare meets equality there, and one
        # that rounds down sits just left of it
        thr = gpu_engine._threshold_keys(splits.reshape(-1), kind) >> 16
        keys = row_keys(X, kind)[:, :d].reshape(-1)
        assert ((keys == thr) == (X >= splits).reshape(-1)).all()
        assert (keys == thr).any() and (keys < thr).any()
        _check(dev, forest, X, kind, f"{kind} rows on split values")

    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    def test_special_values(self, dev, kind):
        d = 5
        forest = _forest(d, 64, 9, kind)
        sub = np.float32(2.0 ** -24) if kind == "f16" else \
            np.array([0x00010000], dtype=np.uint32).view(np.float32)[0]
        vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub,
                         1e20, -1e20, 1e-20, -1e-20], dtype=np.float32)
        X = np.array(_rows(1000, d, kind, 47))
        for r in range(0, 1000, 7):
            X[r] = vals[(np.arange(d) + r) % len(vals)]
        X = round_rows(X, kind)
        _check(dev, forest, X, kind, f"{kind} special values")

    def test_scales(self, dev):
        """A forest fitted on 1e+-20-scale data (bf16 keeps the range)."""
        d, kind = 5, "bf16"

        def make():
            rs = np.random.RandomState(3)
            X = rs.standard_normal((1000, d)).astype(np.float32)
            X[:, 0] *= 1e20
            X[:, 1] *= 1e-20
            X = round_rows(X, kind)
            bag = cpu_engine.sample_bags(1000, 9, 64, seed=17,
                                         bootstrap=False)
            fs = cpu_engine.feature_subsets(d, d, 9, seed=17)
            return cpu_engine.build_forest(X, bag, fs, 17, 64, d, d), X
        forest, X = _memo("scales", make)
        _check(dev, forest, X, kind, "1e+-20 scales")


# ---------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------


class TestLayouts:
    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    @pytest.mark.parametrize("layout", ["pitched", "feature_major"])
    def test_in_place(self, dev, layout, kind):
        d, N = 5, 1000
        forest = _forest(d, 64, 9, kind)
        X = _rows(N, d, kind, 41)
        assert _route(forest, d, kind, layout) == "heap"
        Xt = _to_dev(X, kind, dev)
        if layout == "pitched":
            buf = torch.zeros((N, d + 3), dtype=Xt.dtype, device=dev)
            view = buf[:, :d]
        else:
            buf = torch.zeros((d, N + 5), dtype=Xt.dtype, device=dev)
            view = buf[:, :N].T
        view.copy_(Xt)
        assert not view.is_contiguous()
        assert gpu_engine._rows_in_place(view) is view
        got = gpu_engine.score_forest(Shell(forest), view, finalize=False)
        _assert_bitwise(got.cpu().numpy(), _oracle(forest, X), layout)

    def test_unaligned_rows(self, dev):
        """A contiguous d = 8 tensor at an odd element offset of its storage
        must take the element-wise staging."""
        d, kind = 8, "bf16"
        forest = _forest(d, 64, 8, kind)
        assert _route(forest, d, kind) == "heap"
        X = _rows(1000, d, kind, 91)
        flat = torch.empty(1000 * d + 1, dtype=torch.bfloat16, device=dev)
        Xt = flat[1:].view(1000, d)
        Xt.copy_(_to_dev(X, kind, dev))
        assert Xt.is_contiguous() and Xt.data_ptr() % 16 != 0
        got = gpu_engine.score_forest(Shell(forest), Xt, finalize=False)
        _assert_bitwise(got.cpu().numpy(), _oracle(forest, X), "unaligned X")


# ---------------------------------------------------------------------------
# EIF extension level 0
# ---------------------------------------------------------------------------


class TestEif0:
    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    @pytest.mark.parametrize("d", [5, 32])
    def test_heap_route(self, dev, d, kind):
        forest = _forest(d, 64, 9, kind, ext=0)
        X = _rows(1000, d, kind, 45)
        shell = Shell(forest)
        out, _ = _routed(gpu_engine.score_extended_forest, shell,
                         _to_dev(X, kind, dev), "score_forest")
        (key, (aos, _, extra)), = shell._gpu_forest_cache.items()
        assert key[2][0] == "eif0"
        assert _ext().score_route(kind, d, aos.shape[1], extra["height"],
                                  "packed") == "heap"
        assert extra["heap"] is not None
        assert extra["heap"].shape == (16, 2 << extra["height"])
        _assert_bitwise(out.cpu().numpy(), _oracle(forest, X),
                        f"{kind} eif ext-0 d={d}")


# ---------------------------------------------------------------------------
# the converter alone
# ---------------------------------------------------------------------------


class TestConverter:
    @pytest.mark.parametrize("case", ["n2", "n3", "n8", "n64", "n256", "n300",
                                      "single-leaf", "column", "d63", "d127",
                                      "eif0"])
    def test_word_for_word(self, dev, case):
        kind = "bf16"
        d = {"d63": 63, "d127": 127}.get(case, 5)
        if case == "eif0":
            packed, ncount, H = gpu_engine._eif0_packed_v4(
                _forest(d, 64, 9, kind, ext=0), d, kind)
        else:
            n = {"single-leaf": 64, "column": 256, "d63": 256,
                 "d127": 256}.get(case) or int(case[1:])
            const = {"single-leaf": "all", "column": "column"}.get(case,
                                                                   False)
            packed, ncount, H = gpu_engine._nodes_packed_v4(
                _forest(d, n, 9, kind, constant=const), d, kind)
        assert packed.shape[0] == 16  # 9 trees + 7 padding trees
        assert _ext().score_route(kind, d, packed.shape[1], H,
                                  "packed") == "heap"
        # the instantiation's slab: rpt = 2 where three blocks of it fit a
        # CU next to four trees, else rpt = 1
        tile2 = (d + 1) * 512 * 2
        lds2 = tile2 + 4 * (2 << H) * 4
        lds1 = tile2 // 2 + 4 * (2 << H) * 4
        rpt = 2 if tile2 <= 65536 and lds2 <= 150 * 1024 and \
            min(160 * 1024 // lds2, 3) >= min(160 * 1024 // lds1, 3) else 1
        assert rpt == {"d63": 1, "d127": 1}.get(case, 2)
        want = heap_reference(packed, H, rpt * 512)
        got = _ext().v4_heap_order(torch.from_numpy(packed).to(dev),
                                   torch.from_numpy(ncount).to(dev), H, d)
        assert got.dtype == torch.int32 and got.shape == want.shape
        got = got.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got, want)
        # padding trees: a root pass-through that ends in 0.0f, and (the
        # reference's own construction aside) slot 0 and unreached slots 0
        assert (got[:, 0] == 0).all()
        assert (got[9:, 1] == d * rpt * 512).all()
        assert (got[9:, -1] == 0).all()
        assert (np.delete(got[9:], [1, 3, 7, 15, 31, 63, 127, 255, 511, 1023]
                          [:H + 1], axis=1) == 0).all()


# ---------------------------------------------------------------------------
# the old route
# ---------------------------------------------------------------------------


class TestOldRoute:
    def test_f32_rows(self, dev):
        d, kind = 5, "f32"
        forest = _forest(d, 64, 9, kind)
        _check(dev, forest, _rows(1000, d, kind, 41), kind, "f32",
               route="v4")

    def test_switch(self, dev, monkeypatch):
        """IFA_SCORE_HEAP=0 keeps 16-bit rows on the v4 route, whether the
        pack was made before or after it was set."""
        d, kind = 5, "bf16"
        forest = _forest(d, 64, 9, kind)
        X = _rows(1000, d, kind, 41)
        shell = Shell(forest)
        Xt = _to_dev(X, kind, dev)
        gpu_engine.score_forest(shell, Xt, finalize=False)  # heap pack
        monkeypatch.setenv("IFA_SCORE_HEAP", "0")
        assert os.environ["IFA_SCORE_HEAP"] == "0"
        assert _route(forest, d, kind) == "v4"
        got = gpu_engine.score_forest(shell, Xt, finalize=False)
        _assert_bitwise(got.cpu().numpy(), _oracle(forest, X),
                        "switch, pack made before")
        _check(dev, forest, X, kind, "switch, pack made after", route="v4")
        monkeypatch.delenv("IFA_SCORE_HEAP")
        assert _route(forest, d, kind) == "heap"
