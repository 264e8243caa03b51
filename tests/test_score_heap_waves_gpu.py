"""GPU tests (MI355X) for the 512-thread blocks of score_forest_heap.

Where the heap route takes a 512-row key tile, the tile is walked by 512
threads with one row each (8 waves per block) instead of 256 threads with
two; IFA_HEAP_WAVES=4|8 picks the block size. The tile, its slot map and the
heap records are the same for both (tests/test_score_heap_waves_ref.py), so
what can go wrong is what depends on the thread count: who stages, walks and
stores which row (rows 256-511 of a tile belong to waves 4-7), the stride of
the tree-stage copy, tail tiles whose upper waves hold only sentinel rows,
and the route. Every case asserts the block size score_heap_block reports,
runs under both values, compares each result bitwise with the strict-order
CPU engine, and the two results with each other.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.ops import gpu_engine  # noqa: E402
from tests.test_gpu_edges import Shell, _assert_bitwise, _routed  # noqa: E402
from tests.test_score_heap_gpu import (  # noqa: E402
    _ext,
    _forest,
    _height,
    _oracle,
    _rows,
    _to_dev,
)
from tests.test_score_heap_ref import round_rows  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def _block(forest, d, kind):
    return int(_ext().score_heap_block(kind, d, forest.feature.shape[1],
                                       _height(forest)))


def _both_waves(dev, monkeypatch, forest, X, kind, what, view=None,
                finalize=False, block8=512, one_pack=False):
    """Score under IFA_HEAP_WAVES=4 and =8. `block8` is the block size the
    second run must report: 512, or 256 where no 512-row tile is routed.
    `view(Xt)` re-lays the device rows; `one_pack` scores both runs with
    the pack made under the first."""
    d = X.shape[1]
    want = _oracle(forest, X)
    if finalize:
        want = cpu_engine.scores_from_path_sums(want, forest.num_trees,
                                                forest.num_samples)
    Xt = _to_dev(X, kind, dev)
    if view is not None:
        Xt = view(Xt)
    mn, h = forest.feature.shape[1], _height(forest)
    got = {}
    shell = None
    for waves in (4, 8):
        monkeypatch.setenv("IFA_HEAP_WAVES", str(waves))
        assert _ext().score_route(kind, d, mn, h, "packed") == "heap", what
        assert _block(forest, d, kind) == (256 if waves == 4 else block8), \
            f"{what} waves={waves}"
        if shell is None or not one_pack:
            shell = Shell(forest)
        out = gpu_engine.score_forest(shell, Xt, finalize=finalize)
        (_, _, extra), = shell._gpu_forest_cache.values()
        assert extra["heap"] is not None, what
        got[waves] = out.cpu().numpy()
        _assert_bitwise(got[waves], want, f"{what} waves={waves}")
    assert np.array_equal(got[4].view(np.int32), got[8].view(np.int32)), what


class TestSwitch:
    def test_default_and_invalid_values(self, dev, monkeypatch):
        """Unset and invalid values give the routed choice: 512 threads on
        the flagship's 512-row tile. The (phase, tile rows / 256) pair the
        pack is laid out for does not move with the switch."""
        forest = _forest(32, 256, 8, "bf16")
        mn, h = forest.feature.shape[1], _height(forest)
        monkeypatch.delenv("IFA_HEAP_WAVES", raising=False)
        monkeypatch.delenv("IFA_HEAP_PHASE", raising=False)
        assert _block(forest, 32, "bf16") == 512
        for bad in ("", "0", "2", "6", "16", "x", "-8"):
            monkeypatch.setenv("IFA_HEAP_WAVES", bad)
            assert _block(forest, 32, "bf16") == 512, bad
        for waves, block in ((4, 256), (8, 512)):
            monkeypatch.setenv("IFA_HEAP_WAVES", str(waves))
            assert _block(forest, 32, "bf16") == block
            assert _block(forest, 32, "f16") == block
            assert tuple(_ext().score_heap_cfg("bf16", 32, mn, h)) == (8, 2)
        assert _block(forest, 32, "f32") == 0  # off the heap route

    def test_256_row_tile_keeps_256_threads(self, dev, monkeypatch):
        """d = 45 at H = 8 takes a 256-row tile: 256 threads whatever the
        switch says."""
        d, kind = 45, "bf16"
        forest = _forest(d, 256, 8, kind)
        monkeypatch.delenv("IFA_HEAP_WAVES", raising=False)
        assert tuple(_ext().score_heap_cfg(
            kind, d, forest.feature.shape[1], _height(forest))) == (8, 1)
        assert _block(forest, d, kind) == 256
        _both_waves(dev, monkeypatch, forest, _rows(700, d, kind, 3000 + d),
                    kind, "d=45", block8=256)


class TestRowCounts:
    @pytest.mark.parametrize("N", [1, 255, 256, 257, 511, 512, 513, 1025])
    def test_rows(self, dev, monkeypatch, N):
        d, kind = 32, "bf16"
        forest = _forest(d, 256, 9, kind)
        assert _height(forest) == 8
        _both_waves(dev, monkeypatch, forest, _rows(N, d, kind, 2000 + N),
                    kind, f"N={N}")

    def test_grid_stride(self, dev, monkeypatch):
        """Five tiles over two blocks: block 0 walks tiles 0, 2 and the
        one-row tail tile 4."""
        d, kind, N = 32, "bf16", 2049
        monkeypatch.setenv("IFA_HEAP_MAX_BLOCKS", "2")
        _both_waves(dev, monkeypatch, _forest(d, 256, 9, kind),
                    _rows(N, d, kind, 2000 + N), kind, "grid-stride")

    def test_default_grid(self, dev, monkeypatch):
        """8193 tiles over the default grid of 8192 blocks: block 0 walks a
        second tile, and that tile is a one-row tail."""
        d, kind = 2, "bf16"
        N = 8192 * 512 + 513
        monkeypatch.delenv("IFA_HEAP_MAX_BLOCKS", raising=False)
        _both_waves(dev, monkeypatch, _forest(d, 8, 8, kind),
                    _rows(N, d, kind, 77), kind, "default grid")


class TestTreeCounts:
    @pytest.mark.parametrize("T", [1, 7, 8, 9, 13])
    def test_tree_counts(self, dev, monkeypatch, T):
        d, kind = 5, "bf16"
        _both_waves(dev, monkeypatch, _forest(d, 64, T, kind),
                    _rows(600, d, kind, 41), kind, f"T={T}")

    @pytest.mark.parametrize("phase", [4, 8])
    def test_phases(self, dev, monkeypatch, phase):
        d, kind = 32, "bf16"
        forest = _forest(d, 256, 13, kind)
        monkeypatch.setenv("IFA_HEAP_PHASE", str(phase))
        assert tuple(_ext().score_heap_cfg(
            kind, d, forest.feature.shape[1], _height(forest))) == (phase, 2)
        _both_waves(dev, monkeypatch, forest, _rows(513, d, kind, 2513),
                    kind, f"phase={phase}")


class TestShapes:
    @pytest.mark.parametrize("d", [1, 36])
    def test_widths(self, dev, monkeypatch, d):
        kind = "bf16"
        forest = _forest(d, 256, 8, kind)
        assert forest.feature.shape[1] == 511 and _height(forest) == 8
        _both_waves(dev, monkeypatch, forest, _rows(700, d, kind, 3000 + d),
                    kind, f"d={d}")

    @pytest.mark.parametrize("n,H", [(2, 1), (3, 2), (128, 7)])
    def test_heights(self, dev, monkeypatch, n, H):
        """H = 1: a tree is two 16-byte vectors, fewer than one per
        thread."""
        d, kind = 5, "bf16"
        forest = _forest(d, n, 9, kind)
        assert _height(forest) == H
        _both_waves(dev, monkeypatch, forest, _rows(600, d, kind, 43), kind,
                    f"H={H}")

    @pytest.mark.parametrize("phase", [4, 8])
    def test_fp16_rows(self, dev, monkeypatch, phase):
        d, kind = 32, "f16"
        monkeypatch.setenv("IFA_HEAP_PHASE", str(phase))
        _both_waves(dev, monkeypatch, _forest(d, 256, 9, kind),
                    _rows(700, d, kind, 3032), kind, f"fp16 phase={phase}")

    @pytest.mark.parametrize("finalize", [False, True])
    def test_finalize(self, dev, monkeypatch, finalize):
        d, kind = 32, "bf16"
        _both_waves(dev, monkeypatch, _forest(d, 256, 8, kind),
                    _rows(1000, d, kind, 3000 + d), kind,
                    f"finalize={finalize}", finalize=finalize)

    def test_pack_is_shared(self, dev, monkeypatch):
        """The records do not depend on the block size: a pack made under
        IFA_HEAP_WAVES=4 is walked as it is under 8."""
        d, kind = 32, "bf16"
        _both_waves(dev, monkeypatch, _forest(d, 256, 9, kind),
                    _rows(1025, d, kind, 3025), kind, "one pack",
                    one_pack=True)

    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    def test_special_values_in_the_upper_waves(self, dev, monkeypatch, kind):
        """NaN, +-inf, zeros and denormals in rows 256-511 of both tiles."""
        d, N = 5, 1024
        forest = _forest(d, 64, 9, kind)
        sub = np.float32(2.0 ** -24) if kind == "f16" else \
            np.array([0x00010000], dtype=np.uint32).view(np.float32)[0]
        vals = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, sub, -sub,
                         1e20, -1e20], dtype=np.float32)
        X = np.array(_rows(N, d, kind, 47))
        for base in (256, 768):
            for r in range(base, base + 256, 3):
                X[r] = vals[(np.arange(d) + r) % len(vals)]
            for i, v in enumerate(vals):  # whole rows of one value
                X[base + 1 + 3 * i] = v
        X = round_rows(X, kind)
        assert np.isnan(X[256:512]).any() and np.isinf(X[768:]).any()
        _both_waves(dev, monkeypatch, forest, X, kind,
                    f"{kind} special values")


class TestLayouts:
    @pytest.mark.parametrize("phase", [4, 8])
    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    @pytest.mark.parametrize("layout", ["pitched", "feature_major"])
    def test_layouts(self, dev, monkeypatch, layout, kind, phase):
        """The four strided 512-thread instantiations (bf16 and fp16, 4 and
        8 trees per phase), each on both views."""
        d, N = 5, 513
        forest = _forest(d, 64, 9, kind)
        monkeypatch.setenv("IFA_HEAP_PHASE", str(phase))
        assert _ext().score_route(kind, d, forest.feature.shape[1],
                                  _height(forest), layout) == "heap"
        assert tuple(_ext().score_heap_cfg(
            kind, d, forest.feature.shape[1], _height(forest))) == (phase, 2)

        def view(Xt):
            if layout == "pitched":
                buf = torch.zeros((N, d + 3), dtype=Xt.dtype, device=dev)
                v = buf[:, :d]
            else:
                buf = torch.zeros((d, N + 5), dtype=Xt.dtype, device=dev)
                v = buf[:, :N].T
            v.copy_(Xt)
            assert not v.is_contiguous()
            assert gpu_engine._rows_in_place(v) is v
            return v
        _both_waves(dev, monkeypatch, forest, _rows(N, d, kind, 41), kind,
                    f"{kind} {layout} phase={phase}", view=view)


class TestEif0:
    def test_ext0(self, dev, monkeypatch):
        d, kind = 32, "bf16"
        forest = _forest(d, 64, 9, kind, ext=0)
        X = _rows(600, d, kind, 45)
        want = _oracle(forest, X)
        Xt = _to_dev(X, kind, dev)
        got = {}
        for waves, block in ((4, 256), (8, 512)):
            monkeypatch.setenv("IFA_HEAP_WAVES", str(waves))
            shell = Shell(forest)
            out, _ = _routed(gpu_engine.score_extended_forest, shell, Xt,
                             "score_forest")
            (key, (aos, _, extra)), = shell._gpu_forest_cache.items()
            assert key[2][0] == "eif0" and extra["heap"] is not None
            assert int(_ext().score_heap_block(
                kind, d, aos.shape[1], extra["height"])) == block
            got[waves] = out.cpu().numpy()
            _assert_bitwise(got[waves], want, f"eif ext-0 waves={waves}")
        assert np.array_equal(got[4].view(np.int32), got[8].view(np.int32))
