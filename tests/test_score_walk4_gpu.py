"""GPU tests (MI355X) for the four-instruction visit and the 8-tree barrier
phase of score_forest_heap.

The walk tracks the complemented slot over trees staged reversed in LDS
(tests/test_score_walk4_ref.py has the arithmetic), and stages 8 trees per
barrier phase where that fits, 4 otherwise; IFA_HEAP_PHASE=4|8 picks one.
What can go wrong is the reversed copy (per tree, per 16-byte vector), the
negative index, the `>=` edge of the subtract form, the pass-through
records, the phase boundaries, and the RPT choice moving with the larger
stage. So every case asserts the route, runs under both phases with a pack
made under that phase, compares each result bitwise with the strict-order
CPU engine, and the two results with each other.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

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
from tests.test_score_heap_ref import round_rows, split_rows  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def _cfg(forest, d, kind, height=None):
    h = _height(forest) if height is None else height
    mn = forest.feature.shape[1]
    return (_ext().score_route(kind, d, mn, h, "packed"),
            tuple(_ext().score_heap_cfg(kind, d, mn, h)))


def _both_phases(dev, monkeypatch, forest, X, kind, what, view=None,
                 phase8=8):
    """Score under IFA_HEAP_PHASE=4 and =8, each with its own pack (the
    records are laid out for the RPT the phase chooses). `phase8` is the
    phase the second run must report: 8, or 4 where 8 is not routable.
    `view(Xt)` re-lays the device rows."""
    d = X.shape[1]
    want = _oracle(forest, X)
    Xt = _to_dev(X, kind, dev)
    if view is not None:
        Xt = view(Xt)
    got = {}
    for ph in (4, 8):
        monkeypatch.setenv("IFA_HEAP_PHASE", str(ph))
        route, (phase, rpt) = _cfg(forest, d, kind)
        assert route == "heap", f"{what} phase={ph}"
        assert phase == (4 if ph == 4 else phase8), f"{what} phase={ph}"
        assert rpt in (1, 2)
        shell = Shell(forest)
        out = gpu_engine.score_forest(shell, Xt, finalize=False)
        (_, _, extra), = shell._gpu_forest_cache.values()
        assert extra["heap"] is not None, what
        got[ph] = out.cpu().numpy()
        _assert_bitwise(got[ph], want, f"{what} phase={ph}")
    assert np.array_equal(got[4].view(np.int32), got[8].view(np.int32)), what
    monkeypatch.delenv("IFA_HEAP_PHASE")


class TestSwitch:
    def test_default_and_invalid_values(self, dev, monkeypatch):
        """Unset and invalid values give the routed choice: 8 trees at the
        flagship's H = 8, 4 trees at H = 12 whatever is asked."""
        forest = _forest(32, 256, 8, "bf16")
        monkeypatch.delenv("IFA_HEAP_PHASE", raising=False)
        assert _cfg(forest, 32, "bf16") == ("heap", (8, 2))
        for bad in ("", "0", "6", "16", "x", "-8"):
            monkeypatch.setenv("IFA_HEAP_PHASE", bad)
            assert _cfg(forest, 32, "bf16") == ("heap", (8, 2)), bad
        monkeypatch.setenv("IFA_HEAP_PHASE", "4")
        assert _cfg(forest, 32, "bf16") == ("heap", (4, 2))
        monkeypatch.setenv("IFA_HEAP_PHASE", "8")
        assert _ext().score_route("bf16", 5, 8191, 12, "packed") == "heap"
        assert tuple(_ext().score_heap_cfg("bf16", 5, 8191, 12)) == (4, 2)
        assert _cfg(forest, 32, "f32") == ("v4", (0, 0))


class TestTreeCounts:
    @pytest.mark.parametrize("T", [1, 3, 4, 5, 7, 8, 9, 12, 13, 100])
    def test_tree_counts(self, dev, monkeypatch, T):
        d, kind = 5, "bf16"
        _both_phases(dev, monkeypatch, _forest(d, 64, T, kind),
                     _rows(600, d, kind, 41), kind, f"T={T}")


class TestRowCounts:
    @pytest.mark.parametrize("N", [1, 255, 256, 257, 511, 513, 1025])
    def test_rows(self, dev, monkeypatch, N):
        d, kind = 32, "bf16"
        forest = _forest(d, 64, 9, kind)
        monkeypatch.delenv("IFA_HEAP_PHASE", raising=False)
        assert _cfg(forest, d, kind)[1] == (8, 2)  # RPT = 2: 512-row tiles
        _both_phases(dev, monkeypatch, forest, _rows(N, d, kind, 2000 + N),
                     kind, f"N={N}")


class TestWidths:
    @pytest.mark.parametrize("d", [1, 36, 37, 44, 45, 63, 64, 127])
    def test_widths(self, dev, monkeypatch, d):
        """maxSamples = 256 (H = 8, 511 nodes): the widths either side of
        where RPT = 1 starts with a 4-tree and with an 8-tree stage."""
        kind = "bf16"
        forest = _forest(d, 256, 8, kind)
        assert forest.feature.shape[1] == 511 and _height(forest) == 8
        _both_phases(dev, monkeypatch, forest, _rows(700, d, kind, 3000 + d),
                     kind, f"d={d}")


    def test_phase_switched_after_the_pack(self, dev, monkeypatch):
        """d = 37: the 4-tree phase runs RPT = 2, the 8-tree phase RPT = 1,
        and the records' slab offsets are laid out for one of them. A pack
        made under the other phase must not be walked with them."""
        d, kind = 37, "bf16"
        forest = _forest(d, 256, 8, kind)
        X = _rows(700, d, kind, 3000 + d)
        Xt = _to_dev(X, kind, dev)
        for first, then in ((4, 8), (8, 4)):
            monkeypatch.setenv("IFA_HEAP_PHASE", str(first))
            rpt_first = _cfg(forest, d, kind)[1][1]
            shell = Shell(forest)
            gpu_engine.score_forest(shell, Xt, finalize=False)
            monkeypatch.setenv("IFA_HEAP_PHASE", str(then))
            assert _cfg(forest, d, kind)[1][1] != rpt_first
            got = gpu_engine.score_forest(shell, Xt, finalize=False)
            _assert_bitwise(got.cpu().numpy(), _oracle(forest, X),
                            f"phase {first} pack scored under {then}")


class TestHeights:
    @pytest.mark.parametrize("n,H", [(2, 1), (3, 2), (128, 7), (256, 8),
                                     (2048, 11), (4096, 12)])
    def test_heights(self, dev, monkeypatch, n, H):
        """H = 12 stays on the heap route and runs the 4-tree phase (8 x 32
        KB of records do not fit); H = 11 does too, by resident blocks."""
        d, kind = 5, "bf16"
        forest = _forest(d, n, 9, kind)
        assert _height(forest) == H
        _both_phases(dev, monkeypatch, forest, _rows(600, d, kind, 43), kind,
                     f"H={H}", phase8=8 if H <= 8 else 4)


def _ulp_neighbours(X, kind):
    """X (exact in `kind`) with its 16-bit pattern one step down, as is, and
    one step up, stacked."""
    if kind == "bf16":
        bits = (np.ascontiguousarray(X).view(np.uint32) >> 16).astype(np.int64)
    else:
        bits = X.astype(np.float16).view(np.uint16).astype(np.int64)
    out = []
    for step in (-1, 0, 1):
        b = np.clip(bits + step, 0, 0xFFFF).astype(np.uint32)
        if kind == "bf16":
            out.append((b << 16).astype(np.uint32).view(np.float32))
        else:
            out.append(b.astype(np.uint16).view(np.float16)
                       .astype(np.float32))
    return np.concatenate(out, axis=0)


class TestValues:
    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    def test_on_and_next_to_split_values(self, dev, monkeypatch, kind):
        d = 5
        forest = _forest(d, 256, 9, kind)
        X = _ulp_neighbours(split_rows(forest, 200, d, kind), kind)
        assert X.shape == (600, d)
        assert np.array_equal(round_rows(X, kind).view(np.int32),
                              X.view(np.int32))
        _both_phases(dev, monkeypatch, forest, X, kind,
                     f"{kind} split values +-1 ulp")

    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    def test_special_values(self, dev, monkeypatch, kind):
        d = 5
        forest = _forest(d, 64, 9, kind)
        sub = np.float32(2.0 ** -24) if kind == "f16" else \
            np.array([0x00010000], dtype=np.uint32).view(np.float32)[0]
        vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub,
                         1e20, -1e20, 1e-20, -1e-20], dtype=np.float32)
        X = np.array(_rows(600, d, kind, 47))
        for r in range(0, 600, 3):
            X[r] = vals[(np.arange(d) + r) % len(vals)]
        for i, v in enumerate(vals):  # whole rows of one value
            X[1 + 3 * i] = v
        X = round_rows(X, kind)
        _both_phases(dev, monkeypatch, forest, X, kind,
                     f"{kind} special values")

    def test_constant_column(self, dev, monkeypatch):
        """Shallow leaves: pass-through records most of the height."""
        d, kind = 5, "bf16"
        forest = _forest(d, 256, 9, kind, constant="column")
        assert not (forest.feature == 0).any() and _height(forest) == 8
        _both_phases(dev, monkeypatch, forest, _rows(600, d, kind, 41), kind,
                     "constant column")

    def test_single_leaf_trees(self, dev, monkeypatch):
        """Every root is a leaf: H = 1, the root is a pass-through."""
        d, kind = 5, "bf16"
        forest = _forest(d, 64, 9, kind, constant="all")
        assert (np.asarray(forest.node_count) == 1).all()
        _both_phases(dev, monkeypatch, forest, _rows(600, d, kind, 41), kind,
                     "single-leaf trees")


class TestLayouts:
    @pytest.mark.parametrize("kind", ["bf16", "f16"])
    @pytest.mark.parametrize("layout", ["packed", "pitched", "feature_major"])
    def test_layouts(self, dev, monkeypatch, layout, kind):
        d, N = 5, 513
        forest = _forest(d, 64, 9, kind)
        assert _ext().score_route(kind, d, forest.feature.shape[1],
                                  _height(forest), layout) == "heap"

        def view(Xt):
            if layout == "packed":
                return Xt
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
        _both_phases(dev, monkeypatch, forest, _rows(N, d, kind, 41), kind,
                     f"{kind} {layout}", view=view)


class TestEif0:
    def test_ext0(self, dev, monkeypatch):
        d, kind = 32, "bf16"
        forest = _forest(d, 64, 9, kind, ext=0)
        X = _rows(600, d, kind, 45)
        want = _oracle(forest, X)
        Xt = _to_dev(X, kind, dev)
        got = {}
        for ph in (4, 8):
            monkeypatch.setenv("IFA_HEAP_PHASE", str(ph))
            shell = Shell(forest)
            out, _ = _routed(gpu_engine.score_extended_forest, shell, Xt,
                             "score_forest")
            (key, (aos, _, extra)), = shell._gpu_forest_cache.items()
            assert key[2][0] == "eif0" and extra["heap"] is not None
            assert _ext().score_route(kind, d, aos.shape[1], extra["height"],
                                      "packed") == "heap"
            assert tuple(_ext().score_heap_cfg(
                kind, d, aos.shape[1], extra["height"])) == (ph, 2)
            got[ph] = out.cpu().numpy()
            _assert_bitwise(got[ph], want, f"eif ext-0 phase={ph}")
        assert np.array_equal(got[4].view(np.int32), got[8].view(np.int32))
