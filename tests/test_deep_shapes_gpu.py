"""GPU tests (MI355X): the five deep routes for forests past the 15-bit node
ids (score_forest_deep, explain_forest_deep, score_extended_deep,
explain_extended_deep, shap_forest_deep) at the shapes their own test files
never reach, against the CPU oracle bit for bit:

  * links at the 20-bit cap, bit 31 of the record word in use;
  * barrier phases that mix a single leaf, a stump, spines of depth 40 and
    trees of thousands of nodes; 1, 4, 8 and 9 trees;
  * feature ids up to d - 1 at the widest rows every route stages, one row
    a thread, the 128-bit staging branch on and off;
  * 1, tile - 1, tile and tile + 1 rows, and a block that strides to a
    second and third tile;
  * cells on a threshold of their own walk and one step of the row's type
    to either side, signed zeros, denormals, float64 splits between two f32
    values.

The forests and rows come from tests/deep_shapes.py;
tests/test_deep_shapes_ref.py asserts on the oracle alone that they reach
these places. Every comparison is np.array_equal on the int32 view.
"""

import collections
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.core.forest import ExtendedForest  # noqa: E402
from isolation_forest_amd.ops import gpu_engine  # noqa: E402
from tests import deep_shapes as S  # noqa: E402

KINDS = list(S.KINDS)
N_ROWS = 600     # more than one tile of two rows a thread
N_SHAP = 96      # the oracle's cost grows with rows times leaves
CAP = 1 << 20


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def ext():
    from isolation_forest_amd.ops import load_extension

    return load_extension()


class Shell:
    """What the gpu_engine entry points read of a model."""

    def __init__(self, forest):
        self.forest = forest
        self._gpu_forest_cache = {}


Route = collections.namedtuple(
    "Route", "extended run oracle where fallback pack stage_env min_stage")

ROUTES = {
    "score": Route(
        False,
        lambda m, X: gpu_engine.score_forest(m, X, finalize=False),
        cpu_engine.path_lengths,
        gpu_engine.large_score_route, "wide", "deep", "IFA_DEEP_STAGE", "64"),
    "explain": Route(
        False,
        lambda m, X: gpu_engine.explain_forest(m, X, finalize=False),
        lambda f, X: cpu_engine.feature_contributions(f, X, False),
        gpu_engine.large_explain_route, "cpu", "explain_deep",
        "IFA_EXPLAIN_DEEP_STAGE", "64"),
    "score_eif": Route(
        True,
        lambda m, X: gpu_engine.score_extended_forest_deep(
            m, X, finalize=False),
        cpu_engine.path_lengths_extended,
        gpu_engine.large_score_route, "wide", "eif_deep",
        "IFA_EIF_DEEP_STAGE", "2"),
    "explain_eif": Route(
        True,
        lambda m, X: gpu_engine.explain_extended_forest(m, X, finalize=False),
        lambda f, X: cpu_engine.feature_contributions_extended(f, X, False),
        gpu_engine.large_explain_route, "cpu", "explain_eif_deep",
        "IFA_EXPLAIN_DEEP_STAGE", "2"),
    "shap": Route(
        False,
        lambda m, X: gpu_engine.shap_forest(m, X, True),
        cpu_engine.shap_values,
        gpu_engine.large_shap_route, "cpu", "shap_deep", None, None),
}
WALKS = ["score", "explain", "score_eif", "explain_eif"]


def _cfg(route, kind, d):
    """(rows per thread, stage) the route's binding reports for these rows;
    the extended forests here have two coordinates a hyperplane"""
    e = ext()
    if route == "score":
        return tuple(e.score_deep_cfg(kind, d))
    if route == "explain":
        return tuple(e.explain_deep_cfg(kind, d)[:2])
    if route == "score_eif":
        c = e.score_eif_deep_cfg(kind, d, 2)
        return c[0], c[2]
    c = e.explain_eif_deep_cfg(kind, d, 2)
    return c[0], c[2]


@functools.lru_cache(maxsize=None)
def _widest(route, kind):
    """the widest rows of the kind the route still stages, asked of the
    binding"""
    return max(w for w in range(2, 4095) if _cfg(route, kind, w)[1] > 0)


def _with_last_column(forest, d):
    """the forest itself if it reads column d - 1, else a copy whose first
    root does"""
    ext_ = isinstance(forest, ExtendedForest)
    internal = forest.feature >= 0
    top = (forest.hyper_idx[internal] if ext_ else forest.feature).max()
    if top == d - 1:
        return forest
    forest = S.sliced(forest, forest.num_trees)
    assert forest.feature[0, 0] >= 0
    if ext_:
        forest.hyper_idx[0, 0, -1] = d - 1  # the coordinates stay ascending
    else:
        forest.feature[0, 0] = d - 1
    return forest


@functools.lru_cache(maxsize=None)
def _forest(name, extended=False):
    """("ragged",) ("ragged", T) ("built", d) ("built", d, k) ("foreign", ..)
    ("trie", H): built once, read-only"""
    if name[0] == "ragged":
        forest = S.ragged(S.built(S.SPINE_FEATURES, extended), extended)
        return forest if len(name) == 1 else S.sliced(forest, name[1])
    if name[0] == "built":
        return _with_last_column(S.built(name[1], extended, 5, *name[2:]),
                                 name[1])
    if name[0] == "foreign":
        return S.foreign64(_forest(name[1:], extended))
    assert name[0] == "trie"
    return S.trie(name[1], 6, extended)


def _width(forest):
    return forest.total_num_features


@functools.lru_cache(maxsize=None)
def _case(route, name, kind, n, d=None):
    """(forest, rows of the kind on the host, the oracle's answer for them):
    computed once and shared"""
    forest = _forest(name, ROUTES[route].extended)
    if name[0] == "trie":
        Xk = S.trie_rows(kind, 6, n)
    else:
        # a foreign copy is scored on the rows planted for its original
        base = _forest(name[1:], False) if name[0] == "foreign" else forest
        Xk = S.knife_rows(base, kind, n, d)[0]
    with np.errstate(all="ignore"):
        want = ROUTES[route].oracle(forest, S.widen(Xk))
    want.setflags(write=False)
    return forest, Xk, want


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _run(dev, route, forest, X, shell=None):
    r = ROUTES[route]
    d = int(X.shape[1])
    assert not gpu_engine._packed_fits(forest, d)
    assert r.where(forest, d, X.dtype) == "deep"
    shell = Shell(forest) if shell is None else shell
    return shell, r.run(shell, X.to(dev))


def _check(dev, route, name, kind, n, d=None, shell=None):
    forest, Xk, want = _case(route, name, kind, n, d)
    shell, got = _run(dev, route, forest, Xk, shell)
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))
    return shell


def _pack(shell, route):
    """(records, lds_levels, extra) of the route's pack in the shell's cache"""
    (pack,) = [v for k, v in shell._gpu_forest_cache.items()
               if isinstance(k[2], tuple) and k[2][0] == ROUTES[route].pack]
    return pack


# ---------------------------------------------------------------------------
# links at the cap
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("route,kind", [
    ("score", "f32"), ("score", "bf16"), ("score_eif", "bf16"),
    ("explain", "bf16")])
def test_links_at_the_cap(dev, route, kind):
    """One complete tree of 2^20 - 1 nodes: the last level's links need all
    20 bits, which sets bit 31 of the record word, and the frontier of the
    level-order kernel is 2^19 nodes wide. The oracle's tables for this tree
    take about 10 s for feature_contributions, which is run once here, and
    about a minute for shap_tables; the extended explain tables cost as much
    as the standard ones a second time. That is why shap and EIF explain
    are left out of this case."""
    n = CAP - 1
    shell = _check(dev, route, ("trie", 19), kind, 2000)
    records, lds_levels, _ = _pack(shell, route)
    # the 8-byte standard records pad a tree to an even count
    assert records.shape[1] == (CAP if route == "score" else n)
    words = records[0, :n, 0]
    links = (words.to(torch.int64) & 0xFFFFFFFF) >> 12
    assert int(links.max()) == CAP - 2
    assert bool((words < 0).any())  # bit 31
    assert int(lds_levels[0]) > 1 and not lds_levels[1:].any()


def test_one_node_past_the_cap_leaves_the_deep_routes(dev):
    for extended in (False, True):
        forest = S.sliced(_forest(("ragged",), extended), 1)
        d = _width(forest)
        forest.node_count[:] = CAP
        assert gpu_engine.large_score_route(forest, d, torch.float32) == "deep"
        forest.node_count[:] = CAP + 1
        assert gpu_engine.large_score_route(forest, d, torch.float32) == "wide"
        assert gpu_engine.large_explain_route(
            forest, d, torch.float32) == "cpu"
        if not extended:
            assert gpu_engine.large_shap_route(
                forest, d, torch.float32) == "cpu"


# ---------------------------------------------------------------------------
# the ragged forest
# ---------------------------------------------------------------------------


def _phases(lds_levels):
    levels = lds_levels.cpu().numpy()
    return [levels[i:i + 4] for i in range(0, len(levels), 4)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("route,stage", [
    ("score", None), ("score", "64"), ("explain", None), ("explain", "64"),
    ("score_eif", None), ("score_eif", "2"), ("explain_eif", None),
    ("explain_eif", "64"), ("explain_eif", "2"), ("shap", None)])
def test_ragged_forest(dev, monkeypatch, route, stage, kind):
    """Nine trees, every barrier phase from one record to thousands, at the
    default stage and at the smallest forced one."""
    if stage is not None:
        monkeypatch.setenv(ROUTES[route].stage_env, stage)
    n = N_SHAP if route == "shap" else N_ROWS
    shell = _check(dev, route, ("ragged",), kind, n)
    if route == "shap":
        return
    _, lds_levels, extra = _pack(shell, route)
    assert extra["height"] >= S.SPINE_DEPTH
    assert lds_levels.shape[0] == 12
    if stage is None:
        assert any(p.min() == 0 and p.max() > 1 for p in _phases(lds_levels))
    else:
        assert _cfg(route, kind, S.SPINE_FEATURES)[1] == int(stage)
        assert any(p.min() != p.max() for p in _phases(lds_levels))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("phase", [4, 2, 1])
@pytest.mark.parametrize("route", ["score_eif", "explain_eif"])
def test_ragged_forest_every_eif_phase(dev, monkeypatch, route, phase, kind):
    """IFA_EIF_DEEP_PHASE sets the trees a barrier phase of extended scoring
    stages; extended attribution takes its own from the shapes alone and
    must not be moved by the switch."""
    monkeypatch.setenv("IFA_EIF_DEEP_PHASE", str(phase))
    if route == "score_eif":
        assert ext().score_eif_deep_cfg(kind, S.SPINE_FEATURES, 2)[1] == phase
    _check(dev, route, ("ragged",), kind, N_ROWS)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("T", [1, 4, 8])
@pytest.mark.parametrize("route", ["score", "score_eif", "shap"])
def test_tree_counts(dev, route, T, kind):
    """One tree (a single leaf: records one node wide), a full phase, two
    full phases; test_ragged_forest has the nine."""
    _check(dev, route, ("ragged", T), kind,
           N_SHAP if route == "shap" else N_ROWS)


# ---------------------------------------------------------------------------
# feature ids and wide rows
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("route", WALKS)
def test_widest_rows(dev, route, kind):
    """The widest rows the route stages, one row a thread under the second
    LDS budget, the forest reading key-tile slabs up to d - 1."""
    d = _widest(route, kind)
    assert _cfg(route, kind, d)[0] == 1 and _cfg(route, kind, d + 1)[1] == 0
    name = ("built", d, 48)  # each tree over 48 of the d columns
    forest = _forest(name, ROUTES[route].extended)
    internal = forest.feature >= 0
    if ROUTES[route].extended:
        assert forest.hyper_idx[internal].max() == d - 1
    else:
        assert forest.feature.max() == d - 1
        assert len(np.unique(forest.feature[internal])) > 100
    _check(dev, route, name, kind, 300)


def _vector_width(route, kind, rpt):
    """the narrowest rows of at least 16 columns, a whole number of 16-byte
    pieces, that the route runs `rpt` rows a thread"""
    epv = 4 if kind == "f32" else 8
    return next(w for w in range(16, 4095, epv)
                if _cfg(route, kind, w)[0] == rpt)


@pytest.mark.parametrize("kind", KINDS)
def test_one_row_a_thread_standard_scoring(dev, kind):
    """score_forest_deep_kernel<.., RPT = 1>, rows staged 16 bytes a load."""
    d = _vector_width("score", kind, 1)
    assert ext().score_deep_cfg(kind, d)[0] == 1
    _check(dev, "score", ("built", d), kind, N_ROWS)


@pytest.mark.parametrize("layout", ["packed", "offset", "feature"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("route", WALKS)
def test_staging_branches(dev, route, kind, layout):
    """Rows of a whole number of 16-byte pieces at two rows a thread. Packed,
    stage_tile reads them 128 bits a load; one element off in a buffer one
    column wider (base not on 16 bytes, odd pitch) and feature-major it must
    fall back to element loads. All three give the oracle's bits."""
    d = _vector_width(route, kind, 2)
    name = ("built", d)
    forest, Xk, want = _case(route, name, kind, N_ROWS)
    n = Xk.shape[0]
    if layout == "packed":
        X = Xk.to(dev)
        assert X.is_contiguous() and X.data_ptr() % 16 == 0
    elif layout == "offset":
        X = torch.zeros((n, d + 1), dtype=Xk.dtype, device=dev)[:, 1:]
        X.copy_(Xk)
        assert X.data_ptr() % 16 != 0 and X.stride() == (d + 1, 1)
    else:
        X = torch.zeros((d, n + 5), dtype=Xk.dtype, device=dev)[:, :n].T
        X.copy_(Xk)
        assert X.stride() == (1, n + 5)
    _, got = _run(dev, route, forest, X)
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))


def test_shap_rows_of_4094_columns(dev):
    """The shap kernel keys rows from global memory at any width."""
    assert ext().shap_deep_cfg("f32", 4094, 8)[2] is False
    _check(dev, "shap", ("ragged",), "f32", N_SHAP, 4094)


# ---------------------------------------------------------------------------
# row counts and the grid stride
# ---------------------------------------------------------------------------

MAX_BLOCKS = {"score": "IFA_SCORE_DEEP_MAX_BLOCKS",
              "score_eif": "IFA_SCORE_DEEP_MAX_BLOCKS",
              "explain": "IFA_EXPLAIN_MAX_BLOCKS",
              "explain_eif": "IFA_EXPLAIN_MAX_BLOCKS"}


@pytest.mark.parametrize("route", WALKS)
def test_row_counts_and_grid_stride(dev, monkeypatch, route):
    """1 row, one below, exactly and one past a block's tile; then two tiles
    and a row on ONE block, which stages, walks and stores three times."""
    kind, d = "bf16", 6
    tile = 256 * _cfg(route, kind, d)[0]
    assert tile == 512
    forest, Xk, want = _case(route, ("built", d), kind, 2 * tile + 1)
    shell = Shell(forest)
    for n in (1, tile - 1, tile, tile + 1):
        _, got = _run(dev, route, forest, Xk[:n], shell)
        np.testing.assert_array_equal(_bits(got), want[:n].view(np.int32))
    monkeypatch.setenv(MAX_BLOCKS[route], "1")
    _, got = _run(dev, route, forest, Xk, shell)
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))


# ---------------------------------------------------------------------------
# knife rows and foreign splits
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", [("built", 6), ("foreign", "built", 6),
                                  ("foreign", "ragged")])
@pytest.mark.parametrize("route", ["score", "explain", "shap"])
def test_knife_rows_and_foreign_splits(dev, route, name, kind):
    """Cells on and beside the thresholds of the built forest, and of copies
    whose float64 splits lie strictly between two f32 values: the key of the
    smallest f32 at or above the split has to decide them."""
    _check(dev, route, name, kind, N_SHAP if route == "shap" else N_ROWS)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("route", ["score_eif", "explain_eif"])
def test_knife_rows_extended(dev, route, kind):
    """Non-finite cells included: both routes read every stored coordinate,
    as the oracle does."""
    _check(dev, route, ("built", 6), kind, N_ROWS)
