"""The forests and rows of tests/deep_shapes.py, checked without a GPU.

tests/test_deep_shapes_gpu.py runs them through the deep routes and compares
with the CPU oracle bit for bit. A case is only worth its GPU time while it
still reaches what it was made for: a link at the 20-bit cap, a barrier
phase that mixes a single leaf with thousands of nodes, a cell that sits on
a threshold of its own walk. Those are properties of the oracle's walk, so
they are asserted here, on the oracle alone: a case that stops reaching its
mechanism fails in this file instead of passing silently on the GPU.
"""

import numpy as np
import pytest

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.core.forest import ExtendedForest
from isolation_forest_amd.ops import gpu_engine
from tests import deep_shapes as S

N_KNIFE = 1025  # the most rows the GPU tests take of a knife set


def _ragged(extended):
    return S.ragged(S.built(S.SPINE_FEATURES, extended), extended)


def _leaf_of(forest, X, t):
    paths = S.walk(forest, X, t)
    last = (paths >= 0).sum(axis=1) - 1
    return paths[np.arange(len(X)), last]


@pytest.mark.parametrize("extended", [False, True])
def test_trie_reaches_the_link_cap(extended):
    n = 2 ** 20 - 1
    forest = S.trie(19, 6, extended)
    assert int(forest.node_count[0]) == n == forest.feature.shape[1]
    assert n <= gpu_engine.DEEP_MAX_NODES < n + 2
    assert not gpu_engine._packed_fits(forest, 6)
    X = S.widen(S.trie_rows("bf16", 6))
    ends = _leaf_of(forest, X, 0)
    assert ends[0] == n - 1  # all-high: the last pre-order node
    assert ends[1] == 19     # all-low: the leftmost leaf
    assert len(np.unique(ends)) >= 1000
    score = (cpu_engine.path_lengths_extended if extended
             else cpu_engine.path_lengths)
    assert len(np.unique(score(forest, X))) > 100


def test_trie_twin_walks_like_the_trie():
    X = S.widen(S.trie_rows("f32", 6))
    assert np.array_equal(S.walk(S.trie(12, 6), X, 0),
                          S.walk(S.trie(12, 6, True), X, 0))


@pytest.mark.parametrize("extended", [False, True])
def test_ragged_mixes_every_phase(extended):
    forest = _ragged(extended)
    assert forest.num_trees == 9 and forest.feature.shape[1] > 32767
    nc = forest.node_count
    for phase in (nc[0:4], nc[4:8]):
        assert phase.min() == 1 and phase.max() > 3000
    assert nc[8] > 3000  # shares its phase with three pad trees
    assert sorted(nc[[0, 2, 4, 5, 7]]) == [1, 1, 3, 81, 81]
    depth = gpu_engine._node_depths(forest.feature, forest.right)
    assert depth[forest.feature >= -1].max() >= S.SPINE_DEPTH
    if not extended:
        assert (cpu_engine.shap_tables(forest)["max_m"]
                <= cpu_engine.SHAP_DEEP_MAX_PATH_FEATURES)
    # rows walk both spines to the end
    X = S.widen(S.knife_rows(forest, "f32", N_KNIFE)[0])
    assert (_leaf_of(forest, X, 2) == 2 * S.SPINE_DEPTH).any()
    assert (_leaf_of(forest, X, 5) == S.SPINE_DEPTH).any()


def test_sliced_keeps_the_first_trees():
    forest = _ragged(False)
    for T in (1, 4, 8):
        part = S.sliced(forest, T)
        assert part.num_trees == T
        assert part.feature.shape[1] == forest.feature.shape[1]
        X = S.widen(S.knife_rows(forest, "f32", 64)[0])
        assert np.array_equal(cpu_engine.path_lengths(part, X),
                              cpu_engine.path_lengths(S.sliced(part, T), X))
    assert int(S.sliced(forest, 1).node_count.max()) == 1


def _knife_visits(forest, kind, n=N_KNIFE):
    """(equal, below, above): the planted (row, node) visits of the oracle's
    walk whose cell is the node's f32 threshold, the value of the kind next
    below it, next above it."""
    Xk, planted = S.knife_rows(forest, kind, n)
    X = S.widen(Xk)
    thr = gpu_engine._split_thresholds32(forest)
    paths = {t: S.walk(forest, X, t) for t in range(forest.num_trees)}
    equal = below = above = 0
    for row, t, v, c in planted:
        assert v in paths[t][row], "the planted row no longer reaches its node"
        assert S.split_cell(forest, t, v) == c
        x, s = X[row, c], thr[t, v]
        equal += x == s
        below += x < s and S.step_kind(x, kind, up=True)[0] >= s
        above += x > s and S.step_kind(x, kind, up=False)[0] <= s
    return int(equal), int(below), int(above)


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("kind", list(S.KINDS))
def test_knife_rows_sit_on_thresholds_of_their_walk(kind, extended):
    """The hand-made trees split on sixteenths and dyadic midpoints, exact in
    every row kind, so rows of every kind hit them."""
    equal, below, above = _knife_visits(_ragged(extended), kind)
    assert min(equal, below, above) >= 50, (equal, below, above)


@pytest.mark.parametrize("kind", list(S.KINDS))
def test_knife_rows_on_the_built_forest(kind):
    """Built thresholds are arbitrary f32 values: f32 rows hit them, 16-bit
    rows land one step of their own type to either side."""
    equal, below, above = _knife_visits(S.built(6), kind)
    assert min(below, above) >= 50, (equal, below, above)
    if kind == "f32":
        assert equal >= 50
    else:
        assert equal == 0


@pytest.mark.parametrize("kind", list(S.KINDS))
def test_knife_rows_carry_the_special_cells(kind):
    X = S.widen(S.knife_rows(_ragged(False), kind, N_KNIFE)[0])
    bits = set(X.view(np.uint32).ravel().tolist())
    cells = S.special_cells(kind)
    finite = cells[~np.isnan(cells)]
    assert set(finite.view(np.uint32).tolist()) <= bits
    assert np.isnan(X).any()
    tiny = finite[(finite != 0) & (np.abs(finite) < 2.0 ** -14)]
    assert len(tiny) == 4  # denormals of the kind


@pytest.mark.parametrize("which,kinds", [("built", ["f32"]),
                                         ("ragged", list(S.KINDS))])
def test_foreign_splits_move_a_walk(which, kinds):
    forest = S.built(6) if which == "built" else _ragged(False)
    foreign = S.foreign64(forest)
    assert np.array_equal(foreign.value, forest.value)
    lifted = gpu_engine._split_thresholds32(foreign) != forest.value
    assert 0.4 < lifted[forest.feature >= 0].mean() < 0.6
    for kind in kinds:
        X = S.widen(S.knife_rows(forest, kind, N_KNIFE)[0])
        assert not np.array_equal(cpu_engine.path_lengths(forest, X),
                                  cpu_engine.path_lengths(foreign, X))


def test_one_node_past_the_cap_does_not_fit():
    forest = S.sliced(_ragged(False), 1)
    forest.node_count[:] = (1 << 20) + 1
    assert not gpu_engine._deep_fits(forest, S.SPINE_FEATURES)
    assert not isinstance(forest, ExtendedForest)
