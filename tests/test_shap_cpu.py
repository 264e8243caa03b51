"""Exact TreeSHAP on the CPU oracle (docs/DESIGN.md §9).

cpu_engine.shap_values computes the leaf-path form; this file checks it
against the DEFINITION: the value function v_t(S) is evaluated by descending
the trees, and the Shapley values are enumerated over every feature subset.
The brute force shares nothing with the oracle but node_expectations' cover
counts, which the contract names as the weights.

Gate for the float64 comparisons: 1e-9. For the shapes here that is the
worst-case float64 rounding bound — about 7e4 operations x 2^-53 x a leaf
value of at most about 30; the differences measured are around 1e-15.
"""

import itertools
import math

import numpy as np
import pytest
import torch

from isolation_forest_amd import ExtendedIsolationForest, IsolationForest
from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.core.forest import Forest
from isolation_forest_amd.utils.math import avg_path_length

GATE = 1e-9

# (N, d, maxSamples, T) of the three reference shapes
SHAPES = [(200, 4, 16, 3), (300, 6, 32, 2), (300, 3, 64, 2)]


def gauss(N, d, seed):
    return np.random.RandomState(seed).normal(size=(N, d)).astype(np.float32)


_MODELS = {}


def fitted(N, d, max_samples, T, seed=0, transform=None):
    key = (N, d, max_samples, T, seed, transform)
    if key not in _MODELS:
        X = gauss(N, d, seed=50 + seed + d)
        if transform == "round0":
            X[:, 0] = np.round(X[:, 0] * 2.0)
        elif transform == "const1":
            X[:, 1] = np.float32(0.25)
        model = IsolationForest(numEstimators=T, maxSamples=float(max_samples),
                                randomSeed=11 + seed).fit(X)
        _MODELS[key] = (model, X)
    return _MODELS[key]


def nonfinite_rows(d, seed=5):
    """Rows with NaN, +inf and -inf cells (shared with the GPU test)."""
    X = gauss(12, d, seed)
    specials = [np.nan, np.inf, -np.inf]
    for i in range(9):
        X[i, i % d] = specials[i % 3]
    X[9, :] = np.nan
    X[10, :] = np.inf
    X[11, :] = -np.inf
    return X


# -- the definition ---------------------------------------------------------


def leaf_value(forest, t, v, depth):
    """L = f64(f32(depth) + f32(value)), the depth counted by the caller's
    own walk."""
    return float(np.float64(np.float32(depth)
                            + np.float32(forest.value[t, v])))


def tree_value(forest, n, t, x, S):
    """v_t(S) for one row by descending tree t."""
    feat, right = forest.feature[t], forest.right[t]
    v64 = forest.value64[t]

    def rec(v, depth):
        f = int(feat[v])
        if f < 0:
            return leaf_value(forest, t, v, depth)
        l, r = v + 1, int(right[v])
        if f in S:
            return (rec(l, depth + 1) if np.float64(x[f]) < v64[v]
                    else rec(r, depth + 1))
        nv = int(n[t, v])
        wl, wr = ((int(n[t, l]) / nv, int(n[t, r]) / nv) if nv > 0
                  else (0.5, 0.5))
        return wl * rec(l, depth + 1) + wr * rec(r, depth + 1)

    return rec(0, 0)


def brute_force_shap(forest, X):
    """float64 [N, d] Shapley values of sum_t v_t by subset enumeration."""
    _, n = cpu_engine.node_expectations(forest)
    N, d = X.shape
    phi = np.zeros((N, d), dtype=np.float64)
    subsets = [frozenset(c) for k in range(d + 1)
               for c in itertools.combinations(range(d), k)]
    for r in range(N):
        v = {S: sum(tree_value(forest, n, t, X[r], S)
                    for t in range(forest.num_trees)) for S in subsets}
        for i in range(d):
            for S in subsets:
                if i in S:
                    continue
                w = (math.factorial(len(S)) * math.factorial(d - len(S) - 1)
                     / math.factorial(d))
                phi[r, i] += w * (v[S | {i}] - v[S])
    return phi


def own_path_sum(forest, x):
    """float64 sum over trees of the row's f32 leaf value, walked here."""
    total = 0.0
    for t in range(forest.num_trees):
        v, depth = 0, 0
        while forest.feature[t, v] >= 0:
            f = int(forest.feature[t, v])
            v = (v + 1 if np.float64(x[f]) < forest.value64[t, v]
                 else int(forest.right[t, v]))
            depth += 1
        total += leaf_value(forest, t, v, depth)
    return total


def check_against_definition(forest, rows):
    got = cpu_engine.shap_raw_sums(forest, rows)
    want = brute_force_shap(forest, rows)
    diff = float(np.abs(got - want).max())
    print(f"max |oracle - brute force| = {diff:.3e}")
    assert diff <= GATE
    return got


# -- tests ------------------------------------------------------------------


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_subset_enumeration(shape):
    N, d, ms, T = shape
    model, X = fitted(N, d, ms, T)
    check_against_definition(model.forest, X[:6])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_additivity(shape):
    N, d, ms, T = shape
    model, X = fitted(N, d, ms, T)
    rows = X[:6]
    acc = cpu_engine.shap_raw_sums(model.forest, rows)
    E, _ = cpu_engine.node_expectations(model.forest)
    for r in range(len(rows)):
        lhs = float(E[:, 0].sum()) + float(acc[r].sum())
        gap = abs(lhs - own_path_sum(model.forest, rows[r]))
        print(f"row {r}: additivity gap {gap:.3e}")
        assert gap <= GATE
    # the bias is the existing expected_path_length, unchanged
    assert model.expected_path_length == float(np.float32(E[:, 0].mean()))


def test_single_feature_gets_everything():
    # d = 1: m = 1 on every path, every node on the same feature
    model, X = fitted(200, 1, 16, 3)
    rows = X[:8]
    acc = cpu_engine.shap_raw_sums(model.forest, rows)
    E, _ = cpu_engine.node_expectations(model.forest)
    for r in range(len(rows)):
        want = own_path_sum(model.forest, rows[r]) - float(E[:, 0].sum())
        assert abs(acc[r, 0] - want) <= GATE
    check_against_definition(model.forest, rows[:3])


def test_constant_column_is_exactly_zero():
    model, X = fitted(200, 4, 16, 3, transform="const1")
    assert not (model.forest.feature == 1).any()  # never split
    got = cpu_engine.shap_values(model.forest, X[:40])
    assert (got[:, 1].view(np.int32) == 0).all()  # +0.0, bit for bit
    assert np.abs(got[:, [0, 2, 3]]).max() > 0


def test_ties_and_repeated_features_on_a_path():
    model, X = fitted(300, 3, 64, 2, transform="round0")
    tabs = cpu_engine.shap_tables(model.forest)
    # repeated features: some entry merges more than one node
    assert np.diff(tabs["ent_pn_off"]).max() > 1
    rows = X[:6].copy()
    # rows sitting exactly on split values of column 0
    f, v = model.forest.feature, model.forest.value
    rows[:3, 0] = v[f == 0][:3]
    check_against_definition(model.forest, rows)


def test_nonfinite_cells_follow_the_engine_compare():
    model, _ = fitted(300, 6, 32, 2)
    rows = nonfinite_rows(6)
    acc = check_against_definition(model.forest, rows)  # all 12
    assert np.isfinite(acc).all()
    # NaN goes right at every split, as in path_lengths
    E, _ = cpu_engine.node_expectations(model.forest)
    ps = cpu_engine.path_lengths(model.forest, rows).astype(np.float64)
    lhs = float(E[:, 0].sum()) + acc.sum(axis=1)
    # path_lengths accumulates in float32: 2 trees x leaf values below 16
    assert np.abs(lhs - ps).max() <= 2 * 16 * 2.0 ** -24


def test_finalize():
    model, X = fitted(200, 4, 16, 3)
    rows = X[:20]
    acc = cpu_engine.shap_raw_sums(model.forest, rows)
    raw = cpu_engine.shap_values(model.forest, rows, finalize=False)
    fin = cpu_engine.shap_values(model.forest, rows, finalize=True)
    assert raw.dtype == np.float32 and fin.dtype == np.float32
    assert np.array_equal(raw, acc.astype(np.float32))
    assert np.array_equal(fin, (acc / np.float64(3)).astype(np.float32))


def test_invalidate_derived_drops_the_tables():
    model, X = fitted(200, 4, 16, 3, seed=1)
    forest = model.forest
    tabs = cpu_engine.shap_tables(forest)
    assert cpu_engine.shap_tables(forest) is tabs  # cached
    forest.invalidate_derived()
    assert "_shap_tables" not in forest.__dict__
    again = cpu_engine.shap_tables(forest)
    assert again is not tabs
    assert np.array_equal(again["ent_z"], tabs["ent_z"])


def test_leaves_are_tabulated_in_ascending_node_id():
    model, _ = fitted(300, 6, 32, 2)
    tabs = cpu_engine.shap_tables(model.forest)
    off = tabs["tree_leaf_off"]
    for t in range(model.forest.num_trees):
        ids = tabs["leaf_node"][off[t]:off[t + 1]]
        assert (np.diff(ids) > 0).all()
        assert np.array_equal(
            ids, np.nonzero(model.forest.feature[t] == Forest.LEAF)[0])


def test_model_interface():
    model, X = fitted(200, 4, 16, 3)
    rows = torch.from_numpy(X[:10])
    want = cpu_engine.shap_values(model.forest, X[:10])
    got = model.feature_contributions(rows, method="shap")
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    assert torch.equal(model.shap_values(rows), got)
    raw = model.feature_contributions(rows, finalize=False, method="shap")
    assert np.array_equal(
        raw.numpy(), cpu_engine.shap_values(model.forest, X[:10], False))
    with pytest.raises(ValueError, match="bogus"):
        model.feature_contributions(rows, method="bogus")
    with pytest.raises(ValueError, match="bogus"):
        model.top_contributing_features(rows, 2, method="bogus")
    # the default method is what it was, bit for bit
    path = cpu_engine.feature_contributions(model.forest, X[:10])
    for out in (model.feature_contributions(rows),
                model.feature_contributions(rows, method="path")):
        assert np.array_equal(out.numpy().view(np.int32), path.view(np.int32))
    idx, val = model.top_contributing_features(rows, 2, method="shap")
    order = np.argsort(want, axis=1, kind="stable")[:, :2]
    assert np.array_equal(val.numpy(),
                          np.take_along_axis(want, order, axis=1))


def test_extended_model_raises_with_the_reason():
    X = gauss(200, 4, seed=3)
    eif = ExtendedIsolationForest(numEstimators=3, maxSamples=16.0,
                                  randomSeed=2).fit(X)
    with pytest.raises(ValueError, match="hyperplane"):
        eif.feature_contributions(torch.from_numpy(X[:4]), method="shap")
    with pytest.raises(ValueError, match="hyperplane"):
        eif.shap_values(torch.from_numpy(X[:4]))
    # its default method still works
    assert tuple(eif.feature_contributions(
        torch.from_numpy(X[:4])).shape) == (4, 4)


def test_feature_off_the_rows_own_path_gets_credit():
    """The point of the feature. One tree:

        0: x0 < 0 ? -> 1 : 2        1: leaf, 4 rows, depth 1
        2: x1 < 0 ? -> 3 : 4        3: leaf, 1 row;  4: leaf, 3 rows

    The row (-1, -1) stops at node 1 and never meets the split on x1, so
    "path" gives x1 nothing. Its Shapley value is not 0: were x0 unknown,
    knowing x1 would move the expectation below node 2 from
    L3/4 + 3 L4/4 to L3. phi_1 = 1/2 * [v({1}) - v({})] + 1/2 * 0
          = 1/2 * 1/2 * (L3 - (L3 + 3 L4)/4) = 3/16 * (L3 - L4)."""
    c = lambda m: np.float32(avg_path_length(m))  # noqa: E731
    feature = np.array([[0, -1, 1, -1, -1]], dtype=np.int32)
    value = np.array([[0.0, c(4), 0.0, c(1), c(3)]], dtype=np.float32)
    forest = Forest(
        feature=feature, value=value,
        right=np.array([[2, -1, 4, -1, -1]], dtype=np.int32),
        num_instances=np.array([[-1, 4, -1, 1, 3]], dtype=np.int64),
        node_count=np.array([5], dtype=np.int32),
        num_samples=8, num_features=2, total_num_features=2,
        value64=np.where(feature >= 0, value, 0.0).astype(np.float64))
    row = np.array([[-1.0, -1.0]], dtype=np.float32)
    path = cpu_engine.feature_contributions(forest, row, finalize=False)
    assert path[0, 1] == 0.0 and path[0, 0] != 0.0
    acc = cpu_engine.shap_raw_sums(forest, row)
    L3 = float(np.float32(2.0) + c(1))
    L4 = float(np.float32(2.0) + c(3))
    want1 = 3.0 / 16.0 * (L3 - L4)
    assert abs(acc[0, 1] - want1) <= 1e-14
    assert acc[0, 1] < -0.2  # about -0.226: x1 < 0 isolates faster
    L1 = float(np.float32(1.0) + c(4))
    root = 0.5 * L1 + 0.5 * (0.25 * L3 + 0.75 * L4)
    assert abs(root + acc[0].sum() - L1) <= 1e-14
    shap = cpu_engine.shap_values(forest, row, finalize=False)
    assert shap[0, 1] == np.float32(acc[0, 1])
