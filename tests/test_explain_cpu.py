"""Per-feature attribution, CPU oracle and public API (no GPU).

The contract under test is docs/DESIGN.md §8: a path-length decomposition
whose row sums, plus the model's expected path length, reproduce the mean
path length, with NEGATIVE values marking features that made a row more
anomalous.

Identity bound: |bias + sum_f contrib - path_sum/T| <= 152*T*2^-24. A tree
is at most 19 levels deep (leaf term included), so a row sees at most
8*19*T float32 adds (contribution adds, the path-sum adds and the two
finalising divides folded in generously), each with relative error 2^-24
on partial sums bounded by 19*T, divided by T. At T=64 that is 5.8e-4.
"""

import os

import numpy as np
import pytest
import torch

from isolation_forest_amd import (
    ExtendedIsolationForest,
    ExtendedIsolationForestModel,
    IsolationForest,
    IsolationForestModel,
)
from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.core import forest as fmod
from isolation_forest_amd.utils.math import avg_path_length
from isolation_forest_amd.utils.params import Params
from tests.conftest import GOLDEN


def identity_bound(T):
    return 152.0 * T * 2.0 ** -24


def identity_gap(model, X, path_sum):
    """max_i |bias + sum_f contrib[i, f] - path_sum[i]/T| in float64."""
    contrib = model.feature_contributions(torch.from_numpy(X)).numpy()
    assert contrib.dtype == np.float32 and contrib.shape == X.shape
    T = model.forest.num_trees
    lhs = model.expected_path_length + contrib.astype(np.float64).sum(axis=1)
    return float(np.abs(lhs - path_sum.astype(np.float64) / T).max())


@pytest.fixture(scope="module")
def gauss5():
    return np.random.RandomState(11).normal(size=(2000, 5)).astype(np.float32)


@pytest.fixture(scope="module")
def std_model(gauss5):
    return IsolationForest(numEstimators=64, randomSeed=5).fit(gauss5)


def _hand_tree():
    """root(f0 < 0.5) -> leaf(n=3) | node(f1 < 2.0) -> leaf(n=1) | leaf(n=4)"""
    f = fmod.empty_forest(1, 5, num_samples=8, num_features=2,
                          total_num_features=2)
    f.feature[0] = [0, -1, 1, -1, -1]
    f.value[0] = [0.5, 0, 2.0, 0, 0]
    f.value64[0] = [0.5, 0, 2.0, 0, 0]
    f.right[0] = [2, -1, 4, -1, -1]
    f.num_instances[0] = [-1, 3, -1, 1, 4]
    f.node_count[0] = 5
    f.leaf_values_from_counts()
    return f


class TestNodeExpectations:
    def test_hand_built_tree(self):
        f = _hand_tree()
        E, n = cpu_engine.node_expectations(f)
        c3 = float(np.float32(1.0) + np.float32(avg_path_length(3)))
        c1 = float(np.float32(2.0) + np.float32(avg_path_length(1)))
        c4 = float(np.float32(2.0) + np.float32(avg_path_length(4)))
        e2 = (1 * c1 + 4 * c4) / 5
        e0 = (3 * c3 + 5 * e2) / 8
        np.testing.assert_array_equal(n[0], [8, 3, 5, 1, 4])
        np.testing.assert_allclose(E[0], [e0, c3, e2, c1, c4], rtol=1e-15)
        assert c1 == 2.0  # c(1) = 0: a singleton leaf costs its depth only
        tabs = cpu_engine.explain_tables(f)
        assert tabs["bias"] == np.float32(e0)
        np.testing.assert_array_equal(
            tabs["dl"][0], np.float32([c3 - e0, 0, c1 - e2, 0, 0]))
        np.testing.assert_array_equal(
            tabs["dr"][0], np.float32([e2 - e0, 0, c4 - e2, 0, 0]))

    def test_hand_built_tree_rows(self):
        f = _hand_tree()
        tabs = cpu_engine.explain_tables(f)
        X = np.float32([[0.0, 9.0], [1.0, 1.0], [1.0, 3.0]])
        got = cpu_engine.feature_contributions(f, X)
        dl, dr = tabs["dl"][0], tabs["dr"][0]
        want = np.float32([[dl[0], 0], [dr[0], dl[2]], [dr[0], dr[2]]])
        np.testing.assert_array_equal(got, want)
        ps = cpu_engine.path_lengths(f, X)
        np.testing.assert_allclose(
            float(tabs["bias"]) + got.astype(np.float64).sum(1), ps,
            atol=identity_bound(1))

    def test_cached_tables_follow_leaf_recount(self):
        f = _hand_tree()
        before = cpu_engine.explain_tables(f)
        assert cpu_engine.explain_tables(f) is before  # cached
        f.num_instances[0] = [-1, 1, -1, 6, 1]
        f.leaf_values_from_counts()  # drops the derived tables
        after = cpu_engine.explain_tables(f)
        E, _ = cpu_engine.node_expectations(f)
        assert after["bias"] == np.float32(E[0, 0]) != before["bias"]
        f.num_instances[0, 1] = 2  # any other in-place edit: explicit drop
        f.invalidate_derived()
        assert cpu_engine.explain_tables(f)["bias"] != after["bias"]

    def test_zero_instance_children_average(self):
        f = _hand_tree()
        f.num_instances[0] = [-1, 3, -1, 0, 0]
        f.leaf_values_from_counts()
        E, n = cpu_engine.node_expectations(f)
        assert n[0, 2] == 0 and n[0, 0] == 3
        assert E[0, 2] == (E[0, 3] + E[0, 4]) / 2
        assert E[0, 0] == E[0, 1]  # the empty side carries no weight


class TestIdentity:
    def test_standard(self, std_model, gauss5):
        ps = cpu_engine.path_lengths(std_model.forest, gauss5)
        gap = identity_gap(std_model, gauss5, ps)
        print(f"standard identity gap {gap:.3e}")
        assert gap <= identity_bound(64)

    @pytest.mark.parametrize("level", [0, 4])
    def test_extended(self, gauss5, level):
        model = ExtendedIsolationForest(
            numEstimators=64, randomSeed=5, extensionLevel=level).fit(gauss5)
        assert model.forest.nnz == level + 1
        ps = cpu_engine.path_lengths_extended(model.forest, gauss5)
        gap = identity_gap(model, gauss5, ps)
        print(f"EIF level {level} identity gap {gap:.3e}")
        assert gap <= identity_bound(64)

    def test_extended_shares_follow_squared_weights(self, gauss5):
        model = ExtendedIsolationForest(
            numEstimators=4, randomSeed=2, extensionLevel=4).fit(gauss5)
        fr = model.forest
        tabs = cpu_engine.explain_tables(fr)
        E, _ = cpu_engine.node_expectations(fr)
        t, v = 0, 0
        assert fr.feature[t, v] == 5
        w = fr.hyper_w[t, v].astype(np.float64)
        share = w * w / (w * w).sum()
        np.testing.assert_allclose(
            tabs["dl"][t, v], (E[t, 1] - E[t, 0]) * share, rtol=1e-6)
        np.testing.assert_allclose(
            tabs["dr"][t, v],
            (E[t, fr.right[t, v]] - E[t, 0]) * share, rtol=1e-6)


class TestPlantedOutliers:
    def test_planted_feature_is_most_negative(self):
        rs = np.random.RandomState(3)
        X = rs.normal(size=(2000, 5)).astype(np.float32)
        X[:40] *= np.float32(0.3)
        planted = rs.randint(0, 5, size=40)
        X[np.arange(40), planted] = 8.0
        model = IsolationForest(numEstimators=64, randomSeed=5).fit(X)
        contrib = model.feature_contributions(torch.from_numpy(X[:40])).numpy()
        hits = int((contrib.argmin(axis=1) == planted).sum())
        print(f"planted outliers recovered: {hits}/40")
        np.testing.assert_array_equal(contrib.argmin(axis=1), planted)
        # sign convention: the planted feature shortened the path
        assert (contrib[np.arange(40), planted] < 0).all()


class TestGoldenSparkModels:
    @pytest.mark.parametrize("name,cls,walk", [
        ("savedIsolationForestModel", IsolationForestModel,
         cpu_engine.path_lengths),
        ("savedExtendedIsolationForestModel", ExtendedIsolationForestModel,
         cpu_engine.path_lengths_extended),
    ])
    def test_finite_identity_and_roundtrip(self, name, cls, walk, mammography,
                                           tmp_path):
        model = cls.load(os.path.join(GOLDEN, name))
        X = np.ascontiguousarray(mammography[0][:500])
        contrib = model.feature_contributions(torch.from_numpy(X)).numpy()
        assert np.isfinite(contrib).all()
        T = model.forest.num_trees
        gap = identity_gap(model, X, walk(model.forest, X))
        print(f"{name}: identity gap {gap:.3e} (T={T})")
        assert gap <= identity_bound(T)
        p = str(tmp_path / "again")
        model.save(p)
        again = cls.load(p)
        assert again.expected_path_length == model.expected_path_length
        np.testing.assert_array_equal(
            again.feature_contributions(torch.from_numpy(X)).numpy(), contrib)


class TestApi:
    def test_finalize_false_returns_raw_sums(self, std_model, gauss5):
        X = torch.from_numpy(gauss5[:300])
        raw = std_model.feature_contributions(X, finalize=False).numpy()
        fin = std_model.feature_contributions(X).numpy()
        assert raw.dtype == np.float32
        np.testing.assert_array_equal(
            (raw / np.float32(64)).astype(np.float32), fin)
        assert np.abs(raw).max() > np.abs(fin).max()

    def test_input_kinds_match_score(self, std_model, gauss5):
        X = gauss5[:50]
        a = std_model.feature_contributions(X)  # numpy, like score()
        b = std_model.feature_contributions(torch.from_numpy(X))
        assert isinstance(a, torch.Tensor) and a.dtype == torch.float32
        assert torch.equal(a, b)
        xb = torch.from_numpy(X).to(torch.bfloat16)
        c = std_model.feature_contributions(xb)
        assert torch.equal(
            c, std_model.feature_contributions(xb.float()))

    def test_expected_path_length_is_cached_constant(self, std_model):
        E, _ = cpu_engine.node_expectations(std_model.forest)
        want = float(np.float32(E[:, 0].mean()))
        assert std_model.expected_path_length == want
        assert isinstance(std_model.expected_path_length, float)
        assert std_model.__dict__["_expected_path_length"] == want

    @pytest.mark.parametrize("k", [1, 3, 5])
    def test_top_contributing_features(self, std_model, gauss5, k):
        X = torch.from_numpy(gauss5[:400])
        contrib = std_model.feature_contributions(X).numpy()
        srt = np.sort(contrib, axis=1)
        assert (np.diff(srt, axis=1) > 0).all(), "input must be tie-free"
        idx, val = std_model.top_contributing_features(X, k)
        assert idx.dtype == torch.int64 and val.dtype == torch.float32
        assert tuple(idx.shape) == (400, k) == tuple(val.shape)
        order = np.argsort(contrib, axis=1)[:, :k]
        np.testing.assert_array_equal(idx.numpy(), order)
        np.testing.assert_array_equal(
            val.numpy(), np.take_along_axis(contrib, order, axis=1))

    def test_top_k_out_of_range(self, std_model, gauss5):
        X = torch.from_numpy(gauss5[:4])
        for k in (0, 6):
            with pytest.raises(ValueError, match="k must be"):
                std_model.top_contributing_features(X, k)

    def test_width_mismatch_raises_like_score(self, std_model, gauss5):
        bad = torch.from_numpy(gauss5[:4, :3].copy())
        with pytest.raises(ValueError) as e_score:
            std_model.score(bad)
        with pytest.raises(ValueError) as e_explain:
            std_model.feature_contributions(bad)
        assert str(e_explain.value) == str(e_score.value)
        ext = ExtendedIsolationForest(numEstimators=4, randomSeed=1).fit(gauss5)
        with pytest.raises(ValueError, match="does not match"):
            ext.feature_contributions(bad)

    @pytest.mark.parametrize("extended", [False, True])
    def test_empty_forest_raises_like_score(self, extended):
        if extended:
            from isolation_forest_amd.utils.params import ExtendedParams

            forest = fmod.empty_extended_forest(0, 1, 1, 256, 4, 4, 0)
            model = ExtendedIsolationForestModel(
                uid="empty", forest=forest, params=ExtendedParams())
        else:
            forest = fmod.empty_forest(0, 1, num_samples=256, num_features=4,
                                       total_num_features=4)
            model = IsolationForestModel(uid="empty", forest=forest,
                                         params=Params())
        X = torch.zeros((5, 4))
        with pytest.raises(ValueError, match="no trees"):
            model.score(X)
        with pytest.raises(ValueError, match="no trees"):
            model.feature_contributions(X)
        with pytest.raises(ValueError, match="no trees"):
            model.expected_path_length
