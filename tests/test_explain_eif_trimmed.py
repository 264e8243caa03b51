"""cpu_engine.explain_tables_trimmed on extended forests: the first
max(node_count) columns of explain_tables, bit for bit, at extension levels
0, 1 and d - 1; standard forests keep their 2-D tables."""

import numpy as np
import pytest

from isolation_forest_amd.core import cpu_engine

N, D, T, BAG = 400, 5, 4, 64


def _data():
    return np.random.RandomState(3).standard_normal((N, D)).astype(np.float32)


@pytest.mark.parametrize("level", [0, 1, D - 1])
def test_extended_tables_are_the_first_columns(level):
    bag = cpu_engine.sample_bags(N, T, BAG, seed=11, bootstrap=False)
    fs = cpu_engine.feature_subsets(D, D, T, seed=11)
    forest = cpu_engine.build_extended_forest(
        _data(), bag, fs, 11, BAG, D, D, level)
    m = int(forest.node_count.max())
    assert m < forest.feature.shape[1]  # arrays wider than the trees
    full = cpu_engine.explain_tables(forest)
    got = cpu_engine.explain_tables_trimmed(forest)
    assert got["dl"].shape == (T, m, forest.nnz)
    assert got["bias"].tobytes() == full["bias"].tobytes()
    for name in ("dl", "dr"):
        assert got[name].dtype == np.float32
        np.testing.assert_array_equal(
            got[name].view(np.int32), full[name][:, :m].view(np.int32))


def test_standard_tables_stay_two_dimensional():
    bag = cpu_engine.sample_bags(N, T, BAG, seed=11, bootstrap=False)
    fs = cpu_engine.feature_subsets(D, D, T, seed=11)
    forest = cpu_engine.build_forest(_data(), bag, fs, 11, BAG, D, D)
    m = int(forest.node_count.max())
    full = cpu_engine.explain_tables(forest)
    got = cpu_engine.explain_tables_trimmed(forest)
    for name in ("dl", "dr"):
        assert got[name].shape == (T, m)
        np.testing.assert_array_equal(
            got[name].view(np.int32), full[name][:, :m].view(np.int32))
