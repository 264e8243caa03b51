"""CPU tests: the trimmed attribution tables and the host half of the
explain deep pack (ops/hip/deep_kernels.hip) against explain_tables and
_nodes_deep_host, bit for bit, on the forest of test_explain_deep_gpu.py."""

import functools

import numpy as np
import pytest

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.ops import gpu_engine

N_BAG, D, T = 16385, 6, 5


@functools.lru_cache(maxsize=None)
def _forest():
    X = np.random.RandomState(5).standard_normal((20000, D)).astype(np.float32)
    bag = cpu_engine.sample_bags(20000, T, N_BAG, seed=31, bootstrap=False)
    fs = cpu_engine.feature_subsets(D, D, T, seed=31)
    return cpu_engine.build_forest(X, bag, fs, 31, N_BAG, D, D)


def test_trimmed_tables_are_the_first_columns():
    forest = _forest()
    m = int(forest.node_count.max())
    assert m < forest.feature.shape[1]
    full = cpu_engine.explain_tables(forest)
    trim = cpu_engine.explain_tables_trimmed(forest)
    for k in ("dl", "dr"):
        assert trim[k].dtype == np.float32 and trim[k].shape == (T, m)
        np.testing.assert_array_equal(trim[k].view(np.int32),
                                      full[k][:, :m].view(np.int32))
    assert trim["bias"].dtype == np.float32
    assert trim["bias"].tobytes() == full["bias"].tobytes()


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_host_half_of_the_pack(kind):
    forest = _forest()
    feat, right, w, dl, dr, nc, height = gpu_engine._nodes_explain_deep_host(
        forest, kind)
    for got, want in zip((feat, right, w, nc, height),
                         gpu_engine._nodes_deep_host(forest, kind)):
        np.testing.assert_array_equal(got, want)
    full = cpu_engine.explain_tables(forest)
    live = np.arange(feat.shape[1])[None, :] < nc[:, None]
    assert (feat[live] >= 0).any() and dl.dtype == dr.dtype == np.int32
    for got, k in ((dl, "dl"), (dr, "dr")):
        want = full[k][:, :feat.shape[1]].view(np.int32)
        np.testing.assert_array_equal(got[live], want[live])
