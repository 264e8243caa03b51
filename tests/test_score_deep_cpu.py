"""No GPU: which standard forests the deep scoring records can represent
(gpu_engine._deep_fits) and what their host half holds."""

import types

import numpy as np
import pytest

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.ops import gpu_engine


def _fabricated(node_count, feature_max=3):
    return types.SimpleNamespace(
        node_count=np.array([7, node_count], dtype=np.int32),
        feature=np.array([[feature_max, -1, -1]], dtype=np.int32))


@pytest.mark.parametrize("node_count,feature_max,d,fits", [
    (2 ** 20, 3, 6, True),
    (2 ** 20 + 1, 3, 6, False),   # links are 20 bits
    (40000, 4094, 4094, True),
    (40000, 4095, 4094, False),   # feature ids are 12 bits, d the sentinel
    (40000, 3, 4095, False),
])
def test_deep_fits(node_count, feature_max, d, fits):
    assert gpu_engine._deep_fits(_fabricated(node_count, feature_max), d) is fits
    assert gpu_engine.DEEP_MAX_NODES == 2 ** 20


def test_host_half_is_the_wide_pack_trimmed():
    X = np.random.RandomState(1).standard_normal((600, 4)).astype(np.float32)
    bag = cpu_engine.sample_bags(600, 3, 256, seed=2, bootstrap=False)
    fs = cpu_engine.feature_subsets(4, 4, 3, seed=2)
    forest = cpu_engine.build_forest(X, bag, fs, 2, 256, 4, 4)
    wide, height = gpu_engine._nodes_packed_wide(forest, "bf16")
    feat, right, w, nc, h = gpu_engine._nodes_deep_host(forest, "bf16")
    m0 = int(forest.node_count.max())
    assert feat.shape == (3, m0) and h == height
    live = np.arange(m0)[None, :] < nc[:, None]
    internal = live & (feat >= 0)
    for got, col in ((feat, 0), (right, 1), (w, 2)):
        keep = live if col == 2 else internal
        np.testing.assert_array_equal(got[keep], wide[:, :m0, col][keep])
