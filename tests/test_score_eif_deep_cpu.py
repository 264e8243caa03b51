"""Host half of the eif deep pack (gpu_engine._nodes_eif_deep_host) on a
64-row-bag extended forest: trimmed arrays, offset bits for internal nodes,
f32(depth) + f32(value) bits for leaves."""

import numpy as np

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.ops import gpu_engine


def test_nodes_eif_deep_host():
    d, T, n = 5, 3, 64
    X = np.random.RandomState(2).standard_normal((500, d)).astype(np.float32)
    bag = cpu_engine.sample_bags(500, T, n, seed=4, bootstrap=False)
    fs = cpu_engine.feature_subsets(d, d, T, seed=4)
    forest = cpu_engine.build_extended_forest(X, bag, fs, 4, n, d, d, 2)
    feat, right, vw, nc, hidx, hw, height = gpu_engine._nodes_eif_deep_host(
        forest)
    m0 = int(forest.node_count.max())
    assert m0 < forest.feature.shape[1]
    assert feat.shape == right.shape == vw.shape == (T, m0)
    assert hidx.shape == hw.shape == (T, m0, forest.nnz) and forest.nnz == 3
    np.testing.assert_array_equal(nc, forest.node_count)
    internal = forest.feature[:, :m0] >= 0
    leaf = forest.feature[:, :m0] == forest.LEAF
    assert internal.any() and (feat[internal] == forest.nnz).all()
    assert (feat[~internal] == -1).all()
    value = forest.value[:, :m0]
    np.testing.assert_array_equal(
        vw[internal], value[internal].astype(np.float32).view(np.int32))
    depth = gpu_engine._node_depths(forest.feature[:, :m0],
                                    forest.right[:, :m0])
    want = depth.astype(np.float32) + value.astype(np.float32)
    np.testing.assert_array_equal(vw[leaf], want[leaf].view(np.int32))
    assert height == depth[leaf].max()
    np.testing.assert_array_equal(hidx, forest.hyper_idx[:, :m0])
    np.testing.assert_array_equal(
        hw, forest.hyper_w[:, :m0].astype(np.float32).view(np.int32))
