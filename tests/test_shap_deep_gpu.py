"""GPU tests (MI355X): TreeSHAP for standard forests past the 15-bit node ids
(shap_forest_deep_kernel, docs/DESIGN.md §9) against cpu_engine.shap_values,
bit for bit.

The large-bag forest is the one of tests/test_score_deep_gpu.py (n = 16385,
d = 6, T = 5, about ten thousand leaves, max_m = 6: 8 lanes a row, 32 rows
a block); 203 rows are six full tiles and a tail of 11. Hand-made chains in
arrays 32769 wide reach 16 and 32 lanes a row, merged and empty intervals,
and the 33-feature path the kernel does not hold.
"""

import functools
import logging

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd import IsolationForest  # noqa: E402
from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.core.forest import empty_forest  # noqa: E402
from isolation_forest_amd.ops import gpu_engine  # noqa: E402
from tests.test_score_deep_gpu import Shell, _forest  # noqa: E402

KINDS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
D, N_ROWS, MN = 6, 203, 32769


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


@functools.lru_cache(maxsize=None)
def _rows(kind, n=N_ROWS, d=D):
    """(rows of the kind on the host, the same values as f32 numpy)"""
    X = np.random.RandomState(6).standard_normal((n, d)).astype(np.float32)
    X[3, 1], X[n - 1, 0], X[n // 2, 5], X[20, 2] = np.nan, np.inf, -np.inf, 0.0
    Xk = torch.from_numpy(X).to(KINDS[kind])
    return Xk, Xk.float().numpy()


@functools.lru_cache(maxsize=None)
def _oracle(kind, finalize=True, d=D):
    return cpu_engine.shap_values(_forest("trees"), _rows(kind, d=d)[1],
                                  finalize)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _warned(caplog):
    return [r for r in caplog.records if "CPU oracle" in r.getMessage()]


@pytest.mark.parametrize("finalize", [True, False])
@pytest.mark.parametrize("kind", list(KINDS))
def test_bitwise_against_the_oracle(dev, caplog, kind, finalize):
    forest = _forest("trees")
    assert not gpu_engine._packed_fits(forest, D)
    assert gpu_engine.large_shap_route(forest, D, KINDS[kind]) == "deep"
    assert ext().shap_deep_cfg(kind, D, 6) == (8, True, True)
    with caplog.at_level(logging.WARNING):
        got = gpu_engine.shap_forest(Shell(forest), _rows(kind)[0].to(dev),
                                     finalize)
    assert not _warned(caplog)
    np.testing.assert_array_equal(
        _bits(got), _oracle(kind, finalize).view(np.int32))


@pytest.mark.parametrize("switch,value,warns", [
    ("IFA_SHAP_FORCE_GLOBAL_ACC", "1", False),
    ("IFA_SHAP_MAX_BLOCKS", "1", False),  # one block, seven row tiles
    ("IFA_SHAP_DEEP_SPLIT", "row", False),
    ("IFA_SHAP_DEEP", "0", True),
])
def test_switches(dev, monkeypatch, caplog, switch, value, warns):
    monkeypatch.setenv(switch, value)
    with caplog.at_level(logging.WARNING):
        got = gpu_engine.shap_forest(Shell(_forest("trees")),
                                     _rows("bf16")[0].to(dev), True)
    assert bool(_warned(caplog)) == warns
    np.testing.assert_array_equal(_bits(got), _oracle("bf16").view(np.int32))


def test_rows_too_wide_for_the_tiles(dev):
    d = 1200  # 32 rows of 1201 f32 keys and the weights pass 150 KB
    assert ext().shap_deep_cfg("f32", d, 6) == (8, False, False)
    assert ext().shap_deep_cfg("f32", d // 2, 6) == (8, False, True)
    got = gpu_engine.shap_forest(Shell(_forest("trees")),
                                 _rows("f32", d=d)[0].to(dev), True)
    np.testing.assert_array_equal(_bits(got),
                                  _oracle("f32", d=d).view(np.int32))


def chain(features, values):
    """Node 2i splits on features[i] at values[i]; its left child 2i + 1 is
    a leaf, its right child node 2i + 2. In arrays MN wide: the rest pads."""
    k = len(features)
    f = empty_forest(1, MN, k + 1, max(features) + 1, max(features) + 1)
    f.feature[0, 0:2 * k + 1] = f.LEAF
    f.feature[0, 0:2 * k:2] = features
    f.right[0, 0:2 * k:2] = np.arange(2, 2 * k + 2, 2)
    f.num_instances[0, 1:2 * k + 1:2] = 1
    f.num_instances[0, 2 * k] = 1
    f.value[0, 0:2 * k:2] = values
    f.value64[:] = f.value
    f.node_count[0] = 2 * k + 1
    return f


CHAINS = {  # name: (features, lanes a row or None for the CPU route)
    "12": (list(range(12)), 16),
    "17": (list(range(17)), 32),
    "32": (list(range(32)), 32),
    # feature 0 turns right at node 0 and left at node 4 (a merged
    # interval); feature 1 turns left at -inf, the smallest threshold key
    # (no row key is below it); feature 2 turns right at 0.3 and then left
    # at -0.2 (an empty interval)
    "revisit": ([0, 1, 0, 2, 1, 3, 2, 0], 8),
    "33": (list(range(33)), None),
}


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_chains(dev, caplog, name, kind):
    features, G = CHAINS[name]
    values = np.linspace(-1.0, 1.0, len(features)).astype(np.float32)
    if name == "revisit":
        values = np.float32([-0.5, -np.inf, 0.4, 0.3, 0.1, 0.0, -0.2, 0.9])
    forest = chain(features, values)
    d = max(features) + 4
    max_m = cpu_engine.shap_tables(forest)["max_m"]
    assert max_m == max(features) + 1
    assert not gpu_engine._packed_fits(forest, d)
    route = gpu_engine.large_shap_route(forest, d, KINDS[kind])
    assert route == ("cpu" if G is None else "deep")
    if G is not None:
        assert ext().shap_deep_cfg(kind, d, max_m)[0] == G
    Xk, seen = _rows(kind, 40, d)
    with caplog.at_level(logging.WARNING):
        got = gpu_engine.shap_forest(Shell(forest), Xk.to(dev), True)
    assert bool(_warned(caplog)) == (G is None)
    want = cpu_engine.shap_values(forest, seen)
    assert np.abs(want).max() > 0
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))


def test_public_interface(dev, caplog):
    X = torch.from_numpy(np.random.RandomState(9).standard_normal(
        (20000, D)).astype(np.float32))
    model = IsolationForest(numEstimators=3, maxSamples=16385.0).fit(X.to(dev))
    forest, rows = model.forest, X[:N_ROWS]
    assert gpu_engine.large_shap_route(forest, D, X.dtype) == "deep"
    want = cpu_engine.shap_values(forest, rows.numpy())
    feature_major = torch.zeros((D, N_ROWS + 5), device=dev)[:, :N_ROWS].T
    pitched = torch.zeros((N_ROWS, D + 3), device=dev)[:, :D]
    with caplog.at_level(logging.WARNING):
        for view in (feature_major, pitched):
            view.copy_(rows)
            assert not view.is_contiguous()
            np.testing.assert_array_equal(_bits(model.shap_values(view)),
                                          want.view(np.int32))
            idx, val = model.top_contributing_features(view, 2, method="shap")
            wval = torch.topk(torch.from_numpy(want), 2, dim=1, largest=False,
                              sorted=True)[0]
            assert torch.equal(val.cpu(), wval)
            assert torch.equal(
                torch.gather(torch.from_numpy(want), 1, idx.cpu()), wval)
    assert not _warned(caplog)
    # §8's identity: the bias and the row's SHAP values give its mean path
    mean_path = cpu_engine.path_lengths(forest, rows.numpy()).astype(
        np.float64) / forest.num_trees
    lhs = model.expected_path_length + want.astype(np.float64).sum(axis=1)
    assert np.abs(lhs - mean_path).max() <= 152.0 * forest.num_trees * 2.0**-24
