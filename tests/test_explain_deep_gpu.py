"""GPU tests (MI355X): path attribution for standard forests past the 15-bit
node ids (explain_forest_deep_kernel, ops/hip/deep_kernels.hip) against
cpu_engine.feature_contributions and the CPU model, bit for bit.

The forest is test_score_deep_gpu.py's: n = 16385, d = 6, T = 5, 2.5k-6.2k
nodes a tree, height 15; five trees cross one phase boundary and bring three
pad trees. The levels cross a stage of 64 records after 6 and the default
stage after 9, so both walk phases run either way. 1500 rows are full tiles
and a tail.
"""

import functools
import logging
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd import IsolationForest  # noqa: E402
from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.ops import gpu_engine  # noqa: E402

KINDS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
N_BAG, D, T, N_ROWS = 16385, 6, 5, 1500


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


class Shell:
    """What gpu_engine.explain_forest reads of a model."""

    def __init__(self, forest):
        self.forest = forest
        self._gpu_forest_cache = {}


@functools.lru_cache(maxsize=None)
def _forest(which):
    X = np.random.RandomState(5).standard_normal((20000, D)).astype(np.float32)
    if which == "leaves":  # constant data: every root is a leaf
        X[:] = 1.5
    bag = cpu_engine.sample_bags(20000, T, N_BAG, seed=31, bootstrap=False)
    fs = cpu_engine.feature_subsets(D, D, T, seed=31)
    forest = cpu_engine.build_forest(X, bag, fs, 31, N_BAG, D, D)
    assert forest.feature.shape[1] > 32767
    return forest


@functools.lru_cache(maxsize=None)
def _rows(kind, width=D):
    """(rows of the kind on the host, the same values as f32 numpy)"""
    X = np.random.RandomState(6).standard_normal((N_ROWS, width)).astype(
        np.float32)
    X[3, 1], X[700, 0], X[1499, 5], X[1024, 2] = np.nan, np.inf, -np.inf, 0.0
    Xk = torch.from_numpy(X).to(KINDS[kind])
    return Xk, Xk.float().numpy()


@functools.lru_cache(maxsize=None)
def _oracle(which, kind, finalize=False, width=D):
    with np.errstate(all="ignore"):
        return cpu_engine.feature_contributions(
            _forest(which), _rows(kind, width)[1], finalize)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _deep(dev, which, kind, X=None, finalize=False):
    forest = _forest(which)
    assert not gpu_engine._packed_fits(forest, D)
    shell = Shell(forest)
    X = _rows(kind)[0].to(dev) if X is None else X
    assert gpu_engine.large_explain_route(
        forest, X.shape[1], KINDS[kind]) == "deep"
    return shell, gpu_engine.explain_forest(shell, X, finalize=finalize)


@pytest.mark.parametrize("finalize", [False, True])
@pytest.mark.parametrize("stage", ["64", None])
@pytest.mark.parametrize("kind", list(KINDS))
def test_bitwise_against_the_oracle(dev, monkeypatch, kind, stage, finalize):
    if stage is not None:
        monkeypatch.setenv("IFA_EXPLAIN_DEEP_STAGE", stage)
    _, got = _deep(dev, "trees", kind, finalize=finalize)
    np.testing.assert_array_equal(
        _bits(got), _oracle("trees", kind, finalize).view(np.int32))


@pytest.mark.parametrize("max_blocks", [None, "1"])
@pytest.mark.parametrize("global_acc", [False, True])
def test_accumulator_routes_and_grid_stride(dev, monkeypatch, global_acc,
                                            max_blocks):
    if global_acc:
        monkeypatch.setenv("IFA_EXPLAIN_FORCE_GLOBAL_ACC", "1")
    if max_blocks is not None:  # one block: the tile is zeroed per row tile
        monkeypatch.setenv("IFA_EXPLAIN_MAX_BLOCKS", max_blocks)
    _, got = _deep(dev, "trees", "bf16", finalize=True)
    np.testing.assert_array_equal(
        _bits(got), _oracle("trees", "bf16", True).view(np.int32))


def test_wide_rows_take_one_row_per_thread(dev):
    """64 bf16 columns: the accumulator tile does not fit, so the adds go to
    out at one row per thread; the forest still splits on the first six."""
    X = _rows("bf16", 64)[0].to(dev)
    _, got = _deep(dev, "trees", "bf16", X=X, finalize=True)
    np.testing.assert_array_equal(
        _bits(got), _oracle("trees", "bf16", True, 64).view(np.int32))


@pytest.mark.parametrize("kind", list(KINDS))
def test_single_leaf_trees(dev, kind):
    assert int(_forest("leaves").node_count.max()) == 1
    shell, got = _deep(dev, "leaves", kind)
    assert got.shape == (N_ROWS, D) and not _bits(got).any()
    (records, lds_levels, _), = shell._gpu_forest_cache.values()
    assert records.shape == (8, 1, 4) and not lds_levels.any()


@pytest.mark.parametrize("layout", ["pitched", "feature"])
def test_views_give_the_bits_of_the_packed_call(dev, layout):
    packed = _rows("bf16")[0].to(dev)
    if layout == "pitched":
        view = torch.zeros((N_ROWS, D + 3), dtype=packed.dtype,
                           device=dev)[:, :D]
    else:
        view = torch.zeros((D, N_ROWS + 5), dtype=packed.dtype,
                           device=dev)[:, :N_ROWS].T
    view.copy_(packed)
    assert not view.is_contiguous()
    _, want = _deep(dev, "trees", "bf16")
    _, got = _deep(dev, "trees", "bf16", X=view)
    np.testing.assert_array_equal(_bits(got), _bits(want))


def test_model_fit_and_explain(dev, caplog):
    X = torch.from_numpy(np.random.RandomState(9).standard_normal(
        (25000, D)).astype(np.float32))
    make = lambda: IsolationForest(  # noqa: E731
        numEstimators=3, maxSamples=20000.0, contamination=0.02)
    gpu_m, cpu_m = make().fit(X.to(dev)), make().fit(X)
    assert gpu_engine.large_explain_route(gpu_m.forest, D, X.dtype) == "deep"
    with caplog.at_level(logging.WARNING):
        got = gpu_m.feature_contributions(X[:3000].to(dev))
        top, _ = gpu_m.top_contributing_features(X[:3000].to(dev), k=1)
    assert not [r for r in caplog.records
                if "computing on the CPU oracle" in r.getMessage()]
    np.testing.assert_array_equal(
        _bits(got), _bits(cpu_m.feature_contributions(X[:3000])))
    want_top, _ = cpu_m.top_contributing_features(X[:3000], k=1)
    np.testing.assert_array_equal(top.cpu().numpy(), want_top.numpy())


def test_cpu_fallback(dev, monkeypatch):
    _, deep = _deep(dev, "trees", "f32")
    foreign = types.SimpleNamespace(node_count=np.array([40000]),
                                    feature=np.array([[4095, -1, -1]]))
    assert gpu_engine.large_explain_route(foreign, D, torch.float32) == "cpu"
    monkeypatch.setenv("IFA_EXPLAIN_DEEP", "0")
    forest = _forest("trees")
    assert gpu_engine.large_explain_route(forest, D, torch.float32) == "cpu"
    cpu = gpu_engine.explain_forest(Shell(forest), _rows("f32")[0].to(dev),
                                    finalize=False)
    np.testing.assert_array_equal(_bits(cpu), _bits(deep))
