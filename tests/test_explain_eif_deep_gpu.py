"""GPU tests (MI355X): path attribution for extended forests past the 15-bit
node ids (explain_extended_deep_kernel, ops/hip/deep_kernels.hip) against
cpu_engine.feature_contributions_extended and the CPU model, bit for bit.

The forests are cpu_engine.build_extended_forest's at n = 16385, d = 6,
T = 5 (65535 node slots a tree, height 15), fully extended and at
extensionLevel 1; five trees cross a phase boundary and bring three pad
trees. A stage of 2 records leaves one level to phase A; the default stage
(512 or 1024 records here) ends well above the leaves, so both walk phases
run either way, which every case asserts from the pack's lds_levels. 1500
rows are full tiles and a tail.
"""

import functools
import logging

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd import ExtendedIsolationForest  # noqa: E402
from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.core.forest import (  # noqa: E402
    ExtendedForest, empty_extended_forest)
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
    """What gpu_engine.explain_extended_forest reads of a model."""

    def __init__(self, forest):
        self.forest = forest
        self._gpu_forest_cache = {}


@functools.lru_cache(maxsize=None)
def _forest(level, constant=False):
    X = np.random.RandomState(5).standard_normal((20000, D)).astype(np.float32)
    if constant:  # every root is a leaf
        X[:] = 1.5
    bag = cpu_engine.sample_bags(20000, T, N_BAG, seed=31, bootstrap=False)
    fs = cpu_engine.feature_subsets(D, D, T, seed=31)
    forest = cpu_engine.build_extended_forest(
        X, bag, fs, 31, N_BAG, D, D, level)
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
def _oracle(level, kind, finalize=False, width=D):
    with np.errstate(all="ignore"):
        return cpu_engine.feature_contributions_extended(
            _forest(level), _rows(kind, width)[1], finalize)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _deep(dev, forest, kind, X=None, finalize=False):
    assert not gpu_engine._packed_fits(forest, D)
    shell = Shell(forest)
    X = _rows(kind)[0].to(dev) if X is None else X
    assert gpu_engine.large_explain_route(
        forest, X.shape[1], KINDS[kind]) == "deep"
    return shell, gpu_engine.explain_extended_forest(shell, X,
                                                     finalize=finalize)


def _assert_both_phases(shell, forest):
    (_, lds_levels, extra), = shell._gpu_forest_cache.values()
    levels = lds_levels[:forest.num_trees].cpu().numpy()
    assert 0 < levels.min() and levels.max() < extra["height"]


@pytest.mark.parametrize("finalize", [False, True])
@pytest.mark.parametrize("stage", ["2", None])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("level", [D - 1, 1])
def test_bitwise_against_the_oracle(dev, monkeypatch, level, kind, stage,
                                    finalize):
    if stage is not None:
        monkeypatch.setenv("IFA_EXPLAIN_DEEP_STAGE", stage)
    forest = _forest(level)
    shell, got = _deep(dev, forest, kind, finalize=finalize)
    _assert_both_phases(shell, forest)
    np.testing.assert_array_equal(
        _bits(got), _oracle(level, kind, finalize).view(np.int32))


@pytest.mark.parametrize("switch", ["IFA_EXPLAIN_FORCE_GLOBAL_ACC",
                                    "IFA_EXPLAIN_MAX_BLOCKS"])
def test_accumulators_in_out_and_grid_stride(dev, monkeypatch, switch):
    monkeypatch.setenv(switch, "1")  # one block: the tile is zeroed again
    _, got = _deep(dev, _forest(D - 1), "bf16", finalize=True)
    np.testing.assert_array_equal(
        _bits(got), _oracle(D - 1, "bf16", True).view(np.int32))


def test_wide_rows_take_one_row_per_thread(dev):
    """64 bf16 columns: the accumulator tile does not fit, so the adds go to
    out at one row per thread; the hyperplanes still use the first six."""
    X = _rows("bf16", 64)[0].to(dev)
    _, got = _deep(dev, _forest(D - 1), "bf16", X=X, finalize=True)
    np.testing.assert_array_equal(
        _bits(got), _oracle(D - 1, "bf16", True, 64).view(np.int32))


def test_constant_training_data(dev):
    """An extended tree splits constant data all the same: a chain of
    one-sided splits with zero-instance leaves, 31 nodes, all inside any
    stage. Here the last level ends the walk in phase A."""
    forest = _forest(D - 1, constant=True)
    assert int(forest.node_count.max()) == 31
    with np.errstate(all="ignore"):
        want = cpu_engine.feature_contributions_extended(
            forest, _rows("f32")[1], False)
    _, got = _deep(dev, forest, "f32")
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))


def test_single_leaf_trees(dev):
    """Every root a leaf (no build gives that at this bag size, so the
    arrays are written by hand): nothing to add, and a pack of one record."""
    forest = empty_extended_forest(T, 65535, D, N_BAG, D, D, D - 1)
    forest.feature[:, 0] = ExtendedForest.LEAF
    forest.num_instances[:, 0] = N_BAG
    forest.node_count[:] = 1
    forest.leaf_values_from_counts()
    shell, got = _deep(dev, forest, "bf16")
    assert got.shape == (N_ROWS, D) and not _bits(got).any()
    (nodes, lds_levels, extra), = shell._gpu_forest_cache.values()
    assert nodes.shape == (8, 1, 2) and not lds_levels.any()
    assert extra["payload"].shape == (8, 1, D, 4)


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
    _, got = _deep(dev, _forest(1), "bf16", X=view)
    np.testing.assert_array_equal(
        _bits(got), _oracle(1, "bf16").view(np.int32))


def test_model_fit_and_explain(dev, caplog):
    X = torch.from_numpy(np.random.RandomState(9).standard_normal(
        (25000, D)).astype(np.float32))
    make = lambda: ExtendedIsolationForest(  # noqa: E731
        numEstimators=3, maxSamples=20000.0, contamination=0.02)
    gpu_m, cpu_m = make().fit(X.to(dev)), make().fit(X)
    assert gpu_engine.large_explain_route(gpu_m.forest, D, X.dtype) == "deep"
    with caplog.at_level(logging.WARNING):
        got = gpu_m.feature_contributions(X[:3000].to(dev))
    assert not [r for r in caplog.records
                if "computing on the CPU oracle" in r.getMessage()]
    np.testing.assert_array_equal(
        _bits(got), _bits(cpu_m.feature_contributions(X[:3000])))


def test_cpu_fallback(dev, monkeypatch):
    forest = _forest(1)
    _, deep = _deep(dev, forest, "f32")
    monkeypatch.setenv("IFA_EXPLAIN_DEEP", "0")
    assert gpu_engine.large_explain_route(forest, D, torch.float32) == "cpu"
    cpu = gpu_engine.explain_extended_forest(
        Shell(forest), _rows("f32")[0].to(dev), finalize=False)
    np.testing.assert_array_equal(_bits(cpu), _bits(deep))
