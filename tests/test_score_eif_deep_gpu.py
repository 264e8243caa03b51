"""GPU tests (MI355X): scoring extended forests past the 15-bit node ids on
the deep route (score_extended_deep_kernel, ops/hip/deep_kernels.hip) against
cpu_engine.path_lengths_extended and the CPU model, bit for bit.

The forests and rows are those of test_explain_eif_deep_gpu.py: n = 16385,
d = 6, T = 5 (65535 node slots a tree, height 15; five trees cross a phase
boundary and bring three pad trees), 1500 rows (full tiles and a tail) with a
NaN, both infinities and a zero planted. A stage of 2 records leaves one
level to phase A and the default stage ends well above the leaves, so both
walk phases run either way, which the main case asserts from lds_levels.
"""

import functools

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
    """What gpu_engine.score_extended_forest_deep reads of a model."""

    def __init__(self, forest):
        self.forest = forest
        self._gpu_forest_cache = {}


@functools.lru_cache(maxsize=None)
def _forest(level, constant=False):
    X = np.random.RandomState(5).standard_normal((20000, D)).astype(np.float32)
    if constant:
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
def _oracle(level, kind, width=D):
    with np.errstate(all="ignore"):
        return cpu_engine.path_lengths_extended(
            _forest(level), _rows(kind, width)[1])


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _deep(dev, forest, kind, X=None):
    shell = Shell(forest)
    X = _rows(kind)[0].to(dev) if X is None else X
    assert gpu_engine.large_score_route(
        forest, X.shape[1], KINDS[kind]) == "deep"
    return shell, gpu_engine.score_extended_forest_deep(shell, X,
                                                        finalize=False)


@pytest.mark.parametrize("stage", ["2", None])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("level", [5, 2, 0])  # nnz 6, 3, 1
def test_bitwise_against_the_oracle(dev, monkeypatch, level, kind, stage):
    if stage is not None:
        monkeypatch.setenv("IFA_EIF_DEEP_STAGE", stage)
    forest = _forest(level)
    shell, got = _deep(dev, forest, kind)
    (_, lds_levels, extra), = shell._gpu_forest_cache.values()
    levels = lds_levels[:T].cpu().numpy()
    assert 0 < levels.min() and levels.max() < extra["height"]
    np.testing.assert_array_equal(
        _bits(got), _oracle(level, kind).view(np.int32))


def _width_for_rpt(rpt, nnz):
    """the narrowest bf16 rows of at least D columns that run `rpt` rows a
    thread, asked of the binding"""
    from isolation_forest_amd.ops import load_extension

    cfg = load_extension().score_eif_deep_cfg
    return next(w for w in range(D, 4095) if cfg("bf16", w, nnz)[0] == rpt)


@pytest.mark.parametrize("phase,rpt", [(4, 2), (2, 2), (1, 2), (None, 1)])
def test_every_instantiation_shape(dev, monkeypatch, phase, rpt):
    """Each trees-per-phase value, and rows wide enough for one row a
    thread; the hyperplanes still use the first six columns."""
    from isolation_forest_amd.ops import load_extension

    if phase is not None:
        monkeypatch.setenv("IFA_EIF_DEEP_PHASE", str(phase))
    width = _width_for_rpt(rpt, D)
    cfg = load_extension().score_eif_deep_cfg("bf16", width, D)
    assert cfg[0] == rpt and cfg[2] > 0
    assert phase is None or cfg[1] == phase
    _, got = _deep(dev, _forest(5), "bf16", X=_rows("bf16", width)[0].to(dev))
    np.testing.assert_array_equal(
        _bits(got), _oracle(5, "bf16", width).view(np.int32))


def test_constant_training_data(dev):
    """31-node chains of one-sided splits with zero-instance leaves, all
    inside any stage: the last level ends the walk in phase A."""
    forest = _forest(5, constant=True)
    assert int(forest.node_count.max()) == 31
    with np.errstate(all="ignore"):
        want = cpu_engine.path_lengths_extended(forest, _rows("f32")[1])
    _, got = _deep(dev, forest, "f32")
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))


def test_single_leaf_trees(dev):
    """Every root a leaf, the arrays written by hand: a pack of one record
    a tree."""
    forest = empty_extended_forest(T, 65535, D, N_BAG, D, D, D - 1)
    forest.feature[:, 0] = ExtendedForest.LEAF
    forest.num_instances[:, 0] = N_BAG
    forest.node_count[:] = 1
    forest.leaf_values_from_counts()
    want = cpu_engine.path_lengths_extended(forest, _rows("bf16")[1])
    shell, got = _deep(dev, forest, "bf16")
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))
    (nodes, lds_levels, extra), = shell._gpu_forest_cache.values()
    assert nodes.shape == (8, 1, 2) and not lds_levels.any()
    assert extra["hyper"].shape == (8, 1, D, 2)


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
    _, got = _deep(dev, _forest(2), "bf16", X=view)
    np.testing.assert_array_equal(_bits(got), _oracle(2, "bf16").view(np.int32))


def test_model_fit_and_score(dev):
    X = torch.from_numpy(np.random.RandomState(9).standard_normal(
        (25000, D)).astype(np.float32))
    make = lambda: ExtendedIsolationForest(  # noqa: E731
        numEstimators=3, maxSamples=20000.0, contamination=0.02)
    gpu_m, cpu_m = make().fit(X.to(dev)), make().fit(X)
    assert gpu_engine.large_score_route(gpu_m.forest, D, X.dtype) == "deep"
    assert (np.float64(gpu_m.outlier_score_threshold).tobytes()
            == np.float64(cpu_m.outlier_score_threshold).tobytes())
    np.testing.assert_array_equal(
        _bits(gpu_m.score(X[:3000].to(dev))), _bits(cpu_m.score(X[:3000])))


def test_wide_fallback(dev, monkeypatch):
    forest = _forest(2)
    shell, deep = _deep(dev, forest, "f32")
    for cut, node_count in ((-1, 3), (0, (1 << 20) + 1)):
        foreign = empty_extended_forest(1, 3, D, N_BAG, D, D, D - 1)
        foreign.feature[0] = [D, ExtendedForest.LEAF, ExtendedForest.LEAF]
        foreign.hyper_idx[0, 0, 0] = cut
        foreign.node_count[:] = node_count
        assert gpu_engine.large_score_route(
            foreign, D, torch.float32) == "wide"
    monkeypatch.setenv("IFA_SCORE_DEEP", "0")
    assert gpu_engine.large_score_route(forest, D, torch.float32) == "wide"
    wide = gpu_engine.score_extended_forest(
        shell, _rows("f32")[0].to(dev), finalize=False)
    np.testing.assert_array_equal(_bits(wide), _bits(deep))
