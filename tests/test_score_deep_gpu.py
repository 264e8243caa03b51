"""GPU tests (MI355X): the deep scoring route for standard forests past the
15-bit node ids (ops/hip/deep_kernels.hip) against cpu_engine.path_lengths
and the CPU model, bit for bit.

The forest is n = 16385, d = 6, T = 5: about 3.5k nodes a tree, five trees
cross one phase boundary and bring three pad trees. With IFA_DEEP_STAGE=64
almost every level is walked from global memory; with the default stage the
tree splits between LDS and L2 as in production. 1500 rows are two full
tiles and a tail.
"""

import functools
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
    """What gpu_engine.score_forest reads of a model."""

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
def _rows(kind):
    """(rows of the kind on the host, the same values as f32 numpy)"""
    X = np.random.RandomState(6).standard_normal((N_ROWS, D)).astype(
        np.float32)
    X[3, 1], X[700, 0], X[1499, 5], X[1024, 2] = np.nan, np.inf, -np.inf, 0.0
    Xk = torch.from_numpy(X).to(KINDS[kind])
    return Xk, Xk.float().numpy()


@functools.lru_cache(maxsize=None)
def _oracle(which, kind):
    with np.errstate(all="ignore"):
        return cpu_engine.path_lengths(_forest(which), _rows(kind)[1])


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def _deep(dev, which, kind, X=None):
    forest = _forest(which)
    assert not gpu_engine._packed_fits(forest, D)
    assert gpu_engine.large_score_route(forest, D, KINDS[kind]) == "deep"
    shell = Shell(forest)
    X = _rows(kind)[0].to(dev) if X is None else X
    return shell, gpu_engine.score_forest(shell, X, finalize=False)


@pytest.mark.parametrize("stage", ["64", None])
@pytest.mark.parametrize("kind", list(KINDS))
def test_bitwise_against_the_oracle(dev, monkeypatch, kind, stage):
    if stage is not None:
        monkeypatch.setenv("IFA_DEEP_STAGE", stage)
    _, got = _deep(dev, "trees", kind)
    np.testing.assert_array_equal(
        _bits(got), _oracle("trees", kind).view(np.int32))


@pytest.mark.parametrize("kind", list(KINDS))
def test_single_leaf_trees(dev, kind):
    assert int(_forest("leaves").node_count.max()) == 1
    shell, got = _deep(dev, "leaves", kind)
    np.testing.assert_array_equal(
        _bits(got), _oracle("leaves", kind).view(np.int32))
    (records, lds_levels, _), = shell._gpu_forest_cache.values()
    assert records.shape[0] == 8 and not lds_levels.any()


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


def test_model_fit_score_and_threshold(dev):
    X = torch.from_numpy(np.random.RandomState(9).standard_normal(
        (25000, D)).astype(np.float32))
    make = lambda: IsolationForest(  # noqa: E731
        numEstimators=3, maxSamples=20000.0, contamination=0.02)
    gpu_m, cpu_m = make().fit(X.to(dev)), make().fit(X)
    assert gpu_engine.large_score_route(gpu_m.forest, D, X.dtype) == "deep"
    assert (np.float64(gpu_m.outlier_score_threshold).tobytes()
            == np.float64(cpu_m.outlier_score_threshold).tobytes())
    np.testing.assert_array_equal(_bits(gpu_m.score(X[:3000].to(dev))),
                                  _bits(cpu_m.score(X[:3000])))


def test_wide_fallback(dev, monkeypatch):
    _, deep = _deep(dev, "trees", "f32")
    foreign = types.SimpleNamespace(node_count=np.array([40000]),
                                    feature=np.array([[4095, -1, -1]]))
    assert gpu_engine.large_score_route(foreign, D, torch.float32) == "wide"
    monkeypatch.setenv("IFA_SCORE_DEEP", "0")
    forest = _forest("trees")
    assert gpu_engine.large_score_route(forest, D, torch.float32) == "wide"
    wide = gpu_engine.score_forest(Shell(forest), _rows("f32")[0].to(dev),
                                   finalize=False)
    np.testing.assert_array_equal(_bits(wide), _bits(deep))
