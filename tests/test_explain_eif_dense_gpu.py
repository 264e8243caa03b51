"""explain_extended_dense_kernel (ops/hip/explain_kernels.hip) against the
CPU oracle: extended forests of the default maxSamples = 256 whose whole
tree is staged in LDS, rows and accumulators in registers.

The contract is BITWISE (np.array_equal on the int32 view of
cpu_engine.feature_contributions_extended; the oracle's input is the exact
float32 widening of 16-bit rows). Shapes: every padded width D exact and
padded (d = 8 / 3, 16 / 9, 32 / 17), N = 1, one below and one past a block's
row tile, and one past two tiles on a single block (grid-stride loop,
accumulators zeroed again), T = 1 and 5, the three row types.
"""

import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd import ExtendedIsolationForest  # noqa: E402
from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.ops import gpu_engine  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
route = gpu_engine.extended_explain_route


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def gauss(N, d, seed, dtype=torch.float32):
    X = np.random.RandomState(seed).normal(size=(N, d)).astype(np.float32)
    return torch.from_numpy(X).to(dtype)


_MODELS = {}


def fitted(dev, d, T, n_train=600, **kw):
    """One GPU-fitted model per configuration, shared by the tests."""
    key = (d, T, n_train, tuple(sorted(kw.items())))
    if key not in _MODELS:
        _MODELS[key] = ExtendedIsolationForest(
            numEstimators=T, randomSeed=7 + T, **kw).fit(
                gauss(n_train, d, seed=100 + d).to(dev))
    return _MODELS[key]


def tile_rows(model, d, dtype):
    D, rpt, _, threads = gpu_engine._explain_eif_dense_cfg(
        gpu_engine._row_kind(dtype), d, model.forest.max_nodes)
    assert D >= d and rpt * threads > 0
    return rpt * threads


def check(model, xt, dev, want_route="dense", finalize=True, view=None):
    """xt: CPU rows of the tested dtype; view(x) lays them out on the device."""
    X = view(xt.to(dev)) if view else xt.to(dev)
    assert route(model.forest, xt.shape[1], X.dtype) == want_route
    got = model.feature_contributions(X, finalize=finalize)
    assert got.is_cuda and got.dtype == torch.float32
    got = got.cpu().numpy()
    want = cpu_engine.feature_contributions_extended(
        model.forest, xt.float().numpy(), finalize)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (
        f"{int((got.view(np.int32) != want.view(np.int32)).sum())} cells "
        f"differ, max |diff| {np.nanmax(np.abs(got - want)):.3e}")
    return got


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("d", [3, 8, 9, 16, 17, 32])
def test_fully_extended_shapes(dev, monkeypatch, d, T, kind):
    model = fitted(dev, d, T)
    assert model.forest.nnz == d
    tile = tile_rows(model, d, DTYPES[kind])
    for N in (1, tile - 1, tile + 1):
        check(model, gauss(N, d, N + d, DTYPES[kind]), dev)
    monkeypatch.setenv("IFA_EXPLAIN_MAX_BLOCKS", "1")
    check(model, gauss(2 * tile + 1, d, d, DTYPES[kind]), dev)


def test_finalize_both_ways(dev):
    model = fitted(dev, 9, 5)
    X = gauss(600, 9, 3)
    raw = check(model, X, dev, finalize=False)
    fin = check(model, X, dev)
    assert np.array_equal((raw / np.float32(5)).astype(np.float32), fin)


@pytest.mark.parametrize("kind", list(DTYPES))
def test_non_finite_cells_stay_dense(dev, kind):
    model = fitted(dev, 17, 5)
    X = gauss(1500, 17, 4)
    hit = np.random.RandomState(5).random_sample(X.shape)
    for lo, v in ((0.00, np.nan), (0.05, np.inf), (0.10, -np.inf)):
        X[torch.from_numpy((hit >= lo) & (hit < lo + 0.05))] = v
    check(model, X.to(DTYPES[kind]), dev)


@pytest.mark.parametrize("kw", [
    {"extensionLevel": max(gpu_engine.EIF_EXPLAIN_DENSE_MIN_NNZ, 6) - 1},
    {"maxFeatures": 0.75},  # per-tree coordinate subsets
], ids=["level", "max_features"])
def test_partial_hyperplanes(dev, kw):
    model = fitted(dev, 16, 5, **kw)
    assert gpu_engine.EIF_EXPLAIN_DENSE_MIN_NNZ <= model.forest.nnz < 16
    X = gauss(1100, 16, 6, torch.bfloat16)
    check(model, X, dev)
    X[700, 3] = float("nan")  # this batch takes explain_extended_kernel
    check(model, X, dev)


@pytest.mark.parametrize("layout", ["pitched", "feature"])
def test_views_read_in_place(dev, layout):
    model = fitted(dev, 9, 5)

    def view(x):
        if layout == "feature":
            return x.T.contiguous().T
        table = torch.zeros((x.shape[0], 16), dtype=x.dtype, device=x.device)
        table[:, 2:11] = x
        return table[:, 2:11]

    check(model, gauss(1100, 9, 7, torch.bfloat16), dev, view=view)


def test_switch_keeps_the_strict_kernel_and_the_bits(dev, monkeypatch):
    model = fitted(dev, 17, 5)
    X = gauss(1100, 17, 8, torch.float16)
    dense = check(model, X, dev)
    monkeypatch.setenv("IFA_EXPLAIN_EIF_DENSE", "0")
    strict = check(model, X, dev, want_route="strict")
    assert np.array_equal(dense.view(np.int32), strict.view(np.int32))


def test_routes_that_stay_strict(dev):
    big = fitted(dev, 32, 1, n_train=2000, maxSamples=1024.0)
    assert route(big.forest, 32, torch.bfloat16) == "strict"  # stage > LDS
    forest = copy.deepcopy(fitted(dev, 8, 1).forest)
    assert route(forest, 8, torch.float32) == "dense"
    t, v = np.argwhere(forest.feature >= 0)[0]
    forest.hyper_idx[t, v, [0, 1]] = forest.hyper_idx[t, v, [1, 0]]
    forest.invalidate_derived()
    assert route(forest, 8, torch.float32) == "strict"  # no longer ascending
