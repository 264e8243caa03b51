"""Exact TreeSHAP on the GPU (MI355X): shap_forest_kernel against the CPU
oracle cpu_engine.shap_values (docs/DESIGN.md §9).

The contract is BITWISE (float32 outputs compared as int32): the kernel
runs the oracle's float64 operations in the oracle's order on tables built
once on the host. Rows of a 16-bit dtype are compared against the oracle on
their exact float32 widening.

Shapes are the smallest at which each mechanism can break: N around one
256-row tile and past two, d = 1 (m = 1 everywhere), small d (accumulator
tile in LDS), d = 33 (the tile would leave one block per CU: global float64
scratch by size), d = 150 for float32 and d = 300 for 16-bit rows (no key
tile fits: keys read from X per use), one tree and several, trees of 16 and
64 leaves. The route switches force what size alone would need very deep
trees to reach.
"""

import logging
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd import (  # noqa: E402
    IsolationForest,
    IsolationForestModel,
)
from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.core.forest import Forest  # noqa: E402
from tests.conftest import GOLDEN  # noqa: E402
from tests.test_shap_cpu import nonfinite_rows  # noqa: E402

N_LIST = (1, 255, 256, 257, 600)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


def gauss(N, d, seed):
    return np.random.RandomState(seed).normal(size=(N, d)).astype(np.float32)


_MODELS = {}


def fitted(dev, d, T, max_samples):
    """One GPU-fitted model per configuration, shared by the tests."""
    key = (d, T, max_samples)
    if key not in _MODELS:
        X = torch.from_numpy(gauss(600, d, seed=100 + d)).to(dev)
        _MODELS[key] = IsolationForest(
            numEstimators=T, maxSamples=float(max_samples),
            randomSeed=7 + T).fit(X)
    return _MODELS[key]


def as_input(X, dtype):
    """(torch rows of the requested dtype, the float32 matrix they mean)."""
    xt = torch.from_numpy(X).to(dtype)
    return xt, xt.float().numpy()


def assert_same_bits(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (
        f"max |diff| {np.nanmax(np.abs(got - want)):.3e} over "
        f"{int((got.view(np.int32) != want.view(np.int32)).sum())} cells")


def check_bitwise(model, X, dev, dtype=torch.float32, finalize=True,
                  view=None):
    xt, seen = as_input(X, dtype)
    xd = xt.to(dev)
    if view == "pitched":  # rows of a wider buffer, read in place
        buf = torch.zeros((X.shape[0], X.shape[1] + 3), dtype=dtype,
                          device=dev)
        buf[:, :X.shape[1]] = xd
        xd = buf[:, :X.shape[1]]
        assert not xd.is_contiguous() or X.shape[0] == 1
    elif view == "feature":  # a [d, N] buffer seen through .T
        xd = xd.t().contiguous().t()
        assert xd.stride(0) == 1 or X.shape[1] == 1
    got = model.feature_contributions(xd, finalize=finalize, method="shap")
    assert got.is_cuda and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert_same_bits(got, cpu_engine.shap_values(model.forest, seen, finalize))
    return got


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("max_samples", [16, 64])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("d", [1, 3, 6, 33])
def test_base_parity(dev, d, T, max_samples, kind):
    model = fitted(dev, d, T, max_samples)
    for N in N_LIST:
        check_bitwise(model, gauss(N, d, seed=N + d), dev, DTYPES[kind])


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("view", ["pitched", "feature"])
def test_layouts_are_read_in_place(dev, view, kind):
    model = fitted(dev, 6, 5, 64)
    check_bitwise(model, gauss(257, 6, seed=31), dev, DTYPES[kind], view=view)


@pytest.mark.parametrize("view", [None, "pitched", "feature"])
@pytest.mark.parametrize("kind,d", [("f32", 150), ("bf16", 300),
                                    ("f16", 300)])
def test_rows_too_wide_for_a_key_tile(dev, kind, d, view):
    # 256 rows of d keys (600 bytes a row) plus the weights exceed the 150 KB
    # budget: every lane keys its own cells from X through the two strides.
    # N = 257 leaves 255 lanes of the second tile without a row.
    elem = 4 if kind == "f32" else 2
    assert 256 * d * elem + 17 * 16 * 8 > 150 * 1024
    assert 256 * (d - 6) * elem + 17 * 16 * 8 <= 150 * 1024  # just past it
    model = fitted(dev, d, 3, 64)
    X = gauss(257, d, seed=40 + d)
    X[:12, :6] = nonfinite_rows(6)  # NaN keys from X, too
    check_bitwise(model, X, dev, DTYPES[kind], view=view)


def test_rows_too_wide_grid_stride_and_forced_routes(dev, monkeypatch):
    model = fitted(dev, 150, 3, 64)
    X = gauss(600, 150, seed=41)
    monkeypatch.setenv("IFA_SHAP_MAX_BLOCKS", "1")
    check_bitwise(model, X, dev, finalize=False)
    monkeypatch.setenv("IFA_SHAP_FORCE_GLOBAL_TABLE", "1")
    check_bitwise(model, X, dev, view="feature")


@pytest.mark.parametrize("kind", list(DTYPES))
def test_nonfinite_rows(dev, kind):
    model = fitted(dev, 6, 5, 64)
    X = nonfinite_rows(6)
    got = check_bitwise(model, X, dev, DTYPES[kind])
    assert np.isfinite(got).all()


def test_finalize_false_is_raw_sum(dev):
    model = fitted(dev, 6, 5, 64)
    X = gauss(257, 6, seed=32)
    raw = check_bitwise(model, X, dev, finalize=False)
    fin = check_bitwise(model, X, dev)
    assert np.abs(raw).max() > np.abs(fin).max()


@pytest.mark.parametrize("switches", [
    ("IFA_SHAP_FORCE_GLOBAL_TABLE",),
    ("IFA_SHAP_FORCE_GLOBAL_ACC",),
    ("IFA_SHAP_FORCE_GLOBAL_TABLE", "IFA_SHAP_FORCE_GLOBAL_ACC"),
], ids=["table", "acc", "both"])
def test_forced_global_routes(dev, monkeypatch, switches):
    model = fitted(dev, 6, 5, 64)
    X = gauss(257, 6, seed=33)
    lds = check_bitwise(model, X, dev)
    for s in switches:
        monkeypatch.setenv(s, "1")
    for kind in DTYPES:
        check_bitwise(model, X, dev, DTYPES[kind])
    assert_same_bits(check_bitwise(model, X, dev), lds)
    check_bitwise(model, nonfinite_rows(6), dev)
    check_bitwise(model, X, dev, view="feature")


@pytest.mark.parametrize("force_global", [False, True])
def test_one_block_walks_several_tiles(dev, monkeypatch, force_global):
    monkeypatch.setenv("IFA_SHAP_MAX_BLOCKS", "1")
    if force_global:
        monkeypatch.setenv("IFA_SHAP_FORCE_GLOBAL_ACC", "1")
    model = fitted(dev, 6, 5, 64)
    X = gauss(600, 6, seed=34)  # tiles of 256, 256 and 88 rows
    check_bitwise(model, X, dev)
    check_bitwise(model, X, dev, torch.bfloat16)


def test_loaded_spark_model(dev, mammography):
    model = IsolationForestModel.load(
        os.path.join(GOLDEN, "savedIsolationForestModel"))
    X = np.ascontiguousarray(mammography[0][:257])
    for kind in DTYPES:
        check_bitwise(model, X, dev, DTYPES[kind])


def test_top_contributing_features(dev):
    model = fitted(dev, 6, 5, 64)
    X = gauss(257, 6, seed=35)
    idx, val = model.top_contributing_features(
        torch.from_numpy(X).to(dev), 2, method="shap")
    assert idx.is_cuda and val.is_cuda and idx.dtype == torch.int64
    want = torch.from_numpy(cpu_engine.shap_values(model.forest, X))
    wval, widx = torch.topk(want, 2, dim=1, largest=False, sorted=True)
    assert torch.equal(val.cpu(), wval)
    assert torch.equal(torch.gather(want, 1, idx.cpu()), wval)
    assert torch.equal(model.shap_values(torch.from_numpy(X).to(dev)).cpu(),
                       want)


def test_empty_input(dev):
    model = fitted(dev, 6, 5, 64)
    out = model.shap_values(torch.empty((0, 6), device=dev))
    assert tuple(out.shape) == (0, 6) and out.dtype == torch.float32
    assert out.is_cuda


def test_pack_cache_keys_do_not_collide(dev):
    model = fitted(dev, 6, 5, 64)
    X = gauss(257, 6, seed=36)
    for kind in ("f32", "bf16", "f16", "f32", "f16", "bf16"):
        check_bitwise(model, X, dev, DTYPES[kind])
        xt, seen = as_input(X, DTYPES[kind])
        path = model.feature_contributions(xt.to(dev)).cpu().numpy()
        assert_same_bits(
            path, cpu_engine.feature_contributions(model.forest, seen))


def _with_forest(model, forest):
    return IsolationForestModel(model.uid, forest, model.params)


def test_packed_cap_fallback_returns_the_oracle_bits(dev, caplog):
    # feature ids past the packed records' 12 bits: the CPU oracle answers
    base = fitted(dev, 6, 5, 64).forest
    shift = 4100 - 6
    wide = Forest(
        feature=np.where(base.feature >= 0, base.feature + shift,
                         base.feature).astype(np.int32),
        value=base.value.copy(), right=base.right.copy(),
        num_instances=base.num_instances.copy(),
        node_count=base.node_count.copy(), num_samples=base.num_samples,
        num_features=base.num_features, total_num_features=4100,
        value64=base.value64.copy())
    model = _with_forest(fitted(dev, 6, 5, 64), wide)
    X = gauss(40, 4100, seed=37)
    with caplog.at_level(logging.WARNING):
        got = model.shap_values(torch.from_numpy(X).to(dev))
    assert "CPU oracle" in caplog.text
    assert got.is_cuda and got.dtype == torch.float32
    want = cpu_engine.shap_values(wide, X)
    assert_same_bits(got.cpu().numpy(), want)
    # the same values as the narrow forest gives its 6 columns
    assert_same_bits(np.ascontiguousarray(want[:, shift:]),
                     cpu_engine.shap_values(
                         base, np.ascontiguousarray(X[:, shift:])))
    assert (want[:, :shift] == 0).all()


def test_more_than_16_features_on_a_path_fallback(dev, caplog):
    # a chain of 17 splits, one feature each: node 2i splits on feature i,
    # its left child 2i+1 is a leaf, its right child is node 2i+2
    k = 17
    mn = 2 * k + 1
    feature = np.full((1, mn), Forest.LEAF, dtype=np.int32)
    feature[0, 0:2 * k:2] = np.arange(k)
    right = np.full((1, mn), -1, dtype=np.int32)
    right[0, 0:2 * k:2] = np.arange(2, 2 * k + 2, 2)
    counts = np.where(feature[0] >= 0, -1, 1).astype(np.int64)[None, :]
    value = np.zeros((1, mn), dtype=np.float32)
    chain = Forest(feature=feature, value=value, right=right,
                   num_instances=counts,
                   node_count=np.array([mn], dtype=np.int32),
                   num_samples=k + 1, num_features=k, total_num_features=k,
                   value64=value.astype(np.float64))
    assert cpu_engine.shap_tables(chain)["max_m"] == 17
    model = _with_forest(fitted(dev, 6, 5, 64), chain)
    X = gauss(40, k, seed=38)
    with caplog.at_level(logging.WARNING):
        got = model.shap_values(torch.from_numpy(X).to(dev))
    assert "CPU oracle" in caplog.text and got.is_cuda
    assert_same_bits(got.cpu().numpy(), cpu_engine.shap_values(chain, X))
