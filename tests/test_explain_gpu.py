"""Per-feature attribution on the GPU (MI355X): explain_forest_kernel and
explain_extended_kernel against the CPU oracle.

The contract is BITWISE for both kernels (np.array_equal on the float32
values; EIF included at every extension level, because the explain walk is
strict-order). Explain is compared against cpu_engine.feature_contributions*
and never against score(), whose EIF dense routes carry tolerance contracts.

Shapes are the smallest at which each mechanism can break: N around one
256-row tile and past two, d in {1, 5, 33} (2 rows/thread with 2 trees per
barrier, 2 rows/thread, 1 row/thread) and d = 200 (global accumulators;
global rows too at float32), T in {1, 5, 13} (partial last staging group),
both input dtypes. The bf16 oracle input is the exact float32 widening.
"""

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd import (  # noqa: E402
    ExtendedIsolationForest,
    ExtendedIsolationForestModel,
    IsolationForest,
    IsolationForestModel,
)
from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.ops import gpu_engine  # noqa: E402
from tests.conftest import GOLDEN  # noqa: E402

N_LIST = (1, 255, 256, 257, 513)


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


def fitted(dev, kind, d, T, **kw):
    """One GPU-fitted model per configuration, shared by the tests."""
    key = (kind, d, T, tuple(sorted(kw.items())))
    if key not in _MODELS:
        n_train = int(kw.pop("n_train", 600))
        X = torch.from_numpy(gauss(n_train, d, seed=100 + d)).to(dev)
        cls = IsolationForest if kind == "std" else ExtendedIsolationForest
        _MODELS[key] = cls(numEstimators=T, randomSeed=7 + T, **kw).fit(X)
    return _MODELS[key]


def oracle(model, X, finalize=True):
    fn = (cpu_engine.feature_contributions_extended
          if isinstance(model, ExtendedIsolationForestModel)
          else cpu_engine.feature_contributions)
    return fn(model.forest, X, finalize)


def as_input(X, bf16):
    """(torch rows of the requested dtype, the float32 matrix the kernel
    effectively sees)."""
    xt = torch.from_numpy(X)
    if bf16:
        xt = xt.to(torch.bfloat16)
    return xt, xt.float().numpy()


def check_bitwise(model, X, dev, bf16, finalize=True):
    xt, seen = as_input(X, bf16)
    got = model.feature_contributions(xt.to(dev), finalize=finalize)
    assert got.is_cuda and got.dtype == torch.float32
    assert tuple(got.shape) == X.shape
    got = got.cpu().numpy()
    want = oracle(model, seen, finalize)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (
        f"max |diff| {np.nanmax(np.abs(got - want)):.3e} over "
        f"{int((got.view(np.int32) != want.view(np.int32)).sum())} cells")
    return got


_EDGE_VALUES = np.concatenate([
    np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 3e-41,
              1.1754942e-38, -1.1754944e-38, 3e38, -3e38], dtype=np.float32),
    # denormals that are exact in bf16, so the bf16 variants keep them
    np.array([0x00010000, 0x00400000, 0x807F0000],
             dtype=np.uint32).view(np.float32),
])


def edge_rows(N, d, seed):
    rs = np.random.RandomState(seed)
    X = rs.normal(size=(N, d)).astype(np.float32)
    hit = rs.random_sample((N, d)) < 0.2
    X[hit] = _EDGE_VALUES[rs.randint(0, len(_EDGE_VALUES), size=(N, d))][hit]
    return X


class TestStandardBitwise:
    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    @pytest.mark.parametrize("T", [1, 5, 13])
    @pytest.mark.parametrize("d", [1, 5, 33])
    def test_shapes(self, dev, d, T, bf16):
        model = fitted(dev, "std", d, T)
        for N in N_LIST:
            check_bitwise(model, gauss(N, d, seed=N + d), dev, bf16)

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    def test_d200_global_accumulator_by_size(self, dev, bf16):
        model = fitted(dev, "std", 200, 5)
        for N in (257, 513):
            check_bitwise(model, gauss(N, 200, seed=N), dev, bf16)

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    def test_finalize_false_is_raw_sum(self, dev, bf16):
        model = fitted(dev, "std", 5, 13)
        X = gauss(300, 5, seed=3)
        raw = check_bitwise(model, X, dev, bf16, finalize=False)
        fin = check_bitwise(model, X, dev, bf16)
        assert np.array_equal((raw / np.float32(13)).astype(np.float32), fin)

    def test_forced_global_accumulator_equals_lds_route(self, dev,
                                                        monkeypatch):
        model = fitted(dev, "std", 5, 13)
        X = gauss(513, 5, seed=4)
        lds = check_bitwise(model, X, dev, False)
        monkeypatch.setenv("IFA_EXPLAIN_FORCE_GLOBAL_ACC", "1")
        glob = check_bitwise(model, X, dev, False)
        assert np.array_equal(lds.view(np.int32), glob.view(np.int32))
        xb = torch.from_numpy(X).to(torch.bfloat16)
        monkeypatch.delenv("IFA_EXPLAIN_FORCE_GLOBAL_ACC")
        a = model.feature_contributions(xb.to(dev)).cpu()
        monkeypatch.setenv("IFA_EXPLAIN_FORCE_GLOBAL_ACC", "1")
        b = model.feature_contributions(xb.to(dev)).cpu()
        assert torch.equal(a, b)

    @pytest.mark.parametrize("force_global", [False, True])
    def test_grid_stride_with_partial_last_tile(self, dev, monkeypatch,
                                                force_global):
        # 2 blocks over 1500 rows: every block loops, the last tile is short
        monkeypatch.setenv("IFA_EXPLAIN_MAX_BLOCKS", "2")
        if force_global:
            monkeypatch.setenv("IFA_EXPLAIN_FORCE_GLOBAL_ACC", "1")
        model = fitted(dev, "std", 5, 5)
        check_bitwise(model, gauss(1500, 5, seed=5), dev, False)
        check_bitwise(model, gauss(1500, 5, seed=5), dev, True)

    def test_max_samples_two(self, dev):
        model = fitted(dev, "std", 5, 13, maxSamples=2.0)
        assert int(model.forest.node_count.max()) <= 3
        for bf16 in (False, True):
            check_bitwise(model, gauss(513, 5, seed=6), dev, bf16)

    def test_deep_trees_take_global_node_route(self, dev):
        model = fitted(dev, "std", 5, 4, maxSamples=8192.0, n_train=20000)
        assert model.forest.max_nodes * 16 > 64 * 1024  # past LDS staging
        X = gauss(20000, 5, seed=100 + 5)
        check_bitwise(model, X, dev, False)
        check_bitwise(model, X[:3000], dev, True)

    def test_unsplit_columns_are_exactly_zero(self, dev):
        model = fitted(dev, "std", 6, 1, maxFeatures=0.5)
        f = model.forest.feature
        unused = sorted(set(range(6)) - set(f[f >= 0].tolist()))
        assert unused, "maxFeatures=0.5 must leave columns without a split"
        for bf16 in (False, True):
            got = check_bitwise(model, gauss(513, 6, seed=8), dev, bf16)
            assert (got[:, unused].view(np.int32) == 0).all()
            used = sorted(set(range(6)) - set(unused))
            assert np.abs(got[:, used]).max() > 0

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    @pytest.mark.parametrize("d", [5, 33, 200])
    def test_edge_value_rows(self, dev, d, bf16):
        model = fitted(dev, "std", d, 5)
        X = edge_rows(513, d, seed=9 + d)
        assert np.isnan(X).any() and np.isinf(X).any()
        check_bitwise(model, X, dev, bf16)

    def test_loaded_spark_model_f64_splits(self, dev, mammography):
        model = IsolationForestModel.load(
            os.path.join(GOLDEN, "savedIsolationForestModel"))
        X = np.ascontiguousarray(mammography[0][:513])
        for bf16 in (False, True):
            check_bitwise(model, X, dev, bf16)

    def test_pack_cache_keys_do_not_collide(self, dev):
        model = fitted(dev, "std", 5, 5)
        X = gauss(257, 5, seed=10)
        for bf16 in (False, True, False, True):
            check_bitwise(model, X, dev, bf16)
            # scoring in between shares the 4-entry pack cache
            s = model.score(as_input(X, bf16)[0].to(dev)).cpu().numpy()
            want = model.score(torch.from_numpy(as_input(X, bf16)[1])).numpy()
            assert np.array_equal(s.view(np.int32), want.view(np.int32))

    def test_identity_against_gpu_path_sums(self, dev):
        T = 13
        model = fitted(dev, "std", 5, T)
        X = torch.from_numpy(gauss(513, 5, seed=11)).to(dev)
        contrib = model.feature_contributions(X).cpu().numpy()
        ps = gpu_engine.score_forest(model, X, finalize=False).cpu().numpy()
        lhs = (model.expected_path_length
               + contrib.astype(np.float64).sum(axis=1))
        gap = float(np.abs(lhs - ps.astype(np.float64) / T).max())
        print(f"identity gap vs GPU path sums {gap:.3e}")
        # 8*19*T f32 adds, relative error 2^-24 each on partial sums bounded
        # by 19*T, divided by T (tests/test_explain_cpu.py)
        assert gap <= 152.0 * T * 2.0 ** -24

    def test_empty_input(self, dev):
        model = fitted(dev, "std", 5, 5)
        for dtype in (torch.float32, torch.bfloat16):
            out = model.feature_contributions(
                torch.empty((0, 5), dtype=dtype, device=dev))
            assert tuple(out.shape) == (0, 5) and out.dtype == torch.float32
            assert out.is_cuda

    def test_top_contributing_features_on_device(self, dev):
        model = fitted(dev, "std", 5, 13)
        X = torch.from_numpy(gauss(257, 5, seed=12)).to(dev)
        idx, val = model.top_contributing_features(X, 2)
        assert idx.is_cuda and val.is_cuda and idx.dtype == torch.int64
        contrib = model.feature_contributions(X).cpu().numpy()
        order = np.argsort(contrib, axis=1, kind="stable")[:, :2]
        assert np.array_equal(
            val.cpu().numpy(), np.take_along_axis(contrib, order, axis=1))


class TestExtendedBitwise:
    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    @pytest.mark.parametrize("d,level,T", [
        (1, 0, 13), (5, 0, 5), (5, 2, 1), (5, 4, 13), (33, 0, 13),
        (33, 16, 5), (33, 32, 13),
    ])
    def test_shapes_every_extension_level(self, dev, d, level, T, bf16):
        model = fitted(dev, "eif", d, T, extensionLevel=level)
        assert model.forest.nnz == level + 1
        for N in N_LIST:
            check_bitwise(model, gauss(N, d, seed=N + d + level), dev, bf16)

    @pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
    @pytest.mark.parametrize("level", [0, 2, 4])
    def test_edge_value_rows(self, dev, level, bf16):
        model = fitted(dev, "eif", 5, 5, extensionLevel=level)
        X = edge_rows(513, 5, seed=20 + level)
        check_bitwise(model, X, dev, bf16)

    def test_finalize_false_and_grid_stride(self, dev, monkeypatch):
        monkeypatch.setenv("IFA_EXPLAIN_MAX_BLOCKS", "2")
        model = fitted(dev, "eif", 5, 13, extensionLevel=4)
        X = gauss(1500, 5, seed=21)
        raw = check_bitwise(model, X, dev, False, finalize=False)
        fin = check_bitwise(model, X, dev, False)
        assert np.array_equal((raw / np.float32(13)).astype(np.float32), fin)

    def test_max_samples_two(self, dev):
        model = fitted(dev, "eif", 5, 13, extensionLevel=4, maxSamples=2.0)
        assert int(model.forest.node_count.max()) <= 3
        check_bitwise(model, gauss(513, 5, seed=22), dev, False)

    def test_loaded_spark_model(self, dev, mammography):
        model = ExtendedIsolationForestModel.load(
            os.path.join(GOLDEN, "savedExtendedIsolationForestModel"))
        X = np.ascontiguousarray(mammography[0][:513])
        for bf16 in (False, True):
            check_bitwise(model, X, dev, bf16)

    def test_empty_input(self, dev):
        model = fitted(dev, "eif", 5, 5, extensionLevel=2)
        out = model.feature_contributions(
            torch.empty((0, 5), dtype=torch.float32, device=dev))
        assert tuple(out.shape) == (0, 5) and out.dtype == torch.float32
