"""GPU tests (MI355X) for float16 rows on every GPU path: build, each scoring
route, attribution, the pack cache, the public API and the native CLI.

fp16 -> f32 is exact, so the oracle everywhere is the CPU engine on
``X16.float()`` and fp16 rows follow the f32 row contract of each route:
bitwise on the strict-order routes; on the reassociated dense routes the
fp16 run equals the f32 run on the upcast matrix bit for bit (same kernel,
same weights, same order) and non-finite rows equal the oracle bitwise.

The data holds +-0, fp16 subnormals (0x0001, 0x03FF, both signs), +-65504,
+-inf, NaN, and bit patterns that read differently as bf16 (0x3C00, 0x3F80,
0x4000), so an fp16 tensor that fell into a bf16 instantiation cannot pass.
N = 3000 is no multiple of any row tile.
"""

import copy
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from isolation_forest_amd import (  # noqa: E402
    ExtendedIsolationForest,
    IsolationForest,
)
from isolation_forest_amd.core import cpu_engine  # noqa: E402
from isolation_forest_amd.ops import gpu_engine  # noqa: E402
from isolation_forest_amd.utils.params import ResolvedParams  # noqa: E402
from tests.test_fp16_cpu import edge_rows16  # noqa: E402
from tests.test_gpu_edges import (  # noqa: E402
    Shell,
    _assert_bitwise,
    _assert_dense_contract,
    _bits,
    _c,
    _old_dense_predicate,
    _routed,
    _v4_config,
)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TRAIN = 2000
N_SCORE = 3000


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from isolation_forest_amd.ops import load_extension

    load_extension()  # hard error if missing on a GPU box
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------
# shared data, forests and oracles (computed once, never mutated)
# ---------------------------------------------------------------------------

_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _rows(N, d, seed, nonfinite):
    """(fp16 bits, exact f32 widening) with the planted edge cells."""
    def make():
        bits = edge_rows16(N, d, seed, nonfinite=nonfinite, reps=40)
        X32 = bits.view(np.float16).astype(np.float32)
        bits.setflags(write=False)
        X32.setflags(write=False)
        return bits, X32
    return _memo(("rows", N, d, seed, nonfinite), make)


def _train(d):
    return _rows(N_TRAIN, d, 1000 + d, False)


def _score(d):
    bits, X32 = _rows(N_SCORE, d, 2000 + d, True)
    assert (~np.isfinite(X32)).any(axis=1).sum() >= 60
    sub = (X32 != 0) & (np.abs(X32) < 2.0 ** -14)
    assert sub.any(axis=1).sum() >= 60
    return bits, X32


def _t16(bits, dev):
    """uint16 bit patterns -> torch.float16 tensor on the device."""
    t = torch.from_numpy(np.array(bits).view(np.float16)).to(dev)
    assert t.dtype == torch.float16
    return t


def _t32(X32, dev):
    return torch.from_numpy(np.array(X32)).to(dev)


def _bags(n, d, k, T, seed):
    bag = cpu_engine.sample_bags(N_TRAIN, T, n, seed=seed, bootstrap=False)
    fs = cpu_engine.feature_subsets(d, k, T, seed=seed)
    return bag, fs


def _std_forest(d, n=128, T=16, seed=17):
    def make():
        bag, fs = _bags(n, d, d, T, seed)
        return cpu_engine.build_forest(np.array(_train(d)[1]), bag, fs, seed,
                                       n, d, d)
    return _memo(("std", d, n, T, seed), make)


def _eif_forest(d, ext, n=128, T=16, seed=17):
    def make():
        bag, fs = _bags(n, d, d, T, seed)
        return cpu_engine.build_extended_forest(
            np.array(_train(d)[1]), bag, fs, seed, n, d, d, ext)
    return _memo(("eif", d, ext, n, T, seed), make)


def _oracle(forest, X32):
    def make():
        with np.errstate(all="ignore"):
            if hasattr(forest, "hyper_w"):
                ps = cpu_engine.path_lengths_extended(forest, X32)
            else:
                ps = cpu_engine.path_lengths(forest, X32)
        return forest, X32, ps
    return _memo(("oracle", id(forest), id(X32)), make)[2]


def _ext():
    from isolation_forest_amd.ops import load_extension

    return load_extension()


# ---------------------------------------------------------------------------
# 1. build
# ---------------------------------------------------------------------------


class TestBuild:
    def test_bag_gather_bitwise(self, dev):
        bits, X32 = _score(8)
        idx = cpu_engine.sample_bags(N_SCORE, 10, 64, seed=1,
                                     bootstrap=False)
        bags = _ext().bag_gather(_t16(bits, dev),
                                 torch.from_numpy(idx).to(dev))
        assert bags.dtype == torch.float32
        np.testing.assert_array_equal(_bits(bags), _bits(X32[idx]))

    @pytest.mark.parametrize("d", [3, 8])
    def test_standard_build_identical(self, dev, d):
        n, T, seed = 128, 16, 17
        bits, X32 = _train(d)
        bag, fs = _bags(n, d, d, T, seed)
        cpu_f = _std_forest(d, n, T, seed)
        rp = ResolvedParams(num_samples=n, num_features=d,
                            total_rows=N_TRAIN, total_features=d)
        gpu_f = gpu_engine.build_forest(_t16(bits, dev), bag, fs, seed, rp)
        for name in ["node_count", "feature", "right", "num_instances"]:
            np.testing.assert_array_equal(getattr(gpu_f, name),
                                          getattr(cpu_f, name), err_msg=name)
        np.testing.assert_array_equal(_bits(gpu_f.value), _bits(cpu_f.value))

    @pytest.mark.parametrize("d,ext", [(3, 0), (3, 2), (8, 0), (8, 2),
                                       (8, 7)])
    def test_extended_build_identical(self, dev, d, ext):
        n, T, seed = 128, 16, 17
        bits, X32 = _train(d)
        bag, fs = _bags(n, d, d, T, seed)
        cpu_f = _eif_forest(d, ext, n, T, seed)
        rp = ResolvedParams(num_samples=n, num_features=d,
                            total_rows=N_TRAIN, total_features=d,
                            extension_level=ext)
        gpu_f = gpu_engine.build_extended_forest(_t16(bits, dev), bag, fs,
                                                 seed, rp)
        for name in ["node_count", "feature", "right", "num_instances",
                     "hyper_idx"]:
            np.testing.assert_array_equal(getattr(gpu_f, name),
                                          getattr(cpu_f, name), err_msg=name)
        for name in ["hyper_w", "value"]:
            np.testing.assert_array_equal(_bits(getattr(gpu_f, name)),
                                          _bits(getattr(cpu_f, name)),
                                          err_msg=name)
        np.testing.assert_array_equal(gpu_f.offset64.view(np.int64),
                                      cpu_f.offset64.view(np.int64))


# ---------------------------------------------------------------------------
# 2. standard v4
# ---------------------------------------------------------------------------


def _score_std(shell, Xt):
    out, _ = _routed(gpu_engine.score_forest, shell, Xt, "score_forest")
    return out


class TestStandardV4:
    @pytest.mark.parametrize("switch", ["lds", "glob", "ilp8"])
    @pytest.mark.parametrize("d", [3, 8, 33])
    def test_bitwise(self, dev, monkeypatch, d, switch):
        if switch == "ilp8":
            monkeypatch.setenv("IFA_SCORE_ILP", "8")
        elif switch == "glob":
            monkeypatch.setenv("IFA_SCORE_FORCE_GLOBAL", "1")
        forest = _std_forest(d)
        # fp16 takes the 2-byte configuration, the same as bf16's
        cfg = _v4_config(d, forest.feature.shape[1], True)
        assert cfg["nodes_lds"] and cfg["rows_lds"] == (switch != "glob")
        assert cfg["ilp"] == (8 if switch == "ilp8" else 4)
        bits, X32 = _score(d)
        got = _score_std(Shell(forest), _t16(bits, dev))
        _assert_bitwise(got.cpu().numpy(), _oracle(forest, X32),
                        f"fp16 v4 d={d} {switch}")

    def test_finalized_scores_bitwise(self, dev):
        d = 8
        forest = _std_forest(d)
        bits, X32 = _score(d)
        got = gpu_engine.score_forest(Shell(forest), _t16(bits, dev),
                                      finalize=True).cpu().numpy()
        want = cpu_engine.scores_from_path_sums(
            _oracle(forest, X32), forest.num_trees, forest.num_samples)
        _assert_bitwise(got, want, "fp16 v4 finalized scores")

    def test_device_pack_equals_host_pack(self, dev):
        """A GPU-fit forest packs its thresholds on the device
        (_f16_threshold_keys_dev); the same forest in a fresh shell without
        the raw device tensors packs on the host. Same records, and both
        score bitwise."""
        n, d, T, seed = 128, 8, 16, 17
        bits, X32 = _train(d)
        bag, fs = _bags(n, d, d, T, seed)
        rp = ResolvedParams(num_samples=n, num_features=d,
                            total_rows=N_TRAIN, total_features=d)
        forest = gpu_engine.build_forest(_t16(bits, dev), bag, fs, seed, rp)
        assert forest._device_raw["device"] == str(dev)
        aos_d, nc_d, h_d = gpu_engine._nodes_packed_v4_device(
            forest._device_raw, forest.num_trees, d, "f16")
        aos_h, nc_h, h_h = gpu_engine._nodes_packed_v4(forest, d, "f16")
        np.testing.assert_array_equal(aos_d.cpu().numpy(), aos_h)
        np.testing.assert_array_equal(nc_d.cpu().numpy(), nc_h)
        assert h_d == h_h
        host = copy.copy(forest)
        del host._device_raw
        del host.depth_np
        sbits, S32 = _score(d)
        with np.errstate(all="ignore"):
            want = cpu_engine.path_lengths(forest, S32)
        for what, f in (("device pack", forest), ("host pack", host)):
            got = _score_std(Shell(f), _t16(sbits, dev))
            _assert_bitwise(got.cpu().numpy(), want, f"fp16 v4 {what}")


# ---------------------------------------------------------------------------
# 3. foreign splits
# ---------------------------------------------------------------------------


def _foreign_forest(d):
    """A hand-made 'foreign' forest: the structure of a built one, with
    float64 splits that no build of ours produces — strictly between two
    f32 neighbours, a hair above exact fp16 data values, below the smallest
    fp16 subnormal, and beyond +-65504."""
    def make():
        f = copy.deepcopy(_std_forest(d, seed=23))
        rs = np.random.RandomState(5)
        internal = f.feature >= 0
        v32 = f.value[internal].astype(np.float32)
        up = np.nextafter(v32, np.float32(np.inf)).astype(np.float64)
        v64 = (v32.astype(np.float64) + up) / 2.0  # between f32 neighbours
        kind = rs.randint(0, 10, size=v64.shape)
        x16 = np.array(_score(d)[1]).reshape(-1)
        x16 = x16[np.isfinite(x16)]
        pick = x16[rs.randint(0, len(x16), size=v64.shape)].astype(np.float64)
        v64 = np.where(kind == 1, pick, v64)              # exactly on a value
        v64 = np.where(kind == 2, pick * (1 + 2.0 ** -40) + 1e-300, v64)
        far = rs.choice([65504.0, 65504.0 + 1e-9, 65505.0, 70000.5, 1e6,
                         -65504.0, -65504.0 - 1e-9, -65505.0, -1e6, 1e-10,
                         -1e-10, 2.0 ** -25, 3e38, -3e38], size=v64.shape)
        v64 = np.where(kind == 3, far, v64)
        f.value64 = f.value64.copy()
        f.value64[internal] = v64
        f.value = f.value.copy()
        f.value[internal] = v64.astype(np.float32)
        assert (np.abs(f.value64[internal]) > 65504).sum() >= 20
        lift = f.value[internal].astype(np.float64) != f.value64[internal]
        assert lift.sum() >= 100
        return f
    return _memo(("foreign", d), make)


class TestForeignSplits:
    def test_f64_compare_oracle_bitwise(self, dev):
        d = 8
        forest = _foreign_forest(d)
        bits, X32 = _score(d)
        got = _score_std(Shell(forest), _t16(bits, dev))
        _assert_bitwise(got.cpu().numpy(), _oracle(forest, X32),
                        "fp16 rows, foreign f64 splits")


# ---------------------------------------------------------------------------
# 4. wide records
# ---------------------------------------------------------------------------


class TestWideRecords:
    def test_score_forest_wide(self, dev):
        d = 8
        forest = _foreign_forest(d)
        bits, X32 = _score(d)
        shell = Shell(forest)
        aos, _, ex = gpu_engine._device_forest(shell, dev,
                                               v4_key=("wide", "f16"))
        assert aos.shape[2] == 4
        got = _ext().score_forest_wide(_t16(bits, dev), aos, ex["height"],
                                       _c(forest), False)
        _assert_bitwise(got.cpu().numpy(), _oracle(forest, X32),
                        "fp16 score_forest_wide")

    def test_score_extended_wide(self, dev):
        d = 7
        forest = _eif_forest(d, 2)
        bits, X32 = _score(d)
        aos, _, ex = gpu_engine._device_forest(Shell(forest), dev,
                                               v4_key="eif_wide")
        got = _ext().score_extended_wide(_t16(bits, dev), aos, ex["hidx"],
                                         ex["hw"], _c(forest), False)
        _assert_bitwise(got.cpu().numpy(), _oracle(forest, X32),
                        "fp16 score_extended_wide")


# ---------------------------------------------------------------------------
# 5. EIF routes
# ---------------------------------------------------------------------------


def _score_eif(shell, Xt, expect):
    out, shapes = _routed(gpu_engine.score_extended_forest, shell, Xt,
                          expect)
    return out


class TestEifRoutes:
    def test_ext0_v4_and_nan_fallback(self, dev):
        d = 6
        forest = _eif_forest(d, 0)
        assert gpu_engine._eif0_eligible(forest, d)
        bits, X32 = _score(d)
        keep = ~np.isnan(X32).any(axis=1)
        nb, n32 = np.ascontiguousarray(bits[keep]), np.ascontiguousarray(
            X32[keep])
        assert np.isinf(n32).any(axis=1).sum() >= 30
        shell = Shell(forest)
        got = _score_eif(shell, _t16(nb, dev), "score_forest")
        with np.errstate(all="ignore"):
            want = cpu_engine.path_lengths_extended(forest, n32)
        _assert_bitwise(got.cpu().numpy(), want, "fp16 ext-0 on v4")
        assert np.isnan(X32).any()
        got = _score_eif(shell, _t16(bits, dev), "score_extended_sparse_v2")
        _assert_bitwise(got.cpu().numpy(), _oracle(forest, X32),
                        "fp16 ext-0 NaN batch on sparse v2")

    @pytest.mark.parametrize("nnz", [2, 5])
    def test_sparse_v2(self, dev, nnz):
        d = 7
        forest = _eif_forest(d, nnz - 1)
        assert forest.nnz == nnz
        bits, X32 = _score(d)
        got = _score_eif(Shell(forest), _t16(bits, dev),
                         "score_extended_sparse_v2")
        _assert_bitwise(got.cpu().numpy(), _oracle(forest, X32),
                        f"fp16 sparse v2 nnz={nnz}")

    def test_general_strict_order(self, dev):
        d = 12
        forest = _eif_forest(d, 5)
        assert forest.nnz == 6
        assert not _old_dense_predicate(forest, d)
        bits, X32 = _score(d)
        got = _score_eif(Shell(forest), _t16(bits, dev),
                         "score_extended_forest")
        _assert_bitwise(got.cpu().numpy(), _oracle(forest, X32),
                        "fp16 general kernel nnz=6 d=12")

    @pytest.mark.parametrize("d", [8, 32])
    def test_dense_v2(self, dev, d):
        forest = _eif_forest(d, d - 1)
        assert forest.nnz == d
        bits, X32 = _score(d)
        shell = Shell(forest)
        got16 = _score_eif(shell, _t16(bits, dev),
                           "score_extended_dense_v2").cpu().numpy()
        got32 = _score_eif(shell, _t32(X32, dev),
                           "score_extended_dense_v2").cpu().numpy()
        _assert_bitwise(got16, got32, f"fp16 vs f32 rows, dense v2 d={d}")
        nonfinite = (~np.isfinite(X32)).any(axis=1)
        assert nonfinite.sum() >= 60
        _assert_bitwise(got16[nonfinite], _oracle(forest, X32)[nonfinite],
                        f"fp16 dense v2 d={d}, non-finite rows")

    def test_densified(self, dev):
        d = 12
        forest = _eif_forest(d, 5)
        assert forest.nnz == 6
        bits, X32 = _score(d)
        fin = np.isfinite(X32).all(axis=1)
        fb, f32 = np.ascontiguousarray(bits[fin]), np.ascontiguousarray(
            X32[fin])
        shell = Shell(forest)
        got16 = _score_eif(shell, _t16(fb, dev),
                           "score_extended_dense_v2").cpu().numpy()
        got32 = _score_eif(shell, _t32(f32, dev),
                           "score_extended_dense_v2").cpu().numpy()
        _assert_bitwise(got16, got32, "fp16 vs f32 rows, densified d=12")

    def test_old_dense_kernel_d68(self, dev):
        """nnz = d = 68: past dense v2's d <= 64, the router falls to the
        score_extended_forest binding, which picks the old 4-chain dense
        kernel. The fp16 run must equal the f32 run on the upcast rows bit
        for bit, both are held to the dense contract of test_gpu_edges
        against the oracle on the upcast matrix, and (as the edge test of
        this route checks for f32) a prefix scores to the same bits."""
        d = 68
        forest = _eif_forest(d, d - 1, T=8)
        assert _old_dense_predicate(forest, d)
        bits, X32 = _rows(N_SCORE, d, 2000 + d, False)
        shell = Shell(forest)
        X16t = _t16(bits, dev)
        got16 = _score_eif(shell, X16t, "score_extended_forest")
        got32 = _score_eif(shell, _t32(X32, dev), "score_extended_forest")
        _assert_bitwise(got16.cpu().numpy(), got32.cpu().numpy(),
                        "fp16 vs f32 rows, old dense d=68")
        want = _oracle(forest, X32)
        _assert_dense_contract(got32, want, forest, X32, "old dense f32")
        _assert_dense_contract(got16, want, forest, X32, "old dense fp16")
        full = got16.view(torch.int32)
        for m in (1, 255, 257, 513):
            part = _score_eif(shell, X16t[:m].contiguous(),
                              "score_extended_forest").view(torch.int32)
            assert torch.equal(part, full[:m]), m


# ---------------------------------------------------------------------------
# 6. attribution
# ---------------------------------------------------------------------------

_MODELS = {}


def _fitted16(dev, kind, d, T, n_train=N_TRAIN, **kw):
    """One model per configuration, FIT ON fp16 ROWS on the GPU."""
    key = (kind, d, T, n_train, tuple(sorted(kw.items())))
    if key not in _MODELS:
        bits, _ = _rows(n_train, d, 1000 + d, False)
        cls = IsolationForest if kind == "std" else ExtendedIsolationForest
        _MODELS[key] = cls(numEstimators=T, randomSeed=7 + T, **kw).fit(
            _t16(bits, dev))
    return _MODELS[key]


def _check_explain(model, bits, X32, dev, what):
    fn = (cpu_engine.feature_contributions_extended
          if hasattr(model.forest, "hyper_w")
          else cpu_engine.feature_contributions)
    got = model.feature_contributions(_t16(bits, dev))
    assert got.is_cuda and got.dtype == torch.float32
    assert tuple(got.shape) == X32.shape
    got = got.cpu().numpy()
    with np.errstate(all="ignore"):
        want = fn(model.forest, np.array(X32), True)
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} cells differ from the oracle, max |diff| "
        f"{np.nanmax(np.abs(got - want)):.3e}")


class TestExplain:
    @pytest.mark.parametrize("force_global", [False, True],
                             ids=["lds-acc", "global-acc"])
    @pytest.mark.parametrize("d", [3, 8])
    @pytest.mark.parametrize("kind", ["std", "eif"])
    def test_bitwise(self, dev, monkeypatch, kind, d, force_global):
        if force_global:
            monkeypatch.setenv("IFA_EXPLAIN_FORCE_GLOBAL_ACC", "1")
        model = _fitted16(dev, kind, d, 16)
        bits, X32 = _score(d)
        _check_explain(model, bits, X32, dev, f"fp16 explain {kind} d={d}")

    def test_keys_from_global(self, dev):
        """Width past the 2-byte key tile (docs/DESIGN.md §8, route 3):
        maxSamples 256 -> 511 nodes * 16 B staged, and 256 rows of dpad
        2-byte keys no longer fit the 150 KB budget beside them."""
        d, T, N = 300, 4, 600
        model = _fitted16(dev, "std", d, T, n_train=N)
        mn = model.forest.feature.shape[1]
        dpad = d + 1
        while dpad % 4 != 2:
            dpad += 1
        assert mn * 16 <= 64 * 1024
        assert mn * 16 + 256 * dpad * 2 > 150 * 1024  # mode 2 for fp16
        bits, X32 = _rows(N, d, 2000 + d, True)
        _check_explain(model, bits, X32, dev, "fp16 explain keys-from-global")


# ---------------------------------------------------------------------------
# 7. pack-cache separation
# ---------------------------------------------------------------------------


class TestCacheSeparation:
    def test_f32_f16_bf16_f16_on_one_model(self, dev):
        d = 8
        forest = _std_forest(d)
        bits, X32 = _score(d)
        shell = Shell(forest)
        x16 = _t16(bits, dev)
        xb = x16.to(torch.bfloat16)  # RNE: drops 3 mantissa bits
        Xb32 = xb.float().cpu().numpy()
        assert (Xb32 != X32)[np.isfinite(X32)].mean() > 0.5
        with np.errstate(all="ignore"):
            want_b = cpu_engine.path_lengths(forest, Xb32)
        want = _oracle(forest, X32)
        for what, xt, w in (("f32", _t32(X32, dev), want),
                            ("fp16 after f32", x16, want),
                            ("bf16 after fp16", xb, want_b),
                            ("fp16 after bf16", x16, want)):
            got = _score_std(shell, xt)
            _assert_bitwise(got.cpu().numpy(), w, f"cache: {what}")
        kinds = sorted(k[2][1] for k in shell._gpu_forest_cache)
        assert kinds == ["bf16", "f16", "f32"]

    def test_explain_and_eif0_keys(self, dev):
        d = 6
        forest = _eif_forest(d, 0)
        bits, X32 = _rows(N_SCORE, d, 2000 + d, False)
        shell = Shell(forest)
        want = _oracle(forest, X32)
        for xt in (_t32(X32, dev), _t16(bits, dev), _t32(X32, dev)):
            got = _score_eif(shell, xt, "score_forest")
            _assert_bitwise(got.cpu().numpy(), want, f"eif0 {xt.dtype}")
        std = _fitted16(dev, "std", 8, 16)
        sb, S32 = _score(8)
        want = cpu_engine.feature_contributions(std.forest, np.array(S32))
        for xt in (_t32(S32, dev), _t16(sb, dev)):
            got = std.feature_contributions(xt).cpu().numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ---------------------------------------------------------------------------
# 8. public API end to end
# ---------------------------------------------------------------------------


class TestPublicApi:
    def _fit_pair(self, cls, dev, d, **kw):
        bits, X32 = _train(d)
        g = cls(numEstimators=32, contamination=0.02, randomSeed=5,
                **kw).fit(_t16(bits, dev))
        c = cls(numEstimators=32, contamination=0.02, randomSeed=5,
                **kw).fit(torch.from_numpy(np.array(X32)))
        return g, c, bits, X32

    def _check(self, g, c, bits, X32, dev):
        assert g.outlier_score_threshold == c.outlier_score_threshold
        assert 0.0 < g.outlier_score_threshold < 1.0
        out_g = g.transform(_t16(bits, dev))
        out_c = c.transform(torch.from_numpy(np.array(X32)))
        _assert_bitwise(out_g["outlierScore"].cpu().numpy(),
                        out_c["outlierScore"].numpy(), "transform scores")
        lab_g = out_g["predictedLabel"].cpu().numpy()
        np.testing.assert_array_equal(lab_g,
                                      out_c["predictedLabel"].numpy())
        assert 0 < lab_g.sum() < 0.05 * len(lab_g)
        # most negative contribution per row: index and value as the CPU's
        idx_c, val_c = c.top_contributing_features(
            torch.from_numpy(np.array(X32)), 2)
        contrib = c.feature_contributions(torch.from_numpy(np.array(X32)))
        srt = torch.sort(contrib, dim=1).values
        untied = ((srt[:, 0] < srt[:, 1]) & (srt[:, 1] < srt[:, 2])).numpy()
        assert untied.mean() > 0.95  # ties have no defined order
        idx_g, val_g = g.top_contributing_features(_t16(bits, dev), 2)
        np.testing.assert_array_equal(idx_g.cpu().numpy()[untied],
                                      idx_c.numpy()[untied])
        assert torch.equal(val_g.cpu().view(torch.int32),
                           val_c.view(torch.int32))

    def test_isolation_forest(self, dev):
        g, c, bits, X32 = self._fit_pair(IsolationForest, dev, 8)
        self._check(g, c, bits, X32, dev)

    def test_extended_isolation_forest(self, dev):
        # extensionLevel 2 -> nnz 3 scores on the strict-order sparse route,
        # whose scores (and so the threshold) are bitwise the CPU's
        g, c, bits, X32 = self._fit_pair(ExtendedIsolationForest, dev, 8,
                                         extensionLevel=2)
        self._check(g, c, bits, X32, dev)


# ---------------------------------------------------------------------------
# 9. native CLI --f16
# ---------------------------------------------------------------------------


class TestNativeCliF16:
    def test_cli_f16_matches_engine(self, dev, tmp_path):
        cli = os.path.join(REPO, "tools", "native", "ifa_score")
        if not os.path.exists(cli):
            subprocess.check_call(
                ["bash", os.path.join(REPO, "tools", "native", "build.sh")])
        d = 8
        bits, X32 = _train(d)
        sbits, S32 = _score(d)
        model = IsolationForest(numEstimators=50, randomSeed=13).fit(
            _t16(bits, dev))
        mdir = str(tmp_path / "m")
        model.save(mdir)
        xbin = str(tmp_path / "x.bin")
        np.array(sbits).astype("<u2").tofile(xbin)
        sbin = str(tmp_path / "s.bin")
        out = subprocess.run(
            [cli, mdir, xbin, str(N_SCORE), str(d), sbin, "--f16"],
            capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert "f16" in out.stderr
        cli_scores = np.fromfile(sbin, dtype="<f4")
        eng_scores = model.score(_t16(sbits, dev)).cpu().numpy()
        print("max |cli - engine| =",
              float(np.abs(cli_scores - eng_scores).max()))
        _assert_bitwise(cli_scores, eng_scores, "ifa_score --f16 vs engine")
