"""CPU tests for float16 rows: the fp16 key transform, the fp16 threshold
keys and the four packing routines with the fp16 kind (no GPU needed — numpy
mirrors of the device logic, as in test_score_packing.py).

fp16 -> f32 is exact, so every oracle here is the CPU engine on the upcast
matrix and every comparison is bitwise.
"""

import numpy as np
import pytest

from isolation_forest_amd.core import cpu_engine
from isolation_forest_amd.ops import gpu_engine
from isolation_forest_amd.ops.gpu_engine import (
    _eif0_packed_v4,
    _f16_key_tables,
    _f16_threshold_keys,
    _nodes_packed_explain,
    _nodes_packed_v4,
    _nodes_packed_wide,
)

ALL_BITS = np.arange(65536, dtype=np.uint32).astype(np.uint16)
ALL_F32 = ALL_BITS.view(np.float16).astype(np.float32)  # exact widening


def _stage_key_f16(bits16: np.ndarray) -> np.ndarray:
    """numpy mirror of the device key16_f16() staging transform, written out
    here independently of gpu_engine._key16_f16."""
    b = bits16.astype(np.uint32)
    m = b & np.uint32(0x7FFF)
    k = np.where(b & np.uint32(0x8000), np.uint32(0x7FFF) - m,
                 np.uint32(0x8000) + m).astype(np.uint32)
    k[m == 0] = np.uint32(0x8000)
    k[m > np.uint32(0x7C00)] = np.uint32(0xFFFF)
    return k


def _widen16(k: np.ndarray) -> np.ndarray:
    return (k.astype(np.uint32) << np.uint32(16)) | np.uint32(0xFFFF)


def _split_set(seed=0):
    """The seeded split set of the threshold check: normals, tiny values,
    exact fp16 values, and the edges of fp16's range."""
    rs = np.random.RandomState(seed)
    normals = rs.normal(size=3000).astype(np.float32)
    exact = rs.randint(0, 1 << 16, size=2000).astype(np.uint16).view(
        np.float16).astype(np.float32)
    exact = exact[~np.isnan(exact)]
    edges = np.array(
        [0.0, -0.0, 2.0 ** -24, -(2.0 ** -24), 65504.0, -65504.0, 65505.0,
         1e6, -1e6, 3e38, -3e38, np.inf, -np.inf,
         # beyond the issue's list: just inside/outside the subnormal step
         # and the overflow edge
         1e-10, -1e-10, 65520.0, -65505.0, 2.0 ** -25, 1.5 * 2.0 ** -24],
        dtype=np.float32)
    return np.concatenate([
        normals, (normals[:1000] * np.float32(1e-6)).astype(np.float32),
        exact, edges])


class TestF16Key:
    def test_order_preserving_exhaustive(self):
        k = _stage_key_f16(ALL_BITS)
        nan = np.isnan(ALL_F32)
        assert (k[nan] == 0xFFFF).all()
        assert not (k[~nan] == 0xFFFF).any()
        # +-0 share one key, +inf is 0xFC00
        assert k[0x0000] == k[0x8000] == 0x8000
        assert k[0x7C00] == 0xFC00
        # x < y  <=>  key(x) < key(y) over every pair of non-NaN patterns:
        # sorting by value makes keys non-decreasing, with equal keys exactly
        # where the values are equal
        v, kk = ALL_F32[~nan], k[~nan].astype(np.int64)
        order = np.argsort(v, kind="stable")
        dv, dk = np.diff(v[order]), np.diff(kk[order])
        np.testing.assert_array_equal(dv > 0, dk > 0)
        np.testing.assert_array_equal(dv == 0, dk == 0)

    def test_engine_mirror_agrees(self):
        np.testing.assert_array_equal(
            gpu_engine._key16_f16(ALL_BITS), _stage_key_f16(ALL_BITS))

    def test_tables(self):
        vals, keys = _f16_key_tables()
        assert len(vals) == len(keys) == 63489
        assert np.all(np.diff(vals) > 0)
        assert np.all(np.diff(keys.astype(np.int64)) > 0)
        # the table is exactly the set of keys the staging transform emits
        # for non-NaN input
        staged = np.unique(_stage_key_f16(ALL_BITS[~np.isnan(ALL_F32)]))
        np.testing.assert_array_equal(staged, keys)


class TestF16ThresholdKeys:
    def test_threshold_semantics_exhaustive(self):
        """widen(key(x)) < thr(s)  <=>  f32(x) < s, for all 65,536 x."""
        s = _split_set()
        t = _f16_threshold_keys(s)
        assert t.dtype == np.uint32 and (t & np.uint32(0xFFFF) == 0).all()
        xk = _widen16(_stage_key_f16(ALL_BITS))
        mism = 0
        for lo in range(0, len(s), 256):
            got = xk[None, :] < t[lo:lo + 256, None]
            with np.errstate(invalid="ignore"):
                expect = ALL_F32[None, :] < s[lo:lo + 256, None]
            mism += int((got != expect).sum())
        assert mism == 0

    def test_out_of_range_splits(self):
        t = _f16_threshold_keys(np.array(
            [65505.0, 1e6, 3e38, np.inf, -65505.0, -1e6, -3e38, 1e-10,
             2.0 ** -25, 0.0, -0.0], dtype=np.float32)) >> np.uint32(16)
        k = _stage_key_f16
        inf_key = k(np.array([0x7C00], dtype=np.uint16))[0]
        nmax_key = k(np.array([0xFBFF], dtype=np.uint16))[0]  # -65504
        sub_key = k(np.array([0x0001], dtype=np.uint16))[0]
        assert (t[:4] == inf_key).all()
        assert (t[4:7] == nmax_key).all()
        assert (t[7:9] == sub_key).all()
        assert (t[9:] == 0x8000).all()

    def test_sentinel_and_nan_never_left(self):
        t = _f16_threshold_keys(np.array([np.inf, np.nan], dtype=np.float32))
        assert not np.uint32(0xFFFFFFFF) < t[0]
        # a NaN split sends every row right, as `x < NaN` does
        assert not (_widen16(_stage_key_f16(ALL_BITS)) < t[1]).any()

    def test_kind_spellings(self):
        s = _split_set()[:50]
        np.testing.assert_array_equal(
            gpu_engine._threshold_keys(s, "f16"), _f16_threshold_keys(s))
        np.testing.assert_array_equal(
            gpu_engine._threshold_keys(s, True),
            gpu_engine._bf16_threshold_keys(s))
        np.testing.assert_array_equal(
            gpu_engine._threshold_keys(s, False), gpu_engine._key32(s))
        with pytest.raises(ValueError):
            gpu_engine._row_kind(np.float64)


def edge_rows16(N, d, seed, nonfinite=True, reps=6):
    """fp16 rows (as uint16 bits) with planted edge values: +-0, subnormals
    0x0001/0x03FF of both signs, +-65504, +-inf, NaN, and the patterns
    0x3C00/0x4000/0x3F80, which read 1.0/2.0/1.875 as fp16 but
    0.0078125/2.0/1.0 as bf16: they fall on different sides of the splits
    between, so an fp16 row walked with bf16 keys is caught.
    nonfinite=False leaves +-inf and NaN out; each pattern is planted in
    `reps` random cells."""
    rs = np.random.RandomState(seed)
    X = rs.normal(size=(N, d)).astype(np.float16)
    bits = X.view(np.uint16)
    planted = np.array(
        [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x7BFF, 0xFBFF,
         0x7C00, 0xFC00, 0x7E00, 0x3C00, 0x4000, 0x3F80], dtype=np.uint16)
    if not nonfinite:  # rows a forest can be fit on: drop +-inf and NaN
        planted = planted[(planted & 0x7C00) != 0x7C00]
    rows = rs.randint(0, N, size=reps * len(planted))
    cols = rs.randint(0, d, size=reps * len(planted))
    bits[rows, cols] = np.tile(planted, reps)
    return bits


def _std_forest(seed=11, T=8, n=64, d=5, N=1500):
    bits = edge_rows16(N, d, seed)
    X = bits.view(np.float16).astype(np.float32)
    # fit on finite rows only (the build scans min/max); score everything
    fin = np.isfinite(X).all(axis=1)
    Xf = np.ascontiguousarray(X[fin])
    bag = cpu_engine.sample_bags(len(Xf), T, n, seed=seed, bootstrap=False)
    fs = cpu_engine.feature_subsets(d, d, T, seed=seed)
    forest = cpu_engine.build_forest(Xf, bag, fs, seed, n, d, d)
    return bits, X, forest


def _keys_with_sentinel(bits):
    keys = _widen16(_stage_key_f16(bits.reshape(-1))).reshape(bits.shape)
    return np.concatenate(
        [keys, np.full((bits.shape[0], 1), 0xFFFFFFFF, dtype=np.uint32)],
        axis=1)


class TestPackedF16:
    def test_v4_walk_matches_oracle(self):
        bits, X, forest = _std_forest()
        oracle = cpu_engine.path_lengths(forest, X)
        d = X.shape[1]
        packed, ncount, max_depth = _nodes_packed_v4(forest, d, "f16")
        assert packed.shape[0] % 8 == 0
        w0 = packed[:, :, 0]
        w1 = packed[:, :, 1].view(np.uint32)
        keys = _keys_with_sentinel(bits)
        rows = np.arange(X.shape[0])
        total = np.zeros(X.shape[0], dtype=np.float32)
        for t in range(forest.num_trees):
            cur = np.zeros(X.shape[0], dtype=np.int64)
            for _ in range(max_depth):
                f = w0[t, cur] & 0xFFF
                right = (w0[t, cur] >> 12) & 0x7FFF
                cur = np.where(keys[rows, f] < w1[t, cur], cur + 1, right)
            total = (total + w1[t, cur].view(np.float32)).astype(np.float32)
        np.testing.assert_array_equal(total.view(np.int32),
                                      oracle.view(np.int32))

    def test_v4_differs_from_bf16_pack(self):
        """The fp16 pack is not the bf16 pack: a cache or template mix-up
        cannot hide behind equal records."""
        _, _, forest = _std_forest()
        a, _, _ = _nodes_packed_v4(forest, 5, "f16")
        b, _, _ = _nodes_packed_v4(forest, 5, "bf16")
        c, _, _ = _nodes_packed_v4(forest, 5, True)
        np.testing.assert_array_equal(b, c)
        assert (a[..., 1] != b[..., 1]).any()
        np.testing.assert_array_equal(a[..., 0], b[..., 0])

    def test_wide_walk_matches_oracle(self):
        bits, X, forest = _std_forest(seed=12)
        oracle = cpu_engine.path_lengths(forest, X)
        packed, max_depth = _nodes_packed_wide(forest, "f16")
        feat, right_, w = packed[..., 0], packed[..., 1], packed[..., 2]
        wk = w.view(np.uint32)
        keys = _keys_with_sentinel(bits)
        rows = np.arange(X.shape[0])
        total = np.zeros(X.shape[0], dtype=np.float32)
        for t in range(forest.num_trees):
            cur = np.zeros(X.shape[0], dtype=np.int64)
            for _ in range(max_depth):
                leaf = right_[t, cur] == cur
                f = np.where(leaf, 0, feat[t, cur])
                left = keys[rows, f] < wk[t, cur]
                nxt = np.where(left, cur + 1, right_[t, cur])
                cur = np.where(leaf, cur, nxt)
            total = (total + w[t, cur].view(np.float32)).astype(np.float32)
        np.testing.assert_array_equal(total.view(np.int32),
                                      oracle.view(np.int32))

    @pytest.mark.parametrize("finalize", [False, True])
    def test_explain_walk_matches_oracle(self, finalize):
        bits, X, forest = _std_forest(seed=13)
        oracle = cpu_engine.feature_contributions(forest, X, finalize)
        d = X.shape[1]
        packed, max_depth = _nodes_packed_explain(forest, d, "f16")
        w0 = packed[..., 0]
        w1 = packed[..., 1].view(np.uint32)
        dl = packed[..., 2].view(np.float32)
        dr = packed[..., 3].view(np.float32)
        keys = _keys_with_sentinel(bits)
        rows = np.arange(X.shape[0])
        acc = np.zeros((X.shape[0], d + 1), dtype=np.float32)
        for t in range(forest.num_trees):
            cur = np.zeros(X.shape[0], dtype=np.int64)
            for _ in range(max_depth):
                f = w0[t, cur] & 0xFFF
                right = (w0[t, cur] >> 12) & 0x7FFF
                left = keys[rows, f] < w1[t, cur]
                delta = np.where(left, dl[t, cur], dr[t, cur])
                acc[rows, f] = (acc[rows, f] + delta).astype(np.float32)
                cur = np.where(left, cur + 1, right)
        got = acc[:, :d]
        if finalize:
            got = (got / np.float32(forest.num_trees)).astype(np.float32)
        np.testing.assert_array_equal(
            np.ascontiguousarray(got).view(np.int32), oracle.view(np.int32))


class TestEif0MirrorPackF16:
    """fp16 analogue of test_score_packing.TestEif0MirrorPack: the mirrored
    ext-0 pack over the fp16 key table makes the unmodified v4 walk
    reproduce cpu_engine.path_lengths_extended bitwise on non-NaN rows."""

    def _forest(self, seed, foreign):
        rs = np.random.RandomState(seed)
        d = 5
        bits = edge_rows16(2000, d, seed)
        X = bits.view(np.float16).astype(np.float32)
        keep = ~np.isnan(X).any(axis=1)
        bits, X = np.ascontiguousarray(bits[keep]), np.ascontiguousarray(
            X[keep])
        fin = np.isfinite(X).all(axis=1)
        Xf = np.ascontiguousarray(X[fin])
        bag = cpu_engine.sample_bags(len(Xf), 8, 64, seed=seed,
                                     bootstrap=False)
        fs = cpu_engine.feature_subsets(d, d, 8, seed=seed)
        forest = cpu_engine.build_extended_forest(Xf, bag, fs, seed, 64, d,
                                                  d, 0)
        internal = forest.feature >= 0
        # our builds draw w = +-1: both signs must be present
        w = forest.hyper_w[..., 0][internal]
        assert (w > 0).any() and (w < 0).any()
        if foreign:
            fw = rs.choice([0.5, -3.7, 1e-3, -1e4, 2.0, -1e-20],
                           internal.sum()).astype(np.float32)
            forest.hyper_w[..., 0][internal] = fw
        return forest, bits, X

    @pytest.mark.parametrize("foreign", [False, True])
    def test_walk_matches_oracle(self, foreign):
        forest, bits, X = self._forest(21 + int(foreign), foreign)
        with np.errstate(all="ignore"):
            oracle = cpu_engine.path_lengths_extended(forest, X)
        d = X.shape[1]
        packed, ncount, max_depth = _eif0_packed_v4(forest, d, "f16")
        w0 = packed[:, :, 0]
        w1 = packed[:, :, 1].view(np.uint32).astype(np.uint64)
        keys = _keys_with_sentinel(bits).astype(np.uint64)
        rows = np.arange(X.shape[0])
        total = np.zeros(X.shape[0], dtype=np.float32)
        for t in range(forest.num_trees):
            cur = np.zeros(X.shape[0], dtype=np.int64)
            for _ in range(max_depth):
                f = w0[t, cur] & 0xFFF
                right = (w0[t, cur] >> 12) & 0x7FFF
                cur = np.where(keys[rows, f] < w1[t, cur], cur + 1, right)
            total = (total + packed[t, cur, 1].view(np.float32)).astype(
                np.float32)
        np.testing.assert_array_equal(total.view(np.int32),
                                      oracle.view(np.int32))
