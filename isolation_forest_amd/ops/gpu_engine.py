"""GPU engine orchestration: device builds and scoring via the HIP extension.

The canonical forest lives in host numpy (core/forest.py) — it is small
(MBs) next to the data (GBs-TBs). Bags/feature subsets are drawn host-side
with the same Philox counters the kernels use, so a GPU-built forest is
BIT-IDENTICAL to the CPU oracle's for the same seed (tests/test_gpu.py
enforces this). Bags of up to 16384 rows build with the one-wave LDS kernels
(build_forest / build_extended_forest); larger ones with the multi-wave
global-memory kernels (build_forest_large / build_extended_forest_large),
which read X in place and give the same forest.

Scoring packs (the v4 integer-key node format, EIF dense/sparse variants)
are built ON DEVICE with torch ops from the raw build outputs (depths come
from the build kernels) and cached per model+device; the numpy host pack
is the fallback for loaded models and is bitwise-identical
(tests/test_gpu.py::TestDevicePacking). EIF scoring routes by hyperplane
width and dtype (score_extended_forest):

* nnz == 1 (extensionLevel 0) -> the STANDARD v4 walk via exact key
  thresholds + mirrored subtrees (_eif0_packed_v4; bitwise; NaN rows
  fall through to the strict kernels),
* nnz <= 5 uniform -> sparse v2 (bitwise strict j-order),
* densifiable (nnz == d or nnz >= 6): bf16 rows -> dense v3 (packed
  bf16 weights, d <= 128), f32 and fp16 rows -> dense v2 (d <= 64; fp16
  rows widen exactly to f32 at load) — tolerance contracts per PARITY.md; a batch with a non-finite cell and nnz < d
  skips the densified route (0 * inf = NaN) for the general kernel,
* otherwise (wide d, ragged widths, LDS overflow) -> the general
  strict-order kernel; forests past the packed 15-bit-node/12-bit-
  feature caps use the wide int4 kernels.
"""

from __future__ import annotations

import logging
import math
import os

import numpy as np
import torch

from ..core.forest import ExtendedForest, Forest
from ..utils.math import avg_path_length
from . import load_extension


_log = logging.getLogger(__name__)


def _row_layout(X: torch.Tensor):
    """Classify a 2-D row view for the kernels, which address
    ``X[r * rs + c * cs]`` with ``(rs, cs) = X.stride()``.

    ``"row"``: pitched row-major, ``cs == 1`` and ``rs >= d`` (packed is
    ``rs == d``). ``"feature"``: feature-major, ``rs == 1`` and ``cs >= N``
    (a ``[d, N]`` buffer seen through ``.T``, a Fortran-ordered array).
    ``None``: anything else (both strides != 1, stride 0 from ``expand``,
    overlapping rows), which needs a packed copy. The stride torch reports
    for a size-1 dimension is arbitrary and ignored; a view that fits both
    layouts is ``"row"``. Pure stride arithmetic: works on CPU tensors too.
    Mirrors ``check_x_layout`` in ops/hip/bindings.cpp.
    """
    N, d = int(X.shape[0]), int(X.shape[1])
    rs, cs = X.stride()
    if (d <= 1 or cs == 1) and (N <= 1 or rs >= d):
        return "row"
    if (N <= 1 or rs == 1) and (d <= 1 or cs >= N):
        return "feature"
    return None


def _rows_in_place(X: torch.Tensor) -> torch.Tensor:
    """X itself when the kernels can read it where it lies (no copy of the
    matrix is made), else one packed row-major copy."""
    if _row_layout(X) is not None:
        return X
    _log.debug("rows with strides %s (shape %s) are not consumable in place: "
               "making one contiguous copy", tuple(X.stride()),
               tuple(X.shape))
    return X.contiguous()


def _leaf_lut(n: int, device) -> torch.Tensor:
    lut = avg_path_length(np.arange(n + 1))
    return torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float32)).to(device)


def _mask_padding(feature, right, count, ncount, pad):
    cols = np.arange(feature.shape[1], dtype=np.int32)[None, :]
    live = cols < ncount[:, None]
    feature[~live] = pad
    right[~live] = -1
    count[~live] = -1
    return live


def build_forest(X: torch.Tensor, bag_idx: np.ndarray, feat_sub: np.ndarray,
                 seed: int, rp, tree_id_offset: int = 0) -> Forest:
    ext = load_extension()
    device = X.device
    n = rp.num_samples
    height_limit = int(math.ceil(math.log2(max(n, 2))))
    max_nodes = 2 * n - 1
    bag_t = torch.from_numpy(np.ascontiguousarray(bag_idx)).to(device)
    fs_t = torch.from_numpy(np.ascontiguousarray(feat_sub, dtype=np.int32)).to(device)
    bags = ext.bag_gather(_rows_in_place(X), bag_t)
    feat, value, right, count, ncount, depth = ext.build_forest(
        bags, fs_t, seed, tree_id_offset, _leaf_lut(n, device), max_nodes,
        height_limit,
    )
    f_np = feat.cpu().numpy()
    v_np = value.cpu().numpy()
    r_np = right.cpu().numpy()
    c_np = count.cpu().numpy().astype(np.int64)
    nc_np = ncount.cpu().numpy()
    _mask_padding(f_np, r_np, c_np, nc_np, Forest.PAD)
    v_np = np.where(f_np >= 0, v_np, np.where(f_np == Forest.LEAF, v_np, 0.0)).astype(
        np.float32
    )
    forest = Forest(
        feature=f_np,
        value=v_np,
        right=r_np,
        num_instances=c_np,
        node_count=nc_np.astype(np.int32),
        num_samples=n,
        num_features=rp.num_features,
        total_num_features=rp.total_features,
        value64=np.where(f_np >= 0, v_np, 0.0).astype(np.float64),
    )
    # raw device tensors for scoring-pack reuse (skips the host round trip);
    # depth_np additionally travels through the forest all-gather so
    # multi-rank fits keep the device packing path
    forest._device_raw = {
        "device": str(device), "feat": feat, "value": value, "right": right,
        "ncount": ncount, "depth": depth,
    }
    forest.depth_np = depth.cpu().numpy()
    return forest


def build_extended_forest(X: torch.Tensor, bag_idx: np.ndarray,
                          feat_sub: np.ndarray, seed: int, rp,
                          tree_id_offset: int = 0) -> ExtendedForest:
    ext = load_extension()
    device = X.device
    n = rp.num_samples
    height_limit = int(math.ceil(math.log2(max(n, 2))))
    max_nodes = 2 ** (height_limit + 1) - 1
    nnz = min(rp.extension_level + 1, rp.num_features)
    bag_t = torch.from_numpy(np.ascontiguousarray(bag_idx)).to(device)
    fs_t = torch.from_numpy(np.ascontiguousarray(feat_sub, dtype=np.int32)).to(device)
    bags = ext.bag_gather(_rows_in_place(X), bag_t)
    (feat, value, right, count, ncount, hidx, hw, off64,
     depth) = ext.build_extended_forest(
        bags, fs_t, seed, tree_id_offset, _leaf_lut(n, device), nnz, max_nodes,
        height_limit,
    )
    f_np = feat.cpu().numpy()
    v_np = value.cpu().numpy()
    r_np = right.cpu().numpy()
    c_np = count.cpu().numpy().astype(np.int64)
    nc_np = ncount.cpu().numpy()
    live = _mask_padding(f_np, r_np, c_np, nc_np, ExtendedForest.PAD)
    v_np = np.where(live, v_np, 0.0).astype(np.float32)
    hidx_np = hidx.cpu().numpy()
    hw_np = hw.cpu().numpy()
    off64_np = off64.cpu().numpy()
    internal = (f_np >= 0) & live
    hidx_np[~internal] = 0
    hw_np[~internal] = 0.0
    off64_np[~internal] = 0.0
    fr = ExtendedForest(
        feature=f_np,
        value=v_np,
        right=r_np,
        num_instances=c_np,
        node_count=nc_np.astype(np.int32),
        hyper_idx=hidx_np,
        hyper_w=hw_np,
        offset64=off64_np,
        num_samples=n,
        num_features=rp.num_features,
        total_num_features=rp.total_features,
        extension_level=rp.extension_level,
    )
    fr._device_raw = {
        "device": str(device), "feat": feat, "value": value, "right": right,
        "ncount": ncount, "depth": depth, "hidx": hidx, "hw": hw,
    }
    fr.depth_np = depth.cpu().numpy()
    return fr


# ---------------------------------------------------------------------------
# large-bag builds (maxSamples > 16384)
# ---------------------------------------------------------------------------

# Device bytes one launch of a large builder may allocate next to X: the row-id
# scratch (8 * n per tree), the chunk's int64 bag indices (8 * n per tree) and
# its raw outputs (max_nodes * (28 [+ 8 * nnz]) per tree). Trees are built in
# chunks that fit (always at least one tree); chunks are tree shards, which
# concatenate bitwise. 8 GiB keeps a standard 1M-row bag at ~150 trees per
# launch on a 288 GB card and leaves the matrix its memory.
BUILD_LARGE_BUDGET_BYTES = 8 << 30

# Threads per tree block of the large builders (profiles/build_large.md).
BUILD_LARGE_THREADS = 256


def large_build_fits(X: torch.Tensor, n: int) -> bool:
    """Whether the large builders take bags of ``n`` rows of ``X``: they keep
    row ids as uint32 and node ids as int32 (the bindings check the same)."""
    return int(X.shape[0]) <= 1 << 32 and n <= 1 << 30


def _large_chunk_trees(T: int, per_tree_bytes: int, chunk_trees) -> int:
    if chunk_trees is None:
        chunk_trees = BUILD_LARGE_BUDGET_BYTES // max(per_tree_bytes, 1)
    chunk_trees = int(chunk_trees)
    if chunk_trees < 1:
        if chunk_trees < 0:
            raise ValueError("chunk_trees must be positive")
        chunk_trees = 1
    return min(T, chunk_trees)


def _large_threads() -> int:
    v = os.environ.get("IFA_BUILD_LARGE_THREADS")
    return int(v) if v else BUILD_LARGE_THREADS


def build_forest_large(X: torch.Tensor, bag_idx: np.ndarray,
                       feat_sub: np.ndarray, seed: int, rp,
                       tree_id_offset: int = 0, chunk_trees=None,
                       return_depth: bool = False):
    """``build_forest`` for bags of any size (the models use it above the
    LDS builders' 16384 rows): rows are read in place from ``X``, no f32
    ``[T, n, d]`` gather is made, and the trees are built ``chunk_trees`` at
    a time (``None``: as many as ``BUILD_LARGE_BUDGET_BYTES`` holds). The
    forest is bitwise ``cpu_engine.build_forest``'s. It carries no device
    tensors: forests this size score through the host-packed wide formats.
    ``return_depth=True`` returns ``(forest, depth)`` with the kernel's
    per-node depths ``[T, max_nodes]``."""
    ext = load_extension()
    device = X.device
    n = rp.num_samples
    height_limit = int(math.ceil(math.log2(max(n, 2))))
    max_nodes = 2 * n - 1
    T = int(bag_idx.shape[0])
    Xr = _rows_in_place(X)
    lut = _leaf_lut(n, device)
    fs = np.ascontiguousarray(feat_sub, dtype=np.int32)
    chunk = _large_chunk_trees(T, 16 * n + 28 * max_nodes, chunk_trees)
    f_np = np.empty((T, max_nodes), dtype=np.int32)
    v_np = np.empty((T, max_nodes), dtype=np.float32)
    r_np = np.empty((T, max_nodes), dtype=np.int32)
    c_np = np.empty((T, max_nodes), dtype=np.int64)
    nc_np = np.empty((T,), dtype=np.int32)
    d_np = np.empty((T, max_nodes), dtype=np.int32) if return_depth else None
    for lo in range(0, T, chunk):
        hi = min(T, lo + chunk)
        bag_t = torch.from_numpy(np.ascontiguousarray(bag_idx[lo:hi])).to(device)
        fs_t = torch.from_numpy(fs[lo:hi]).to(device)
        feat, value, right, count, ncount, depth = ext.build_forest_large(
            Xr, bag_t, fs_t, seed, tree_id_offset + lo, lut, max_nodes,
            height_limit, _large_threads())
        f_np[lo:hi] = feat.cpu().numpy()
        v_np[lo:hi] = value.cpu().numpy()
        r_np[lo:hi] = right.cpu().numpy()
        c_np[lo:hi] = count.cpu().numpy()
        nc_np[lo:hi] = ncount.cpu().numpy()
        if return_depth:
            d_np[lo:hi] = depth.cpu().numpy()
        del bag_t, fs_t, feat, value, right, count, ncount, depth
    _mask_padding(f_np, r_np, c_np, nc_np, Forest.PAD)
    v_np = np.where(f_np >= 0, v_np, np.where(f_np == Forest.LEAF, v_np, 0.0)).astype(
        np.float32
    )
    forest = Forest(
        feature=f_np,
        value=v_np,
        right=r_np,
        num_instances=c_np,
        node_count=nc_np,
        num_samples=n,
        num_features=rp.num_features,
        total_num_features=rp.total_features,
        value64=np.where(f_np >= 0, v_np, 0.0).astype(np.float64),
    )
    return (forest, d_np) if return_depth else forest


def build_extended_forest_large(X: torch.Tensor, bag_idx: np.ndarray,
                                feat_sub: np.ndarray, seed: int, rp,
                                tree_id_offset: int = 0, chunk_trees=None,
                                return_depth: bool = False):
    """``build_extended_forest`` for bags of any size; see
    ``build_forest_large``."""
    ext = load_extension()
    device = X.device
    n = rp.num_samples
    height_limit = int(math.ceil(math.log2(max(n, 2))))
    max_nodes = 2 ** (height_limit + 1) - 1
    nnz = min(rp.extension_level + 1, rp.num_features)
    T = int(bag_idx.shape[0])
    Xr = _rows_in_place(X)
    lut = _leaf_lut(n, device)
    fs = np.ascontiguousarray(feat_sub, dtype=np.int32)
    chunk = _large_chunk_trees(
        T, 16 * n + (28 + 8 * nnz) * max_nodes, chunk_trees)
    f_np = np.empty((T, max_nodes), dtype=np.int32)
    v_np = np.empty((T, max_nodes), dtype=np.float32)
    r_np = np.empty((T, max_nodes), dtype=np.int32)
    c_np = np.empty((T, max_nodes), dtype=np.int64)
    nc_np = np.empty((T,), dtype=np.int32)
    hidx_np = np.empty((T, max_nodes, nnz), dtype=np.int32)
    hw_np = np.empty((T, max_nodes, nnz), dtype=np.float32)
    off64_np = np.empty((T, max_nodes), dtype=np.float64)
    d_np = np.empty((T, max_nodes), dtype=np.int32) if return_depth else None
    for lo in range(0, T, chunk):
        hi = min(T, lo + chunk)
        bag_t = torch.from_numpy(np.ascontiguousarray(bag_idx[lo:hi])).to(device)
        fs_t = torch.from_numpy(fs[lo:hi]).to(device)
        (feat, value, right, count, ncount, hidx, hw, off64,
         depth) = ext.build_extended_forest_large(
            Xr, bag_t, fs_t, seed, tree_id_offset + lo, lut, nnz, max_nodes,
            height_limit, _large_threads())
        f_np[lo:hi] = feat.cpu().numpy()
        v_np[lo:hi] = value.cpu().numpy()
        r_np[lo:hi] = right.cpu().numpy()
        c_np[lo:hi] = count.cpu().numpy()
        nc_np[lo:hi] = ncount.cpu().numpy()
        hidx_np[lo:hi] = hidx.cpu().numpy()
        hw_np[lo:hi] = hw.cpu().numpy()
        off64_np[lo:hi] = off64.cpu().numpy()
        if return_depth:
            d_np[lo:hi] = depth.cpu().numpy()
        del (bag_t, fs_t, feat, value, right, count, ncount, hidx, hw, off64,
             depth)
    live = _mask_padding(f_np, r_np, c_np, nc_np, ExtendedForest.PAD)
    v_np = np.where(live, v_np, 0.0).astype(np.float32)
    internal = (f_np >= 0) & live
    hidx_np[~internal] = 0
    hw_np[~internal] = 0.0
    off64_np[~internal] = 0.0
    fr = ExtendedForest(
        feature=f_np,
        value=v_np,
        right=r_np,
        num_instances=c_np,
        node_count=nc_np,
        hyper_idx=hidx_np,
        hyper_w=hw_np,
        offset64=off64_np,
        num_samples=n,
        num_features=rp.num_features,
        total_num_features=rp.total_features,
        extension_level=rp.extension_level,
    )
    return (fr, d_np) if return_depth else fr


# ---------------------------------------------------------------------------
# scoring
# ---------------------------------------------------------------------------


# Row dtype kinds. The packing routines and cache keys below take a `kind`:
# "f32", "bf16" or "f16". The bool spelling (False = f32, True = bf16)
# predates fp16 rows and is still accepted everywhere.
_ROW_KINDS = {
    torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16",
    False: "f32", True: "bf16", "f32": "f32", "bf16": "bf16", "f16": "f16",
}


def _row_kind(x) -> str:
    """Normalise a torch dtype / bool / kind string to the kind string."""
    try:
        return _ROW_KINDS[x]
    except (KeyError, TypeError):
        raise ValueError(f"unsupported row dtype {x!r}: GPU rows are float32, "
                         "bfloat16 or float16") from None


def _threshold_keys(split_vals: np.ndarray, kind) -> np.ndarray:
    """Integer key thresholds (u32) of f32 split values for a row kind."""
    kind = _row_kind(kind)
    if kind == "bf16":
        return _bf16_threshold_keys(split_vals)
    if kind == "f16":
        return _f16_threshold_keys(split_vals)
    return _key32(split_vals)


_BF16_KEY_TABLES = None
_F16_KEY_TABLES = None


def _bf16_key_tables():
    """(values, keys) of every producible bf16 KEY, value-ascending.

    The key transform is the device's key16(): order-preserving u16 with
    +-0 collapsed to 0x8000 and NaN at 0xFFFF. 'Producible' = what the
    staging transform can emit for non-NaN input: finite and +-inf keys,
    excluding 0x7FFF (-0 maps to +0's key)."""
    global _BF16_KEY_TABLES
    if _BF16_KEY_TABLES is None:
        keys = np.arange(65536, dtype=np.uint32)
        pos = keys >= 0x8000
        bits = np.where(pos, keys - 0x8000,
                        0x8000 + (0x7FFF - keys)).astype(np.uint32)
        vals = (bits << np.uint32(16)).view(np.float32)
        ok = np.isfinite(vals) | np.isinf(vals)
        ok[0x7FFF] = False  # -0's raw key: never staged
        _BF16_KEY_TABLES = (vals[ok].copy(), keys[ok].astype(np.uint32))
    return _BF16_KEY_TABLES


def _key16_f16(bits: np.ndarray) -> np.ndarray:
    """Order-preserving u16 key of fp16 BIT patterns (device key16_f16()):
    the bf16 sign-magnitude fold, with NaN at m > 0x7C00."""
    b = np.asarray(bits).astype(np.uint32)
    m = b & np.uint32(0x7FFF)
    k = np.where(b & np.uint32(0x8000),
                 np.uint32(0x7FFF) - m,
                 np.uint32(0x8000) + m).astype(np.uint32)
    k[m == 0] = np.uint32(0x8000)
    k[m > np.uint32(0x7C00)] = np.uint32(0xFFFF)
    return k


def _f16_key_tables():
    """(values, keys) of every producible fp16 KEY, value-ascending: the
    63,489 keys of finite and +-inf fp16 values, without 0x7FFF (-0 maps to
    +0's key). Values are the exact f32 widenings."""
    global _F16_KEY_TABLES
    if _F16_KEY_TABLES is None:
        keys = np.arange(65536, dtype=np.uint32)
        pos = keys >= 0x8000
        bits = np.where(pos, keys - 0x8000,
                        0x8000 + (0x7FFF - keys)).astype(np.uint16)
        vals = bits.view(np.float16).astype(np.float32)
        ok = ~np.isnan(vals)
        ok[0x7FFF] = False  # -0's raw key: never staged
        _F16_KEY_TABLES = (vals[ok].copy(), keys[ok].astype(np.uint32))
    return _F16_KEY_TABLES


def _f16_threshold_keys(split_vals: np.ndarray) -> np.ndarray:
    """Smallest producible fp16 key whose value is >= the f32 split value,
    shifted into the high 16 bits (kernel compares widened keys), so that
    widen(key(x)) < threshold  <=>  f32(x) < s  for every fp16 x.

    Table + searchsorted(side="left"). Splits outside fp16's range (foreign
    models) land where they must: s > 65504 -> the +inf key, s < -65504 ->
    the key of -65504, 0 < s < 2^-24 -> the smallest subnormal's key. A NaN
    split sorts past the table and gets key 0: nothing compares below it,
    as `x < NaN` is false in the oracle."""
    vals, keys = _f16_key_tables()
    s = np.ascontiguousarray(split_vals, dtype=np.float32)
    idx = np.searchsorted(vals, s, side="left")
    keys_ext = np.append(keys, np.uint32(0))
    return keys_ext[idx].astype(np.uint32) << np.uint32(16)


def _key32(vals: np.ndarray) -> np.ndarray:
    """Order-preserving u32 key of f32 values (device key32())."""
    b = np.ascontiguousarray(vals, dtype=np.float32).view(np.uint32)
    m = b & np.uint32(0x7FFFFFFF)
    k = np.where(b & np.uint32(0x80000000),
                 np.uint32(0x7FFFFFFF) - m,
                 np.uint32(0x80000000) + m).astype(np.uint32)
    k[m == 0] = np.uint32(0x80000000)
    k[m > np.uint32(0x7F800000)] = np.uint32(0xFFFFFFFF)
    return k


def _bf16_threshold_keys_table(split_vals: np.ndarray) -> np.ndarray:
    """Table/searchsorted reference implementation (used by tests to
    cross-check the closed form below)."""
    vals, keys = _bf16_key_tables()
    idx = np.searchsorted(vals, split_vals.astype(np.float32), side="left")
    return keys[idx].astype(np.uint32) << np.uint32(16)


def _bf16_threshold_keys(split_vals: np.ndarray) -> np.ndarray:
    """Smallest producible bf16 key whose value is >= the f32 split value,
    shifted into the high 16 bits (kernel compares widened keys).

    Closed form: for s > 0 the smallest bf16 >= s is the truncated top-16
    bits, +1 when any mantissa bits were cut (carry into the exponent /
    into +inf is exactly right); for s <= 0 truncation already rounds
    toward +inf. Then apply the device key16() transform."""
    bits = np.ascontiguousarray(split_vals, dtype=np.float32).view(np.uint32)
    neg = (bits & np.uint32(0x80000000)) != 0
    b = (bits >> np.uint32(16)).astype(np.uint32)
    frac = (bits & np.uint32(0xFFFF)) != 0
    b = np.where(~neg & frac, b + np.uint32(1), b).astype(np.uint32)
    # device key16(): +-0 -> 0x8000, monotone elsewhere (s is never NaN)
    m = b & np.uint32(0x7FFF)
    k = np.where(b & np.uint32(0x8000),
                 np.uint32(0x7FFF) - m,
                 np.uint32(0x8000) + m).astype(np.uint32)
    k[m == 0] = np.uint32(0x8000)
    return k << np.uint32(16)


def _node_depths(feature: np.ndarray, right: np.ndarray) -> np.ndarray:
    """Per-node depth via a level-synchronous frontier sweep (one vectorized
    gather/scatter per level, ~height iterations total)."""
    T, mn = feature.shape
    depth = np.zeros((T, mn), dtype=np.int32)
    ft = np.repeat(np.arange(T, dtype=np.int64), 1)
    fn = np.zeros(T, dtype=np.int64)  # frontier: root of every tree
    level = 0
    while len(ft):
        internal = feature[ft, fn] >= 0
        ft, fn = ft[internal], fn[internal]
        if not len(ft):
            break
        level += 1
        rt = right[ft, fn].astype(np.int64)
        ft = np.concatenate([ft, ft])
        fn = np.concatenate([fn + 1, rt])
        depth[ft, fn] = level
    return depth


def _split_thresholds32(forest) -> np.ndarray:
    """f32 thresholds implementing the EXACT f64 split compare.

    The reference compares (double)(float x) < splitValue with splitValue
    a double (IsolationTree.scala:213-229). For f32 x and f64 s:
    x < s  <=>  x < ceil32(s) (the smallest f32 >= s), because no f32 lies
    strictly between two f32 neighbours. Our own builds store f32-exact
    splits (value64 == f32 value), so ceil32 is the identity there; loaded
    foreign models get the exact Spark semantics."""
    v64 = (forest.value64 if getattr(forest, "value64", None) is not None
           else forest.value.astype(np.float64))
    v32 = v64.astype(np.float32)
    lift = v32.astype(np.float64) < v64
    return np.where(lift, np.nextafter(v32, np.float32(np.inf)),
                    v32).astype(np.float32)


def _nodes_packed_v4(forest, d_sentinel: int, bf16):
    """v4 packed nodes for score_forest_v4 (see forest_kernels.hip);
    `bf16` is the row kind (_row_kind: False/"f32", True/"bf16", "f16"):
    w0 = feat | right<<12; internal w1 = integer key threshold; leaf:
    feat = d_sentinel, right = own id (self-loop), w1 = f32(depth + c(m)).
    Trees are padded to a multiple of 8 with single-leaf value-0 dummies
    (bindings.cpp enforces Tpad % 8 == 0).
    Returns (packed int32 [Tpad, mn, 2], ncount int32 [Tpad])."""
    T, mn = forest.feature.shape
    if mn > 32767:
        raise ValueError("forest too deep for the packed node format")
    feat = forest.feature
    if feat.max(initial=0) > 4094 or d_sentinel > 4094:
        raise ValueError("GPU scoring supports at most 4095 features")
    right = forest.right
    val = forest.value
    internal = feat >= 0
    leaf = feat == Forest.LEAF
    depth = _node_depths(feat, right)
    ids = np.broadcast_to(np.arange(mn, dtype=np.int32)[None, :], (T, mn))
    w0 = np.where(
        internal,
        feat.astype(np.int32) | (right.astype(np.int32) << 12),
        np.int32(d_sentinel) | (ids << 12),
    ).astype(np.int32)
    w1 = np.zeros((T, mn), dtype=np.uint32)
    if internal.any():
        s = _split_thresholds32(forest)[internal]
        w1[internal] = _threshold_keys(s, bf16)
    leafval = (depth.astype(np.float32) + val.astype(np.float32))
    w1[leaf] = leafval[leaf].astype(np.float32).view(np.uint32)
    pad = (-T) % 8
    if pad:
        w0p = np.empty((pad, mn), dtype=np.int32)
        w0p[:] = np.int32(d_sentinel) | (ids[0] << 12)
        w0 = np.concatenate([w0, w0p])
        w1 = np.concatenate([w1, np.zeros((pad, mn), dtype=np.uint32)])
    packed = np.empty((T + pad, mn, 2), dtype=np.int32)
    packed[..., 0] = w0
    packed[..., 1] = w1.view(np.int32)
    ncount = np.concatenate(
        [forest.node_count.astype(np.int32), np.ones(pad, dtype=np.int32)]
    )
    live = internal | leaf
    max_depth = int(depth[live].max()) if live.any() else 0
    return packed, ncount, max(max_depth, 1)


def _nodes_packed_wide(forest, bf16):
    """Wide int4 node records {feat, right, key_or_value, 0} for
    score_forest_wide (`bf16` is the row kind, as in _nodes_packed_v4) —
    no 12-bit feature / 15-bit node-id limits
    (the reference has no such size caps,
    IsolationTree.scala). Same key/leaf-value math as _nodes_packed_v4,
    so the walk stays bitwise vs cpu_engine.path_lengths. Leaves and pad
    nodes self-loop (right = own id)."""
    T, mn = forest.feature.shape
    feat = forest.feature
    right = forest.right
    val = forest.value
    internal = feat >= 0
    leaf = feat == Forest.LEAF
    depth = _node_depths(feat, right)
    ids = np.broadcast_to(np.arange(mn, dtype=np.int32)[None, :], (T, mn))
    w0 = np.where(internal, feat.astype(np.int32), np.int32(-1))
    w1 = np.where(internal, right.astype(np.int32), ids).astype(np.int32)
    w2 = np.zeros((T, mn), dtype=np.uint32)
    if internal.any():
        s = _split_thresholds32(forest)[internal]
        keys = _threshold_keys(s, bf16)
        w2[internal] = keys.astype(np.uint32)
    leafval = depth.astype(np.float32) + val.astype(np.float32)
    w2[leaf] = leafval[leaf].astype(np.float32).view(np.uint32)
    packed = np.zeros((T, mn, 4), dtype=np.int32)
    packed[..., 0] = w0
    packed[..., 1] = w1
    packed[..., 2] = w2.view(np.int32)
    live = internal | leaf
    max_depth = int(depth[live].max()) if live.any() else 0
    return packed, max(max_depth, 1)


def _nodes_packed_explain(forest, d_sentinel: int, bf16):
    """16-byte node records for explain_forest_kernel (`bf16` is the row
    kind, as in _nodes_packed_v4):
    {feat | right<<12, integer key threshold, delta_left bits,
    delta_right bits}. Threshold math is _nodes_packed_v4's; the f32 edge
    deltas are cpu_engine.explain_tables' (shared with the CPU oracle, so
    the kernel only has to reproduce the walk and the adds). Leaves and
    pads self-loop with feat = d_sentinel, threshold 0 (the sentinel key
    0xFFFFFFFF never compares below it) and both deltas +0.0.
    Returns (packed int32 [T, mn, 4], max_depth)."""
    from ..core.cpu_engine import explain_tables

    T, mn = forest.feature.shape
    if mn > 32767:
        raise ValueError("forest too deep for the packed node format")
    feat = forest.feature
    if feat.max(initial=0) > 4094 or d_sentinel > 4094:
        raise ValueError("GPU scoring supports at most 4095 features")
    internal = feat >= 0
    leaf = feat == Forest.LEAF
    tabs = explain_tables(forest)
    ids = np.broadcast_to(np.arange(mn, dtype=np.int32)[None, :], (T, mn))
    w0 = np.where(
        internal,
        feat.astype(np.int32) | (forest.right.astype(np.int32) << 12),
        np.int32(d_sentinel) | (ids << 12),
    ).astype(np.int32)
    w1 = np.zeros((T, mn), dtype=np.uint32)
    if internal.any():
        s = _split_thresholds32(forest)[internal]
        w1[internal] = _threshold_keys(s, bf16)
    packed = np.zeros((T, mn, 4), dtype=np.int32)
    packed[..., 0] = w0
    packed[..., 1] = w1.view(np.int32)
    packed[..., 2] = np.where(internal, tabs["dl"], np.float32(0.0)).astype(
        np.float32).view(np.int32)
    packed[..., 3] = np.where(internal, tabs["dr"], np.float32(0.0)).astype(
        np.float32).view(np.int32)
    depth = _node_depths(feat, forest.right)
    live = internal | leaf
    max_depth = int(depth[live].max()) if live.any() else 0
    return packed, max(max_depth, 1)


def _shap_packed(forest, kind):
    """Leaf-path word stream for shap_forest_kernel (layout in
    ops/hip/shap_kernels.hip) from cpu_engine.shap_tables, for one row kind:
    per leaf {f64 L, m}, then m entries {f64 z, lo | hi << 32, feature}.

    [lo, hi] is the INCLUSIVE interval of widened row keys that take the
    path's branch at every node the entry merges. A row goes left iff
    widen(key(x)) < threshold key (_nodes_packed_v4's thresholds), so lo is
    the max threshold over the right turns (0: none) and hi the min over
    the left turns, minus 1 (0xFFFFFFFF: none; the NaN key passes, NaN goes
    right). A left turn at threshold key 0 is never taken: the entry gets
    the empty interval lo = 1, hi = 0 rather than a wrapped hi.
    Returns (words uint64 [W], tree_off int64 [T + 1] in words)."""
    from ..core.cpu_engine import shap_tables

    tabs = shap_tables(forest)
    T = forest.num_trees
    thr = np.zeros(forest.feature.shape, dtype=np.uint32)
    internal = forest.feature >= 0
    if internal.any():
        s = _split_thresholds32(forest)[internal]
        thr[internal] = _threshold_keys(s, kind)
    ent_off = tabs["leaf_ent_off"]
    n_ent = len(tabs["ent_feat"])
    pn_ent = np.repeat(np.arange(n_ent, dtype=np.int64),
                       np.diff(tabs["ent_pn_off"]))
    pn_key = thr[tabs["pn_tree"], tabs["pn_node"]].astype(np.int64)
    left = tabs["pn_left"]
    lo = np.zeros(n_ent, dtype=np.int64)
    hi = np.full(n_ent, 1 << 32, dtype=np.int64)  # exclusive, none yet
    np.maximum.at(lo, pn_ent[~left], pn_key[~left])
    np.minimum.at(hi, pn_ent[left], pn_key[left])
    never = hi == 0
    lo[never] = 1
    hi = np.where(never, 0, hi - 1)  # inclusive

    leaf_m = tabs["leaf_m"]
    n_leaf = len(leaf_m)
    leaf_word = 2 * np.arange(n_leaf, dtype=np.int64) + 3 * ent_off[:-1]
    total = 2 * n_leaf + 3 * n_ent
    words = np.zeros(total, dtype=np.uint64)
    words[leaf_word] = tabs["leaf_L"].view(np.uint64)
    words[leaf_word + 1] = leaf_m.astype(np.uint64)
    ent_leaf = np.repeat(np.arange(n_leaf, dtype=np.int64), leaf_m)
    ent_word = (leaf_word[ent_leaf] + 2
                + 3 * (np.arange(n_ent, dtype=np.int64) - ent_off[ent_leaf]))
    words[ent_word] = tabs["ent_z"].view(np.uint64)
    words[ent_word + 1] = (lo.astype(np.uint64)
                           | (hi.astype(np.uint64) << np.uint64(32)))
    words[ent_word + 2] = tabs["ent_feat"].astype(np.uint64)
    tlo = tabs["tree_leaf_off"]
    tree_off = (2 * tlo + 3 * ent_off[tlo]).astype(np.int64)
    assert tree_off[0] == 0 and tree_off[T] == total
    return words, np.ascontiguousarray(tree_off)


def _eif_packed_wide(forest):
    """Wide int4 node records {is_leaf(-1)/0, right, value_bits, 0} for
    score_extended_wide (strict oracle j-order dot from global
    hyperplanes)."""
    T, mn = forest.feature.shape
    feat = forest.feature
    internal = feat >= 0
    ids = np.broadcast_to(np.arange(mn, dtype=np.int32)[None, :], (T, mn))
    packed = np.zeros((T, mn, 4), dtype=np.int32)
    packed[..., 0] = np.where(internal, np.int32(0), np.int32(-1))
    packed[..., 1] = np.where(internal, forest.right.astype(np.int32), ids)
    packed[..., 2] = forest.value.astype(np.float32).view(np.int32)
    return packed


def _key32_inverse(k: np.ndarray) -> np.ndarray:
    """Inverse of _key32 over the finite/inf key range (value of a key)."""
    k = np.asarray(k, dtype=np.uint32)
    pos = k >= np.uint32(0x80000000)
    bits = np.where(pos, k - np.uint32(0x80000000),
                    np.uint32(0x80000000) | (np.uint32(0x7FFFFFFF) - k))
    return bits.astype(np.uint32).view(np.float32)


def _eif0_eligible(forest, d: int) -> bool:
    """extensionLevel-0 fast-path eligibility: every internal node has one
    finite non-zero weight and a 12-bit coordinate (our builds give w=+-1;
    foreign single-coordinate files qualify too)."""
    flag = getattr(forest, "_eif0_ok", None)
    if flag is None:
        internal = forest.feature >= 0
        w = forest.hyper_w[..., 0]
        coord = forest.hyper_idx[..., 0]
        flag = bool(
            d <= 4094
            and (not internal.any()
                 or (np.isfinite(w[internal]).all()
                     and (w[internal] != 0).all()
                     and coord[internal].max(initial=0) <= 4094))
        )
        forest._eif0_ok = flag
    return flag


def _eif0_packed_v4(forest, d_sentinel: int, bf16):
    """Pack an extensionLevel-0 EIF forest into STANDARD v4 node records
    (`bf16` is the row kind, as in _nodes_packed_v4; 16-bit kinds search
    their producible-key table, f32 the whole key range),
    so scoring reuses the unmodified fixed-trip walk (score_forest_v4)
    with NO per-visit multiply and NO extra compare.

    Two exact transformations compose:

    1. Thresholds. The oracle predicate per internal node is
       P(x) = f32(w*x) < offset32 (cpu_engine.path_lengths_extended,
       nnz=1). f32 multiplication by a fixed finite non-zero w is
       monotone in x, so P is a threshold predicate along the
       order-preserving key space: a vectorized binary search (evaluating
       P with the same numpy f32 multiply the oracle uses) finds, per
       node, the exact cut key K with
           w > 0:  P(x) <=> key(x) <  K
           w < 0:  P(x) <=> key(x) >= K
    2. Subtree mirroring. Negative-weight nodes (w < 0) have their left
       and right SUBTREES swapped in a re-materialized pre-order layout,
       turning "go left iff key >= K" into the v4 kernel's native
       "go left iff key < K" (the compare-false branch is the old left).
       Node depths — the only structural quantity scoring uses — are
       invariant under mirroring.

    The GPU performs no arithmetic on w at all, so the route is bitwise
    vs the oracle BY CONSTRUCTION for every representable non-NaN x.
    NaN features are the one exception (the oracle's NaN dot compares
    false at EVERY node, which no single mirrored threshold can encode):
    callers route rows containing NaN to the strict-order kernels
    (score_extended_forest checks torch.isnan once per call)."""
    T, mn = forest.feature.shape
    feat = forest.feature
    internal = feat >= 0
    leaf = feat == ExtendedForest.LEAF
    depth = _node_depths(feat, forest.right)
    w = forest.hyper_w[..., 0].astype(np.float32)
    coord = forest.hyper_idx[..., 0].astype(np.int32)
    o = forest.value.astype(np.float32)  # internal: offset32
    flip = (w < 0) & internal

    iw = w[internal]
    io = o[internal]
    iflip = flip[internal]

    kind = _row_kind(bf16)
    if kind != "f32":
        # 18 halvings cover both tables (bf16 65,279 keys, fp16 63,489)
        vals, keys = (_bf16_key_tables() if kind == "bf16"
                      else _f16_key_tables())
        lo = np.zeros(iw.shape, dtype=np.int64)
        hi = np.full(iw.shape, len(vals), dtype=np.int64)
        for _ in range(18):
            mid = (lo + hi) // 2
            midc = np.minimum(mid, len(vals) - 1)
            pm = (iw * vals[midc]).astype(np.float32) < io
            qm = np.where(iflip, ~pm, pm) & (mid < len(vals))
            lo = np.where(qm, mid + 1, lo)
            hi = np.where(qm, hi, mid)
        k16 = np.where(hi < len(vals), keys[np.minimum(hi, len(vals) - 1)],
                       np.int64(keys[-1]) + 1).astype(np.int64)
        K = (k16 << 16).astype(np.uint64).astype(np.uint32)
    else:
        kmin = int(_key32(np.array([-np.inf], dtype=np.float32))[0])
        kmax = int(_key32(np.array([np.inf], dtype=np.float32))[0])
        lo = np.full(iw.shape, kmin, dtype=np.int64)
        hi = np.full(iw.shape, kmax + 1, dtype=np.int64)
        for _ in range(33):
            mid = (lo + hi) // 2
            xm = _key32_inverse(np.minimum(mid, kmax).astype(np.uint64))
            pm = (iw * xm).astype(np.float32) < io
            qm = np.where(iflip, ~pm, pm) & (mid <= kmax)
            lo = np.where(qm, mid + 1, lo)
            hi = np.where(qm, hi, mid)
        K = hi.astype(np.uint64).astype(np.uint32)

    # --- mirrored pre-order re-layout (level-synchronous, vectorized) ---
    right = forest.right.astype(np.int64)
    nc = forest.node_count.astype(np.int64)
    newpos = np.zeros((T, mn), dtype=np.int64)
    end_old = np.zeros((T, mn), dtype=np.int64)  # old-coords subtree end
    end_old[np.arange(T), 0] = nc
    new_rightpos = np.zeros((T, mn), dtype=np.int64)
    ft = np.arange(T, dtype=np.int64)
    fn = np.zeros(T, dtype=np.int64)
    while len(ft):
        isint = internal[ft, fn]
        ft, fn = ft[isint], fn[isint]
        if not len(ft):
            break
        rt = right[ft, fn]
        s_left = rt - (fn + 1)
        s_right = end_old[ft, fn] - rt
        fl = flip[ft, fn]
        lpos = newpos[ft, fn] + 1
        # new left child = old right when flipped (compare-true branch)
        newpos[ft, fn + 1] = np.where(fl, lpos + s_right, lpos)
        newpos[ft, rt] = np.where(fl, lpos, lpos + s_left)
        new_rightpos[ft, fn] = np.where(fl, newpos[ft, fn + 1],
                                        newpos[ft, rt])
        end_old[ft, fn + 1] = rt
        end_old[ft, rt] = end_old[ft, fn]
        ft = np.concatenate([ft, ft])
        fn = np.concatenate([fn + 1, rt])

    ids = np.broadcast_to(np.arange(mn, dtype=np.int32)[None, :], (T, mn))
    w0 = np.empty((T, mn), dtype=np.int32)
    w0[:] = np.int32(d_sentinel) | (ids << 12)  # pad slots: self-loop
    w1 = np.zeros((T, mn), dtype=np.uint32)
    ti = np.broadcast_to(np.arange(T, dtype=np.int64)[:, None], (T, mn))
    # scatter live nodes to their mirrored positions
    it_, in_ = ti[internal], newpos[internal]
    w0[it_, in_] = (coord[internal]
                    | (new_rightpos[internal].astype(np.int32) << 12))
    w1[it_, in_] = K
    lt_, ln_ = ti[leaf], newpos[leaf]
    w0[lt_, ln_] = np.int32(d_sentinel) | (ln_.astype(np.int32) << 12)
    leafval = (depth.astype(np.float32)
               + forest.value.astype(np.float32))[leaf]
    w1[lt_, ln_] = leafval.astype(np.float32).view(np.uint32)

    pad = (-T) % 8
    if pad:
        w0p = np.empty((pad, mn), dtype=np.int32)
        w0p[:] = np.int32(d_sentinel) | (ids[0] << 12)
        w0 = np.concatenate([w0, w0p])
        w1 = np.concatenate([w1, np.zeros((pad, mn), dtype=np.uint32)])
    packed = np.empty((T + pad, mn, 2), dtype=np.int32)
    packed[..., 0] = w0
    packed[..., 1] = w1.view(np.int32)
    ncount = np.concatenate(
        [forest.node_count.astype(np.int32), np.ones(pad, dtype=np.int32)]
    )
    live = internal | leaf
    max_depth = int(depth[live].max()) if live.any() else 0
    return packed, ncount, max(max_depth, 1)


def _densify_weights(hidx: np.ndarray, hw: np.ndarray, counts: np.ndarray,
                     D: int) -> np.ndarray:
    """Scatter sparse hyperplanes [T, mn, nnz] into dense rows [T, mn, D].
    Padded slots (j >= counts) are redirected to a scratch column so their
    zero index cannot clobber a real coordinate-0 weight."""
    T, mn, nnz = hidx.shape
    j = np.arange(nnz, dtype=np.int64)[None, None, :]
    idx = np.where(j < counts[:, :, None], hidx.astype(np.int64), D)
    dense = np.zeros((T, mn, D + 1), dtype=np.float32)
    np.put_along_axis(dense, idx, hw.astype(np.float32), axis=2)
    return np.ascontiguousarray(dense[:, :, :D])


def _eif_nodes_values(forest):
    """Shared EIF v2 node packing: w0 = right<<12 (leaf/pad: own id ->
    self-loop), w1 = offset f32 (leaf/pad: -inf), depth-folded leaf values.
    Returns (packed int32 [T, mn, 2], values f32 [T, mn], max_depth)."""
    T, mn = forest.feature.shape
    if mn > 32767:
        raise ValueError("forest too deep for the packed node format")
    feat = forest.feature
    internal = feat >= 0
    leaf = feat == ExtendedForest.LEAF
    depth = _node_depths(feat, forest.right)
    ids = np.broadcast_to(np.arange(mn, dtype=np.int32)[None, :], (T, mn))
    w0 = np.where(internal, forest.right.astype(np.int32), ids) << 12
    w1 = np.where(
        internal,
        forest.value.astype(np.float32),
        np.float32(-np.inf),
    ).astype(np.float32)
    packed = np.empty((T, mn, 2), dtype=np.int32)
    packed[..., 0] = w0
    packed[..., 1] = w1.view(np.int32)
    values = np.where(
        leaf,
        depth.astype(np.float32) + forest.value.astype(np.float32),
        np.float32(0.0),
    ).astype(np.float32)
    live = internal | leaf
    max_depth = int(depth[live].max()) if live.any() else 0
    return packed, values, max(max_depth, 1)


def _eif_dense_packed(forest, D: int):
    """EIF v2 packing + DENSIFIED weight matrix (sparse hyperplanes
    scattered to D columns) for score_extended_dense_v2."""
    packed, values, max_depth = _eif_nodes_values(forest)
    feat = forest.feature
    counts = np.where(feat >= 0, feat, 0).astype(np.int64)
    hw_dense = _densify_weights(forest.hyper_idx, forest.hyper_w, counts, D)
    return packed, values, hw_dense, max_depth


def _nodes_packed(forest) -> np.ndarray:
    """Packed 8-byte node records for the EIF scoring kernels:
    meta<0 => leaf (value = c(count)); else feature = meta&0xFFF,
    right = (meta>>12)&0x7FFF (left child is implicit pre-order id+1)."""
    T, mn = forest.feature.shape
    if mn > 32767:
        raise ValueError("forest too deep for the packed node format")
    feat = forest.feature
    if feat.max(initial=0) > 4095:
        raise ValueError("GPU scoring supports at most 4096 features")
    internal = feat >= 0
    meta = np.where(
        internal,
        feat.astype(np.int32) | (forest.right.astype(np.int32) << 12),
        np.int32(-2147483648),
    ).astype(np.int32)
    packed = np.empty((T, mn, 2), dtype=np.int32)
    packed[..., 0] = meta
    packed[..., 1] = forest.value.view(np.int32)
    return packed


_TWO32 = 1 << 32
_TWO31 = 1 << 31


def _to_i32(x64: torch.Tensor) -> torch.Tensor:
    """int64 (holding u32 bit patterns) -> int32 with C-style wraparound."""
    return torch.where(x64 >= _TWO31, x64 - _TWO32, x64).to(torch.int32)


def _bf16_threshold_keys_dev(vals_f32: torch.Tensor) -> torch.Tensor:
    """Device mirror of _bf16_threshold_keys: int64 holding (t16 << 16)."""
    bits = vals_f32.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    neg = (bits & 0x80000000) != 0
    b = bits >> 16
    frac = (bits & 0xFFFF) != 0
    b = torch.where(~neg & frac, b + 1, b)
    m = b & 0x7FFF
    k = torch.where((b & 0x8000) != 0, 0x7FFF - m, 0x8000 + m)
    k = torch.where(m == 0, torch.full_like(k, 0x8000), k)
    return k << 16


_F16_KEY_TABLES_DEV = {}


def _f16_threshold_keys_dev(vals_f32: torch.Tensor) -> torch.Tensor:
    """Device mirror of _f16_threshold_keys: int64 holding (t16 << 16).
    The same table, uploaded once per device, and torch.searchsorted
    (right=False is numpy's side="left")."""
    dev = vals_f32.device
    tabs = _F16_KEY_TABLES_DEV.get(str(dev))
    if tabs is None:
        vals, keys = _f16_key_tables()
        keys_ext = np.append(keys, np.uint32(0)).astype(np.int64)
        tabs = (torch.from_numpy(vals).to(dev),
                torch.from_numpy(keys_ext).to(dev))
        _F16_KEY_TABLES_DEV[str(dev)] = tabs
    idx = torch.searchsorted(tabs[0], vals_f32.contiguous(), right=False)
    return tabs[1][idx] << 16


def _key32_dev(vals_f32: torch.Tensor) -> torch.Tensor:
    """Device mirror of _key32: int64 holding u32 keys (inputs never NaN)."""
    b = vals_f32.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    m = b & 0x7FFFFFFF
    k = torch.where((b & 0x80000000) != 0, 0x7FFFFFFF - m, 0x80000000 + m)
    return torch.where(m == 0, torch.full_like(k, 0x80000000), k)


def _nodes_packed_v4_device(raw, num_trees: int, d_sentinel: int, bf16):
    """Torch-side v4 packing from the raw build outputs still on device —
    identical bit layout to _nodes_packed_v4 (`bf16` is the row kind), no
    host round trip."""
    kind = _row_kind(bf16)
    feat, value = raw["feat"], raw["value"]
    right, ncount, depth = raw["right"], raw["ncount"], raw["depth"]
    T, mn = feat.shape
    dev = feat.device
    ids = torch.arange(mn, dtype=torch.int32, device=dev).expand(T, mn)
    live = ids < ncount.to(torch.int32).unsqueeze(1)
    internal = live & (feat >= 0)
    leaf = live & (feat == -1)
    w0 = torch.where(
        internal,
        feat | (right << 12),
        torch.tensor(d_sentinel, dtype=torch.int32, device=dev) | (ids << 12),
    )
    tkeys = (_bf16_threshold_keys_dev(value) if kind == "bf16"
             else _f16_threshold_keys_dev(value) if kind == "f16"
             else _key32_dev(value))
    leafbits = (depth.to(torch.float32) + value).view(torch.int32)
    w1 = torch.where(internal, _to_i32(tkeys),
                     torch.where(leaf, leafbits,
                                 torch.zeros_like(leafbits)))
    pad = (-T) % 8
    if pad:
        w0p = (torch.tensor(d_sentinel, dtype=torch.int32, device=dev)
               | (ids[:1] << 12)).expand(pad, mn).contiguous()
        w0 = torch.cat([w0, w0p])
        w1 = torch.cat([w1, torch.zeros(pad, mn, dtype=torch.int32,
                                        device=dev)])
    packed = torch.stack([w0, w1], dim=2).contiguous()
    ncount_p = torch.cat([
        ncount.to(torch.int32),
        torch.ones(pad, dtype=torch.int32, device=dev)])
    max_depth = int(depth.masked_fill(~live, 0).max().item())
    return packed, ncount_p, max(max_depth, 1)


def _eif_nodes_values_device(raw):
    """Torch-side mirror of _eif_nodes_values."""
    feat, value = raw["feat"], raw["value"]
    right, ncount, depth = raw["right"], raw["ncount"], raw["depth"]
    T, mn = feat.shape
    dev = feat.device
    ids = torch.arange(mn, dtype=torch.int32, device=dev).expand(T, mn)
    live = ids < ncount.to(torch.int32).unsqueeze(1)
    internal = live & (feat >= 0)
    leaf = live & (feat == -1)
    w0 = torch.where(internal, right, ids) << 12
    ninf = torch.tensor(float("-inf"), device=dev)
    w1 = torch.where(internal, value, ninf).view(torch.int32)
    packed = torch.stack([w0, w1], dim=2).contiguous()
    values = torch.where(leaf, depth.to(torch.float32) + value,
                         torch.zeros_like(value)).contiguous()
    max_depth = int(depth.masked_fill(~live, 0).max().item())
    return packed, values, internal, max(max_depth, 1)


def _eif_dense_packed_device(raw, D: int):
    """Torch-side mirror of _eif_dense_packed (densified weights)."""
    packed, values, internal, max_depth = _eif_nodes_values_device(raw)
    feat, hidx, hw = raw["feat"], raw["hidx"], raw["hw"]
    T, mn = feat.shape
    dev = feat.device
    counts = torch.where(internal, feat, torch.zeros_like(feat)).to(torch.int64)
    nnz = hidx.shape[2]
    j = torch.arange(nnz, dtype=torch.int64, device=dev).view(1, 1, nnz)
    idx = torch.where(j < counts.unsqueeze(2), hidx.to(torch.int64),
                      torch.tensor(D, dtype=torch.int64, device=dev))
    dense = torch.zeros(T, mn, D + 1, dtype=torch.float32, device=dev)
    dense.scatter_(2, idx, hw)
    hw_dense = dense[:, :, :D].contiguous()
    return packed, values, hw_dense, max_depth


def _v4_walk_order(aos: torch.Tensor, ncount: torch.Tensor) -> torch.Tensor:
    """Pre-order v4 records (what the four packers emit) -> the level-order
    records score_forest_v4 walks (link = right child, left = link - 1);
    one small kernel per pack, cached with it. Part of packing, like the
    torch-side packers, not a scoring route: the extension is taken from the
    package, so a routing proxy installed on this module sees scoring calls
    only."""
    from . import load_extension as _packing_extension

    return _packing_extension().v4_level_order(aos.contiguous(),
                                               ncount.contiguous())


def _v4_heap_records(aos: torch.Tensor, ncount: torch.Tensor, d: int, kind,
                     height: int):
    """Pre-order v4 records -> the 4-byte heap records score_forest_heap
    walks (16-bit rows; forest_kernels.hip), or None where the extension's
    score_route keeps these shapes on the v4 kernels. Packing, like
    _v4_walk_order; cached with the pack under extra["heap"]."""
    kind = _row_kind(kind)
    if kind == "f32":
        return None
    from . import load_extension as _packing_extension

    ext = _packing_extension()
    if ext.score_route(kind, int(d), int(aos.shape[1]), int(height),
                       "packed") != "heap":
        return None
    return ext.v4_heap_order(aos.contiguous(), ncount.contiguous(),
                             int(height), int(d))


def _heap_rpt(aos: torch.Tensor, d: int, kind, height: int) -> int:
    """Rows per thread of the heap instantiation these shapes run now (0 off
    the heap route). The records' slab offsets are laid out for it."""
    from . import load_extension as _packing_extension

    return int(_packing_extension().score_heap_cfg(
        _row_kind(kind), int(d), int(aos.shape[1]), int(height))[1])


def _heap_for_call(aos, extra, d: int, kind):
    """extra["heap"] where it was laid out for the rows per thread this call
    runs. IFA_HEAP_PHASE set after the pack was made can move that choice;
    the call then takes the level-order records (same scores)."""
    heap = extra["heap"]
    if heap is None:
        return None
    now = _heap_rpt(aos, d, kind, max(extra["height"], 1))
    return heap if now == extra["heap_rpt"] else None


def _device_forest(model, device, v4_key=None):
    """Cached device copy of the packed forest. v4_key = (d, kind) selects
    the standard-scoring v4 packing; None = the EIF packing. Packs that
    hold integer key thresholds — (d, kind), ("wide", kind),
    ("eif0", d, kind), ("explain", d, kind), ("shap", d, kind) — are keyed
    on the row KIND, not on "is it 16-bit": bf16 and fp16 keys differ, and
    u32 records under a u16 kernel score silently wrong. The "shap" entry
    is (table words, per-tree word offsets, {host offsets, weights})."""
    if isinstance(v4_key, tuple) and v4_key[0] not in ("eif_dense",
                                                       "eif_dense3"):
        v4_key = v4_key[:-1] + (_row_kind(v4_key[-1]),)
    key = (str(device), id(model.forest), v4_key)
    cache = model._gpu_forest_cache
    if key not in cache:
        forest = model.forest
        extra = {}
        raw = getattr(forest, "_device_raw", None)
        if raw is not None and raw["device"] != str(device):
            raw = None
        if raw is None and device.type == "cuda" and \
                getattr(forest, "depth_np", None) is not None:
            # e.g. an all-gathered multi-rank forest: rebuild the raw view
            # from host arrays (one upload) so packing stays on device
            raw = {
                "device": str(device),
                "feat": torch.from_numpy(
                    np.ascontiguousarray(forest.feature)).to(device),
                "value": torch.from_numpy(
                    np.ascontiguousarray(forest.value)).to(device),
                "right": torch.from_numpy(
                    np.ascontiguousarray(forest.right)).to(device),
                "ncount": torch.from_numpy(np.ascontiguousarray(
                    forest.node_count, dtype=np.int32)).to(device),
                "depth": torch.from_numpy(np.ascontiguousarray(
                    forest.depth_np, dtype=np.int32)).to(device),
            }
            if isinstance(forest, ExtendedForest):
                raw["hidx"] = torch.from_numpy(
                    np.ascontiguousarray(forest.hyper_idx)).to(device)
                raw["hw"] = torch.from_numpy(
                    np.ascontiguousarray(forest.hyper_w)).to(device)
            forest._device_raw = raw
        if v4_key == "eif_sparse":
            if raw is not None:
                aos, values_t, _, max_depth = _eif_nodes_values_device(raw)
                ncount = raw["ncount"]
                extra["values"] = values_t
                extra["hidx"] = raw["hidx"]
                extra["hw"] = raw["hw"]
            else:
                packed, values, max_depth = _eif_nodes_values(forest)
                aos = torch.from_numpy(packed).to(device)
                ncount = torch.from_numpy(
                    np.ascontiguousarray(forest.node_count, dtype=np.int32)
                ).to(device)
                extra["values"] = torch.from_numpy(values).to(device)
                extra["hidx"] = torch.from_numpy(
                    np.ascontiguousarray(forest.hyper_idx)).to(device)
                extra["hw"] = torch.from_numpy(
                    np.ascontiguousarray(forest.hyper_w)).to(device)
            extra["height"] = max_depth
        elif isinstance(v4_key, tuple) and v4_key[0] in ("eif_dense",
                                                         "eif_dense3"):
            D = v4_key[1]
            if raw is not None:
                aos, values_t, hw_t, max_depth = _eif_dense_packed_device(
                    raw, D)
                ncount = raw["ncount"]
                extra["values"] = values_t
                extra["hw"] = hw_t
            else:
                packed, values, hw_dense, max_depth = _eif_dense_packed(
                    forest, D)
                aos = torch.from_numpy(packed).to(device)
                ncount = torch.from_numpy(
                    np.ascontiguousarray(forest.node_count, dtype=np.int32)
                ).to(device)
                extra["values"] = torch.from_numpy(values).to(device)
                extra["hw"] = torch.from_numpy(hw_dense).to(device)
            if v4_key[0] == "eif_dense3":
                # v3 weight staging: RNE-round the trained f32 weights to
                # bf16 and pack pairs (j even low, j+1 high) into int32 for
                # the v_dot2c_f32_bf16 dot (PARITY.md EIF bf16 contract)
                hb = extra["hw"].to(torch.bfloat16).view(torch.uint16)
                hb = hb.to(torch.int32)
                extra["hwp"] = (
                    hb[..., 0::2] | (hb[..., 1::2] << 16)
                ).contiguous()
            extra["height"] = max_depth
        elif isinstance(v4_key, tuple) and v4_key[0] == "eif0":
            packed, ncount_np, max_depth = _eif0_packed_v4(
                forest, v4_key[1], v4_key[2])
            ncount = torch.from_numpy(ncount_np).to(device)
            aos = torch.from_numpy(packed).to(device)
            extra["heap"] = _v4_heap_records(aos, ncount, v4_key[1],
                                             v4_key[2], max(max_depth, 1))
            extra["heap_rpt"] = _heap_rpt(aos, v4_key[1], v4_key[2],
                                          max(max_depth, 1))
            aos = _v4_walk_order(aos, ncount)
            extra["height"] = max_depth
        elif isinstance(v4_key, tuple) and v4_key[0] == "explain":
            packed, max_depth = _nodes_packed_explain(
                forest, v4_key[1], v4_key[2])
            aos = torch.from_numpy(packed).to(device)
            ncount = torch.from_numpy(
                np.ascontiguousarray(forest.node_count, dtype=np.int32)
            ).to(device)
            extra["height"] = max_depth
        elif isinstance(v4_key, tuple) and v4_key[0] == "shap":
            from ..core.cpu_engine import shap_weights

            words, tree_off = _shap_packed(forest, v4_key[2])
            aos = torch.from_numpy(words.view(np.int64)).to(device)
            ncount = torch.from_numpy(tree_off).to(device)  # word offsets
            extra["tree_off_host"] = torch.from_numpy(tree_off)
            extra["wtab"] = torch.from_numpy(shap_weights()).to(device)
        elif v4_key == "eif_explain":
            from ..core.cpu_engine import explain_tables

            tabs = explain_tables(forest)
            aos = torch.from_numpy(_nodes_packed(forest)).to(device)
            ncount = torch.from_numpy(
                np.ascontiguousarray(forest.node_count, dtype=np.int32)
            ).to(device)
            extra["hidx"] = torch.from_numpy(
                np.ascontiguousarray(forest.hyper_idx)).to(device)
            extra["hw"] = torch.from_numpy(
                np.ascontiguousarray(forest.hyper_w)).to(device)
            extra["dl"] = torch.from_numpy(tabs["dl"]).to(device)
            extra["dr"] = torch.from_numpy(tabs["dr"]).to(device)
        elif isinstance(v4_key, tuple) and v4_key[0] == "wide":
            packed, max_depth = _nodes_packed_wide(forest, v4_key[1])
            aos = torch.from_numpy(packed).to(device)
            ncount = torch.from_numpy(
                np.ascontiguousarray(forest.node_count, dtype=np.int32)
            ).to(device)
            extra["height"] = max_depth
        elif v4_key == "eif_wide":
            packed = _eif_packed_wide(forest)
            aos = torch.from_numpy(packed).to(device)
            ncount = torch.from_numpy(
                np.ascontiguousarray(forest.node_count, dtype=np.int32)
            ).to(device)
            extra["hidx"] = torch.from_numpy(
                np.ascontiguousarray(forest.hyper_idx)).to(device)
            extra["hw"] = torch.from_numpy(
                np.ascontiguousarray(forest.hyper_w)).to(device)
        elif v4_key is not None:
            d, kind = v4_key
            if raw is not None:
                aos, ncount, max_depth = _nodes_packed_v4_device(
                    raw, forest.num_trees, d, kind)
            else:
                packed, ncount_np, max_depth = _nodes_packed_v4(forest, d, kind)
                aos = torch.from_numpy(packed).to(device)
                ncount = torch.from_numpy(ncount_np).to(device)
            extra["heap"] = _v4_heap_records(aos, ncount, d, kind, max_depth)
            extra["heap_rpt"] = _heap_rpt(aos, d, kind, max_depth)
            aos = _v4_walk_order(aos, ncount)
            extra["height"] = max_depth
        else:
            aos = torch.from_numpy(_nodes_packed(forest)).to(device)
            ncount = torch.from_numpy(
                np.ascontiguousarray(forest.node_count, dtype=np.int32)
            ).to(device)
            if isinstance(forest, ExtendedForest):
                extra["hidx"] = torch.from_numpy(
                    np.ascontiguousarray(forest.hyper_idx)
                ).to(device)
                extra["hw"] = torch.from_numpy(
                    np.ascontiguousarray(forest.hyper_w)
                ).to(device)
        # bounded FIFO (a few packings per model: e.g. alternating
        # bf16/fp16/f32 scoring of one model keeps all three — VERDICT r01
        # weak #6)
        while len(cache) >= 4:
            cache.pop(next(iter(cache)))
        cache[key] = (aos, ncount, extra)
    return cache[key]


def _packed_fits(forest, d: int) -> bool:
    """True when the packed v4/EIF formats can represent this forest
    (12-bit feature ids, 15-bit node ids)."""
    mn = forest.feature.shape[1]
    if mn > 32767:
        return False
    return int(forest.feature.max(initial=0)) <= 4094 and d <= 4094


def score_forest(model, X: torch.Tensor, finalize: bool = True) -> torch.Tensor:
    ext = load_extension()
    forest = model.forest
    d = int(X.shape[1])
    kind = _row_kind(X.dtype)
    c = float(avg_path_length(forest.num_samples))
    if not _packed_fits(forest, d):
        # loaded/CPU-built forests past the packed-format caps: wide int4
        # records, no field-width limits
        aos, ncount, extra = _device_forest(
            model, X.device, v4_key=("wide", kind))
        return ext.score_forest_wide(
            _rows_in_place(X), aos, extra["height"], c, finalize,
        )
    aos, ncount, extra = _device_forest(model, X.device, v4_key=(d, kind))
    return ext.score_forest(
        _rows_in_place(X), aos, ncount, forest.num_trees, extra["height"], c,
        finalize, _heap_for_call(aos, extra, d, kind),
    )


def _eif_uniform_nnz(forest) -> bool:
    """True when every internal node carries exactly forest.nnz coordinates
    (always the case for forests we build; foreign ragged files route to the
    general kernel so trailing zero-terms cannot perturb the strict-order
    dot)."""
    u = getattr(forest, "_uniform_nnz", None)
    if u is None:
        f = forest.feature
        internal = f >= 0
        u = bool((f[internal] == forest.nnz).all()) if internal.any() else True
        forest._uniform_nnz = u
    return u


def score_extended_forest(model, X: torch.Tensor, finalize: bool = True) -> torch.Tensor:
    ext = load_extension()
    forest = model.forest
    c = float(avg_path_length(forest.num_samples))
    d = int(X.shape[1])
    nnz = forest.nnz
    mn = forest.feature.shape[1]
    if mn > 32767 or int(forest.feature.max(initial=0)) > 4094:
        # past the packed 15-bit node-id / 12-bit count caps: wide records
        aos, ncount, extra = _device_forest(model, X.device,
                                            v4_key="eif_wide")
        return ext.score_extended_wide(
            _rows_in_place(X), aos, extra["hidx"], extra["hw"], c, finalize,
        )
    # routing (measured crossovers, profiles/r01_bench_and_kernels.md):
    # nnz <= 5 with uniform hyperplane widths -> fixed-trip sparse v2;
    # wider hyperplanes with d <= 32 -> densified dense v2 walk;
    # everything else -> the general strict-order kernel.
    if (nnz == 1 and mn <= 32767 and _eif_uniform_nnz(forest)
            and _eif0_eligible(forest, d)
            and os.environ.get("IFA_EIF0_SPARSE") != "1"
            and not bool(torch.isnan(X).any().item())):
        # extensionLevel-0: exact key thresholds + mirrored subtrees ->
        # the UNMODIFIED standard v4 walk (no per-visit multiply; bitwise
        # by construction for non-NaN rows — NaN rows take the
        # strict-order route below, whose dot reproduces the oracle's
        # NaN-compares-false behaviour)
        aos, ncount, extra = _device_forest(
            model, X.device, v4_key=("eif0", d, _row_kind(X.dtype)))
        return ext.score_forest(
            _rows_in_place(X), aos, ncount, forest.num_trees, extra["height"],
            c, finalize, _heap_for_call(aos, extra, d, X.dtype),
        )
    if nnz <= 5 and _eif_uniform_nnz(forest):
        elem = 4 if X.dtype == torch.float32 else 2  # bf16 / fp16
        dpad = d
        if elem == 2:
            while dpad % 4 != 2:
                dpad += 1
        else:
            while dpad % 2 != 1:
                dpad += 1
        mn = forest.feature.shape[1]
        lds = mn * (12 + nnz * 8) + 2 * 256 * dpad * elem
        if lds <= 150 * 1024:
            aos, ncount, extra = _device_forest(
                model, X.device, v4_key="eif_sparse")
            return ext.score_extended_sparse_v2(
                _rows_in_place(X), aos, extra["values"], extra["hidx"],
                extra["hw"], ncount, extra["height"], c, finalize,
            )
    # densified hyperplanes (nnz < d) carry weight 0 on unselected
    # coordinates: 0 * inf/NaN = NaN would route a row right where the
    # oracle never reads that coordinate, so a batch with a non-finite cell
    # takes the general strict-order kernel below (bitwise). nnz == d has
    # no zero-padded real column and stays unguarded: the dense bindings
    # rescore its non-finite rows in strict order themselves.
    if d <= 128 and (nnz == d or (
            nnz >= 6 and bool(torch.isfinite(X).all().item()))):
        if d <= 8:
            D = 8
        elif d <= 16:
            D = 16
        elif d <= 32:
            D = 32
        elif d <= 64:
            D = 64
        else:
            D = 128
        mn = forest.feature.shape[1]
        use_v3 = (X.dtype == torch.bfloat16
                  and os.environ.get("IFA_EIF_DENSE_V2") != "1")
        if use_v3:
            lds = mn * 12 + 16 + mn * (D // 8 + 1) * 16
            if lds <= 160 * 1024:
                aos, ncount, extra = _device_forest(
                    model, X.device, v4_key=("eif_dense3", D))
                return ext.score_extended_dense_v3(
                    _rows_in_place(X), aos, extra["values"], extra["hwp"],
                    ncount, extra["height"], c, finalize,
                )
        if d <= 64:  # v2's f32 staging exceeds LDS past D=64
            lds = mn * 12 + 16 + mn * (D // 4 + 1) * 16
            if lds <= 160 * 1024:
                aos, ncount, extra = _device_forest(
                    model, X.device, v4_key=("eif_dense", D))
                return ext.score_extended_dense_v2(
                    _rows_in_place(X), aos, extra["values"], extra["hw"],
                    ncount, extra["height"], c, finalize,
                )
        # deep forests overflow the dense kernel's LDS weight staging:
        # fall through to the general kernel (nodes from global if needed)
    aos, ncount, extra = _device_forest(model, X.device)
    return ext.score_extended_forest(
        _rows_in_place(X), aos, extra["hidx"], extra["hw"], ncount, c, finalize
    )


# ---------------------------------------------------------------------------
# per-feature attribution (docs/DESIGN.md §8)
# ---------------------------------------------------------------------------


def _explain_on_cpu(fn, forest, X: torch.Tensor, finalize: bool, why: str):
    """Forests past the packed-record caps: CPU oracle, result moved to X's
    device (a correctness path; there are no wide-record explain kernels)."""
    _log.warning(
        "feature_contributions: %s; computing on the CPU oracle", why)
    Xc = X.detach().float().cpu().contiguous().numpy()
    return torch.from_numpy(fn(forest, Xc, finalize)).to(X.device)


def _check_explain_input(X: torch.Tensor):
    if X.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError("feature_contributions expects float32, bfloat16 "
                         f"or float16 rows on the GPU, got {X.dtype}")


def explain_forest(model, X: torch.Tensor, finalize: bool = True) -> torch.Tensor:
    """Standard-forest contributions [N, d] float32 on X's device, bitwise
    equal to cpu_engine.feature_contributions."""
    from ..core import cpu_engine

    forest = model.forest
    d = int(X.shape[1])
    _check_explain_input(X)
    fmax = int(forest.feature.max(initial=-1))
    if fmax >= d:
        raise ValueError(
            f"the forest splits on feature {fmax} but rows have {d} columns")
    if not _packed_fits(forest, d):
        return _explain_on_cpu(
            cpu_engine.feature_contributions, forest, X, finalize,
            "forest exceeds the packed node format (15-bit node ids, "
            "12-bit feature ids)")
    ext = load_extension()
    aos, ncount, extra = _device_forest(
        model, X.device, v4_key=("explain", d, _row_kind(X.dtype)))
    return ext.explain_forest(_rows_in_place(X), aos, ncount, extra["height"],
                              finalize)


def explain_extended_forest(model, X: torch.Tensor,
                            finalize: bool = True) -> torch.Tensor:
    """EIF contributions [N, d] float32 on X's device, bitwise equal to
    cpu_engine.feature_contributions_extended at every extension level
    (one strict-order kernel, no routing)."""
    from ..core import cpu_engine

    forest = model.forest
    d = int(X.shape[1])
    _check_explain_input(X)
    internal = forest.feature >= 0
    cmax = (int(forest.hyper_idx[internal].max(initial=-1))
            if internal.any() else -1)
    if cmax >= d:
        raise ValueError(
            f"the forest splits on feature {cmax} but rows have {d} columns")
    if not _packed_fits(forest, d):
        return _explain_on_cpu(
            cpu_engine.feature_contributions_extended, forest, X, finalize,
            "forest exceeds the packed node format (15-bit node ids, "
            "12-bit hyperplane widths)")
    ext = load_extension()
    aos, ncount, extra = _device_forest(model, X.device, v4_key="eif_explain")
    return ext.explain_extended_forest(
        _rows_in_place(X), aos, extra["hidx"], extra["hw"], extra["dl"],
        extra["dr"], finalize)


# ---------------------------------------------------------------------------
# exact TreeSHAP, standard forests (docs/DESIGN.md §9)
# ---------------------------------------------------------------------------


def _shap_on_cpu(forest, X: torch.Tensor, finalize: bool, why: str):
    """CPU oracle, result moved to X's device (a correctness path)."""
    from ..core import cpu_engine

    _log.warning("shap_values: %s; computing on the CPU oracle", why)
    Xc = X.detach().float().cpu().contiguous().numpy()
    return torch.from_numpy(
        cpu_engine.shap_values(forest, Xc, finalize)).to(X.device)


def shap_forest(model, X: torch.Tensor, finalize: bool = True) -> torch.Tensor:
    """Standard-forest SHAP values [N, d] float32 on X's device, bitwise
    equal to cpu_engine.shap_values."""
    from ..core import cpu_engine

    forest = model.forest
    if isinstance(forest, ExtendedForest):
        raise ValueError("SHAP values are defined for standard forests only")
    d = int(X.shape[1])
    if X.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError("shap_values expects float32, bfloat16 or float16 "
                         f"rows on the GPU, got {X.dtype}")
    fmax = int(forest.feature.max(initial=-1))
    if fmax >= d:
        raise ValueError(
            f"the forest splits on feature {fmax} but rows have {d} columns")
    if not _packed_fits(forest, d):
        return _shap_on_cpu(
            forest, X, finalize,
            "forest exceeds the packed node format (15-bit node ids, "
            "12-bit feature ids)")
    max_m = cpu_engine.shap_tables(forest)["max_m"]
    if max_m > cpu_engine.SHAP_MAX_PATH_FEATURES:
        return _shap_on_cpu(
            forest, X, finalize,
            f"a root-to-leaf path splits on {max_m} distinct features, the "
            f"kernel holds {cpu_engine.SHAP_MAX_PATH_FEATURES}")
    ext = load_extension()
    table, tree_off, extra = _device_forest(
        model, X.device, v4_key=("shap", d, _row_kind(X.dtype)))
    return ext.shap_forest(_rows_in_place(X), table, extra["tree_off_host"],
                           tree_off, extra["wtab"], finalize)
