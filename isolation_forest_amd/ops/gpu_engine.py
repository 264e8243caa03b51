"""GPU engine orchestration: device builds and scoring via the HIP extension.

The canonical forest lives in host numpy (core/forest.py) — it is small
(MBs) next to the data (GBs-TBs). Feature subsets are drawn host-side and
bags on the device (sample_bags_device, bitwise the host sampler's), all
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

Standard forests past the 15-bit node ids (maxSamples > 16384) score through
compact level-order records, top levels in LDS and the tail from L2
(score_forest_deep; large_score_route), and fall back to the wide kernel
past that format's own caps.

``torch.sparse_csr`` matrices (standard forests inside the packed caps) are
scored without a dense copy by the tree-parallel walk of
ops/hip/csr_kernels.hip (score_forest_csr) over the same v4 pack, and built
from bags scattered out of the stored entries (build_forest); both bitwise
the dense calls on ``X.to_dense()``.
"""

from __future__ import annotations

import logging
import math
import os
import types

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


_CSR_DENSIFY = ("{} is not supported: densify the rows first (X.to_dense(); "
                "docs/API.md, Sparse input)")


def _first_true(mask: torch.Tensor) -> torch.Tensor:
    """0-d int64 tensor: index of the first True, or ``mask.numel()``."""
    n = mask.numel()
    if n == 0:
        return torch.zeros((), dtype=torch.int64, device=mask.device)
    return torch.where(mask.any(), mask.to(torch.uint8).argmax(),
                       torch.full((), n, dtype=torch.int64,
                                  device=mask.device))


def _csr_parts(X: torch.Tensor):
    """``(crow_indices, col_indices, values, N, d)`` of a 2-D
    ``torch.sparse_csr`` matrix, validated with torch ops on X's device and
    one host sync: ``crow`` non-decreasing from 0 to nnz, every column in
    ``[0, d)``, columns strictly ascending within a row. A duplicated or
    unsorted column has no agreed dense meaning, so it is refused with a
    ``ValueError`` that names the first offending row. The only temporaries
    are masks of one byte per stored entry and an int64 copy of ``crow``."""
    if X.layout != torch.sparse_csr or X.dim() != 2:
        raise ValueError("expected a 2-D torch.sparse_csr matrix, got "
                         f"layout {X.layout} with {X.dim()} dimensions")
    crow, col, values = X.crow_indices(), X.col_indices(), X.values()
    N, d = int(X.shape[0]), int(X.shape[1])
    _row_kind(values.dtype)
    if values.dim() != 1 or d < 1:
        raise ValueError("a sparse CSR matrix needs scalar values and at "
                         f"least one column; got values of shape "
                         f"{tuple(values.shape)} and d = {d}")
    nnz = int(values.shape[0])
    c64 = crow.to(torch.int64)
    bad_row = (c64[:-1] < 0) | (c64[1:] < c64[:-1]) | (c64[1:] > nnz)
    ends_ok = (c64[0] == 0) & (c64[-1] == nnz)
    cc = c64.clamp(0, nnz)  # safe to index with, whatever crow holds
    bad_col = (col < 0) | (col >= d)
    starts = torch.zeros(nnz + 1, dtype=torch.bool, device=col.device)
    starts[cc[:-1]] = True
    bad_ord = (col[1:] <= col[:-1]) & ~starts[1:nnz]
    e_col, e_ord = _first_true(bad_col), _first_true(bad_ord) + 1
    entries = torch.stack([e_col, e_ord])
    rows = torch.searchsorted(cc, entries, right=True) - 1
    r_crow, ok, e_col, e_ord, r_col, r_ord = torch.cat([
        torch.stack([_first_true(bad_row), ends_ok.to(torch.int64)]),
        entries, rows]).tolist()
    if r_crow < N or not ok:
        row = r_crow if r_crow < N else (0 if int(c64[0]) != 0 else N - 1)
        raise ValueError(
            f"sparse CSR input: crow_indices must be non-decreasing from 0 "
            f"to nnz = {nnz}; first offending row {row}")
    if e_col < nnz:
        raise ValueError(
            f"sparse CSR input: column index outside [0, {d}) in row {r_col}")
    if e_ord < nnz:
        raise ValueError(
            "sparse CSR input: column indices must be strictly ascending "
            f"within a row (no duplicates); first offending row {r_ord}")
    return crow.contiguous(), col.contiguous(), values.contiguous(), N, d


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


# ---------------------------------------------------------------------------
# on-device bag sampling (ops/hip/bag_kernels.hip, docs/DESIGN.md §2c)
# ---------------------------------------------------------------------------

# Largest bag the one-block-per-tree LDS sampler takes: its hash table of
# 8 bytes * (next power of two >= 2n) is 128 KB there (kBagLdsMaxSamples in
# bindings.cpp, which checks it). Larger bags use the global-table kernels.
BAG_LDS_MAX_SAMPLES = 8192


def bag_device_fits(total_rows: int, n: int) -> bool:
    """Whether ``sample_bags_device`` takes bags of ``n`` out of
    ``total_rows`` rows: draws are 32-bit and the all-ones word marks an empty
    table entry, so ``total_rows <= 2^32 - 1``; slot ids as in the large
    builders, ``n <= 2^30``."""
    return 1 <= int(total_rows) <= (1 << 32) - 1 and int(n) <= 1 << 30


def bag_device_enabled(total_rows: int, n: int) -> bool:
    """The estimators' switch: the device sampler unless ``IFA_BAG_DEVICE=0``
    (A/B runs, escape hatch) or the shape does not fit it."""
    return (os.environ.get("IFA_BAG_DEVICE", "1") != "0"
            and bag_device_fits(total_rows, n))


def _bag_table_cap(n: int) -> int:
    cap = 2
    while cap < 2 * n:
        cap <<= 1
    return cap


def _bag_sampler_bytes(total_rows: int, n: int, bootstrap: bool) -> int:
    """Device bytes per tree the sampler allocates next to its output: the
    global route's table and loser flags, or the dense regime's key matrix
    with torch.sort's outputs and workspace (4 int64 per row)."""
    if bootstrap or n <= 0:
        return 0
    if 2 * n > total_rows:
        return 32 * total_rows
    if n <= BAG_LDS_MAX_SAMPLES:
        return 0
    return 8 * _bag_table_cap(n) + n


def sample_bags_device(total_rows: int, num_trees: int, num_samples: int,
                       seed: int, bootstrap: bool, tree_id_offset: int = 0,
                       row_offset: int = 0, device="cuda") -> torch.Tensor:
    """``cpu_engine.sample_bags`` drawn on the GPU: the same int64
    ``[num_trees, num_samples]`` matrix, bitwise, as a tensor on ``device``
    (what ``bag_gather`` and the large builders read). Routes: bootstrap (one
    draw per slot); without replacement and ``2n <= N`` a per-tree hash table
    from value to smallest slot, in LDS up to ``BAG_LDS_MAX_SAMPLES`` rows a
    bag and in global memory above (one host sync per redraw round); ``2n >
    N`` the oracle's permutation as a ``torch.sort`` of composite keys."""
    ext = load_extension()
    N, T, n = int(total_rows), int(num_trees), int(num_samples)
    if not bootstrap and n > N:
        raise ValueError("cannot sample more rows than the dataset holds")
    if not bag_device_fits(N, n):
        raise ValueError(
            f"device bag sampling needs total_rows <= 2^32 - 1 and "
            f"num_samples <= 2^30 (got {N}, {n})")
    device = torch.device(device)
    with torch.cuda.device(device):
        out = torch.empty((T, n), dtype=torch.int64, device=device)
        if T == 0 or n == 0:
            return out
        if bootstrap:
            ext.bag_bootstrap(out, N, seed, tree_id_offset, row_offset)
            return out
        per_tree = _bag_sampler_bytes(N, n, False)
        if 2 * n > N:
            chunk = max(1, BUILD_LARGE_BUDGET_BYTES // per_tree)
            for lo in range(0, T, chunk):
                hi = min(T, lo + chunk)
                keys = torch.empty((hi - lo, N), dtype=torch.int64,
                                   device=device)
                ext.bag_dense_keys(keys, seed, tree_id_offset + lo)
                first = torch.sort(keys, dim=1).values[:, :n]
                out[lo:hi] = (first & 0xFFFFFFFF) + row_offset
                del keys, first
            return out
        if n <= BAG_LDS_MAX_SAMPLES:
            v = os.environ.get("IFA_BAG_LDS_THREADS")
            ext.bag_sample_lds(out, N, seed, tree_id_offset, row_offset,
                               int(v) if v else 0)
            return out
        # grid.y carries the tree; the loser total is an int32
        chunk = max(1, min(65535, (2 ** 31 - 1) // n,
                           BUILD_LARGE_BUDGET_BYTES // per_tree))
        for lo in range(0, T, chunk):
            hi = min(T, lo + chunk)
            ext.bag_sample_global(out[lo:hi], N, seed, tree_id_offset + lo,
                                  row_offset)
        return out


def _bag_tensor(bag_idx, device) -> torch.Tensor:
    """Bags as the kernels read them: an int64 device tensor as it is (no
    copy crosses PCIe), a numpy matrix uploaded."""
    if isinstance(bag_idx, torch.Tensor):
        if bag_idx.dtype != torch.int64 or bag_idx.device != device:
            raise ValueError(
                f"bag_idx tensor must be int64 on {device}; got "
                f"{bag_idx.dtype} on {bag_idx.device}")
        return bag_idx.contiguous()
    return torch.from_numpy(np.ascontiguousarray(bag_idx)).to(device)


def build_forest(X: torch.Tensor, bag_idx, feat_sub: np.ndarray,
                 seed: int, rp, tree_id_offset: int = 0) -> Forest:
    ext = load_extension()
    device = X.device
    n = rp.num_samples
    height_limit = int(math.ceil(math.log2(max(n, 2))))
    max_nodes = 2 * n - 1
    bag_t = _bag_tensor(bag_idx, device)
    fs_t = torch.from_numpy(np.ascontiguousarray(feat_sub, dtype=np.int32)).to(device)
    if X.layout == torch.sparse_csr:
        # the same f32 [T, n, d] bags, scattered from the stored entries
        if n > 16384:
            raise NotImplementedError(_CSR_DENSIFY.format(
                "maxSamples > 16384 on a sparse CSR matrix"))
        crow, col, values, _, d = _csr_parts(X)
        bags = ext.bag_gather_csr(crow, col, values, d, bag_t)
    else:
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


def build_extended_forest(X: torch.Tensor, bag_idx,
                          feat_sub: np.ndarray, seed: int, rp,
                          tree_id_offset: int = 0) -> ExtendedForest:
    ext = load_extension()
    device = X.device
    n = rp.num_samples
    height_limit = int(math.ceil(math.log2(max(n, 2))))
    max_nodes = 2 ** (height_limit + 1) - 1
    nnz = min(rp.extension_level + 1, rp.num_features)
    bag_t = _bag_tensor(bag_idx, device)
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


def _large_chunk_bags(bag_idx, lo: int, hi: int, X: torch.Tensor, n: int,
                      seed: int, bootstrap: bool, tree_id_offset: int):
    """Trees ``lo:hi`` of the bags on X's device: a slice of ``bag_idx``, or
    with ``bag_idx=None`` drawn there by global tree id, so that the whole
    ``[T, n]`` index matrix never exists."""
    if bag_idx is None:
        return sample_bags_device(int(X.shape[0]), hi - lo, n, seed, bootstrap,
                                  tree_id_offset=tree_id_offset + lo,
                                  device=X.device)
    return _bag_tensor(bag_idx[lo:hi], X.device)


def build_forest_large(X: torch.Tensor, bag_idx,
                       feat_sub: np.ndarray, seed: int, rp,
                       tree_id_offset: int = 0, chunk_trees=None,
                       return_depth: bool = False, bootstrap: bool = False):
    """``build_forest`` for bags of any size (the models use it above the
    LDS builders' 16384 rows): rows are read in place from ``X``, no f32
    ``[T, n, d]`` gather is made, and the trees are built ``chunk_trees`` at
    a time (``None``: as many as ``BUILD_LARGE_BUDGET_BYTES`` holds). The
    forest is bitwise ``cpu_engine.build_forest``'s. It carries no device
    tensors: forests this size score through the deep records (standard;
    large_score_route) or the host-packed wide formats.
    ``return_depth=True`` returns ``(forest, depth)`` with the kernel's
    per-node depths ``[T, max_nodes]``. ``bag_idx`` is a numpy matrix, an
    int64 tensor on X's device, or ``None``: each chunk's bags are then drawn
    on the device (``sample_bags_device`` with ``bootstrap``)."""
    ext = load_extension()
    device = X.device
    n = rp.num_samples
    height_limit = int(math.ceil(math.log2(max(n, 2))))
    max_nodes = 2 * n - 1
    Xr = _rows_in_place(X)
    lut = _leaf_lut(n, device)
    fs = np.ascontiguousarray(feat_sub, dtype=np.int32)
    T = int(fs.shape[0] if bag_idx is None else bag_idx.shape[0])
    drawn = (_bag_sampler_bytes(int(X.shape[0]), n, bootstrap)
             if bag_idx is None else 0)
    chunk = _large_chunk_trees(T, 16 * n + 28 * max_nodes + drawn, chunk_trees)
    f_np = np.empty((T, max_nodes), dtype=np.int32)
    v_np = np.empty((T, max_nodes), dtype=np.float32)
    r_np = np.empty((T, max_nodes), dtype=np.int32)
    c_np = np.empty((T, max_nodes), dtype=np.int64)
    nc_np = np.empty((T,), dtype=np.int32)
    d_np = np.empty((T, max_nodes), dtype=np.int32) if return_depth else None
    for lo in range(0, T, chunk):
        hi = min(T, lo + chunk)
        bag_t = _large_chunk_bags(bag_idx, lo, hi, X, n, seed, bootstrap,
                                  tree_id_offset)
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


def build_extended_forest_large(X: torch.Tensor, bag_idx,
                                feat_sub: np.ndarray, seed: int, rp,
                                tree_id_offset: int = 0, chunk_trees=None,
                                return_depth: bool = False,
                                bootstrap: bool = False):
    """``build_extended_forest`` for bags of any size; see
    ``build_forest_large``."""
    ext = load_extension()
    device = X.device
    n = rp.num_samples
    height_limit = int(math.ceil(math.log2(max(n, 2))))
    max_nodes = 2 ** (height_limit + 1) - 1
    nnz = min(rp.extension_level + 1, rp.num_features)
    Xr = _rows_in_place(X)
    lut = _leaf_lut(n, device)
    fs = np.ascontiguousarray(feat_sub, dtype=np.int32)
    T = int(fs.shape[0] if bag_idx is None else bag_idx.shape[0])
    drawn = (_bag_sampler_bytes(int(X.shape[0]), n, bootstrap)
             if bag_idx is None else 0)
    chunk = _large_chunk_trees(
        T, 16 * n + (28 + 8 * nnz) * max_nodes + drawn, chunk_trees)
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
        bag_t = _large_chunk_bags(bag_idx, lo, hi, X, n, seed, bootstrap,
                                  tree_id_offset)
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


def _nodes_deep_host(forest, kind):
    """Host half of the deep pack (ops/hip/deep_kernels.hip): the pre-order
    arrays TRIMMED to the largest node_count, as three int32 matrices
    [T, M0] (feature id, -1 for leaves and dead slots; pre-order right
    child; integer key threshold of the row kind for an internal node, f32
    bits of depth + c(m) for a leaf), the node counts and the forest's
    depth. Same key and leaf-value math as _nodes_packed_wide, on 2n - 1
    minus the padding columns; deep_level_order reorders on the device."""
    nc = np.ascontiguousarray(forest.node_count, dtype=np.int32)
    m0 = max(int(nc.max(initial=1)), 1)
    feat = np.ascontiguousarray(forest.feature[:, :m0])
    right = np.ascontiguousarray(forest.right[:, :m0], dtype=np.int32)
    internal = feat >= 0
    leaf = feat == Forest.LEAF
    depth = _node_depths(feat, right)
    w = np.zeros(feat.shape, dtype=np.uint32)
    if internal.any():
        v64 = getattr(forest, "value64", None)
        trimmed = types.SimpleNamespace(
            value=forest.value[:, :m0],
            value64=None if v64 is None else v64[:, :m0])
        w[internal] = _threshold_keys(
            _split_thresholds32(trimmed)[internal], kind)
    leafval = depth.astype(np.float32) + forest.value[:, :m0].astype(
        np.float32)
    w[leaf] = leafval[leaf].astype(np.float32).view(np.uint32)
    live = internal | leaf
    max_depth = int(depth[live].max()) if live.any() else 0
    return (np.where(internal, feat, -1).astype(np.int32), right,
            w.view(np.int32), nc, max(max_depth, 1))


def _nodes_explain_deep_host(forest, kind):
    """Host half of the explain deep pack (ops/hip/deep_kernels.hip):
    _nodes_deep_host's trimmed pre-order arrays (feature id, right child,
    key threshold of the row kind) plus the f32 bits of the two edge deltas,
    int32 [T, M0] each, from cpu_engine.explain_tables_trimmed — the CPU
    oracle's deltas without its [T, 2n - 1] float64 sweep. Leaf slots of
    the threshold array still hold _nodes_deep_host's leaf values; the
    reorder on the device writes threshold 0 into every leaf record.
    Returns (feat, right, w, dl, dr, node_count, max_depth)."""
    from ..core.cpu_engine import explain_tables_trimmed

    feat, right, w, nc, max_depth = _nodes_deep_host(forest, kind)
    tabs = explain_tables_trimmed(forest)
    return (feat, right, w, np.ascontiguousarray(tabs["dl"]).view(np.int32),
            np.ascontiguousarray(tabs["dr"]).view(np.int32), nc, max_depth)


def _nodes_explain_eif_deep_host(forest):
    """Host half of the explain eif deep pack (ops/hip/deep_kernels.hip):
    the pre-order arrays of an extended forest TRIMMED to the largest
    node_count. int32 [T, M0]: the coordinate count k of an internal node
    (-1 for leaves and dead slots), the pre-order right child, the f32 bits
    of the offset; int32 [T, M0, nnz]: the coordinates and the f32 bits of
    the weights and of the two edges' shares, from
    cpu_engine.explain_tables_trimmed — the CPU oracle's shares without its
    [T, 2^(H+1) - 1, nnz] float64 sweep. Returns (feat, right, w,
    node_count, hidx, hw, dl, dr, max_depth)."""
    from ..core.cpu_engine import explain_tables_trimmed

    nc = np.ascontiguousarray(forest.node_count, dtype=np.int32)
    m0 = max(int(nc.max(initial=1)), 1)
    feat = np.ascontiguousarray(forest.feature[:, :m0])
    right = np.ascontiguousarray(forest.right[:, :m0], dtype=np.int32)
    internal = feat >= 0
    live = internal | (feat == ExtendedForest.LEAF)
    depth = _node_depths(feat, right)
    max_depth = int(depth[live].max()) if live.any() else 0
    tabs = explain_tables_trimmed(forest)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)  # noqa: E731
    return (np.where(internal, feat, -1).astype(np.int32), right,
            bits(forest.value[:, :m0]), nc,
            np.ascontiguousarray(forest.hyper_idx[:, :m0], dtype=np.int32),
            bits(forest.hyper_w[:, :m0]), bits(tabs["dl"]), bits(tabs["dr"]),
            max(max_depth, 1))


def _nodes_eif_deep_host(forest):
    """Host half of the eif deep pack (ops/hip/deep_kernels.hip): the
    pre-order arrays of an extended forest TRIMMED to the largest
    node_count, with no [T, 2^(H+1) - 1, ...] temporary. int32 [T, M0]: the
    coordinate count k of an internal node (-1 for leaves and dead slots),
    the pre-order right child, and one value word a node: the f32 bits of
    the offset, or for a leaf of f32(depth) + f32(value), what
    cpu_engine.path_lengths_extended adds per tree; int32 [T, M0, nnz]: the
    coordinates and the f32 bits of the weights. Returns (feat, right, vw,
    node_count, hidx, hw, max_depth)."""
    nc = np.ascontiguousarray(forest.node_count, dtype=np.int32)
    m0 = max(int(nc.max(initial=1)), 1)
    feat = np.ascontiguousarray(forest.feature[:, :m0])
    right = np.ascontiguousarray(forest.right[:, :m0], dtype=np.int32)
    internal = feat >= 0
    leaf = feat == ExtendedForest.LEAF
    depth = _node_depths(feat, right)
    value = np.ascontiguousarray(forest.value[:, :m0], dtype=np.float32)
    vw = np.where(leaf, depth.astype(np.float32) + value, value)
    live = internal | leaf
    max_depth = int(depth[live].max()) if live.any() else 0
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.int32)  # noqa: E731
    return (np.where(internal, feat, -1).astype(np.int32), right, bits(vw),
            nc, np.ascontiguousarray(forest.hyper_idx[:, :m0], dtype=np.int32),
            bits(forest.hyper_w[:, :m0]), max(max_depth, 1))


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


def _shap_deep_packed(forest, kind):
    """Deep leaf stream for shap_forest_deep_kernel (layout at the top of
    ops/hip/shap_kernels.hip) from cpu_engine.shap_tables, for one row kind:
    per leaf {f64 L, m}, z[m], then for 16-bit rows e[m] = lo16 | hi16 << 16
    | feature << 32, for f32 rows iv[m] = lo | hi << 32 and ceil(m / 4)
    words of 16-bit feature ids.

    The intervals are _shap_packed's (§9), but the threshold keys are
    computed for the path nodes the tables name only: no [T, 2n - 1]
    temporary. For 16-bit rows the inclusive widened interval [lo, hi] is
    stored in the domain of the unwidened key k, widen(k) = k << 16 | 0xFFFF:
    lo <= widen(k) <=> lo >> 16 <= k, widen(k) <= hi <=> k <= (hi - 0xFFFF)
    >> 16 (negative: no key passes, the empty interval lo16 = 1, hi16 = 0).
    Returns (words uint64 [W], tree_off int64 [T + 1] in words)."""
    from ..core.cpu_engine import shap_tables

    kind = _row_kind(kind)
    tabs = shap_tables(forest)
    T = forest.num_trees
    pt, pv = tabs["pn_tree"], tabs["pn_node"]
    v64 = getattr(forest, "value64", None)
    splits = types.SimpleNamespace(
        value=forest.value[pt, pv],
        value64=None if v64 is None else v64[pt, pv])
    pn_key = _threshold_keys(_split_thresholds32(splits), kind).astype(
        np.int64)
    n_ent = len(tabs["ent_feat"])
    pn_ent = np.repeat(np.arange(n_ent, dtype=np.int64),
                       np.diff(tabs["ent_pn_off"]))
    left = tabs["pn_left"]
    lo = np.zeros(n_ent, dtype=np.int64)
    hi = np.full(n_ent, 1 << 32, dtype=np.int64)  # exclusive, none yet
    np.maximum.at(lo, pn_ent[~left], pn_key[~left])
    np.minimum.at(hi, pn_ent[left], pn_key[left])
    never = hi == 0
    lo[never] = 1
    hi = np.where(never, 0, hi - 1)  # inclusive
    feat = tabs["ent_feat"].astype(np.uint64)
    assert n_ent == 0 or int(feat.max()) <= 4094
    k16 = kind != "f32"
    if k16:
        lo = lo >> 16
        hi = (hi - 0xFFFF) >> 16
        never = (hi < lo) | (hi < 0)
        lo[never], hi[never] = 1, 0
        ent_word1 = (lo.astype(np.uint64) | (hi.astype(np.uint64)
                                             << np.uint64(16))
                     | (feat << np.uint64(32)))
    else:
        ent_word1 = lo.astype(np.uint64) | (hi.astype(np.uint64)
                                            << np.uint64(32))

    leaf_m = tabs["leaf_m"]
    ent_off = tabs["leaf_ent_off"]
    n_leaf = len(leaf_m)
    leaf_words = 2 + 2 * leaf_m + (0 if k16 else (leaf_m + 3) // 4)
    leaf_word = np.zeros(n_leaf + 1, dtype=np.int64)
    np.cumsum(leaf_words, out=leaf_word[1:])
    total = int(leaf_word[-1])
    words = np.zeros(total, dtype=np.uint64)
    words[leaf_word[:-1]] = tabs["leaf_L"].view(np.uint64)
    words[leaf_word[:-1] + 1] = leaf_m.astype(np.uint64)
    ent_leaf = np.repeat(np.arange(n_leaf, dtype=np.int64), leaf_m)
    k = np.arange(n_ent, dtype=np.int64) - ent_off[ent_leaf]  # slot in leaf
    z_word = leaf_word[ent_leaf] + 2 + k
    words[z_word] = tabs["ent_z"].view(np.uint64)
    words[z_word + leaf_m[ent_leaf]] = ent_word1
    if not k16:
        f_word = leaf_word[ent_leaf] + 2 + 2 * leaf_m[ent_leaf] + k // 4
        np.bitwise_or.at(words, f_word,
                         feat << (np.uint64(16) * (k % 4).astype(np.uint64)))
    tree_off = np.ascontiguousarray(leaf_word[tabs["tree_leaf_off"]])
    assert tree_off[0] == 0 and tree_off[T] == total
    return words, tree_off


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


def _eif_explain_dense_packed(forest, D: int):
    """The ("eif_explain_dense", D) pack of explain_extended_dense_kernel
    (ops/hip/explain_kernels.hip), for forests extended_explain_route calls
    "dense" (every internal node nnz distinct coordinates below D):

    * nodes int32 [T, mn, 2]: right | slot << 16 and the f32 offset bits,
      slot being the node's rank among its tree's internal nodes; leaves and
      pads hold their own id and 0;
    * rows float32 [T, MI, 3, D]: per slot the hyperplane weights and the
      delta_left / delta_right shares of cpu_engine.explain_tables, scattered
      to their coordinates' columns (copies, nothing recomputed); every
      other column is +0.0;
    * ncount, icount int32 [T] (live records, internal nodes) and the
      forest's height."""
    from ..core.cpu_engine import explain_tables

    tabs = explain_tables(forest)
    feat = forest.feature
    T, mn = feat.shape
    internal = feat >= 0
    live = internal | (feat == ExtendedForest.LEAF)
    slot = np.cumsum(internal, axis=1, dtype=np.int32) - 1
    icount = internal.sum(axis=1).astype(np.int32)
    ids = np.broadcast_to(np.arange(mn, dtype=np.int32)[None, :], (T, mn))
    nodes = np.empty((T, mn, 2), dtype=np.int32)
    nodes[..., 0] = np.where(
        internal, forest.right.astype(np.int32) | (slot << 16), ids)
    nodes[..., 1] = np.where(internal, forest.value.view(np.int32), 0)
    rows = np.zeros((T, max(int(icount.max(initial=0)), 1), 3, D),
                    dtype=np.float32)
    ti, vi = np.nonzero(internal)
    at = (ti[:, None], slot[ti, vi][:, None])
    cols = forest.hyper_idx[ti, vi].astype(np.int64)
    rows[at + (0, cols)] = forest.hyper_w[ti, vi]
    rows[at + (1, cols)] = tabs["dl"][ti, vi]
    rows[at + (2, cols)] = tabs["dr"][ti, vi]
    depth = _node_depths(feat, forest.right)
    max_depth = int(depth[live].max()) if live.any() else 0
    return (nodes, rows,
            np.ascontiguousarray(forest.node_count, dtype=np.int32), icount,
            max_depth)


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
    ("deep", d, stage, kind), ("eif0", d, kind), ("explain", d, kind),
    ("explain_deep", d, stage, kind), ("shap", d, kind),
    ("shap_deep", d, kind) — are keyed
    on the row KIND, not on "is it 16-bit": bf16 and fp16 keys differ, and
    u32 records under a u16 kernel score silently wrong. The "shap" and
    "shap_deep" entries are (table words, per-tree word offsets, {host
    offsets, weights}).
    ("explain_eif_deep", stage), ("eif_deep", stage) and
    ("eif_explain_dense", D) hold f32 offsets and weights and serve every
    row kind."""
    if isinstance(v4_key, tuple) and v4_key[0] not in (
            "eif_dense", "eif_dense3", "explain_eif_deep", "eif_deep",
            "eif_explain_dense"):
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
        elif isinstance(v4_key, tuple) and v4_key[0] == "shap_deep":
            # ("shap_deep", d, kind): as "shap", the deep leaf stream and
            # the [33, 32] weights
            from ..core.cpu_engine import (SHAP_DEEP_MAX_PATH_FEATURES,
                                           shap_weights)

            words, tree_off = _shap_deep_packed(forest, v4_key[2])
            aos = torch.from_numpy(words.view(np.int64)).to(device)
            ncount = torch.from_numpy(tree_off).to(device)  # word offsets
            extra["tree_off_host"] = torch.from_numpy(tree_off)
            extra["wtab"] = torch.from_numpy(
                shap_weights(SHAP_DEEP_MAX_PATH_FEATURES)).to(device)
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
        elif isinstance(v4_key, tuple) and v4_key[0] == "eif_explain_dense":
            # ("eif_explain_dense", D): aos = the node records, ncount =
            # live records a tree, extra["rows"] = the dense weight and
            # share rows, extra["icount"] = internal nodes a tree
            nodes, rows, nc, ic, max_depth = _eif_explain_dense_packed(
                forest, v4_key[1])
            aos = torch.from_numpy(nodes).to(device)
            ncount = torch.from_numpy(nc).to(device)
            extra["rows"] = torch.from_numpy(rows).to(device)
            extra["icount"] = torch.from_numpy(ic).to(device)
            extra["height"] = max_depth
        elif isinstance(v4_key, tuple) and v4_key[0] == "wide":
            packed, max_depth = _nodes_packed_wide(forest, v4_key[1])
            aos = torch.from_numpy(packed).to(device)
            ncount = torch.from_numpy(
                np.ascontiguousarray(forest.node_count, dtype=np.int32)
            ).to(device)
            extra["height"] = max_depth
        elif isinstance(v4_key, tuple) and v4_key[0] == "deep":
            # ("deep", d, stage, kind): aos = the level-order records,
            # ncount = lds_levels, both made on the device
            from . import load_extension as _packing_extension

            feat, right, w, nc, max_depth = _nodes_deep_host(
                forest, v4_key[3])
            aos, ncount = _packing_extension().deep_level_order(
                torch.from_numpy(feat).to(device),
                torch.from_numpy(right).to(device),
                torch.from_numpy(w).to(device),
                torch.from_numpy(nc).to(device), v4_key[1], v4_key[2])
            extra["height"] = max_depth
        elif isinstance(v4_key, tuple) and v4_key[0] == "explain_deep":
            # ("explain_deep", d, stage, kind): as "deep", 16-byte records
            from . import load_extension as _packing_extension

            feat, right, w, dl, dr, nc, max_depth = _nodes_explain_deep_host(
                forest, v4_key[3])
            aos, ncount = _packing_extension().explain_deep_level_order(
                *(torch.from_numpy(a).to(device)
                  for a in (feat, right, w, dl, dr, nc)),
                v4_key[1], v4_key[2])
            extra["height"] = max_depth
        elif isinstance(v4_key, tuple) and v4_key[0] == "explain_eif_deep":
            # ("explain_eif_deep", stage): aos = the level-order node
            # records, ncount = lds_levels, extra["payload"] = the
            # per-coordinate entries, all made on the device
            from . import load_extension as _packing_extension

            *arrays, max_depth = _nodes_explain_eif_deep_host(forest)
            aos, extra["payload"], ncount = \
                _packing_extension().explain_eif_deep_pack(
                    *(torch.from_numpy(a).to(device) for a in arrays),
                    max(_coord_range(forest)[1], 0) + 1, v4_key[1])
            extra["height"] = max_depth
        elif isinstance(v4_key, tuple) and v4_key[0] == "eif_deep":
            # ("eif_deep", stage): aos = the level-order node records,
            # ncount = lds_levels, extra["hyper"] = the {coordinate, w}
            # entries, all made on the device
            from . import load_extension as _packing_extension

            *arrays, max_depth = _nodes_eif_deep_host(forest)
            aos, extra["hyper"], ncount = \
                _packing_extension().eif_deep_pack(
                    *(torch.from_numpy(a).to(device) for a in arrays),
                    max(_coord_range(forest)[1], 0) + 1, v4_key[1])
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


# Largest node_count the deep records hold: links are 20 bits.
DEEP_MAX_NODES = 1 << 20


def _feature_max(forest) -> int:
    """Largest split feature id (0 for a forest of leaves), cached on the
    forest: a pass over [T, 2n - 1], made once."""
    fmax = getattr(forest, "_feature_max", None)
    if fmax is None:
        fmax = forest._feature_max = int(forest.feature.max(initial=0))
    return fmax


def _deep_fits(forest, d: int) -> bool:
    """True when the deep records (ops/hip/deep_kernels.hip) can represent
    this standard forest: 20-bit links over the TRIMMED trees (node_count,
    not the 2n - 1 array width), 12-bit feature ids with d as the leaf
    sentinel."""
    if isinstance(forest, ExtendedForest):
        return False
    if int(np.max(forest.node_count, initial=1)) > DEEP_MAX_NODES:
        return False
    return _feature_max(forest) <= 4094 and d <= 4094


def _deep_stage(kind: str, d: int) -> int:
    """Records per tree the deep walk stages for these rows now (0: the key
    tile leaves no room). Asked of the package's extension, like the packing
    helpers: a routing proxy installed on this module sees scoring calls."""
    from . import load_extension as _packing_extension

    return int(_packing_extension().deep_stage(kind, int(d)))


def _eif_deep_stage(kind: str, d: int, nnz: int) -> int:
    """Node records per tree the deep EIF scoring walk stages for these rows
    and this hyperplane width now (0: the row tile leaves no room); see
    _deep_stage."""
    from . import load_extension as _packing_extension

    return int(_packing_extension().eif_deep_stage(kind, int(d), int(nnz)))


def large_score_route(forest, d: int, dtype) -> str:
    """The kernel family that scores a forest past the packed 15-bit node
    ids: ``"deep"`` (compact level-order records, top levels in LDS, tail
    from L2) or ``"wide"`` (int4 records, one global read per visit; for an
    extended forest the entries of the hyperplane too).
    ``IFA_SCORE_DEEP=0`` keeps the wide route; so do forests past
    ``DEEP_MAX_NODES`` nodes a tree or 4094 features, and rows too wide for
    the tile to leave a stage in LDS. An extended forest also stays wide
    with a hyperplane coordinate outside ``[0, min(d - 1, 4094)]`` or more
    than 4094 coordinates a hyperplane."""
    if os.environ.get("IFA_SCORE_DEEP", "1") == "0":
        return "wide"
    if isinstance(forest, ExtendedForest):
        if int(np.max(forest.node_count, initial=1)) > DEEP_MAX_NODES:
            return "wide"
        cmin, cmax = _coord_range(forest)
        if cmin < 0 or cmax > min(d - 1, 4094) or max(d, forest.nnz) > 4094:
            return "wide"
        stage = _eif_deep_stage(_row_kind(dtype), d, forest.nnz)
        return "deep" if stage > 0 else "wide"
    if not _deep_fits(forest, d):
        return "wide"
    return "deep" if _deep_stage(_row_kind(dtype), d) > 0 else "wide"


def score_forest(model, X: torch.Tensor, finalize: bool = True) -> torch.Tensor:
    ext = load_extension()
    forest = model.forest
    d = int(X.shape[1])
    kind = _row_kind(X.dtype)
    c = float(avg_path_length(forest.num_samples))
    if not _packed_fits(forest, d):
        if large_score_route(forest, d, kind) == "deep":
            stage = _deep_stage(kind, d)
            records, lds_levels, extra = _device_forest(
                model, X.device, v4_key=("deep", d, stage, kind))
            return ext.score_forest_deep(
                _rows_in_place(X), records, lds_levels, forest.num_trees,
                extra["height"], stage, c, finalize,
            )
        # past the deep records' caps too (or IFA_SCORE_DEEP=0): wide int4
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


def score_forest_csr(model, X: torch.Tensor,
                     finalize: bool = True) -> torch.Tensor:
    """``score_forest`` for a ``torch.sparse_csr`` matrix on the device,
    bitwise the dense call on ``X.to_dense()``: an absent cell is +0.0, and
    no dense copy is made (ops/hip/csr_kernels.hip walks the (d, kind) pack
    of the dense route). Standard forests inside the packed caps only."""
    ext = load_extension()
    forest = model.forest
    if isinstance(forest, ExtendedForest):
        raise NotImplementedError(_CSR_DENSIFY.format(
            "an extended forest on a sparse CSR matrix"))
    crow, col, values, N, d = _csr_parts(X)
    kind = _row_kind(values.dtype)
    if not _packed_fits(forest, d):
        raise NotImplementedError(_CSR_DENSIFY.format(
            "a forest past maxSamples 16384 or 4094 features on a sparse "
            "CSR matrix"))
    c = float(avg_path_length(forest.num_samples))
    aos, ncount, extra = _device_forest(model, X.device, v4_key=(d, kind))
    return ext.score_forest_csr(
        crow, col, values, N, d, aos, ncount.contiguous(), forest.num_trees,
        extra["height"], c, finalize,
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


def score_extended_forest_deep(model, X: torch.Tensor,
                               finalize: bool = True) -> torch.Tensor:
    """Scores an extended forest whose node arrays are wider than 32767 on
    the deep route (score_extended_deep_kernel), where ``large_score_route``
    says ``"deep"``; anything else is an error, not a fall-back. Bitwise
    equal to cpu_engine.score_extended_forest, like the wide kernel."""
    forest = model.forest
    d = int(X.shape[1])
    kind = _row_kind(X.dtype)
    if large_score_route(forest, d, kind) != "deep":
        raise ValueError(
            f"large_score_route keeps {kind} rows of {d} columns on the wide "
            "kernel for this forest; score it with score_extended_forest")
    stage = _eif_deep_stage(kind, d, forest.nnz)
    nodes, lds_levels, extra = _device_forest(
        model, X.device, v4_key=("eif_deep", stage))
    return load_extension().score_extended_deep(
        _rows_in_place(X), nodes, extra["hyper"], lds_levels,
        forest.num_trees, extra["height"], stage,
        float(avg_path_length(forest.num_samples)), finalize, forest.nnz)


def score_extended_forest(model, X: torch.Tensor, finalize: bool = True) -> torch.Tensor:
    """Scores an extended forest on the packed routes, and past their caps
    (node arrays wider than 32767, more than 4094 coordinates) on the wide
    kernel, always. The deep route for large bags is a separate entry point,
    score_extended_forest_deep, which ExtendedIsolationForestModel.score
    picks with large_score_route, as the model picks
    build_extended_forest_large for the build."""
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
            rowtile=False,  # extended forests keep the v4 / heap walks
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


def _explain_deep_stage(kind: str, d: int) -> int:
    """Records per tree the deep explain walk stages for these rows now (0:
    the key tile leaves no room); see _deep_stage."""
    from . import load_extension as _packing_extension

    return int(_packing_extension().explain_deep_stage(kind, int(d)))


def _explain_eif_deep_stage(kind: str, d: int, nnz: int) -> int:
    """Node records per tree the deep EIF explain walk stages for these rows
    and this hyperplane width now (0: the tiles leave no room); see
    _deep_stage."""
    from . import load_extension as _packing_extension

    return int(_packing_extension().explain_eif_deep_stage(
        kind, int(d), int(nnz)))


def _coord_range(forest):
    """(smallest, largest) hyperplane coordinate over the internal nodes of
    an extended forest, (0, -1) for a forest of leaves; cached on the forest
    like _feature_max: a pass over [T, 2^(H+1) - 1, nnz], made once."""
    rng = getattr(forest, "_coord_range", None)
    if rng is None:
        internal = forest.feature >= 0
        rng = (0, -1)
        if internal.any():
            idx = forest.hyper_idx[internal]
            rng = (int(idx.min()), int(idx.max()))
        forest._coord_range = rng
    return rng


def large_explain_route(forest, d: int, dtype) -> str:
    """Where ``explain_forest`` and ``explain_extended_forest`` attribute a
    forest past the packed 15-bit node ids: ``"deep"`` (explain_forest_deep /
    explain_extended_deep: level-order records, top levels in LDS, tail from
    L2) or ``"cpu"`` (the oracle, with a logged warning).
    ``IFA_EXPLAIN_DEEP=0`` keeps the CPU path; so do forests past
    ``DEEP_MAX_NODES`` nodes a tree or 4094 features (extended: coordinates,
    hyperplane widths), and rows too wide for the tiles to leave a stage in
    LDS."""
    if os.environ.get("IFA_EXPLAIN_DEEP", "1") == "0":
        return "cpu"
    if isinstance(forest, ExtendedForest):
        if int(np.max(forest.node_count, initial=1)) > DEEP_MAX_NODES:
            return "cpu"
        if max(_coord_range(forest)[1], d, forest.nnz) > 4094:
            return "cpu"
        stage = _explain_eif_deep_stage(_row_kind(dtype), d, forest.nnz)
        return "deep" if stage > 0 else "cpu"
    if not _deep_fits(forest, d):
        return "cpu"
    return "deep" if _explain_deep_stage(_row_kind(dtype), d) > 0 else "cpu"


# Narrowest hyperplane (coordinates a node) that extended_explain_route sends
# to the dense kernel when nnz < d. Measured at d = 32, the widest rows the
# kernel takes: the smallest of nnz 2, 6 and 16 at which it beats the strict
# kernel, and it does at all three (profiles/explain_eif_dense.md).
EIF_EXPLAIN_DENSE_MIN_NNZ = 2


def _eif_coords_ascending(forest) -> bool:
    """True when every internal node of an extended forest carries exactly
    forest.nnz coordinates in strictly ascending order (so they are distinct,
    and a dot over dense columns adds its terms in the oracle's order);
    cached on the forest like _coord_range, dropped by invalidate_derived().
    Forests built here always do; foreign files may not."""
    ok = getattr(forest, "_coords_ascending", None)
    if ok is None:
        internal = forest.feature >= 0
        ok = True
        if internal.any():
            idx = forest.hyper_idx[internal]
            ok = bool((forest.feature[internal] == forest.nnz).all()
                      and (idx[:, 1:] > idx[:, :-1]).all())
        forest._coords_ascending = ok
    return ok


def _explain_eif_dense_cfg(kind: str, d: int, max_nodes: int):
    """(D, rows per thread, trees per phase, block threads) the dense EIF
    explain kernel runs these rows with against node arrays this wide, zeros
    where it has no instantiation or a tree's stage does not fit in LDS; see
    _deep_stage."""
    from . import load_extension as _packing_extension

    return tuple(int(v) for v in _packing_extension().explain_eif_dense_cfg(
        kind, int(d), int(max_nodes)))


def extended_explain_route(forest, d: int, dtype) -> str:
    """Where ``explain_extended_forest`` attributes an extended forest:

    * ``"dense"`` (explain_extended_dense_kernel: the whole tree staged in
      LDS as dense weight and share rows, rows and accumulators in
      registers) for a forest inside the packed caps with ``d <= 32``,
      every internal node holding ``nnz`` strictly ascending coordinates
      below ``d``, ``nnz == d`` or ``nnz >= EIF_EXPLAIN_DENSE_MIN_NNZ``, and
      a tree's stage fitting in LDS (maxSamples 256 does at every such d);
    * ``"strict"`` (explain_extended_kernel, one thread a row from global
      memory) for every other forest inside the packed caps, and for all of
      them under ``IFA_EXPLAIN_EIF_DENSE=0``;
    * past the packed caps, ``large_explain_route``'s ``"deep"`` or
      ``"cpu"``.

    With ``nnz < d`` the dense kernel multiplies unselected cells by a zero
    weight, so ``explain_extended_forest`` sends a batch there only when all
    of its cells are finite; the strict kernel takes the others. All routes
    return the same bits."""
    if not _packed_fits(forest, d):
        return large_explain_route(forest, d, dtype)
    if os.environ.get("IFA_EXPLAIN_EIF_DENSE", "1") == "0" or d > 32:
        return "strict"
    nnz = forest.nnz
    if nnz != d and nnz < EIF_EXPLAIN_DENSE_MIN_NNZ:
        return "strict"
    cmin, cmax = _coord_range(forest)
    if cmin < 0 or cmax >= d or not _eif_coords_ascending(forest):
        return "strict"
    cfg = _explain_eif_dense_cfg(_row_kind(dtype), d, forest.feature.shape[1])
    return "dense" if cfg[0] > 0 else "strict"


def _explain_on_cpu(fn, forest, X: torch.Tensor, finalize: bool, why: str):
    """Forests past the packed-record caps that the deep explain route does
    not take either: CPU oracle, result moved to X's device (a correctness
    path)."""
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
    # wide arrays (2n - 1 columns past the 15-bit ids): the cached maximum
    fmax = (_feature_max(forest) if forest.feature.shape[1] > 32767
            else int(forest.feature.max(initial=-1)))
    if fmax >= d:
        raise ValueError(
            f"the forest splits on feature {fmax} but rows have {d} columns")
    if not _packed_fits(forest, d):
        kind = _row_kind(X.dtype)
        if large_explain_route(forest, d, kind) == "deep":
            stage = _explain_deep_stage(kind, d)
            records, lds_levels, extra = _device_forest(
                model, X.device, v4_key=("explain_deep", d, stage, kind))
            return load_extension().explain_forest_deep(
                _rows_in_place(X), records, lds_levels, forest.num_trees,
                extra["height"], stage, finalize)
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
    (inside the packed caps the dense register-resident kernel or the
    strict-order one, see extended_explain_route; past them
    explain_extended_deep, see large_explain_route)."""
    from ..core import cpu_engine

    forest = model.forest
    d = int(X.shape[1])
    _check_explain_input(X)
    cmin, cmax = _coord_range(forest)
    if cmax >= d:
        raise ValueError(
            f"the forest splits on feature {cmax} but rows have {d} columns")
    if not _packed_fits(forest, d):
        kind = _row_kind(X.dtype)
        if cmin >= 0 and large_explain_route(forest, d, kind) == "deep":
            stage = _explain_eif_deep_stage(kind, d, forest.nnz)
            nodes, lds_levels, extra = _device_forest(
                model, X.device, v4_key=("explain_eif_deep", stage))
            return load_extension().explain_extended_deep(
                _rows_in_place(X), nodes, extra["payload"], lds_levels,
                forest.num_trees, extra["height"], stage, finalize)
        return _explain_on_cpu(
            cpu_engine.feature_contributions_extended, forest, X, finalize,
            "forest exceeds the packed node format (15-bit node ids, "
            "12-bit hyperplane widths)")
    ext = load_extension()
    # a zero weight times a non-finite cell is NaN where the oracle never
    # reads that cell: nnz < d goes dense with finite batches only (the
    # guard of score_extended_forest); nnz == d has no zero column
    if (extended_explain_route(forest, d, X.dtype) == "dense"
            and (forest.nnz == d or bool(torch.isfinite(X).all().item()))):
        D = _explain_eif_dense_cfg(_row_kind(X.dtype), d,
                                   forest.feature.shape[1])[0]
        nodes, ncount, extra = _device_forest(
            model, X.device, v4_key=("eif_explain_dense", D))
        return ext.explain_extended_dense(
            _rows_in_place(X), nodes, extra["rows"], ncount, extra["icount"],
            extra["height"], finalize)
    aos, ncount, extra = _device_forest(model, X.device, v4_key="eif_explain")
    return ext.explain_extended_forest(
        _rows_in_place(X), aos, extra["hidx"], extra["hw"], extra["dl"],
        extra["dr"], finalize)


# ---------------------------------------------------------------------------
# exact TreeSHAP, standard forests (docs/DESIGN.md §9)
# ---------------------------------------------------------------------------


def large_shap_route(forest, d: int, dtype) -> str:
    """Where ``shap_forest`` computes TreeSHAP for a forest past the packed
    15-bit node ids: ``"deep"`` (shap_forest_deep_kernel: a group of lanes a
    row, one path feature a lane, the leaf stream from L2) or ``"cpu"`` (the
    oracle, with a logged warning). ``IFA_SHAP_DEEP=0`` keeps the CPU path;
    so do extended forests, node arrays that fit the packed formats' 32767
    (a cap on feature ids alone sent them here), forests past
    ``DEEP_MAX_NODES`` nodes a tree or 4094 features, and a path that merges
    more than ``cpu_engine.SHAP_DEEP_MAX_PATH_FEATURES`` features. The kernel
    keys rows of any width, so ``dtype`` does not move the answer."""
    from ..core import cpu_engine

    _row_kind(dtype)
    if os.environ.get("IFA_SHAP_DEEP", "1") == "0":
        return "cpu"
    if forest.feature.shape[1] <= 32767 or not _deep_fits(forest, d):
        return "cpu"
    max_m = cpu_engine.shap_tables(forest)["max_m"]
    return ("deep" if max_m <= cpu_engine.SHAP_DEEP_MAX_PATH_FEATURES
            else "cpu")


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
    # wide arrays (2n - 1 columns past the 15-bit ids): the cached maximum
    fmax = (_feature_max(forest) if forest.feature.shape[1] > 32767
            else int(forest.feature.max(initial=-1)))
    if fmax >= d:
        raise ValueError(
            f"the forest splits on feature {fmax} but rows have {d} columns")
    if not _packed_fits(forest, d):
        kind = _row_kind(X.dtype)
        if large_shap_route(forest, d, kind) != "deep":
            return _shap_on_cpu(
                forest, X, finalize,
                "forest exceeds the packed node format (15-bit node ids, "
                "12-bit feature ids) and the deep route's caps "
                f"({cpu_engine.SHAP_DEEP_MAX_PATH_FEATURES} features on a "
                "path)")
        max_m = cpu_engine.shap_tables(forest)["max_m"]
        ext = load_extension()
        if (os.environ.get("IFA_SHAP_DEEP_SPLIT") == "row"
                and max_m <= cpu_engine.SHAP_MAX_PATH_FEATURES):
            # A/B only: one row per thread, the table read from global memory
            table, tree_off, extra = _device_forest(
                model, X.device, v4_key=("shap", d, kind))
            return ext.shap_forest(
                _rows_in_place(X), table, extra["tree_off_host"], tree_off,
                extra["wtab"], finalize)
        table, tree_off, extra = _device_forest(
            model, X.device, v4_key=("shap_deep", d, kind))
        return ext.shap_forest_deep(
            _rows_in_place(X), table, extra["tree_off_host"], tree_off,
            extra["wtab"], max_m, finalize)
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
