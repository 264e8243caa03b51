// MI355X (gfx950, CDNA4) Isolation Forest kernels.
//
// Hand-written HIP implementations of the reference's JVM hot loops
// (design rationale and measured limits in
// docs/DESIGN.md):
//  * build_forest_kernel          — K1 (min/max scan + constant-feature
//    retry), K2 (stable row partition), K11 (per-node feature Fisher-Yates):
//    one 64-lane wavefront per tree, row-index permutation in LDS, ballot/
//    popcount stable partition, shfl-xor min/max reductions; emits per-node
//    depths for the scoring pack.
//  * build_extended_forest_kernel — K3-K5 (EIF Gaussian hyperplane draw,
//    L2 normalize, per-coordinate min/max + offset, dot-product partition).
//  * build_forest_large_kernel /
//    build_extended_forest_large_kernel — the same two builds for bags of
//    more than 16384 rows: one multi-wave block per tree, 32-bit row ids in
//    a global ping-pong scratch, rows read in place from X (any admitted
//    dtype and layout), block-wide min/max and stable partition. Bitwise the
//    same forests.
//  * score_forest_v4              — K6/K8 standard scoring: integer-KEY
//    compares (rows staged in LDS as order-preserving u16/u32 keys,
//    per-node integer thresholds), depth folded into f32 leaf values,
//    self-looping leaves => FIXED-trip walks with zero bookkeeping,
//    2 rows x 4 staged trees = 8 chains/thread with batch-phased LDS reads
//    (staggered lgkmcnt waits). Bitwise == cpu_engine.path_lengths.
//  * score_forest_heap            — the same walk for bf16/fp16 rows over
//    4-byte heap records (16-bit threshold | slab offset, implicit
//    children; v4_heap_order_kernel): half the staging traffic, and 4 VALU
//    per visit instead of 7 (complemented slot index over trees staged
//    reversed in LDS: node address, key address, subtract, funnel shift).
//    8 trees per barrier phase, all walked together, where they fit next to
//    the tile; else 4. score_forest_v4 keeps f32 rows, d >= 128, deep
//    forests and the global fallbacks (bindings.cpp, pick_score_cfg).
//  * score_extended_dense_v2      — K7 fast path (hyperplanes densified to
//    D in {8,16,32,64} columns; f32 rows): rows resident in f32 REGISTERS
//    across the whole tree loop, one tree's nodes+values+weights staged in
//    LDS (conflict-breaking D/4+1 float4 row stride), exec-masked finished
//    lanes, offset=-inf self-looping leaves. Tolerance contract (4-partial
//    fma dot), routing in ops/gpu_engine.score_extended_forest.
//  * score_extended_dense_v3      — K7 fast path for bf16 rows, D up to
//    128: weights staged as RNE-rounded PACKED bf16 (half the LDS bytes
//    of v2 — its measured bound), rows as packed-bf16 register pairs,
//    dot on v_dot2c_f32_bf16. Contract: PARITY.md "Numeric contracts".
//  * score_extended_dense_nonfinite_rows — runs after dense v2/v3: rows
//    with an inf/NaN cell are rescored in strict j-order (bitwise), since
//    overflowing partial sums make their branch depend on the dot order.
//  * score_extended_sparse_v2     — K7 small-nnz path (templated NNZ<=5):
//    same fixed-trip structure, strict oracle j-order dot (bitwise).
//    extensionLevel-0 forests do NOT use it: they are packed onto
//    score_forest_v4 via exact key thresholds + mirrored subtrees
//    (ops/gpu_engine._eif0_packed_v4 — bitwise, zero per-visit overhead).
//  * score_extended_forest_kernel — K7 general strict-order fallback
//    (wide d / ragged hyperplane widths).
//  * score_forest_wide /
//    score_extended_wide          — full-width int4 node records for
//    forests past the packed 12-bit-feature/15-bit-node caps (foreign or
//    CPU-built deep models); global-memory walks, correctness path.
//  * bag_gather_kernel            — K9/K10 device side: gather sampled rows
//    into per-tree bags (indices drawn host-side by the same Philox).
//
// PRECISION CONTRACT: see core/cpu_engine.py. All randomness: philox.h;
// EIF gaussians: det_math.h. Wavefront size is 64 (CDNA4) and is hard-coded.
// This TU is torch-free: tools/native/ifa_score.cpp links it directly.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "det_math.h"
#include "philox.h"
#include "row_dtype.h"

#define WAVE 64
#define LANE_MASK_LT(lane) ((1ull << (lane)) - 1ull)

namespace ifa {

// ---------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------

__device__ __forceinline__ float wave_reduce_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, WAVE));
  return v;
}

__device__ __forceinline__ float wave_reduce_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
  return v;
}

// split point: float64 draw rounded to float32, bumped off the left edge
// (cpu_engine._split_value32)
__device__ __forceinline__ float split_value32(float fmin, float fmax, double u) {
  double s64 = (double)fmin + u * ((double)fmax - (double)fmin);
  float s32 = (float)s64;
  if (!(fmin < s32)) s32 = nextafterf(fmin, __builtin_inff());
  return s32;
}

struct SegEntry {
  uint16_t start, end;
  int16_t height;
  int16_t patch;  // node whose `right` points at the node this entry emits
};

// ---------------------------------------------------------------------------
// bag gather: bags[T][n][d] (f32) <- X[N][d] (f32, bf16 or fp16) at idx[T][n]
//
// Every kernel that reads X takes its two element strides: X[r][c] sits at
// X[r * rs + c * cs] (64-bit offsets). The bindings admit pitched row-major
// (cs == 1, rs >= d) and feature-major (rs == 1, cs >= N) sources; outputs
// and LDS tiles do not depend on the source layout.
// ---------------------------------------------------------------------------

// 16-bit rows come in two formats. uint16_t as the element/key type means
// bf16 bits; f16_t is the DISTINCT type for IEEE fp16 bits (same size and
// codegen as uint16_t, so every bf16 instantiation has an fp16 sibling that
// differs only in the helpers below).
enum class f16_t : uint16_t {};

// fp16 -> f32, exact for every input (subnormals included: v_cvt_f32_f16
// honours fp16 denormals, and every fp16 subnormal is a normal f32)
__device__ __forceinline__ float f16_bits_to_f32(uint16_t b) {
  union { uint16_t u; _Float16 h; } cv;
  cv.u = b;
  return (float)cv.h;
}

template <typename XT>
__device__ __forceinline__ float load_feat(const XT* X, int64_t off);

template <>
__device__ __forceinline__ float load_feat<float>(const float* X, int64_t off) {
  return X[off];
}
template <>
__device__ __forceinline__ float load_feat<uint16_t>(const uint16_t* X, int64_t off) {
  union { uint32_t u; float f; } cv;
  cv.u = ((uint32_t)X[off]) << 16;  // bf16 -> f32 (exact)
  return cv.f;
}
template <>
__device__ __forceinline__ float load_feat<f16_t>(const f16_t* X, int64_t off) {
  return f16_bits_to_f32((uint16_t)X[off]);
}

template <typename XT>
__global__ void bag_gather_kernel(const XT* __restrict__ X,
                                  const int64_t* __restrict__ bag_idx,
                                  float* __restrict__ bags, int64_t T, int64_t n,
                                  int64_t d, int64_t rs, int64_t cs) {
  int64_t total = T * n * d;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
       g += (int64_t)gridDim.x * blockDim.x) {
    int64_t j = g % d;
    int64_t ts = g / d;  // t*n + s
    int64_t row = bag_idx[ts];
    bags[g] = load_feat<XT>(X, row * rs + j * cs);
  }
}

// ---------------------------------------------------------------------------
// standard build: one wavefront per tree
// ---------------------------------------------------------------------------

extern __shared__ __attribute__((aligned(16))) char smem[];

__global__ void __launch_bounds__(WAVE) build_forest_kernel(
    const float* __restrict__ bags,        // [T][n][d]
    const int32_t* __restrict__ feat_sub,  // [T][k] sorted global feature ids
    int32_t* __restrict__ out_feat,        // [T][max_nodes]
    float* __restrict__ out_value,         // [T][max_nodes]
    int32_t* __restrict__ out_right,       // [T][max_nodes]
    int32_t* __restrict__ out_count,       // [T][max_nodes] (leaf counts; -1)
    int32_t* __restrict__ out_ncount,      // [T]
    int32_t* __restrict__ out_depth,       // [T][max_nodes]
    const float* __restrict__ leaf_lut,    // [n+1]: c(m) float32
    uint64_t seed, int32_t tree_id_offset, int32_t n, int32_t d, int32_t k,
    int32_t max_nodes, int32_t height_limit) {
  const int t = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t gtree = (uint32_t)(t + tree_id_offset);

  uint16_t* idx = (uint16_t*)smem;               // [n]
  uint16_t* tmp = idx + n;                       // [n]
  uint16_t* avail = tmp + n;                     // [k]
  SegEntry* stack = (SegEntry*)(((uintptr_t)(avail + k) + 15) & ~15ull);

  const float* bag = bags + (int64_t)t * n * d;
  int32_t* feat = out_feat + (int64_t)t * max_nodes;
  float* value = out_value + (int64_t)t * max_nodes;
  int32_t* right = out_right + (int64_t)t * max_nodes;
  int32_t* count = out_count + (int64_t)t * max_nodes;
  int32_t* depth = out_depth + (int64_t)t * max_nodes;
  const int32_t* features = feat_sub + (int64_t)t * k;

  for (int i = lane; i < n; i += WAVE) idx[i] = (uint16_t)i;
  if (lane == 0) stack[0] = SegEntry{0, (uint16_t)n, 0, -1};
  __syncthreads();

  int sp = 1;
  int next_id = 0;
  while (sp > 0) {
    SegEntry e = stack[--sp];
    const int node = next_id++;
    if (lane == 0) {
      if (e.patch >= 0) right[e.patch] = node;
      depth[node] = e.height;
    }
    const int start = e.start, end = e.end, m = end - start;

    if (m <= 1 || e.height >= height_limit) {
      if (lane == 0) {
        feat[node] = -1;
        value[node] = leaf_lut[m];
        count[node] = m;
      }
      continue;
    }

    // ---- feature selection with constant-feature retry (K1 + K11) ----
    for (int j = lane; j < k; j += WAVE) avail[j] = (uint16_t)features[j];
    __syncthreads();
    int found = -1;
    float fmin = 0.f, fmax = 0.f;
    for (int j = 0; j < k; ++j) {
      uint32_t r = rng_below(seed, P_FEATSEL, gtree, (uint32_t)node,
                             (uint32_t)(k - j), (uint32_t)j);
      int tsel = j + (int)r;
      if (lane == 0) {
        uint16_t a = avail[j];
        avail[j] = avail[tsel];
        avail[tsel] = a;
      }
      __syncthreads();
      const int f = avail[j];
      float lo = __builtin_inff(), hi = -__builtin_inff();
      for (int i = start + lane; i < end; i += WAVE) {
        float v = bag[(int64_t)idx[i] * d + f];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
      }
      lo = wave_reduce_min(lo);
      hi = wave_reduce_max(hi);
      if (lo < hi) {
        found = f;
        fmin = lo;
        fmax = hi;
        break;
      }
    }
    if (found < 0) {
      if (lane == 0) {
        feat[node] = -1;
        value[node] = leaf_lut[m];
        count[node] = m;
      }
      continue;
    }

    const double u = rng_uniform(seed, P_SPLIT, gtree, (uint32_t)node);
    const float s32 = split_value32(fmin, fmax, u);

    // ---- stable partition via ballot/popcount (K2) ----
    int cntL = 0;
    for (int base = start; base < end; base += WAVE) {
      const int i = base + lane;
      const bool valid = i < end;
      float v = valid ? bag[(int64_t)idx[i] * d + found] : 0.f;
      const bool p = valid && (v < s32);
      cntL += __popcll(__ballot(p));
    }
    int runL = 0, runR = 0;
    for (int base = start; base < end; base += WAVE) {
      const int i = base + lane;
      const bool valid = i < end;
      uint16_t my = valid ? idx[i] : (uint16_t)0;
      float v = valid ? bag[(int64_t)my * d + found] : 0.f;
      const bool p = valid && (v < s32);
      const uint64_t maskL = __ballot(p);
      const uint64_t maskR = __ballot(valid && !p);
      if (p)
        tmp[start + runL + __popcll(maskL & LANE_MASK_LT(lane))] = my;
      else if (valid)
        tmp[start + cntL + runR + __popcll(maskR & LANE_MASK_LT(lane))] = my;
      runL += __popcll(maskL);
      runR += __popcll(maskR);
    }
    __syncthreads();
    for (int i = start + lane; i < end; i += WAVE) idx[i] = tmp[i];
    __syncthreads();

    if (lane == 0) {
      feat[node] = found;
      value[node] = s32;
      count[node] = -1;
      // pre-order: push right, then left (left pops first = node+1)
      stack[sp] = SegEntry{(uint16_t)(start + cntL), (uint16_t)end,
                           (int16_t)(e.height + 1), (int16_t)node};
      stack[sp + 1] = SegEntry{(uint16_t)start, (uint16_t)(start + cntL),
                               (int16_t)(e.height + 1), (int16_t)-1};
    }
    __syncthreads();
    sp += 2;
  }
  if (lane == 0) out_ncount[t] = next_id;
}

// ---------------------------------------------------------------------------
// extended build: one wavefront per tree
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(WAVE) build_extended_forest_kernel(
    const float* __restrict__ bags, const int32_t* __restrict__ feat_sub,
    int32_t* __restrict__ out_feat, float* __restrict__ out_value,
    int32_t* __restrict__ out_right, int32_t* __restrict__ out_count,
    int32_t* __restrict__ out_ncount,
    int32_t* __restrict__ out_hidx,    // [T][max_nodes][nnz]
    float* __restrict__ out_hw,        // [T][max_nodes][nnz]
    double* __restrict__ out_off64,    // [T][max_nodes]
    int32_t* __restrict__ out_depth,   // [T][max_nodes]
    const float* __restrict__ leaf_lut, uint64_t seed, int32_t tree_id_offset,
    int32_t n, int32_t d, int32_t k, int32_t nnz, int32_t max_nodes,
    int32_t height_limit) {
  const int t = blockIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const uint32_t gtree = (uint32_t)(t + tree_id_offset);

  uint16_t* idx = (uint16_t*)smem;   // [n]
  uint16_t* tmp = idx + n;           // [n]
  uint16_t* avail = tmp + n;         // [k]
  int32_t* coords =                  // [nnz]
      (int32_t*)(((uintptr_t)(avail + k) + 15) & ~15ull);
  float* wf = (float*)(coords + nnz);  // [nnz]
  SegEntry* stack = (SegEntry*)(((uintptr_t)(wf + nnz) + 15) & ~15ull);

  const float* bag = bags + (int64_t)t * n * d;
  int32_t* feat = out_feat + (int64_t)t * max_nodes;
  float* value = out_value + (int64_t)t * max_nodes;
  int32_t* right = out_right + (int64_t)t * max_nodes;
  int32_t* count = out_count + (int64_t)t * max_nodes;
  int32_t* hidx = out_hidx + (int64_t)t * max_nodes * nnz;
  float* hw = out_hw + (int64_t)t * max_nodes * nnz;
  double* off64p = out_off64 + (int64_t)t * max_nodes;
  int32_t* depth = out_depth + (int64_t)t * max_nodes;
  const int32_t* features = feat_sub + (int64_t)t * k;

  for (int i = lane; i < n; i += WAVE) idx[i] = (uint16_t)i;
  if (lane == 0) stack[0] = SegEntry{0, (uint16_t)n, 0, -1};
  __syncthreads();

  int sp = 1;
  int next_id = 0;
  while (sp > 0) {
    SegEntry e = stack[--sp];
    const int node = next_id++;
    if (lane == 0) {
      if (e.patch >= 0) right[e.patch] = node;
      depth[node] = e.height;
    }
    const int start = e.start, end = e.end, m = end - start;

    if (m <= 1 || e.height >= height_limit) {
      if (lane == 0) {
        feat[node] = -1;
        value[node] = leaf_lut[m];
        count[node] = m;
      }
      continue;
    }

    // ---- coordinate subset: Fisher-Yates over the tree's subspace ----
    for (int j = lane; j < k; j += WAVE) avail[j] = (uint16_t)features[j];
    __syncthreads();
    for (int j = 0; j < nnz; ++j) {
      uint32_t r = rng_below(seed, P_EIF_COORD, gtree, (uint32_t)node,
                             (uint32_t)(k - j), (uint32_t)j);
      if (lane == 0) {
        int tsel = j + (int)r;
        uint16_t a = avail[j];
        avail[j] = avail[tsel];
        avail[tsel] = a;
      }
      __syncthreads();
    }
    // sort the first nnz ascending (lane 0, insertion sort; nnz <= ~128)
    if (lane == 0) {
      for (int a = 1; a < nnz; ++a) {
        uint16_t key = avail[a];
        int b = a - 1;
        while (b >= 0 && avail[b] > key) {
          avail[b + 1] = avail[b];
          --b;
        }
        avail[b + 1] = key;
      }
      for (int j = 0; j < nnz; ++j) coords[j] = (int32_t)avail[j];
    }
    __syncthreads();

    // ---- Gaussian weights per sorted slot (det Box-Muller), parallel ----
    const uint32_t base = (uint32_t)node * 4096u;
    for (int j = lane; j < nnz; j += WAVE) {
      double u1, u2;
      rng_uniform2(seed, P_EIF_NORMAL, gtree, base + (uint32_t)j, &u1, &u2);
      wf[j] = (float)det_gaussian(u1, u2);
    }
    __syncthreads();
    // sequential float32 norm (order == CPU oracle)
    float acc = 0.f;
    for (int j = 0; j < nnz; ++j) acc = __fadd_rn(acc, __fmul_rn(wf[j], wf[j]));
    if (acc <= 0.f) {  // theoretical zero-norm leaf
      if (lane == 0) {
        feat[node] = -1;
        value[node] = leaf_lut[m];
        count[node] = m;
      }
      continue;
    }
    // sqrt/divide through double: __fsqrt_rn/__fdiv_rn are NOT correctly
    // rounded on this toolchain (1 ulp), numpy's f32 ops are; f64-then-round
    // is provably identical to correctly-rounded f32 (53 >= 2*24+2).
    const float norm = (float)sqrt((double)acc);
    for (int j = lane; j < nnz; j += WAVE)
      wf[j] = (float)((double)wf[j] / (double)norm);
    __syncthreads();

    // ---- intercepts per sorted coordinate + offset (float64) ----
    double off64 = 0.0;
    for (int j = 0; j < nnz; ++j) {
      const int c = coords[j];
      float lo = __builtin_inff(), hi = -__builtin_inff();
      for (int i = start + lane; i < end; i += WAVE) {
        float v = bag[(int64_t)idx[i] * d + c];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
      }
      lo = wave_reduce_min(lo);
      hi = wave_reduce_max(hi);
      const double u =
          rng_uniform(seed, P_EIF_INTERCEPT, gtree, base + (uint32_t)j);
      const double intercept = (double)lo + u * ((double)hi - (double)lo);
      off64 += (double)wf[j] * intercept;
    }
    const float off32 = (float)off64;

    // ---- partition by hyperplane dot (no retry; empty sides allowed) ----
    int cntL = 0;
    for (int basei = start; basei < end; basei += WAVE) {
      const int i = basei + lane;
      const bool valid = i < end;
      float dot = 0.f;
      if (valid) {
        const float* rowp = bag + (int64_t)idx[i] * d;
        for (int j = 0; j < nnz; ++j)
          dot = __fadd_rn(dot, __fmul_rn(wf[j], rowp[coords[j]]));
      }
      cntL += __popcll(__ballot(valid && (dot < off32)));
    }
    int runL = 0, runR = 0;
    for (int basei = start; basei < end; basei += WAVE) {
      const int i = basei + lane;
      const bool valid = i < end;
      uint16_t my = valid ? idx[i] : (uint16_t)0;
      float dot = 0.f;
      if (valid) {
        const float* rowp = bag + (int64_t)my * d;
        for (int j = 0; j < nnz; ++j)
          dot = __fadd_rn(dot, __fmul_rn(wf[j], rowp[coords[j]]));
      }
      const bool p = valid && (dot < off32);
      const uint64_t maskL = __ballot(p);
      const uint64_t maskR = __ballot(valid && !p);
      if (p)
        tmp[start + runL + __popcll(maskL & LANE_MASK_LT(lane))] = my;
      else if (valid)
        tmp[start + cntL + runR + __popcll(maskR & LANE_MASK_LT(lane))] = my;
      runL += __popcll(maskL);
      runR += __popcll(maskR);
    }
    __syncthreads();
    for (int i = start + lane; i < end; i += WAVE) idx[i] = tmp[i];
    __syncthreads();

    if (lane == 0) {
      feat[node] = nnz;
      value[node] = off32;
      off64p[node] = off64;
      count[node] = -1;
      for (int j = 0; j < nnz; ++j) {
        hidx[(int64_t)node * nnz + j] = coords[j];
        hw[(int64_t)node * nnz + j] = wf[j];
      }
      stack[sp] = SegEntry{(uint16_t)(start + cntL), (uint16_t)end,
                           (int16_t)(e.height + 1), (int16_t)node};
      stack[sp + 1] = SegEntry{(uint16_t)start, (uint16_t)(start + cntL),
                               (int16_t)(e.height + 1), (int16_t)-1};
    }
    __syncthreads();
    sp += 2;
  }
  if (lane == 0) out_ncount[t] = next_id;
}

// ---------------------------------------------------------------------------
// large-bag build (n > 16384): one block of several waves per tree
//
// The two kernels above keep a bag's row positions in LDS as 16-bit values
// and read a pre-gathered f32 copy of every bag; neither survives big bags.
// Their siblings here keep the working set in global memory:
//   * scratch[t][2][n] (uint32) holds the tree's row permutation. It stores
//     the GLOBAL ROW IDS of X (bag_idx[t][slot], narrowed to 32 bits; the
//     bindings check N <= 2^32), not bag slots, so a cell is one dependent
//     load away (scratch -> X) instead of two. Rows are read in place from X
//     through load_feat<XT> and the two element strides.
//   * the two halves ping-pong: a segment at height h lives in half h & 1,
//     its partition writes the children into half (h + 1) & 1. Pending stack
//     entries cover ranges disjoint from the current one, so nothing live is
//     overwritten and no copy-back pass exists.
//   * stack entries, node ids and segment bounds are 32-bit.
// The pre-order DFS stays serial per tree (Philox draws are keyed by the
// pre-order node id); the block parallelises inside a node. Min/max: wave
// shuffle, then per-wave partials combined through LDS (fminf/fmaxf give the
// same bits in any order). Partition: every wave owns a contiguous slice of
// the segment, counts its left-goers, an exclusive prefix over the waves'
// counts gives each slice its left and right base, then the slice is placed
// with the ballot/popcount ranks of the one-wave kernels. A stable partition
// has one result, so the forest is bitwise the one-wave kernels' (and
// cpu_engine's). Segments of at most one wave skip the LDS combine: every
// wave computes the whole segment itself and wave 0 alone stores.
// Every branch around a barrier is block-uniform (m, height, found, acc).
// ---------------------------------------------------------------------------

#define BL_MAX_THREADS 512
#define BL_MAX_WAVES (BL_MAX_THREADS / WAVE)
#define BL_G 8  // coordinates per min/max pass of the extended build

struct SegEntryL {
  uint32_t start, end;
  int32_t height;
  int32_t patch;  // node whose `right` points at the node this entry emits
};

// Per-wave partials, double-buffered: each block-wide combine writes half
// `pp`, meets at ONE barrier, reads, and flips pp. A half is rewritten two
// combines later at the earliest, i.e. after a barrier every thread reached
// only once it had finished reading it.
struct BlockPartials {
  float lo[2][BL_MAX_WAVES][BL_G];
  float hi[2][BL_MAX_WAVES][BL_G];
  uint32_t cnt[2][BL_MAX_WAVES];
};

// min/max of G columns (element offsets coff[g] = column * cs) over the rows
// src[start, end), block-wide; every thread returns all G results
template <typename XT, int G>
__device__ __forceinline__ void seg_minmax(
    const XT* __restrict__ X, int64_t rs, const int64_t (&coff)[G],
    const uint32_t* __restrict__ src, uint32_t start, uint32_t end,
    BlockPartials& bp, int& pp, float (&lo)[G], float (&hi)[G]) {
  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const uint32_t nw = blockDim.x / WAVE;
  const bool small = end - start <= WAVE;  // block-uniform
#pragma unroll
  for (int g = 0; g < G; ++g) {
    lo[g] = __builtin_inff();
    hi[g] = -__builtin_inff();
  }
  const uint32_t step = small ? WAVE : blockDim.x;
#pragma unroll 4
  for (uint32_t i = start + (small ? lane : tid); i < end; i += step) {
    const int64_t ro = (int64_t)src[i] * rs;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float v = load_feat<XT>(X, ro + coff[g]);
      lo[g] = fminf(lo[g], v);
      hi[g] = fmaxf(hi[g], v);
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    lo[g] = wave_reduce_min(lo[g]);
    hi[g] = wave_reduce_max(hi[g]);
  }
  if (!small) {
    if (lane == 0) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        bp.lo[pp][wave][g] = lo[g];
        bp.hi[pp][wave][g] = hi[g];
      }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float a = bp.lo[pp][0][g], b = bp.hi[pp][0][g];
      for (uint32_t w = 1; w < nw; ++w) {
        a = fminf(a, bp.lo[pp][w][g]);
        b = fmaxf(b, bp.hi[pp][w][g]);
      }
      lo[g] = a;
      hi[g] = b;
    }
    pp ^= 1;
  }
}

// Stable partition of the rows src[start, end) by pred(row) (true = left)
// into dst[start, end); returns the left count to every thread. The caller
// puts a barrier after it before anyone reads dst.
template <typename Pred>
__device__ __forceinline__ uint32_t seg_partition(
    const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
    uint32_t start, uint32_t end, BlockPartials& bp, int& pp, Pred pred) {
  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const uint32_t nw = blockDim.x / WAVE;
  const uint32_t m = end - start;
  if (m <= WAVE) {  // block-uniform; no barrier inside
    const uint32_t i = start + lane;
    const bool valid = i < end;
    const uint32_t my = valid ? src[i] : 0u;
    const bool p = valid && pred(my);
    const uint64_t maskL = __ballot(p);
    const uint64_t maskR = __ballot(valid && !p);
    const uint32_t cntL = (uint32_t)__popcll(maskL);
    if (wave == 0) {
      if (p)
        dst[start + __popcll(maskL & LANE_MASK_LT(lane))] = my;
      else if (valid)
        dst[start + cntL + __popcll(maskR & LANE_MASK_LT(lane))] = my;
    }
    return cntL;
  }
  // contiguous slice per wave, a whole number of 64-row steps
  const uint32_t chunk = ((m + nw - 1) / nw + (WAVE - 1)) & ~(uint32_t)(WAVE - 1);
  const uint32_t wo = min(wave * chunk, m);
  const uint32_t ws = start + wo;
  const uint32_t we = start + min(wo + chunk, m);
  uint32_t c = 0;
#pragma unroll 4
  for (uint32_t i = ws + lane; i < we; i += WAVE) c += pred(src[i]) ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, WAVE);
  if (lane == 0) bp.cnt[pp][wave] = c;
  __syncthreads();
  uint32_t cntL = 0, leftBase = 0;
  for (uint32_t w = 0; w < nw; ++w) {
    const uint32_t v = bp.cnt[pp][w];
    if (w < wave) leftBase += v;
    cntL += v;
  }
  pp ^= 1;
  uint32_t posL = start + leftBase;
  uint32_t posR = start + cntL + (wo - leftBase);
  for (uint32_t base = ws; base < we; base += 4 * WAVE) {
    uint32_t my[4];
    bool valid[4], p[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t i = base + u * WAVE + lane;
      valid[u] = i < we;
      my[u] = valid[u] ? src[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) p[u] = valid[u] && pred(my[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t maskL = __ballot(p[u]);
      const uint64_t maskR = __ballot(valid[u] && !p[u]);
      if (p[u])
        dst[posL + __popcll(maskL & LANE_MASK_LT(lane))] = my[u];
      else if (valid[u])
        dst[posR + __popcll(maskR & LANE_MASK_LT(lane))] = my[u];
      posL += (uint32_t)__popcll(maskL);
      posR += (uint32_t)__popcll(maskR);
    }
  }
  return cntL;
}

template <typename XT>
__global__ void __launch_bounds__(BL_MAX_THREADS) build_forest_large_kernel(
    const XT* __restrict__ X, int64_t rs, int64_t cs,
    const int64_t* __restrict__ bag_idx,   // [T][n] rows of X
    uint32_t* __restrict__ scratch,        // [T][2][n]
    const int32_t* __restrict__ feat_sub,  // [T][k] sorted global feature ids
    int32_t* __restrict__ out_feat,        // [T][max_nodes]
    float* __restrict__ out_value,         // [T][max_nodes]
    int32_t* __restrict__ out_right,       // [T][max_nodes], pre-filled -1
    int32_t* __restrict__ out_count,       // [T][max_nodes] (leaf counts; -1)
    int32_t* __restrict__ out_ncount,      // [T]
    int32_t* __restrict__ out_depth,       // [T][max_nodes]
    const float* __restrict__ leaf_lut,    // [n+1]: c(m) float32
    uint64_t seed, int32_t tree_id_offset, int32_t n, int32_t k,
    int32_t max_nodes, int32_t height_limit) {
  __shared__ BlockPartials bp;
  const int t = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint32_t gtree = (uint32_t)(t + tree_id_offset);

  int32_t* avail = (int32_t*)smem;  // [k]
  SegEntryL* stack = (SegEntryL*)(((uintptr_t)(avail + k) + 15) & ~15ull);

  uint32_t* buf0 = scratch + (int64_t)t * 2 * n;
  uint32_t* buf1 = buf0 + n;
  const int64_t* bagp = bag_idx + (int64_t)t * n;
  int32_t* feat = out_feat + (int64_t)t * max_nodes;
  float* value = out_value + (int64_t)t * max_nodes;
  int32_t* right = out_right + (int64_t)t * max_nodes;
  int32_t* count = out_count + (int64_t)t * max_nodes;
  int32_t* depth = out_depth + (int64_t)t * max_nodes;
  const int32_t* features = feat_sub + (int64_t)t * k;

  for (uint32_t i = tid; i < (uint32_t)n; i += blockDim.x)
    buf0[i] = (uint32_t)bagp[i];
  if (tid == 0) stack[0] = SegEntryL{0u, (uint32_t)n, 0, -1};
  __syncthreads();

  int sp = 1, pp = 0;
  int32_t next_id = 0;
  while (sp > 0) {
    const SegEntryL e = stack[--sp];
    const int32_t node = next_id++;
    if (tid == 0) {
      if (e.patch >= 0) right[e.patch] = node;
      depth[node] = e.height;
    }
    const uint32_t start = e.start, end = e.end, m = end - start;

    if (m <= 1 || e.height >= height_limit) {
      if (tid == 0) {
        feat[node] = -1;
        value[node] = leaf_lut[m];
        count[node] = (int32_t)m;
      }
      continue;
    }
    const uint32_t* src = (e.height & 1) ? buf1 : buf0;
    uint32_t* dst = (e.height & 1) ? buf0 : buf1;

    // ---- feature selection with constant-feature retry (K1 + K11) ----
    for (uint32_t j = tid; j < (uint32_t)k; j += blockDim.x)
      avail[j] = features[j];
    __syncthreads();
    int found = -1;
    float fmin = 0.f, fmax = 0.f;
    for (int j = 0; j < k; ++j) {
      uint32_t r = rng_below(seed, P_FEATSEL, gtree, (uint32_t)node,
                             (uint32_t)(k - j), (uint32_t)j);
      int tsel = j + (int)r;
      if (tid == 0) {
        int32_t a = avail[j];
        avail[j] = avail[tsel];
        avail[tsel] = a;
      }
      __syncthreads();
      const int f = avail[j];
      const int64_t coff[1] = {(int64_t)f * cs};
      float lo[1], hi[1];
      seg_minmax<XT, 1>(X, rs, coff, src, start, end, bp, pp, lo, hi);
      if (lo[0] < hi[0]) {
        found = f;
        fmin = lo[0];
        fmax = hi[0];
        break;
      }
    }
    if (found < 0) {
      if (tid == 0) {
        feat[node] = -1;
        value[node] = leaf_lut[m];
        count[node] = (int32_t)m;
      }
      // the last avail[j] reads end here, before the next node refills it
      __syncthreads();
      continue;
    }

    const double u = rng_uniform(seed, P_SPLIT, gtree, (uint32_t)node);
    const float s32 = split_value32(fmin, fmax, u);

    // ---- stable partition (K2) ----
    const int64_t foff = (int64_t)found * cs;
    const uint32_t cntL = seg_partition(
        src, dst, start, end, bp, pp, [&](uint32_t row) {
          return load_feat<XT>(X, (int64_t)row * rs + foff) < s32;
        });

    if (tid == 0) {
      feat[node] = found;
      value[node] = s32;
      count[node] = -1;
      // pre-order: push right, then left (left pops first = node+1)
      stack[sp] = SegEntryL{start + cntL, end, e.height + 1, node};
      stack[sp + 1] = SegEntryL{start, start + cntL, e.height + 1, -1};
    }
    __syncthreads();  // dst and the stack, for every wave
    sp += 2;
  }
  if (tid == 0) out_ncount[t] = next_id;
}

template <typename XT>
__global__ void __launch_bounds__(BL_MAX_THREADS)
build_extended_forest_large_kernel(
    const XT* __restrict__ X, int64_t rs, int64_t cs,
    const int64_t* __restrict__ bag_idx, uint32_t* __restrict__ scratch,
    const int32_t* __restrict__ feat_sub, int32_t* __restrict__ out_feat,
    float* __restrict__ out_value, int32_t* __restrict__ out_right,
    int32_t* __restrict__ out_count, int32_t* __restrict__ out_ncount,
    int32_t* __restrict__ out_hidx,    // [T][max_nodes][nnz]
    float* __restrict__ out_hw,        // [T][max_nodes][nnz]
    double* __restrict__ out_off64,    // [T][max_nodes]
    int32_t* __restrict__ out_depth,   // [T][max_nodes]
    const float* __restrict__ leaf_lut, uint64_t seed, int32_t tree_id_offset,
    int32_t n, int32_t k, int32_t nnz, int32_t max_nodes,
    int32_t height_limit) {
  __shared__ BlockPartials bp;
  const int t = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  const uint32_t gtree = (uint32_t)(t + tree_id_offset);

  int64_t* coff = (int64_t*)smem;           // [nnz] coords[j] * cs
  int32_t* avail = (int32_t*)(coff + nnz);  // [k]
  int32_t* coords = avail + k;              // [nnz]
  float* wf = (float*)(coords + nnz);       // [nnz]
  SegEntryL* stack = (SegEntryL*)(((uintptr_t)(wf + nnz) + 15) & ~15ull);

  uint32_t* buf0 = scratch + (int64_t)t * 2 * n;
  uint32_t* buf1 = buf0 + n;
  const int64_t* bagp = bag_idx + (int64_t)t * n;
  int32_t* feat = out_feat + (int64_t)t * max_nodes;
  float* value = out_value + (int64_t)t * max_nodes;
  int32_t* right = out_right + (int64_t)t * max_nodes;
  int32_t* count = out_count + (int64_t)t * max_nodes;
  int32_t* hidx = out_hidx + (int64_t)t * max_nodes * nnz;
  float* hw = out_hw + (int64_t)t * max_nodes * nnz;
  double* off64p = out_off64 + (int64_t)t * max_nodes;
  int32_t* depth = out_depth + (int64_t)t * max_nodes;
  const int32_t* features = feat_sub + (int64_t)t * k;

  for (uint32_t i = tid; i < (uint32_t)n; i += blockDim.x)
    buf0[i] = (uint32_t)bagp[i];
  if (tid == 0) stack[0] = SegEntryL{0u, (uint32_t)n, 0, -1};
  __syncthreads();

  int sp = 1, pp = 0;
  int32_t next_id = 0;
  while (sp > 0) {
    const SegEntryL e = stack[--sp];
    const int32_t node = next_id++;
    if (tid == 0) {
      if (e.patch >= 0) right[e.patch] = node;
      depth[node] = e.height;
    }
    const uint32_t start = e.start, end = e.end, m = end - start;

    if (m <= 1 || e.height >= height_limit) {
      if (tid == 0) {
        feat[node] = -1;
        value[node] = leaf_lut[m];
        count[node] = (int32_t)m;
      }
      continue;
    }
    const uint32_t* src = (e.height & 1) ? buf1 : buf0;
    uint32_t* dst = (e.height & 1) ? buf0 : buf1;

    // ---- coordinate subset: Fisher-Yates over the tree's subspace ----
    for (uint32_t j = tid; j < (uint32_t)k; j += blockDim.x)
      avail[j] = features[j];
    __syncthreads();
    // thread 0 alone draws, swaps and sorts (insertion sort, ascending);
    // the others meet it at the barrier after the Gaussian draws
    if (tid == 0) {
      for (int j = 0; j < nnz; ++j) {
        uint32_t r = rng_below(seed, P_EIF_COORD, gtree, (uint32_t)node,
                               (uint32_t)(k - j), (uint32_t)j);
        int tsel = j + (int)r;
        int32_t a = avail[j];
        avail[j] = avail[tsel];
        avail[tsel] = a;
      }
      for (int a = 1; a < nnz; ++a) {
        int32_t key = avail[a];
        int b = a - 1;
        while (b >= 0 && avail[b] > key) {
          avail[b + 1] = avail[b];
          --b;
        }
        avail[b + 1] = key;
      }
      for (int j = 0; j < nnz; ++j) {
        coords[j] = avail[j];
        coff[j] = (int64_t)avail[j] * cs;
      }
    }

    // ---- Gaussian weights per sorted slot (det Box-Muller), parallel ----
    const uint32_t base = (uint32_t)node * 4096u;
    for (uint32_t j = tid; j < (uint32_t)nnz; j += blockDim.x) {
      double u1, u2;
      rng_uniform2(seed, P_EIF_NORMAL, gtree, base + j, &u1, &u2);
      wf[j] = (float)det_gaussian(u1, u2);
    }
    __syncthreads();
    // sequential float32 norm (order == CPU oracle)
    float acc = 0.f;
    for (int j = 0; j < nnz; ++j) acc = __fadd_rn(acc, __fmul_rn(wf[j], wf[j]));
    // every wave has summed the raw weights before any is normalised, and
    // before the next node's draws on the zero-norm path
    __syncthreads();
    if (acc <= 0.f) {  // theoretical zero-norm leaf
      if (tid == 0) {
        feat[node] = -1;
        value[node] = leaf_lut[m];
        count[node] = (int32_t)m;
      }
      continue;
    }
    // sqrt/divide through double, as build_extended_forest_kernel
    const float norm = (float)sqrt((double)acc);
    for (uint32_t j = tid; j < (uint32_t)nnz; j += blockDim.x)
      wf[j] = (float)((double)wf[j] / (double)norm);
    __syncthreads();

    // ---- intercepts per sorted coordinate + offset (float64, j order) ----
    // BL_G coordinates share one pass over the segment
    double off64 = 0.0;
    for (int j0 = 0; j0 < nnz; j0 += BL_G) {
      int64_t co[BL_G];
#pragma unroll
      for (int g = 0; g < BL_G; ++g) co[g] = coff[min(j0 + g, nnz - 1)];
      float lo[BL_G], hi[BL_G];
      seg_minmax<XT, BL_G>(X, rs, co, src, start, end, bp, pp, lo, hi);
#pragma unroll
      for (int g = 0; g < BL_G; ++g) {
        const int j = j0 + g;
        if (j < nnz) {
          const double u =
              rng_uniform(seed, P_EIF_INTERCEPT, gtree, base + (uint32_t)j);
          const double intercept =
              (double)lo[g] + u * ((double)hi[g] - (double)lo[g]);
          off64 += (double)wf[j] * intercept;
        }
      }
    }
    const float off32 = (float)off64;

    // ---- partition by hyperplane dot (no retry; empty sides allowed) ----
    const uint32_t cntL = seg_partition(
        src, dst, start, end, bp, pp, [&](uint32_t row) {
          const int64_t ro = (int64_t)row * rs;
          float dot = 0.f;
          for (int j = 0; j < nnz; ++j)
            dot = __fadd_rn(dot,
                            __fmul_rn(wf[j], load_feat<XT>(X, ro + coff[j])));
          return dot < off32;
        });

    for (uint32_t j = tid; j < (uint32_t)nnz; j += blockDim.x) {
      hidx[(int64_t)node * nnz + j] = coords[j];
      hw[(int64_t)node * nnz + j] = wf[j];
    }
    if (tid == 0) {
      feat[node] = nnz;
      value[node] = off32;
      off64p[node] = off64;
      count[node] = -1;
      stack[sp] = SegEntryL{start + cntL, end, e.height + 1, node};
      stack[sp + 1] = SegEntryL{start, start + cntL, e.height + 1, -1};
    }
    __syncthreads();  // dst, the stack, and the last coords/wf reads
    sp += 2;
  }
  if (tid == 0) out_ncount[t] = next_id;
}

// ---------------------------------------------------------------------------
// standard scoring kernel (K6/K8) — v4
//
// (16-bit rows that fit it take the 4-byte heap records of
// score_forest_heap, further down, made from the same packer output.)
//
// Node record is 8 bytes {uint32 w0, uint32 w1}, trees in LEVEL order
// (v4_level_order_kernel below re-lays the packers' pre-order output once
// per pack; left child = right_child - 1):
//   w0 = feature(12 bits) | right_child(15 bits) << 12
//   internal: w1 = integer KEY threshold (order-preserving transform of the
//             f32 split value; bf16 keys live in the HIGH 16 bits)
//   leaf:     feature = d (a sentinel column staged as all-ones), right =
//             OWN id (self-loop), w1 = f32 bits of (depth + c(numInstances))
//
// Rows are staged in LDS as order-preserving integer keys (u16 for bf16
// input, u32 for f32), feature-major, so each visit is: ds_read_b64 node,
// ds_read LDS key, one unsigned compare, one subtract-with-borrow
// (cur = right_child - (x < t)) — no float convert, no leaf branch, no
// depth counter. Both reads are laid out against LDS bank conflicts
// (profiles/score_layout.md). Leaves self-loop (sentinel key 0xFF..F
// compares false against every threshold), so the walk is a FIXED
// height_limit-trip loop
// with zero per-chain bookkeeping; the leaf value (depth folded in, as the
// reference's ONNX converter does: isolation_forest_converter.py:343-373)
// is read once after the loop. Each thread walks RPT rows x 4 trees = 4*RPT
// independent dependent-load chains. Bitwise-identical to
// cpu_engine.path_lengths (tree-order f32 accumulation).
// ---------------------------------------------------------------------------

__device__ __forceinline__ float cvt_feat(float v) { return v; }
__device__ __forceinline__ float cvt_feat(uint16_t v) {
  union { uint32_t u; float f; } cv;
  cv.u = ((uint32_t)v) << 16;
  return cv.f;
}
__device__ __forceinline__ float cvt_feat(f16_t v) {
  return f16_bits_to_f32((uint16_t)v);
}

__device__ __forceinline__ int pn_feat(int meta) { return meta & 0xFFF; }
__device__ __forceinline__ int pn_right(int meta) { return (meta >> 12) & 0x7FFF; }

// order-preserving key transforms (match gpu_engine._key16/_key32):
// +-0 collapse to the +0 key, NaN maps to the max key (so `x < t` is false:
// NaN routes right, same as the f32 compare in the oracle).
__device__ __forceinline__ uint32_t key16(uint32_t b) {
  const uint32_t m = b & 0x7FFFu;
  uint32_t k = (b & 0x8000u) ? (0x7FFFu - m) : (0x8000u + m);
  if (m == 0) k = 0x8000u;
  if (m > 0x7F80u) k = 0xFFFFu;
  return k;
}
// fp16 bits: same sign-magnitude fold, NaN is m > 0x7C00 (+inf -> 0xFC00)
__device__ __forceinline__ uint32_t key16_f16(uint32_t b) {
  const uint32_t m = b & 0x7FFFu;
  uint32_t k = (b & 0x8000u) ? (0x7FFFu - m) : (0x8000u + m);
  if (m == 0) k = 0x8000u;
  if (m > 0x7C00u) k = 0xFFFFu;
  return k;
}
__device__ __forceinline__ uint32_t key32(uint32_t b) {
  const uint32_t m = b & 0x7FFFFFFFu;
  uint32_t k = (b & 0x80000000u) ? (0x7FFFFFFFu - m) : (0x80000000u + m);
  if (m == 0) k = 0x80000000u;
  if (m > 0x7F800000u) k = 0xFFFFFFFFu;
  return k;
}

// KT = uint16_t (bf16 input), f16_t (fp16 input) or uint32_t (f32 input)
template <typename KT>
__device__ __forceinline__ KT key_of_bits(KT b);
template <>
__device__ __forceinline__ f16_t key_of_bits<f16_t>(f16_t b) {
  return (f16_t)(uint16_t)key16_f16((uint32_t)(uint16_t)b);
}
template <>
__device__ __forceinline__ uint16_t key_of_bits<uint16_t>(uint16_t b) {
  return (uint16_t)key16((uint32_t)b);
}
template <>
__device__ __forceinline__ uint32_t key_of_bits<uint32_t>(uint32_t b) {
  return key32(b);
}

// widen a stored key for the compare: bf16 keys sit in the high 16 bits with
// low bits saturated so the sentinel (0xFFFF) widens to 0xFFFFFFFF and
// compares false against every w1 (including leaf f32 payloads).
__device__ __forceinline__ uint32_t widen_key(uint16_t k) {
  return ((uint32_t)k << 16) | 0xFFFFu;
}
__device__ __forceinline__ uint32_t widen_key(f16_t k) {
  return widen_key((uint16_t)k);
}
__device__ __forceinline__ uint32_t widen_key(uint32_t k) { return k; }

// all-ones key: the leaf sentinel column (and the NaN key)
template <typename KT>
__device__ __forceinline__ KT key_sentinel() { return (KT)~(KT)0; }
template <>
__device__ __forceinline__ f16_t key_sentinel<f16_t>() { return (f16_t)0xFFFFu; }

// row stride in elements for the extended kernels: keep rows 16-B aligned
template <typename XT>
__device__ __host__ __forceinline__ int row_stride(int d) {
  const int pad = 16 / (int)sizeof(XT);  // 8 for bf16/fp16, 4 for f32
  return d + pad;
}


// ---------------------------------------------------------------------------
// v4 records, pre-order -> level order. The packers emit pre-order trees
// (left child at cur+1, link = right child). The walk reads them breadth-
// first: each level contiguous and left to right, the two children of a node
// adjacent, link = the RIGHT child's new index (left = link-1); leaves keep
// link = own new index. At walk iteration `it` every chain sits at depth
// `it` or rests at a shallower leaf, so the <= 32 nodes of levels 0..5 fall
// on distinct 8-byte bank pairs of a ds_read_b64 instead of being scattered
// over the whole pre-order array. One wave per tree; a level's nodes are
// numbered by a ballot prefix count. Records past ncount (dead tail) and
// single-leaf padding trees come out unchanged.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) v4_level_order_kernel(
    const int2* __restrict__ in,       // [Tpad][max_nodes] pre-order
    const int32_t* __restrict__ ncnt,  // [Tpad]
    int2* __restrict__ out,            // [Tpad][max_nodes] level order
    int32_t max_nodes) {
  uint16_t* order = (uint16_t*)smem;  // [max_nodes] new index -> old index
  const int lane = threadIdx.x;
  const int2* src = in + (int64_t)blockIdx.x * max_nodes;
  int2* dst = out + (int64_t)blockIdx.x * max_nodes;
  const int n = min(max(ncnt[blockIdx.x], 1), max_nodes);
  for (int i = n + lane; i < max_nodes; i += WAVE) dst[i] = src[i];
  if (lane == 0) order[0] = 0;
  __syncthreads();
  int begin = 0, end = 1;  // the current level, in new indices
  while (begin < end) {
    int tail = end;  // next free new index (wave-uniform)
    for (int base = begin; base < end; base += WAVE) {
      const int i = base + lane;
      int2 rec = make_int2(0, 0);
      int old = 0, right = 0;
      bool internal = false;
      if (i < end) {
        old = min((int)order[i], n - 1);
        rec = src[old];
        right = pn_right(rec.x);
        // a leaf links to itself; children outside the tree (a malformed
        // record) are not followed, so every index stays below n
        internal = right != old && right < n && old + 1 < n;
      }
      const uint64_t m = __ballot(internal);
      int link = i;
      if (internal) {
        const int l = tail + 2 * __popcll(m & LANE_MASK_LT(lane));
        if (l + 1 < n) {
          order[l] = (uint16_t)(old + 1);
          order[l + 1] = (uint16_t)right;
          link = l + 1;
        }
      }
      if (i < end)
        dst[i] = make_int2((rec.x & ~(0x7FFF << 12)) | (link << 12), rec.y);
      tail = min(tail + 2 * __popcll(m), n);
    }
    __syncthreads();  // the next level's order[] entries are written
    begin = end;
    end = tail;
  }
  // nodes no link reaches (never in a packed tree): self-loops, so that
  // every record of the output is defined and in bounds
  for (int i = end + lane; i < n; i += WAVE)
    dst[i] = make_int2((src[i].x & ~(0x7FFF << 12)) | (i << 12), src[i].y);
}

// element offset of block row j inside one slab of the v4 key tile. 32-bit
// keys: element j. 16-bit keys: P = RPT*128 words per slab, row j in word
// (j mod P), half (j / P) — RPT=2 pairs rows tid and tid+256 in one word,
// RPT=1 pairs rows tid and tid+128. RPT here is tile rows / 256: the heap
// walk's 512-thread blocks pass 2 for their one row per thread, so a 512-row
// tile has one map however its rows are shared out among threads.
template <typename KT, int RPT>
__device__ __forceinline__ int v4_tile_slot(int j) {
  if (sizeof(KT) == 4) return j;
  constexpr int P = RPT * 128;
  return (j % P) * 2 + j / P;
}

// PACKED: the source is packed [N][d] and the strides fold to (d, 1) at
// compile time (entry point score_forest_v4_packed, below). Runtime strides
// cost the packed 20M x 32 pass 0.3-0.5 % (profiles/strided.md). The packed
// entry point exists only for rows and nodes staged in LDS at ILP 4, the
// shape that pass runs; everything else has one entry point for all layouts.
// More would push tools/native/ifa_score, which links every kernel of this
// file but the heap-record ones, past the
// 2048 KB that tools/lint_offline.py allows any file of the tree
// (tests/test_timing_and_bench.py runs it after the build).
template <typename KT, int RPT, bool ROWS_LDS, int V4_ILP, bool NODES_LDS,
          bool PACKED>
__device__ __forceinline__ void score_forest_v4_body(
    const KT* __restrict__ X,          // raw bf16/fp16/f32 bits [N][d]
    const int2* __restrict__ nodes,    // [Tpad][max_nodes] packed v4
    const int32_t* __restrict__ ncnt,  // [Tpad]
    float* __restrict__ out,           // [N] (path sum or score)
    int64_t N, int32_t d, int32_t Tpad, int32_t max_nodes,
    int32_t height_limit, float fT, float c_norm, int32_t finalize,
    int64_t rs_, int64_t cs_) {
  const int tid = threadIdx.x;
  const int rows_per_iter = RPT * 256;
  const int64_t rs = PACKED ? (int64_t)d : rs_;
  const int64_t cs = PACKED ? (int64_t)1 : cs_;
  // key tile, feature-major: slab f = keys of feature f for every row of the
  // block, slab d = the all-ones leaf sentinel. FS is the slab stride in
  // elements; row j sits at element v4_tile_slot(j) of each slab, so the 64
  // lanes of a wave read lane-adjacent words and the bank is (lane mod 32)
  // for ANY per-lane mix of features (the row-major tile was conflict-free
  // only when every lane wanted the same feature).
  constexpr int FS = RPT * 256;

  int2* tlds = (int2*)smem;  // [V4_ILP * max_nodes] when NODES_LDS
  KT* rows = (KT*)(tlds + (NODES_LDS ? V4_ILP * max_nodes : 0));

  for (int64_t block_row0 = (int64_t)blockIdx.x * rows_per_iter; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * rows_per_iter) {
    const int rows_here = (int)min((int64_t)rows_per_iter, N - block_row0);

    if (ROWS_LDS) {
      __syncthreads();  // previous iteration's readers done
      // each thread stages its own rows: lanes with consecutive rows store
      // consecutive words of a slab (conflict-free), row-major rows are
      // fetched in 16-byte pieces when their starts are 16-byte aligned.
      // A feature-major source (rs == 1) takes the element loop, where the
      // lanes of a wave read consecutive addresses of one feature.
      constexpr int EPV = 16 / (int)sizeof(KT);
      const bool vec = cs == 1 && d % EPV == 0 && rs % EPV == 0 &&
                       ((uintptr_t)X & 15) == 0;
#pragma unroll
      for (int r = 0; r < RPT; ++r) {
        const int j = tid + r * 256;
        KT* dst = rows + v4_tile_slot<KT, RPT>(j);
        if (j < rows_here) {
          const KT* src = X + (block_row0 + j) * rs;
          if (vec) {
            for (int c = 0; c < d; c += EPV) {
              union { uint4 v; KT e[EPV]; } pc;
              pc.v = *(const uint4*)(src + c);
#pragma unroll
              for (int k = 0; k < EPV; ++k)
                dst[(c + k) * FS] = key_of_bits<KT>(pc.e[k]);
            }
          } else {
            if (PACKED) {
              for (int c = 0; c < d; ++c)
                dst[c * FS] = key_of_bits<KT>(src[c]);
            } else {
              for (int c = 0; c < d; ++c, src += cs)
                dst[c * FS] = key_of_bits<KT>(*src);
            }
          }
        } else {
          // tail block: rows past N are walked but never stored
          for (int c = 0; c < d; ++c) dst[c * FS] = key_sentinel<KT>();
        }
        dst[d * FS] = key_sentinel<KT>();  // leaf sentinel slab
      }
      __syncthreads();
    }

    const KT* rb[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r)
      rb[r] = rows + v4_tile_slot<KT, RPT>(tid + r * 256);

    float psum[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) psum[r] = 0.f;

    for (int t = 0; t < Tpad; t += V4_ILP) {
      if (NODES_LDS) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < V4_ILP; ++s) {
          const int ncs = ncnt[t + s];
          const int2* ss = nodes + (int64_t)(t + s) * max_nodes;
          for (int i = tid; i < ncs; i += 256) tlds[s * max_nodes + i] = ss[i];
        }
        __syncthreads();
      }
      const int2* nbase[V4_ILP];
#pragma unroll
      for (int s = 0; s < V4_ILP; ++s)
        nbase[s] = NODES_LDS ? nullptr
                             : nodes + (int64_t)(t + s) * max_nodes;

      int cur[RPT][V4_ILP];
#pragma unroll
      for (int r = 0; r < RPT; ++r)
#pragma unroll
        for (int s = 0; s < V4_ILP; ++s) cur[r][s] = 0;

      // one level of all RPT*V4_ILP chains
      auto visit = [&]() __attribute__((always_inline)) {
        // three explicit phases so the compiler BATCHES the LDS reads
        // (8 node reads -> one wait -> 8 key reads -> one wait -> VALU)
        // instead of serializing 8 dependent read+wait round-trips.
        int2 nd[RPT][V4_ILP];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int s = 0; s < V4_ILP; ++s)
            nd[r][s] = NODES_LDS ? tlds[s * max_nodes + cur[r][s]]
                                 : nbase[s][cur[r][s]];
        KT kraw[RPT][V4_ILP];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
#pragma unroll
          for (int s = 0; s < V4_ILP; ++s) {
            int f = pn_feat(nd[r][s].x);
            if (ROWS_LDS) {
              // keep the mask and the slab shift apart: folded into
              // (meta << k) & mask the address costs shift+and+add, left
              // alone it is v_and + one v_lshl_add as for the old tile
              asm("" : "+v"(f));
              kraw[r][s] = rb[r][f * FS];
            } else {
              // global fallback: the sentinel column does not exist in X,
              // so guard the leaf feature index.
              const int64_t my_row = block_row0 + tid + r * 256;
              kraw[r][s] =
                  (f < d && my_row < N) ? X[my_row * rs + f * cs] : KT{};
            }
          }
        }
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
#pragma unroll
          for (int s = 0; s < V4_ILP; ++s) {
            uint32_t x;
            if (ROWS_LDS) {
              x = widen_key(kraw[r][s]);
            } else {
              const int f = pn_feat(nd[r][s].x);
              x = (f < d) ? widen_key(key_of_bits<KT>(kraw[r][s]))
                          : 0xFFFFFFFFu;
            }
            // level order: link = right child, left child = link - 1; a
            // leaf compares false (sentinel key) and keeps link = itself
            cur[r][s] = pn_right(nd[r][s].x) - (x < (uint32_t)nd[r][s].y);
            // keep the index whole (v_bfe, v_subbrev, next v_lshl_add):
            // folded into the next node address it costs two more VALU
            asm("" : "+v"(cur[r][s]));
          }
        }
      };
      // two levels per trip, by hand: the asm statement above counts as
      // convergent, which rules out `#pragma unroll 2` with a remainder
      int it = 0;
      for (; it + 2 <= height_limit; it += 2) {
        visit();
        visit();
      }
      if (it < height_limit) visit();
      // every chain rests at its leaf (self-loop); read value = depth + c(m)
#pragma unroll
      for (int r = 0; r < RPT; ++r)
#pragma unroll
        for (int s = 0; s < V4_ILP; ++s)
          psum[r] = __fadd_rn(
              psum[r],
              __int_as_float((NODES_LDS ? tlds[s * max_nodes + cur[r][s]]
                                        : nbase[s][cur[r][s]]).y));
    }

#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t my_row = block_row0 + tid + r * 256;
      if (my_row < N) {
        if (finalize) {
          const float mean32 = (float)((double)psum[r] / (double)fT);
          const double ratio = (double)mean32 / (double)c_norm;
          out[my_row] = (float)exp2(-ratio);
        } else {
          out[my_row] = psum[r];
        }
      }
    }
  }
}

// Entry points of the body above. score_forest_v4 serves every in-place
// layout with runtime strides; score_forest_v4_packed has the argument list
// the kernel had before it took strides and folds them to (d, 1).
template <typename KT, int RPT, bool ROWS_LDS, int V4_ILP, bool NODES_LDS>
__global__ void __launch_bounds__(256) score_forest_v4(
    const KT* __restrict__ X, const int2* __restrict__ nodes,
    const int32_t* __restrict__ ncnt, float* __restrict__ out, int64_t N,
    int32_t d, int32_t Tpad, int32_t max_nodes, int32_t height_limit,
    float fT, float c_norm, int32_t finalize, int64_t rs, int64_t cs) {
  score_forest_v4_body<KT, RPT, ROWS_LDS, V4_ILP, NODES_LDS, false>(
      X, nodes, ncnt, out, N, d, Tpad, max_nodes, height_limit, fT, c_norm,
      finalize, rs, cs);
}

template <typename KT, int RPT, int V4_ILP>
__global__ void __launch_bounds__(256) score_forest_v4_packed(
    const KT* __restrict__ X, const int2* __restrict__ nodes,
    const int32_t* __restrict__ ncnt, float* __restrict__ out, int64_t N,
    int32_t d, int32_t Tpad, int32_t max_nodes, int32_t height_limit,
    float fT, float c_norm, int32_t finalize) {
  score_forest_v4_body<KT, RPT, true, V4_ILP, true, true>(
      X, nodes, ncnt, out, N, d, Tpad, max_nodes, height_limit, fT, c_norm,
      finalize, d, 1);
}

// ---------------------------------------------------------------------------
// standard scoring, 16-bit rows — heap records
//
// For bf16/fp16 rows the key threshold is 16 bits wide (w1 = key << 16), and
// a tree of height H fits the implicit layout (children of slot c are 2c and
// 2c+1, root at slot 1, slot 0 unused) in 2^(H+1) slots, so the link is
// redundant too. v4_heap_order_kernel turns the packers' pre-order v4
// records into uint32 [Tpad][2^(H+1)]:
//   internal, slot c:  thr16 << 16 | byte offset of the feature's slab in
//                      the key tile (feature * RPT*256 * 2)
//   leaf at depth < H: pass-through records down its always-right path to
//                      level H-1: low half = the sentinel slab's offset,
//                      whose key 0xFFFF is >= every threshold
//   level H:           f32 bits of the leaf value (depth + c(numInstances)),
//                      today's w1
//   never reached:     0
// The visit is ds_read_b32 record, ds_read_u16 key at rows_base + (rec &
// 0xFFFF), a 16-bit compare against the high half, cur = 2*cur + (key >=
// thr16) — the same `x < t goes left` as v4, NaN keys (0xFFFF) right (the
// kernel computes it on the complemented slot, see score_forest_heap). After
// H visits every chain sits on level H; one more read gives the value. A
// tree is a fixed 2^(H+1) * 4 bytes and trees are contiguous, so the stage
// is one linear 16-byte copy with no node count to wait for. Sums are the
// same f32 adds in the same tree order as v4: bitwise the same result.
// The route (bindings.cpp, pick_score_cfg) needs 16-bit rows,
// (d + 1) * RPT*256 * 2 <= 65536 and 4 or 8 trees of 2^(H+1) * 4 bytes in
// LDS next to the tile; everything else stays on score_forest_v4.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) v4_heap_order_kernel(
    const int2* __restrict__ in,       // [Tpad][max_nodes] pre-order v4
    const int32_t* __restrict__ ncnt,  // [Tpad]
    uint32_t* __restrict__ out,        // [Tpad][2 << H]
    int32_t max_nodes, int32_t H, int32_t slab_bytes) {
  int16_t* st = (int16_t*)smem;  // [2 << H] slot -> pre-order index, -1 none
  const int lane = threadIdx.x;
  const int slots = 2 << H;
  const int2* src = in + (int64_t)blockIdx.x * max_nodes;
  uint32_t* dst = out + (int64_t)blockIdx.x * slots;
  const int n = min(max(ncnt[blockIdx.x], 1), max_nodes);
  if (lane == 0) {
    st[1] = 0;
    dst[0] = 0;
  }
  __syncthreads();
  for (int k = 0; k < H; ++k) {
    const int lo = 1 << k;
    for (int c = lo + lane; c < 2 * lo; c += WAVE) {
      const int old = st[c];
      uint32_t rec = 0;
      int l = -1, r = -1;
      if (old >= 0) {
        const int2 nd = src[old];
        const int right = pn_right(nd.x);
        // same test as v4_level_order_kernel: a leaf links to itself, and
        // children outside the tree are not followed
        const bool internal = right != old && right < n && old + 1 < n;
        rec = (internal ? ((uint32_t)nd.y & 0xFFFF0000u) : 0u) |
              ((uint32_t)(pn_feat(nd.x) * slab_bytes) & 0xFFFFu);
        l = internal ? old + 1 : -1;
        r = internal ? right : old;  // a leaf passes through to the right
      }
      dst[c] = rec;
      st[2 * c] = (int16_t)l;
      st[2 * c + 1] = (int16_t)r;
    }
    __syncthreads();  // the next level's st[] entries are written
  }
  for (int c = (1 << H) + lane; c < slots; c += WAVE) {
    const int old = st[c];
    dst[c] = old >= 0 ? (uint32_t)src[old].y : 0u;
  }
}

// Stage one block's rows into the v4 key tile: the staging of
// score_forest_v4_body, which keeps its own copy inline so that its code
// does not move. The caller puts a barrier on either side. BT threads stage
// RPT rows each: thread tid owns rows tid, tid + BT, ... of the RPT*BT-row
// tile, whose slot map depends on the tile's size alone.
template <typename KT, int RPT, bool PACKED, int BT>
__device__ __forceinline__ void v4_stage_tile(KT* rows,
                                              const KT* __restrict__ X,
                                              int64_t block_row0,
                                              int rows_here, int32_t d,
                                              int64_t rs, int64_t cs) {
  constexpr int FS = RPT * BT;
  constexpr int EPV = 16 / (int)sizeof(KT);
  const int tid = threadIdx.x;
  const bool vec = cs == 1 && d % EPV == 0 && rs % EPV == 0 &&
                   ((uintptr_t)X & 15) == 0;
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int j = tid + r * BT;
    KT* dst = rows + v4_tile_slot<KT, RPT * BT / 256>(j);
    if (j < rows_here) {
      const KT* src = X + (block_row0 + j) * rs;
      if (vec) {
        for (int c = 0; c < d; c += EPV) {
          union { uint4 v; KT e[EPV]; } pc;
          pc.v = *(const uint4*)(src + c);
#pragma unroll
          for (int k = 0; k < EPV; ++k)
            dst[(c + k) * FS] = key_of_bits<KT>(pc.e[k]);
        }
      } else {
        if (PACKED) {
          for (int c = 0; c < d; ++c)
            dst[c * FS] = key_of_bits<KT>(src[c]);
        } else {
          for (int c = 0; c < d; ++c, src += cs)
            dst[c * FS] = key_of_bits<KT>(*src);
        }
      }
    } else {
      // tail block: rows past N are walked but never stored
      for (int c = 0; c < d; ++c) dst[c * FS] = key_sentinel<KT>();
    }
    dst[d * FS] = key_sentinel<KT>();  // leaf sentinel slab
  }
}

// PH trees (4 or 8) are staged per barrier phase and walked together: each
// thread keeps RPT rows x PH trees in flight (16 chains at RPT = 2, PH = 8).
//
// The walk tracks the complemented slot n = ~cur (n = ~1 at the root). With
// x = key - thr16 in 32 bits (both below 65536, so no overflow) bit 31 of x
// is `key < thr16`, and cur' = 2*cur + 1 - lt is ~cur' = 2*~cur + lt: one
// subtract and one funnel shift, n' = (n:x) >> 31, where the direct form
// needs a compare, a select and a shift-or. A pass-through record has thr16
// = 0 and the sentinel key 0xFFFF, so x >= 0 and it still goes right. To
// keep the node address one shift-add, every tree is staged REVERSED: word c
// of the global tree sits at word slots-1-c of its LDS window, which is
// tree_end + 4*n bytes with n read as a negative int. The global records
// are untouched. Reversal maps a byte address a to const - a, a bijection on
// banks.
//
// BT threads per block (256 or 512) walk a tile of RPT*BT rows. A 512-row
// tile is the same LDS, the same slot map and the same records whether 256
// threads own two rows each or 512 threads one: the second form puts twice
// the waves on a CU for the same chains in flight (bindings.cpp,
// pick_score_cfg, takes it where the register file holds them all).
template <typename KT, int RPT, bool PACKED, int PH, int BT>
__global__ void __launch_bounds__(BT) score_forest_heap(
    const KT* __restrict__ X,           // raw bf16/fp16 bits
    const uint32_t* __restrict__ heap,  // [Tpad][2 << H] heap records
    float* __restrict__ out,            // [N] (path sum or score)
    int64_t N, int32_t d, int32_t Tpad, int32_t H, float fT, float c_norm,
    int32_t finalize, int64_t rs_, int64_t cs_) {
  static_assert(sizeof(KT) == 2, "heap records hold 16-bit thresholds");
  static_assert(PH == 4 || PH == 8, "4 or 8 trees per barrier phase");
  static_assert(BT == 256 || BT == 512, "4 or 8 waves per block");
  constexpr int ILP = PH;
  const int tid = threadIdx.x;
  const int rows_per_iter = RPT * BT;
  const int64_t rs = PACKED ? (int64_t)d : rs_;
  const int64_t cs = PACKED ? (int64_t)1 : cs_;
  const int slots = 2 << H;
  // 16-byte vectors per tree: slots / 4 = 1 << (H - 1), H >= 1
  const int vmask = (1 << (H - 1)) - 1;

  uint32_t* tlds = (uint32_t*)smem;  // [PH * slots], each tree reversed
  KT* rows = (KT*)(tlds + PH * slots);

  for (int64_t block_row0 = (int64_t)blockIdx.x * rows_per_iter; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * rows_per_iter) {
    const int rows_here = (int)min((int64_t)rows_per_iter, N - block_row0);

    __syncthreads();  // previous iteration's readers done
    v4_stage_tile<KT, RPT, PACKED, BT>(rows, X, block_row0, rows_here, d, rs,
                                       cs);
    // the first stage's leading barrier orders these stores before the walk

    const char* rb[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r)
      rb[r] = (const char*)(rows +
                            v4_tile_slot<KT, RPT * BT / 256>(tid + r * BT));

    float psum[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) psum[r] = 0.f;

    // end of tree s's window: slot c is tend[s][~c]
    const uint32_t* tend[ILP];
#pragma unroll
    for (int s = 0; s < ILP; ++s) tend[s] = tlds + (s + 1) * slots;

    for (int t = 0; t < Tpad; t += PH) {
      // Tpad is a multiple of 4, not necessarily of PH: the last phase may
      // hold half as many trees. The copy stops at tree Tpad - 1; the
      // windows past it are filled with 0, which walks like a padding tree
      // (slab 0, threshold 0) and adds 0.0f
      const int nt = min(PH, Tpad - t);
      __syncthreads();
      {
        // nt * slots >= 16 words, so both sides stay 16-byte aligned. Vector
        // j of a tree goes to vector (slots/4 - 1 - j) of the same tree with
        // its words swapped end for end: i ^ vmask flips j and keeps the tree
        const uint4* src = (const uint4*)(heap + (int64_t)t * slots);
        uint4* dst = (uint4*)tlds;
        const int nvec = nt * (slots / 4);
        for (int i = tid; i < nvec; i += BT) {
          const uint4 v = src[i];
          dst[i ^ vmask] = make_uint4(v.w, v.z, v.y, v.x);
        }
        for (int i = nvec + tid; i < PH * (slots / 4); i += BT)
          dst[i] = make_uint4(0u, 0u, 0u, 0u);
      }
      __syncthreads();

      uint32_t n[RPT][ILP];
#pragma unroll
      for (int r = 0; r < RPT; ++r)
#pragma unroll
        for (int s = 0; s < ILP; ++s) n[r][s] = ~1u;

      // one level of all RPT*ILP chains, reads batched as in v4
      auto visit = [&]() __attribute__((always_inline)) {
        uint32_t rec[RPT][ILP];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int s = 0; s < ILP; ++s)
            rec[r][s] = tend[s][(int32_t)n[r][s]];
        uint32_t key[RPT][ILP];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int s = 0; s < ILP; ++s)
            key[r][s] =
                *(const uint16_t*)(rb[r] + (rec[r][s] & 0xFFFFu));
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int s = 0; s < ILP; ++s)
            n[r][s] = __builtin_amdgcn_alignbit(
                n[r][s], key[r][s] - (rec[r][s] >> 16), 31);
      };
      int it = 0;
      for (; it + 2 <= H; it += 2) {
        visit();
        visit();
      }
      if (it < H) visit();
      // every chain sits on level H: the slot holds depth + c(m)
#pragma unroll
      for (int r = 0; r < RPT; ++r)
#pragma unroll
        for (int s = 0; s < ILP; ++s)
          psum[r] = __fadd_rn(
              psum[r], __uint_as_float(tend[s][(int32_t)n[r][s]]));
    }

#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t my_row = block_row0 + tid + r * BT;
      if (my_row < N) {
        if (finalize) {
          const float mean32 = (float)((double)psum[r] / (double)fT);
          const double ratio = (double)mean32 / (double)c_norm;
          out[my_row] = (float)exp2(-ratio);
        } else {
          out[my_row] = psum[r];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// extended scoring, dense fast path (nnz == d): per visit a dense dot
// row[0..d) . w[0..d). WLDS stages the live tree's weight matrix in LDS
// (L2 could not feed the ~17 TB/s the global-weight variant demanded);
// rows are read as 8-byte vectors (4 bf16/fp16 or 2 f32 at a time).
// Accumulation: 4 partial sums, pairwise combine (deterministic, not the
// oracle's j-order — scoring parity tests use tolerance).
// ---------------------------------------------------------------------------

__device__ __forceinline__ void row4(const uint16_t* p, int j4, float& x0,
                                     float& x1, float& x2, float& x3) {
  const uint2 v = *(const uint2*)(p + 4 * j4);  // 8 B: 4 bf16
  union { uint32_t u; float f; } a, b, c, e;
  a.u = (v.x & 0xFFFFu) << 16;
  b.u = (v.x & 0xFFFF0000u);
  c.u = (v.y & 0xFFFFu) << 16;
  e.u = (v.y & 0xFFFF0000u);
  x0 = a.f; x1 = b.f; x2 = c.f; x3 = e.f;
}

__device__ __forceinline__ void row4(const f16_t* p, int j4, float& x0,
                                     float& x1, float& x2, float& x3) {
  const uint2 v = *(const uint2*)(p + 4 * j4);  // 8 B: 4 fp16
  x0 = f16_bits_to_f32((uint16_t)(v.x & 0xFFFFu));
  x1 = f16_bits_to_f32((uint16_t)(v.x >> 16));
  x2 = f16_bits_to_f32((uint16_t)(v.y & 0xFFFFu));
  x3 = f16_bits_to_f32((uint16_t)(v.y >> 16));
}

__device__ __forceinline__ void row4(const float* p, int j4, float& x0,
                                     float& x1, float& x2, float& x3) {
  const float4 v = *(const float4*)(p + 4 * j4);
  x0 = v.x; x1 = v.y; x2 = v.z; x3 = v.w;
}

// Row tile of a feature-major source (rs == 1) for the staging loops whose
// flat index g -> (g / d, g % d) is coalesced only over packed rows: the row
// index runs fastest, so the lanes of a wave read consecutive rows of one
// column. X0 = X + block_row0; 256 threads; fn maps a loaded element to the
// stored one. rows_here * d stays far below 2^31 (<= 512 rows, d <= 4095).
template <typename T, typename Fn>
__device__ __forceinline__ void stage_tile_feature_major(
    T* rows, const T* X0, int rows_here, int d, int dpad, int64_t cs, int tid,
    Fn fn) {
  const uint32_t total = (uint32_t)rows_here * (uint32_t)d;
  for (uint32_t g = tid; g < total; g += 256) {
    const int c = (int)(g / (uint32_t)rows_here);
    const int r = (int)(g % (uint32_t)rows_here);
    rows[r * dpad + c] = fn(X0[r + (int64_t)c * cs]);
  }
}

template <typename T>
__device__ __forceinline__ T stage_as_is(T v) { return v; }

template <typename XT, bool ROWS_LDS, bool WLDS>
__global__ void __launch_bounds__(256) score_extended_dense_kernel(
    const XT* __restrict__ X, const int2* __restrict__ nodes,
    const float* __restrict__ hw_g,  // [T][max_nodes][d] dense weights
    const int32_t* __restrict__ ncnt, float* __restrict__ out, int64_t N,
    int32_t d, int64_t rs, int64_t cs, int32_t dpad, int32_t T,
    int32_t max_nodes, float fT, float c_norm, int32_t finalize) {
  const int tid = threadIdx.x;
  const int d4 = d >> 2;

  int2* tlds = (int2*)smem;                  // [max_nodes]
  float* wlds = (float*)(tlds + max_nodes);  // [max_nodes * d] if WLDS
  XT* rows = (XT*)(wlds + (WLDS ? max_nodes * d : 0));

  for (int64_t block_row0 = (int64_t)blockIdx.x * 256; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * 256) {
    const int64_t my_row = block_row0 + tid;
    const int rows_here = (int)min((int64_t)256, N - block_row0);

    if (ROWS_LDS) {
      __syncthreads();
      if (rs == 1) {
        stage_tile_feature_major(rows, X + block_row0, rows_here, d, dpad, cs,
                                 tid, stage_as_is<XT>);
      } else {
        const int64_t total = (int64_t)rows_here * d;
        for (int64_t g = tid; g < total; g += 256) {
          const int r = (int)(g / d), c = (int)(g % d);
          rows[r * dpad + c] = X[(block_row0 + r) * rs + c * cs];
        }
      }
      __syncthreads();
    }
    const XT* my_lrow = rows + tid * dpad;

    float path_sum = 0.f;
    for (int t = 0; t < T; ++t) {
      __syncthreads();
      const int nc = ncnt[t];
      const int2* src = nodes + (int64_t)t * max_nodes;
      for (int i = tid; i < nc; i += 256) tlds[i] = src[i];
      if (WLDS) {
        const float4* wsrc = (const float4*)(hw_g + (int64_t)t * max_nodes * d);
        float4* wdst = (float4*)wlds;
        const int n4 = nc * d4;
        for (int i = tid; i < n4; i += 256) wdst[i] = wsrc[i];
      }
      __syncthreads();

      if (my_row < N) {
        const float* wbase =
            WLDS ? wlds : hw_g + (int64_t)t * max_nodes * d;
        int cur = 0, dep = 0;
        float leaf = 0.f;
        while (true) {
          const int2 nd = tlds[cur];
          if (nd.x < 0) {
            leaf = __int_as_float(nd.y);
            break;
          }
          const float4* wp = (const float4*)(wbase + (int64_t)cur * d);
          float ax = 0.f, ay = 0.f, az = 0.f, aw = 0.f;
          for (int j = 0; j < d4; ++j) {
            const float4 w = wp[j];
            float x0, x1, x2, x3;
            if (ROWS_LDS) {
              row4(my_lrow, j, x0, x1, x2, x3);
            } else {
              const int64_t xo = my_row * rs + 4 * j * cs;
              x0 = load_feat<XT>(X, xo);
              x1 = load_feat<XT>(X, xo + cs);
              x2 = load_feat<XT>(X, xo + 2 * cs);
              x3 = load_feat<XT>(X, xo + 3 * cs);
            }
            ax = __fadd_rn(ax, __fmul_rn(w.x, x0));
            ay = __fadd_rn(ay, __fmul_rn(w.y, x1));
            az = __fadd_rn(az, __fmul_rn(w.z, x2));
            aw = __fadd_rn(aw, __fmul_rn(w.w, x3));
          }
          const float dot =
              __fadd_rn(__fadd_rn(ax, ay), __fadd_rn(az, aw));
          cur = (dot < __int_as_float(nd.y)) ? cur + 1 : pn_right(nd.x);
          ++dep;
        }
        path_sum = __fadd_rn(path_sum, __fadd_rn((float)dep, leaf));
      }
    }
    if (my_row < N) {
      if (finalize) {
        const float mean32 = (float)((double)path_sum / (double)fT);
        const double ratio = (double)mean32 / (double)c_norm;
        out[my_row] = (float)exp2(-ratio);
      } else {
        out[my_row] = path_sum;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// extended scoring, dense fast path v2 (nnz == d, d <= 32).
//
// Rows live in REGISTERS (f32, templated D) across the whole tree loop —
// loaded once per 512-row block iteration, reused for all T trees. Per tree
// the node records {right|self-loop, offset32 / -inf}, the depth-folded leaf
// values and the dense weight matrix (row stride D+4 words to spread the
// b128 reads across banks) are staged in LDS. Each thread walks RPT rows
// concurrently through a FIXED height-trip loop (leaves self-loop: zero
// weight row + offset -inf routes right). The dot uses 4 partial fma
// accumulators (same reassociation contract as v1 — tolerance, not
// bitwise; build stays bitwise).
// ---------------------------------------------------------------------------

template <typename KT>  // u16 = bf16 rows, f16_t = fp16 rows, u32 = f32 rows
__device__ __forceinline__ float load_row_f32(const KT* X, int64_t off);
template <>
__device__ __forceinline__ float load_row_f32<f16_t>(const f16_t* X,
                                                     int64_t off) {
  return f16_bits_to_f32((uint16_t)X[off]);
}
template <>
__device__ __forceinline__ float load_row_f32<uint16_t>(const uint16_t* X,
                                                        int64_t off) {
  return cvt_feat(X[off]);
}
template <>
__device__ __forceinline__ float load_row_f32<uint32_t>(const uint32_t* X,
                                                        int64_t off) {
  union { uint32_t u; float f; } cv;
  cv.u = X[off];
  return cv.f;
}

// Row storage for the dense-EIF walk: rows are converted to f32 ONCE at
// load (bf16->f32 is an exact shift, fp16->f32 an exact convert) and held
// in registers across the
// whole tree loop, so the dot needs zero per-visit unpack VALU. Register
// budget: D=32 runs RPT=1 (32 row VGPRs), D<=16 runs RPT=2.
template <typename KT, int D>
struct RowReg {
  float v[D];
  __device__ __forceinline__ void load(const KT* X, int64_t base, int64_t cs,
                                       int d, bool ok) {
#pragma unroll
    for (int j = 0; j < D; ++j)
      v[j] = (ok && j < d) ? load_row_f32<KT>(X, base + j * cs) : 0.f;
  }
  __device__ __forceinline__ float get(int j) const { return v[j]; }
};

#define EIFD_THREADS 512

template <typename KT, int D, int RPT>
__global__ void __launch_bounds__(EIFD_THREADS,
                                  (D == 64) ? 2 : 4) score_extended_dense_v2(
    const KT* __restrict__ X,           // raw bits [N][d]
    const int2* __restrict__ nodes,     // [T][max_nodes] {w0, offset/-inf}
    const float* __restrict__ values,   // [T][max_nodes] leaf value+depth
    const float* __restrict__ hw,       // [T][max_nodes][D] PADDED dense w
    const int32_t* __restrict__ ncnt,   // [T]
    float* __restrict__ out, int64_t N, int32_t d, int64_t rs, int64_t cs,
    int32_t T, int32_t max_nodes, int32_t height_limit, float fT,
    float c_norm, int32_t finalize) {
  const int tid = threadIdx.x;
  const int rows_per_iter = RPT * EIFD_THREADS;
  const int DW4 = D / 4 + 1;  // LDS weight-row stride in float4s

  int2* tlds = (int2*)smem;                  // [max_nodes]
  float* vlds = (float*)(tlds + max_nodes);  // [max_nodes]
  float4* wlds = (float4*)(((uintptr_t)(vlds + max_nodes) + 15) & ~15ull);

  for (int64_t block_row0 = (int64_t)blockIdx.x * rows_per_iter; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * rows_per_iter) {
    RowReg<KT, D> row[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t my_row = block_row0 + tid + r * EIFD_THREADS;
      row[r].load(X, my_row * rs, cs, d, my_row < N);
    }

    float psum[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) psum[r] = 0.f;

    for (int t = 0; t < T; ++t) {
      __syncthreads();
      const int nc = ncnt[t];
      {
        const int2* ss = nodes + (int64_t)t * max_nodes;
        const float* vs = values + (int64_t)t * max_nodes;
        for (int i = tid; i < nc; i += EIFD_THREADS) {
          tlds[i] = ss[i];
          vlds[i] = vs[i];
        }
        // weights are host-padded to D columns: pure float4 copy with
        // shift indexing (D/4 is a power of two for D in {8,16,32})
        const float4* ws = (const float4*)(hw + (int64_t)t * max_nodes * D);
        const int total4 = nc * (D / 4);
        for (int g = tid; g < total4; g += EIFD_THREADS) {
          const int i = g / (D / 4), j4 = g % (D / 4);
          wlds[i * DW4 + j4] = ws[g];
        }
      }
      __syncthreads();

      int cur[RPT];
#pragma unroll
      for (int r = 0; r < RPT; ++r) cur[r] = 0;

      for (int it = 0; it < height_limit; ++it) {
        int2 nd[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) nd[r] = tlds[cur[r]];
        // weight reads in chunks to bound live registers (quarter chunks at
        // D=32 keep the kernel under 128 VGPRs). Lanes whose walk already
        // ended (leaf self-loop: right == own id) are exec-masked out of
        // the dot — masked lanes issue no LDS accesses, cutting the bank-
        // conflict cycles that bound this kernel.
        constexpr int CHUNKS = (D >= 64) ? 8 : ((D >= 32) ? 4 : 2);
        constexpr int CW4 = D / (4 * CHUNKS);  // float4s per chunk
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
          const int right = pn_right(nd[r].x);
          if (right != cur[r]) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
            for (int ch = 0; ch < CHUNKS; ++ch) {
              float4 w[CW4];
              const float4* wp = wlds + cur[r] * DW4 + ch * CW4;
#pragma unroll
              for (int j4 = 0; j4 < CW4; ++j4) w[j4] = wp[j4];
#pragma unroll
              for (int j4 = 0; j4 < CW4; ++j4) {
                const int j = ch * (D / CHUNKS) + 4 * j4;
                a0 = __builtin_fmaf(w[j4].x, row[r].get(j + 0), a0);
                a1 = __builtin_fmaf(w[j4].y, row[r].get(j + 1), a1);
                a2 = __builtin_fmaf(w[j4].z, row[r].get(j + 2), a2);
                a3 = __builtin_fmaf(w[j4].w, row[r].get(j + 3), a3);
              }
            }
            const float dot = __fadd_rn(__fadd_rn(a0, a1),
                                        __fadd_rn(a2, a3));
            cur[r] = (dot < __int_as_float(nd[r].y)) ? cur[r] + 1 : right;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < RPT; ++r)
        psum[r] = __fadd_rn(psum[r], vlds[cur[r]]);
    }

#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t my_row = block_row0 + tid + r * EIFD_THREADS;
      if (my_row < N) {
        if (finalize) {
          const float mean32 = (float)((double)psum[r] / (double)fT);
          const double ratio = (double)mean32 / (double)c_norm;
          out[my_row] = (float)exp2(-ratio);
        } else {
          out[my_row] = psum[r];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// extended scoring, dense fast path v3 — bf16 INPUT rows only.
//
// The v2 kernel is bound by its per-visit 128-B f32 LDS weight-row read
// (PMC: 27% LDS conflict cycles, WAIT_ANY 44% — profiles/
// r01_bench_and_kernels.md). v3 halves that traffic: weights are staged in
// LDS as PACKED bf16 (round-to-nearest-even from the trained f32 weights,
// done once on device), rows are kept as packed-bf16 register pairs (the
// input is already bf16, so the pack is exact), and the dot runs on
// v_dot2c_f32_bf16 (2 MACs/instr, f32 accumulate) — 4 partial accumulator
// chains, same reassociation family as v2. Per wave-visit: 4x ds_read_b128
// (16 LDS-array cycles before conflicts) instead of v2's 8 (32 cycles),
// and ~half the dot VALU. Numerics: weights are bf16-rounded => knife-edge
// walk decisions can differ from the f32-weight oracle; the contract is
// documented in PARITY.md and tested against a bf16-weight oracle with the
// same isolated-flip allowance as the v2 dense route. f32 input rows keep
// the v2 kernel (unchanged f32-weight numerics).
// ---------------------------------------------------------------------------

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float dot2_bf16(uint32_t w, uint32_t x, float acc) {
  union { uint32_t u; bf16x2_t v; } cw, cx;
  cw.u = w;
  cx.u = x;
  return __builtin_amdgcn_fdot2_f32_bf16(cw.v, cx.v, acc, false);
}

template <int D, int RPT>
__global__ void __launch_bounds__(EIFD_THREADS,
                                  (D == 128) ? 2
                                             : ((D == 64
                                                 || (D == 32 && RPT == 2))
                                                    ? 4
                                                    : 6))
score_extended_dense_v3(
    const uint16_t* __restrict__ X,     // raw bf16 bits [N][d]
    const int2* __restrict__ nodes,     // [T][max_nodes] {right<<12, offset/-inf}
    const float* __restrict__ values,   // [T][max_nodes] leaf value+depth
    const uint32_t* __restrict__ hwp,   // [T][max_nodes][D/2] packed bf16 pairs
    const int32_t* __restrict__ ncnt,   // [T]
    float* __restrict__ out, int64_t N, int32_t d, int64_t rs, int64_t cs,
    int32_t T, int32_t max_nodes, int32_t height_limit, float fT,
    float c_norm, int32_t finalize) {
  const int tid = threadIdx.x;
  const int rows_per_iter = RPT * EIFD_THREADS;
  constexpr int PW4 = D / 8 + 1;  // LDS weight-row stride in uint4s

  int2* tlds = (int2*)smem;                  // [max_nodes]
  float* vlds = (float*)(tlds + max_nodes);  // [max_nodes]
  uint4* wlds = (uint4*)(((uintptr_t)(vlds + max_nodes) + 15) & ~15ull);

  for (int64_t block_row0 = (int64_t)blockIdx.x * rows_per_iter; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * rows_per_iter) {
    uint32_t xp[RPT][D / 2];  // packed bf16 feature pairs, exact
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t my_row = block_row0 + tid + r * EIFD_THREADS;
      const bool ok = my_row < N;
      const int64_t base = my_row * rs;
#pragma unroll
      for (int j2 = 0; j2 < D / 2; ++j2) {
        const uint32_t lo = (ok && 2 * j2 < d) ? X[base + 2 * j2 * cs] : 0u;
        const uint32_t hi =
            (ok && 2 * j2 + 1 < d) ? X[base + (2 * j2 + 1) * cs] : 0u;
        xp[r][j2] = lo | (hi << 16);
      }
    }

    float psum[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) psum[r] = 0.f;

    for (int t = 0; t < T; ++t) {
      __syncthreads();
      const int nc = ncnt[t];
      {
        const int2* ss = nodes + (int64_t)t * max_nodes;
        const float* vs = values + (int64_t)t * max_nodes;
        for (int i = tid; i < nc; i += EIFD_THREADS) {
          tlds[i] = ss[i];
          vlds[i] = vs[i];
        }
        // packed rows are D/8 uint4s wide in global, PW4 in LDS
        const uint4* ws = (const uint4*)(hwp + (int64_t)t * max_nodes * (D / 2));
        const int total4 = nc * (D / 8);
        for (int g = tid; g < total4; g += EIFD_THREADS) {
          const int i = g / (D / 8), j4 = g % (D / 8);
          wlds[i * PW4 + j4] = ws[g];
        }
      }
      __syncthreads();

      int cur[RPT];
#pragma unroll
      for (int r = 0; r < RPT; ++r) cur[r] = 0;

      for (int it = 0; it < height_limit; ++it) {
        int2 nd[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) nd[r] = tlds[cur[r]];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
          const int right = pn_right(nd[r].x);
          if (right != cur[r]) {  // exec-mask finished walks out of the dot
            // chunked reads bound live w registers (D=32 stays under the
            // 80-VGPR budget that keeps 6 waves/SIMD resident)
            constexpr int CHUNKS = (D >= 32) ? 2 : 1;
            constexpr int CW4 = D / (8 * CHUNKS);  // uint4s per chunk
            const uint4* wp = wlds + cur[r] * PW4;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
            for (int ch = 0; ch < CHUNKS; ++ch) {
              uint4 w[CW4];
#pragma unroll
              for (int j4 = 0; j4 < CW4; ++j4) w[j4] = wp[ch * CW4 + j4];
#pragma unroll
              for (int j4 = 0; j4 < CW4; ++j4) {
                const int p = (ch * CW4 + j4) * 4;
                a0 = dot2_bf16(w[j4].x, xp[r][p + 0], a0);
                a1 = dot2_bf16(w[j4].y, xp[r][p + 1], a1);
                a2 = dot2_bf16(w[j4].z, xp[r][p + 2], a2);
                a3 = dot2_bf16(w[j4].w, xp[r][p + 3], a3);
              }
            }
            const float dot = __fadd_rn(__fadd_rn(a0, a1),
                                        __fadd_rn(a2, a3));
            cur[r] = (dot < __int_as_float(nd[r].y)) ? cur[r] + 1 : right;
          }
        }
      }
#pragma unroll
      for (int r = 0; r < RPT; ++r)
        psum[r] = __fadd_rn(psum[r], vlds[cur[r]]);
    }

#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t my_row = block_row0 + tid + r * EIFD_THREADS;
      if (my_row < N) {
        if (finalize) {
          const float mean32 = (float)((double)psum[r] / (double)fT);
          const double ratio = (double)mean32 / (double)c_norm;
          out[my_row] = (float)exp2(-ratio);
        } else {
          out[my_row] = psum[r];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// dense v2/v3 companion: rows holding an inf/NaN cell, rescored in the
// oracle's strict j-order.
//
// With nnz == d such a row's dot is inf or NaN in every summation order,
// but WHICH of the two depends on the order once finite partial sums
// overflow (+-3e38 cells): -inf + (a + b -> +inf) = NaN, while
// ((-inf + a) + b) = -inf, and NaN < offset is false where -inf < offset is
// true. The 4-chain kernels above therefore cannot promise the oracle's
// branch on these rows. This pass runs after them on the same stream: a
// coalesced scan flags the rows of each 256-row tile that hold a
// non-finite cell, and only those rows walk every tree again with the
// strict mul/add dot (weights and nodes from global memory — a correctness
// path) and overwrite their output. Clean rows are left untouched, so the
// fast kernels keep their registers and occupancy. PACKED_W = v3's packed
// bf16 weight pairs, else v2's padded f32 weights. Bitwise vs
// cpu_engine.path_lengths_extended for nnz == d.
// ---------------------------------------------------------------------------

__device__ __forceinline__ bool nonfinite_bits(uint16_t b) {
  return (b & 0x7F80u) == 0x7F80u;
}
__device__ __forceinline__ bool nonfinite_bits(f16_t b) {
  return ((uint16_t)b & 0x7C00u) == 0x7C00u;
}
__device__ __forceinline__ bool nonfinite_bits(uint32_t b) {
  return (b & 0x7F800000u) == 0x7F800000u;
}

template <typename KT, bool PACKED_W>
__global__ void __launch_bounds__(256) score_extended_dense_nonfinite_rows(
    const KT* __restrict__ X,           // raw bits [N][d]
    const int2* __restrict__ nodes,     // [T][max_nodes] {right<<12, offset/-inf}
    const float* __restrict__ values,   // [T][max_nodes] leaf value+depth
    const void* __restrict__ wts,       // f32 [T][max_nodes][D] or packed
                                        // bf16 pairs u32 [T][max_nodes][D/2]
    float* __restrict__ out, int64_t N, int32_t d, int64_t rs, int64_t cs,
    int32_t D, int32_t T, int32_t max_nodes, int32_t height_limit, float fT,
    float c_norm, int32_t finalize) {
  __shared__ int flagged[256];
  const int tid = threadIdx.x;
  for (int64_t block_row0 = (int64_t)blockIdx.x * 256; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * 256) {
    const int rows_here = (int)min((int64_t)256, N - block_row0);
    __syncthreads();  // previous iteration's flag readers done
    flagged[tid] = 0;
    __syncthreads();
    const int total = rows_here * d;
    if (rs == 1) {  // feature-major: lanes scan consecutive rows of a column
      for (int g = tid; g < total; g += 256) {
        const int c = g / rows_here, r = g % rows_here;
        if (nonfinite_bits(X[block_row0 + r + (int64_t)c * cs]))
          flagged[r] = 1;  // every writer stores the same value
      }
    } else {
      for (int g = tid; g < total; g += 256) {
        const int r = g / d, c = g % d;
        if (nonfinite_bits(X[(block_row0 + r) * rs + c * cs]))
          flagged[r] = 1;  // every writer stores the same value
      }
    }
    __syncthreads();
    if (tid >= rows_here || !flagged[tid]) continue;

    const int64_t my_row = block_row0 + tid;
    float psum = 0.f;
    for (int t = 0; t < T; ++t) {
      const int64_t tbase = (int64_t)t * max_nodes;
      int cur = 0;
      for (int it = 0; it < height_limit; ++it) {
        const int2 nd = nodes[tbase + cur];
        const int right = pn_right(nd.x);
        if (right == cur) break;  // leaf self-loop
        float dot = 0.f;
        for (int j = 0; j < d; ++j) {  // oracle j-order
          float w;
          if (PACKED_W) {
            const uint32_t pw =
                ((const uint32_t*)wts)[(tbase + cur) * (D / 2) + (j >> 1)];
            w = __uint_as_float((j & 1) ? (pw & 0xFFFF0000u) : (pw << 16));
          } else {
            w = ((const float*)wts)[(tbase + cur) * D + j];
          }
          dot = __fadd_rn(dot,
                          __fmul_rn(w, load_row_f32<KT>(X,
                          my_row * rs + j * cs)));
        }
        cur = (dot < __int_as_float(nd.y)) ? cur + 1 : right;
      }
      psum = __fadd_rn(psum, values[tbase + cur]);
    }
    if (finalize) {
      const float mean32 = (float)((double)psum / (double)fT);
      const double ratio = (double)mean32 / (double)c_norm;
      out[my_row] = (float)exp2(-ratio);
    } else {
      out[my_row] = psum;
    }
  }
}

// ---------------------------------------------------------------------------
// extended scoring, sparse fast path v2 (nnz <= 5, templated):
// same node/value packing as the dense v2 kernel (self-looping leaves with
// offset -inf and zero weights => fixed-trip walks), rows staged native in
// LDS, hyperplanes (idx+w) staged in LDS, RPT=2 chains per thread with
// batch-phased reads. The dot keeps the ORACLE's strict j-order f32
// accumulation (bitwise vs cpu_engine.path_lengths_extended).
// ---------------------------------------------------------------------------

template <typename KT, int NNZ, int RPT>
__global__ void __launch_bounds__(256) score_extended_sparse_v2(
    const KT* __restrict__ X,           // raw bits [N][d]
    const int2* __restrict__ nodes,     // [T][max_nodes] {w0, offset/-inf}
    const float* __restrict__ values,   // [T][max_nodes] leaf value+depth
    const int32_t* __restrict__ hidx_g, // [T][max_nodes][NNZ]
    const float* __restrict__ hw_g,     // [T][max_nodes][NNZ]
    const int32_t* __restrict__ ncnt, float* __restrict__ out, int64_t N,
    int32_t d, int64_t rs, int64_t cs, int32_t dpad, int32_t T,
    int32_t max_nodes, int32_t height_limit, float fT, float c_norm,
    int32_t finalize) {
  const int tid = threadIdx.x;
  const int rows_per_iter = RPT * 256;

  int2* tlds = (int2*)smem;                   // [max_nodes]
  float* vlds = (float*)(tlds + max_nodes);   // [max_nodes]
  int32_t* ilds = (int32_t*)(vlds + max_nodes);  // [max_nodes][NNZ]
  float* wlds = (float*)(ilds + max_nodes * NNZ);  // [max_nodes][NNZ]
  KT* rows = (KT*)(wlds + max_nodes * NNZ);   // [rows_per_iter][dpad]

  for (int64_t block_row0 = (int64_t)blockIdx.x * rows_per_iter; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * rows_per_iter) {
    const int rows_here = (int)min((int64_t)rows_per_iter, N - block_row0);
    __syncthreads();  // previous iteration's readers done
    if (rs == 1) {
      stage_tile_feature_major(rows, X + block_row0, rows_here, d, dpad, cs,
                               tid, stage_as_is<KT>);
    } else {
      const int64_t total = (int64_t)rows_here * d;
      for (int64_t g = tid; g < total; g += 256) {
        const int r = (int)(g / (uint32_t)d), c = (int)(g % (uint32_t)d);
        rows[r * dpad + c] = X[(block_row0 + r) * rs + c * cs];
      }
    }
    __syncthreads();
    const KT* rb[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) rb[r] = rows + (tid + r * 256) * dpad;

    float psum[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) psum[r] = 0.f;

    for (int t = 0; t < T; ++t) {
      __syncthreads();
      const int nc = ncnt[t];
      {
        const int2* ss = nodes + (int64_t)t * max_nodes;
        const float* vs = values + (int64_t)t * max_nodes;
        for (int i = tid; i < nc; i += 256) {
          tlds[i] = ss[i];
          vlds[i] = vs[i];
        }
        const int32_t* is = hidx_g + (int64_t)t * max_nodes * NNZ;
        const float* ws = hw_g + (int64_t)t * max_nodes * NNZ;
        for (int g = tid; g < nc * NNZ; g += 256) {
          ilds[g] = is[g];
          wlds[g] = ws[g];
        }
      }
      __syncthreads();

      int cur[RPT];
#pragma unroll
      for (int r = 0; r < RPT; ++r) cur[r] = 0;

      for (int it = 0; it < height_limit; ++it) {
        int2 nd[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) nd[r] = tlds[cur[r]];
        int32_t ci[RPT][NNZ];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int j = 0; j < NNZ; ++j) ci[r][j] = ilds[cur[r] * NNZ + j];
        float cw[RPT][NNZ];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int j = 0; j < NNZ; ++j) cw[r][j] = wlds[cur[r] * NNZ + j];
        float xv[RPT][NNZ];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int j = 0; j < NNZ; ++j)
            xv[r][j] = load_row_f32<KT>(rb[r], ci[r][j]);
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
          float dot = 0.f;
#pragma unroll
          for (int j = 0; j < NNZ; ++j)  // oracle j-order
            dot = __fadd_rn(dot, __fmul_rn(cw[r][j], xv[r][j]));
          const int right = pn_right(nd[r].x);
          cur[r] = (dot < __int_as_float(nd[r].y)) ? cur[r] + 1 : right;
        }
      }
#pragma unroll
      for (int r = 0; r < RPT; ++r)
        psum[r] = __fadd_rn(psum[r], vlds[cur[r]]);
    }

#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t my_row = block_row0 + tid + r * 256;
      if (my_row < N) {
        if (finalize) {
          const float mean32 = (float)((double)psum[r] / (double)fT);
          const double ratio = (double)mean32 / (double)c_norm;
          out[my_row] = (float)exp2(-ratio);
        } else {
          out[my_row] = psum[r];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// extended scoring, sparse general path (nnz < d): exact oracle order.
// ---------------------------------------------------------------------------

template <typename XT, bool ROWS_LDS, bool HYPER_LDS, bool NODES_LDS>
__global__ void __launch_bounds__(256) score_extended_forest_kernel(
    const XT* __restrict__ X, const int2* __restrict__ nodes,
    const int32_t* __restrict__ hidx_g,  // [T][max_nodes][nnz]
    const float* __restrict__ hw_g,      // [T][max_nodes][nnz]
    const int32_t* __restrict__ ncnt, float* __restrict__ out, int64_t N,
    int32_t d, int64_t rs, int64_t cs, int32_t T, int32_t max_nodes,
    int32_t nnz, float fT, float c_norm, int32_t finalize) {
  const int tid = threadIdx.x;
  const int dpad = row_stride<XT>(d);

  int2* tlds = (int2*)smem;  // [max_nodes] when NODES_LDS
  int32_t* hidx_lds = (int32_t*)(tlds + (NODES_LDS ? max_nodes : 0));
  float* hw_lds = (float*)(hidx_lds + (HYPER_LDS ? max_nodes * nnz : 0));
  XT* rows = (XT*)(hw_lds + (HYPER_LDS ? max_nodes * nnz : 0));

  for (int64_t block_row0 = (int64_t)blockIdx.x * 256; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * 256) {
    const int64_t my_row = block_row0 + tid;
    const int rows_here = (int)min((int64_t)256, N - block_row0);

    if (ROWS_LDS) {
      __syncthreads();
      if (rs == 1) {
        stage_tile_feature_major(rows, X + block_row0, rows_here, d, dpad, cs,
                                 tid, stage_as_is<XT>);
      } else {
        const int64_t total = (int64_t)rows_here * d;
        for (int64_t g = tid; g < total; g += 256) {
          const int r = (int)(g / d), c = (int)(g % d);
          rows[r * dpad + c] = X[(block_row0 + r) * rs + c * cs];
        }
      }
      __syncthreads();
    }
    const XT* my_lrow = rows + tid * dpad;

    float path_sum = 0.f;
    for (int t = 0; t < T; ++t) {
      __syncthreads();
      const int nc = ncnt[t];
      const int2* src = nodes + (int64_t)t * max_nodes;
      if (NODES_LDS)
        for (int i = tid; i < nc; i += 256) tlds[i] = src[i];
      if (HYPER_LDS) {
        const int64_t hbase = (int64_t)t * max_nodes * nnz;
        for (int i = tid; i < nc * nnz; i += 256) {
          hidx_lds[i] = hidx_g[hbase + i];
          hw_lds[i] = hw_g[hbase + i];
        }
      }
      __syncthreads();

      if (my_row < N) {
        const int64_t hbase = (int64_t)t * max_nodes * nnz;
        int cur = 0, dep = 0;
        float leaf = 0.f;
        while (true) {
          const int2 nd = NODES_LDS ? tlds[cur] : src[cur];
          if (nd.x < 0) {
            leaf = __int_as_float(nd.y);
            break;
          }
          float dot = 0.f;
          const int32_t* ci = HYPER_LDS ? hidx_lds + cur * nnz
                                        : hidx_g + hbase + (int64_t)cur * nnz;
          const float* cw = HYPER_LDS ? hw_lds + cur * nnz
                                      : hw_g + hbase + (int64_t)cur * nnz;
          for (int j = 0; j < nnz; ++j) {
            const float xv = ROWS_LDS
                                 ? cvt_feat(my_lrow[ci[j]])
                                 : load_feat<XT>(X, my_row * rs + ci[j] * cs);
            dot = __fadd_rn(dot, __fmul_rn(cw[j], xv));
          }
          cur = (dot < __int_as_float(nd.y)) ? cur + 1 : pn_right(nd.x);
          ++dep;
        }
        path_sum = __fadd_rn(path_sum, __fadd_rn((float)dep, leaf));
      }
    }
    if (my_row < N) {
      if (finalize) {
        const float mean32 = (float)((double)path_sum / (double)fT);
        const double ratio = (double)mean32 / (double)c_norm;
        out[my_row] = (float)exp2(-ratio);
      } else {
        out[my_row] = path_sum;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// WIDE-format fallback scoring (no packed-field width limits).
//
// The packed v4/EIF node formats cap feature ids at 12 bits (4094) and
// node ids at 15 bits (32767 nodes/tree = maxSamples 16384). Forests
// loaded from foreign files (or CPU-built past the GPU build cap) can
// exceed both; these kernels store each node as a full int4
// {feat, right, key/value, 0} read from GLOBAL memory (L2-served: every
// workgroup walks trees in the same order) with rows read from global —
// a correctness path, not a throughput path (the reference has no such
// size limits: IsolationTree.scala). Same integer-key compare math as v4
// => bitwise vs cpu_engine.path_lengths.
// ---------------------------------------------------------------------------

template <typename KT>
__global__ void __launch_bounds__(256) score_forest_wide(
    const KT* __restrict__ X,          // raw bf16/fp16/f32 bits [N][d]
    const int4* __restrict__ nodes,    // [T][max_nodes] {feat, right, w, 0}
    float* __restrict__ out, int64_t N, int32_t d, int64_t rs, int64_t cs,
    int32_t T, int64_t max_nodes, int32_t height_limit, float fT,
    float c_norm, int32_t finalize) {
  for (int64_t my_row = (int64_t)blockIdx.x * 256 + threadIdx.x; my_row < N;
       my_row += (int64_t)gridDim.x * 256) {
    float psum = 0.f;
    for (int t = 0; t < T; ++t) {
      const int4* base = nodes + (int64_t)t * max_nodes;
      int cur = 0;
      for (int it = 0; it < height_limit; ++it) {
        const int4 nd = base[cur];
        if (nd.y != cur) {  // leaves self-loop (right == own id)
          const uint32_t x =
              widen_key(key_of_bits<KT>(X[my_row * rs + nd.x * cs]));
          cur = (x < (uint32_t)nd.z) ? cur + 1 : nd.y;
        }
      }
      psum = __fadd_rn(psum, __int_as_float(base[cur].z));
    }
    if (finalize) {
      const float mean32 = (float)((double)psum / (double)fT);
      const double ratio = (double)mean32 / (double)c_norm;
      out[my_row] = (float)exp2(-ratio);
    } else {
      out[my_row] = psum;
    }
  }
}

// EIF wide fallback: full-width node records, strict oracle j-order dot
// from global hyperplanes (bitwise vs cpu_engine.path_lengths_extended).
template <typename XT>
__global__ void __launch_bounds__(256) score_extended_wide(
    const XT* __restrict__ X, const int4* __restrict__ nodes,
    const int32_t* __restrict__ hidx_g,  // [T][max_nodes][nnz]
    const float* __restrict__ hw_g,      // [T][max_nodes][nnz]
    float* __restrict__ out, int64_t N, int32_t d, int64_t rs, int64_t cs,
    int32_t T, int64_t max_nodes, int32_t nnz, float fT, float c_norm,
    int32_t finalize) {
  for (int64_t my_row = (int64_t)blockIdx.x * 256 + threadIdx.x; my_row < N;
       my_row += (int64_t)gridDim.x * 256) {
    float path_sum = 0.f;
    for (int t = 0; t < T; ++t) {
      const int4* base = nodes + (int64_t)t * max_nodes;
      const int64_t hbase = (int64_t)t * max_nodes * nnz;
      int cur = 0, dep = 0;
      float leaf = 0.f;
      while (true) {
        const int4 nd = base[cur];
        if (nd.x < 0) {
          leaf = __int_as_float(nd.z);
          break;
        }
        float dot = 0.f;
        const int32_t* ci = hidx_g + hbase + (int64_t)cur * nnz;
        const float* cw = hw_g + hbase + (int64_t)cur * nnz;
        for (int j = 0; j < nnz; ++j) {
          const float xv = load_feat<XT>(X, my_row * rs + ci[j] * cs);
          dot = __fadd_rn(dot, __fmul_rn(cw[j], xv));
        }
        cur = (dot < __int_as_float(nd.z)) ? cur + 1 : nd.y;
        ++dep;
      }
      path_sum = __fadd_rn(path_sum, __fadd_rn((float)dep, leaf));
    }
    if (finalize) {
      const float mean32 = (float)((double)path_sum / (double)fT);
      const double ratio = (double)mean32 / (double)c_norm;
      out[my_row] = (float)exp2(-ratio);
    } else {
      out[my_row] = path_sum;
    }
  }
}

// ---------------------------------------------------------------------------
// Per-feature attribution (docs/DESIGN.md §8): the v4 fixed-trip walk over
// integer keys with one more thing carried along. Node records are 16 B
// {feat | right<<12, key threshold, delta_left bits, delta_right bits};
// leaves and pads self-loop with feat = d (the sentinel column) and both
// deltas +0.0, so the walk needs no leaf test. A row visiting internal node
// v adds the taken edge's f32 delta to acc[row][feat(v)].
//
// The contract is BITWISE vs cpu_engine.feature_contributions, so a row's
// adds happen in one fixed order: trees 0..T-1, root to leaf. A row's trees
// are therefore walked one after another; the independent chains that hide
// LDS latency are the RPT rows a thread owns (plus the other resident
// waves), never several trees of one row. Each thread owns its rows
// outright: no atomics anywhere.
//
// ACC_LDS: accumulators live in an LDS tile [rows][astride] (odd word
// stride; column d absorbs the self-loop +0.0 adds), zeroed per row tile and
// flushed coalesced. Otherwise they are the pre-zeroed out[N][d] itself
// (thread-owned, L2-resident), with the add predicated on f < d.
// ROWS_LDS: keys staged in LDS with the sentinel column, as in v4; else
// read from X and keyed per visit. NODES_LDS: `tps` trees staged per
// barrier; else node records come from global/L2 (deep forests).
// ---------------------------------------------------------------------------

// f32 quotient that is correctly rounded by construction: f64 divide, then
// one rounding (53 >= 2*24+2), so it equals numpy's f32 divide bit for bit.
// Same detour as the hyperplane normalisation in
// build_extended_forest_kernel (whose note records a 1-ulp miss of
// __fdiv_rn) and the mean in score_forest_v4; whether the plain f32 divide
// would also do here has not been measured.
__device__ __forceinline__ float div32_exact(float a, float b) {
  return (float)((double)a / (double)b);
}

// PACKED: the strides fold to (d, 1); instantiated only for mode 0
// (accumulators, rows and nodes in LDS) and used for packed rows. The stride
// arguments come last so that the arguments before them keep their kernarg
// offsets: the PACKED instantiations then compile to the instruction stream
// the kernel had before it took strides, register names aside
// (profiles/strided.md).
template <typename KT, int RPT, bool ACC_LDS, bool ROWS_LDS, bool NODES_LDS,
          bool PACKED>
__global__ void __launch_bounds__(256) explain_forest_kernel(
    const KT* __restrict__ X,          // raw bf16/fp16/f32 bits [N][d]
    const int4* __restrict__ nodes,    // [T][max_nodes] explain records
    const int32_t* __restrict__ ncnt,  // [T]
    float* __restrict__ out,           // [N][d] (pre-zeroed when !ACC_LDS)
    int64_t N, int32_t d, int32_t dpad, int32_t astride, int32_t T,
    int32_t max_nodes, int32_t tps, int32_t height_limit, float fT,
    int32_t finalize, int64_t rs_, int64_t cs_) {
  const int tid = threadIdx.x;
  const int rows_per_iter = RPT * 256;
  const int64_t rs = PACKED ? (int64_t)d : rs_;
  const int64_t cs = PACKED ? (int64_t)1 : cs_;

  int4* tlds = (int4*)smem;  // [tps * max_nodes] when NODES_LDS
  float* acc = (float*)(tlds + (NODES_LDS ? tps * max_nodes : 0));
  KT* rows = (KT*)(acc + (ACC_LDS ? rows_per_iter * astride : 0));

  for (int64_t block_row0 = (int64_t)blockIdx.x * rows_per_iter; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * rows_per_iter) {
    const int rows_here = (int)min((int64_t)rows_per_iter, N - block_row0);

    __syncthreads();  // previous tile's flush / readers done
    if (ROWS_LDS) {
      if (!PACKED && rs == 1) {
        stage_tile_feature_major(rows, X + block_row0, rows_here, d, dpad, cs,
                                 tid, key_of_bits<KT>);
      } else {
        const int64_t total = (int64_t)rows_here * d;
        for (int64_t g = tid; g < total; g += 256) {
          const int r = (int)(g / (uint32_t)d), c = (int)(g % (uint32_t)d);
          rows[r * dpad + c] =
              key_of_bits<KT>(X[(block_row0 + r) * rs + c * cs]);
        }
      }
      for (int r = tid; r < rows_per_iter; r += 256)
        rows[r * dpad + d] = key_sentinel<KT>();  // leaf sentinel column
    }
    if (ACC_LDS)
      for (int i = tid; i < rows_per_iter * astride; i += 256) acc[i] = 0.f;
    // (the staging barrier below orders these writes before the walk)

    const KT* rb[RPT];
    float* ab[RPT];
    int64_t my_row[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      rb[r] = rows + (tid + r * 256) * dpad;
      ab[r] = acc + (tid + r * 256) * astride;
      my_row[r] = block_row0 + tid + r * 256;
    }

    for (int t0 = 0; t0 < T; t0 += tps) {
      const int nst = min(tps, T - t0);
      __syncthreads();
      if (NODES_LDS) {
        for (int s = 0; s < nst; ++s) {
          const int ncs = ncnt[t0 + s];
          const int4* ss = nodes + (int64_t)(t0 + s) * max_nodes;
          for (int i = tid; i < ncs; i += 256) tlds[s * max_nodes + i] = ss[i];
        }
        __syncthreads();
      }
      for (int s = 0; s < nst; ++s) {  // a row's trees: strictly in order
        const int4* nb = NODES_LDS ? tlds + s * max_nodes
                                   : nodes + (int64_t)(t0 + s) * max_nodes;
        int cur[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) cur[r] = 0;

#pragma unroll 2
        for (int it = 0; it < height_limit; ++it) {
          int4 nd[RPT];
#pragma unroll
          for (int r = 0; r < RPT; ++r) nd[r] = nb[cur[r]];
          uint32_t x[RPT];
#pragma unroll
          for (int r = 0; r < RPT; ++r) {
            const int f = pn_feat(nd[r].x);
            if (ROWS_LDS) {
              x[r] = widen_key(rb[r][f]);
            } else {
              // the sentinel column does not exist in X: guard it
              x[r] = (f < d && my_row[r] < N)
                         ? widen_key(key_of_bits<KT>(
                               X[my_row[r] * rs + f * cs]))
                         : 0xFFFFFFFFu;
            }
          }
#pragma unroll
          for (int r = 0; r < RPT; ++r) {
            const int f = pn_feat(nd[r].x);
            const bool left = x[r] < (uint32_t)nd[r].y;
            const float delta = __int_as_float(left ? nd[r].z : nd[r].w);
            if (ACC_LDS) {
              ab[r][f] = __fadd_rn(ab[r][f], delta);
            } else if (f < d && my_row[r] < N) {
              float* o = out + my_row[r] * d + f;
              *o = __fadd_rn(*o, delta);
            }
            cur[r] = left ? cur[r] + 1 : pn_right(nd[r].x);
          }
        }
      }
    }

    if (ACC_LDS) {
      __syncthreads();  // every row's accumulators final
      const int64_t total = (int64_t)rows_here * d;
      for (int64_t g = tid; g < total; g += 256) {
        const int r = (int)(g / (uint32_t)d), c = (int)(g % (uint32_t)d);
        const float v = acc[r * astride + c];
        out[(block_row0 + r) * d + c] = finalize ? div32_exact(v, fT) : v;
      }
    } else if (finalize) {
#pragma unroll
      for (int r = 0; r < RPT; ++r)
        if (my_row[r] < N)
          for (int c = 0; c < d; ++c) {
            float* o = out + my_row[r] * d + c;
            *o = div32_exact(*o, fT);
          }
    }
  }
}

// EIF attribution: one thread per row, everything from global memory, the
// strict j-order dot of score_extended_forest_kernel, walk until the leaf.
// The taken edge's per-coordinate f32 shares (host-computed, [T][mn][nnz])
// are added to the pre-zeroed out[row][hidx[j]] in ascending j over the
// node's k = meta & 0xFFF coordinates. Bitwise vs
// cpu_engine.feature_contributions_extended at every extension level.
template <typename XT>
__global__ void __launch_bounds__(256) explain_extended_kernel(
    const XT* __restrict__ X, const int2* __restrict__ nodes,
    const int32_t* __restrict__ hidx_g,  // [T][max_nodes][nnz]
    const float* __restrict__ hw_g,      // [T][max_nodes][nnz]
    const float* __restrict__ dl_g,      // [T][max_nodes][nnz]
    const float* __restrict__ dr_g,      // [T][max_nodes][nnz]
    float* __restrict__ out,             // [N][d] pre-zeroed
    int64_t N, int32_t d, int64_t rs, int64_t cs, int32_t T,
    int32_t max_nodes, int32_t nnz, float fT, int32_t finalize) {
  for (int64_t my_row = (int64_t)blockIdx.x * 256 + threadIdx.x; my_row < N;
       my_row += (int64_t)gridDim.x * 256) {
    float* orow = out + my_row * d;
    for (int t = 0; t < T; ++t) {
      const int2* base = nodes + (int64_t)t * max_nodes;
      const int64_t hbase = (int64_t)t * max_nodes * nnz;
      int cur = 0;
      while (true) {
        const int2 nd = base[cur];
        if (nd.x < 0) break;
        const int64_t hoff = hbase + (int64_t)cur * nnz;
        const int32_t* ci = hidx_g + hoff;
        const float* cw = hw_g + hoff;
        float dot = 0.f;
        for (int j = 0; j < nnz; ++j) {
          const float xv = load_feat<XT>(X, my_row * rs + ci[j] * cs);
          dot = __fadd_rn(dot, __fmul_rn(cw[j], xv));
        }
        const bool left = dot < __int_as_float(nd.y);
        const float* dj = (left ? dl_g : dr_g) + hoff;
        const int k = min(pn_feat(nd.x), nnz);
        for (int j = 0; j < k; ++j) {
          float* o = orow + ci[j];
          *o = __fadd_rn(*o, dj[j]);
        }
        cur = left ? cur + 1 : pn_right(nd.x);
      }
    }
    if (finalize)
      for (int c = 0; c < d; ++c) orow[c] = div32_exact(orow[c], fT);
  }
}

}  // namespace ifa

// ---------------------------------------------------------------------------
// host-side launchers (bindings.cpp is compiled by g++, so every kernel
// launch lives in this hipcc TU)
// ---------------------------------------------------------------------------

namespace ifa {

static inline void raise_lds(const void* func, size_t bytes) {
  if (bytes > 64 * 1024)
    (void)hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)bytes);
}

void launch_bag_gather(RowDtype dt, const void* X, const int64_t* bag_idx,
                       float* bags, int64_t T, int64_t n, int64_t d,
                       int64_t rs, int64_t cs,
                       hipStream_t stream) {
  int64_t total = T * n * d;
  int threads = 256;
  int blocks = (int)((total + threads - 1) / threads);
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  if (dt == ROW_BF16)
    hipLaunchKernelGGL(bag_gather_kernel<uint16_t>, dim3(blocks), dim3(threads),
                       0, stream, (const uint16_t*)X, bag_idx, bags, T, n, d,
                       rs, cs);
  else if (dt == ROW_F16)
    hipLaunchKernelGGL(bag_gather_kernel<f16_t>, dim3(blocks), dim3(threads),
                       0, stream, (const f16_t*)X, bag_idx, bags, T, n, d, rs,
                       cs);
  else
    hipLaunchKernelGGL(bag_gather_kernel<float>, dim3(blocks), dim3(threads), 0,
                       stream, (const float*)X, bag_idx, bags, T, n, d, rs, cs);
}

void launch_build_forest(const float* bags, const int32_t* feat_sub,
                         int32_t* feat, float* value, int32_t* right,
                         int32_t* count, int32_t* ncount, int32_t* depth,
                         const float* leaf_lut, uint64_t seed,
                         int32_t tree_id_offset, int32_t T, int32_t n,
                         int32_t d, int32_t k, int32_t max_nodes,
                         int32_t height_limit, size_t lds,
                         hipStream_t stream) {
  raise_lds((const void*)build_forest_kernel, lds);
  hipLaunchKernelGGL(build_forest_kernel, dim3(T), dim3(WAVE), lds, stream,
                     bags, feat_sub, feat, value, right, count, ncount,
                     depth, leaf_lut, seed, tree_id_offset, n, d, k,
                     max_nodes, height_limit);
}

void launch_build_extended_forest(const float* bags, const int32_t* feat_sub,
                                  int32_t* feat, float* value, int32_t* right,
                                  int32_t* count, int32_t* ncount,
                                  int32_t* hidx, float* hw, double* off64,
                                  int32_t* depth,
                                  const float* leaf_lut, uint64_t seed,
                                  int32_t tree_id_offset, int32_t T, int32_t n,
                                  int32_t d, int32_t k, int32_t nnz,
                                  int32_t max_nodes, int32_t height_limit,
                                  size_t lds, hipStream_t stream) {
  raise_lds((const void*)build_extended_forest_kernel, lds);
  hipLaunchKernelGGL(build_extended_forest_kernel, dim3(T), dim3(WAVE), lds,
                     stream, bags, feat_sub, feat, value, right, count, ncount,
                     hidx, hw, off64, depth, leaf_lut, seed, tree_id_offset,
                     n, d, k, nnz, max_nodes, height_limit);
}

// tools/native/ifa_score only scores: it is built with IFA_NO_LARGE_BUILD and
// leaves these six instantiations out (binary size cap, as above the heap
// route below).
#ifndef IFA_NO_LARGE_BUILD
// threads: a multiple of 64, at most BL_MAX_THREADS
void launch_build_forest_large(RowDtype dt, const void* X, int64_t rs,
                               int64_t cs, const int64_t* bag_idx,
                               uint32_t* scratch, const int32_t* feat_sub,
                               int32_t* feat, float* value, int32_t* right,
                               int32_t* count, int32_t* ncount, int32_t* depth,
                               const float* leaf_lut, uint64_t seed,
                               int32_t tree_id_offset, int32_t T, int32_t n,
                               int32_t k, int32_t max_nodes,
                               int32_t height_limit, int threads, size_t lds,
                               hipStream_t stream) {
#define BL_LAUNCH(XT)                                                         \
  do {                                                                        \
    raise_lds((const void*)build_forest_large_kernel<XT>, lds);               \
    hipLaunchKernelGGL(build_forest_large_kernel<XT>, dim3(T), dim3(threads), \
                       lds, stream, (const XT*)X, rs, cs, bag_idx, scratch,   \
                       feat_sub, feat, value, right, count, ncount, depth,    \
                       leaf_lut, seed, tree_id_offset, n, k, max_nodes,       \
                       height_limit);                                         \
  } while (0)
  if (dt == ROW_BF16)
    BL_LAUNCH(uint16_t);
  else if (dt == ROW_F16)
    BL_LAUNCH(f16_t);
  else
    BL_LAUNCH(float);
#undef BL_LAUNCH
}

void launch_build_extended_forest_large(
    RowDtype dt, const void* X, int64_t rs, int64_t cs, const int64_t* bag_idx,
    uint32_t* scratch, const int32_t* feat_sub, int32_t* feat, float* value,
    int32_t* right, int32_t* count, int32_t* ncount, int32_t* hidx, float* hw,
    double* off64, int32_t* depth, const float* leaf_lut, uint64_t seed,
    int32_t tree_id_offset, int32_t T, int32_t n, int32_t k, int32_t nnz,
    int32_t max_nodes, int32_t height_limit, int threads, size_t lds,
    hipStream_t stream) {
#define BL_LAUNCH(XT)                                                         \
  do {                                                                        \
    raise_lds((const void*)build_extended_forest_large_kernel<XT>, lds);      \
    hipLaunchKernelGGL(build_extended_forest_large_kernel<XT>, dim3(T),       \
                       dim3(threads), lds, stream, (const XT*)X, rs, cs,      \
                       bag_idx, scratch, feat_sub, feat, value, right, count, \
                       ncount, hidx, hw, off64, depth, leaf_lut, seed,        \
                       tree_id_offset, n, k, nnz, max_nodes, height_limit);   \
  } while (0)
  if (dt == ROW_BF16)
    BL_LAUNCH(uint16_t);
  else if (dt == ROW_F16)
    BL_LAUNCH(f16_t);
  else
    BL_LAUNCH(float);
#undef BL_LAUNCH
}
#endif  // IFA_NO_LARGE_BUILD

void launch_v4_level_order(const void* nodes, const int32_t* ncount,
                           void* out, int32_t Tpad, int32_t max_nodes,
                           hipStream_t stream) {
  hipLaunchKernelGGL(v4_level_order_kernel, dim3(Tpad), dim3(WAVE),
                     (size_t)max_nodes * 2, stream, (const int2*)nodes, ncount,
                     (int2*)out, max_nodes);
}

void launch_v4_heap_order(const void* nodes, const int32_t* ncount,
                          void* out, int32_t Tpad, int32_t max_nodes,
                          int32_t height, int32_t slab_bytes,
                          hipStream_t stream) {
  hipLaunchKernelGGL(v4_heap_order_kernel, dim3(Tpad), dim3(WAVE),
                     (size_t)(2 << height) * 2, stream, (const int2*)nodes,
                     ncount, (uint32_t*)out, max_nodes, height, slab_bytes);
}

// 16-bit rows only (ROW_BF16 / ROW_F16); rpt 1 or 2; phase 4 or 8 trees;
// threads 256, or 512 with rpt 1.
// tools/native/ifa_score stays on the level-order route (bitwise the same
// scores) and is built with IFA_NO_HEAP_ROUTE: with these instantiations
// linked in, the binary passes the 2048 KB tools/lint_offline.py allows.
#ifndef IFA_NO_HEAP_ROUTE
namespace {
// the instantiation (dt, rpt, packed, phase, threads) names, as a host
// function pointer
const void* score_forest_heap_fn(RowDtype dt, int rpt, bool packed, int phase,
                                 int threads) {
#define HF2(KT, RPT, PK, PH, BT)                                              \
  ((const void*)score_forest_heap<KT, RPT, PK, PH, BT>)
#define HF1(KT, RPT, BT)                                                      \
  (packed ? (phase == 8 ? HF2(KT, RPT, true, 8, BT)                           \
                        : HF2(KT, RPT, true, 4, BT))                          \
          : (phase == 8 ? HF2(KT, RPT, false, 8, BT)                          \
                        : HF2(KT, RPT, false, 4, BT)))
#define HF(KT)                                                                \
  (threads == 512 ? HF1(KT, 1, 512)                                           \
                  : (rpt == 2 ? HF1(KT, 2, 256) : HF1(KT, 1, 256)))
  return dt == ROW_BF16 ? HF(uint16_t) : HF(f16_t);
#undef HF
#undef HF1
#undef HF2
}
}  // namespace

// blocks of `threads` threads with `lds` bytes each that one CU keeps
// resident for this instantiation (registers, LDS and wave slots together),
// as the runtime reports it; 0 where it cannot say
int score_forest_heap_resident(RowDtype dt, int rpt, bool packed, int phase,
                               int threads, size_t lds) {
  const void* fn = score_forest_heap_fn(dt, rpt, packed, phase, threads);
  raise_lds(fn, lds);
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, lds) !=
      hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

// returns the launch's status for the caller to check
hipError_t launch_score_forest_heap(RowDtype dt, int rpt, int phase,
                                    int threads, const void* X,
                                    const void* heap, float* out, int64_t N,
                                    int32_t d, int64_t rs, int64_t cs,
                                    int32_t Tpad, int32_t height, float fT,
                                    float c_norm, int finalize, size_t lds,
                                    int blocks, hipStream_t stream) {
  const bool packed = rs == d && cs == 1;
  const void* fn = score_forest_heap_fn(dt, rpt, packed, phase, threads);
  raise_lds(fn, lds);
  // every instantiation has this signature but for the row pointer's type
  const uint32_t* hp = (const uint32_t*)heap;
  void* args[] = {&X, &hp, &out, &N, &d, &Tpad, &height, &fT, &c_norm,
                  &finalize, &rs, &cs};
  return hipLaunchKernel(fn, dim3(blocks), dim3(threads), args, lds, stream);
}
#endif  // IFA_NO_HEAP_ROUTE

void launch_score_forest(RowDtype dt, int rpt, bool rows_lds, bool nodes_lds,
                         int ilp, const void* X, const void* nodes,
                         const int32_t* ncount, float* out, int64_t N,
                         int32_t d, int64_t rs, int64_t cs, int32_t Tpad,
                         int32_t max_nodes, int32_t height_limit, float fT,
                         float c_norm, int finalize, size_t lds, int blocks,
                         hipStream_t stream) {
  // packed rows take the packed entry point where one exists: rows and
  // nodes staged in LDS at ILP 4. The global-X walk, the deep-forest node
  // walk and the other ILPs have one entry point for every layout.
  const bool packed = rs == d && cs == 1;
#define LS1(KT, RPT, RL, TI, NL)                                              \
  do {                                                                        \
    raise_lds((const void*)score_forest_v4<KT, RPT, RL, TI, NL>, lds);        \
    hipLaunchKernelGGL((score_forest_v4<KT, RPT, RL, TI, NL>), dim3(blocks),  \
                       dim3(256), lds, stream, (const KT*)X,                  \
                       (const int2*)nodes, ncount, out, N, d, Tpad,           \
                       max_nodes, height_limit, fT, c_norm, finalize, rs,     \
                       cs);                                                   \
  } while (0)
#define LS1P(KT, RPT)                                                         \
  do {                                                                        \
    raise_lds((const void*)score_forest_v4_packed<KT, RPT, 4>, lds);          \
    hipLaunchKernelGGL((score_forest_v4_packed<KT, RPT, 4>), dim3(blocks),    \
                       dim3(256), lds, stream, (const KT*)X,                  \
                       (const int2*)nodes, ncount, out, N, d, Tpad,           \
                       max_nodes, height_limit, fT, c_norm, finalize);        \
  } while (0)
#define LS(KT, RPT, RL, TI)                                                   \
  do {                                                                        \
    if (nodes_lds && packed && RL && TI == 4) LS1P(KT, RPT);                  \
    else if (nodes_lds) LS1(KT, RPT, RL, TI, true);                           \
    else LS1(KT, RPT, RL, TI, false);                                         \
  } while (0)
#define LS_ILP(KT, RPT, RL)                                                   \
  do {                                                                        \
    if (ilp == 8) LS(KT, RPT, RL, 8);                                         \
    else if (ilp == 2) LS(KT, RPT, RL, 2);                                    \
    else LS(KT, RPT, RL, 4);                                                  \
  } while (0)
  if (dt == ROW_BF16) {
    if (rows_lds && rpt == 2) LS_ILP(uint16_t, 2, true);
    else if (rows_lds) LS_ILP(uint16_t, 1, true);
    else LS_ILP(uint16_t, 1, false);
  } else if (dt == ROW_F16) {
    if (rows_lds && rpt == 2) LS_ILP(f16_t, 2, true);
    else if (rows_lds) LS_ILP(f16_t, 1, true);
    else LS_ILP(f16_t, 1, false);
  } else {
    if (rows_lds && rpt == 2) LS_ILP(uint32_t, 2, true);
    else if (rows_lds) LS_ILP(uint32_t, 1, true);
    else LS_ILP(uint32_t, 1, false);
  }
#undef LS_ILP
#undef LS
#undef LS1P
#undef LS1
}

void launch_score_extended_dense(RowDtype dt, bool rows_lds, bool wlds,
                                 const void* X, const void* nodes,
                                 const float* hw, const int32_t* ncount,
                                 float* out, int64_t N, int32_t d, int64_t rs,
                                 int64_t cs, int32_t dpad, int32_t T,
                                 int32_t max_nodes, float fT, float c_norm,
                                 int finalize, size_t lds, int blocks,
                                 hipStream_t stream) {
#define LSD(XT, RL, WL)                                                       \
  do {                                                                        \
    raise_lds((const void*)score_extended_dense_kernel<XT, RL, WL>, lds);     \
    hipLaunchKernelGGL((score_extended_dense_kernel<XT, RL, WL>),             \
                       dim3(blocks), dim3(256), lds, stream, (const XT*)X,    \
                       (const int2*)nodes, hw, ncount, out, N, d, rs, cs,     \
                       dpad, T,                                               \
                       max_nodes, fT, c_norm, finalize);                      \
  } while (0)
  if (dt == ROW_BF16) {
    if (rows_lds && wlds) LSD(uint16_t, true, true);
    else if (rows_lds) LSD(uint16_t, true, false);
    else if (wlds) LSD(uint16_t, false, true);
    else LSD(uint16_t, false, false);
  } else if (dt == ROW_F16) {
    if (rows_lds && wlds) LSD(f16_t, true, true);
    else if (rows_lds) LSD(f16_t, true, false);
    else if (wlds) LSD(f16_t, false, true);
    else LSD(f16_t, false, false);
  } else {
    if (rows_lds && wlds) LSD(float, true, true);
    else if (rows_lds) LSD(float, true, false);
    else if (wlds) LSD(float, false, true);
    else LSD(float, false, false);
  }
#undef LSD
}

void launch_score_extended_dense_v2(RowDtype dt, int D, const void* X,
                                    const void* nodes, const float* values,
                                    const float* hw, const int32_t* ncount,
                                    float* out, int64_t N, int32_t d,
                                    int64_t rs, int64_t cs,
                                    int32_t T, int32_t max_nodes,
                                    int32_t height_limit, float fT,
                                    float c_norm, int finalize, size_t lds,
                                    int blocks, hipStream_t stream) {
#define LSD2(KT, DD, RR)                                                      \
  do {                                                                        \
    raise_lds((const void*)score_extended_dense_v2<KT, DD, RR>, lds);         \
    hipLaunchKernelGGL((score_extended_dense_v2<KT, DD, RR>), dim3(blocks),   \
                       dim3(EIFD_THREADS), lds, stream, (const KT*)X,         \
                       (const int2*)nodes, values, hw, ncount, out, N, d,     \
                       rs, cs, T,                                             \
                       max_nodes, height_limit, fT, c_norm, finalize);        \
  } while (0)
  // D=32 runs RPT=1: 2 rows/thread would spill past the 128-VGPR budget
  // that keeps 4 waves/SIMD resident (2 blocks/CU at ~80 KB LDS each)
  if (dt == ROW_BF16) {
    if (D == 8) LSD2(uint16_t, 8, 2);
    else if (D == 16) LSD2(uint16_t, 16, 2);
    else if (D == 64) LSD2(uint16_t, 64, 1);
    else LSD2(uint16_t, 32, 1);
  } else if (dt == ROW_F16) {
    if (D == 8) LSD2(f16_t, 8, 2);
    else if (D == 16) LSD2(f16_t, 16, 2);
    else if (D == 64) LSD2(f16_t, 64, 1);
    else LSD2(f16_t, 32, 1);
  } else {
    if (D == 8) LSD2(uint32_t, 8, 2);
    else if (D == 16) LSD2(uint32_t, 16, 2);
    else if (D == 64) LSD2(uint32_t, 64, 1);
    else LSD2(uint32_t, 32, 1);
  }
#undef LSD2
}

void launch_score_forest_wide(RowDtype dt, const void* X, const void* nodes,
                              float* out, int64_t N, int32_t d, int64_t rs,
                              int64_t cs, int32_t T,
                              int64_t max_nodes, int32_t height_limit,
                              float fT, float c_norm, int finalize,
                              int blocks, hipStream_t stream) {
  if (dt == ROW_BF16)
    hipLaunchKernelGGL((score_forest_wide<uint16_t>), dim3(blocks), dim3(256),
                       0, stream, (const uint16_t*)X, (const int4*)nodes, out,
                       N, d, rs, cs, T, max_nodes, height_limit, fT, c_norm,
                       finalize);
  else if (dt == ROW_F16)
    hipLaunchKernelGGL((score_forest_wide<f16_t>), dim3(blocks), dim3(256),
                       0, stream, (const f16_t*)X, (const int4*)nodes, out,
                       N, d, rs, cs, T, max_nodes, height_limit, fT, c_norm,
                       finalize);
  else
    hipLaunchKernelGGL((score_forest_wide<uint32_t>), dim3(blocks), dim3(256),
                       0, stream, (const uint32_t*)X, (const int4*)nodes, out,
                       N, d, rs, cs, T, max_nodes, height_limit, fT, c_norm,
                       finalize);
}

void launch_score_extended_wide(RowDtype dt, const void* X, const void* nodes,
                                const int32_t* hidx, const float* hw,
                                float* out, int64_t N, int32_t d, int64_t rs,
                                int64_t cs, int32_t T,
                                int64_t max_nodes, int32_t nnz, float fT,
                                float c_norm, int finalize, int blocks,
                                hipStream_t stream) {
  if (dt == ROW_BF16)
    hipLaunchKernelGGL((score_extended_wide<uint16_t>), dim3(blocks),
                       dim3(256), 0, stream, (const uint16_t*)X,
                       (const int4*)nodes, hidx, hw, out, N, d, rs, cs, T,
                       max_nodes, nnz, fT, c_norm, finalize);
  else if (dt == ROW_F16)
    hipLaunchKernelGGL((score_extended_wide<f16_t>), dim3(blocks),
                       dim3(256), 0, stream, (const f16_t*)X,
                       (const int4*)nodes, hidx, hw, out, N, d, rs, cs, T,
                       max_nodes, nnz, fT, c_norm, finalize);
  else
    hipLaunchKernelGGL((score_extended_wide<float>), dim3(blocks), dim3(256),
                       0, stream, (const float*)X, (const int4*)nodes, hidx,
                       hw, out, N, d, rs, cs, T, max_nodes, nnz, fT, c_norm,
                       finalize);
}

void launch_score_extended_dense_v3(int D, bool rpt2, const void* X,
                                    const void* nodes, const float* values,
                                    const uint32_t* hwp,
                                    const int32_t* ncount, float* out,
                                    int64_t N, int32_t d, int64_t rs,
                                    int64_t cs, int32_t T,
                                    int32_t max_nodes, int32_t height_limit,
                                    float fT, float c_norm, int finalize,
                                    size_t lds, int blocks,
                                    hipStream_t stream) {
#define LSD3(DD, RR)                                                          \
  do {                                                                        \
    raise_lds((const void*)score_extended_dense_v3<DD, RR>, lds);             \
    hipLaunchKernelGGL((score_extended_dense_v3<DD, RR>), dim3(blocks),       \
                       dim3(EIFD_THREADS), lds, stream, (const uint16_t*)X,   \
                       (const int2*)nodes, values, hwp, ncount, out, N, d,    \
                       rs, cs, T,                                             \
                       max_nodes, height_limit, fT, c_norm, finalize);        \
  } while (0)
  if (D == 8) LSD3(8, 2);
  else if (D == 16) LSD3(16, 2);
  else if (D == 32 && rpt2) LSD3(32, 2);  // A/B: halved staging amortization
  else if (D == 32) LSD3(32, 1);
  else if (D == 64) LSD3(64, 1);
  else LSD3(128, 1);
#undef LSD3
}

void launch_score_extended_dense_nonfinite_rows(
    RowDtype dt, bool packed_w, const void* X, const void* nodes,
    const float* values, const void* wts, float* out, int64_t N, int32_t d,
    int64_t rs, int64_t cs,
    int32_t D, int32_t T, int32_t max_nodes, int32_t height_limit, float fT,
    float c_norm, int finalize, int blocks, hipStream_t stream) {
#define LNF(KT, PW)                                                           \
  hipLaunchKernelGGL((score_extended_dense_nonfinite_rows<KT, PW>),           \
                     dim3(blocks), dim3(256), 0, stream, (const KT*)X,        \
                     (const int2*)nodes, values, wts, out, N, d, rs, cs, D,   \
                     T,                                                       \
                     max_nodes, height_limit, fT, c_norm, finalize)
  // v3 (packed weights) takes bf16 rows only
  if (dt == ROW_BF16) {
    if (packed_w) LNF(uint16_t, true); else LNF(uint16_t, false);
  } else if (dt == ROW_F16) {
    LNF(f16_t, false);
  } else {
    LNF(uint32_t, false);
  }
#undef LNF
}

void launch_score_extended_sparse_v2(RowDtype dt, int nnz, const void* X,
                                     const void* nodes, const float* values,
                                     const int32_t* hidx, const float* hw,
                                     const int32_t* ncount, float* out,
                                     int64_t N, int32_t d, int64_t rs,
                                     int64_t cs, int32_t dpad,
                                     int32_t T, int32_t max_nodes,
                                     int32_t height_limit, float fT,
                                     float c_norm, int finalize, size_t lds,
                                     int blocks, hipStream_t stream) {
#define LSS2(KT, NZ)                                                          \
  do {                                                                        \
    raise_lds((const void*)score_extended_sparse_v2<KT, NZ, 2>, lds);         \
    hipLaunchKernelGGL((score_extended_sparse_v2<KT, NZ, 2>), dim3(blocks),   \
                       dim3(256), lds, stream, (const KT*)X,                  \
                       (const int2*)nodes, values, hidx, hw, ncount, out, N,  \
                       d, rs, cs, dpad, T, max_nodes, height_limit, fT,       \
                       c_norm, finalize);                                     \
  } while (0)
#define LSS2_ALL(KT)                                                          \
  do {                                                                        \
    switch (nnz) {                                                            \
      case 1: LSS2(KT, 1); break;                                             \
      case 2: LSS2(KT, 2); break;                                             \
      case 3: LSS2(KT, 3); break;                                             \
      case 4: LSS2(KT, 4); break;                                             \
      default: LSS2(KT, 5); break;                                            \
    }                                                                         \
  } while (0)
  if (dt == ROW_BF16) LSS2_ALL(uint16_t);
  else if (dt == ROW_F16) LSS2_ALL(f16_t);
  else LSS2_ALL(uint32_t);
#undef LSS2_ALL
#undef LSS2
}

void launch_score_extended_forest(RowDtype dt, bool rows_lds, bool hyper_lds,
                                  bool nodes_lds, const void* X,
                                  const void* nodes, const int32_t* hidx,
                                  const float* hw, const int32_t* ncount,
                                  float* out, int64_t N, int32_t d, int64_t rs,
                                  int64_t cs, int32_t T,
                                  int32_t max_nodes, int32_t nnz, float fT,
                                  float c_norm, int finalize, size_t lds,
                                  int blocks, hipStream_t stream) {
#define LSE(XT, RL, HL)                                                       \
  do {                                                                        \
    if (nodes_lds) {                                                          \
      raise_lds((const void*)score_extended_forest_kernel<XT, RL, HL, true>,  \
                lds);                                                         \
      hipLaunchKernelGGL((score_extended_forest_kernel<XT, RL, HL, true>),    \
                         dim3(blocks), dim3(256), lds, stream, (const XT*)X,  \
                         (const int2*)nodes, hidx, hw, ncount, out, N, d,     \
                         rs, cs, T,                                           \
                         max_nodes, nnz, fT, c_norm, finalize);               \
    } else {                                                                  \
      raise_lds((const void*)score_extended_forest_kernel<XT, RL, HL,         \
      false>,                                                                 \
                lds);                                                         \
      hipLaunchKernelGGL((score_extended_forest_kernel<XT, RL, HL, false>),   \
                         dim3(blocks), dim3(256), lds, stream, (const XT*)X,  \
                         (const int2*)nodes, hidx, hw, ncount, out, N, d,     \
                         rs, cs, T,                                           \
                         max_nodes, nnz, fT, c_norm, finalize);               \
    }                                                                         \
  } while (0)
  if (dt == ROW_BF16) {
    if (rows_lds && hyper_lds) LSE(uint16_t, true, true);
    else if (rows_lds) LSE(uint16_t, true, false);
    else if (hyper_lds) LSE(uint16_t, false, true);
    else LSE(uint16_t, false, false);
  } else if (dt == ROW_F16) {
    if (rows_lds && hyper_lds) LSE(f16_t, true, true);
    else if (rows_lds) LSE(f16_t, true, false);
    else if (hyper_lds) LSE(f16_t, false, true);
    else LSE(f16_t, false, false);
  } else {
    if (rows_lds && hyper_lds) LSE(float, true, true);
    else if (rows_lds) LSE(float, true, false);
    else if (hyper_lds) LSE(float, false, true);
    else LSE(float, false, false);
  }
#undef LSE
}

// mode: 0 = accumulators + rows in LDS (rpt 1 or 2), 1 = global
// accumulators with rows in LDS, 2 = global accumulators and global rows
void launch_explain_forest(RowDtype dt, int mode, int rpt, bool nodes_lds,
                           const void* X, const void* nodes,
                           const int32_t* ncount, float* out, int64_t N,
                           int32_t d, int64_t rs, int64_t cs, int32_t dpad,
                           int32_t astride, int32_t T, int32_t max_nodes,
                           int32_t tps, int32_t height_limit, float fT,
                           int finalize, size_t lds, int blocks,
                           hipStream_t stream) {
  // packed rows take the PACKED instantiation of mode 0 with staged nodes
  const bool packed = rs == d && cs == 1;
#define LX1(KT, RPT, AL, RL, NL, PK)                                          \
  do {                                                                        \
    raise_lds((const void*)explain_forest_kernel<KT, RPT, AL, RL, NL, PK>,    \
              lds);                                                           \
    hipLaunchKernelGGL((explain_forest_kernel<KT, RPT, AL, RL, NL, PK>),      \
                       dim3(blocks), dim3(256), lds, stream, (const KT*)X,    \
                       (const int4*)nodes, ncount, out, N, d, dpad, astride,  \
                       T, max_nodes, tps, height_limit, fT, finalize, rs,     \
                       cs);                                                   \
  } while (0)
#define LX(KT, RPT, AL, RL, NL)                                               \
  do {                                                                        \
    if (packed) LX1(KT, RPT, AL, RL, NL, (AL && RL && NL));                   \
    else LX1(KT, RPT, AL, RL, NL, false);                                     \
  } while (0)
#define LX_MODE(KT, NL)                                                       \
  do {                                                                        \
    if (mode == 0 && rpt == 2) LX(KT, 2, true, true, NL);                     \
    else if (mode == 0) LX(KT, 1, true, true, NL);                            \
    else if (mode == 1) LX(KT, 1, false, true, NL);                           \
    else LX(KT, 1, false, false, NL);                                         \
  } while (0)
  if (dt == ROW_BF16) {
    if (nodes_lds) LX_MODE(uint16_t, true); else LX_MODE(uint16_t, false);
  } else if (dt == ROW_F16) {
    if (nodes_lds) LX_MODE(f16_t, true); else LX_MODE(f16_t, false);
  } else {
    if (nodes_lds) LX_MODE(uint32_t, true); else LX_MODE(uint32_t, false);
  }
#undef LX_MODE
#undef LX
#undef LX1
}

void launch_explain_extended(RowDtype dt, const void* X, const void* nodes,
                             const int32_t* hidx, const float* hw,
                             const float* dl, const float* dr, float* out,
                             int64_t N, int32_t d, int64_t rs, int64_t cs,
                             int32_t T, int32_t max_nodes, int32_t nnz,
                             float fT, int finalize, int blocks,
                             hipStream_t stream) {
  if (dt == ROW_BF16)
    hipLaunchKernelGGL((explain_extended_kernel<uint16_t>), dim3(blocks),
                       dim3(256), 0, stream, (const uint16_t*)X,
                       (const int2*)nodes, hidx, hw, dl, dr, out, N, d, rs, cs,
                       T, max_nodes, nnz, fT, finalize);
  else if (dt == ROW_F16)
    hipLaunchKernelGGL((explain_extended_kernel<f16_t>), dim3(blocks),
                       dim3(256), 0, stream, (const f16_t*)X,
                       (const int2*)nodes, hidx, hw, dl, dr, out, N, d, rs, cs,
                       T, max_nodes, nnz, fT, finalize);
  else
    hipLaunchKernelGGL((explain_extended_kernel<float>), dim3(blocks),
                       dim3(256), 0, stream, (const float*)X,
                       (const int2*)nodes, hidx, hw, dl, dr, out, N, d, rs, cs,
                       T, max_nodes, nnz, fT, finalize);
}

}  // namespace ifa
