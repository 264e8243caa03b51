// MI355X (gfx950, CDNA4) standard scoring for forests past the 15-bit node
// ids of the v4 and heap records (every maxSamples > 16384): compact
// level-order records, the top of each tree walked from LDS and the rest
// from L2 (docs/DESIGN.md §3b). BITWISE equal to cpu_engine.path_lengths,
// like every standard walk: integer-key compares, tree-order f32 sum.
//
// Records ("deep" pack), int2 [Tpad][M], M = the largest node_count (even):
//   x = feat | link << 12   12-bit feature id, 20-bit link
//   y = key threshold of the row kind (internal) / f32 bits of depth + c(m)
// in LEVEL order with the two children of a node adjacent: link is the right
// child's index, the left child is link - 1, one step is
//   cur = link - (key < thr).
// A leaf has link = its own index and feat = d, the sentinel slab of the key
// tile (all-ones keys), so it compares false and rests where it is. Pad trees
// (Tpad is a multiple of the phase) are single leaves of value +0.0. The
// first S records of a tree are its top levels; lds_levels[t] counts the
// leading levels that lie wholly inside them and hold an internal node.
//
// deep_level_order_kernel turns trimmed pre-order arrays into these records:
// one block per tree, level by level. A block-wide prefix sum over "has
// children" hands every node of a level the slots of its two children in the
// next one; the old indices of a level (the frontier) ping-pong between two
// global scratch rows, so a tree of any size is reordered, not only one that
// fits in LDS.
//
// score_forest_deep: a block of 256 threads owns a tile of RPT * 256 rows,
// keyed into the feature-major LDS tile of the v4 walk. PH trees per barrier
// phase: the first S records of each are copied into LDS, then every thread
// walks its RPT * PH chains
//   phase A  a fixed number of trips that read only LDS (no flags, no votes;
//            a chain at a leaf self-loops), reads batched as in v4;
//   phase B  the remaining levels. A chain is finished once it has read a
//            record whose link is its own index; finished chains load
//            nothing, live ones read their 8-byte record from global memory
//            (L2: all blocks walk the trees in the same order), all loads of
//            a trip before any use. A wave leaves the loop when none of its
//            lanes has a live chain. The record that finishes a chain is its
//            leaf, whose y is the value to add.
//
// This TU is torch-free and stands alone, like shap_kernels.hip: the key
// helpers it shares with forest_kernels.hip are duplicated (namespace
// ifa::deep) so that the other TU, and the native scorer that links only it,
// do not change.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "row_dtype.h"

namespace ifa {
namespace deep {

#define DEEP_BT 256
#define DEEP_WAVE 64

// IEEE fp16 bits as a type of their own; uint16_t means bf16 bits
enum class f16_t : uint16_t {};

__device__ __forceinline__ uint32_t key16(uint32_t b) {
  const uint32_t m = b & 0x7FFFu;
  uint32_t k = (b & 0x8000u) ? (0x7FFFu - m) : (0x8000u + m);
  if (m == 0) k = 0x8000u;
  if (m > 0x7F80u) k = 0xFFFFu;
  return k;
}
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

// 16-bit keys sit in the high half with the low bits saturated: the sentinel
// widens to 0xFFFFFFFF and compares false against every y, leaf values too
__device__ __forceinline__ uint32_t widen_key(uint16_t k) {
  return ((uint32_t)k << 16) | 0xFFFFu;
}
__device__ __forceinline__ uint32_t widen_key(f16_t k) {
  return widen_key((uint16_t)k);
}
__device__ __forceinline__ uint32_t widen_key(uint32_t k) { return k; }

template <typename KT>
__device__ __forceinline__ KT key_sentinel() { return (KT)~(KT)0; }
template <>
__device__ __forceinline__ f16_t key_sentinel<f16_t>() {
  return (f16_t)0xFFFFu;
}

__device__ __forceinline__ int rec_feat(int x) { return x & 0xFFF; }
__device__ __forceinline__ int rec_link(int x) {
  return (int)((uint32_t)x >> 12);
}
__device__ __forceinline__ int2 leaf_rec(int d, int i, int y) {
  return make_int2(d | (i << 12), y);
}

// The level-order kernel writes either record type. The int4 ("explain
// deep") record carries two more payload words, the f32 bits of the edge
// deltas; its leaves hold threshold 0 and +0.0 twice whatever w says.
__device__ __forceinline__ void put_node(int2* dst, int i, int x, int y, int,
                                         int) {
  dst[i] = make_int2(x, y);
}
__device__ __forceinline__ void put_node(int4* dst, int i, int x, int y, int z,
                                         int w) {
  dst[i] = make_int4(x, y, z, w);
}
__device__ __forceinline__ void put_leaf(int2* dst, int d, int i, int y) {
  dst[i] = leaf_rec(d, i, y);
}
__device__ __forceinline__ void put_leaf(int4* dst, int d, int i, int) {
  dst[i] = make_int4(d | (i << 12), 0, 0, 0);
}

extern __shared__ __align__(16) unsigned char smem[];

// ---------------------------------------------------------------------------
// pre-order -> level order, one block per tree
// ---------------------------------------------------------------------------
template <typename REC>
__global__ void __launch_bounds__(DEEP_BT) deep_level_order_kernel(
    const int32_t* __restrict__ feat,   // [T][M0] feature id, < 0: leaf
    const int32_t* __restrict__ right,  // [T][M0] pre-order right child
    const int32_t* __restrict__ w,      // [T][M0] key threshold / leaf value
    const int32_t* __restrict__ pz,     // [T][M0] int4 records: delta_left
    const int32_t* __restrict__ pw,     // [T][M0] and delta_right bits
    const int32_t* __restrict__ ncnt,   // [T]
    uint32_t* __restrict__ front_a,     // [T][M0] scratch: a level's old ids
    uint32_t* __restrict__ front_b,     // [T][M0]
    REC* __restrict__ out,              // [Tpad][M]
    int32_t* __restrict__ lds_levels,   // [Tpad]
    int32_t T, int32_t M0, int32_t M, int32_t S, int32_t d) {
  __shared__ int wsum[DEEP_BT / DEEP_WAVE];
  const int t = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (DEEP_WAVE - 1), wave = tid / DEEP_WAVE;
  constexpr bool kPayload = sizeof(REC) == 16;
  REC* dst = out + (int64_t)t * M;
  if (t >= T) {  // pad tree: a single leaf of value +0.0
    for (int i = tid; i < M; i += DEEP_BT) put_leaf(dst, d, i, 0);
    if (tid == 0) lds_levels[t] = 0;
    return;
  }
  const int32_t* sf = feat + (int64_t)t * M0;
  const int32_t* sr = right + (int64_t)t * M0;
  const int32_t* sw = w + (int64_t)t * M0;
  uint32_t* cur = front_a + (int64_t)t * M0;
  uint32_t* nxt = front_b + (int64_t)t * M0;
  const int n = min(max(ncnt[t], 1), M0);
  for (int i = n + tid; i < M; i += DEEP_BT) put_leaf(dst, d, i, 0);
  if (tid == 0) cur[0] = 0;
  __syncthreads();

  int begin = 0, end = 1;  // the current level, in new indices
  int levels = 0;
  while (begin < end) {
    int tail = end;  // next free new index (block-uniform)
    int level_internal = 0;
    for (int base = begin; base < end; base += DEEP_BT) {
      const int i = base + tid;
      int old = 0, f = -1, r = 0, wv = 0, zv = 0, yv = 0;
      bool internal = false;
      if (i < end) {
        old = min((int)cur[i - begin], n - 1);
        f = sf[old];
        r = sr[old];
        wv = sw[old];
        if (kPayload) {
          zv = pz[(int64_t)t * M0 + old];
          yv = pw[(int64_t)t * M0 + old];
        }
        // children outside the tree (a malformed record) are not followed,
        // so every index stays below n
        internal = f >= 0 && r > old + 1 && r < n;
      }
      const uint64_t m = __ballot(internal);
      if (lane == 0) wsum[wave] = __popcll(m);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int k = 0; k < DEEP_BT / DEEP_WAVE; ++k) {
        const int c = wsum[k];
        if (k < wave) before += c;
        total += c;
      }
      __syncthreads();  // wsum is written again by the next chunk
      int link = i;
      if (internal) {
        const int l =
            tail + 2 * (before + __popcll(m & ((1ull << lane) - 1ull)));
        if (l + 1 < n) {
          nxt[l - end] = (uint32_t)(old + 1);
          nxt[l + 1 - end] = (uint32_t)r;
          link = l + 1;
        }
      }
      if (i < end) {
        if (link != i)
          put_node(dst, i, f | (link << 12), wv, zv, yv);
        else
          put_leaf(dst, d, i, wv);
      }
      tail = min(tail + 2 * total, n);
      level_internal += total;
    }
    __syncthreads();  // the next level's frontier is written
    if (end <= S && level_internal > 0) ++levels;
    begin = end;
    end = tail;
    uint32_t* sw2 = cur;
    cur = nxt;
    nxt = sw2;
  }
  // nodes no link reaches (never in a built tree): self-loops, so that every
  // record of the output is defined and in bounds
  for (int i = end + tid; i < n; i += DEEP_BT) put_leaf(dst, d, i, 0);
  if (tid == 0) lds_levels[t] = levels;
}

// ---------------------------------------------------------------------------
// scoring
// ---------------------------------------------------------------------------

// element offset of block row j inside one slab of the key tile (the v4
// tile: forest_kernels.hip, v4_tile_slot)
template <typename KT, int RPT>
__device__ __forceinline__ int tile_slot(int j) {
  if (sizeof(KT) == 4) return j;
  constexpr int P = RPT * 128;
  return (j % P) * 2 + j / P;
}

// every thread keys its own rows into the tile; barriers are the caller's.
// !KEYS (the extended walk): the raw bits are stored, rows past N are +0.0
// and there is no sentinel slab.
template <typename KT, int RPT, bool KEYS = true>
__device__ __forceinline__ void stage_tile(KT* rows, const KT* __restrict__ X,
                                           int64_t block_row0, int rows_here,
                                           int32_t d, int64_t rs, int64_t cs) {
  constexpr int FS = RPT * DEEP_BT;
  constexpr int EPV = 16 / (int)sizeof(KT);
  const int tid = threadIdx.x;
  const bool vec = cs == 1 && d % EPV == 0 && rs % EPV == 0 &&
                   ((uintptr_t)X & 15) == 0;
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int j = tid + r * DEEP_BT;
    KT* dst = rows + tile_slot<KT, RPT>(j);
    if (j < rows_here) {
      const KT* src = X + (block_row0 + j) * rs;
      if (vec) {
        for (int c = 0; c < d; c += EPV) {
          union { uint4 v; KT e[EPV]; } pc;
          pc.v = *(const uint4*)(src + c);
#pragma unroll
          for (int k = 0; k < EPV; ++k)
            dst[(c + k) * FS] = KEYS ? key_of_bits<KT>(pc.e[k]) : pc.e[k];
        }
      } else {
        for (int c = 0; c < d; ++c, src += cs)
          dst[c * FS] = KEYS ? key_of_bits<KT>(*src) : *src;
      }
    } else {
      // tail block: rows past N are walked but never stored
      for (int c = 0; c < d; ++c)
        dst[c * FS] = KEYS ? key_sentinel<KT>() : (KT)0;
    }
    if (KEYS) dst[d * FS] = key_sentinel<KT>();  // leaf sentinel slab
  }
}

template <typename KT, int RPT, int PH>
__global__ void __launch_bounds__(DEEP_BT) score_forest_deep_kernel(
    const KT* __restrict__ X,               // raw bf16/fp16/f32 bits
    const int2* __restrict__ nodes,         // [Tpad][M] deep records
    const int32_t* __restrict__ lds_levels, // [Tpad]
    float* __restrict__ out,                // [N] (path sum or score)
    int64_t N, int32_t d, int32_t Tpad, int32_t M, int32_t S, int32_t height,
    float fT, float c_norm, int32_t finalize, int64_t rs, int64_t cs) {
  constexpr int FS = RPT * DEEP_BT;
  constexpr int rows_per_iter = RPT * DEEP_BT;
  const int tid = threadIdx.x;
  const int staged = min(S, M);  // records of a tree that the stage holds

  int2* tlds = (int2*)smem;  // [PH][S]
  KT* rows = (KT*)(tlds + PH * S);

  for (int64_t block_row0 = (int64_t)blockIdx.x * rows_per_iter;
       block_row0 < N; block_row0 += (int64_t)gridDim.x * rows_per_iter) {
    const int rows_here = (int)min((int64_t)rows_per_iter, N - block_row0);

    __syncthreads();  // previous tile's readers done
    stage_tile<KT, RPT>(rows, X, block_row0, rows_here, d, rs, cs);
    // the first phase's barriers order these stores before the walk

    const KT* rb[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r)
      rb[r] = rows + tile_slot<KT, RPT>(tid + r * DEEP_BT);

    float psum[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) psum[r] = 0.f;

    for (int t = 0; t < Tpad; t += PH) {
      __syncthreads();  // previous phase's LDS readers done
      // M is even, so a tree starts on 16 bytes: two records per copy
#pragma unroll
      for (int s = 0; s < PH; ++s) {
        const uint4* src = (const uint4*)(nodes + (int64_t)(t + s) * M);
        uint4* dst = (uint4*)(tlds + s * S);
        for (int i = tid; i < staged / 2; i += DEEP_BT) dst[i] = src[i];
      }
      // trips that stay inside every tree's stage. 0 levels means the root
      // is a leaf, which rests at record 0 for any number of trips.
      int la = height;
#pragma unroll
      for (int s = 0; s < PH; ++s) {
        const int l = lds_levels[t + s];
        if (l > 0) la = min(la, l);
      }
      __syncthreads();

      const int2* nbase[PH];
#pragma unroll
      for (int s = 0; s < PH; ++s) nbase[s] = nodes + (int64_t)(t + s) * M;

      int cur[RPT][PH];
#pragma unroll
      for (int r = 0; r < RPT; ++r)
#pragma unroll
        for (int s = 0; s < PH; ++s) cur[r][s] = 0;

      // ---- phase A: one level of all chains, LDS only --------------------
      auto visit = [&]() __attribute__((always_inline)) {
        int2 nd[RPT][PH];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int s = 0; s < PH; ++s) nd[r][s] = tlds[s * S + cur[r][s]];
        KT kraw[RPT][PH];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int s = 0; s < PH; ++s)
            kraw[r][s] = rb[r][rec_feat(nd[r][s].x) * FS];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int s = 0; s < PH; ++s)
            cur[r][s] = rec_link(nd[r][s].x) -
                        (widen_key(kraw[r][s]) < (uint32_t)nd[r][s].y);
      };
      int it = 0;
      for (; it + 2 <= la; it += 2) {
        visit();
        visit();
      }
      if (it < la) visit();

      // ---- phase B: the tail ---------------------------------------------
      // bit r * PH + s of `live`: the chain has not read its leaf yet
      uint32_t live = (1u << (RPT * PH)) - 1u;
      int val[RPT][PH];
      // `first`: the level after the staged ones straddles the stage's end,
      // and a chain that rested at a leaf in phase A sits inside it: records
      // below S come from LDS on this trip
      auto tail_trip = [&](auto first) __attribute__((always_inline)) {
        int2 nd[RPT][PH];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int s = 0; s < PH; ++s)
            if (live & (1u << (r * PH + s))) {
              if (decltype(first)::value && cur[r][s] < S)
                nd[r][s] = tlds[s * S + cur[r][s]];
              else
                nd[r][s] = nbase[s][cur[r][s]];
            }
        KT kraw[RPT][PH];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int s = 0; s < PH; ++s)
            if (live & (1u << (r * PH + s)))
              kraw[r][s] = rb[r][rec_feat(nd[r][s].x) * FS];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
          for (int s = 0; s < PH; ++s)
            if (live & (1u << (r * PH + s))) {
              const int link = rec_link(nd[r][s].x);
              val[r][s] = nd[r][s].y;
              if (link == cur[r][s])
                live &= ~(1u << (r * PH + s));
              else
                cur[r][s] = link - (widen_key(kraw[r][s]) <
                                    (uint32_t)nd[r][s].y);
            }
      };
      tail_trip(std::true_type{});
      // a chain at depth `height` is a leaf: height - la more trips read it
      for (int k = la; k < height && __any(live != 0); ++k)
        tail_trip(std::false_type{});

#pragma unroll
      for (int r = 0; r < RPT; ++r)
#pragma unroll
        for (int s = 0; s < PH; ++s)
          psum[r] = __fadd_rn(psum[r], __int_as_float(val[r][s]));
    }

#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t my_row = block_row0 + tid + r * DEEP_BT;
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
// attribution (docs/DESIGN.md §8): the deep walk with the taken edge's f32
// delta added to acc[row][feat] along the path. BITWISE equal to
// cpu_engine.feature_contributions, so a row's adds keep one order: trees
// 0..T-1, root to leaf. A thread therefore walks the trees of a phase
// strictly one after another and takes its independent chains from its RPT
// rows (and the other resident waves), never from several trees of a row.
//
// Records ("explain deep" pack), int4 [Tpad][M]: x and y as above, z / w the
// f32 bits of delta_left / delta_right; a leaf has threshold 0 and both
// deltas +0.0. Per tree:
//   phase A  lds_levels[t] fixed trips (the tree is block-uniform, so no
//            minimum over the phase): one 128-bit LDS read of the record,
//            the key read, the compare, the add, the step. A chain at a leaf
//            self-loops and adds +0.0 (to column d when ACC_LDS).
//   phase B  as in scoring, with 16-byte records; a finished chain adds
//            nothing.
// ACC_LDS: accumulators in a feature-major LDS tile [d + 1][FS] of f32: the
// bank is the thread's own whatever feature a lane adds to, slab d absorbs
// the self-loop adds; zeroed per row tile, flushed with coalesced stores.
// Otherwise the pre-zeroed out[N][d] itself, thread-owned, the add
// predicated on f < d and row < N, finalized in place. No atomics.
// ---------------------------------------------------------------------------

#define XDEEP_PH 4

// correctly rounded f32 quotient: numpy's f32 divide bit for bit
// (forest_kernels.hip, div32_exact)
__device__ __forceinline__ float div32_exact(float a, float b) {
  return (float)((double)a / (double)b);
}

template <typename KT, int RPT, bool ACC_LDS>
__global__ void __launch_bounds__(DEEP_BT) explain_forest_deep_kernel(
    const KT* __restrict__ X,               // raw bf16/fp16/f32 bits
    const int4* __restrict__ nodes,         // [Tpad][M] explain deep records
    const int32_t* __restrict__ lds_levels, // [Tpad]
    float* __restrict__ out,                // [N][d] (pre-zeroed if !ACC_LDS)
    int64_t N, int32_t d, int32_t Tpad, int32_t M, int32_t S, int32_t height,
    float fT, int32_t finalize, int64_t rs, int64_t cs) {
  constexpr int FS = RPT * DEEP_BT;
  constexpr int PH = XDEEP_PH;
  constexpr uint32_t ALL = (1u << RPT) - 1u;
  const int tid = threadIdx.x;
  const int staged = min(S, M);  // records of a tree that the stage holds

  int4* tlds = (int4*)smem;              // [PH][S]
  float* acc = (float*)(tlds + PH * S);  // [d + 1][FS] when ACC_LDS
  KT* rows = (KT*)(acc + (ACC_LDS ? (d + 1) * FS : 0));

  for (int64_t block_row0 = (int64_t)blockIdx.x * FS; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * FS) {
    const int rows_here = (int)min((int64_t)FS, N - block_row0);

    __syncthreads();  // previous tile's flush / readers done
    stage_tile<KT, RPT>(rows, X, block_row0, rows_here, d, rs, cs);
    if (ACC_LDS)
      for (int i = tid; i < (d + 1) * FS; i += DEEP_BT) acc[i] = 0.f;
    // the first phase's barriers order these stores before the walk

    const KT* rb[RPT];
    float* ab[RPT];     // ACC_LDS: the row's column 0 in the tile
    int64_t ooff[RPT];  // else: the row's offset in out
    bool inb[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int j = tid + r * DEEP_BT;
      rb[r] = rows + tile_slot<KT, RPT>(j);
      ab[r] = acc + j;
      ooff[r] = (block_row0 + j) * d;
      inb[r] = j < rows_here;
    }

    // adds delta[r] to the accumulator of (row r, feature f[r]) for every r
    // in `on`: all reads before all writes (the rows' cells are distinct)
    auto accumulate = [&](const int (&f)[RPT], const float (&delta)[RPT],
                          uint32_t on) __attribute__((always_inline)) {
      float a[RPT];
      if (ACC_LDS) {
#pragma unroll
        for (int r = 0; r < RPT; ++r)
          if (on & (1u << r)) a[r] = ab[r][f[r] * FS];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
          if (on & (1u << r)) ab[r][f[r] * FS] = __fadd_rn(a[r], delta[r]);
      } else {
        uint32_t ok = 0;
#pragma unroll
        for (int r = 0; r < RPT; ++r)
          if ((on & (1u << r)) && f[r] < d && inb[r]) ok |= 1u << r;
#pragma unroll
        for (int r = 0; r < RPT; ++r)
          if (ok & (1u << r)) a[r] = out[ooff[r] + f[r]];
#pragma unroll
        for (int r = 0; r < RPT; ++r)
          if (ok & (1u << r)) out[ooff[r] + f[r]] = __fadd_rn(a[r], delta[r]);
      }
    };

    for (int t = 0; t < Tpad; t += PH) {
      __syncthreads();  // previous phase's LDS readers done
#pragma unroll
      for (int s = 0; s < PH; ++s) {
        const int4* src = nodes + (int64_t)(t + s) * M;
        int4* dst = tlds + s * S;
        for (int i = tid; i < staged; i += DEEP_BT) dst[i] = src[i];
      }
      __syncthreads();

#pragma unroll 1
      for (int s = 0; s < PH; ++s) {  // a row's trees: strictly in order
        const int4* ts = tlds + s * S;
        const int4* nb = nodes + (int64_t)(t + s) * M;
        const int la = min(lds_levels[t + s], height);
        int cur[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) cur[r] = 0;

        // ---- phase A: la levels, LDS only ---------------------------------
        for (int it = 0; it < la; ++it) {
          int4 nd[RPT];
#pragma unroll
          for (int r = 0; r < RPT; ++r) nd[r] = ts[cur[r]];
          int f[RPT];
          KT kraw[RPT];
#pragma unroll
          for (int r = 0; r < RPT; ++r) {
            f[r] = rec_feat(nd[r].x);
            kraw[r] = rb[r][f[r] * FS];
          }
          float delta[RPT];
#pragma unroll
          for (int r = 0; r < RPT; ++r) {
            const bool left = widen_key(kraw[r]) < (uint32_t)nd[r].y;
            delta[r] = __int_as_float(left ? nd[r].z : nd[r].w);
            cur[r] = rec_link(nd[r].x) - (int)left;
          }
          accumulate(f, delta, ALL);
        }

        // ---- phase B: the tail ---------------------------------------------
        // bit r of `live`: the chain has not read its leaf yet. `first`: see
        // score_forest_deep_kernel
        uint32_t live = ALL;
        auto tail_trip = [&](auto first) __attribute__((always_inline)) {
          int4 nd[RPT];
#pragma unroll
          for (int r = 0; r < RPT; ++r)
            if (live & (1u << r)) {
              if (decltype(first)::value && cur[r] < S)
                nd[r] = ts[cur[r]];
              else
                nd[r] = nb[cur[r]];
            }
          int f[RPT];
          KT kraw[RPT];
#pragma unroll
          for (int r = 0; r < RPT; ++r)
            if (live & (1u << r)) {
              f[r] = rec_feat(nd[r].x);
              kraw[r] = rb[r][f[r] * FS];
            }
          float delta[RPT];
#pragma unroll
          for (int r = 0; r < RPT; ++r)
            if (live & (1u << r)) {
              const int link = rec_link(nd[r].x);
              if (link == cur[r]) {
                live &= ~(1u << r);
              } else {
                const bool left = widen_key(kraw[r]) < (uint32_t)nd[r].y;
                delta[r] = __int_as_float(left ? nd[r].z : nd[r].w);
                cur[r] = link - (int)left;
              }
            }
          // a chain that has read its leaf adds nothing
          accumulate(f, delta, live);
        };
        tail_trip(std::true_type{});
        // a chain at depth `height` is a leaf: height - la more trips read it
        for (int k = la; k < height && __any(live != 0); ++k)
          tail_trip(std::false_type{});
      }
    }

    if (ACC_LDS) {
      __syncthreads();  // every row's accumulators final
      const int total = rows_here * d;
      float* o = out + block_row0 * d;
      for (int g = tid; g < total; g += DEEP_BT) {
        const int r = (int)((uint32_t)g / (uint32_t)d), c = g - r * d;
        const float v = acc[c * FS + r];
        o[g] = finalize ? div32_exact(v, fT) : v;
      }
    } else if (finalize) {
#pragma unroll
      for (int r = 0; r < RPT; ++r)
        if (inb[r])
          for (int c = 0; c < d; ++c) {
            float* o = out + ooff[r] + c;
            *o = div32_exact(*o, fT);
          }
    }
  }
}

// ---------------------------------------------------------------------------
// extended forests (docs/DESIGN.md §8): the same two-phase walk over
// hyperplane nodes. BITWISE equal to cpu_engine.feature_contributions_extended:
// the dot is fadd(dot, fmul(w_j, x_j)) in ascending j from 0.f over all nnz
// stored coordinates of an internal node (no FMA), the decision is
// dot < offset (NaN goes right), and the taken edge's per-coordinate shares
// are added in ascending j over the node's k coordinates, trees 0..T-1, root
// to leaf. Coordinates of a node may repeat: a row's adds of one visit are
// read-add-write one after another.
//
// Pack ("explain eif deep"), level order as above:
//   nodes    int2 [Tpad][M]       x = k | link << 12, y = f32 bits of offset;
//                                 a leaf has link = its own index and k = 0
//   payload  int4 [Tpad][M][nnz]  {coordinate, w bits, delta_left share bits,
//                                  delta_right share bits}
// eif_deep_gather_kernel makes both from the int4 records that
// deep_level_order_kernel<int4> writes when it is handed each slot's
// pre-order index as the "delta_left" word (and 0 as the leaf sentinel).
//
// Rows are staged as raw bits in their own element type (the widening at the
// read is exact). PHT trees per barrier phase: the first S node records and
// their S * nnz payload entries, copied linearly. A visit reads the record,
// runs the dot over the payload (16 bytes a coordinate), compares, runs the
// payload again for the taken shares and steps; a chain at a leaf reads no
// payload and adds nothing. Phase A: lds_levels[t] trips from LDS, no flags;
// phase B: records and payload from global memory, one wave vote a trip, the
// first trip still from LDS below S.
// ---------------------------------------------------------------------------

__device__ __forceinline__ float widen_row(uint16_t b) {
  return __uint_as_float((uint32_t)b << 16);  // bf16 -> f32
}
__device__ __forceinline__ float widen_row(f16_t b) {
  union { uint16_t u; _Float16 h; } cv;
  cv.u = (uint16_t)b;
  return (float)cv.h;  // exact, subnormals included
}
__device__ __forceinline__ float widen_row(uint32_t b) {
  return __uint_as_float(b);
}

// one thread per (tree, slot): the node record, and the payload of an
// internal node gathered from its pre-order slot `old`
__global__ void __launch_bounds__(DEEP_BT) eif_deep_gather_kernel(
    const int4* __restrict__ lvl,      // [Tpad][M] {k | link << 12, offset,
                                       //            old index, -}
    const int32_t* __restrict__ hidx,  // [T][M0][nnz]
    const int32_t* __restrict__ hw,    // [T][M0][nnz] f32 bits
    const int32_t* __restrict__ dl,    // [T][M0][nnz] f32 bits
    const int32_t* __restrict__ dr,    // [T][M0][nnz] f32 bits
    int2* __restrict__ nodes,          // [Tpad][M]
    int4* __restrict__ payload,        // [Tpad][M][nnz]
    int32_t T, int32_t Tpad, int32_t M0, int32_t M, int32_t nnz, int32_t d) {
  const int64_t total = (int64_t)Tpad * M;
  for (int64_t g = (int64_t)blockIdx.x * DEEP_BT + threadIdx.x; g < total;
       g += (int64_t)gridDim.x * DEEP_BT) {
    const int t = (int)(g / M), i = (int)(g - (int64_t)t * M);
    const int4 rec = lvl[g];
    const bool internal = t < T && rec_link(rec.x) != i;
    nodes[g] = make_int2(rec.x, internal ? rec.y : 0);
    const int old = min(max(rec.z, 0), M0 - 1);
    const int64_t src = ((int64_t)t * M0 + old) * nnz;
    int4* dst = payload + g * nnz;
    for (int j = 0; j < nnz; ++j)
      dst[j] = internal ? make_int4(min(max(hidx[src + j], 0), d - 1),
                                    hw[src + j], dl[src + j], dr[src + j])
                        : make_int4(0, 0, 0, 0);
  }
}

template <typename XT, int RPT, bool ACC_LDS>
__global__ void __launch_bounds__(DEEP_BT) explain_extended_deep_kernel(
    const XT* __restrict__ X,               // raw bf16/fp16/f32 bits
    const int2* __restrict__ nodes,         // [Tpad][M]
    const int4* __restrict__ payload,       // [Tpad][M][nnz]
    const int32_t* __restrict__ lds_levels, // [Tpad]
    float* __restrict__ out,                // [N][d] (pre-zeroed if !ACC_LDS)
    int64_t N, int32_t d, int32_t nnz, int32_t Tpad, int32_t M, int32_t S,
    int32_t PHT, int32_t height, float fT, int32_t finalize, int64_t rs,
    int64_t cs) {
  constexpr int FS = RPT * DEEP_BT;
  constexpr uint32_t ALL = (1u << RPT) - 1u;
  const int tid = threadIdx.x;
  const int staged = min(S, M);  // records of a tree that the stage holds

  int4* plds = (int4*)smem;                        // [PHT][S][nnz]
  int2* tlds = (int2*)(plds + (size_t)PHT * S * nnz);  // [PHT][S]
  float* acc = (float*)(tlds + PHT * S);           // [d][FS] when ACC_LDS
  XT* rows = (XT*)(acc + (ACC_LDS ? d * FS : 0));  // [d][FS]

  for (int64_t block_row0 = (int64_t)blockIdx.x * FS; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * FS) {
    const int rows_here = (int)min((int64_t)FS, N - block_row0);

    __syncthreads();  // previous tile's flush / readers done
    stage_tile<XT, RPT, false>(rows, X, block_row0, rows_here, d, rs, cs);
    if (ACC_LDS)
      for (int i = tid; i < d * FS; i += DEEP_BT) acc[i] = 0.f;
    // the first phase's barriers order these stores before the walk

    const XT* rb[RPT];
    float* ab[RPT];     // ACC_LDS: the row's column 0 in the tile
    int64_t ooff[RPT];  // else: the row's offset in out
    bool inb[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int j = tid + r * DEEP_BT;
      rb[r] = rows + tile_slot<XT, RPT>(j);
      ab[r] = acc + j;
      ooff[r] = (block_row0 + j) * d;
      inb[r] = j < rows_here;
    }

    for (int t = 0; t < Tpad; t += PHT) {
      __syncthreads();  // previous phase's LDS readers done
      for (int s = 0; s < PHT; ++s) {
        const int2* nsrc = nodes + (int64_t)(t + s) * M;
        const int4* psrc = payload + (int64_t)(t + s) * M * nnz;
        int2* ndst = tlds + s * S;
        int4* pdst = plds + (size_t)s * S * nnz;
        for (int i = tid; i < staged; i += DEEP_BT) ndst[i] = nsrc[i];
        for (int i = tid; i < staged * nnz; i += DEEP_BT) pdst[i] = psrc[i];
      }
      __syncthreads();

#pragma unroll 1
      for (int s = 0; s < PHT; ++s) {  // a row's trees: strictly in order
        const int2* ts = tlds + s * S;
        const int4* ps = plds + (size_t)s * S * nnz;
        const int2* nb = nodes + (int64_t)(t + s) * M;
        const int4* pb = payload + (int64_t)(t + s) * M * nnz;
        const int la = min(lds_levels[t + s], height);
        int cur[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) cur[r] = 0;
        // bit r of `live`: the chain has not read its leaf yet (phase B)
        uint32_t live = ALL;

        // One level of the thread's chains. MODE 0: phase A, every record
        // and payload entry from LDS. MODE 1: the first tail trip, from LDS
        // below S (the level after the staged ones straddles the stage's
        // end, and a chain may rest at a staged leaf). MODE 2: from global.
        auto trip = [&](auto mode) __attribute__((always_inline)) {
          constexpr int MODE = decltype(mode)::value;
          const uint32_t walk = MODE == 0 ? ALL : live;
          int2 nd[RPT];
          uint32_t in_lds = 0;
#pragma unroll
          for (int r = 0; r < RPT; ++r)
            if (walk & (1u << r)) {
              if (MODE == 0 || (MODE == 1 && cur[r] < S)) {
                nd[r] = ts[cur[r]];
                in_lds |= 1u << r;
              } else {
                nd[r] = nb[cur[r]];
              }
            }
          // `on`: the chain reads an internal node on this trip
          uint32_t on = 0;
          int64_t pbase[RPT];
#pragma unroll
          for (int r = 0; r < RPT; ++r)
            if (walk & (1u << r)) {
              if (rec_link(nd[r].x) != cur[r]) on |= 1u << r;
              else if (MODE != 0) live &= ~(1u << r);
              pbase[r] = (int64_t)cur[r] * nnz;
            }
          auto entry = [&](int r, int j) __attribute__((always_inline)) {
            return (in_lds & (1u << r)) ? ps[(int)pbase[r] + j]
                                        : pb[pbase[r] + j];
          };
          float dot[RPT];
#pragma unroll
          for (int r = 0; r < RPT; ++r) dot[r] = 0.f;
          for (int j = 0; j < nnz; ++j) {
            int4 p[RPT];
#pragma unroll
            for (int r = 0; r < RPT; ++r)
              if (on & (1u << r)) p[r] = entry(r, j);
            XT xr[RPT];
#pragma unroll
            for (int r = 0; r < RPT; ++r)
              if (on & (1u << r)) xr[r] = rb[r][p[r].x * FS];
#pragma unroll
            for (int r = 0; r < RPT; ++r)
              if (on & (1u << r))
                dot[r] = __fadd_rn(
                    dot[r], __fmul_rn(__int_as_float(p[r].y), widen_row(xr[r])));
          }
          uint32_t left = 0;
#pragma unroll
          for (int r = 0; r < RPT; ++r)
            if ((on & (1u << r)) && dot[r] < __int_as_float(nd[r].y))
              left |= 1u << r;
          // the taken edge's shares, ascending j over the node's k
          // coordinates; per row: read, add, write before the next j
          for (int j = 0; j < nnz; ++j) {
            uint32_t add = 0;
            int4 p[RPT];
#pragma unroll
            for (int r = 0; r < RPT; ++r)
              if ((on & (1u << r)) && j < rec_feat(nd[r].x)) {
                p[r] = entry(r, j);
                add |= 1u << r;
              }
            float a[RPT];
            if (ACC_LDS) {
#pragma unroll
              for (int r = 0; r < RPT; ++r)
                if (add & (1u << r)) a[r] = ab[r][p[r].x * FS];
            } else {
#pragma unroll
              for (int r = 0; r < RPT; ++r) {
                if ((add & (1u << r)) &&
                    (!inb[r] || (uint32_t)p[r].x >= (uint32_t)d))
                  add &= ~(1u << r);
                if (add & (1u << r)) a[r] = out[ooff[r] + p[r].x];
              }
            }
#pragma unroll
            for (int r = 0; r < RPT; ++r)
              if (add & (1u << r)) {
                const float v = __fadd_rn(
                    a[r], __int_as_float((left & (1u << r)) ? p[r].z : p[r].w));
                if (ACC_LDS) ab[r][p[r].x * FS] = v;
                else out[ooff[r] + p[r].x] = v;
              }
          }
#pragma unroll
          for (int r = 0; r < RPT; ++r)
            if (on & (1u << r))
              cur[r] = rec_link(nd[r].x) - (int)((left >> r) & 1u);
        };

        for (int it = 0; it < la; ++it)
          trip(std::integral_constant<int, 0>{});
        trip(std::integral_constant<int, 1>{});
        // a chain at depth `height` is a leaf: height - la more trips read it
        for (int k = la; k < height && __any(live != 0); ++k)
          trip(std::integral_constant<int, 2>{});
      }
    }

    if (ACC_LDS) {
      __syncthreads();  // every row's accumulators final
      const int total = rows_here * d;
      float* o = out + block_row0 * d;
      for (int g = tid; g < total; g += DEEP_BT) {
        const int r = (int)((uint32_t)g / (uint32_t)d), c = g - r * d;
        const float v = acc[c * FS + r];
        o[g] = finalize ? div32_exact(v, fT) : v;
      }
    } else if (finalize) {
#pragma unroll
      for (int r = 0; r < RPT; ++r)
        if (inb[r])
          for (int c = 0; c < d; ++c) {
            float* o = out + ooff[r] + c;
            *o = div32_exact(*o, fT);
          }
    }
  }
}

// ---------------------------------------------------------------------------
// extended scoring (docs/DESIGN.md §3b): the two-phase walk over hyperplane
// nodes with nothing to add along the path. BITWISE equal to
// cpu_engine.path_lengths_extended: per visit the dot is
// fadd(dot, fmul(w_j, x_j)) from 0.f in ascending j over all nnz stored
// coordinates (no FMA), the step is cur = link - (dot < offset) (NaN goes
// right), and a row's leaf values f32(depth) + f32(value) are added in tree
// order. Only that last add is ordered, so a thread walks the PH trees of a
// phase together: RPT * PH independent chains.
//
// Pack ("eif deep"), level order as above, f32 throughout (every row kind):
//   nodes  int2 [Tpad][M]      x = k | link << 12, y = f32 bits of the offset;
//                              a leaf has link = its own index, k = 0 and
//                              y = f32 bits of depth + value
//   hyper  int2 [Tpad][M][HS]  {coordinate, f32 bits of w}; HS = nnz rounded
//                              up to even (1 stays 1), so that the entries of
//                              a node start on 16 bytes and two are read per
//                              128-bit load. Leaves and the pad entry are zero;
//                              the pad entry is never read.
// eif_score_gather_kernel makes both from the int2 records that
// deep_level_order_kernel<int2> writes when it is handed each slot's
// pre-order index as its threshold word (and 0 as the leaf sentinel).
//
// A chain is at a leaf when the record's link is its own index; the step is
// predicated on that, never on the dot: a leaf's entries are {0, 0.f} and
// 0 * inf is NaN. Phase A reads a resting chain's record and entries again
// (all inside the stage); phase B loads nothing for a finished chain and
// nothing past the first entry load for a chain that turns out to be at its
// leaf.
// ---------------------------------------------------------------------------

__host__ __device__ __forceinline__ int eif_hyper_stride(int nnz) {
  return nnz == 1 ? 1 : (nnz + 1) & ~1;
}

// one thread per (tree, slot): the node record with the host's value word,
// and the entries of an internal node gathered from its pre-order slot
__global__ void __launch_bounds__(DEEP_BT) eif_score_gather_kernel(
    const int2* __restrict__ lvl,      // [Tpad][M] {k | link << 12, old index}
    const int32_t* __restrict__ vw,    // [T][M0] offset / leaf value bits
    const int32_t* __restrict__ hidx,  // [T][M0][nnz]
    const int32_t* __restrict__ hw,    // [T][M0][nnz] f32 bits
    int2* __restrict__ nodes,          // [Tpad][M]
    int2* __restrict__ hyper,          // [Tpad][M][HS]
    int32_t T, int32_t Tpad, int32_t M0, int32_t M, int32_t nnz, int32_t d) {
  const int hs = eif_hyper_stride(nnz);
  const int64_t total = (int64_t)Tpad * M;
  for (int64_t g = (int64_t)blockIdx.x * DEEP_BT + threadIdx.x; g < total;
       g += (int64_t)gridDim.x * DEEP_BT) {
    const int t = (int)(g / M), i = (int)(g - (int64_t)t * M);
    const int2 rec = lvl[g];
    // only the root has pre-order index 0: any other slot that carries it is
    // one the reorder filled in (past the tree's nodes, or a pad tree)
    const bool slot = t < T && (i == 0 || rec.y > 0);
    const bool internal = slot && rec_link(rec.x) != i;
    const int old = min(max(rec.y, 0), M0 - 1);
    const int64_t src = (int64_t)t * M0 + old;
    nodes[g] = make_int2(rec.x, slot ? vw[src] : 0);
    int2* dst = hyper + g * hs;
    for (int j = 0; j < hs; ++j)
      dst[j] = internal && j < nnz
                   ? make_int2(min(max(hidx[src * nnz + j], 0), d - 1),
                               hw[src * nnz + j])
                   : make_int2(0, 0);
  }
}

// n 8-byte words from global memory into LDS, all threads of the block; dst
// is on 16 bytes. The reads are 16-byte pieces from src's first 16-byte
// boundary on (a tree of an odd M starts on 8), the stores too where src
// itself is on 16.
__device__ __forceinline__ void stage_words(int2* dst,
                                            const int2* __restrict__ src,
                                            int n) {
  const int tid = threadIdx.x;
  const int head = min((int)(((uintptr_t)src >> 3) & 1), n);
  if (tid < head) dst[0] = src[0];
  const uint4* s4 = (const uint4*)(src + head);
  const int pairs = (n - head) >> 1;
  if (head == 0) {
    for (int i = tid; i < pairs; i += DEEP_BT) ((uint4*)dst)[i] = s4[i];
  } else {
    for (int i = tid; i < pairs; i += DEEP_BT) {
      const uint4 v = s4[i];
      dst[1 + 2 * i] = make_int2((int)v.x, (int)v.y);
      dst[2 + 2 * i] = make_int2((int)v.z, (int)v.w);
    }
  }
  if (((n - head) & 1) && tid == DEEP_BT - 1) dst[n - 1] = src[n - 1];
}

// The dots of a thread's chains are independent f32 multiplies and adds,
// which the compiler would pair into packed instructions; this walk keeps
// one scalar v_mul_f32 / v_add_f32 per term.
#if defined(__HIP_DEVICE_COMPILE__)
#define DEEP_SCALAR_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define DEEP_SCALAR_F32  // the host pass compiles only the launch stub
#endif

template <typename XT, int RPT, int PH>
__global__ void DEEP_SCALAR_F32 __launch_bounds__(DEEP_BT)
score_extended_deep_kernel(
    const XT* __restrict__ X,               // raw bf16/fp16/f32 bits
    const int2* __restrict__ nodes,         // [Tpad][M]
    const int2* __restrict__ hyper,         // [Tpad][M][HS]
    const int32_t* __restrict__ lds_levels, // [Tpad]
    float* __restrict__ out,                // [N] (path sum or score)
    int64_t N, int32_t d, int32_t nnz, int32_t Tpad, int32_t M, int32_t S,
    int32_t height, float fT, float c_norm, int32_t finalize, int64_t rs,
    int64_t cs) {
  constexpr int FS = RPT * DEEP_BT;
  constexpr int NC = RPT * PH;  // chain c: row c / PH, tree c % PH
  constexpr uint32_t ALL = (1u << NC) - 1u;
  const int tid = threadIdx.x;
  const int staged = min(S, M);  // records of a tree that the stage holds
  const int hs = eif_hyper_stride(nnz);
  const int npair = nnz >> 1;

  int2* hlds = (int2*)smem;                 // [PH][S][HS]
  int2* tlds = hlds + (size_t)PH * S * hs;  // [PH][S]
  XT* rows = (XT*)(tlds + PH * S);          // [d][FS]

  for (int64_t block_row0 = (int64_t)blockIdx.x * FS; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * FS) {
    const int rows_here = (int)min((int64_t)FS, N - block_row0);

    __syncthreads();  // previous tile's readers done
    stage_tile<XT, RPT, false>(rows, X, block_row0, rows_here, d, rs, cs);
    // the first phase's barriers order these stores before the walk

    const XT* rb[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r)
      rb[r] = rows + tile_slot<XT, RPT>(tid + r * DEEP_BT);

    float psum[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) psum[r] = 0.f;

    for (int t = 0; t < Tpad; t += PH) {
      __syncthreads();  // previous phase's LDS readers done
#pragma unroll
      for (int s = 0; s < PH; ++s) {
        stage_words(tlds + s * S, nodes + (int64_t)(t + s) * M, staged);
        stage_words(hlds + (size_t)s * S * hs,
                    hyper + (int64_t)(t + s) * M * hs, staged * hs);
      }
      // trips that stay inside every tree's stage. 0 levels means the root
      // is a leaf, which rests at record 0 for any number of trips.
      int la = height;
#pragma unroll
      for (int s = 0; s < PH; ++s) {
        const int l = lds_levels[t + s];
        if (l > 0) la = min(la, l);
      }
      __syncthreads();

      const int2* nbase[PH];
      const int2* hbase[PH];
#pragma unroll
      for (int s = 0; s < PH; ++s) {
        nbase[s] = nodes + (int64_t)(t + s) * M;
        hbase[s] = hyper + (int64_t)(t + s) * M * hs;
      }

      int cur[NC], val[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) cur[c] = val[c] = 0;
      // bit c of `live`: the chain has not read its leaf yet (phase B)
      uint32_t live = ALL;

      // One level of the thread's chains. MODE 0: phase A, every record and
      // entry from LDS, no flags. MODE 1: the first tail trip, from LDS below
      // S (the level after the staged ones straddles the stage's end, and a
      // chain may rest at a staged leaf). MODE 2: from global memory.
      auto trip = [&](auto mode) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode)::value;
        const uint32_t walk = MODE == 0 ? ALL : live;
        int2 nd[NC];
        uint32_t in_lds = MODE == 0 ? ALL : 0u;
        int lo[NC];      // first entry of the node: in the stage,
        int64_t go[NC];  // in the tree
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (walk & (1u << c)) {
            const int s = c % PH;
            if (MODE == 1 && cur[c] < S) in_lds |= 1u << c;
            if (in_lds & (1u << c)) {
              nd[c] = tlds[s * S + cur[c]];
              lo[c] = (s * S + cur[c]) * hs;
            } else {
              nd[c] = nbase[s][cur[c]];
              go[c] = (int64_t)cur[c] * hs;
            }
          }
        float dot[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) dot[c] = 0.f;
        // `on`: the chain reads an internal node on this trip. The first
        // entry load of a tail trip does not wait for the record to say so.
        uint32_t on = 0;
        for (int j = 0; j < npair; ++j) {
          const uint32_t ld = (MODE == 0 || j == 0) ? walk : on;
          int4 p[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (ld & (1u << c))
              p[c] = (in_lds & (1u << c))
                         ? *(const int4*)(hlds + lo[c] + 2 * j)
                         : *(const int4*)(hbase[c % PH] + go[c] + 2 * j);
          XT xa[NC], xb[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (ld & (1u << c)) {
              xa[c] = rb[c / PH][p[c].x * FS];
              xb[c] = rb[c / PH][p[c].z * FS];
            }
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (ld & (1u << c)) {
              dot[c] = __fadd_rn(dot[c], __fmul_rn(__int_as_float(p[c].y),
                                                   widen_row(xa[c])));
              dot[c] = __fadd_rn(dot[c], __fmul_rn(__int_as_float(p[c].w),
                                                   widen_row(xb[c])));
            }
          if (MODE != 0 && j == 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
              if ((walk & (1u << c)) && rec_link(nd[c].x) != cur[c])
                on |= 1u << c;
          }
        }
        if (nnz & 1) {
          uint32_t ld = walk;
          if (MODE != 0 && npair > 0) ld = on;
          int2 p[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (ld & (1u << c))
              p[c] = (in_lds & (1u << c))
                         ? hlds[lo[c] + nnz - 1]
                         : hbase[c % PH][go[c] + nnz - 1];
          XT xa[NC];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (ld & (1u << c)) xa[c] = rb[c / PH][p[c].x * FS];
#pragma unroll
          for (int c = 0; c < NC; ++c)
            if (ld & (1u << c))
              dot[c] = __fadd_rn(dot[c], __fmul_rn(__int_as_float(p[c].y),
                                                   widen_row(xa[c])));
        }
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (walk & (1u << c)) {
            const int link = rec_link(nd[c].x);
            const bool internal = link != cur[c];
            if (MODE != 0) {
              val[c] = nd[c].y;
              if (!internal) live &= ~(1u << c);
            }
            cur[c] = link - (int)(internal &&
                                  dot[c] < __int_as_float(nd[c].y));
          }
      };

      for (int it = 0; it < la; ++it) trip(std::integral_constant<int, 0>{});
      trip(std::integral_constant<int, 1>{});
      // a chain at depth `height` is a leaf: height - la more trips read it
      for (int k = la; k < height && __any(live != 0); ++k)
        trip(std::integral_constant<int, 2>{});

#pragma unroll
      for (int r = 0; r < RPT; ++r)
#pragma unroll
        for (int s = 0; s < PH; ++s)
          psum[r] = __fadd_rn(psum[r], __int_as_float(val[r * PH + s]));
    }

#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t my_row = block_row0 + tid + r * DEEP_BT;
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

}  // namespace deep

// host-side launchers (bindings.cpp is compiled by g++)

void launch_deep_level_order(const int32_t* feat, const int32_t* right,
                             const int32_t* w, const int32_t* ncount,
                             uint32_t* front_a, uint32_t* front_b, void* out,
                             int32_t* lds_levels, int32_t T, int32_t Tpad,
                             int32_t M0, int32_t M, int32_t S, int32_t d,
                             hipStream_t stream) {
  hipLaunchKernelGGL(deep::deep_level_order_kernel<int2>, dim3(Tpad),
                     dim3(DEEP_BT), 0, stream, feat, right, w,
                     (const int32_t*)nullptr, (const int32_t*)nullptr, ncount,
                     front_a, front_b, (int2*)out, lds_levels, T, M0, M, S, d);
}

void launch_explain_deep_level_order(
    const int32_t* feat, const int32_t* right, const int32_t* w,
    const int32_t* dl, const int32_t* dr, const int32_t* ncount,
    uint32_t* front_a, uint32_t* front_b, void* out, int32_t* lds_levels,
    int32_t T, int32_t Tpad, int32_t M0, int32_t M, int32_t S, int32_t d,
    hipStream_t stream) {
  hipLaunchKernelGGL(deep::deep_level_order_kernel<int4>, dim3(Tpad),
                     dim3(DEEP_BT), 0, stream, feat, right, w, dl, dr, ncount,
                     front_a, front_b, (int4*)out, lds_levels, T, M0, M, S, d);
}

hipError_t launch_score_forest_deep(RowDtype dt, int rpt, const void* X,
                                    const void* nodes,
                                    const int32_t* lds_levels, float* out,
                                    int64_t N, int32_t d, int64_t rs,
                                    int64_t cs, int32_t Tpad, int32_t M,
                                    int32_t S, int32_t height, float fT,
                                    float c_norm, int finalize, size_t lds,
                                    int blocks, hipStream_t stream) {
  hipError_t err = hipSuccess;
#define LDP1(KT, RPT)                                                         \
  do {                                                                        \
    const void* fn = (const void*)deep::score_forest_deep_kernel<KT, RPT, 4>; \
    if (lds > 64 * 1024)                                                      \
      err = hipFuncSetAttribute(                                              \
          fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);          \
    if (err != hipSuccess) return err;                                        \
    hipLaunchKernelGGL((deep::score_forest_deep_kernel<KT, RPT, 4>),          \
                       dim3(blocks), dim3(DEEP_BT), lds, stream,              \
                       (const KT*)X, (const int2*)nodes, lds_levels, out, N,  \
                       d, Tpad, M, S, height, fT, c_norm, finalize, rs, cs);  \
  } while (0)
#define LDP(KT)                                                               \
  do {                                                                        \
    if (rpt == 2) LDP1(KT, 2);                                                \
    else LDP1(KT, 1);                                                         \
  } while (0)
  if (dt == ROW_BF16) LDP(uint16_t);
  else if (dt == ROW_F16) LDP(deep::f16_t);
  else LDP(uint32_t);
#undef LDP
#undef LDP1
  return hipGetLastError();
}

hipError_t launch_explain_forest_deep(RowDtype dt, int rpt, bool acc_lds,
                                      const void* X, const void* nodes,
                                      const int32_t* lds_levels, float* out,
                                      int64_t N, int32_t d, int64_t rs,
                                      int64_t cs, int32_t Tpad, int32_t M,
                                      int32_t S, int32_t height, float fT,
                                      int finalize, size_t lds, int blocks,
                                      hipStream_t stream) {
  // the binding's two shapes: two rows a thread with the accumulator tile,
  // one row a thread with the accumulators in out
  if ((rpt != 2 || !acc_lds) && (rpt != 1 || acc_lds))
    return hipErrorInvalidValue;
  hipError_t err = hipSuccess;
#define LXD1(KT, RPT, AL)                                                     \
  do {                                                                        \
    const void* fn =                                                          \
        (const void*)deep::explain_forest_deep_kernel<KT, RPT, AL>;           \
    if (lds > 64 * 1024)                                                      \
      err = hipFuncSetAttribute(                                              \
          fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);          \
    if (err != hipSuccess) return err;                                        \
    hipLaunchKernelGGL((deep::explain_forest_deep_kernel<KT, RPT, AL>),       \
                       dim3(blocks), dim3(DEEP_BT), lds, stream,              \
                       (const KT*)X, (const int4*)nodes, lds_levels, out, N,  \
                       d, Tpad, M, S, height, fT, finalize, rs, cs);          \
  } while (0)
#define LXD(KT)                                                               \
  do {                                                                        \
    if (acc_lds) LXD1(KT, 2, true);                                           \
    else LXD1(KT, 1, false);                                                  \
  } while (0)
  if (dt == ROW_BF16) LXD(uint16_t);
  else if (dt == ROW_F16) LXD(deep::f16_t);
  else LXD(uint32_t);
#undef LXD
#undef LXD1
  return hipGetLastError();
}

// lvl: the int4 records of launch_explain_deep_level_order run with every
// slot's pre-order index as its delta_left word and d = 0
void launch_eif_deep_gather(const void* lvl, const int32_t* hidx,
                            const int32_t* hw, const int32_t* dl,
                            const int32_t* dr, void* nodes, void* payload,
                            int32_t T, int32_t Tpad, int32_t M0, int32_t M,
                            int32_t nnz, int32_t d, hipStream_t stream) {
  const int64_t total = (int64_t)Tpad * M;
  const int blocks =
      (int)std::min<int64_t>((total + DEEP_BT - 1) / DEEP_BT, 65535);
  hipLaunchKernelGGL(deep::eif_deep_gather_kernel, dim3(blocks), dim3(DEEP_BT),
                     0, stream, (const int4*)lvl, hidx, hw, dl, dr,
                     (int2*)nodes, (int4*)payload, T, Tpad, M0, M, nnz, d);
}

hipError_t launch_explain_extended_deep(
    RowDtype dt, int rpt, bool acc_lds, const void* X, const void* nodes,
    const void* payload, const int32_t* lds_levels, float* out, int64_t N,
    int32_t d, int32_t nnz, int64_t rs, int64_t cs, int32_t Tpad, int32_t M,
    int32_t S, int32_t trees_per_phase, int32_t height, float fT, int finalize,
    size_t lds, int blocks, hipStream_t stream) {
  // the binding's two shapes, as in launch_explain_forest_deep
  if ((rpt != 2 || !acc_lds) && (rpt != 1 || acc_lds))
    return hipErrorInvalidValue;
  if (trees_per_phase < 1 || Tpad % trees_per_phase != 0)
    return hipErrorInvalidValue;
  hipError_t err = hipSuccess;
#define LXE1(XT, RPT, AL)                                                     \
  do {                                                                        \
    const void* fn =                                                          \
        (const void*)deep::explain_extended_deep_kernel<XT, RPT, AL>;         \
    if (lds > 64 * 1024)                                                      \
      err = hipFuncSetAttribute(                                              \
          fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);          \
    if (err != hipSuccess) return err;                                        \
    hipLaunchKernelGGL((deep::explain_extended_deep_kernel<XT, RPT, AL>),     \
                       dim3(blocks), dim3(DEEP_BT), lds, stream,              \
                       (const XT*)X, (const int2*)nodes,                      \
                       (const int4*)payload, lds_levels, out, N, d, nnz,      \
                       Tpad, M, S, trees_per_phase, height, fT, finalize, rs, \
                       cs);                                                   \
  } while (0)
#define LXE(XT)                                                               \
  do {                                                                        \
    if (acc_lds) LXE1(XT, 2, true);                                           \
    else LXE1(XT, 1, false);                                                  \
  } while (0)
  if (dt == ROW_BF16) LXE(uint16_t);
  else if (dt == ROW_F16) LXE(deep::f16_t);
  else LXE(uint32_t);
#undef LXE
#undef LXE1
  return hipGetLastError();
}

// entries per node of the eif deep pack's hyper array
int32_t eif_deep_hyper_stride(int32_t nnz) {
  return deep::eif_hyper_stride(nnz);
}

// lvl: the int2 records of launch_deep_level_order run with every slot's
// pre-order index as its threshold word and d = 0
void launch_eif_score_gather(const void* lvl, const int32_t* vw,
                             const int32_t* hidx, const int32_t* hw,
                             void* nodes, void* hyper, int32_t T, int32_t Tpad,
                             int32_t M0, int32_t M, int32_t nnz, int32_t d,
                             hipStream_t stream) {
  const int64_t total = (int64_t)Tpad * M;
  const int blocks =
      (int)std::min<int64_t>((total + DEEP_BT - 1) / DEEP_BT, 65535);
  hipLaunchKernelGGL(deep::eif_score_gather_kernel, dim3(blocks),
                     dim3(DEEP_BT), 0, stream, (const int2*)lvl, vw, hidx, hw,
                     (int2*)nodes, (int2*)hyper, T, Tpad, M0, M, nnz, d);
}

hipError_t launch_score_extended_deep(
    RowDtype dt, int rpt, int phase, const void* X, const void* nodes,
    const void* hyper, const int32_t* lds_levels, float* out, int64_t N,
    int32_t d, int32_t nnz, int64_t rs, int64_t cs, int32_t Tpad, int32_t M,
    int32_t S, int32_t height, float fT, float c_norm, int finalize,
    size_t lds, int blocks, hipStream_t stream) {
  if ((rpt != 1 && rpt != 2) || (phase != 1 && phase != 2 && phase != 4) ||
      Tpad % phase != 0)
    return hipErrorInvalidValue;
  hipError_t err = hipSuccess;
#define LSE1(XT, RPT, PH)                                                     \
  do {                                                                        \
    const void* fn =                                                          \
        (const void*)deep::score_extended_deep_kernel<XT, RPT, PH>;           \
    if (lds > 64 * 1024)                                                      \
      err = hipFuncSetAttribute(                                              \
          fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);          \
    if (err != hipSuccess) return err;                                        \
    hipLaunchKernelGGL((deep::score_extended_deep_kernel<XT, RPT, PH>),       \
                       dim3(blocks), dim3(DEEP_BT), lds, stream,              \
                       (const XT*)X, (const int2*)nodes, (const int2*)hyper,  \
                       lds_levels, out, N, d, nnz, Tpad, M, S, height, fT,    \
                       c_norm, finalize, rs, cs);                             \
  } while (0)
#define LSE2(XT, RPT)                                                         \
  do {                                                                        \
    if (phase == 4) LSE1(XT, RPT, 4);                                         \
    else if (phase == 2) LSE1(XT, RPT, 2);                                    \
    else LSE1(XT, RPT, 1);                                                    \
  } while (0)
#define LSE(XT)                                                               \
  do {                                                                        \
    if (rpt == 2) LSE2(XT, 2);                                                \
    else LSE2(XT, 1);                                                         \
  } while (0)
  if (dt == ROW_BF16) LSE(uint16_t);
  else if (dt == ROW_F16) LSE(deep::f16_t);
  else LSE(uint32_t);
#undef LSE
#undef LSE2
#undef LSE1
  return hipGetLastError();
}

}  // namespace ifa
