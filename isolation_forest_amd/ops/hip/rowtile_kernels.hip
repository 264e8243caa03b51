// Dense rows past the key tile of the row-per-thread walks
// (docs/DESIGN.md §3d).
//
// score_forest_v4 and score_forest_heap give a thread a row and keep 256 or
// 512 rows' keys in LDS; past d = 295 (16-bit rows) or d = 147 (f32 rows)
// that tile does not fit and every visited key used to come from global
// memory. score_forest_rowtile_kernel takes the split of the CSR walk
// (csr_kernels.hip, §3c) to dense input: a block of 256 threads holds the
// FULL key vectors of R rows (R a power of two, 4 .. 256) and takes its
// parallelism from the trees.
//
//   tile   row-major [R][SW words] in the row kind's key type (u16 for
//          bf16/fp16, u32 for f32), column d the all-ones leaf sentinel.
//          SW >= the words of d + 1 keys and is odd, so consecutive rows
//          start in different banks.
//   stage  dense: every cell 0 .. d is overwritten, no zero fill, no scatter.
//          Row-major X (cs == 1): the G = 256 / R lanes of a row (always
//          inside one wave) read consecutive elements of their own row and
//          store consecutive LDS words. 16-bit rows that start on a 4-byte
//          boundary are read and stored a word (two keys) at a time; rows
//          with an odd element offset take the element loop.
//          Feature-major X (rs == 1): the block runs the flat index of the
//          [R][d] tile row-fastest, so a wave reads runs of consecutive
//          elements of one column; any lane writes any row, and the barrier
//          after the fill covers that.
//          Rows past N get the key of +0.0 and are never stored. X is read
//          in place through its two element strides with 64-bit offsets.
//   walk   per barrier phase PH = m * G trees (m <= 4) are staged linearly
//          into LDS (NODES_LDS) or read in place from global memory / L2.
//          Lane g of a group walks trees g, g + G, ... of the phase, up to
//          four chains in flight; each trip issues all record reads, then
//          all key reads, then the VALU. Fixed trip count: the pack's height.
//   sum    every walk's leaf value goes to an LDS slot [c][r][g]; after the
//          phase lane 0 of the group adds the phase's values to the row's
//          f32 running sum with __fadd_rn in ascending tree order. Trees
//          past the pack add +0.0. That order is cpu_engine.path_lengths',
//          so the result is bitwise every other dense route's.
//
// The walk and the sum repeat csr_kernels.hip's on purpose: that file and its
// compiled figures stay as they were.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "row_dtype.h"

namespace ifa {
namespace rowtile {

#define RT_BT 256
#define RT_C 4  // most chains a lane walks per phase: PH <= RT_C * G

// fp16 bits as a type of their own, as in forest_kernels.hip
enum class f16_t : uint16_t {};

// order-preserving keys (gpu_engine._key32 and friends): +-0 collapse to the
// +0 key, NaN is the all-ones key and never compares below a threshold
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

__device__ __forceinline__ f16_t key_of_bits(f16_t b) {
  return (f16_t)(uint16_t)key16_f16((uint32_t)(uint16_t)b);
}
__device__ __forceinline__ uint16_t key_of_bits(uint16_t b) {
  return (uint16_t)key16((uint32_t)b);
}
__device__ __forceinline__ uint32_t key_of_bits(uint32_t b) { return key32(b); }

// the keys of the two 16-bit elements of one 32-bit word of a row
template <typename KT>
__device__ __forceinline__ uint32_t key_pair(uint32_t w) {
  const uint32_t lo = (uint32_t)(uint16_t)key_of_bits((KT)(uint16_t)w);
  const uint32_t hi = (uint32_t)(uint16_t)key_of_bits((KT)(uint16_t)(w >> 16));
  return lo | (hi << 16);
}
template <>
__device__ __forceinline__ uint32_t key_pair<uint32_t>(uint32_t w) {
  return key32(w);  // never taken: f32 rows have one key a word
}

// 16-bit keys are compared in the high half with the low half saturated, so
// the sentinel widens to 0xFFFFFFFF (thresholds are key << 16)
__device__ __forceinline__ uint32_t widen_key(uint16_t k) {
  return ((uint32_t)k << 16) | 0xFFFFu;
}
__device__ __forceinline__ uint32_t widen_key(f16_t k) {
  return widen_key((uint16_t)k);
}
__device__ __forceinline__ uint32_t widen_key(uint32_t k) { return k; }

__device__ __forceinline__ int rec_feat(int x) { return x & 0xFFF; }
__device__ __forceinline__ int rec_link(int x) { return (x >> 12) & 0x7FFF; }

extern __shared__ __align__(16) unsigned char smem[];

template <typename KT, int G, bool NODES_LDS>
__global__ void __launch_bounds__(RT_BT) score_forest_rowtile_kernel(
    const KT* __restrict__ X,          // raw bf16/fp16/f32 bits, strided
    int64_t rs, int64_t cs,            // element strides of a row, a column
    const int2* __restrict__ nodes,    // [Tpad][max_nodes] level-order v4
    const int32_t* __restrict__ ncnt,  // [Tpad]
    float* __restrict__ out,           // [N] (path sum or score)
    int64_t N, int32_t d, int32_t SW, int32_t Tpad, int32_t max_nodes,
    int32_t height, int32_t PH, float fT, float c_norm, int32_t finalize) {
  constexpr int R = RT_BT / G;
  constexpr int EPW = 4 / (int)sizeof(KT);  // keys per 32-bit word
  const int tid = threadIdx.x;
  const int r = tid / G, g = tid % G;
  const int cmax = PH / G;  // chains a lane walks per phase (1 .. RT_C)

  int2* tlds = (int2*)smem;  // [PH * max_nodes] when NODES_LDS
  float* slots = (float*)(tlds + (NODES_LDS ? (size_t)PH * max_nodes : 0));
  uint32_t* tile32 = (uint32_t*)(slots + RT_C * RT_BT);  // [R][SW]
  uint32_t* row32 = tile32 + (size_t)r * SW;
  KT* rowk = (KT*)row32;
  const KT ones = (KT)~(uint32_t)0;  // the sentinel key
  const KT zero = (KT)0;             // bits of +0.0

  for (int64_t row0 = (int64_t)blockIdx.x * R; row0 < N;
       row0 += (int64_t)gridDim.x * R) {
    __syncthreads();  // the previous tile's walks are done
    const int64_t row = row0 + r;
    if (cs == 1) {
      // row-major: a group fills its own row, lane g the cells g, g + G, ...
      const bool rv = row < N;
      const KT* xr = X + (rv ? row : 0) * rs;
      int c0 = 0;
      if (EPW == 2 && ((uintptr_t)xr & 3) == 0) {
        const uint32_t* xw = (const uint32_t*)xr;
        const int nw = d >> 1;
        for (int w = g; w < nw; w += G)
          row32[w] = key_pair<KT>(rv ? xw[w] : 0u);
        c0 = nw << 1;
      }
      for (int c = c0 + g; c < d; c += G)
        rowk[c] = key_of_bits(rv ? xr[c] : zero);
      if (g == 0) rowk[d] = ones;
    } else {
      // feature-major: flat index over [d][R], row-fastest
      KT* tilek = (KT*)tile32;
      const int total = d * R;
      for (int i = tid; i < total; i += RT_BT) {
        const int rr = i % R, c = i / R;
        const int64_t rw = row0 + rr;
        const KT v = rw < N ? X[rw * rs + (int64_t)c * cs] : zero;
        tilek[(size_t)rr * SW * EPW + c] = key_of_bits(v);
      }
      if (tid < R) tilek[(size_t)tid * SW * EPW + d] = ones;
    }
    __syncthreads();

    float psum = 0.f;
    for (int t0 = 0; t0 < Tpad; t0 += PH) {
      const int ph_here = min(PH, Tpad - t0);
      if (NODES_LDS) {
        __syncthreads();  // the previous phase's walks are done
        for (int s = 0; s < ph_here; ++s) {
          const int ncs = min(ncnt[t0 + s], max_nodes);
          const int2* ss = nodes + (int64_t)(t0 + s) * max_nodes;
          int2* dd = tlds + (size_t)s * max_nodes;
          for (int i = tid; i < ncs; i += RT_BT) dd[i] = ss[i];
        }
        __syncthreads();
      }

      // chain c walks tree g + c * G of the phase; a chain past the phase
      // walks tree 0 and its value is dropped
      bool live[RT_C];
      int toff[RT_C];           // LDS: record offset of the tree
      const int2* tglb[RT_C];   // global: the tree's records
      int cur[RT_C];
#pragma unroll
      for (int c = 0; c < RT_C; ++c) {
        const int k = g + c * G;
        live[c] = k < ph_here;
        const int kk = live[c] ? k : 0;
        toff[c] = kk * max_nodes;
        tglb[c] = nodes + (int64_t)(t0 + kk) * max_nodes;
        cur[c] = 0;
      }
      for (int it = 0; it < height; ++it) {
        // three passes, so that the reads of all chains are in flight
        // together: records, keys, then the VALU
        int2 nd[RT_C];
#pragma unroll
        for (int c = 0; c < RT_C; ++c)
          if (c < cmax)
            nd[c] = NODES_LDS ? tlds[toff[c] + cur[c]] : tglb[c][cur[c]];
        KT kr[RT_C];
#pragma unroll
        for (int c = 0; c < RT_C; ++c)
          if (c < cmax) kr[c] = rowk[min(rec_feat(nd[c].x), d)];
#pragma unroll
        for (int c = 0; c < RT_C; ++c)
          if (c < cmax)
            // link = right child, left = link - 1; a leaf reads the
            // sentinel, compares false and keeps link = itself
            cur[c] = rec_link(nd[c].x) -
                     (widen_key(kr[c]) < (uint32_t)nd[c].y);
      }
#pragma unroll
      for (int c = 0; c < RT_C; ++c)
        if (c < cmax) {
          const int y =
              (NODES_LDS ? tlds[toff[c] + cur[c]] : tglb[c][cur[c]]).y;
          // slot of tree k = c * G + g of row r: [c][r][g]
          slots[c * RT_BT + tid] = live[c] ? __int_as_float(y) : 0.f;
        }
      __syncthreads();
      if (g == 0) {
        const float* sr = slots + r * G;
        for (int c = 0; c < cmax; ++c)
#pragma unroll
          for (int j = 0; j < G; ++j)
            psum = __fadd_rn(psum, sr[c * RT_BT + j]);
      }
      __syncthreads();  // slots are free for the next phase
    }

    if (g == 0 && row < N) {
      if (finalize) {
        const float mean32 = (float)((double)psum / (double)fT);
        const double ratio = (double)mean32 / (double)c_norm;
        out[row] = (float)exp2(-ratio);
      } else {
        out[row] = psum;
      }
    }
  }
}

}  // namespace rowtile

hipError_t launch_score_forest_rowtile(
    RowDtype dt, int G, bool nodes_lds, const void* X, int64_t rs, int64_t cs,
    const void* nodes, const int32_t* ncnt, float* out, int64_t N, int32_t d,
    int32_t SW, int32_t Tpad, int32_t max_nodes, int32_t height, int32_t PH,
    float fT, float c_norm, int finalize, size_t lds, int blocks,
    hipStream_t stream) {
  hipError_t err = hipSuccess;
#define LR1(KT, GG, NL)                                                       \
  do {                                                                        \
    const void* fn =                                                          \
        (const void*)rowtile::score_forest_rowtile_kernel<KT, GG, NL>;        \
    if (lds > 64 * 1024)                                                      \
      err = hipFuncSetAttribute(                                              \
          fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);          \
    if (err != hipSuccess) return err;                                        \
    hipLaunchKernelGGL((rowtile::score_forest_rowtile_kernel<KT, GG, NL>),    \
                       dim3(blocks), dim3(RT_BT), lds, stream, (const KT*)X,  \
                       rs, cs, (const int2*)nodes, ncnt, out, N, d, SW, Tpad, \
                       max_nodes, height, PH, fT, c_norm, finalize);          \
  } while (0)
#define LR_NL(KT, GG)                                                         \
  do {                                                                        \
    if (nodes_lds) LR1(KT, GG, true);                                         \
    else LR1(KT, GG, false);                                                  \
  } while (0)
#define LR(KT)                                                                \
  do {                                                                        \
    switch (G) {                                                              \
      case 1: LR_NL(KT, 1); break;                                            \
      case 2: LR_NL(KT, 2); break;                                            \
      case 4: LR_NL(KT, 4); break;                                            \
      case 8: LR_NL(KT, 8); break;                                            \
      case 16: LR_NL(KT, 16); break;                                          \
      case 32: LR_NL(KT, 32); break;                                          \
      case 64: LR_NL(KT, 64); break;                                          \
      default: return hipErrorInvalidValue;                                   \
    }                                                                         \
  } while (0)
  if (dt == ROW_BF16) LR(uint16_t);
  else if (dt == ROW_F16) LR(rowtile::f16_t);
  else LR(uint32_t);
#undef LR
#undef LR_NL
#undef LR1
  return hipGetLastError();
}

}  // namespace ifa
