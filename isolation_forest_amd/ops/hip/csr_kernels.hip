// Sparse CSR input for standard forests (docs/DESIGN.md §3c).
//
// score_forest_csr_kernel walks the level-order v4 records of
// forest_kernels.hip ({feat | link << 12, key threshold}; leaves self-loop on
// the sentinel feature d; a step is cur = link - (key < thr)) over rows given
// as CSR, without a dense copy of the matrix. The dense walks give a thread a
// row and keep 256 or 512 rows' keys in LDS, which stops fitting near d = 290
// (16-bit rows). Here a block holds the FULL key vectors of R rows (R a power
// of two, 4 .. 256) and takes its parallelism from the trees:
//
//   tile   row-major [R][SW words] in the row kind's key type (u16 for
//          bf16/fp16, u32 for f32), column d the all-ones leaf sentinel.
//          SW >= the words of d + 1 keys and is odd, so consecutive rows
//          start in different banks.
//   stage  a row's group of G = 256 / R lanes (always inside one wave) fills
//          its row with the key of +0.0 and the sentinel; after a barrier it
//          loops over crow[row] .. crow[row + 1], consecutive lanes reading
//          consecutive entries, and stores key_of_bits(value) at [r][col]
//          where col < d. No search and no atomics: a row's entries are
//          written by its own group only, and validated input has no
//          duplicate column.
//   walk   per barrier phase PH = m * G trees (m <= 4) are staged linearly
//          into LDS (NODES_LDS) or read in place from global memory / L2.
//          Lane g of a group walks trees g, g + G, ... of the phase, up to
//          four chains in flight, reads batched as in v4 (records, keys,
//          VALU). The loop is fixed-trip over the pack's height.
//   sum    every walk's leaf value goes to an LDS slot; after the phase lane
//          0 of the group adds the phase's values to the row's f32 running
//          sum with __fadd_rn in ascending tree order. Trees past the pack
//          add +0.0. That order is cpu_engine.path_lengths', so the result
//          is bitwise the dense walks' on X.to_dense().
//
// bag_gather_csr_kernel scatters CSR rows into the f32 [T, n, d] bag tensor
// of bag_gather (zeroed by the binding), one wave per bag row, for the
// unchanged LDS tree builders.
//
// Every index read from the matrix is clamped or predicated (entry ranges to
// [0, nnz], columns to < d, bag rows to < N), so unvalidated input cannot
// address outside the arrays; gpu_engine._csr_parts refuses it beforehand.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "row_dtype.h"

namespace ifa {
namespace csr {

#define CSR_BT 256
#define CSR_C 4  // most chains a lane walks per phase: PH <= CSR_C * G

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

// exact widening of a stored value to f32
__device__ __forceinline__ float widen_value(float v) { return v; }
__device__ __forceinline__ float widen_value(uint16_t v) {
  return __uint_as_float((uint32_t)v << 16);
}
__device__ __forceinline__ float widen_value(f16_t v) {
  union { uint16_t u; _Float16 h; } cv;
  cv.u = (uint16_t)v;
  return (float)cv.h;
}

extern __shared__ __align__(16) unsigned char smem[];

template <typename KT, typename IT, int G, bool NODES_LDS>
__global__ void __launch_bounds__(CSR_BT) score_forest_csr_kernel(
    const IT* __restrict__ crow,       // [N + 1]
    const IT* __restrict__ col,        // [nnz]
    const KT* __restrict__ values,     // [nnz] raw bf16/fp16/f32 bits
    int64_t nnz,
    const int2* __restrict__ nodes,    // [Tpad][max_nodes] level-order v4
    const int32_t* __restrict__ ncnt,  // [Tpad]
    float* __restrict__ out,           // [N] (path sum or score)
    int64_t N, int32_t d, int32_t SW, int32_t Tpad, int32_t max_nodes,
    int32_t height, int32_t PH, float fT, float c_norm, int32_t finalize) {
  constexpr int R = CSR_BT / G;
  constexpr int EPW = 4 / (int)sizeof(KT);  // keys per 32-bit word
  const int tid = threadIdx.x;
  const int r = tid / G, g = tid % G;
  const int cmax = PH / G;  // chains a lane walks per phase (1 .. CSR_C)

  int2* tlds = (int2*)smem;  // [PH * max_nodes] when NODES_LDS
  float* slots = (float*)(tlds + (NODES_LDS ? (size_t)PH * max_nodes : 0));
  uint32_t* row32 = (uint32_t*)(slots + CSR_C * CSR_BT) + (size_t)r * SW;
  KT* rowk = (KT*)row32;

  // the word that holds column d: the sentinel, next to column d - 1 (the
  // key of +0.0) or to a padding column
  const uint32_t zero_word = sizeof(KT) == 4 ? 0x80000000u : 0x80008000u;
  const int sent_word = d / EPW;
  const uint32_t sent_val = sizeof(KT) == 4 ? 0xFFFFFFFFu
                            : (d & 1)       ? 0xFFFF8000u
                                            : 0x8000FFFFu;

  for (int64_t row0 = (int64_t)blockIdx.x * R; row0 < N;
       row0 += (int64_t)gridDim.x * R) {
    __syncthreads();  // the previous tile's walks are done
    for (int w = g; w < SW; w += G)
      row32[w] = w == sent_word ? sent_val : zero_word;
    __syncthreads();
    const int64_t row = row0 + r;
    if (row < N) {  // rows past N keep the all-zero row and are never stored
      const int64_t lo = max((int64_t)crow[row], (int64_t)0);
      const int64_t hi = min((int64_t)crow[row + 1], nnz);
#pragma unroll 2
      for (int64_t e = lo + g; e < hi; e += G) {
        const int64_t c = (int64_t)col[e];
        const KT v = values[e];
        if ((uint64_t)c < (uint64_t)d) rowk[c] = key_of_bits(v);
      }
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
          for (int i = tid; i < ncs; i += CSR_BT) dd[i] = ss[i];
        }
        __syncthreads();
      }

      // chain c walks tree g + c * G of the phase; a chain past the phase
      // walks tree 0 and its value is dropped
      bool live[CSR_C];
      int toff[CSR_C];           // LDS: record offset of the tree
      const int2* tglb[CSR_C];   // global: the tree's records
      int cur[CSR_C];
#pragma unroll
      for (int c = 0; c < CSR_C; ++c) {
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
        int2 nd[CSR_C];
#pragma unroll
        for (int c = 0; c < CSR_C; ++c)
          if (c < cmax)
            nd[c] = NODES_LDS ? tlds[toff[c] + cur[c]] : tglb[c][cur[c]];
        KT kr[CSR_C];
#pragma unroll
        for (int c = 0; c < CSR_C; ++c)
          if (c < cmax) kr[c] = rowk[min(rec_feat(nd[c].x), d)];
#pragma unroll
        for (int c = 0; c < CSR_C; ++c)
          if (c < cmax)
            // link = right child, left = link - 1; a leaf reads the
            // sentinel, compares false and keeps link = itself
            cur[c] = rec_link(nd[c].x) -
                     (widen_key(kr[c]) < (uint32_t)nd[c].y);
      }
#pragma unroll
      for (int c = 0; c < CSR_C; ++c)
        if (c < cmax) {
          const int y =
              (NODES_LDS ? tlds[toff[c] + cur[c]] : tglb[c][cur[c]]).y;
          // slot of tree k = c * G + g of row r: [c][r][g]
          slots[c * CSR_BT + tid] = live[c] ? __int_as_float(y) : 0.f;
        }
      __syncthreads();
      if (g == 0) {
        const float* sr = slots + r * G;
        for (int c = 0; c < cmax; ++c)
#pragma unroll
          for (int j = 0; j < G; ++j)
            psum = __fadd_rn(psum, sr[c * CSR_BT + j]);
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

template <typename XT, typename IT>
__global__ void __launch_bounds__(CSR_BT) bag_gather_csr_kernel(
    const IT* __restrict__ crow, const IT* __restrict__ col,
    const XT* __restrict__ values, int64_t nnz, int64_t N,
    const int64_t* __restrict__ bag_idx,  // [T * n]
    float* __restrict__ bags,             // [T * n][d], zero on entry
    int64_t TN, int64_t d) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (CSR_BT / 64);
  for (int64_t s = (int64_t)blockIdx.x * (CSR_BT / 64) + (threadIdx.x >> 6);
       s < TN; s += waves) {
    const int64_t row = bag_idx[s];
    if ((uint64_t)row >= (uint64_t)N) continue;
    const int64_t lo = max((int64_t)crow[row], (int64_t)0);
    const int64_t hi = min((int64_t)crow[row + 1], nnz);
    float* dst = bags + s * d;
    for (int64_t e = lo + lane; e < hi; e += 64) {
      const int64_t c = (int64_t)col[e];
      const XT v = values[e];
      if ((uint64_t)c < (uint64_t)d) dst[c] = widen_value(v);
    }
  }
}

}  // namespace csr

hipError_t launch_score_forest_csr(
    RowDtype dt, bool idx64, int G, bool nodes_lds, const void* crow,
    const void* col, const void* values, int64_t nnz, const void* nodes,
    const int32_t* ncnt, float* out, int64_t N, int32_t d, int32_t SW,
    int32_t Tpad, int32_t max_nodes, int32_t height, int32_t PH, float fT,
    float c_norm, int finalize, size_t lds, int blocks, hipStream_t stream) {
  hipError_t err = hipSuccess;
#define LC1(KT, IT, GG, NL)                                                   \
  do {                                                                        \
    const void* fn =                                                          \
        (const void*)csr::score_forest_csr_kernel<KT, IT, GG, NL>;            \
    if (lds > 64 * 1024)                                                      \
      err = hipFuncSetAttribute(                                              \
          fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);          \
    if (err != hipSuccess) return err;                                        \
    hipLaunchKernelGGL((csr::score_forest_csr_kernel<KT, IT, GG, NL>),        \
                       dim3(blocks), dim3(CSR_BT), lds, stream,               \
                       (const IT*)crow, (const IT*)col, (const KT*)values,    \
                       nnz, (const int2*)nodes, ncnt, out, N, d, SW, Tpad,    \
                       max_nodes, height, PH, fT, c_norm, finalize);          \
  } while (0)
#define LC_NL(KT, IT, GG)                                                     \
  do {                                                                        \
    if (nodes_lds) LC1(KT, IT, GG, true);                                     \
    else LC1(KT, IT, GG, false);                                              \
  } while (0)
#define LC_G(KT, IT)                                                          \
  do {                                                                        \
    switch (G) {                                                              \
      case 1: LC_NL(KT, IT, 1); break;                                        \
      case 2: LC_NL(KT, IT, 2); break;                                        \
      case 4: LC_NL(KT, IT, 4); break;                                        \
      case 8: LC_NL(KT, IT, 8); break;                                        \
      case 16: LC_NL(KT, IT, 16); break;                                      \
      case 32: LC_NL(KT, IT, 32); break;                                      \
      case 64: LC_NL(KT, IT, 64); break;                                      \
      default: return hipErrorInvalidValue;                                   \
    }                                                                         \
  } while (0)
#define LC(KT)                                                                \
  do {                                                                        \
    if (idx64) LC_G(KT, int64_t);                                             \
    else LC_G(KT, int32_t);                                                   \
  } while (0)
  if (dt == ROW_BF16) LC(uint16_t);
  else if (dt == ROW_F16) LC(csr::f16_t);
  else LC(uint32_t);
#undef LC
#undef LC_G
#undef LC_NL
#undef LC1
  return hipGetLastError();
}

hipError_t launch_bag_gather_csr(RowDtype dt, bool idx64, const void* crow,
                                 const void* col, const void* values,
                                 int64_t nnz, int64_t N,
                                 const int64_t* bag_idx, float* bags,
                                 int64_t TN, int64_t d, int blocks,
                                 hipStream_t stream) {
#define LG1(XT, IT)                                                           \
  hipLaunchKernelGGL((csr::bag_gather_csr_kernel<XT, IT>), dim3(blocks),      \
                     dim3(CSR_BT), 0, stream, (const IT*)crow,                \
                     (const IT*)col, (const XT*)values, nnz, N, bag_idx,      \
                     bags, TN, d)
#define LG(XT)                                                                \
  do {                                                                        \
    if (idx64) LG1(XT, int64_t);                                              \
    else LG1(XT, int32_t);                                                    \
  } while (0)
  if (dt == ROW_BF16) LG(uint16_t);
  else if (dt == ROW_F16) LG(csr::f16_t);
  else LG(float);
#undef LG
#undef LG1
  return hipGetLastError();
}

}  // namespace ifa
