// MI355X (gfx950, CDNA4) exact TreeSHAP for standard isolation forests.
//
// The contract is docs/DESIGN.md §9: path-dependent Shapley values in the
// direct leaf-path form, all arithmetic float64 in one fixed order, BITWISE
// equal to cpu_engine.shap_values. The host builds the per-leaf tables once
// (cpu_engine.shap_tables, packed per row kind by gpu_engine); the kernel
// reproduces the loop and nothing else. It has no division except the
// finalize.
//
// Table stream, 8-byte words, trees back to back (tree t owns the words
// [tree_off[t], tree_off[t+1])), leaves in ascending node id:
//   leaf header : { f64 L , m }
//   m entries   : { f64 z , lo | hi << 32 , feature }
// o_k(x) = lo <= widen(key(x[feature])) <= hi, an INCLUSIVE interval of
// widened integer keys: lo is the max of the path's right-turn thresholds
// on that feature (0: none), hi the min of its left-turn thresholds minus 1
// (0xFFFFFFFF: none, which admits the NaN key, so NaN goes right). A left
// turn at threshold key 0 can never be taken: the host stores the empty
// interval lo = 1, hi = 0. No wrap-around anywhere.
//
// Rows are thread-owned (no atomics). A row's trees run one after another
// and a tree's leaves in order, so a block walks the table stream in
// lockstep: every table read is a wave-uniform broadcast and only o differs
// between lanes (selects, never branches). All loop bounds (m, cnt) are
// uniform too. c[] is a fixed array of 17 doubles, indexed by fully unrolled
// constants behind uniform guards so that it stays in registers.
//
// LDS tiles are feature-major, [column][256 rows]: a uniform column index
// makes every lane's access consecutive, conflict-free for the u16/u32 keys
// and for the float64 accumulators alike.
//
// TABLE_LDS: one tree's table staged per barrier pair; else read from
// global memory at wave-uniform addresses. ACC_LDS: float64 accumulators in
// an LDS tile, flushed coalesced; else a pre-zeroed global float64 scratch
// [N][d], thread-owned. rows_lds (run time): keys staged in LDS, else read
// from X and keyed per use (very wide rows).
//
// This TU is torch-free and stands alone: the few key helpers it shares with
// forest_kernels.hip are duplicated here (namespace ifa::shap) so that the
// other TU's code, and the native scorer that links only it, do not change.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "row_dtype.h"

namespace ifa {
namespace shap {

#define IFA_SHAP_MAXM 16

// IEEE fp16 bits as a type of their own; uint16_t means bf16 bits
enum class f16_t : uint16_t {};

// order-preserving key transforms (gpu_engine._key32 and friends): +-0
// collapse to the +0 key, NaN maps to the all-ones key
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

// 16-bit keys sit in the high half with the low bits saturated, as in the
// walks: the NaN key widens to 0xFFFFFFFF
__device__ __forceinline__ uint32_t widen_key(uint16_t k) {
  return ((uint32_t)k << 16) | 0xFFFFu;
}
__device__ __forceinline__ uint32_t widen_key(f16_t k) {
  return widen_key((uint16_t)k);
}
__device__ __forceinline__ uint32_t widen_key(uint32_t k) { return k; }

extern __shared__ __align__(16) unsigned char smem[];

template <typename KT, bool TABLE_LDS, bool ACC_LDS>
__global__ void __launch_bounds__(256) shap_forest_kernel(
    const KT* __restrict__ X,               // raw bf16/fp16/f32 bits
    const uint64_t* __restrict__ table,     // leaf-path stream (see above)
    const int64_t* __restrict__ tree_off,   // [T + 1], in words
    const double* __restrict__ wtab_g,      // [17][16] Shapley weights
    double* __restrict__ acc_g,             // [N][d] pre-zeroed (!ACC_LDS)
    float* __restrict__ out,                // [N][d]
    int64_t N, int32_t d, int32_t T, int32_t table_words, int32_t rows_lds,
    double dT, int32_t finalize, int64_t rs, int64_t cs) {
  const int tid = threadIdx.x;

  // LDS carve-up, 8-byte items first
  uint64_t* tlds = (uint64_t*)smem;  // [table_words] when TABLE_LDS
  double* wtab = (double*)(tlds + (TABLE_LDS ? table_words : 0));
  double* acc = wtab + 17 * IFA_SHAP_MAXM;  // [d][256] when ACC_LDS
  KT* keys = (KT*)(acc + (ACC_LDS ? (int64_t)d * 256 : 0));  // [d][256]

  for (int i = tid; i < 17 * IFA_SHAP_MAXM; i += 256) wtab[i] = wtab_g[i];

  for (int64_t row0 = (int64_t)blockIdx.x * 256; row0 < N;
       row0 += (int64_t)gridDim.x * 256) {
    const int rows_here = (int)min((int64_t)256, N - row0);
    const int64_t my_row = row0 + tid;
    const bool live = tid < rows_here;

    __syncthreads();  // previous tile's flush done
    if (rows_lds) {
      const uint32_t total = (uint32_t)rows_here * (uint32_t)d;
      if (rs == 1) {  // feature-major source: rows run fastest
        for (uint32_t g = tid; g < total; g += 256) {
          const int c = (int)(g / (uint32_t)rows_here);
          const int r = (int)(g % (uint32_t)rows_here);
          keys[c * 256 + r] = key_of_bits<KT>(X[(row0 + r) + (int64_t)c * cs]);
        }
      } else {
        for (uint32_t g = tid; g < total; g += 256) {
          const int r = (int)(g / (uint32_t)d), c = (int)(g % (uint32_t)d);
          keys[c * 256 + r] = key_of_bits<KT>(X[(row0 + r) * rs + c * cs]);
        }
      }
      // rows past the end of a short tile: any defined key will do, their
      // lanes compute along and store nothing
      if (!live)
        for (int c = 0; c < d; ++c) keys[c * 256 + tid] = (KT)0;
    }
    if (ACC_LDS)
      for (int c = 0; c < d; ++c) acc[c * 256 + tid] = 0.0;
    // (the barrier at the top of the tree loop orders these writes)

    for (int t = 0; t < T; ++t) {
      const int64_t w0 = tree_off[t];
      const int nwords = (int)(tree_off[t + 1] - w0);
      __syncthreads();  // tile staged / previous tree's readers done
      if (TABLE_LDS) {
        for (int i = tid; i < nwords; i += 256) tlds[i] = table[w0 + i];
        __syncthreads();
      }
      const uint64_t* tb = TABLE_LDS ? tlds : table + w0;

      int p = 0;
      while (p < nwords) {  // leaves, ascending node id
        const double L = __longlong_as_double((long long)tb[p]);
        const int m = (int)(uint32_t)tb[p + 1];
        const uint64_t* en = tb + p + 2;
        p += 2 + 3 * m;

        // o bits of this leaf's entries for this lane's row
        uint32_t omask = 0;
        for (int k = 0; k < m; ++k) {
          const uint64_t iv = en[3 * k + 1];
          const int f = (int)(uint32_t)en[3 * k + 2];
          uint32_t key;
          if (rows_lds) {
            key = widen_key(keys[f * 256 + tid]);
          } else {
            key = live ? widen_key(key_of_bits<KT>(X[my_row * rs + f * cs]))
                       : 0u;
          }
          const bool o = (uint32_t)iv <= key && key <= (uint32_t)(iv >> 32);
          omask |= (o ? 1u : 0u) << k;
        }

        for (int a = 0; a < m; ++a) {
          double c[IFA_SHAP_MAXM + 1];
          c[0] = 1.0;
#pragma unroll
          for (int k = 1; k <= IFA_SHAP_MAXM; ++k) c[k] = 0.0;
          int cnt = 0;
          for (int b = 0; b < m; ++b) {
            if (b == a) continue;
            const double zb = __longlong_as_double((long long)en[3 * b]);
            const bool ob = (omask >> b) & 1u;
#pragma unroll
            for (int k = IFA_SHAP_MAXM - 1; k >= 0; --k) {
              if (k <= cnt) {  // uniform
                const double s = __dadd_rn(c[k + 1], c[k]);
                c[k + 1] = ob ? s : c[k + 1];
                c[k] = __dmul_rn(c[k], zb);
              }
            }
            ++cnt;
          }
          double W = 0.0;
          const double* wm = wtab + m * IFA_SHAP_MAXM;
#pragma unroll
          for (int k = 0; k < IFA_SHAP_MAXM; ++k)
            if (k < m) W = __dadd_rn(W, __dmul_rn(c[k], wm[k]));  // uniform

          const double za = __longlong_as_double((long long)en[3 * a]);
          const int fa = (int)(uint32_t)en[3 * a + 2];
          const double oa = ((omask >> a) & 1u) ? 1.0 : 0.0;
          const double term =
              __dmul_rn(__dmul_rn(L, __dsub_rn(oa, za)), W);
          if (ACC_LDS) {
            double* q = acc + fa * 256 + tid;
            *q = __dadd_rn(*q, term);
          } else if (live) {
            double* q = acc_g + my_row * d + fa;
            *q = __dadd_rn(*q, term);
          }
        }
      }
    }

    if (ACC_LDS) {
      __syncthreads();  // every row's accumulators final
      const uint32_t total = (uint32_t)rows_here * (uint32_t)d;
      for (uint32_t g = tid; g < total; g += 256) {
        const int r = (int)(g / (uint32_t)d), c = (int)(g % (uint32_t)d);
        const double v = acc[c * 256 + r];
        out[(row0 + r) * d + c] = finalize ? (float)(v / dT) : (float)v;
      }
    } else if (live) {
      for (int c = 0; c < d; ++c) {
        const double v = acc_g[my_row * d + c];
        out[my_row * d + c] = finalize ? (float)(v / dT) : (float)v;
      }
    }
  }
}

}  // namespace shap

// host-side launcher (bindings.cpp is compiled by g++)
void launch_shap_forest(RowDtype dt, bool table_lds, bool acc_lds,
                        const void* X, const void* table,
                        const int64_t* tree_off, const double* wtab,
                        double* acc_g, float* out, int64_t N, int32_t d,
                        int64_t rs, int64_t cs, int32_t T, int32_t table_words,
                        int rows_lds, int finalize, size_t lds, int blocks,
                        hipStream_t stream) {
#define LSH1(KT, TL, AL)                                                      \
  do {                                                                        \
    if (lds > 64 * 1024)                                                      \
      (void)hipFuncSetAttribute(                                              \
          (const void*)shap::shap_forest_kernel<KT, TL, AL>,                  \
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);              \
    hipLaunchKernelGGL((shap::shap_forest_kernel<KT, TL, AL>), dim3(blocks),  \
                       dim3(256), lds, stream, (const KT*)X,                  \
                       (const uint64_t*)table, tree_off, wtab, acc_g, out, N, \
                       d, T, table_words, rows_lds, (double)T, finalize, rs,  \
                       cs);                                                   \
  } while (0)
#define LSH(KT)                                                               \
  do {                                                                        \
    if (table_lds && acc_lds) LSH1(KT, true, true);                           \
    else if (table_lds) LSH1(KT, true, false);                                \
    else if (acc_lds) LSH1(KT, false, true);                                  \
    else LSH1(KT, false, false);                                              \
  } while (0)
  if (dt == ROW_BF16) LSH(uint16_t);
  else if (dt == ROW_F16) LSH(shap::f16_t);
  else LSH(uint32_t);
#undef LSH
#undef LSH1
}

}  // namespace ifa
