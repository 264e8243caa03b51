// MI355X (gfx950, CDNA4) per-feature attribution for extended forests whose
// whole tree fits in LDS and whose hyperplanes are coordinate-sorted: the
// default maxSamples = 256 model, fully extended or wide enough to densify
// (docs/DESIGN.md §8). BITWISE equal to
// cpu_engine.feature_contributions_extended, like explain_extended_kernel,
// which this route replaces where gpu_engine.extended_explain_route says
// "dense".
//
// Pack ("eif_explain_dense", D), D in {8, 16, 32} the padded row width:
//   nodes int2 [T][max_nodes]   x = right | slot << 16, y = f32 offset bits
//   rows  f32  [T][MI][3][D]    per INTERNAL node (slot = its rank among the
//                               tree's internal nodes, pre-order): the dense
//                               weight row, the delta_left share row and the
//                               delta_right share row
// right is the pre-order id of the right child (15 bits; the left child is
// id + 1). A leaf or pad record has right = its own id, slot 0 and offset 0:
// a chain that reaches it rests there. Columns no hyperplane selects, and
// pad columns j >= d, hold weight +0.0 and share +0.0.
//
// explain_extended_dense_kernel<KT, D, RPT, BT>: a block of BT threads owns
// a tile of RPT * BT rows. A thread widens its rows to f32 once and keeps
// them, with D f32 accumulators a row, in registers for the whole tree loop
// (every index an unrolled constant: no LDS tile, no global read-modify-
// write, no atomics, no scratch). One tree a barrier phase is staged in LDS:
// the records, then the three rows of each internal node back to back, a row
// D/4 + 1 float4s apart so that a node's block starts an odd number of
// float4s after its neighbour's and the b128 reads of lanes at different
// nodes spread over the banks. A visit of a live chain is
//   pass 1  dot = fadd(dot, fmul(w_j, x_j)) from 0.f in ascending j: one
//           chain, the oracle's order (its coordinates ascend, and a zero
//           weight adds +-0.0 to a sum that is never -0.0);
//   side    left = dot < offset (NaN goes right);
//   pass 2  acc_j = fadd(acc_j, share_j) over the taken side's row only, D
//           independent adds (a cell gets one add a node, so every cell's
//           adds come in tree order, root to leaf).
// A chain resting at a leaf skips both passes under the exec mask, so its
// lane issues no LDS read. The walk is fixed-trip over the forest's height.
// The accumulators are written to out[N, d] once a tile.
//
// This TU is torch-free and stands alone, like deep_kernels.hip: the row
// helpers it shares with forest_kernels.hip are duplicated (namespace
// ifa::exd) so that the other TU, and the native scorer that links only it,
// do not change.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "row_dtype.h"

namespace ifa {
namespace exd {

// IEEE fp16 bits as a type of their own; uint16_t means bf16 bits
enum class f16_t : uint16_t {};

// exact widenings: bf16 is a shift, every fp16 (subnormals too) is an f32
__device__ __forceinline__ float widen(uint16_t b) {
  return __uint_as_float((uint32_t)b << 16);
}
__device__ __forceinline__ float widen(f16_t b) {
  union { uint16_t u; _Float16 h; } cv;
  cv.u = (uint16_t)b;
  return (float)cv.h;
}
__device__ __forceinline__ float widen(float v) { return v; }

// f32 quotient that is correctly rounded by construction (f64 divide, one
// rounding: 53 >= 2*24+2), numpy's f32 divide bit for bit; see
// forest_kernels.hip
__device__ __forceinline__ float div32_exact(float a, float b) {
  return (float)((double)a / (double)b);
}

__device__ __forceinline__ int rec_right(int x) { return x & 0x7FFF; }
__device__ __forceinline__ int rec_slot(int x) {
  return (int)((uint32_t)x >> 16);
}

extern __shared__ __align__(16) unsigned char smem[];

// The adds of pass 2 and of neighbouring rows are independent, and the
// compiler would pair them into packed instructions; the walk keeps one
// scalar v_mul_f32 / v_add_f32 per term.
#if defined(__HIP_DEVICE_COMPILE__)
#define EXD_SCALAR_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define EXD_SCALAR_F32  // the host pass compiles only the launch stub
#endif

// float4s of one LDS row, and of the three rows of one internal node
template <int D>
struct Stage {
  static constexpr int ROW4 = D / 4 + 1;
  static constexpr int NODE4 = 3 * ROW4;  // 9, 15, 27: odd
};

template <typename KT, int D, int RPT, int BT>
__global__ void EXD_SCALAR_F32 __launch_bounds__(BT)
explain_extended_dense_kernel(
    const KT* __restrict__ X,           // raw bf16/fp16/f32 rows
    const int2* __restrict__ nodes,     // [T][max_nodes]
    const float4* __restrict__ rows,    // [T][max_internal][3][D / 4]
    const int32_t* __restrict__ ncnt,   // [T] live records
    const int32_t* __restrict__ icnt,   // [T] internal nodes
    float* __restrict__ out,            // [N][d]
    int64_t N, int32_t d, int64_t rs, int64_t cs, int32_t T, int32_t max_nodes,
    int32_t max_internal, int32_t height, float fT, int32_t finalize) {
  constexpr int ROW4 = Stage<D>::ROW4;
  constexpr int NODE4 = Stage<D>::NODE4;
  constexpr int Q = D / 4;             // float4s of a packed row
  constexpr int CW4 = (D >= 32) ? 2 : Q;  // float4s read ahead of their use
  constexpr int FS = RPT * BT;
  const int tid = threadIdx.x;

  // the row base is an offset from smem, not a rounded-up integer cast: the
  // cast would lose the LDS address space and make every read a flat load
  int2* tlds = (int2*)smem;                                // [max_nodes]
  float4* rlds = (float4*)smem + ((max_nodes + 1) >> 1);   // 16-byte aligned

  for (int64_t block_row0 = (int64_t)blockIdx.x * FS; block_row0 < N;
       block_row0 += (int64_t)gridDim.x * FS) {
    float x[RPT][D], acc[RPT][D];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t my_row = block_row0 + tid + r * BT;
      const bool ok = my_row < N;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        x[r][j] = (ok && j < d) ? widen(X[my_row * rs + j * cs]) : 0.f;
        acc[r][j] = 0.f;
      }
    }

    for (int t = 0; t < T; ++t) {
      __syncthreads();  // the previous tree's readers are done
      {
        const int nc = ncnt[t];
        const int2* ss = nodes + (int64_t)t * max_nodes;
        for (int i = tid; i < nc; i += BT) tlds[i] = ss[i];
        // packed rows of Q float4s -> LDS rows ROW4 apart; the three rows
        // of a node are consecutive in both
        const float4* ws = rows + (int64_t)t * max_internal * (3 * Q);
        const int total4 = icnt[t] * (3 * Q);
        for (int g = tid; g < total4; g += BT)
          rlds[(g / Q) * ROW4 + (g % Q)] = ws[g];
      }
      __syncthreads();

      int cur[RPT];
#pragma unroll
      for (int r = 0; r < RPT; ++r) cur[r] = 0;

      for (int it = 0; it < height; ++it) {
        int2 nd[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) nd[r] = tlds[cur[r]];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
          const int right = rec_right(nd[r].x);
          if (right != cur[r]) {  // resting lanes are masked out of the reads
            const float4* wp = rlds + rec_slot(nd[r].x) * NODE4;
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < Q; c += CW4) {
              float4 w[CW4];
#pragma unroll
              for (int q = 0; q < CW4; ++q) w[q] = wp[c + q];
#pragma unroll
              for (int q = 0; q < CW4; ++q) {
                const int j = 4 * (c + q);
                dot = __fadd_rn(dot, __fmul_rn(w[q].x, x[r][j + 0]));
                dot = __fadd_rn(dot, __fmul_rn(w[q].y, x[r][j + 1]));
                dot = __fadd_rn(dot, __fmul_rn(w[q].z, x[r][j + 2]));
                dot = __fadd_rn(dot, __fmul_rn(w[q].w, x[r][j + 3]));
              }
            }
            const bool left = dot < __int_as_float(nd[r].y);
            const float4* sp = wp + (left ? ROW4 : 2 * ROW4);
#pragma unroll
            for (int c = 0; c < Q; c += CW4) {
              float4 s[CW4];
#pragma unroll
              for (int q = 0; q < CW4; ++q) s[q] = sp[c + q];
#pragma unroll
              for (int q = 0; q < CW4; ++q) {
                const int j = 4 * (c + q);
                acc[r][j + 0] = __fadd_rn(acc[r][j + 0], s[q].x);
                acc[r][j + 1] = __fadd_rn(acc[r][j + 1], s[q].y);
                acc[r][j + 2] = __fadd_rn(acc[r][j + 2], s[q].z);
                acc[r][j + 3] = __fadd_rn(acc[r][j + 3], s[q].w);
              }
            }
            cur[r] = left ? cur[r] + 1 : right;
          }
        }
      }
    }

#pragma unroll
    for (int r = 0; r < RPT; ++r) {
      const int64_t my_row = block_row0 + tid + r * BT;
      if (my_row < N) {
        float* o = out + my_row * d;
#pragma unroll
        for (int j = 0; j < D; ++j)
          if (j < d) o[j] = finalize ? div32_exact(acc[r][j], fT) : acc[r][j];
      }
    }
  }
}

// The instantiation table: rows per thread and block size by D. D = 32 holds
// 32 row and 32 accumulator registers a row and runs one row a thread in a
// block of 1024 (one 114 KB stage a CU at 255 internal nodes, shared by 16
// waves: 4 a SIMD under the 128-register cap of the block size); D <= 16
// runs two rows a thread in blocks of 512, as score_extended_dense_v2 does.
template <int D> struct Shape;
template <> struct Shape<8> { static constexpr int RPT = 2, BT = 512; };
template <> struct Shape<16> { static constexpr int RPT = 2, BT = 512; };
template <> struct Shape<32> { static constexpr int RPT = 1, BT = 1024; };

template <typename KT, int D>
static hipError_t launch_one(const void* X, const void* nodes,
                             const float* rows, const int32_t* ncnt,
                             const int32_t* icnt, float* out, int64_t N,
                             int32_t d, int64_t rs, int64_t cs, int32_t T,
                             int32_t max_nodes, int32_t max_internal,
                             int32_t height, float fT, int finalize,
                             size_t lds, int blocks, hipStream_t stream) {
  constexpr int RPT = Shape<D>::RPT, BT = Shape<D>::BT;
  const void* fn = (const void*)explain_extended_dense_kernel<KT, D, RPT, BT>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(
        fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((explain_extended_dense_kernel<KT, D, RPT, BT>),
                     dim3(blocks), dim3(BT), lds, stream, (const KT*)X,
                     (const int2*)nodes, (const float4*)rows, ncnt, icnt, out,
                     N, d, rs, cs, T, max_nodes, max_internal, height, fT,
                     finalize);
  return hipGetLastError();
}

template <typename KT>
static hipError_t launch_kind(int D, const void* X, const void* nodes,
                              const float* rows, const int32_t* ncnt,
                              const int32_t* icnt, float* out, int64_t N,
                              int32_t d, int64_t rs, int64_t cs, int32_t T,
                              int32_t max_nodes, int32_t max_internal,
                              int32_t height, float fT, int finalize,
                              size_t lds, int blocks, hipStream_t stream) {
#define EXD_ARGS                                                             \
  X, nodes, rows, ncnt, icnt, out, N, d, rs, cs, T, max_nodes, max_internal, \
      height, fT, finalize, lds, blocks, stream
  if (D == 8) return launch_one<KT, 8>(EXD_ARGS);
  if (D == 16) return launch_one<KT, 16>(EXD_ARGS);
  if (D == 32) return launch_one<KT, 32>(EXD_ARGS);
  return hipErrorInvalidValue;
}

}  // namespace exd

// (rows per thread, block threads) the dense EIF explain kernel runs at
// padded width D, and the LDS bytes of one staged tree; rpt = 0 for a D it
// has no instantiation for
void explain_eif_dense_shape(int D, int32_t max_nodes, int32_t max_internal,
                             int* rpt, int* threads, size_t* lds) {
  *rpt = *threads = 0;
  *lds = 0;
  int row4 = 0;
  if (D == 8) {
    *rpt = exd::Shape<8>::RPT, *threads = exd::Shape<8>::BT;
    row4 = exd::Stage<8>::ROW4;
  } else if (D == 16) {
    *rpt = exd::Shape<16>::RPT, *threads = exd::Shape<16>::BT;
    row4 = exd::Stage<16>::ROW4;
  } else if (D == 32) {
    *rpt = exd::Shape<32>::RPT, *threads = exd::Shape<32>::BT;
    row4 = exd::Stage<32>::ROW4;
  } else {
    return;
  }
  *lds = (((size_t)max_nodes * 8 + 15) & ~(size_t)15) +
         (size_t)max_internal * 3 * row4 * 16;
}

hipError_t launch_explain_extended_dense(
    RowDtype dt, int D, const void* X, const void* nodes, const float* rows,
    const int32_t* ncnt, const int32_t* icnt, float* out, int64_t N, int32_t d,
    int64_t rs, int64_t cs, int32_t T, int32_t max_nodes, int32_t max_internal,
    int32_t height, float fT, int finalize, size_t lds, int blocks,
    hipStream_t stream) {
  if (dt == ROW_BF16) return exd::launch_kind<uint16_t>(D, EXD_ARGS);
  if (dt == ROW_F16) return exd::launch_kind<exd::f16_t>(D, EXD_ARGS);
  return exd::launch_kind<float>(D, EXD_ARGS);
}
#undef EXD_ARGS

}  // namespace ifa
