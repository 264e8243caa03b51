// MI355X (gfx950, CDNA4) on-device bag sampling: Philox draws and collision
// resolution, BITWISE equal to cpu_engine.sample_bags (docs/DESIGN.md §2c).
//
// Without replacement and 2n <= N, tree t, the oracle is: slot s holds
// v = rng_below(seed, P_BAG, t, s, N, attempt); after each round, among the
// slots that hold one value the smallest slot id keeps it and every other
// one redraws with the round number as attempt (a settled slot is displaced
// when a smaller slot draws its value); repeat until no slot loses, at most
// 256 redraw rounds. The numpy version sorts all slots every round. Here one
// open-addressing hash table per tree maps a value to the MINIMUM slot that
// ever inserted it; it persists across the rounds and nothing is deleted.
//
//   entry : one 64-bit word, value << 32 | slot; empty = all ones (no value
//           is 0xFFFFFFFF because values are < N <= 2^32 - 1)
//   insert: linear probe from a hash of the value. 64-bit compare-and-swap
//           of empty -> mine; if the word holds the same value (same high
//           half) a 64-bit unsigned atomic min instead; another value: next.
//   check : the same probe until the value is found. A slot loses iff the
//           entry's low half is not its own id.
//
// Why this is exact:
//   (1) The minimum slot m that ever held v never loses v: it would only
//       redraw if a smaller slot held v in that round, and none ever did.
//       So m still holds v, it is the smallest CURRENT holder as well, and
//       "entry != me" is the oracle's loser test.
//   (2) Hence value -> holder is injective over the table: it never carries
//       more than n values, and a capacity of the next power of two >= 2n
//       keeps the load at or below 1/2 in every round.
// Where different values land depends on the race; which slot wins a value
// does not.
//
// Routes (gpu_engine.sample_bags_device picks one):
//   bag_sample_lds_kernel   n <= BAG_LDS_MAX_SAMPLES: one block per tree, the
//                           table in LDS, all rounds inside one launch
//   bag_draw_insert_kernel  larger n: table in global memory, grid (slot
//   + bag_check_kernel      tile, tree), two plain launches per round; the
//                           host reads the loser total after each round
//   bag_bootstrap_kernel    with replacement: one draw per slot, no table
//   bag_dense_keys_kernel   2n > N: sort keys for the oracle's permutation
//
// Every loop is bounded: rounds by the oracle's 256, probes by the capacity.
// Overflow sets a per-launch error word that the binding turns into the
// oracle's RuntimeError. All arithmetic is integer; this TU is torch-free and
// is not linked into the native scorer.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace ifa {
namespace bag {

typedef unsigned long long u64;

constexpr u64 kEmpty = ~0ull;
constexpr int kMaxAttempt = 256;  // cpu_engine.sample_bags raises past this
constexpr int32_t kErrRounds = 1;
constexpr int32_t kErrProbe = 2;
constexpr int kTile = 256;  // slots per block of the global-route kernels

// Fibonacci hash to log2(cap) bits; shift = 32 - log2(cap), in [1, 31]
__device__ __forceinline__ uint32_t slot_hash(uint32_t v, int shift) {
  return (v * 0x9E3779B1u) >> shift;
}

// false: the bounded probe ran out (cannot happen at load <= 1/2)
__device__ __forceinline__ bool table_insert(u64* tab, uint32_t mask,
                                             int shift, uint32_t v,
                                             uint32_t slot) {
  const u64 mine = ((u64)v << 32) | slot;
  uint32_t h = slot_hash(v, shift);
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const u64 old = atomicCAS(&tab[h], kEmpty, mine);
    if (old == kEmpty) return true;
    if ((uint32_t)(old >> 32) == v) {
      if (mine < old) atomicMin(&tab[h], mine);
      return true;
    }
    h = (h + 1) & mask;
  }
  return false;
}

// the slot recorded for v, which every holder of v inserted before the check;
// false: v is not in the table (an internal error, reported like a full probe)
__device__ __forceinline__ bool table_holder(const u64* tab, uint32_t mask,
                                             int shift, uint32_t v,
                                             uint32_t* holder) {
  uint32_t h = slot_hash(v, shift);
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const u64 e = tab[h];
    if ((uint32_t)(e >> 32) == v) {
      *holder = (uint32_t)e;
      return true;
    }
    if (e == kEmpty) return false;
    h = (h + 1) & mask;
  }
  return false;
}

// ---------------------------------------------------------------------------
// LDS route: block = tree. Thread tid owns the slots tid + j * blockDim.x.
// SPT > 0: blockDim.x * SPT >= n, a slot's value lives in val[j] and its
// loser flag in bit j of `lose`. SPT == 0: any n; the state lives in the
// output row (value in the low half, loser flag in bit 63), which only the
// owning thread touches, and the row is rewritten at the end.
// Two barriers per round (inserts | checks + count); every branch around
// them depends on the block-wide count, the block-wide error and the round.
// ---------------------------------------------------------------------------

constexpr int64_t kLoseBit = INT64_MIN;  // bit 63

template <int SPT>
__global__ void __launch_bounds__(1024)
    bag_sample_lds_kernel(int64_t* __restrict__ out, int32_t* __restrict__ err,
                          uint64_t seed, uint32_t tree0, uint32_t N, int32_t n,
                          int64_t row_offset, uint32_t mask, int shift) {
  extern __shared__ u64 tab[];
  __shared__ int32_t s_losers[2];
  __shared__ int32_t s_bad;

  const int tid = threadIdx.x, nt = blockDim.x;
  const uint32_t tree = tree0 + blockIdx.x;
  int64_t* __restrict__ row = out + (int64_t)blockIdx.x * n;

  for (uint32_t i = tid; i <= mask; i += nt) tab[i] = kEmpty;
  if (tid < 2) s_losers[tid] = 0;
  if (tid == 0) s_bad = 0;

  uint32_t val[SPT > 0 ? SPT : 1];
  uint32_t lose = 0xFFFFFFFFu;  // round 0: every slot draws
  if (SPT == 0)
    for (int s = tid; s < n; s += nt) row[s] = kLoseBit;
  __syncthreads();

  bool settled = false;
  for (int round = 0; round <= kMaxAttempt; ++round) {
    bool bad = false;
    // draw for the active slots and insert
    if (SPT > 0) {
#pragma unroll
      for (int j = 0; j < SPT; ++j) {
        const int s = tid + j * nt;
        if (s < n && ((lose >> j) & 1u)) {
          val[j] = rng_below(seed, P_BAG, tree, (uint32_t)s, N, (uint32_t)round);
          bad |= !table_insert(tab, mask, shift, val[j], (uint32_t)s);
        }
      }
    } else {
      for (int s = tid; s < n; s += nt) {
        if (row[s] < 0) {
          const uint32_t v =
              rng_below(seed, P_BAG, tree, (uint32_t)s, N, (uint32_t)round);
          row[s] = (int64_t)v | kLoseBit;
          bad |= !table_insert(tab, mask, shift, v, (uint32_t)s);
        }
      }
    }
    __syncthreads();

    // check every slot, settled ones included: they can be displaced
    int mine = 0;
    if (SPT > 0) {
      lose = 0;
#pragma unroll
      for (int j = 0; j < SPT; ++j) {
        const int s = tid + j * nt;
        if (s < n) {
          uint32_t holder = (uint32_t)s;
          bad |= !table_holder(tab, mask, shift, val[j], &holder);
          const uint32_t l = holder != (uint32_t)s;
          lose |= l << j;
          mine += (int)l;
        }
      }
    } else {
      for (int s = tid; s < n; s += nt) {
        const uint32_t v = (uint32_t)row[s];
        uint32_t holder = (uint32_t)s;
        bad |= !table_holder(tab, mask, shift, v, &holder);
        const bool l = holder != (uint32_t)s;
        row[s] = l ? ((int64_t)v | kLoseBit) : (int64_t)v;
        mine += (int)l;
      }
    }
    if (mine) atomicAdd(&s_losers[round & 1], mine);
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();

    const int32_t losers = s_losers[round & 1];
    if (s_bad) {  // block-uniform
      if (tid == 0) atomicOr(err, kErrProbe);
      return;
    }
    if (losers == 0) {
      settled = true;
      break;
    }
    // the other counter was last read before this round's first barrier
    if (tid == 0) s_losers[(round + 1) & 1] = 0;
  }
  if (!settled) {  // block-uniform
    if (tid == 0) atomicOr(err, kErrRounds);
    return;
  }

  if (SPT > 0) {
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tid + j * nt;
      if (s < n) row[s] = (int64_t)val[j] + row_offset;
    }
  } else {
    for (int s = tid; s < n; s += nt) row[s] = (row[s] & ~kLoseBit) + row_offset;
  }
}

// ---------------------------------------------------------------------------
// Global route: grid (slot tile, tree). out holds value + row_offset from the
// first round on; lose[t][s] says which slots redraw (not read in round 0).
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(kTile)
    bag_draw_insert_kernel(int64_t* __restrict__ out,
                           const uint8_t* __restrict__ lose,
                           u64* __restrict__ tabs, int32_t* __restrict__ err,
                           uint64_t seed, uint32_t tree0, uint32_t N, int32_t n,
                           int64_t row_offset, uint32_t mask, int shift,
                           int32_t round) {
  const int64_t s = (int64_t)blockIdx.x * kTile + threadIdx.x;
  if (s >= n) return;
  const int64_t at = (int64_t)blockIdx.y * n + s;
  if (round > 0 && !lose[at]) return;
  const uint32_t v = rng_below(seed, P_BAG, tree0 + blockIdx.y, (uint32_t)s, N,
                               (uint32_t)round);
  out[at] = (int64_t)v + row_offset;
  u64* tab = tabs + (int64_t)blockIdx.y * ((int64_t)mask + 1);
  if (!table_insert(tab, mask, shift, v, (uint32_t)s)) atomicOr(err, kErrProbe);
}

// one integer atomic add per wave that has losers, into this round's total
__global__ void __launch_bounds__(kTile)
    bag_check_kernel(const int64_t* __restrict__ out,
                     uint8_t* __restrict__ lose, const u64* __restrict__ tabs,
                     int32_t* __restrict__ err, int32_t* __restrict__ total,
                     int32_t n, int64_t row_offset, uint32_t mask, int shift) {
  const int64_t s = (int64_t)blockIdx.x * kTile + threadIdx.x;
  bool l = false;
  if (s < n) {
    const int64_t at = (int64_t)blockIdx.y * n + s;
    const uint32_t v = (uint32_t)(out[at] - row_offset);
    const u64* tab = tabs + (int64_t)blockIdx.y * ((int64_t)mask + 1);
    uint32_t holder = (uint32_t)s;
    if (!table_holder(tab, mask, shift, v, &holder)) atomicOr(err, kErrProbe);
    l = holder != (uint32_t)s;
    lose[at] = l ? 1 : 0;
  }
  const int cnt = __popcll(__ballot(l));
  if (cnt && (threadIdx.x & 63) == 0) atomicAdd(total, cnt);
}

// ---------------------------------------------------------------------------
// bootstrap and the dense regime's sort keys: one Philox call per element
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
    bag_bootstrap_kernel(int64_t* __restrict__ out, uint64_t seed,
                         uint32_t tree0, uint32_t N, int64_t T, int64_t n,
                         int64_t row_offset) {
  const int64_t total = T * n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const int64_t t = i / n, s = i - t * n;
    out[i] = (int64_t)rng_below(seed, P_BAG, tree0 + (uint32_t)t, (uint32_t)s,
                                N) + row_offset;
  }
}

// (key ^ 0x80000000) << 32 | row as int64: unique, and its SIGNED order is
// the oracle's stable argsort order (key, then row)
__global__ void __launch_bounds__(256)
    bag_dense_keys_kernel(int64_t* __restrict__ keys, uint64_t seed,
                          uint32_t tree0, int64_t T, int64_t N) {
  const int64_t total = T * N;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    const int64_t t = i / N, r = i - t * N;
    const uint32_t k =
        rng_u32(seed, P_BAG, tree0 + (uint32_t)t, (uint32_t)r, 0xFFFFu);
    keys[i] = (int64_t)(((u64)(k ^ 0x80000000u) << 32) | (u64)r);
  }
}

}  // namespace bag
}  // namespace ifa

// ---------------------------------------------------------------------------
// host-side launchers (bindings.cpp is compiled by g++)
// ---------------------------------------------------------------------------

namespace ifa {

static inline int log2_pow2(uint32_t cap) {
  int b = 0;
  while ((1u << b) < cap) ++b;
  return b;
}

static inline int grid_stride_blocks(int64_t total) {
  int64_t blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// Threads and slots per thread of the LDS route. Auto: a thread per slot up
// to 1024 slots, then 4 and 8 slots per thread on blocks of up to 1024.
// `threads` > 0 fixes the block; slot state then moves to the output row
// (spt 0) when 8 slots per thread do not cover n.
static void bag_lds_shape(int32_t n, int threads, int* block, int* spt) {
  if (threads <= 0) {
    *spt = n <= 1024 ? 1 : (n <= 4096 ? 4 : 8);
    const int per = (n + *spt - 1) / *spt;
    *block = ((per + 63) / 64) * 64;
    return;
  }
  *block = threads;
  const int64_t cover = (int64_t)threads;
  *spt = n <= cover ? 1 : (n <= 4 * cover ? 4 : (n <= 8 * cover ? 8 : 0));
}

template <int SPT>
static void launch_lds(int64_t* out, int32_t* err, uint64_t seed,
                       uint32_t tree0, int32_t T, uint32_t N, int32_t n,
                       int64_t row_offset, uint32_t cap, int block,
                       hipStream_t stream) {
  const size_t lds = (size_t)cap * 8;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)bag::bag_sample_lds_kernel<SPT>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
  hipLaunchKernelGGL(bag::bag_sample_lds_kernel<SPT>, dim3(T), dim3(block),
                     lds, stream, out, err, seed, tree0, N, n, row_offset,
                     cap - 1, 32 - log2_pow2(cap));
}

// cap: power of two in [2, 2^14] with cap >= 2n; block: multiple of 64 in
// [64, 1024] (0: chosen from n). Returns the slots per thread it ran with.
int launch_bag_sample_lds(int64_t* out, int32_t* err, uint64_t seed,
                          uint32_t tree0, int32_t T, uint32_t N, int32_t n,
                          int64_t row_offset, uint32_t cap, int threads,
                          hipStream_t stream) {
  int block, spt;
  bag_lds_shape(n, threads, &block, &spt);
  switch (spt) {
    case 1:
      launch_lds<1>(out, err, seed, tree0, T, N, n, row_offset, cap, block,
                    stream);
      break;
    case 4:
      launch_lds<4>(out, err, seed, tree0, T, N, n, row_offset, cap, block,
                    stream);
      break;
    case 8:
      launch_lds<8>(out, err, seed, tree0, T, N, n, row_offset, cap, block,
                    stream);
      break;
    default:
      launch_lds<0>(out, err, seed, tree0, T, N, n, row_offset, cap, block,
                    stream);
  }
  return spt;
}

// one round of the global route: T <= 65535 trees (grid.y), cap a power of
// two in [2, 2^31]; `total` is this round's own zeroed counter
void launch_bag_global_round(int64_t* out, uint8_t* lose,
                             unsigned long long* tabs, int32_t* err,
                             int32_t* total, uint64_t seed, uint32_t tree0,
                             int32_t T, uint32_t N, int32_t n,
                             int64_t row_offset, uint32_t cap, int32_t round,
                             hipStream_t stream) {
  const dim3 grid((uint32_t)((n + bag::kTile - 1) / bag::kTile), (uint32_t)T);
  const int shift = 32 - log2_pow2(cap);
  hipLaunchKernelGGL(bag::bag_draw_insert_kernel, grid, dim3(bag::kTile), 0,
                     stream, out, (const uint8_t*)lose, tabs, err, seed, tree0,
                     N, n, row_offset, cap - 1, shift, round);
  hipLaunchKernelGGL(bag::bag_check_kernel, grid, dim3(bag::kTile), 0, stream,
                     (const int64_t*)out, lose,
                     (const unsigned long long*)tabs, err, total, n,
                     row_offset, cap - 1, shift);
}

void launch_bag_bootstrap(int64_t* out, uint64_t seed, uint32_t tree0,
                          uint32_t N, int64_t T, int64_t n, int64_t row_offset,
                          hipStream_t stream) {
  hipLaunchKernelGGL(bag::bag_bootstrap_kernel,
                     dim3(grid_stride_blocks(T * n)), dim3(256), 0, stream,
                     out, seed, tree0, N, T, n, row_offset);
}

void launch_bag_dense_keys(int64_t* keys, uint64_t seed, uint32_t tree0,
                           int64_t T, int64_t N, hipStream_t stream) {
  hipLaunchKernelGGL(bag::bag_dense_keys_kernel,
                     dim3(grid_stride_blocks(T * N)), dim3(256), 0, stream,
                     keys, seed, tree0, T, N);
}

}  // namespace ifa
