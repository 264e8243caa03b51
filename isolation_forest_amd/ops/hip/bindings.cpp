// Torch-extension bindings for the MI355X isolation-forest kernels.
// Pure host glue (compiled by g++): tensor checks, LDS sizing, dispatch into
// the hipcc-compiled launchers in forest_kernels.hip.

#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <algorithm>
#include <climits>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "row_dtype.h"

namespace ifa {

void launch_bag_gather(RowDtype dt, const void* X, const int64_t* bag_idx,
                       float* bags, int64_t T, int64_t n, int64_t d,
                       int64_t rs, int64_t cs,
                       hipStream_t stream);

void launch_build_forest(const float* bags, const int32_t* feat_sub,
                         int32_t* feat, float* value, int32_t* right,
                         int32_t* count, int32_t* ncount, int32_t* depth,
                         const float* leaf_lut, uint64_t seed,
                         int32_t tree_id_offset, int32_t T, int32_t n,
                         int32_t d, int32_t k, int32_t max_nodes,
                         int32_t height_limit, size_t lds, hipStream_t stream);

void launch_build_extended_forest(const float* bags, const int32_t* feat_sub,
                                  int32_t* feat, float* value, int32_t* right,
                                  int32_t* count, int32_t* ncount,
                                  int32_t* hidx, float* hw, double* off64,
                                  int32_t* depth,
                                  const float* leaf_lut, uint64_t seed,
                                  int32_t tree_id_offset, int32_t T, int32_t n,
                                  int32_t d, int32_t k, int32_t nnz,
                                  int32_t max_nodes, int32_t height_limit,
                                  size_t lds, hipStream_t stream);

void launch_build_forest_large(RowDtype dt, const void* X, int64_t rs,
                               int64_t cs, const int64_t* bag_idx,
                               uint32_t* scratch, const int32_t* feat_sub,
                               int32_t* feat, float* value, int32_t* right,
                               int32_t* count, int32_t* ncount, int32_t* depth,
                               const float* leaf_lut, uint64_t seed,
                               int32_t tree_id_offset, int32_t T, int32_t n,
                               int32_t k, int32_t max_nodes,
                               int32_t height_limit, int threads, size_t lds,
                               hipStream_t stream);

void launch_build_extended_forest_large(
    RowDtype dt, const void* X, int64_t rs, int64_t cs, const int64_t* bag_idx,
    uint32_t* scratch, const int32_t* feat_sub, int32_t* feat, float* value,
    int32_t* right, int32_t* count, int32_t* ncount, int32_t* hidx, float* hw,
    double* off64, int32_t* depth, const float* leaf_lut, uint64_t seed,
    int32_t tree_id_offset, int32_t T, int32_t n, int32_t k, int32_t nnz,
    int32_t max_nodes, int32_t height_limit, int threads, size_t lds,
    hipStream_t stream);

void launch_v4_level_order(const void* nodes, const int32_t* ncount,
                           void* out, int32_t Tpad, int32_t max_nodes,
                           hipStream_t stream);

void launch_v4_heap_order(const void* nodes, const int32_t* ncount,
                          void* out, int32_t Tpad, int32_t max_nodes,
                          int32_t height, int32_t slab_bytes,
                          hipStream_t stream);

hipError_t launch_score_forest_heap(RowDtype dt, int rpt, int phase,
                                    int threads, const void* X,
                                    const void* heap, float* out, int64_t N,
                                    int32_t d, int64_t rs, int64_t cs,
                                    int32_t Tpad, int32_t height, float fT,
                                    float c_norm, int finalize, size_t lds,
                                    int blocks, hipStream_t stream);

int score_forest_heap_resident(RowDtype dt, int rpt, bool packed, int phase,
                               int threads, size_t lds);

void launch_score_forest(RowDtype dt, int rpt, bool rows_lds, bool nodes_lds,
                         int ilp, const void* X, const void* nodes,
                         const int32_t* ncount, float* out, int64_t N,
                         int32_t d, int64_t rs, int64_t cs, int32_t Tpad,
                         int32_t max_nodes, int32_t height_limit, float fT,
                         float c_norm, int finalize, size_t lds, int blocks,
                         hipStream_t stream);

void launch_score_extended_dense(RowDtype dt, bool rows_lds, bool wlds,
                                 const void* X, const void* nodes,
                                 const float* hw, const int32_t* ncount,
                                 float* out, int64_t N, int32_t d, int64_t rs,
                                 int64_t cs, int32_t dpad, int32_t T,
                                 int32_t max_nodes, float fT, float c_norm,
                                 int finalize, size_t lds, int blocks,
                                 hipStream_t stream);

void launch_score_extended_forest(RowDtype dt, bool rows_lds, bool hyper_lds,
                                  bool nodes_lds, const void* X,
                                  const void* nodes, const int32_t* hidx,
                                  const float* hw, const int32_t* ncount,
                                  float* out, int64_t N, int32_t d, int64_t rs,
                                  int64_t cs, int32_t T,
                                  int32_t max_nodes, int32_t nnz, float fT,
                                  float c_norm, int finalize, size_t lds,
                                  int blocks, hipStream_t stream);

void launch_score_extended_sparse_v2(RowDtype dt, int nnz, const void* X,
                                     const void* nodes, const float* values,
                                     const int32_t* hidx, const float* hw,
                                     const int32_t* ncount, float* out,
                                     int64_t N, int32_t d, int64_t rs,
                                     int64_t cs, int32_t dpad,
                                     int32_t T, int32_t max_nodes,
                                     int32_t height_limit, float fT,
                                     float c_norm, int finalize, size_t lds,
                                     int blocks, hipStream_t stream);

void launch_score_extended_dense_v2(RowDtype dt, int D, const void* X,
                                    const void* nodes, const float* values,
                                    const float* hw, const int32_t* ncount,
                                    float* out, int64_t N, int32_t d,
                                    int64_t rs, int64_t cs,
                                    int32_t T, int32_t max_nodes,
                                    int32_t height_limit, float fT,
                                    float c_norm, int finalize, size_t lds,
                                    int blocks, hipStream_t stream);

void launch_score_extended_dense_v3(int D, bool rpt2, const void* X,
                                    const void* nodes, const float* values,
                                    const uint32_t* hwp,
                                    const int32_t* ncount, float* out,
                                    int64_t N, int32_t d, int64_t rs,
                                    int64_t cs, int32_t T,
                                    int32_t max_nodes, int32_t height_limit,
                                    float fT, float c_norm, int finalize,
                                    size_t lds, int blocks,
                                    hipStream_t stream);

void launch_score_extended_dense_nonfinite_rows(
    RowDtype dt, bool packed_w, const void* X, const void* nodes,
    const float* values, const void* wts, float* out, int64_t N, int32_t d,
    int64_t rs, int64_t cs,
    int32_t D, int32_t T, int32_t max_nodes, int32_t height_limit, float fT,
    float c_norm, int finalize, int blocks, hipStream_t stream);
void launch_score_forest_wide(RowDtype dt, const void* X, const void* nodes,
                              float* out, int64_t N, int32_t d, int64_t rs,
                              int64_t cs, int32_t T,
                              int64_t max_nodes, int32_t height_limit,
                              float fT, float c_norm, int finalize,
                              int blocks, hipStream_t stream);

void launch_score_extended_wide(RowDtype dt, const void* X, const void* nodes,
                                const int32_t* hidx, const float* hw,
                                float* out, int64_t N, int32_t d, int64_t rs,
                                int64_t cs, int32_t T,
                                int64_t max_nodes, int32_t nnz, float fT,
                                float c_norm, int finalize, int blocks,
                                hipStream_t stream);

void launch_explain_forest(RowDtype dt, int mode, int rpt, bool nodes_lds,
                           const void* X, const void* nodes,
                           const int32_t* ncount, float* out, int64_t N,
                           int32_t d, int64_t rs, int64_t cs, int32_t dpad,
                           int32_t astride, int32_t T, int32_t max_nodes,
                           int32_t tps, int32_t height_limit, float fT,
                           int finalize, size_t lds, int blocks,
                           hipStream_t stream);

void launch_explain_extended(RowDtype dt, const void* X, const void* nodes,
                             const int32_t* hidx, const float* hw,
                             const float* dl, const float* dr, float* out,
                             int64_t N, int32_t d, int64_t rs, int64_t cs,
                             int32_t T, int32_t max_nodes, int32_t nnz,
                             float fT, int finalize, int blocks,
                             hipStream_t stream);

// shap_kernels.hip
void launch_shap_forest(RowDtype dt, bool table_lds, bool acc_lds,
                        const void* X, const void* table,
                        const int64_t* tree_off, const double* wtab,
                        double* acc_g, float* out, int64_t N, int32_t d,
                        int64_t rs, int64_t cs, int32_t T, int32_t table_words,
                        int rows_lds, int finalize, size_t lds, int blocks,
                        hipStream_t stream);

}  // namespace ifa

namespace {

constexpr size_t kMaxLds = 160 * 1024;

#define CHECK_CUDA(x) TORCH_CHECK((x).is_cuda(), #x " must be a GPU tensor")
#define CHECK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")

hipStream_t current_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

bool is_bf16(const torch::Tensor& t) {
  return t.scalar_type() == torch::kBFloat16;
}

// row element type of a checked X (check_x admits exactly these three)
ifa::RowDtype row_dtype(const torch::Tensor& t) {
  if (t.scalar_type() == torch::kBFloat16) return ifa::ROW_BF16;
  if (t.scalar_type() == torch::kHalf) return ifa::ROW_F16;
  return ifa::ROW_F32;
}

void check_x(const torch::Tensor& X) {
  TORCH_CHECK(X.dim() == 2, "X must be [N, d]");
  TORCH_CHECK(X.scalar_type() == torch::kFloat32 ||
                  X.scalar_type() == torch::kBFloat16 ||
                  X.scalar_type() == torch::kHalf,
              "X must be float32, bfloat16 or float16");
}

// element strides the kernels address X with: X[r][c] = X[r * rs + c * cs]
struct XLayout {
  int64_t rs, cs;
};

// Layout contract for a checked X (docs/API.md "Input layouts"): consumed in
// place when pitched row-major (stride(1) == 1, stride(0) >= d) or
// feature-major (stride(0) == 1, stride(1) >= N), at any storage offset and
// alignment. The stride torch reports for a size-1 dimension is arbitrary
// and ignored (that index is always 0); it is returned normalised so the
// kernels' alignment tests see the packed value. A view that fits both
// layouts is row-major. Everything else is the caller's to copy
// (gpu_engine._rows_in_place).
XLayout check_x_layout(const torch::Tensor& X) {
  const int64_t N = X.size(0), d = X.size(1);
  const int64_t s0 = X.stride(0), s1 = X.stride(1);
  const bool row = (d <= 1 || s1 == 1) && (N <= 1 || s0 >= d);
  const bool feat = (N <= 1 || s0 == 1) && (d <= 1 || s1 >= N);
  TORCH_CHECK(row || feat,
              "X must be pitched row-major (stride(1) == 1, stride(0) >= d) "
              "or feature-major (stride(0) == 1, stride(1) >= N); got shape [",
              N, ", ", d, "] with strides (", s0, ", ", s1, ")");
  if (row) return {N <= 1 ? std::max<int64_t>(d, 1) : s0, 1};
  return {1, s1};
}

// The instantiation one standard scoring call runs, from shapes alone (and
// the IFA_SCORE_* switches). score_forest launches by it, v4_heap_order lays
// the heap records out for it, and score_route reports it.
struct ScoreCfg {
  // score_forest_v4
  int rpt, ilp;
  bool rows_lds, nodes_lds;
  size_t lds;
  // score_forest_heap: taken when `heap` and the caller has the records
  // heap_rpt is tile rows / 256 (what the records' slab offsets are laid
  // out for); heap_threads (256 or 512) share the tile's rows out
  bool heap;
  int heap_rpt, heap_phase, heap_threads;
  size_t heap_lds;
};

// Blocks per CU that every 512-thread heap instantiation of `phase` (bf16
// and fp16, packed and strided) keeps resident at this LDS size: the least
// of the runtime's four occupancy figures, asked once per (device, phase,
// size) and one map lookup after that. pick_score_cfg runs on every score
// call, and the first may fall inside a stream capture: the function
// attribute and the occupancy query are host-side and put nothing on a
// stream, so they are safe there.
int heap_wide_resident(int phase, size_t lds) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, size_t>, int> memo;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  const auto key = std::make_tuple(dev, phase, lds);
  std::lock_guard<std::mutex> lock(mu);
  auto it = memo.find(key);
  if (it == memo.end()) {
    int least = INT_MAX;
    for (ifa::RowDtype dt : {ifa::ROW_BF16, ifa::ROW_F16})
      for (bool packed : {true, false})
        least = std::min(least, ifa::score_forest_heap_resident(
                                    dt, 1, packed, phase, 512, lds));
    it = memo.emplace(key, least).first;
  }
  return it->second;
}

ScoreCfg pick_score_cfg(int elem_bytes, int64_t d, int64_t max_nodes,
                        int64_t height) {
  ScoreCfg c{};
  const size_t elem = (size_t)elem_bytes;
  // staged-tree ILP: 4 (default) or 8; 8 halves the number of barrier-
  // bounded staging phases at the cost of occupancy (A/B via env)
  int ilp = 4;
  bool ilp_forced = false;
  if (const char* e = getenv("IFA_SCORE_ILP")) {
    ilp = atoi(e) == 8 ? 8 : 4;
    ilp_forced = ilp == 8;
  }
  // feature-major key tile: d feature slabs plus the sentinel slab, each
  // rows_per_block keys, lane-adjacent — no padding needed
  const int64_t slabs = d + 1;
  // deep forests (large maxSamples) overflow LDS node staging: walk nodes
  // from global/L2 instead (NODES_LDS=false) — correct for any tree size
  bool nodes_lds =
      (size_t)2 * max_nodes * 8 + (size_t)256 * slabs * elem <= 150 * 1024;
  // config search over (rpt, ilp): wide-d rows inflate the LDS row tile,
  // so dropping staged-tree ILP to 2 can buy back a resident block
  // (measured: d=128 went 1 block/CU at ILP=4 -> 124M rows/s; ILP=2 at 2
  // blocks is the faster shape). Prefer the candidate with the most
  // resident blocks, breaking ties toward more chains (rpt*ilp).
  int rpt = 2;
  bool rows_lds = true;
  size_t lds = 0;
  int best_blocks = 0;
  {
    struct Cand { int rpt, ilp; };
    const Cand cands[] = {{2, ilp}, {1, ilp}, {2, 2}, {1, 2}};
    int best_chains = 0;
    bool found = false;
    for (const Cand& cnd : cands) {
      size_t nb = nodes_lds ? (size_t)cnd.ilp * max_nodes * 8 : 0;
      size_t l = nb + (size_t)cnd.rpt * 256 * slabs * elem;
      if (l > 150 * 1024) continue;
      int blocks_cu = (int)std::min<size_t>(kMaxLds / std::max(l, (size_t)1),
                                            3);
      int chains = cnd.rpt * cnd.ilp;
      if (blocks_cu > best_blocks ||
          (blocks_cu == best_blocks && chains > best_chains)) {
        best_blocks = blocks_cu;
        best_chains = chains;
        rpt = cnd.rpt;
        ilp = cnd.ilp;
        lds = l;
        found = true;
      }
    }
    if (!found) {  // rows exceed LDS even alone: global-X walk
      rows_lds = false;
      rpt = 1;
      lds = nodes_lds ? (size_t)ilp * max_nodes * 8 : 0;
    }
  }
  bool force_global = false;
  if (const char* e = getenv("IFA_SCORE_FORCE_GLOBAL")) {
    if (atoi(e)) {
      force_global = true;
      rows_lds = false;
      rpt = 1;
      lds = nodes_lds ? (size_t)ilp * max_nodes * 8 : 0;
    }
  }
  c.rpt = rpt;
  c.ilp = ilp;
  c.rows_lds = rows_lds;
  c.nodes_lds = nodes_lds;
  c.lds = lds;

  // heap records (score_forest_heap): 16-bit rows, rows and one barrier
  // phase of trees (4 or 8, 2^(height+1) 4-byte slots each) in LDS, the
  // last slab's byte offset within the record's low half. Same budget and
  // the same preference as above; taken only where it holds at least the
  // blocks the v4 candidate holds. The 8-tree phase halves the barriers and
  // is taken where its best candidate keeps at least the resident blocks of
  // the 4-tree one; it may choose another RPT than the 4-tree phase would
  // (the larger stage moves the RPT bound), and v4_heap_order lays the
  // records out for the RPT chosen here.
  // IFA_SCORE_HEAP=0 keeps the v4 route (A/B inside one build); so do the
  // other two switches, which name v4 instantiations. IFA_HEAP_PHASE=4|8
  // picks the phase where that phase is routable; any other value is
  // ignored.
  // A 512-row tile is walked by 512 threads with one row each (8 waves per
  // block in the same LDS) where every 512-thread instantiation of the
  // phase keeps the blocks counted here resident, by the runtime's own
  // occupancy figure; IFA_HEAP_WAVES=4|8 picks the block size where both
  // are routable (any other value is ignored). The records are the same.
  bool heap_on = true;
  if (const char* e = getenv("IFA_SCORE_HEAP")) heap_on = atoi(e) != 0;
  int phase_want = 0;
  if (const char* e = getenv("IFA_HEAP_PHASE")) {
    const int v = atoi(e);
    if (v == 4 || v == 8) phase_want = v;
  }
  if (heap_on && elem == 2 && rows_lds && nodes_lds && !force_global &&
      !ilp_forced && height >= 1 && height <= 13) {
    const size_t slots = (size_t)2 << height;
    struct HeapCand { int blocks, rpt; size_t lds; };
    auto best_of = [&](int phase) {
      HeapCand h{0, 0, 0};
      for (int r : {2, 1}) {
        const size_t tile = (size_t)r * 256 * slabs * elem;
        if (tile > 65536) continue;  // slab offsets are 16 bits
        const size_t l = (size_t)phase * slots * 4 + tile;
        if (l > 150 * 1024) continue;
        const int blocks_cu = (int)std::min<size_t>(kMaxLds / l, 3);
        if (blocks_cu > h.blocks) {  // r = 2 first: ties go to more chains
          h.blocks = blocks_cu;
          h.rpt = r;
          h.lds = l;
        }
      }
      return h;
    };
    const HeapCand h4 = best_of(4), h8 = best_of(8);
    const bool can8 = h8.blocks > 0 && h8.blocks >= h4.blocks;
    const bool take8 = can8 && phase_want != 4;
    const HeapCand& h = take8 ? h8 : h4;
    c.heap_phase = take8 ? 8 : 4;
    c.heap_rpt = h.rpt;
    c.heap_lds = h.lds;
    c.heap = h.blocks > 0 && h.blocks >= best_blocks;
    c.heap_threads = 256;
    int waves_want = 0;
    if (const char* e = getenv("IFA_HEAP_WAVES")) {
      const int v = atoi(e);
      if (v == 4 || v == 8) waves_want = v;
    }
    if (c.heap && h.rpt == 2 && waves_want != 4 &&
        heap_wide_resident(c.heap_phase, h.lds) >= h.blocks)
      c.heap_threads = 512;
  }
  return c;
}

}  // namespace

torch::Tensor bag_gather(torch::Tensor X, torch::Tensor bag_idx) {
  CHECK_CUDA(X);
  CHECK_CUDA(bag_idx);
  CHECK_CONTIG(bag_idx);
  check_x(X);
  const XLayout xl = check_x_layout(X);
  TORCH_CHECK(bag_idx.dim() == 2 && bag_idx.scalar_type() == torch::kInt64,
              "bag_idx must be int64 [T, n]");
  int64_t T = bag_idx.size(0), n = bag_idx.size(1), d = X.size(1);
  auto bags = torch::empty({T, n, d}, X.options().dtype(torch::kFloat32));
  ifa::launch_bag_gather(row_dtype(X), X.data_ptr(),
                         bag_idx.data_ptr<int64_t>(), bags.data_ptr<float>(),
                         T, n, d, xl.rs, xl.cs, current_stream());
  return bags;
}

std::vector<torch::Tensor> build_forest(torch::Tensor bags,
                                        torch::Tensor feat_sub, int64_t seed,
                                        int64_t tree_id_offset,
                                        torch::Tensor leaf_lut,
                                        int64_t max_nodes,
                                        int64_t height_limit) {
  CHECK_CUDA(bags);
  CHECK_CONTIG(bags);
  CHECK_CUDA(feat_sub);
  CHECK_CONTIG(feat_sub);
  CHECK_CUDA(leaf_lut);
  CHECK_CONTIG(leaf_lut);
  TORCH_CHECK(bags.dim() == 3 && bags.scalar_type() == torch::kFloat32);
  TORCH_CHECK(feat_sub.scalar_type() == torch::kInt32);
  int64_t T = bags.size(0), n = bags.size(1), d = bags.size(2);
  int64_t k = feat_sub.size(1);
  TORCH_CHECK(n <= 16384, "GPU build supports maxSamples <= 16384");
  TORCH_CHECK(max_nodes <= 32767, "max_nodes must fit int16 patch ids");

  auto opts = bags.options().dtype(torch::kInt32);
  auto feat = torch::empty({T, max_nodes}, opts);
  auto value = torch::empty({T, max_nodes}, bags.options());
  auto right = torch::full({T, max_nodes}, -1, opts);
  auto count = torch::empty({T, max_nodes}, opts);
  auto ncount = torch::empty({T}, opts);
  auto depth = torch::zeros({T, max_nodes}, opts);

  size_t lds = align16(4 * n + 2 * k) + (height_limit + 8) * 8;
  TORCH_CHECK(lds <= kMaxLds, "build LDS request too large");
  ifa::launch_build_forest(
      bags.data_ptr<float>(), feat_sub.data_ptr<int32_t>(),
      feat.data_ptr<int32_t>(), value.data_ptr<float>(),
      right.data_ptr<int32_t>(), count.data_ptr<int32_t>(),
      ncount.data_ptr<int32_t>(), depth.data_ptr<int32_t>(),
      leaf_lut.data_ptr<float>(), (uint64_t)seed,
      (int32_t)tree_id_offset, (int32_t)T, (int32_t)n, (int32_t)d, (int32_t)k,
      (int32_t)max_nodes, (int32_t)height_limit, lds, current_stream());
  return {feat, value, right, count, ncount, depth};
}

std::vector<torch::Tensor> build_extended_forest(
    torch::Tensor bags, torch::Tensor feat_sub, int64_t seed,
    int64_t tree_id_offset, torch::Tensor leaf_lut, int64_t nnz,
    int64_t max_nodes, int64_t height_limit) {
  CHECK_CUDA(bags);
  CHECK_CONTIG(bags);
  CHECK_CUDA(feat_sub);
  CHECK_CONTIG(feat_sub);
  CHECK_CUDA(leaf_lut);
  int64_t T = bags.size(0), n = bags.size(1), d = bags.size(2);
  int64_t k = feat_sub.size(1);
  TORCH_CHECK(n <= 16384, "GPU build supports maxSamples <= 16384");
  TORCH_CHECK(max_nodes <= 32767);
  TORCH_CHECK(nnz >= 1 && nnz <= k);

  auto opts = bags.options().dtype(torch::kInt32);
  auto feat = torch::empty({T, max_nodes}, opts);
  auto value = torch::empty({T, max_nodes}, bags.options());
  auto right = torch::full({T, max_nodes}, -1, opts);
  auto count = torch::empty({T, max_nodes}, opts);
  auto ncount = torch::empty({T}, opts);
  auto hidx = torch::zeros({T, max_nodes, nnz}, opts);
  auto hw = torch::zeros({T, max_nodes, nnz}, bags.options());
  auto off64 =
      torch::zeros({T, max_nodes}, bags.options().dtype(torch::kFloat64));
  auto depth = torch::zeros({T, max_nodes}, opts);

  size_t lds =
      align16(4 * n + 2 * k) + align16(8 * nnz) + (height_limit + 8) * 8 + 32;
  TORCH_CHECK(lds <= kMaxLds, "build LDS request too large");
  ifa::launch_build_extended_forest(
      bags.data_ptr<float>(), feat_sub.data_ptr<int32_t>(),
      feat.data_ptr<int32_t>(), value.data_ptr<float>(),
      right.data_ptr<int32_t>(), count.data_ptr<int32_t>(),
      ncount.data_ptr<int32_t>(), hidx.data_ptr<int32_t>(),
      hw.data_ptr<float>(), off64.data_ptr<double>(),
      depth.data_ptr<int32_t>(),
      leaf_lut.data_ptr<float>(), (uint64_t)seed, (int32_t)tree_id_offset,
      (int32_t)T, (int32_t)n, (int32_t)d, (int32_t)k, (int32_t)nnz,
      (int32_t)max_nodes, (int32_t)height_limit, lds, current_stream());
  return {feat, value, right, count, ncount, hidx, hw, off64, depth};
}

// ---------------------------------------------------------------------------
// large-bag builds (n > 16384): rows read in place from X, row ids in a
// global scratch of 8 * n bytes per tree (the caller chunks the trees)
// ---------------------------------------------------------------------------

namespace {

struct LargeBuildShape {
  int64_t T, n, d, k;
  XLayout xl;
};

// Admission shared by the two large builders: everything the kernels index
// with must fit its type, and every index they read must be in range.
LargeBuildShape check_large_build(const torch::Tensor& X,
                                  const torch::Tensor& bag_idx,
                                  const torch::Tensor& feat_sub,
                                  const torch::Tensor& leaf_lut,
                                  int64_t tree_id_offset, int64_t max_nodes,
                                  int64_t height_limit, int64_t nnz,
                                  bool extended, int64_t threads) {
  CHECK_CUDA(X);
  CHECK_CUDA(bag_idx);
  CHECK_CONTIG(bag_idx);
  CHECK_CUDA(feat_sub);
  CHECK_CONTIG(feat_sub);
  CHECK_CUDA(leaf_lut);
  CHECK_CONTIG(leaf_lut);
  check_x(X);
  LargeBuildShape s;
  s.xl = check_x_layout(X);
  TORCH_CHECK(bag_idx.dim() == 2 && bag_idx.scalar_type() == torch::kInt64,
              "bag_idx must be int64 [T, n]");
  TORCH_CHECK(feat_sub.dim() == 2 && feat_sub.scalar_type() == torch::kInt32 &&
                  feat_sub.size(0) == bag_idx.size(0),
              "feat_sub must be int32 [T, k]");
  s.T = bag_idx.size(0);
  s.n = bag_idx.size(1);
  s.d = X.size(1);
  s.k = feat_sub.size(1);
  const int64_t N = X.size(0);
  TORCH_CHECK(s.T >= 1 && s.T <= INT_MAX &&
                  s.T + tree_id_offset <= (int64_t)INT_MAX &&
                  tree_id_offset >= 0,
              "tree ids must fit int32");
  // row ids are kept as uint32, segment bounds and 2n-1 node ids as 32-bit
  TORCH_CHECK(N >= 1 && N <= ((int64_t)1 << 32),
              "large GPU build keeps 32-bit row ids: N must be <= 2^32");
  TORCH_CHECK(s.n >= 1 && s.n <= ((int64_t)1 << 30),
              "large GPU build supports maxSamples <= 2^30");
  TORCH_CHECK(height_limit >= 0 && height_limit <= 30, "height_limit > 30");
  TORCH_CHECK(max_nodes >= 1 && max_nodes <= (int64_t)INT_MAX,
              "max_nodes must fit int32 node ids");
  // the most nodes a tree can emit: a full binary tree of the height limit,
  // and for standard trees (no empty sides) also 2n-1
  const int64_t full = ((int64_t)2 << height_limit) - 1;
  const int64_t need = extended ? full : std::min(full, 2 * s.n - 1);
  TORCH_CHECK(max_nodes >= need, "max_nodes ", max_nodes,
              " cannot hold a tree of up to ", need, " nodes");
  // avail[] holds feature ids as int32
  TORCH_CHECK(s.d >= 1 && s.d <= (int64_t)INT_MAX, "d must fit int32");
  TORCH_CHECK(s.k >= 1 && s.k <= s.d, "k must be in [1, d]");
  TORCH_CHECK(nnz >= 1 && nnz <= s.k, "nnz must be in [1, k]");
  TORCH_CHECK(max_nodes <= INT64_MAX / s.T / nnz,
              "T * max_nodes * nnz overflows int64");
  TORCH_CHECK(leaf_lut.scalar_type() == torch::kFloat32 &&
                  leaf_lut.numel() >= s.n + 1,
              "leaf_lut must be float32 [n + 1]");
  TORCH_CHECK(threads >= 64 && threads <= 512 && threads % 64 == 0,
              "threads must be a multiple of 64 in [64, 512]");
  // one reduction each; a bad index would otherwise be a wild global read
  TORCH_CHECK(bag_idx.min().item<int64_t>() >= 0 &&
                  bag_idx.max().item<int64_t>() < N,
              "bag_idx holds a row outside [0, N)");
  TORCH_CHECK(feat_sub.min().item<int32_t>() >= 0 &&
                  feat_sub.max().item<int32_t>() < s.d,
              "feat_sub holds a feature outside [0, d)");
  return s;
}

// static LDS of the large build kernels (BlockPartials), rounded up
constexpr size_t kLargeBuildStaticLds = 1024;

}  // namespace

std::vector<torch::Tensor> build_forest_large(
    torch::Tensor X, torch::Tensor bag_idx, torch::Tensor feat_sub,
    int64_t seed, int64_t tree_id_offset, torch::Tensor leaf_lut,
    int64_t max_nodes, int64_t height_limit, int64_t threads) {
  const LargeBuildShape s =
      check_large_build(X, bag_idx, feat_sub, leaf_lut, tree_id_offset,
                        max_nodes, height_limit, 1, false, threads);
  const size_t lds = align16(4 * s.k) + (height_limit + 8) * 16;
  TORCH_CHECK(lds + kLargeBuildStaticLds <= kMaxLds,
              "build LDS request too large");

  auto opts = bag_idx.options().dtype(torch::kInt32);
  auto fopts = bag_idx.options().dtype(torch::kFloat32);
  auto scratch = torch::empty({s.T, 2, s.n}, opts);
  auto feat = torch::empty({s.T, max_nodes}, opts);
  auto value = torch::empty({s.T, max_nodes}, fopts);
  auto right = torch::full({s.T, max_nodes}, -1, opts);
  auto count = torch::empty({s.T, max_nodes}, opts);
  auto ncount = torch::empty({s.T}, opts);
  auto depth = torch::zeros({s.T, max_nodes}, opts);

  ifa::launch_build_forest_large(
      row_dtype(X), X.data_ptr(), s.xl.rs, s.xl.cs,
      bag_idx.data_ptr<int64_t>(), (uint32_t*)scratch.data_ptr<int32_t>(),
      feat_sub.data_ptr<int32_t>(), feat.data_ptr<int32_t>(),
      value.data_ptr<float>(), right.data_ptr<int32_t>(),
      count.data_ptr<int32_t>(), ncount.data_ptr<int32_t>(),
      depth.data_ptr<int32_t>(), leaf_lut.data_ptr<float>(), (uint64_t)seed,
      (int32_t)tree_id_offset, (int32_t)s.T, (int32_t)s.n, (int32_t)s.k,
      (int32_t)max_nodes, (int32_t)height_limit, (int)threads, lds,
      current_stream());
  return {feat, value, right, count, ncount, depth};
}

std::vector<torch::Tensor> build_extended_forest_large(
    torch::Tensor X, torch::Tensor bag_idx, torch::Tensor feat_sub,
    int64_t seed, int64_t tree_id_offset, torch::Tensor leaf_lut, int64_t nnz,
    int64_t max_nodes, int64_t height_limit, int64_t threads) {
  const LargeBuildShape s =
      check_large_build(X, bag_idx, feat_sub, leaf_lut, tree_id_offset,
                        max_nodes, height_limit, nnz, true, threads);
  // coff[nnz] i64 | avail[k] i32 | coords[nnz] i32 | wf[nnz] f32 | stack
  const size_t lds =
      align16(8 * nnz + 4 * s.k + 8 * nnz) + (height_limit + 8) * 16 + 16;
  TORCH_CHECK(lds + kLargeBuildStaticLds <= kMaxLds,
              "build LDS request too large");

  auto opts = bag_idx.options().dtype(torch::kInt32);
  auto fopts = bag_idx.options().dtype(torch::kFloat32);
  auto scratch = torch::empty({s.T, 2, s.n}, opts);
  auto feat = torch::empty({s.T, max_nodes}, opts);
  auto value = torch::empty({s.T, max_nodes}, fopts);
  auto right = torch::full({s.T, max_nodes}, -1, opts);
  auto count = torch::empty({s.T, max_nodes}, opts);
  auto ncount = torch::empty({s.T}, opts);
  auto hidx = torch::zeros({s.T, max_nodes, nnz}, opts);
  auto hw = torch::zeros({s.T, max_nodes, nnz}, fopts);
  auto off64 = torch::zeros({s.T, max_nodes},
                            bag_idx.options().dtype(torch::kFloat64));
  auto depth = torch::zeros({s.T, max_nodes}, opts);

  ifa::launch_build_extended_forest_large(
      row_dtype(X), X.data_ptr(), s.xl.rs, s.xl.cs,
      bag_idx.data_ptr<int64_t>(), (uint32_t*)scratch.data_ptr<int32_t>(),
      feat_sub.data_ptr<int32_t>(), feat.data_ptr<int32_t>(),
      value.data_ptr<float>(), right.data_ptr<int32_t>(),
      count.data_ptr<int32_t>(), ncount.data_ptr<int32_t>(),
      hidx.data_ptr<int32_t>(), hw.data_ptr<float>(),
      off64.data_ptr<double>(), depth.data_ptr<int32_t>(),
      leaf_lut.data_ptr<float>(), (uint64_t)seed, (int32_t)tree_id_offset,
      (int32_t)s.T, (int32_t)s.n, (int32_t)s.k, (int32_t)nnz,
      (int32_t)max_nodes, (int32_t)height_limit, (int)threads, lds,
      current_stream());
  return {feat, value, right, count, ncount, hidx, hw, off64, depth};
}

// pre-order v4 records (what the packers emit) -> the level-order records
// score_forest walks; see v4_level_order_kernel
torch::Tensor v4_level_order(torch::Tensor nodes_packed,
                             torch::Tensor ncount) {
  CHECK_CUDA(nodes_packed);
  CHECK_CONTIG(nodes_packed);
  CHECK_CUDA(ncount);
  CHECK_CONTIG(ncount);
  TORCH_CHECK(nodes_packed.dim() == 3 && nodes_packed.size(2) == 2 &&
                  nodes_packed.scalar_type() == torch::kInt32,
              "nodes must be packed int32 [Tpad, max_nodes, 2]");
  TORCH_CHECK(ncount.scalar_type() == torch::kInt32 && ncount.dim() == 1 &&
                  ncount.size(0) == nodes_packed.size(0),
              "ncount must be int32 [Tpad]");
  TORCH_CHECK(nodes_packed.size(1) >= 1 && nodes_packed.size(1) <= 32767,
              "packed node ids are 15 bits");
  auto out = torch::empty_like(nodes_packed);
  if (nodes_packed.size(0) == 0) return out;
  ifa::launch_v4_level_order(nodes_packed.data_ptr<int32_t>(),
                             ncount.data_ptr<int32_t>(),
                             out.data_ptr<int32_t>(),
                             (int32_t)nodes_packed.size(0),
                             (int32_t)nodes_packed.size(1), current_stream());
  return out;
}

// pre-order v4 records with 16-bit key thresholds -> the heap records
// score_forest_heap walks (see v4_heap_order_kernel), laid out for the
// instantiation pick_score_cfg chooses for (d, max_nodes, height)
torch::Tensor v4_heap_order(torch::Tensor nodes_packed, torch::Tensor ncount,
                            int64_t height, int64_t d) {
  CHECK_CUDA(nodes_packed);
  CHECK_CONTIG(nodes_packed);
  CHECK_CUDA(ncount);
  CHECK_CONTIG(ncount);
  TORCH_CHECK(nodes_packed.dim() == 3 && nodes_packed.size(2) == 2 &&
                  nodes_packed.scalar_type() == torch::kInt32,
              "nodes must be packed int32 [Tpad, max_nodes, 2]");
  TORCH_CHECK(ncount.scalar_type() == torch::kInt32 && ncount.dim() == 1 &&
                  ncount.size(0) == nodes_packed.size(0),
              "ncount must be int32 [Tpad]");
  TORCH_CHECK(nodes_packed.size(1) >= 1 && nodes_packed.size(1) <= 32767,
              "packed node ids are 15 bits");
  const ScoreCfg cfg = pick_score_cfg(2, d, nodes_packed.size(1), height);
  TORCH_CHECK(cfg.heap, "no heap route for d=", d, " max_nodes=",
              nodes_packed.size(1), " height=", height);
  auto out = torch::empty({nodes_packed.size(0), (int64_t)2 << height},
                          nodes_packed.options());
  if (nodes_packed.size(0) == 0) return out;
  ifa::launch_v4_heap_order(nodes_packed.data_ptr<int32_t>(),
                            ncount.data_ptr<int32_t>(),
                            out.data_ptr<int32_t>(),
                            (int32_t)nodes_packed.size(0),
                            (int32_t)nodes_packed.size(1), (int32_t)height,
                            cfg.heap_rpt * 256 * 2, current_stream());
  return out;
}

// which kernel family score_forest runs for these shapes: "heap", "v4",
// "v4_global_nodes" (nodes walked from L2) or "v4_global_rows" (rows too).
// `layout` ("packed", "pitched", "feature_major") picks an entry point of
// the same family, never another route.
std::string score_route(const std::string& dtype, int64_t d,
                        int64_t max_nodes, int64_t height,
                        const std::string& layout) {
  TORCH_CHECK(dtype == "bf16" || dtype == "f16" || dtype == "f32",
              "dtype must be bf16, f16 or f32");
  TORCH_CHECK(layout == "packed" || layout == "pitched" ||
                  layout == "feature_major",
              "layout must be packed, pitched or feature_major");
  const ScoreCfg cfg =
      pick_score_cfg(dtype == "f32" ? 4 : 2, d, max_nodes, height);
  if (cfg.heap) return "heap";
  if (!cfg.rows_lds) return "v4_global_rows";
  return cfg.nodes_lds ? "v4" : "v4_global_nodes";
}

// (trees per barrier phase, rows per thread) of the heap instantiation
// these shapes run, or (0, 0) where score_route is not "heap"
std::pair<int64_t, int64_t> score_heap_cfg(const std::string& dtype,
                                           int64_t d, int64_t max_nodes,
                                           int64_t height) {
  TORCH_CHECK(dtype == "bf16" || dtype == "f16" || dtype == "f32",
              "dtype must be bf16, f16 or f32");
  const ScoreCfg cfg =
      pick_score_cfg(dtype == "f32" ? 4 : 2, d, max_nodes, height);
  if (!cfg.heap) return {0, 0};
  return {cfg.heap_phase, cfg.heap_rpt};
}

// threads per block of the heap instantiation these shapes run (256, or 512
// where a 512-row tile is walked one row per thread), 0 off the heap route
int64_t score_heap_block(const std::string& dtype, int64_t d,
                         int64_t max_nodes, int64_t height) {
  TORCH_CHECK(dtype == "bf16" || dtype == "f16" || dtype == "f32",
              "dtype must be bf16, f16 or f32");
  const ScoreCfg cfg =
      pick_score_cfg(dtype == "f32" ? 4 : 2, d, max_nodes, height);
  return cfg.heap ? cfg.heap_threads : 0;
}

torch::Tensor score_forest(torch::Tensor X, torch::Tensor nodes_packed,
                           torch::Tensor ncount, int64_t num_trees,
                           int64_t height_limit, double c_norm,
                           bool finalize,
                           c10::optional<torch::Tensor> heap) {
  CHECK_CUDA(X);
  CHECK_CUDA(nodes_packed);
  CHECK_CONTIG(nodes_packed);
  CHECK_CUDA(ncount);
  check_x(X);
  const XLayout xl = check_x_layout(X);
  TORCH_CHECK(nodes_packed.dim() == 3 && nodes_packed.size(2) == 2 &&
                  nodes_packed.scalar_type() == torch::kInt32,
              "nodes must be packed int32 [Tpad, max_nodes, 2]");
  int64_t N = X.size(0), d = X.size(1);
  int64_t Tpad = nodes_packed.size(0), max_nodes = nodes_packed.size(1);
  TORCH_CHECK(Tpad % 8 == 0, "packed tree count must be padded to 8");
  TORCH_CHECK(d <= 4094, "scoring supports d <= 4094 (12-bit feature field "
                         "plus the leaf sentinel column)");
  auto out = torch::empty({N}, X.options().dtype(torch::kFloat32));
  if (N == 0) return out;

  const ifa::RowDtype dt = row_dtype(X);
  const ScoreCfg cfg = pick_score_cfg(ifa::row_elem_bytes(dt), d, max_nodes,
                                      height_limit);
  if (cfg.heap && heap.has_value()) {
    const torch::Tensor& hp = *heap;
    CHECK_CUDA(hp);
    CHECK_CONTIG(hp);
    TORCH_CHECK(hp.dim() == 2 && hp.scalar_type() == torch::kInt32 &&
                    hp.size(0) == Tpad &&
                    hp.size(1) == ((int64_t)2 << height_limit),
                "heap records must be int32 [Tpad, 2^(height+1)]");
    // rows per thread of the instantiation: the tile's rows over its threads
    const int rpt = cfg.heap_rpt * 256 / cfg.heap_threads;
    const int64_t tiles = (N + cfg.heap_rpt * 256 - 1) / (cfg.heap_rpt * 256);
    // 8192 blocks at the most. A grid of one block per resident slot, or a
    // small multiple of that, was measured: it lost, or (10 per slot) did
    // not clear the noise rule (profiles/score_waves.md).
    // IFA_HEAP_MAX_BLOCKS=<n> lowers the limit so that tests reach the
    // grid-stride loop at small N.
    int64_t max_blocks = 8192;
    if (const char* e = getenv("IFA_HEAP_MAX_BLOCKS")) {
      const int64_t v = atoll(e);
      if (v >= 1) max_blocks = std::min<int64_t>(v, 8192);
    }
    int blocks = (int)std::min<int64_t>(tiles, max_blocks);
    const hipError_t err = ifa::launch_score_forest_heap(
        dt, rpt, cfg.heap_phase, cfg.heap_threads, X.data_ptr(),
        hp.data_ptr<int32_t>(), out.data_ptr<float>(), N, (int32_t)d, xl.rs,
        xl.cs, (int32_t)Tpad, (int32_t)height_limit, (float)num_trees,
        (float)c_norm, finalize ? 1 : 0, cfg.heap_lds, blocks,
        current_stream());
    TORCH_CHECK(err == hipSuccess, "score_forest_heap launch failed (",
                cfg.heap_threads, " threads, ", cfg.heap_lds, " B of LDS): ",
                hipGetErrorString(err));
    return out;
  }
  const int rpt = cfg.rpt, ilp = cfg.ilp;
  const bool rows_lds = cfg.rows_lds, nodes_lds = cfg.nodes_lds;
  const size_t lds = cfg.lds;
  int64_t rows_per_block = (int64_t)(rows_lds ? rpt : 1) * 256;
  int blocks = (int)std::min<int64_t>(
      (N + rows_per_block - 1) / rows_per_block, 8192);
  ifa::launch_score_forest(dt, rpt, rows_lds, nodes_lds, ilp, X.data_ptr(),
                           nodes_packed.data_ptr<int32_t>(),
                           ncount.data_ptr<int32_t>(), out.data_ptr<float>(),
                           N, (int32_t)d, xl.rs, xl.cs, (int32_t)Tpad,
                           (int32_t)max_nodes, (int32_t)height_limit,
                           (float)num_trees, (float)c_norm, finalize ? 1 : 0,
                           lds, blocks, current_stream());
  return out;
}


torch::Tensor score_extended_forest(torch::Tensor X,
                                    torch::Tensor nodes_packed,
                                    torch::Tensor hidx, torch::Tensor hw,
                                    torch::Tensor ncount, double c_norm,
                                    bool finalize) {
  CHECK_CUDA(X);
  CHECK_CUDA(nodes_packed);
  CHECK_CONTIG(nodes_packed);
  CHECK_CUDA(hidx);
  CHECK_CONTIG(hidx);
  CHECK_CUDA(hw);
  CHECK_CONTIG(hw);
  check_x(X);
  const XLayout xl = check_x_layout(X);
  TORCH_CHECK(nodes_packed.dim() == 3 && nodes_packed.size(2) == 2 &&
                  nodes_packed.scalar_type() == torch::kInt32,
              "nodes must be packed int32 [T, max_nodes, 2]");
  int64_t N = X.size(0), d = X.size(1);
  int64_t T = nodes_packed.size(0), max_nodes = nodes_packed.size(1);
  int64_t nnz = hidx.size(2);
  TORCH_CHECK(d <= 4095, "scoring supports d <= 4095");
  auto out = torch::empty({N}, X.options().dtype(torch::kFloat32));
  if (N == 0) return out;

  const ifa::RowDtype dt = row_dtype(X);
  const size_t elem = (size_t)ifa::row_elem_bytes(dt);
  const size_t pad = 16 / elem;
  size_t row_bytes = (size_t)256 * (d + pad) * elem;
  size_t node_bytes = (size_t)max_nodes * 8;
  int blocks = (int)std::min<int64_t>((N + 255) / 256, 8192);

  if (nnz == d && (d % 4) == 0 && node_bytes <= 120 * 1024) {
    // fully-extended dense hyperplanes: implicit indices, vectorized dot.
    // 8-B-aligned row stride for the uint2/float4 row reads.
    int64_t pad4 = (4 - (d % 4)) % 4;
    int64_t dpad = d + (pad4 == 0 ? 4 : pad4);
    size_t drow_bytes = (size_t)256 * dpad * elem;
    size_t w_bytes = (size_t)max_nodes * d * 4;
    bool wlds = node_bytes + w_bytes + drow_bytes <= 152 * 1024;
    bool rows_lds =
        node_bytes + (wlds ? w_bytes : 0) + drow_bytes <= 152 * 1024;
    size_t lds = node_bytes + (wlds ? w_bytes : 0) + (rows_lds ? drow_bytes : 0);
    ifa::launch_score_extended_dense(
        dt, rows_lds, wlds, X.data_ptr(), nodes_packed.data_ptr<int32_t>(),
        hw.data_ptr<float>(), ncount.data_ptr<int32_t>(), out.data_ptr<float>(),
        N, (int32_t)d, xl.rs, xl.cs, (int32_t)dpad, (int32_t)T,
        (int32_t)max_nodes, (float)T, (float)c_norm, finalize ? 1 : 0, lds,
        blocks, current_stream());
    return out;
  }

  // deep forests: stage what fits, walk the rest from global/L2
  bool nodes_lds = node_bytes <= 120 * 1024;
  size_t nb = nodes_lds ? node_bytes : 0;
  size_t hyper_bytes = (size_t)max_nodes * nnz * 8;
  bool hyper_lds = nb + hyper_bytes <= 96 * 1024;
  bool rows_lds =
      nb + (hyper_lds ? hyper_bytes : 0) + row_bytes <= 144 * 1024;
  size_t lds =
      nb + (hyper_lds ? hyper_bytes : 0) + (rows_lds ? row_bytes : 0);
  ifa::launch_score_extended_forest(
      dt, rows_lds, hyper_lds, nodes_lds, X.data_ptr(),
      nodes_packed.data_ptr<int32_t>(), hidx.data_ptr<int32_t>(),
      hw.data_ptr<float>(), ncount.data_ptr<int32_t>(), out.data_ptr<float>(),
      N, (int32_t)d, xl.rs, xl.cs, (int32_t)T, (int32_t)max_nodes,
      (int32_t)nnz, (float)T,
      (float)c_norm, finalize ? 1 : 0, lds, blocks, current_stream());
  return out;
}

torch::Tensor score_extended_dense_v2(torch::Tensor X,
                                      torch::Tensor nodes_packed,
                                      torch::Tensor values, torch::Tensor hw,
                                      torch::Tensor ncount,
                                      int64_t height_limit, double c_norm,
                                      bool finalize) {
  CHECK_CUDA(X);
  CHECK_CUDA(nodes_packed);
  CHECK_CONTIG(nodes_packed);
  CHECK_CUDA(values);
  CHECK_CONTIG(values);
  CHECK_CUDA(hw);
  CHECK_CONTIG(hw);
  CHECK_CUDA(ncount);
  check_x(X);
  const XLayout xl = check_x_layout(X);
  TORCH_CHECK(nodes_packed.dim() == 3 && nodes_packed.size(2) == 2 &&
                  nodes_packed.scalar_type() == torch::kInt32,
              "nodes must be packed int32 [T, max_nodes, 2]");
  TORCH_CHECK(hw.dim() == 3 && hw.scalar_type() == torch::kFloat32,
              "hw must be float32 [T, max_nodes, d]");
  int64_t N = X.size(0), d = X.size(1);
  int64_t T = nodes_packed.size(0), max_nodes = nodes_packed.size(1);
  TORCH_CHECK(d <= 64, "dense v2 supports d <= 64");
  const int D = d <= 8 ? 8 : (d <= 16 ? 16 : (d <= 32 ? 32 : 64));
  TORCH_CHECK(hw.size(2) == D, "hw must be host-padded to D columns");
  auto out = torch::empty({N}, X.options().dtype(torch::kFloat32));
  if (N == 0) return out;

  size_t lds = (size_t)max_nodes * 12 + 16 + (size_t)max_nodes * (D / 4 + 1) * 16;
  TORCH_CHECK(lds <= kMaxLds, "tree too large for LDS staging");
  int blocks = (int)std::min<int64_t>((N + 511) / 512, 8192);
  ifa::launch_score_extended_dense_v2(
      row_dtype(X), D, X.data_ptr(), nodes_packed.data_ptr<int32_t>(),
      values.data_ptr<float>(), hw.data_ptr<float>(),
      ncount.data_ptr<int32_t>(), out.data_ptr<float>(), N, (int32_t)d, xl.rs,
      xl.cs, (int32_t)T, (int32_t)max_nodes, (int32_t)height_limit, (float)T,
      (float)c_norm, finalize ? 1 : 0, lds, blocks, current_stream());
  // rows with an inf/NaN cell: strict-order rescoring (see the kernel)
  ifa::launch_score_extended_dense_nonfinite_rows(
      row_dtype(X), false, X.data_ptr(), nodes_packed.data_ptr<int32_t>(),
      values.data_ptr<float>(), hw.data_ptr<float>(), out.data_ptr<float>(),
      N, (int32_t)d, xl.rs, xl.cs, (int32_t)D, (int32_t)T, (int32_t)max_nodes,
      (int32_t)height_limit, (float)T, (float)c_norm, finalize ? 1 : 0,
      (int)std::min<int64_t>((N + 255) / 256, 8192), current_stream());
  return out;
}

torch::Tensor score_extended_dense_v3(torch::Tensor X,
                                      torch::Tensor nodes_packed,
                                      torch::Tensor values, torch::Tensor hwp,
                                      torch::Tensor ncount,
                                      int64_t height_limit, double c_norm,
                                      bool finalize) {
  CHECK_CUDA(X);
  CHECK_CUDA(nodes_packed);
  CHECK_CONTIG(nodes_packed);
  CHECK_CUDA(values);
  CHECK_CONTIG(values);
  CHECK_CUDA(hwp);
  CHECK_CONTIG(hwp);
  CHECK_CUDA(ncount);
  check_x(X);
  const XLayout xl = check_x_layout(X);
  TORCH_CHECK(is_bf16(X),
              "dense v3 requires bf16 rows (f32/fp16 rows route to v2)");
  TORCH_CHECK(nodes_packed.dim() == 3 && nodes_packed.size(2) == 2 &&
                  nodes_packed.scalar_type() == torch::kInt32,
              "nodes must be packed int32 [T, max_nodes, 2]");
  TORCH_CHECK(hwp.dim() == 3 && hwp.scalar_type() == torch::kInt32,
              "hwp must be int32 [T, max_nodes, D/2] packed bf16 pairs");
  int64_t N = X.size(0), d = X.size(1);
  int64_t T = nodes_packed.size(0), max_nodes = nodes_packed.size(1);
  TORCH_CHECK(d <= 128, "dense v3 supports d <= 128");
  const int D = d <= 8 ? 8
                       : (d <= 16 ? 16
                                  : (d <= 32 ? 32 : (d <= 64 ? 64 : 128)));
  TORCH_CHECK(hwp.size(2) == D / 2, "hwp must be packed to D/2 dwords");
  auto out = torch::empty({N}, X.options().dtype(torch::kFloat32));
  if (N == 0) return out;

  size_t lds = (size_t)max_nodes * 12 + 16 + (size_t)max_nodes * (D / 8 + 1) * 16;
  TORCH_CHECK(lds <= kMaxLds, "tree too large for LDS staging");
  const char* rpt_env = getenv("IFA_EIF_V3_RPT2");
  const bool rpt2 = rpt_env && rpt_env[0] == '1';
  const int rows_per_iter = (D >= 64 || (D == 32 && !rpt2)) ? 512 : 1024;
  int blocks = (int)std::min<int64_t>(
      (N + rows_per_iter - 1) / rows_per_iter, 8192);
  ifa::launch_score_extended_dense_v3(
      D, rpt2, X.data_ptr(), nodes_packed.data_ptr<int32_t>(),
      values.data_ptr<float>(), (const uint32_t*)hwp.data_ptr<int32_t>(),
      ncount.data_ptr<int32_t>(), out.data_ptr<float>(), N, (int32_t)d, xl.rs,
      xl.cs, (int32_t)T, (int32_t)max_nodes, (int32_t)height_limit, (float)T,
      (float)c_norm, finalize ? 1 : 0, lds, blocks, current_stream());
  // rows with an inf/NaN cell: strict-order rescoring (see the kernel)
  ifa::launch_score_extended_dense_nonfinite_rows(
      ifa::ROW_BF16, true, X.data_ptr(), nodes_packed.data_ptr<int32_t>(),
      values.data_ptr<float>(), hwp.data_ptr<int32_t>(), out.data_ptr<float>(),
      N, (int32_t)d, xl.rs, xl.cs, (int32_t)D, (int32_t)T, (int32_t)max_nodes,
      (int32_t)height_limit, (float)T, (float)c_norm, finalize ? 1 : 0,
      (int)std::min<int64_t>((N + 255) / 256, 8192), current_stream());
  return out;
}

torch::Tensor score_extended_sparse_v2(torch::Tensor X,
                                       torch::Tensor nodes_packed,
                                       torch::Tensor values,
                                       torch::Tensor hidx, torch::Tensor hw,
                                       torch::Tensor ncount,
                                       int64_t height_limit, double c_norm,
                                       bool finalize) {
  CHECK_CUDA(X);
  CHECK_CUDA(nodes_packed);
  CHECK_CONTIG(nodes_packed);
  CHECK_CUDA(values);
  CHECK_CONTIG(values);
  CHECK_CUDA(hidx);
  CHECK_CONTIG(hidx);
  CHECK_CUDA(hw);
  CHECK_CONTIG(hw);
  CHECK_CUDA(ncount);
  check_x(X);
  const XLayout xl = check_x_layout(X);
  int64_t N = X.size(0), d = X.size(1);
  int64_t T = nodes_packed.size(0), max_nodes = nodes_packed.size(1);
  int64_t nnz = hidx.size(2);
  TORCH_CHECK(nnz >= 1 && nnz <= 5, "sparse v2 supports nnz <= 5");
  auto out = torch::empty({N}, X.options().dtype(torch::kFloat32));
  if (N == 0) return out;

  const ifa::RowDtype dt = row_dtype(X);
  const size_t elem = (size_t)ifa::row_elem_bytes(dt);
  int64_t dpad = d;
  if (elem == 2) {
    while (dpad % 4 != 2) ++dpad;
  } else {
    while (dpad % 2 != 1) ++dpad;
  }
  size_t lds = (size_t)max_nodes * (12 + nnz * 8)
               + (size_t)2 * 256 * dpad * elem;
  TORCH_CHECK(lds <= 150 * 1024, "sparse v2 LDS overflow; use general path");
  int blocks = (int)std::min<int64_t>((N + 511) / 512, 8192);
  ifa::launch_score_extended_sparse_v2(
      dt, (int)nnz, X.data_ptr(), nodes_packed.data_ptr<int32_t>(),
      values.data_ptr<float>(), hidx.data_ptr<int32_t>(), hw.data_ptr<float>(),
      ncount.data_ptr<int32_t>(), out.data_ptr<float>(), N, (int32_t)d, xl.rs,
      xl.cs, (int32_t)dpad, (int32_t)T, (int32_t)max_nodes,
      (int32_t)height_limit, (float)T, (float)c_norm, finalize ? 1 : 0, lds,
      blocks, current_stream());
  return out;
}

torch::Tensor score_forest_wide(torch::Tensor X, torch::Tensor nodes_wide,
                                int64_t height_limit, double c_norm,
                                bool finalize) {
  CHECK_CUDA(X);
  CHECK_CUDA(nodes_wide);
  CHECK_CONTIG(nodes_wide);
  check_x(X);
  const XLayout xl = check_x_layout(X);
  TORCH_CHECK(nodes_wide.dim() == 3 && nodes_wide.size(2) == 4 &&
                  nodes_wide.scalar_type() == torch::kInt32,
              "nodes must be wide int32 [T, max_nodes, 4]");
  int64_t N = X.size(0), d = X.size(1);
  int64_t T = nodes_wide.size(0), max_nodes = nodes_wide.size(1);
  auto out = torch::empty({N}, X.options().dtype(torch::kFloat32));
  if (N == 0) return out;
  int blocks = (int)std::min<int64_t>((N + 255) / 256, 8192);
  ifa::launch_score_forest_wide(
      row_dtype(X), X.data_ptr(), nodes_wide.data_ptr<int32_t>(),
      out.data_ptr<float>(), N, (int32_t)d, xl.rs, xl.cs, (int32_t)T, max_nodes,
      (int32_t)height_limit, (float)T, (float)c_norm, finalize ? 1 : 0,
      blocks, current_stream());
  return out;
}

torch::Tensor score_extended_wide(torch::Tensor X, torch::Tensor nodes_wide,
                                  torch::Tensor hidx, torch::Tensor hw,
                                  double c_norm, bool finalize) {
  CHECK_CUDA(X);
  CHECK_CUDA(nodes_wide);
  CHECK_CONTIG(nodes_wide);
  CHECK_CUDA(hidx);
  CHECK_CONTIG(hidx);
  CHECK_CUDA(hw);
  CHECK_CONTIG(hw);
  check_x(X);
  const XLayout xl = check_x_layout(X);
  TORCH_CHECK(nodes_wide.dim() == 3 && nodes_wide.size(2) == 4 &&
                  nodes_wide.scalar_type() == torch::kInt32,
              "nodes must be wide int32 [T, max_nodes, 4]");
  int64_t N = X.size(0), d = X.size(1);
  int64_t T = nodes_wide.size(0), max_nodes = nodes_wide.size(1);
  int64_t nnz = hidx.size(2);
  auto out = torch::empty({N}, X.options().dtype(torch::kFloat32));
  if (N == 0) return out;
  int blocks = (int)std::min<int64_t>((N + 255) / 256, 8192);
  ifa::launch_score_extended_wide(
      row_dtype(X), X.data_ptr(), nodes_wide.data_ptr<int32_t>(),
      hidx.data_ptr<int32_t>(), hw.data_ptr<float>(), out.data_ptr<float>(), N,
      (int32_t)d, xl.rs, xl.cs, (int32_t)T, max_nodes, (int32_t)nnz, (float)T,
      (float)c_norm, finalize ? 1 : 0, blocks, current_stream());
  return out;
}

// Per-feature attribution, standard forests (explain_forest_kernel).
// Returns the f32 [N, d] contribution matrix (raw sums when !finalize).
torch::Tensor explain_forest(torch::Tensor X, torch::Tensor nodes_explain,
                             torch::Tensor ncount, int64_t height_limit,
                             bool finalize) {
  CHECK_CUDA(X);
  CHECK_CUDA(nodes_explain);
  CHECK_CONTIG(nodes_explain);
  CHECK_CUDA(ncount);
  CHECK_CONTIG(ncount);
  check_x(X);
  const XLayout xl = check_x_layout(X);
  TORCH_CHECK(nodes_explain.dim() == 3 && nodes_explain.size(2) == 4 &&
                  nodes_explain.scalar_type() == torch::kInt32,
              "nodes must be explain records int32 [T, max_nodes, 4]");
  int64_t N = X.size(0), d = X.size(1);
  int64_t T = nodes_explain.size(0), max_nodes = nodes_explain.size(1);
  TORCH_CHECK(ncount.scalar_type() == torch::kInt32 && ncount.dim() == 1 &&
                  ncount.size(0) == T,
              "ncount must be int32 [T]");
  TORCH_CHECK(T >= 1, "explain needs at least one tree");
  TORCH_CHECK(d >= 1 && d <= 4094,
              "explain supports 1 <= d <= 4094 (12-bit feature field plus "
              "the leaf sentinel column)");
  TORCH_CHECK(max_nodes >= 1 && max_nodes <= 32767,
              "explain records hold 15-bit node ids");
  TORCH_CHECK(height_limit >= 1, "height_limit must be >= 1");
  const auto out_opts = X.options().dtype(torch::kFloat32);
  if (N == 0) return torch::empty({N, d}, out_opts);

  const ifa::RowDtype dt = row_dtype(X);
  const size_t elem = (size_t)ifa::row_elem_bytes(dt);
  const size_t budget = 150 * 1024;
  // odd-WORD strides (all LDS banks hit) with room for column d: the key
  // sentinel in the row tile, the self-loop sink in the accumulator tile
  int64_t dpad = d + 1;
  if (elem == 2) {
    while (dpad % 4 != 2) ++dpad;
  } else {
    while (dpad % 2 != 1) ++dpad;
  }
  const int64_t astride = (d + 1) | 1;
  const size_t tree_b = (size_t)max_nodes * 16;
  const size_t rows_b = (size_t)256 * dpad * elem;
  const size_t acc_b = (size_t)256 * astride * 4;
  // deep forests overflow LDS node staging: records come from global/L2
  const bool nodes_lds = tree_b <= 64 * 1024;
  const size_t nb1 = nodes_lds ? tree_b : 0;
  // accumulator routing: LDS tile, else the pre-zeroed out itself; rows
  // that do not fit even alone are read from X
  int mode = nb1 + rows_b + acc_b <= budget ? 0
             : (nb1 + rows_b <= budget ? 1 : 2);
  if (const char* e = getenv("IFA_EXPLAIN_FORCE_GLOBAL_ACC"))
    if (atoi(e) && mode == 0) mode = 1;
  // the LDS-tile flush writes every cell; the global routes add into out
  auto out = mode == 0 ? torch::empty({N, d}, out_opts)
                       : torch::zeros({N, d}, out_opts);
  // (rpt, trees per barrier): most resident blocks first, then rows per
  // thread (independent chains), then fewer barriers
  const size_t row_unit = mode == 0 ? rows_b + acc_b : (mode == 1 ? rows_b : 0);
  int rpt = 1, tps = 1;
  size_t lds = nb1 + row_unit;
  {
    int best_blocks = 0, best_rpt = 0, best_tps = 0;
    for (int r = (mode == 0 ? 2 : 1); r >= 1; --r) {
      for (int s = 4; s >= 1; s >>= 1) {
        if (!nodes_lds && s != 1) continue;
        size_t l = (size_t)s * nb1 + (size_t)r * row_unit;
        if (l > budget) continue;
        int blocks_cu =
            (int)std::min<size_t>(kMaxLds / std::max(l, (size_t)1), 4);
        if (blocks_cu > best_blocks ||
            (blocks_cu == best_blocks &&
             (r > best_rpt || (r == best_rpt && s > best_tps)))) {
          best_blocks = blocks_cu;
          best_rpt = r;
          best_tps = s;
          rpt = r;
          tps = s;
          lds = l;
        }
      }
    }
  }
  if (!nodes_lds) tps = (int)std::min<int64_t>(T, 1 << 30);  // one barrier
  int64_t max_blocks = 8192;
  if (const char* e = getenv("IFA_EXPLAIN_MAX_BLOCKS")) {
    const int64_t v = atoll(e);
    if (v >= 1) max_blocks = std::min<int64_t>(v, 8192);
  }
  const int64_t rows_per_block = (int64_t)rpt * 256;
  int blocks = (int)std::min<int64_t>(
      (N + rows_per_block - 1) / rows_per_block, max_blocks);
  ifa::launch_explain_forest(
      dt, mode, rpt, nodes_lds, X.data_ptr(), nodes_explain.data_ptr<int32_t>(),
      ncount.data_ptr<int32_t>(), out.data_ptr<float>(), N, (int32_t)d, xl.rs,
      xl.cs, (int32_t)dpad, (int32_t)astride, (int32_t)T, (int32_t)max_nodes,
      (int32_t)tps, (int32_t)height_limit, (float)T, finalize ? 1 : 0, lds,
      blocks, current_stream());
  return out;
}

// Per-feature attribution, extended forests (explain_extended_kernel).
torch::Tensor explain_extended_forest(torch::Tensor X,
                                      torch::Tensor nodes_packed,
                                      torch::Tensor hidx, torch::Tensor hw,
                                      torch::Tensor dl, torch::Tensor dr,
                                      bool finalize) {
  CHECK_CUDA(X);
  CHECK_CUDA(nodes_packed);
  CHECK_CONTIG(nodes_packed);
  CHECK_CUDA(hidx);
  CHECK_CONTIG(hidx);
  CHECK_CUDA(hw);
  CHECK_CONTIG(hw);
  CHECK_CUDA(dl);
  CHECK_CONTIG(dl);
  CHECK_CUDA(dr);
  CHECK_CONTIG(dr);
  check_x(X);
  const XLayout xl = check_x_layout(X);
  TORCH_CHECK(nodes_packed.dim() == 3 && nodes_packed.size(2) == 2 &&
                  nodes_packed.scalar_type() == torch::kInt32,
              "nodes must be packed int32 [T, max_nodes, 2]");
  int64_t N = X.size(0), d = X.size(1);
  int64_t T = nodes_packed.size(0), max_nodes = nodes_packed.size(1);
  TORCH_CHECK(hidx.dim() == 3 && hidx.scalar_type() == torch::kInt32 &&
                  hidx.size(0) == T && hidx.size(1) == max_nodes,
              "hidx must be int32 [T, max_nodes, nnz]");
  int64_t nnz = hidx.size(2);
  TORCH_CHECK(hw.scalar_type() == torch::kFloat32 &&
                  hw.sizes() == hidx.sizes(),
              "hw must be float32 [T, max_nodes, nnz]");
  TORCH_CHECK(dl.scalar_type() == torch::kFloat32 &&
                  dl.sizes() == hidx.sizes() &&
                  dr.scalar_type() == torch::kFloat32 &&
                  dr.sizes() == hidx.sizes(),
              "edge deltas must be float32 [T, max_nodes, nnz]");
  TORCH_CHECK(T >= 1, "explain needs at least one tree");
  TORCH_CHECK(d >= 1 && d <= 4095, "explain supports 1 <= d <= 4095");
  TORCH_CHECK(max_nodes <= 32767, "packed records hold 15-bit node ids");
  auto out = torch::zeros({N, d}, X.options().dtype(torch::kFloat32));
  if (N == 0) return out;
  int64_t max_blocks = 8192;
  if (const char* e = getenv("IFA_EXPLAIN_MAX_BLOCKS")) {
    const int64_t v = atoll(e);
    if (v >= 1) max_blocks = std::min<int64_t>(v, 8192);
  }
  int blocks = (int)std::min<int64_t>((N + 255) / 256, max_blocks);
  ifa::launch_explain_extended(
      row_dtype(X), X.data_ptr(), nodes_packed.data_ptr<int32_t>(),
      hidx.data_ptr<int32_t>(), hw.data_ptr<float>(), dl.data_ptr<float>(),
      dr.data_ptr<float>(), out.data_ptr<float>(), N, (int32_t)d, xl.rs, xl.cs,
      (int32_t)T, (int32_t)max_nodes, (int32_t)nnz, (float)T, finalize ? 1 : 0,
      blocks, current_stream());
  return out;
}

// Exact TreeSHAP, standard forests (shap_forest_kernel, docs/DESIGN.md §9).
// `table` is the leaf-path word stream of gpu_engine._shap_packed for X's row
// kind, `tree_off` its per-tree word offsets: once on the host (checked
// here, it sizes the LDS staging) and once on the device (read by the
// kernel). Returns the f32 [N, d] SHAP matrix (raw sums when !finalize).
torch::Tensor shap_forest(torch::Tensor X, torch::Tensor table,
                          torch::Tensor tree_off_host, torch::Tensor tree_off,
                          torch::Tensor wtab, bool finalize) {
  CHECK_CUDA(X);
  CHECK_CUDA(table);
  CHECK_CONTIG(table);
  CHECK_CUDA(tree_off);
  CHECK_CONTIG(tree_off);
  CHECK_CUDA(wtab);
  CHECK_CONTIG(wtab);
  CHECK_CONTIG(tree_off_host);
  check_x(X);
  const XLayout xl = check_x_layout(X);
  TORCH_CHECK(table.dim() == 1 && table.scalar_type() == torch::kInt64,
              "table must be the int64 word stream");
  TORCH_CHECK(!tree_off_host.is_cuda() && tree_off_host.dim() == 1 &&
                  tree_off_host.scalar_type() == torch::kInt64 &&
                  tree_off_host.size(0) >= 2,
              "tree_off_host must be a host int64 [T + 1]");
  TORCH_CHECK(tree_off.dim() == 1 && tree_off.scalar_type() == torch::kInt64 &&
                  tree_off.size(0) == tree_off_host.size(0),
              "tree_off must be int64 [T + 1] like tree_off_host");
  TORCH_CHECK(wtab.scalar_type() == torch::kFloat64 && wtab.numel() == 17 * 16,
              "wtab must be float64 [17, 16]");
  const int64_t N = X.size(0), d = X.size(1);
  const int64_t T = tree_off_host.size(0) - 1;
  const int64_t* to = tree_off_host.data_ptr<int64_t>();
  TORCH_CHECK(to[0] == 0 && to[T] == table.numel(),
              "tree_off must span the table exactly");
  int64_t table_words = 0;
  for (int64_t t = 0; t < T; ++t) {
    TORCH_CHECK(to[t + 1] >= to[t], "tree_off must be non-decreasing");
    table_words = std::max(table_words, to[t + 1] - to[t]);
  }
  TORCH_CHECK(table_words < (int64_t)1 << 28, "one tree's table is too large");
  TORCH_CHECK(d >= 1 && d <= 4094, "shap supports 1 <= d <= 4094");
  const auto out_opts = X.options().dtype(torch::kFloat32);
  if (N == 0) return torch::empty({N, d}, out_opts);

  const ifa::RowDtype dt = row_dtype(X);
  const size_t elem = (size_t)ifa::row_elem_bytes(dt);
  const size_t budget = 150 * 1024;
  const size_t wtab_b = 17 * 16 * 8;
  const size_t keys_b = align16((size_t)256 * d * elem);
  const size_t acc_b = (size_t)256 * d * 8;
  const size_t table_b = (size_t)table_words * 8;
  // what goes to LDS, in this order of preference: the key tile, the
  // accumulators (touched once per term by every lane), one tree's table
  // (broadcast reads, L2 serves them well)
  const bool rows_lds = wtab_b + keys_b <= budget;
  size_t lds = wtab_b + (rows_lds ? keys_b : 0);
  // The accumulator tile is taken only while two blocks still fit a CU.
  // Measured (profiles/shap.md): with two or more resident blocks either
  // way the LDS tile is 3 % faster than the global scratch; a tile that
  // holds a CU to one block (one wave per SIMD) is 27 % slower than it.
  const size_t all_lds =
      lds + acc_b + (lds + acc_b + table_b <= budget ? table_b : 0);
  bool acc_lds = lds + acc_b <= budget && all_lds <= kMaxLds / 2;
  if (const char* e = getenv("IFA_SHAP_FORCE_GLOBAL_ACC"))
    if (atoi(e)) acc_lds = false;
  if (acc_lds) lds += acc_b;
  bool table_lds = lds + table_b <= budget;
  if (const char* e = getenv("IFA_SHAP_FORCE_GLOBAL_TABLE"))
    if (atoi(e)) table_lds = false;
  if (table_lds) lds += table_b;

  auto out = torch::empty({N, d}, out_opts);
  torch::Tensor acc_g;
  if (!acc_lds)
    acc_g = torch::zeros({N, d}, X.options().dtype(torch::kFloat64));
  int64_t max_blocks = 8192;
  if (const char* e = getenv("IFA_SHAP_MAX_BLOCKS")) {
    const int64_t v = atoll(e);
    if (v >= 1) max_blocks = std::min<int64_t>(v, 8192);
  }
  const int blocks = (int)std::min<int64_t>((N + 255) / 256, max_blocks);
  ifa::launch_shap_forest(
      dt, table_lds, acc_lds, X.data_ptr(), table.data_ptr<int64_t>(),
      tree_off.data_ptr<int64_t>(), wtab.data_ptr<double>(),
      acc_lds ? nullptr : acc_g.data_ptr<double>(), out.data_ptr<float>(), N,
      (int32_t)d, xl.rs, xl.cs, (int32_t)T, (int32_t)table_words,
      rows_lds ? 1 : 0, finalize ? 1 : 0, lds, blocks, current_stream());
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("bag_gather", &bag_gather, "gather per-tree bags (K9/K10)");
  m.def("build_forest", &build_forest, "build standard iTrees (K1/K2/K11)");
  m.def("build_extended_forest", &build_extended_forest,
        "build extended iTrees (K3-K5)");
  m.def("build_forest_large", &build_forest_large,
        "build standard iTrees over bags of any size, rows read in place",
        py::arg("X"), py::arg("bag_idx"), py::arg("feat_sub"), py::arg("seed"),
        py::arg("tree_id_offset"), py::arg("leaf_lut"), py::arg("max_nodes"),
        py::arg("height_limit"), py::arg("threads") = 256);
  m.def("build_extended_forest_large", &build_extended_forest_large,
        "build extended iTrees over bags of any size, rows read in place",
        py::arg("X"), py::arg("bag_idx"), py::arg("feat_sub"), py::arg("seed"),
        py::arg("tree_id_offset"), py::arg("leaf_lut"), py::arg("nnz"),
        py::arg("max_nodes"), py::arg("height_limit"),
        py::arg("threads") = 256);
  m.def("v4_level_order", &v4_level_order,
        "re-lay pre-order v4 node records in level order for score_forest");
  m.def("v4_heap_order", &v4_heap_order,
        "pre-order v4 node records -> 4-byte heap records (16-bit rows)");
  m.def("score_route", &score_route,
        "kernel family score_forest runs for (dtype, d, max_nodes, height, "
        "layout)");
  m.def("score_heap_block", &score_heap_block,
        "threads per block of the heap instantiation (0 off the heap route)",
        py::arg("dtype"), py::arg("d"), py::arg("max_nodes"),
        py::arg("height"));
  m.def("score_heap_cfg", &score_heap_cfg,
        "(trees per phase, rows per thread) of the heap walk for (dtype, d, "
        "max_nodes, height); (0, 0) off the heap route");
  m.def("score_forest", &score_forest, "batched path-length scoring (K6)",
        py::arg("X"), py::arg("nodes_packed"), py::arg("ncount"),
        py::arg("num_trees"), py::arg("height_limit"), py::arg("c_norm"),
        py::arg("finalize"), py::arg("heap") = py::none());
  m.def("score_extended_forest", &score_extended_forest,
        "batched EIF scoring (K7)");
  m.def("score_extended_sparse_v2", &score_extended_sparse_v2,
        "sparse EIF scoring, fixed-trip batched walk (K7 small-nnz path)");
  m.def("score_extended_dense_v2", &score_extended_dense_v2,
        "dense EIF scoring, rows-in-registers (K7 fast path)");
  m.def("score_extended_dense_v3", &score_extended_dense_v3,
        "dense EIF scoring, packed-bf16 weights + v_dot2c (K7 bf16 path)");
  m.def("score_forest_wide", &score_forest_wide,
        "wide-format standard scoring (no packed-field limits)");
  m.def("score_extended_wide", &score_extended_wide,
        "wide-format EIF scoring (no packed-field limits)");
  m.def("explain_forest", &explain_forest,
        "per-feature path-length attribution, standard forests");
  m.def("explain_extended_forest", &explain_extended_forest,
        "per-feature path-length attribution, extended forests");
  m.def("shap_forest", &shap_forest,
        "exact path-dependent TreeSHAP values, standard forests");
  m.attr("WAVE") = 64;
}
