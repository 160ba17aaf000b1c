// fx_api.cpp — context management and the batch driver behind include/fx.h.
//
// A context owns every device buffer (sized once from fx_limits: no allocation in the
// steady state), a stream, and lazily created pinned host mirrors.  fx_process_batch
// enqueues the stage kernels of fx_kernels.hip on the context's stream; with FX_OUT_HOST
// it also copies the results back and synchronises.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../../include/fx.h"
#include "fx_launch.h"
#include "fx_scan_query.h"

namespace {
thread_local std::string g_last_error;

fx_status fail(fx_status s, const std::string &msg) {
  g_last_error = msg;
  return s;
}
#define FX_HIP(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(e_ == hipErrorOutOfMemory ? FX_ERR_OOM : FX_ERR_HIP,                            \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                             \
  } while (0)

constexpr int kMetaSlots = 8;
// Test and experiment hooks read the environment only in the TEST build of the library (lib/libfx_hip_test.so, compiled
// with -DFX_TEST_HOOKS: feature_extraction_amd/build.py); the product library never changes tiers, grids or kernels because
// of the caller's environment.
inline const char *test_hook(const char *name) {
#ifdef FX_TEST_HOOKS
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
constexpr uint32_t kListCap = 4096, kDenseMin = 1024;
// default CSR block: 128 entries a row (1 KB: the dense pool's 7956 B / 8; the test scenes average 15 to 77 non-zero words)
constexpr uint32_t kCsrRowEntries = 128;

// The back end's per-context scratch (fx_match_descriptors_csr ... fx_map_update).  One policy for both types: a buffer that is
// large enough is used as it is — no allocation, no synchronisation; one that is not is replaced by a buffer of
// max(bytes, twice the old size, 4096) bytes, and the old one is freed only after the context's stream, which may still read
// it, was synchronised.  Buffers never shrink; a DevScratch is allocated at its first reserve whatever the size; fx_destroy
// releases them.
struct DevScratch {
  uint8_t *d = nullptr;
  size_t bytes = 0;
  fx_status reserve(fx_ctx *c, size_t need, const char *what);
  void release();
};
// Pinned host staging, its device twin and the event of the last upload, which the next call waits for before it writes
// the staging again.
struct Staging {
  uint8_t *h = nullptr, *d = nullptr;
  size_t bytes = 0;
  hipEvent_t ev = nullptr;
  fx_status reserve(fx_ctx *c, size_t need, const char *what);  // room for `need` bytes in h and d; h is free to write
  fx_status upload(fx_ctx *c, size_t n);                        // h[0, n) to d on the context's stream
  void release();
};
}  // namespace

struct fx_ctx {
  fx_params params;
  fx_limits lim;
  int device = 0;
  // the launch policy (csrc/fx_launch_plan.h): what is fixed for the context or set by a setter or a test hook, and what one
  // batch leaves for the next
  FxPlanConfig plan_cfg;
  FxPlanState plan_state;
  FxDevParams dp;
  FxBuffers buf;
  std::vector<void *> dev_allocs;
  std::vector<void *> host_allocs;
  hipStream_t own_stream = nullptr, stream = nullptr;
  // per-batch scan table: ring of pinned slots so back-to-back batches never overwrite one in flight
  FxScanMeta *h_meta[kMetaSlots] = {};
  hipEvent_t meta_ev[kMetaSlots] = {};
  bool meta_used[kMetaSlots] = {};
  int meta_next = 0;
  FxScanMeta *d_meta = nullptr;
  float box_margin = 0.f;
  uint32_t ring_lds_cap = 0;     // points a ring may have in the workgroup ring tier's LDS (<= max_ring_points; beyond: k_slow)
  uint32_t merge_huge_cap = 0;   // candidates the large merge tier (coordinates in HBM, tables in LDS) holds (<= max_candidates; beyond: k_slow)
  uint32_t merge_huge_ccap = 0;  // clusters the large merge tier can order (>= max_keypoints)
  // host-input staging
  float *d_stage = nullptr;
  uint32_t stage_stride = 0;  // record stride the staging buffer is sized for
  // pinned host mirrors (lazy)
  uint32_t *h_hdr = nullptr;  // the per-scan words' block (hdr_stride words an array, the device block's layout): one copy a batch
  size_t hdr_stride = 0;
  uint32_t *h_n_kp = nullptr, *h_kp_offset = nullptr, *h_flags = nullptr, *h_n_filt = nullptr, *h_n_kpc = nullptr,
           *h_n_cand = nullptr, *h_cand_size = nullptr, *h_kpc_cand = nullptr, *h_kp_size = nullptr,
           *h_kp_nbrs = nullptr;
  int32_t *h_cand_kp = nullptr;
  float *h_keypoints = nullptr, *h_desc = nullptr, *h_filtered = nullptr, *h_kpc = nullptr, *h_cand = nullptr;
  // profiling
  // profiling: a ring of event sets so a whole timed region can be read back afterwards
  bool profiling = false;
  std::vector<hipEvent_t> ev_ring;  // depth * (FX_N_STAGES + 1)
  uint32_t ev_depth = 0, ev_count = 0;
  uint32_t prof_mask = ~0u;        // stages that get events (bit i = stage i); fx_set_profiling_stages
  std::vector<uint32_t> ev_mask;   // the mask each ring slot was recorded with
  std::vector<uint64_t> ev_seq;    // the batch sequence number each ring slot belongs to (k_prep's clock slot)
  uint64_t batch_seq = 0;          // batches enqueued so far
  double clk_khz = 100000.0;       // rate of the device's constant clock
  hipEvent_t *ev = nullptr;  // set of the batch being enqueued
  // HIP graphs of the stage sequence, one per batch size (batches up to graph_max_batch)
  std::vector<std::pair<uint32_t, hipGraphExec_t>> graphs;
  uint32_t graph_max_batch = 0;
  bool debug_sync = false;
  // the previous batch's work for the rarely used tiers (pinned; written by the device: FxBuffers::tier_hint)
  volatile uint32_t *tier_hint = nullptr;
  // A batch that failed after its kernels were enqueued leaves state the next batch would build on: descriptor rows are
  // cleared by un-writing what the last batch recorded for them (desc_nbins / desc_bins), the work-list counters are
  // cleared by the batch's first kernel, the tier hints size the next grids.  The next batch then starts from scratch:
  // every row is cleared whole, counters and hints are reset (fx_process_batch).
  bool state_suspect = false;
  uint32_t fail_after = 0;     // test hook (FX_FAIL_AFTER_ENQUEUE = n: the n-th batch returns an error after its kernels were enqueued)
  // FX_OUT_DESC_CSR: the context's CSR block of descriptor rows (max_total_keypoints rows, csr_cap entries) and its pinned
  // mirror, allocated at the first batch that asks for it and grown (never shrunk) when a batch needs more entries
  uint8_t *d_csr = nullptr, *h_csr = nullptr;
  uint32_t csr_cap = 0;          // entries of the allocated block
  uint32_t csr_cap_want = 0;     // fx_set_descriptor_csr_capacity (0: max_total_keypoints * kCsrRowEntries)
  bool csr_resize = false;       // fx_set_descriptor_csr_capacity after the block was allocated: reallocate at the next use
  bool csr_valid = false;        // the last batch was FX_OUT_HOST | FX_OUT_DESC_CSR (fx_get_descriptors_csr)
  uint32_t csr_rows = 0, csr_nnz = 0;
  uint32_t csr_full_rows = 0;    // test hook (FX_CSR_FULL_ROWS): every row through the whole-row path
  // fx_match_descriptors_csr: the pairs and the work list (staged), and the blocks' row norms and the mutual table
  Staging match_stage;
  DevScratch match_scratch;
  Staging reg_stage;         // fx_register_matches: the pairs
  DevScratch track_scratch;  // fx_track_landmarks: the per-row scratch arrays
  DevScratch map_scratch;    // fx_map_update: the batch landmark's map id, the blocks' counts
  DevScratch merge_scratch;  // fx_map_merge: the grid (bucket counts, landmarks in bucket order), proposals, kept links;
                             // fx_map_localize: the same grid, then each row's landmark and distance;
                             // fx_map_observe: the landmarks' list counts, cursors and prefix, each row's target and distance, the lists;
                             // fx_map_expect: the grid, this call's counts of both kinds, each row's named landmark;
                             // fx_map_discover: the grid, a second grid over the free rows, their staged points and sources, each
                             // one's leader, distance and verdicts, the leaders' supports and prefix;
                             // fx_map_compact: the marks, the new ids, the blocks' counts, the kept records and sums staged;
                             // fx_map_retire: the same, and the kept landmarks' counters staged;
                             // fx_map_append: the state words; fx_map_append_host: the snapshot's bytes before them;
                             // fx_map_join_segments, fx_map_close_loop: the grid, each query's target and distance, the list of
                             // correspondences
  DevScratch splice_scratch; // fx_splice_blocks: the plan words
  // fx_map_import_host, fx_map_append_host: the snapshot's bytes, pinned, until the copies enqueued from them are done (snap_ev)
  uint8_t *snap_h = nullptr;
  size_t snap_bytes = 0;
  hipEvent_t snap_ev = nullptr;
};

// A persistent landmark map (include/fx.h fx_map_create): one device buffer, carved up once.
struct fx_map {
  fx_ctx *ctx = nullptr;
  int device = 0;
  uint8_t *d = nullptr;
  FxMapArgs a{};  // the map's own pointers and capacities; the rest is filled in per call
};

namespace {

template <typename T>
fx_status dev_alloc(fx_ctx *c, T **p, size_t count) {
  void *q = nullptr;
  const size_t bytes = (count ? count : 1) * sizeof(T);
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return fail(FX_ERR_OOM, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
  c->dev_allocs.push_back(q);
  *p = (T *)q;
  return FX_OK;
}
template <typename T>
fx_status host_alloc(fx_ctx *c, T **p, size_t count) {
  if (*p) return FX_OK;
  void *q = nullptr;
  const size_t bytes = (count ? count : 1) * sizeof(T);
  hipError_t e = hipHostMalloc(&q, bytes, hipHostMallocDefault);
  if (e != hipSuccess) return fail(FX_ERR_OOM, std::string("hipHostMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
  c->host_allocs.push_back(q);
  *p = (T *)q;
  return FX_OK;
}
#define FX_TRY(expr)              \
  do {                            \
    fx_status s_ = (expr);        \
    if (s_ != FX_OK) return s_;   \
  } while (0)

fx_status DevScratch::reserve(fx_ctx *c, size_t need, const char *what) {
  if (d && need <= bytes) return FX_OK;
  if (d) {
    FX_HIP(hipStreamSynchronize(c->stream));
    FX_HIP(hipFree(d));
    d = nullptr;
  }
  const size_t n = std::max({need, 2 * bytes, (size_t)4096});
  bytes = 0;
  void *q = nullptr;
  hipError_t e = hipMalloc(&q, n);
  if (e != hipSuccess) return fail(FX_ERR_OOM, std::string(what) + " hipMalloc(" + std::to_string(n) + "): " + hipGetErrorString(e));
  d = (uint8_t *)q, bytes = n;
  return FX_OK;
}
void DevScratch::release() {
  if (d) (void)hipFree(d);
}
fx_status Staging::reserve(fx_ctx *c, size_t need, const char *what) {
  if (!ev) FX_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  if (need > bytes) {
    if (d) {
      FX_HIP(hipStreamSynchronize(c->stream));
      FX_HIP(hipFree(d));
      FX_HIP(hipHostFree(h));
      d = h = nullptr;
    }
    const size_t n = std::max({need, 2 * bytes, (size_t)4096});
    bytes = 0;
    void *qd = nullptr, *qh = nullptr;
    hipError_t e = hipMalloc(&qd, n);
    if (e == hipSuccess && (e = hipHostMalloc(&qh, n, hipHostMallocDefault)) != hipSuccess) (void)hipFree(qd);
    if (e != hipSuccess) return fail(FX_ERR_OOM, std::string(what) + " hipMalloc + hipHostMalloc(" + std::to_string(n) + "): " + hipGetErrorString(e));
    d = (uint8_t *)qd, h = (uint8_t *)qh, bytes = n;
  }
  FX_HIP(hipEventSynchronize(ev));  // (the last upload; done at once when none was recorded)
  return FX_OK;
}
fx_status Staging::upload(fx_ctx *c, size_t n) {
  if (!n) return FX_OK;
  FX_HIP(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, c->stream));
  FX_HIP(hipEventRecord(ev, c->stream));
  return FX_OK;
}
void Staging::release() {
  if (d) (void)hipFree(d);
  if (h) (void)hipHostFree(h);
  if (ev) (void)hipEventDestroy(ev);
}

// The query ranges of the pairs must be disjoint: the match writes one record, the register one inlier word a query row
fx_status query_ranges_disjoint(const fx_match_pair *pairs, uint32_t n_pairs) {
  std::vector<std::pair<uint64_t, uint64_t>> r;
  for (uint32_t p = 0; p < n_pairs; ++p)
    if (pairs[p].q_rows) r.emplace_back((uint64_t)pairs[p].q_row0, (uint64_t)pairs[p].q_row0 + pairs[p].q_rows);
  std::sort(r.begin(), r.end());
  for (size_t i = 1; i < r.size(); ++i)
    if (r[i].first < r[i - 1].second)
      return fail(FX_ERR_INVALID_ARG, "query ranges of the pairs overlap at row " + std::to_string(r[i].first));
  return FX_OK;
}

// The CSR block's offsets and entry counts are u32: every row of the descriptor pool stored whole must fit
bool csr_pool_fits(const fx_limits &L) { return (uint64_t)L.max_total_keypoints * FX_DESC_FLOATS <= 0xffffffffull; }
size_t csr_col_offset(uint32_t max_rows) { return 16u + 4u * csr_rp_words(max_rows); }
size_t csr_val_offset(uint32_t max_rows, uint32_t cap) { return csr_col_offset(max_rows) + 4u * csr_cap_words(cap); }
// k_csr_count / k_csr_write: grid-stride, a wavefront a row, up to eight workgroups a CU
fx_status enqueue_csr(fx_ctx *c, hipStream_t s, void *dst, uint32_t max_rows, uint32_t cap) {
  const uint32_t rows_bound = std::min(c->lim.max_total_keypoints, 0xffffffffu - 3u);
  const uint32_t grid = std::max(1u, std::min((rows_bound + 3u) / 4u, 8u * c->plan_cfg.n_cu));
  FX_HIP(fxk_pack_csr(s, c->dp, c->buf, c->plan_state.last_batch, dst, max_rows, cap, grid, c->csr_full_rows));
  return FX_OK;
}
// The context's block with room for `cap` entries (max_total_keypoints rows).  An existing block is freed once the stream
// is done with it: a reallocation happens at the first CSR batch, after fx_set_descriptor_csr_capacity, and when a batch
// needs more entries than the block has.
fx_status csr_reserve(fx_ctx *c, uint32_t cap) {
  if (c->d_csr && c->csr_cap == cap) return FX_OK;
  if (c->d_csr) {
    FX_HIP(hipStreamSynchronize(c->stream));
    FX_HIP(hipFree(c->d_csr));
    FX_HIP(hipHostFree(c->h_csr));
    c->d_csr = c->h_csr = nullptr;
    c->csr_cap = 0;
  }
  const size_t bytes = fxk_csr_bytes(c->lim.max_total_keypoints, cap);
  void *q = nullptr;
  hipError_t e = hipMalloc(&q, bytes);
  if (e != hipSuccess) return fail(FX_ERR_OOM, std::string("CSR block hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
  c->d_csr = (uint8_t *)q;
  q = nullptr;
  e = hipHostMalloc(&q, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipFree(c->d_csr);
    c->d_csr = nullptr;
    return fail(FX_ERR_OOM, std::string("CSR block hipHostMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
  }
  c->h_csr = (uint8_t *)q;
  c->csr_cap = cap;
  return FX_OK;
}

}  // namespace

namespace {
// k_prep's arctangent (elevation_fast): atan(c + d) = sum_k a_k d^k about c = i / FX_ATAN_N, a_0 = atan(c),
// a_k = (-1)^(k-1) sin^k(th) sin(k th) / k with th = pi/2 - atan(c) (the k-th derivative of the arctangent in closed form);
// evaluated in long double: the entries are good to the last bit or two of double.
std::vector<double> atan_table() {
  std::vector<double> at((FX_ATAN_N + 1) * (FX_ATAN_DEG + 1));
  for (int i = 0; i <= FX_ATAN_N; ++i) {
    const long double cpt = (long double)i / FX_ATAN_N, a0 = atanl(cpt), th = atan2l(1.0L, cpt), st = sinl(th);
    long double pw = 1.0L;
    at[(size_t)i * (FX_ATAN_DEG + 1)] = (double)a0;
    for (int kk = 1; kk <= FX_ATAN_DEG; ++kk) {
      pw *= st;
      at[(size_t)i * (FX_ATAN_DEG + 1) + kk] = (double)(((kk & 1) ? 1.0L : -1.0L) * pw * sinl(kk * th) / kk);
    }
  }
  return at;
}

// Enqueues the stage kernels of one batch on stream s (the whole device-side pipeline between the
// scan-table upload and the result copies), as `plan` says (csrc/fx_launch_plan.h decides; nothing is decided here).  Also
// what a HIP graph of the batch is captured from.
fx_status enqueue_stages(fx_ctx *c, hipStream_t s, uint32_t batch, bool prof, const FxLaunchPlan &plan) {
  const fx_limits &L = c->lim;
  const FxDevParams &P = c->dp;
  const FxBuffers &B = c->buf;
  if (prof) {
    c->ev = &c->ev_ring[(size_t)(c->ev_count % c->ev_depth) * (FX_N_STAGES + 1)];
    c->ev_mask[c->ev_count % c->ev_depth] = c->prof_mask;
    c->ev_seq[c->ev_count % c->ev_depth] = c->batch_seq;
  }
  const uint32_t pmask = c->prof_mask;
  auto mark = [&](int i) -> hipError_t {
    if (c->debug_sync) {  // FX_DEBUG_SYNC=1: name the stage a device fault belongs to
      fprintf(stderr, "[fx] stage %d enqueued\n", i);
      hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess) return e;
    }
    // event i closes stage i - 1 and opens stage i; the first and last always bracket the batch
    const bool wanted = i == 0 || i == FX_N_STAGES || ((pmask >> i) & 1u) || ((pmask >> (i - 1)) & 1u);
    return (prof && wanted) ? hipEventRecord(c->ev[i], s) : hipSuccess;
  };
  FX_HIP(mark(0));
  if (!batch) {
    FX_HIP(hipMemsetAsync(B.counters, 0, FX_N_COUNTERS * sizeof(uint32_t), s));  // (k_prep clears them otherwise)
    for (int i = 1; i <= FX_N_STAGES; ++i) FX_HIP(mark(i));
    return FX_OK;
  }
  const uint32_t clk_slot = (uint32_t)(c->batch_seq % FX_CLK_SLOTS), clk_next = (uint32_t)((c->batch_seq + 1) % FX_CLK_SLOTS);
  const float el0 = (float)c->params.el0_deg, inv_step = (float)(1.0 / c->params.el_step_deg);
  if (plan.front != FX_FRONT_SEPARATE) {
    // stages 0-4: the front in one of its launch sets, then k_front_redo for the scans that do not fit k_front's tables and
    // k_slow for what exceeds that shape's LDS too.  All go with EVERY batch: the plan sizes grids, it never decides whether
    // a scan gets what it needs.
    if (plan.front == FX_FRONT_STREAMED) {  // (stage 0: the streaming pass, stage 1: ring split + k_front_cd)
      fxk_prep_sliced(s, P, B, batch, plan.prep_slices, c->box_margin, el0, inv_step, clk_slot);
      FX_HIP(mark(1));
      fxk_bucket_sliced(s, P, B, batch, plan.prep_slices, el0, inv_step, clk_next);
      fxk_front_cd(s, P, B, batch, clk_slot, plan.front_merge_cap, 0u, 1u, plan.force_redo);
    } else if (plan.front == FX_FRONT_FUSED) {
      fxk_front(s, P, B, batch, c->box_margin, el0, inv_step, clk_slot, plan.front_merge_cap, plan.force_redo);
      FX_HIP(mark(1));
    } else {  // (stage 0: k_front_ab, stage 1: k_front_cd)
      fxk_front_ab(s, P, B, batch, c->box_margin, el0, inv_step, clk_slot, plan.force_redo);
      FX_HIP(mark(1));
      fxk_front_cd(s, P, B, batch, clk_slot, plan.front_merge_cap, plan.front == FX_FRONT_TWO_LEAN ? 1u : 0u, 0u, 0u);
    }
    for (int i = 2; i <= 4; ++i) FX_HIP(mark(i));
    if (plan.redo_grid) fxk_front_redo(s, P, B, el0, inv_step, c->merge_huge_ccap, plan.force_slow, plan.redo_grid);
    fxk_slow(s, P, B, c->merge_huge_ccap, plan.slow_grid, batch, clk_next);  // (its last workgroup does the batch's keypoint offsets too)
    FX_HIP(mark(5));
  } else {
    if (plan.prep_slices > 1) {
      fxk_prep_sliced(s, P, B, batch, plan.prep_slices, c->box_margin, el0, inv_step, clk_slot);
      FX_HIP(mark(1));
      fxk_bucket_sliced(s, P, B, batch, plan.prep_slices, el0, inv_step, clk_next);
    } else {
      fxk_prep(s, P, B, batch, c->box_margin, el0, inv_step, clk_slot);
      FX_HIP(mark(1));
      fxk_bucket(s, P, B, batch, el0, inv_step, clk_next, plan.many_rings ? 1u : 0u);
    }
    FX_HIP(mark(2));
    fxk_rings_runs(s, P, B, batch, L.max_ring_points, plan.runs_grid);
    FX_HIP(mark(3));
    if (plan.runs2_grid) fxk_rings_runs2(s, P, B, L.max_ring_points, plan.runs2_grid);
    fxk_rings_large(s, P, B, c->ring_lds_cap, c->ring_lds_cap, plan.large_grid, plan.runs2_grid ? 1u : 0u);
    FX_HIP(mark(4));
    fxk_merge_small(s, P, B, batch, plan.merge_small_cap);
    fxk_merge_big(s, P, B, c->plan_cfg.merge_big_cap, plan.merge_big_grid, plan.merge_big_last);
    if (plan.merge_huge_grid) {
      if (plan.merge_huge_slices > 1)
        fxk_merge_huge_split(s, P, B, c->merge_huge_cap, c->merge_huge_ccap, plan.merge_huge_grid, plan.merge_huge_slices);
      else
        fxk_merge_huge(s, P, B, c->merge_huge_cap, c->merge_huge_ccap, plan.merge_huge_grid);
    }
    fxk_slow(s, P, B, c->merge_huge_ccap, plan.slow_grid, batch, clk_next);  // (rings / merges beyond the LDS tiers, and the batch's keypoint offsets: see the front path)
    FX_HIP(mark(5));
  }
  if (plan.descriptors) {
    fxk_gather(s, P, B, batch, c->box_margin, plan.gather, plan.gather_n);
    if (plan.rng_ord) fxk_rng_ord(s, P, B, batch);
    FX_HIP(mark(6));
    // every descriptor tier in ONE launch, timed in the group tier's slot (the next slot brackets nothing) — the gather has
    // classified every row, so no tier waits for another (k_desc)
    fxk_desc(s, P, B, batch, plan.desc_cap, plan.desc_wg, plan.desc_wave, plan.desc_group, plan.desc_dslow);
    FX_HIP(mark(7));
    FX_HIP(mark(8));
    if (plan.dense) fxk_dense(s, P, B, plan.dense_sort_grid, plan.dense_density_grid, plan.dense_finish_grid, plan.dense_skip);
  } else {
    for (int i = 6; i <= 8; ++i) FX_HIP(mark(i));
  }
  FX_HIP(mark(9));
  FX_HIP(hipGetLastError());
  return FX_OK;
}

// Small batches are launch-bound (about 30 launches for a few hundred microseconds of work): replay the
// sequence as one HIP graph per batch size.  Kernel arguments depend on the batch size only; the scan
// table lives in the fixed d_meta buffer and is uploaded before the graph runs.
fx_status launch_graph(fx_ctx *c, hipStream_t s, uint32_t batch, bool front) {
  hipGraphExec_t exec = nullptr;
  const uint32_t key = batch | (front ? 0x80000000u : 0u);
  for (auto &g : c->graphs)
    if (g.first == key) exec = g.second;
  if (!exec) {
    hipGraph_t graph = nullptr;
    FX_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    // (a graph's grids are fixed: the full ones, bounded by the batch; its front is what this batch was given)
    FxPlanConfig cfg = c->plan_cfg;
    cfg.front_ok = front;
    const uint32_t no_hints[FX_N_HINTS] = {};  // (not read under capture, and the state is not touched)
    const FxLaunchPlan plan = fx_plan_batch(cfg, &c->plan_state, no_hints, batch, true);
    fx_status st = enqueue_stages(c, s, batch, false, plan);
    hipError_t e = hipStreamEndCapture(s, &graph);
    if (st != FX_OK) {
      if (graph) (void)hipGraphDestroy(graph);
      return st;
    }
    FX_HIP(e);
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    FX_HIP(e);
    if (c->graphs.size() >= 8) {  // bounded cache: drop the oldest batch size
      (void)hipGraphExecDestroy(c->graphs.front().second);
      c->graphs.erase(c->graphs.begin());
    }
    c->graphs.emplace_back(key, exec);
  }
  FX_HIP(hipGraphLaunch(exec, s));
  return FX_OK;
}

// What the calls on a map share (fx_map_reset ... fx_map_import_host).
// the prologue: the handles, and whatever else the call cannot do without, are there, and the map is this
// context's
fx_status map_call_check(const fx_ctx *c, const fx_map *m, bool others_given = true) {
  if (!c || !m || !others_given) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (m->ctx != c) return fail(FX_ERR_INVALID_ARG, "the map belongs to another context");
  return FX_OK;
}
// What the map calls that run on the context's scratch share (fx_map_merge ... fx_map_find_loop).
// a grid over the map m with the gate `dist`: the map's own memory, the gate in fp64 and the grid's cell edge, dist (1 + 2^-8),
// exact (csrc/fx_map_grid.h proves the margin), and the table
void map_grid_view(FxMapMergeArgs *G, const fx_map *m, double dist) {
  G->header = m->a.header, G->records = m->a.records, G->acc = m->a.acc, G->carry = m->a.carry, G->alias = m->a.alias;
  G->cap = m->a.cap, G->max_carry = m->a.max_carry;
  G->md2 = dist * dist, G->inv_edge = 1.0 / (dist * (1.0 + 1.0 / 256.0));
  G->table = fxk_map_merge_table(G->cap);
}
// the options of the consensus over a nearest search: fx_map_localize, fx_map_join_segments, fx_map_close_loop
template <typename Options>
fx_status consensus_options_check(const Options &o) {
  if (!(std::isfinite(o.search_dist) && o.search_dist > 0.f)) return fail(FX_ERR_INVALID_ARG, "search_dist must be finite and positive");
  if (!(o.inlier_dist > 0.f) || !std::isfinite(o.inlier_dist) || !(o.min_baseline > 0.f) || !std::isfinite(o.min_baseline))
    return fail(FX_ERR_INVALID_ARG, "inlier_dist and min_baseline must be finite and positive");
  if (o.hyp_corr < 2u || o.hyp_corr > 128u) return fail(FX_ERR_INVALID_ARG, "hyp_corr must be 2..128");
  if (o.min_inliers < 2u) return fail(FX_ERR_INVALID_ARG, "min_inliers must be at least 2");
  if (!o.min_landmark_obs) return fail(FX_ERR_INVALID_ARG, "min_landmark_obs must be at least 1");
  return FX_OK;
}
// the options of the constellation search: fx_map_relocalize, fx_map_find_loop
template <typename Options>
fx_status constellation_options_check(const Options &o) {
  auto positive = [](float v) { return std::isfinite(v) && v > 0.f; };
  if (!positive(o.inlier_dist)) return fail(FX_ERR_INVALID_ARG, "inlier_dist must be finite and positive");
  if (!positive(o.pair_tol)) return fail(FX_ERR_INVALID_ARG, "pair_tol must be finite and positive");
  if (!positive(o.min_baseline)) return fail(FX_ERR_INVALID_ARG, "min_baseline must be finite and positive");
  if (!(std::isfinite(o.max_baseline) && o.max_baseline >= o.min_baseline))
    return fail(FX_ERR_INVALID_ARG, "max_baseline must be finite and at least min_baseline");
  if (o.max_seeds < 1u || o.max_seeds > FX_RELOC_MAX_KP) return fail(FX_ERR_INVALID_ARG, "max_seeds must be 1..64");
  if (o.min_inliers < 3u) return fail(FX_ERR_INVALID_ARG, "min_inliers must be at least 3");
  if (!o.min_margin) return fail(FX_ERR_INVALID_ARG, "min_margin must be at least 1");
  if (!o.min_landmark_obs) return fail(FX_ERR_INVALID_ARG, "min_landmark_obs must be at least 1");
  return FX_OK;
}
static_assert(FX_FIND_MAX_QUERY == FX_RELOC_MAX_KP, "max_seeds' bound is one for both constellation searches");
// the two grids of a constellation search, P for the pairs and Q for the score, and what both calls take from the options: the
// gates in fp64 (csrc/fx_map_constellation.h derives the pair grid's gate (xb + pt)(1 + 2^-20) from the hypothesis's length gate)
template <typename Args, typename Options>
void constellation_args(Args *A, const fx_map *m, const Options &o) {
  map_grid_view(&A->P, m, ((double)o.max_baseline + (double)o.pair_tol) * (1.0 + 1.0 / 1048576.0));
  map_grid_view(&A->Q, m, (double)o.inlier_dist);
  A->inlier_dist = o.inlier_dist, A->pair_tol = o.pair_tol, A->min_baseline = o.min_baseline, A->max_baseline = o.max_baseline;
  A->max_seeds = o.max_seeds, A->min_inliers = o.min_inliers, A->min_margin = o.min_margin, A->min_landmark_obs = o.min_landmark_obs;
  A->chunks = (A->P.cap + FXR_CHUNK - 1u) / FXR_CHUNK;
}
// the prior of the join and the loop: on the host or on the device, not both, and finite where the host can see it
fx_status prior_check(const fx_pose *prior_host, const double *prior_device) {
  if (prior_host && prior_device) return fail(FX_ERR_INVALID_ARG, "give the prior on the host or on the device, not both");
  if (prior_host && !finite_pose(*prior_host)) return fail(FX_ERR_INVALID_ARG, "prior_host must be finite");
  return FX_OK;
}
// What the calls that read a keypoint block as a query share (fx_track_landmarks, fx_map_localize ... fx_map_expect; fx_device.h
// FxKpQuery): the refusal of the caller's scans, and the query in the launch arguments
fx_status query_check(uint32_t max_scans, uint32_t n_scans) {
  if (!n_scans || n_scans > max_scans)
    return fail(FX_ERR_INVALID_ARG, "n_scans must be 1..max_scans (" + std::to_string(n_scans) + " of " + std::to_string(max_scans) + ")");
  return FX_OK;
}
void query_args(FxKpQuery *K, const void *kp, uint32_t max_scans, uint32_t max_total, uint32_t n_scans, uint32_t q_max_rows) {
  K->kp = (const uint32_t *)kp, K->max_scans = max_scans, K->max_total = max_total, K->n_scans = n_scans, K->q_max_rows = q_max_rows;
}
// require_flags of the calls that read localisations (fx_map_observe, fx_map_expect)
fx_status loc_flags_check(uint32_t require_flags) {
  const uint32_t known = FX_LOC_VALID | FX_LOC_TRUNCATED | FX_LOC_NO_HYPOTHESIS | FX_LOC_BAD_PRIOR | FX_LOC_NO_SCAN;
  if (require_flags & ~known) return fail(FX_ERR_INVALID_ARG, "unknown require_flags bits (only the FX_LOC_* flags are defined)");
  return FX_OK;
}
// the map's own memory in the arguments of fx_map_compact and fx_map_retire
void map_compact_view(FxMapCompactArgs *A, const fx_map *m) {
  A->header = m->a.header, A->records = m->a.records, A->acc = m->a.acc, A->carry = m->a.carry, A->alias = m->a.alias;
  A->cap = m->a.cap, A->max_carry = m->a.max_carry;
}
// the association's part of the join's and the loop's arguments (fx_device.h FxMapAssocArgs); no prior is the identity
template <typename Options>
void assoc_args(FxMapAssocArgs *S, const fx_map *m, const Options &o, const fx_pose *prior_host, const double *prior_device, int32_t *match) {
  map_grid_view(&S->G, m, (double)o.search_dist);
  S->mode = o.mode;
  S->prior[0] = 1.0;
  if (prior_host)
    S->prior[0] = prior_host->c, S->prior[1] = prior_host->s, S->prior[2] = prior_host->tx, S->prior[3] = prior_host->ty, S->prior[4] = prior_host->tz;
  S->prior_device = prior_device;
  S->inlier_dist = o.inlier_dist, S->min_baseline = o.min_baseline;
  S->hyp_corr = o.hyp_corr, S->min_inliers = o.min_inliers, S->min_landmark_obs = o.min_landmark_obs;
  S->match = match;
}
// the tail of a call: room in the context's scratch for what `launch` needs of it, A's pointers carved out of it, the launches
#define FX_MAP_RUN(launch, what)                                                      \
  do {                                                                                \
    FX_TRY(c->merge_scratch.reserve(c, launch##_scratch(&A, nullptr), what));         \
    (void)launch##_scratch(&A, c->merge_scratch.d);                                   \
    FX_HIP(launch(c->stream, A));                                                     \
  } while (0)
}  // namespace

extern "C" {

const char *fx_last_error(void) { return g_last_error.c_str(); }

fx_status fx_check_abi(uint32_t header_version, size_t sizeof_params, size_t sizeof_limits, size_t sizeof_scan_desc, size_t sizeof_batch_view) {
  const uint32_t lib_version = ((uint32_t)FX_VERSION_MAJOR << 16) | FX_VERSION_MINOR;
  if (header_version == lib_version && sizeof_params == sizeof(fx_params) && sizeof_limits == sizeof(fx_limits) &&
      sizeof_scan_desc == sizeof(fx_scan_desc) && sizeof_batch_view == sizeof(fx_batch_view))
    return FX_OK;
  char msg[256];
  snprintf(msg, sizeof msg, "caller compiled against fx.h %u.%u (fx_params %zu, fx_limits %zu, fx_scan_desc %zu, fx_batch_view %zu bytes); "
           "this library is %u.%u (%zu, %zu, %zu, %zu)", header_version >> 16, header_version & 0xffffu, sizeof_params, sizeof_limits,
           sizeof_scan_desc, sizeof_batch_view, lib_version >> 16, lib_version & 0xffffu, sizeof(fx_params), sizeof(fx_limits),
           sizeof(fx_scan_desc), sizeof(fx_batch_view));
  return fail(FX_ERR_INVALID_ARG, msg);
}

fx_status fx_create(const fx_params *params, const fx_limits *limits, int device_id, fx_ctx **out) {
  if (!params || !limits || !out) return fail(FX_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  int n_dev = 0;
  hipError_t e = hipGetDeviceCount(&n_dev);
  if (e != hipSuccess || n_dev <= 0)
    return fail(FX_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + (e != hipSuccess ? hipGetErrorString(e) : "0 devices"));
  if (device_id < 0 || device_id >= n_dev) return fail(FX_ERR_INVALID_ARG, "device_id out of range");

  fx_limits L = *limits;
  fx_limits D;
  fx_limits_default(&D, L.max_batch, L.max_points);
  if (!L.max_ring_points) L.max_ring_points = D.max_ring_points;
  if (!L.max_ring_candidates) L.max_ring_candidates = D.max_ring_candidates;
  if (!L.max_candidates) L.max_candidates = D.max_candidates;
  if (!L.max_keypoints) L.max_keypoints = D.max_keypoints;
  if (!L.max_neighbors) L.max_neighbors = D.max_neighbors;
  if (!L.max_total_keypoints) L.max_total_keypoints = D.max_total_keypoints;
  if (!L.max_kpc_points) L.max_kpc_points = D.max_kpc_points;
  if (!L.max_dense_points) L.max_dense_points = D.max_dense_points;
  if (!L.max_overflow_points) L.max_overflow_points = D.max_overflow_points;
  if (L.max_batch == 0 || L.max_points == 0) return fail(FX_ERR_INVALID_ARG, "max_batch and max_points must be > 0");
  if (L.max_batch > 65535) return fail(FX_ERR_INVALID_ARG, "max_batch > 65535 (one grid row per scan in the support gather)");
  if (L.max_points > (1u << 20)) return fail(FX_ERR_INVALID_ARG, "max_points > 2^20 (descriptor sort key packs the point index in 20 bits)");
  if (params->n_rings < 1 || params->n_rings > 1024) return fail(FX_ERR_INVALID_ARG, "n_rings must be in [1, 1024]");
  if (!(params->descriptor_radius > 0.0) || !(params->el_step_deg > 0.0))
    return fail(FX_ERR_INVALID_ARG, "descriptor_radius and el_step_deg must be > 0");
  if (params->descriptor_radius < 1e-12 || params->descriptor_radius > 1e12)  // (the squared radii stay normal floats with room to scale)
    return fail(FX_ERR_INVALID_ARG, "descriptor_radius out of range");
  if (L.max_ring_candidates > L.max_ring_points) L.max_ring_candidates = L.max_ring_points;
  // LDS budget of the large tiers (160 KiB per workgroup on gfx950); what the limits allow beyond it takes the slow tier
  // (k_slow: the same bodies on scratch in HBM)
  const size_t kLds = 160 * 1024;
  if (L.max_ring_points > 32768 || L.max_candidates > 32768 || L.max_keypoints > 65535)
    return fail(FX_ERR_INVALID_ARG, "limit exceeds the 16-bit packing of the order replay (max_ring_points, max_candidates <= 32768)");
  uint32_t ring_lds_cap = L.max_ring_points;
  while (fxk_ring_large_lds_bytes(ring_lds_cap, ring_lds_cap) > kLds) ring_lds_cap -= ring_lds_cap > 64 ? 16 : 1;
  // merge tiers: up to merge_big_cap candidates a scan live in LDS as points; beyond that (dense many-ring scans)
  // the large tier keeps only parents and a cell sort in LDS
  uint32_t merge_big_cap = L.max_candidates;
  while (fxk_merge_lds_bytes(merge_big_cap, params->n_rings) > kLds) merge_big_cap -= merge_big_cap > 64 ? 64 : 1;
  if (const char *e = test_hook("FX_MERGE_BIG_CAP")) {  // test hook: push scans on to the large merge tier
    const uint32_t v = (uint32_t)atoi(e);
    if (v >= 16 && v < merge_big_cap) merge_big_cap = v;
  }
  const uint32_t merge_huge_ccap = L.max_keypoints > 64 ? L.max_keypoints : 64;
  uint32_t merge_huge_cap = L.max_candidates;
  while (merge_huge_cap > merge_big_cap && fxk_merge_huge_lds_bytes(merge_huge_cap, merge_huge_ccap, params->n_rings) > kLds) merge_huge_cap -= 64;
  if (merge_huge_cap < merge_big_cap) merge_huge_cap = merge_big_cap;
  if (const char *e = test_hook("FX_MERGE_HUGE_CAP")) {  // test hook: push scans on from the large merge tier to the slow one
    const uint32_t v = (uint32_t)atoi(e);
    if (v >= merge_big_cap && v < merge_huge_cap) merge_huge_cap = v;
  }
  if (const char *e = test_hook("FX_RING_LDS_CAP")) {  // test hook: push rings on from the workgroup ring tier to the slow one
    const uint32_t v = (uint32_t)atoi(e);
    if (v >= 16 && v < ring_lds_cap) ring_lds_cap = v & ~3u;
  }
  if (fxk_gather_lds_bytes(L.max_keypoints) > kLds) return fail(FX_ERR_INVALID_ARG, "support gather: LDS tables beyond the budget (build parameter FX_GATHER_KCAP)");

  FX_HIP(hipSetDevice(device_id));
  fx_ctx *c = new fx_ctx();
  c->params = *params;
  c->lim = L;
  c->device = device_id;
  c->ring_lds_cap = ring_lds_cap;
  FxPlanConfig &pc = c->plan_cfg;
  pc.merge_big_cap = merge_big_cap;
  c->merge_huge_cap = merge_huge_cap;
  c->merge_huge_ccap = merge_huge_ccap;
  if (const char *e = test_hook("FX_DESC_WGS_PER_CU")) {  // experiment hook: ignored outside 1..32
    const int v = atoi(e);
    if (v >= 1 && v <= 32) pc.desc_wgs_per_cu = (uint32_t)v;
  }
  if (const char *e = test_hook("FX_DESC_GRID")) pc.desc_grid_abs = (uint32_t)std::max(0, atoi(e));
  if (const char *e = test_hook("FX_DEBUG_SYNC")) c->debug_sync = atoi(e) != 0;
  if (const char *e = test_hook("FX_GRAPH_MAX_BATCH")) {
    const int v = atoi(e);
    if (v >= 0) c->graph_max_batch = (uint32_t)v;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) pc.n_cu = (uint32_t)prop.multiProcessorCount;

  // ---- constants, narrowed where PCL narrows them
  FxDevParams &P = c->dp;
  std::memset(&P, 0, sizeof(P));
  P.x_min = (float)params->x_min;  // PassThrough::setFilterLimits(const float&, const float&)
  P.x_max = (float)params->x_max;
  P.y_min = (float)params->y_min;
  P.y_max = (float)params->y_max;
  P.z_min = (float)params->z_min;
  P.z_max = (float)params->z_max;
  P.n_rings = params->n_rings;
  {
    // EuclideanClusterExtraction narrows the tolerance to float; KdTreeFLANN squares it in double
    const double tol = (double)(float)params->cluster_tolerance;
    P.r2_cluster = (float)(tol * tol);
    const double crt = (double)(float)params->cluster_radius_threshold;
    P.r2_merge = (float)(crt * crt);
  }
  P.min_count = (uint32_t)params->cluster_min_count;
  P.max_count = (uint32_t)params->cluster_max_count;
  P.gate_diameter = 2 * params->cluster_radius_threshold;
  P.crt = params->cluster_radius_threshold;
  P.ndc = (uint32_t)params->number_detection_channels;
  P.secondary_max = (uint32_t)params->secondary_max;
  {
    const double R = params->descriptor_radius, rd = params->descriptor_radius / 5.0;
    P.r2_search = (float)(R * R);  // 3DSC hands its radii to the tree as doubles
    P.r2_density = (float)(rd * rd);
    const double rs = (R + rd) * 1.0001 + 1e-4;  // conservative superset radius of the support set
    P.r2_support = (float)(rs * rs);
    c->box_margin = (float)(rs * 1.001 + 1e-3);  // k_gather's bounding-box reject, conservative
  }
  P.estimate_descriptors = params->estimate_descriptors;
  P.max_points = L.max_points;
  P.max_ring_cands = L.max_ring_candidates;
  P.max_candidates = L.max_candidates;
  P.max_keypoints = L.max_keypoints;
  P.max_total_kp = L.max_total_keypoints;
  P.max_kpc = L.max_kpc_points;
  P.max_neighbors = L.max_neighbors;
  P.max_ring_points = L.max_ring_points;
  P.list_cap = L.max_neighbors < kListCap ? L.max_neighbors : kListCap;
  P.near_words = fxk_near_words(L.max_points);
  // dense tier pools (fx_limits.max_dense_points; default: as many entries as the batch has points, at least 32 scans' worth)
  P.dense_min = kDenseMin;
  P.ovf_cap = L.max_overflow_points > 0x7ff00000u ? 0x7ff00000u : L.max_overflow_points;  // a scan's overflow region (fx_limits.max_overflow_points)
  {
    const unsigned long long want = L.max_dense_points ? L.max_dense_points : (unsigned long long)(L.max_batch > 32u ? L.max_batch : 32u) * L.max_points;
    P.dense_cap = (uint32_t)(want > 0xfff00000ull ? 0xfff00000ull : (want < 4096ull ? 4096ull : want));  // (a row takes its support points + 700 entries of it)
    const uint32_t per_row = P.list_cap < P.dense_min ? P.list_cap : P.dense_min;  // a dense row has more support points than this
    const unsigned long long rows = (unsigned long long)P.dense_cap / (per_row ? per_row : 1u) + 1ull;
    P.max_dense_rows = (uint32_t)(rows < L.max_total_keypoints ? rows : L.max_total_keypoints);
  }
  P.dense_qcap = P.dense_cap > 0x7ff00000u ? 0xfff00000u : 2u * P.dense_cap;  // (cells' queries padded to four: typically 1.2 entries per query)
  P.dense_lds_keys = fxk_dfin_k();
  if (const char *e = test_hook("FX_DENSE_LDS_KEYS")) {  // test hook: push rows on to the global-memory key sort (can only lower the cap)
    const int v = atoi(e);
    if (v >= 1 && (uint32_t)v < P.dense_lds_keys) P.dense_lds_keys = (uint32_t)v;
  }
  P.dense_won_points = 0xffffffffu;  // (the kernel's own bit map bounds it)
  if (const char *e = test_hook("FX_DENSE_WON_POINTS")) {  // test hook: rows of more points mark their queries in the sorted region itself
    const int v = atoi(e);
    if (v >= 0) P.dense_won_points = (uint32_t)v;
  }
  P.ring_slot_cap = 2 * L.max_points;  // worst case: every point on a window boundary, i.e. in two rings
  P.ring_list_cap = ((L.max_batch + 7) / 8) * (uint32_t)params->n_rings;  // rings of the scans of one XCD class

  fx_status st = FX_OK;
  auto bail = [&](fx_status s) {
    fx_destroy(c);
    return s;
  };
#define FX_A(expr)                     \
  st = (expr);                         \
  if (st != FX_OK) return bail(st)

  const size_t B = L.max_batch, R = (size_t)params->n_rings;
  FxBuffers &b = c->buf;
  std::memset(&b, 0, sizeof(b));
  FX_A(dev_alloc(c, &c->d_meta, B));
  b.meta = c->d_meta;
  float2 *d_win = nullptr;
  FX_A(dev_alloc(c, &d_win, R));
  b.ring_win = d_win;
  double *d_atan = nullptr;
  FX_A(dev_alloc(c, &d_atan, (size_t)(FX_ATAN_N + 1) * (FX_ATAN_DEG + 1)));
  b.atan_tab = d_atan;
  FxScTables *d_tab = nullptr;
  FX_A(dev_alloc(c, &d_tab, 1));
  b.tables = d_tab;
  float2 *d_xa = nullptr;
  FX_A(dev_alloc(c, &d_xa, L.max_keypoints));
  b.xaxis = d_xa;
  FX_A(dev_alloc(c, &b.filt, B * L.max_points));
  {
    // the five words a scan the host reads back after every batch — counts, the keypoint offsets, flags — in ONE block, so
    // that FX_OUT_HOST is one copy instead of five
    c->hdr_stride = (B + 1 + 3) & ~(size_t)3;
    uint32_t *hdr = nullptr;
    FX_A(dev_alloc(c, &hdr, 5 * c->hdr_stride));
    if (hipMemset(hdr, 0, 5 * c->hdr_stride * sizeof(uint32_t)) != hipSuccess) return bail(fail(FX_ERR_HIP, "hipMemset"));
    b.n_kp = hdr, b.kp_offset = hdr + c->hdr_stride, b.flags = hdr + 2 * c->hdr_stride, b.n_filt = hdr + 3 * c->hdr_stride,
    b.n_kpc = hdr + 4 * c->hdr_stride;
  }
  FX_A(dev_alloc(c, &b.near_bits, B * P.near_words));
  FX_A(dev_alloc(c, &b.prep_cnt, B * fxk_prep_slices_max()));
  FX_A(dev_alloc(c, &b.prep_ring_cnt, B * fxk_prep_slices_max() * R));
  FX_A(dev_alloc(c, &b.ring_cand, B * R * L.max_ring_candidates));
  FX_A(dev_alloc(c, &b.ring_cand_size, B * R * L.max_ring_candidates));
  FX_A(dev_alloc(c, &b.ring_cand_cnt, B * R));
  FX_A(dev_alloc(c, &b.ring_pts, B * P.ring_slot_cap));
  FX_A(dev_alloc(c, &b.ring_off, B * R));
  FX_A(dev_alloc(c, &b.ring_cnt, B * R));
  FX_A(dev_alloc(c, &b.kpc_pool, B * P.ring_slot_cap));
  FX_A(dev_alloc(c, &b.kpc_pool_cand, B * P.ring_slot_cap));
  FX_A(dev_alloc(c, &b.kpc_ring_cnt, B * R));
  FX_A(dev_alloc(c, &b.cand, B * L.max_candidates));
  FX_A(dev_alloc(c, &b.cand_size, B * L.max_candidates));
  FX_A(dev_alloc(c, &b.cand_kp, B * L.max_candidates));
  FX_A(dev_alloc(c, &b.n_cand, B));
  FX_A(dev_alloc(c, &b.keypoints, B * L.max_keypoints));
  FX_A(dev_alloc(c, &b.kp_size, B * L.max_keypoints));
  FX_A(dev_alloc(c, &b.kp_nbrs, B * L.max_keypoints));
  FX_A(dev_alloc(c, &b.kpc, B * L.max_kpc_points));
  FX_A(dev_alloc(c, &b.kpc_cand, B * L.max_kpc_points));
  FX_A(dev_alloc(c, &b.desc, (size_t)L.max_total_keypoints * FX_DESC_FLOATS + 4));
  FX_A(dev_alloc(c, &b.desc_nbins, (size_t)L.max_total_keypoints));
  FX_A(dev_alloc(c, &b.desc_bins, (size_t)L.max_total_keypoints * fxk_group_cap()));
  FX_A(dev_alloc(c, &b.row_class, (size_t)L.max_total_keypoints));  // (written for every row of a batch before it is read)
  // rows start out zero with nothing recorded in them: a row's owner then clears it by un-writing what was recorded last time
  if (hipMemset(b.desc, 0, ((size_t)L.max_total_keypoints * FX_DESC_FLOATS + 4) * sizeof(float)) != hipSuccess ||
      hipMemset(b.desc_nbins, 0, (size_t)L.max_total_keypoints * sizeof(uint32_t)) != hipSuccess)
    return bail(fail(FX_ERR_HIP, "hipMemset"));
  FX_A(dev_alloc(c, &b.huge_rings, (size_t)8 * P.ring_list_cap));
  FX_A(dev_alloc(c, &b.huge_rings2, (size_t)8 * P.ring_list_cap));
  FX_A(dev_alloc(c, &b.big_merge, B));
  FX_A(dev_alloc(c, &b.huge_merge, B));
  FX_A(dev_alloc(c, &b.redo, B));
  FX_A(dev_alloc(c, &b.front_n, B));
  FX_A(dev_alloc(c, &b.slow, B));
  FX_A(dev_alloc(c, &b.slow_state, B));
  FX_A(dev_alloc(c, &b.ring_pending, B * ((R + 31) / 32)));
  if (hipMemset(b.slow_state, 0, B * sizeof(uint32_t)) != hipSuccess || hipMemset(b.ring_pending, 0, B * ((R + 31) / 32) * sizeof(uint32_t)) != hipSuccess)
    return bail(fail(FX_ERR_HIP, "hipMemset"));
  {
    // the slow tier's scratch: a region per workgroup of its largest grid — a CU's worth of workgroups, fewer for small
    // contexts or huge limits (256 MB at most)
    const size_t words = fxk_slow_words(L.max_ring_points, L.max_candidates, c->merge_huge_ccap);
    size_t slots = std::min<size_t>((size_t)c->plan_cfg.n_cu, B);
    while (slots > 1 && slots * words * 4 > ((size_t)256 << 20)) --slots;
    P.gs_words = (uint32_t)words;
    P.gs_slots = (uint32_t)slots;
    FX_A(dev_alloc(c, &b.gs_pool, slots * words));
  }
  {
    // dense_slow_loop's scratch: a region per workgroup (a handful of them), 128 MB at most
    const size_t words = fxk_dense_slow_words(L.max_points);
    size_t slots = 32;
    while (slots > 1 && slots * words * 4 > ((size_t)128 << 20)) --slots;
    P.gsd_words = (uint32_t)words;
    P.gsd_slots = (uint32_t)slots;
    FX_A(dev_alloc(c, &b.gsd_pool, slots * words));
  }
  // (the large merge tier's bin-ordered copy: k_merge_huge, and k_front_redo — whose LDS image holds fewer candidates as points
  //  than k_merge_big's — whenever a scan has more candidates than that)
  FX_A(dev_alloc(c, &b.merge_sorted, (size_t)B * L.max_candidates));
  // (the large merge tier as three launches: a region per scan, when the tier exists and the regions stay within 256 MB)
  if (c->plan_cfg.merge_big_cap < L.max_candidates && (size_t)B * fxk_merge_hp_words(c->merge_huge_cap) * 4 <= ((size_t)256 << 20))
    FX_A(dev_alloc(c, &b.merge_hp, (size_t)B * fxk_merge_hp_words(c->merge_huge_cap)));
  FX_A(dev_alloc(c, &b.list_desc, L.max_total_keypoints));
  FX_A(dev_alloc(c, &b.s_pts, (size_t)L.max_total_keypoints * P.list_cap));
  FX_A(dev_alloc(c, &b.s_cnt, L.max_total_keypoints));
  FX_A(dev_alloc(c, &b.gather_cnt, (size_t)B * fxk_gather_counted_max() * L.max_keypoints));
  FX_A(dev_alloc(c, &b.row_map, L.max_total_keypoints));
  FX_A(dev_alloc(c, &b.row_kp, L.max_total_keypoints));
  FX_A(dev_alloc(c, &b.row_xa, L.max_total_keypoints));
  FX_A(dev_alloc(c, &b.wave_desc, L.max_total_keypoints));
  FX_A(dev_alloc(c, &b.group_desc, (size_t)FX_GROUP_CLASSES * L.max_total_keypoints));
  // dense tier
  FX_A(dev_alloc(c, &b.dense_rows, P.max_dense_rows));
  FX_A(dev_alloc(c, &b.dense_order, (size_t)4 * P.max_dense_rows));
  FX_A(dev_alloc(c, &b.dense_off, P.max_dense_rows));
  FX_A(dev_alloc(c, &b.dense_koff, P.max_dense_rows));
  FX_A(dev_alloc(c, &b.dense_nq, P.max_dense_rows));
  FX_A(dev_alloc(c, &b.dense_nm, P.max_dense_rows));
  FX_A(dev_alloc(c, &b.dense_cells, (size_t)P.max_dense_rows * fxk_dense_cells()));
  FX_A(dev_alloc(c, &b.dense_items, (size_t)P.dense_cap / 256 + P.max_dense_rows + 1));
  FX_A(dev_alloc(c, &b.dense_pts, P.dense_cap));
  FX_A(dev_alloc(c, &b.dense_q, P.dense_qcap));
  FX_A(dev_alloc(c, &b.dense_qoff, P.max_dense_rows));
  FX_A(dev_alloc(c, &b.dense_key, P.dense_cap));
  FX_A(dev_alloc(c, &b.dens_cache, B * L.max_points));
  FX_A(dev_alloc(c, &b.seq, 1));
  FX_A(dev_alloc(c, &b.ovf_pts, (size_t)B * P.ovf_cap));
  FX_A(dev_alloc(c, &b.ovf_kp, (size_t)B * P.ovf_cap));
  FX_A(dev_alloc(c, &b.ovf_cnt, B));
  if (hipMemset(b.dens_cache, 0, B * L.max_points * sizeof(unsigned long long)) != hipSuccess) return bail(fail(FX_ERR_HIP, "hipMemset"));
  if (hipMemset(b.seq, 0, sizeof(unsigned long long)) != hipSuccess) return bail(fail(FX_ERR_HIP, "hipMemset"));
  if (hipMemset(b.ovf_cnt, 0, B * sizeof(uint32_t)) != hipSuccess) return bail(fail(FX_ERR_HIP, "hipMemset"));
  FX_A(dev_alloc(c, &b.counters, FX_N_COUNTER_WORDS));
  {
    uint32_t *h = nullptr;
    FX_A(host_alloc(c, &h, FX_N_HINTS));
    for (int i = 0; i < FX_N_HINTS; ++i) h[i] = 0xffffffffu;  // nothing known yet: full grids
    void *dv = nullptr;
    if (hipHostGetDevicePointer(&dv, h, 0) != hipSuccess) return bail(fail(FX_ERR_HIP, "hipHostGetDevicePointer"));
    b.tier_hint = (uint32_t *)dv;
    c->tier_hint = h;
    if (const char *e = test_hook("FX_TIER_MIN_GRID")) pc.tier_min_grid = (uint32_t)std::max(0, atoi(e));
  }
  FX_A(dev_alloc(c, &b.clk, 2 * FX_CLK_SLOTS));
  {
    std::vector<unsigned long long> init(2 * FX_CLK_SLOTS);
    for (int i = 0; i < FX_CLK_SLOTS; ++i) init[2 * i] = ~0ull, init[2 * i + 1] = 0ull;
    if (hipMemcpy(b.clk, init.data(), init.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return bail(fail(FX_ERR_HIP, "hipMemcpy"));
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_id) == hipSuccess && khz > 0) c->clk_khz = khz;
  }
  FX_A(dev_alloc(c, &b.stamps, 64 * 64));
  if (hipMemset(b.stamps, 0, 64 * 64 * 8) != hipSuccess) return bail(fail(FX_ERR_HIP, "hipMemset"));

  // ---- tables
  {
    std::vector<float2> win(R);
    const double half = params->el_step_deg / 2.0;
    for (size_t i = 0; i < R; ++i) {
      // ref: node.cpp:200-201: centre (i-7)*2-1, limits centre -+ 1.0, narrowed to float by PassThrough
      const double centre = params->el0_deg + (double)i * params->el_step_deg;
      win[i].x = (float)(centre - half);
      win[i].y = (float)(centre + half);
    }
    if (hipMemcpy(d_win, win.data(), R * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess)
      return bail(fail(FX_ERR_HIP, "upload ring windows"));
    {
      const std::vector<double> at = atan_table();
      if (hipMemcpy(d_atan, at.data(), at.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return bail(fail(FX_ERR_HIP, "upload arctangent table"));
    }
    FxScTables T;
    std::vector<float> lut(FX_DESC_BINS);
    fx_sc3d_tables(params->descriptor_radius, T.radii, T.theta, T.phi, lut.data());
    for (int k = 0; k < 11; ++k)
      for (int j = 0; j < 15; ++j) T.lut[k * 15 + j] = lut[k * 15 + j];  // azimuth bin 0; all azimuth bins are equal
    if (hipMemcpy(d_tab, &T, sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
      return bail(fail(FX_ERR_HIP, "upload 3DSC tables"));
    std::vector<float2> xa(L.max_keypoints);
    for (uint32_t k = 0; k < L.max_keypoints; ++k) {
      float xy[2];
      fx_sc3d_xaxis(k, xy);
      xa[k].x = xy[0];
      xa[k].y = xy[1];
    }
    if (hipMemcpy(d_xa, xa.data(), xa.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess)
      return bail(fail(FX_ERR_HIP, "upload 3DSC x-axes"));
  }
  for (int i = 0; i < kMetaSlots; ++i) {
    FX_A(host_alloc(c, &c->h_meta[i], B));
    if (hipEventCreateWithFlags(&c->meta_ev[i], hipEventDisableTiming) != hipSuccess)
      return bail(fail(FX_ERR_HIP, "hipEventCreate"));
  }
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(FX_ERR_HIP, "hipStreamCreate"));
  c->stream = c->own_stream;
  {
    hipError_t ce = fxk_configure(fxk_ring_large_lds_bytes(c->ring_lds_cap, c->ring_lds_cap), fxk_merge_lds_bytes(c->plan_cfg.merge_big_cap, params->n_rings),
                                  c->plan_cfg.merge_big_cap < L.max_candidates ? fxk_merge_huge_lds_bytes(c->merge_huge_cap, c->merge_huge_ccap, params->n_rings) : 0,
                                  fxk_desc_lds_bytes(P.list_cap < P.dense_min ? P.list_cap : P.dense_min), fxk_gather_lds_bytes(L.max_keypoints));
    if (ce != hipSuccess) return bail(fail(FX_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(ce)));
  }
  if (hipMemset(b.counters, 0, FX_N_COUNTER_WORDS * sizeof(uint32_t)) != hipSuccess) return bail(fail(FX_ERR_HIP, "hipMemset"));
  // ---- the launch policy's view of the context (csrc/fx_launch_plan.h)
  pc.n_rings = (uint32_t)params->n_rings, pc.estimate_descriptors = P.estimate_descriptors != 0;
  pc.max_points = L.max_points, pc.max_keypoints = L.max_keypoints, pc.max_total_keypoints = L.max_total_keypoints;
  pc.max_candidates = L.max_candidates, pc.max_ring_points = L.max_ring_points;
  pc.list_cap = P.list_cap, pc.dense_min = P.dense_min, pc.gs_slots = P.gs_slots, pc.gsd_slots = P.gsd_slots;
  pc.merge_hp = b.merge_hp != nullptr, pc.gather_cnt = b.gather_cnt != nullptr;
  pc.prep_slices_max = fxk_prep_slices_max(), pc.merge_slices_max = fxk_merge_slices_max(), pc.gather_counted_max = fxk_gather_counted_max();
  pc.front_merge_cap = fxk_front_merge_cap(), pc.gather_kcap = fxk_gather_kcap(), pc.gather_slices_big = fxk_gather_slices_big();
  pc.dsort_per_cu = fxk_dsort_per_cu(), pc.ddens_per_cu = fxk_ddens_per_cu();
  pc.front_ok = (uint32_t)params->n_rings <= fxk_front_max_rings();
  if (const char *e = test_hook("FX_FRONT")) pc.front_ok = pc.front_ok && atoi(e) != 0;  // 0 = the separate kernels (measurements; tests of those kernels)
  // 1: k_front hands every scan to k_front_redo; 2: and that one every ring and merge to the slow tier, k_slow (tests of those two)
  if (const char *e = test_hook("FX_FRONT_FORCE")) pc.front_force = (uint32_t)std::max(0, atoi(e));
  if (const char *e = test_hook("FX_FRONT_STREAM")) pc.front_stream = atoi(e) != 0 ? 1 : 0;
  if (const char *e = test_hook("FX_FRONT_SPLIT")) pc.front_split = std::max(0, std::min(2, atoi(e)));  // (2: k_front_cd with the lean image)
  if (const char *e = test_hook("FX_FAIL_AFTER_ENQUEUE")) c->fail_after = (uint32_t)std::max(0, atoi(e));
  if (const char *e = test_hook("FX_SKIP_EMPTY")) pc.skip_mask = (uint32_t)std::max(0, atoi(e));
  if (const char *e = test_hook("FX_DENSE_SLOW")) pc.dense_force = atoi(e) != 0 ? 1 : 0;
  if (const char *e = test_hook("FX_PREP_SLICES")) pc.prep_slices = std::max(1, atoi(e));
  if (const char *e = test_hook("FX_MERGE_SLICES")) pc.merge_slices = std::max(1, atoi(e));
  if (const char *e = test_hook("FX_GATHER_COUNTED")) pc.gather_slices = std::max(1, atoi(e));
  if (const char *e = test_hook("FX_GATHER_ONE")) {  // one workgroup a scan at any batch size: 256 k_gather, 1024 k_gather_wide
    const int v = atoi(e);
    if (v == 256 || v == 1024) pc.gather_one = v;
  }
  if (const char *e = test_hook("FX_CSR_FULL_ROWS")) c->csr_full_rows = atoi(e) != 0 ? 1u : 0u;
  if (pc.front_ok) {
    hipError_t ce = fxk_configure_front();
    if (ce != hipSuccess) return bail(fail(FX_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(ce)));
  }
  if (hipMemset(b.kp_offset, 0, (B + 1) * sizeof(uint32_t)) != hipSuccess) return bail(fail(FX_ERR_HIP, "hipMemset"));
  if (hipMemset(b.n_kp, 0, B * sizeof(uint32_t)) != hipSuccess) return bail(fail(FX_ERR_HIP, "hipMemset"));
#undef FX_A
  *out = c;
  return FX_OK;
}

void fx_destroy(fx_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
  (void)hipDeviceSynchronize();
  for (void *p : c->dev_allocs) (void)hipFree(p);
  for (void *p : c->host_allocs) (void)hipHostFree(p);
  if (c->d_stage) (void)hipFree(c->d_stage);
  if (c->d_csr) (void)hipFree(c->d_csr);
  if (c->h_csr) (void)hipHostFree(c->h_csr);
  c->match_stage.release(), c->match_scratch.release(), c->reg_stage.release(), c->track_scratch.release(), c->map_scratch.release(),
      c->merge_scratch.release(), c->splice_scratch.release();
  if (c->snap_h) (void)hipHostFree(c->snap_h);
  if (c->snap_ev) (void)hipEventDestroy(c->snap_ev);
  for (int i = 0; i < kMetaSlots; ++i)
    if (c->meta_ev[i]) (void)hipEventDestroy(c->meta_ev[i]);
  for (hipEvent_t e : c->ev_ring) (void)hipEventDestroy(e);
  for (auto &g : c->graphs) (void)hipGraphExecDestroy(g.second);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

fx_status fx_set_stream(fx_ctx *c, void *hip_stream) {
  if (!c) return fail(FX_ERR_INVALID_ARG, "null ctx");
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
  return FX_OK;
}
fx_status fx_get_stream(fx_ctx *c, void **hip_stream) {
  if (!c || !hip_stream) return fail(FX_ERR_INVALID_ARG, "null argument");
  *hip_stream = (void *)c->stream;
  return FX_OK;
}
fx_status fx_set_batches_in_flight(fx_ctx *c, uint32_t n) {
  if (!c) return fail(FX_ERR_INVALID_ARG, "null ctx");
  c->plan_cfg.batches_in_flight = n ? n : 1u;
  if (!c->graphs.empty()) {  // (captured grids are fixed: graphs are rebuilt with the new ones — once no replay of an old one is still running)
    FX_HIP(hipSetDevice(c->device));
    FX_HIP(hipStreamSynchronize(c->stream));
    for (auto &g : c->graphs) (void)hipGraphExecDestroy(g.second);
    c->graphs.clear();
  }
  return FX_OK;
}
fx_status fx_set_graph_batch(fx_ctx *c, uint32_t max_batch) {
  if (!c) return fail(FX_ERR_INVALID_ARG, "null ctx");
  c->graph_max_batch = max_batch;
  return FX_OK;
}

fx_status fx_set_profiling(fx_ctx *c, int depth) {
  if (!c || depth < 0) return fail(FX_ERR_INVALID_ARG, "bad argument");
  FX_HIP(hipSetDevice(c->device));
  FX_HIP(hipStreamSynchronize(c->stream));
  for (hipEvent_t e : c->ev_ring) (void)hipEventDestroy(e);
  c->ev_ring.clear();
  c->ev_depth = (uint32_t)depth;
  c->ev_count = 0;
  c->profiling = depth > 0;
  c->ev_ring.resize((size_t)depth * (FX_N_STAGES + 1), nullptr);
  c->ev_mask.assign((size_t)depth, ~0u);
  c->ev_seq.assign((size_t)depth, 0);
  for (hipEvent_t &e : c->ev_ring) FX_HIP(hipEventCreate(&e));
  return FX_OK;
}
fx_status fx_get_limits(const fx_ctx *c, fx_limits *l) {
  if (!c || !l) return fail(FX_ERR_INVALID_ARG, "null argument");
  *l = c->lim;
  return FX_OK;
}
fx_status fx_set_profiling_stages(fx_ctx *c, uint32_t stage_mask) {
  if (!c) return fail(FX_ERR_INVALID_ARG, "null ctx");
  c->prof_mask = stage_mask;
  return FX_OK;
}
fx_status fx_get_timings(fx_ctx *c, uint32_t back, fx_timings *t) {
  if (!c || !t) return fail(FX_ERR_INVALID_ARG, "null argument");
  std::memset(t, 0, sizeof(*t));
  if (!c->profiling || back >= c->ev_count || back >= c->ev_depth)
    return fail(FX_ERR_INVALID_ARG, "no profiled batch that far back (fx_set_profiling(depth) first)");
  hipEvent_t *ev = &c->ev_ring[(size_t)((c->ev_count - 1 - back) % c->ev_depth) * (FX_N_STAGES + 1)];
  FX_HIP(hipEventSynchronize(ev[FX_N_STAGES]));
  const uint32_t mask = c->ev_mask[(c->ev_count - 1 - back) % c->ev_depth];
  for (int i = 0; i < FX_N_STAGES; ++i)
    if ((mask >> i) & 1u) FX_HIP(hipEventElapsedTime(&t->ms[i], ev[i], ev[i + 1]));  // (stages without events stay 0)
  FX_HIP(hipEventElapsedTime(&t->total_ms, ev[0], ev[FX_N_STAGES]));
  {  // k_prep's own execution span (the batch has completed: its clock slot is final, and not yet reused)
    const uint64_t seq = c->ev_seq[(c->ev_count - 1 - back) % c->ev_depth];
    unsigned long long span[2] = {0, 0};
    if (c->batch_seq - seq < FX_CLK_SLOTS - 1) {
      FX_HIP(hipMemcpy(span, c->buf.clk + 2 * (seq % FX_CLK_SLOTS), sizeof(span), hipMemcpyDeviceToHost));
      if (span[1] > span[0]) t->k_prep_exec_ms = (float)((double)(span[1] - span[0]) / c->clk_khz);
    }
  }
  return FX_OK;
}
// Algorithmic bytes per stage of the last batch, from the batch's own counts (diagnostic: small device-to-host copies).
fx_status fx_get_stage_bytes(fx_ctx *c, fx_stage_bytes *out) {
  if (!c || !out) return fail(FX_ERR_INVALID_ARG, "null argument");
  std::memset(out, 0, sizeof(*out));
  const uint32_t B = c->plan_state.last_batch;
  if (!B) return FX_OK;
  FX_HIP(hipSetDevice(c->device));
  FX_HIP(hipStreamSynchronize(c->stream));
  const fx_limits &L = c->lim;
  const FxBuffers &b = c->buf;
  const size_t R = (size_t)c->params.n_rings;
  auto fetch = [&](const uint32_t *src, size_t n, std::vector<uint32_t> &v) -> hipError_t {
    v.resize(n);
    return n ? hipMemcpy(v.data(), src, n * 4, hipMemcpyDeviceToHost) : hipSuccess;
  };
  std::vector<uint32_t> n_filt, ring_cnt, ring_cand, kpc_ring, n_cand, n_kp, n_kpc, kp_off, s_cnt, near;
  std::vector<FxScanMeta> meta(B);
  FX_HIP(hipMemcpy(meta.data(), c->d_meta, (size_t)B * sizeof(FxScanMeta), hipMemcpyDeviceToHost));
  FX_HIP(fetch(b.n_filt, B, n_filt));
  FX_HIP(fetch(b.ring_cnt, B * R, ring_cnt));
  FX_HIP(fetch(b.ring_cand_cnt, B * R, ring_cand));
  FX_HIP(fetch(b.kpc_ring_cnt, B * R, kpc_ring));
  FX_HIP(fetch(b.n_cand, B, n_cand));
  FX_HIP(fetch(b.n_kp, B, n_kp));
  FX_HIP(fetch(b.n_kpc, B, n_kpc));
  FX_HIP(fetch(b.kp_offset, B + 1, kp_off));
  uint32_t total_kp = kp_off[B] < L.max_total_keypoints ? kp_off[B] : L.max_total_keypoints;
  FX_HIP(fetch(b.s_cnt, total_kp, s_cnt));
  FX_HIP(fetch(b.near_bits, (size_t)B * c->dp.near_words, near));
  double n_pts = 0, nf = 0, n_ring = 0, n_rc = 0, n_mem = 0, nc = 0, nk = 0, nkpc = 0, near_pts = 0;
  for (uint32_t i = 0; i < B; ++i) {
    n_pts += meta[i].n, nf += n_filt[i], nc += n_cand[i], nk += n_kp[i], nkpc += n_kpc[i];
    for (size_t r = 0; r < R; ++r) n_ring += ring_cnt[i * R + r], n_rc += ring_cand[i * R + r], n_mem += kpc_ring[i * R + r];
    if (n_kp[i]) {  // (k_gather does not touch a scan without keypoints)
      const uint32_t words = (meta[i].n + 127u) / 128u;  // one bit per four points
      for (uint32_t w = 0; w < words && w < c->dp.near_words; ++w) near_pts += 4.0 * __builtin_popcount(near[(size_t)i * c->dp.near_words + w]);
    }
  }
  double s_small = 0, s_mid = 0, s_dense = 0, rows_mid = 0, rows_dense = 0;
  for (uint32_t r = 0; r < total_kp; ++r) {
    const double n = s_cnt[r];
    if (s_cnt[r] > c->dp.dense_min || s_cnt[r] > c->dp.list_cap)
      s_dense += n, rows_dense += 1;
    else if (s_cnt[r] > 64u)
      s_mid += n, rows_mid += 1;
    else
      s_small += n;
  }
  const bool desc = c->params.estimate_descriptors != 0;
  double *rd = out->read, *wr = out->written;
  rd[0] = 16.0 * n_pts, wr[0] = 16.0 * nf + n_pts / 32.0 + 4.0 * R * B;      // k_prep: the scan; ~cloud, near-sector bits, ring counts
  rd[1] = 16.0 * nf, wr[1] = 16.0 * n_ring;                                     // k_bucket: ~cloud; ring-major copy
  rd[2] = 16.0 * n_ring, wr[2] = 20.0 * n_rc + 20.0 * n_mem;                   // ring tiers: ring points; candidates + sizes, members + their candidate
  rd[3] = 0, wr[3] = 0;                                                         // (the larger ring tiers' share is counted with the first)
  rd[4] = 20.0 * n_rc + 20.0 * n_mem, wr[4] = 24.0 * nc + 20.0 * nk + 20.0 * nkpc;  // merge: candidates, members; keypoints_full + maps, keypoints, keypoint_cloud
  if (c->plan_state.front_last) {  // k_front: the scan in; ~cloud, near bits, ring counts, keypoints_full + maps, keypoints, keypoint_cloud out — no intermediates
    wr[0] += wr[4];
    for (int i = 1; i <= 4; ++i) rd[i] = wr[i] = 0;
  }
  if (desc) {
    rd[5] = 16.0 * near_pts + 16.0 * nk, wr[5] = 16.0 * (s_small + s_mid + s_dense) + 40.0 * nk;  // k_gather: near sectors; support lists + row tables
    rd[6] = 16.0 * s_small + 44.0 * total_kp, wr[6] = 7956.0 * total_kp;       // k_desc (timed in the k_desc_group slot), group tier: short lists; every row (cleared by its tier)
    rd[7] = 16.0 * s_mid, wr[7] = 0.0 * rows_mid;                               // k_desc, wave and list tiers (the k_desc_mid slot of the accounting): lists; (non-empty bins of rows already counted)
    rd[8] = 16.0 * s_dense, wr[8] = 0.0 * rows_dense;                           // dense tier: lists
  }
  return FX_OK;
}
fx_status fx_synchronize(fx_ctx *c) {
  if (!c) return fail(FX_ERR_INVALID_ARG, "null ctx");
  FX_HIP(hipStreamSynchronize(c->stream));
  return FX_OK;
}

fx_status fx_process_batch(fx_ctx *c, const fx_scan_desc *scans, uint32_t batch, uint32_t flags, fx_batch_view *out) {
  if (!c || (!scans && batch) || !out) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (batch > c->lim.max_batch) return fail(FX_ERR_TOO_LARGE, "batch > max_batch");
  const bool csr = (flags & FX_OUT_DESC_CSR) != 0;
  if (csr && !(flags & FX_OUT_HOST)) return fail(FX_ERR_INVALID_ARG, "FX_OUT_DESC_CSR needs FX_OUT_HOST");
  if (csr && !csr_pool_fits(c->lim)) return fail(FX_ERR_TOO_LARGE, "FX_OUT_DESC_CSR: max_total_keypoints * 1989 exceeds 2^32 - 1");
  c->csr_valid = false;
  FX_HIP(hipSetDevice(c->device));
  const fx_limits &L = c->lim;
  hipStream_t s = c->stream;

  // ---- scan table
  const int slot = c->meta_next;
  c->meta_next = (c->meta_next + 1) % kMetaSlots;
  if (c->meta_used[slot]) FX_HIP(hipEventSynchronize(c->meta_ev[slot]));
  FxScanMeta *hm = c->h_meta[slot];
  const bool in_dev = (flags & FX_IN_DEVICE) != 0;
  for (uint32_t i = 0; i < batch; ++i) {
    const fx_scan_desc &d = scans[i];
    if (d.n_points > L.max_points) return fail(FX_ERR_TOO_LARGE, "scan has more points than max_points");
    if (d.n_points && !d.points) return fail(FX_ERR_INVALID_ARG, "scan with null points");
    if (d.stride_bytes < 16 || (d.stride_bytes % 16) != 0 || d.stride_bytes > 256)
      return fail(FX_ERR_INVALID_ARG, "stride_bytes must be a multiple of 16 in [16, 256]");
    if (((uintptr_t)d.points % 16) != 0) return fail(FX_ERR_INVALID_ARG, "points must be 16-byte aligned");
    hm[i].n = d.n_points;
    hm[i].pad_ = 0;
    // (scans of one sensor and instant share their attitude: the matrix — four trigonometric calls — is built once per run of
    //  equal angles; a 1024-scan batch spent 0.25 ms of host time here, most of the enqueue)
    if (i && d.roll == scans[i - 1].roll && d.pitch == scans[i - 1].pitch)
      std::memcpy(hm[i].R, hm[i - 1].R, sizeof(hm[i].R));
    else
      fx_rotation_from_roll_pitch(d.roll, d.pitch, hm[i].R);
    if (in_dev) {
      hm[i].pts = (const float *)d.points;
      hm[i].stride_f = d.stride_bytes / 4;
    }
  }
  if (!in_dev && batch) {
    // Host scans go over as they are, whatever their record stride (16: packed x y z i; 32: pcl::PointXYZI in memory, what
    // the reference-side binding has — ref: node.cpp:81): the kernels stride over the records (FxScanMeta::stride_f), so
    // nothing is repacked on the host and nothing is waited for.  The staging buffer holds max_batch scans of the widest
    // stride seen so far.
    uint32_t stride = 16;
    for (uint32_t i = 0; i < batch; ++i) stride = std::max(stride, scans[i].stride_bytes);
    if (!c->d_stage || stride > c->stage_stride) {
      if (c->d_stage) {  // (an earlier batch issued without FX_OUT_HOST may still be reading it)
        FX_HIP(hipStreamSynchronize(s));
        FX_HIP(hipFree(c->d_stage));
        c->d_stage = nullptr;
      }
      void *q = nullptr;
      hipError_t e = hipMalloc(&q, (size_t)L.max_batch * L.max_points * stride);
      if (e != hipSuccess) return fail(FX_ERR_OOM, std::string("staging hipMalloc: ") + hipGetErrorString(e));
      c->d_stage = (float *)q;
      c->stage_stride = stride;
    }
    const size_t slot_bytes = (size_t)L.max_points * c->stage_stride;
    for (uint32_t i = 0; i < batch; ++i) {
      const fx_scan_desc &d = scans[i];
      uint8_t *dst = (uint8_t *)c->d_stage + (size_t)i * slot_bytes;
      hm[i].pts = (const float *)dst;
      hm[i].stride_f = d.stride_bytes / 4;
      if (!d.n_points) continue;
      // full-size scans that follow one another in host memory (a stacked batch) go over in one copy
      // (up to the last record's x y z i: nothing behind it is read, on the host or on the device)
      uint32_t j = i;
      size_t bytes = (size_t)(d.n_points - 1u) * d.stride_bytes + 16u;
      while (d.n_points == L.max_points && d.stride_bytes == c->stage_stride && j + 1 < batch && scans[j + 1].stride_bytes == d.stride_bytes &&
             scans[j + 1].n_points == L.max_points && (const uint8_t *)scans[j + 1].points == (const uint8_t *)scans[j].points + slot_bytes) {
        ++j;
        bytes += slot_bytes;
        hm[j].pts = (const float *)((uint8_t *)c->d_stage + (size_t)j * slot_bytes);
        hm[j].stride_f = d.stride_bytes / 4;
      }
      FX_HIP(hipMemcpyAsync(dst, d.points, bytes, hipMemcpyHostToDevice, s));
      i = j;
    }
  }
  if (batch) FX_HIP(hipMemcpyAsync(c->d_meta, hm, (size_t)batch * sizeof(FxScanMeta), hipMemcpyHostToDevice, s));
  FX_HIP(hipEventRecord(c->meta_ev[slot], s));
  c->meta_used[slot] = true;

  // ---- state a failed batch may have left behind (see fx_ctx::state_suspect)
  if (c->state_suspect) {
    FX_HIP(hipMemsetAsync(c->buf.desc_nbins, 0xff, (size_t)L.max_total_keypoints * sizeof(uint32_t), s));  // FX_ROW_DIRTY: clear whole
    FX_HIP(hipMemsetAsync(c->buf.counters, 0, FX_N_COUNTER_WORDS * sizeof(uint32_t), s));
    FX_HIP(hipMemsetAsync(c->buf.slow_state, 0, (size_t)L.max_batch * sizeof(uint32_t), s));  // (the slow tier's list markers: k_slow clears what it has done)
    FX_HIP(hipMemsetAsync(c->buf.ring_pending, 0, (size_t)L.max_batch * (((size_t)c->params.n_rings + 31) / 32) * sizeof(uint32_t), s));
    FX_HIP(hipStreamSynchronize(s));  // (the hints are host memory the device writes: nothing of the failed batch may land after the reset)
    for (int i = 0; i < FX_N_HINTS; ++i) c->tier_hint[i] = FX_HINT_UNKNOWN;
    c->plan_state.reset();
    c->state_suspect = false;
  }
  struct Suspect {  // armed from the first launch to the successful return
    fx_ctx *c;
    bool armed = false;
    ~Suspect() {
      if (armed) c->state_suspect = true;
    }
  } suspect{c};
  suspect.armed = true;
  // ---- kernels
  const FxDevParams &P = c->dp;
  const FxBuffers &B = c->buf;
  const bool prof = c->profiling;
  // what the last COMPLETED batch of this context left for the rarely used tiers (with batches in flight: an older batch's
  // counts, possibly of another size — they decide speed only, never a result), read once
  uint32_t hints[FX_N_HINTS];
  for (int i = 0; i < FX_N_HINTS; ++i) hints[i] = c->tier_hint[i];
  if (!prof && !c->debug_sync && batch && batch <= c->graph_max_batch && s != nullptr)  // (a graph replays a plan made at its capture: only the front is decided per batch)
    FX_TRY(launch_graph(c, s, batch, fx_plan_front(c->plan_cfg, &c->plan_state, hints[FX_HINT_REDO_SCANS], batch)));
  else
    FX_TRY(enqueue_stages(c, s, batch, prof, fx_plan_batch(c->plan_cfg, &c->plan_state, hints, batch, false)));
#ifdef FX_TEST_HOOKS
  if (c->fail_after && c->batch_seq + 1 == c->fail_after) {  // a failure after the kernels went out
    ++c->batch_seq;
    return fail(FX_ERR_HIP, "FX_FAIL_AFTER_ENQUEUE (test hook)");
  }
#endif
  if (prof) ++c->ev_count;
  ++c->batch_seq;

  // ---- view
  std::memset(out, 0, sizeof(*out));
  out->batch = batch;
  out->max_points = L.max_points;
  out->max_keypoints = L.max_keypoints;
  out->max_candidates = L.max_candidates;
  out->max_kpc_points = L.max_kpc_points;
  out->d_n_keypoints = B.n_kp;
  out->d_kp_offset = B.kp_offset;
  out->d_keypoints = (const float *)B.keypoints;
  out->d_descriptors = B.desc;
  out->d_flags = B.flags;
  out->d_n_filtered = B.n_filt;
  out->d_filtered = (const float *)B.filt;
  out->d_n_kpc = B.n_kpc;
  out->d_kpc = (const float *)B.kpc;

  if (!(flags & FX_OUT_HOST)) {
    suspect.armed = false;
    return FX_OK;
  }
  const size_t Bm = L.max_batch;
  const size_t S = c->hdr_stride;
  FX_TRY(host_alloc(c, &c->h_hdr, 5 * S));
  c->h_n_kp = c->h_hdr, c->h_kp_offset = c->h_hdr + S, c->h_flags = c->h_hdr + 2 * S, c->h_n_filt = c->h_hdr + 3 * S, c->h_n_kpc = c->h_hdr + 4 * S;
  FX_TRY(host_alloc(c, &c->h_keypoints, Bm * L.max_keypoints * 4));
  if (!csr) FX_TRY(host_alloc(c, &c->h_desc, (size_t)L.max_total_keypoints * FX_DESC_FLOATS));
  if (csr) {
    // the batch's rows packed behind its kernels; the header comes back with the per-scan words
    if (!c->d_csr || c->csr_resize) {
      const uint32_t want = c->csr_cap_want ? c->csr_cap_want
                                            : (uint32_t)std::min<uint64_t>((uint64_t)L.max_total_keypoints * kCsrRowEntries,
                                                                           (uint64_t)L.max_total_keypoints * FX_DESC_FLOATS);
      FX_TRY(csr_reserve(c, std::max(want, 1u)));
      c->csr_resize = false;
    }
    FX_TRY(enqueue_csr(c, s, c->d_csr, L.max_total_keypoints, c->csr_cap));
    FX_HIP(hipMemcpyAsync(c->h_csr, c->d_csr, 16, hipMemcpyDeviceToHost, s));
  }
  if (batch) {
    // (n_kp | kp_offset | flags | n_filt | n_kpc, S words each: everything up to the last array's last scan of this batch)
    FX_HIP(hipMemcpyAsync(c->h_hdr, B.n_kp, (4 * S + batch) * 4, hipMemcpyDeviceToHost, s));
    FX_HIP(hipMemcpyAsync(c->h_keypoints, B.keypoints, (size_t)batch * L.max_keypoints * 16, hipMemcpyDeviceToHost, s));
  } else {
    c->h_kp_offset[0] = 0;
  }
  FX_HIP(hipStreamSynchronize(s));
  uint32_t total = batch ? c->h_kp_offset[batch] : 0;
  if (total > L.max_total_keypoints) total = L.max_total_keypoints;
  out->total_keypoints = total;
  // (about as many rows as the last call had, copied BEFORE the wait, and the per-scan words in one block instead of five
  //  copies: measured for a scan per call, 0.244 ms either way — the copies are not what the call waits for; the one block stayed)
  if (total && P.estimate_descriptors && !csr)
    FX_HIP(hipMemcpyAsync(c->h_desc, B.desc, (size_t)total * FX_DESC_FLOATS * 4, hipMemcpyDeviceToHost, s));
  if (csr) {
    const uint32_t *hd = (const uint32_t *)c->h_csr;  // {rows, nnz_stored, nnz_needed, rows_stored}
    const uint32_t rows = hd[0], nnz = hd[2];
    if (hd[3] < rows) {
      // lossless: the dense rows are intact until the next batch — a larger block (an eighth of slack) and the pack again
      const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)nnz + nnz / 8u, (uint64_t)L.max_total_keypoints * FX_DESC_FLOATS);
      FX_TRY(csr_reserve(c, cap));
      FX_TRY(enqueue_csr(c, s, c->d_csr, L.max_total_keypoints, c->csr_cap));
    }
    const size_t col = csr_col_offset(L.max_total_keypoints), val = csr_val_offset(L.max_total_keypoints, c->csr_cap);
    FX_HIP(hipMemcpyAsync(c->h_csr + 16, c->d_csr + 16, ((size_t)rows + 1u) * 4u, hipMemcpyDeviceToHost, s));
    if (nnz) {
      FX_HIP(hipMemcpyAsync(c->h_csr + col, c->d_csr + col, (size_t)nnz * 4u, hipMemcpyDeviceToHost, s));
      FX_HIP(hipMemcpyAsync(c->h_csr + val, c->d_csr + val, (size_t)nnz * 4u, hipMemcpyDeviceToHost, s));
    }
    c->csr_rows = rows, c->csr_nnz = nnz;
  }
  if (flags & FX_OUT_CLOUDS) {
    FX_TRY(host_alloc(c, &c->h_filtered, Bm * L.max_points * 4));
    FX_TRY(host_alloc(c, &c->h_kpc, Bm * L.max_kpc_points * 4));
    for (uint32_t i = 0; i < batch; ++i) {
      if (c->h_n_filt[i])
        FX_HIP(hipMemcpyAsync(c->h_filtered + (size_t)i * L.max_points * 4, B.filt + (size_t)i * L.max_points,
                              (size_t)c->h_n_filt[i] * 16, hipMemcpyDeviceToHost, s));
      if (c->h_n_kpc[i])
        FX_HIP(hipMemcpyAsync(c->h_kpc + (size_t)i * L.max_kpc_points * 4, B.kpc + (size_t)i * L.max_kpc_points,
                              (size_t)c->h_n_kpc[i] * 16, hipMemcpyDeviceToHost, s));
    }
    out->h_filtered = c->h_filtered;
    out->h_kpc = c->h_kpc;
  }
  if (flags & FX_OUT_DEBUG) {
    FX_TRY(host_alloc(c, &c->h_n_cand, Bm));
    FX_TRY(host_alloc(c, &c->h_cand, Bm * L.max_candidates * 4));
    FX_TRY(host_alloc(c, &c->h_cand_size, Bm * L.max_candidates));
    FX_TRY(host_alloc(c, &c->h_cand_kp, Bm * L.max_candidates));
    FX_TRY(host_alloc(c, &c->h_kpc_cand, Bm * L.max_kpc_points));
    FX_TRY(host_alloc(c, &c->h_kp_size, Bm * L.max_keypoints));
    FX_TRY(host_alloc(c, &c->h_kp_nbrs, Bm * L.max_keypoints));
    if (batch) {
      FX_HIP(hipMemcpyAsync(c->h_n_cand, B.n_cand, batch * 4, hipMemcpyDeviceToHost, s));
      FX_HIP(hipMemcpyAsync(c->h_cand, B.cand, (size_t)batch * L.max_candidates * 16, hipMemcpyDeviceToHost, s));
      FX_HIP(hipMemcpyAsync(c->h_cand_size, B.cand_size, (size_t)batch * L.max_candidates * 4, hipMemcpyDeviceToHost, s));
      FX_HIP(hipMemcpyAsync(c->h_cand_kp, B.cand_kp, (size_t)batch * L.max_candidates * 4, hipMemcpyDeviceToHost, s));
      FX_HIP(hipMemcpyAsync(c->h_kpc_cand, B.kpc_cand, (size_t)batch * L.max_kpc_points * 4, hipMemcpyDeviceToHost, s));
      FX_HIP(hipMemcpyAsync(c->h_kp_size, B.kp_size, (size_t)batch * L.max_keypoints * 4, hipMemcpyDeviceToHost, s));
      FX_HIP(hipMemcpyAsync(c->h_kp_nbrs, B.kp_nbrs, (size_t)batch * L.max_keypoints * 4, hipMemcpyDeviceToHost, s));
    }
    out->h_n_candidates = c->h_n_cand;
    out->h_candidates = c->h_cand;
    out->h_cand_size = c->h_cand_size;
    out->h_cand_keypoint = c->h_cand_kp;
    out->h_kpc_cand = c->h_kpc_cand;
    out->h_kp_size = c->h_kp_size;
    out->h_kp_neighbors = c->h_kp_nbrs;
  }
  FX_HIP(hipStreamSynchronize(s));
  out->h_n_keypoints = c->h_n_kp;
  out->h_kp_offset = c->h_kp_offset;
  out->h_keypoints = c->h_keypoints;
  out->h_descriptors = csr ? nullptr : c->h_desc;
  out->h_flags = c->h_flags;
  c->csr_valid = csr;
  out->h_n_filtered = c->h_n_filt;
  out->h_n_kpc = c->h_n_kpc;
  suspect.armed = false;
  return FX_OK;
}

#ifdef FX_TEST_HOOKS
// Test hook: k_prep's two elevation paths on caller-supplied points.
fx_status fx_test_elevation_device(int device, const float *xyz, uint32_t n, float *fast_out, uint8_t *fast_ok_out, float *exact_out) {
  if (!xyz || !fast_out || !fast_ok_out || !exact_out) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (!n) return FX_OK;
  FX_HIP(hipSetDevice(device));
  const std::vector<double> at = atan_table();
  char *d = nullptr;
  const size_t o_tab = ((size_t)n * 12 + 7) & ~(size_t)7, o_fast = o_tab + at.size() * 8, o_exact = o_fast + (size_t)n * 4, o_ok = o_exact + (size_t)n * 4;
  FX_HIP(hipMalloc((void **)&d, o_ok + n));
  hipError_t e = hipMemcpy(d, xyz, (size_t)n * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + o_tab, at.data(), at.size() * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    fxk_test_elevation(nullptr, (const float *)d, n, (const double *)(d + o_tab), (float *)(d + o_fast), (uint8_t *)(d + o_ok), (float *)(d + o_exact));
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(fast_out, d + o_fast, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(exact_out, d + o_exact, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(fast_ok_out, d + o_ok, n, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  FX_HIP(e);
  return FX_OK;
}

// Test hook: the descriptor tiers' packed within-radius count and the plain compare it replaces.
fx_status fx_test_within_device(int device, const float *support_xyzw, uint32_t n, const float *query_xyzw, uint32_t nq, float r2,
                                uint32_t *packed_out, uint32_t *plain_out) {
  if (!support_xyzw || !query_xyzw || !packed_out || !plain_out) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (!nq) return FX_OK;
  FX_HIP(hipSetDevice(device));
  char *d = nullptr;
  const size_t o_q = (size_t)(n ? n : 1) * 16, o_a = o_q + (size_t)nq * 16, o_c = o_a + (size_t)nq * 4;
  FX_HIP(hipMalloc((void **)&d, o_c + (size_t)nq * 4));
  hipError_t e = n ? hipMemcpy(d, support_xyzw, (size_t)n * 16, hipMemcpyHostToDevice) : hipSuccess;
  if (e == hipSuccess) e = hipMemcpy(d + o_q, query_xyzw, (size_t)nq * 16, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    fxk_test_within(nullptr, (const float4 *)d, n, (const float4 *)(d + o_q), nq, r2, (uint32_t *)(d + o_a), (uint32_t *)(d + o_c));
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(packed_out, d + o_a, (size_t)nq * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(plain_out, d + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  FX_HIP(e);
  return FX_OK;
}

// Test hook: what the support gather of the last batch left (include/fx.h).  Copies only: the stream is waited for, nothing is
// launched and nothing on the device is written.  Every access to s_pts, s_cnt, ovf_*, row_map, row_kp, row_class, row_xa, the
// work lists and their counters (4, 6, 8, FX_CNT_GROUP ..) behind gather_body and k_rng_ord in fx_kernels.hip is a load — the
// tiers draw TICKETS from other counters —, and near_bits is written by the streaming pass alone: what is read here after a
// batch is what the gather left.  (kp_nbrs is not read back: the descriptor tiers overwrite its flags with counts.)
fx_status fx_test_gather_state(fx_ctx *c, fx_test_gather_info *info, const fx_test_gather_out *out) {
  if (!c || !info) return fail(FX_ERR_INVALID_ARG, "null argument");
  std::memset(info, 0, sizeof(*info));
  const FxDevParams &P = c->dp;
  const FxBuffers &b = c->buf;
  const uint32_t B = c->plan_state.last_batch;
  info->batch = B;
  info->near_words = P.near_words, info->list_cap = P.list_cap, info->ovf_cap = P.ovf_cap, info->dense_min = P.dense_min;
  info->max_dense_rows = P.max_dense_rows;
  info->r2_support = P.r2_support, info->r2_search = P.r2_search, info->box_margin = c->box_margin;
  if (!B || !P.estimate_descriptors) return FX_OK;
  FX_HIP(hipSetDevice(c->device));
  FX_HIP(hipStreamSynchronize(c->stream));
  auto get = [](void *dst, const void *src, size_t bytes) -> hipError_t {
    return dst && bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
  };
  uint32_t total = 0;
  FX_HIP(hipMemcpy(&total, b.kp_offset + B, 4, hipMemcpyDeviceToHost));
  const uint32_t rows = total < P.max_total_kp ? total : P.max_total_kp;
  info->rows = rows;
  std::vector<uint32_t> cnt(FX_N_COUNTERS), ovf(B);
  FX_HIP(hipMemcpy(cnt.data(), b.counters, FX_N_COUNTERS * 4, hipMemcpyDeviceToHost));
  FX_HIP(hipMemcpy(ovf.data(), b.ovf_cnt, (size_t)B * 4, hipMemcpyDeviceToHost));
  info->n_list = cnt[4], info->n_wave = cnt[8], info->n_dense = cnt[6];
  for (uint32_t g = 0; g < FX_GROUP_CLASSES; ++g) info->n_group[g] = cnt[FX_CNT_GROUP + g];
  for (uint32_t i = 0; i < B; ++i) info->ovf_stored = std::max(info->ovf_stored, std::min(ovf[i], P.ovf_cap));
  if (!out) return FX_OK;
  const size_t S = info->ovf_stored;
  FX_HIP(get(out->near_bits, b.near_bits, (size_t)B * P.near_words * 4));
  FX_HIP(get(out->s_cnt, b.s_cnt, (size_t)rows * 4));
  FX_HIP(get(out->s_pts, b.s_pts, (size_t)rows * P.list_cap * 16));
  if (out->ovf_cnt) std::memcpy(out->ovf_cnt, ovf.data(), (size_t)B * 4);
  for (uint32_t i = 0; i < B; ++i) {
    const size_t n = std::min(ovf[i], P.ovf_cap);
    FX_HIP(get(out->ovf_pts ? out->ovf_pts + i * S * 4 : nullptr, b.ovf_pts + (size_t)i * P.ovf_cap, n * 16));
    FX_HIP(get(out->ovf_kp ? out->ovf_kp + i * S : nullptr, b.ovf_kp + (size_t)i * P.ovf_cap, n * 4));
  }
  FX_HIP(get(out->row_map, b.row_map, (size_t)rows * 8));
  FX_HIP(get(out->row_kp, b.row_kp, (size_t)rows * 16));
  FX_HIP(get(out->row_class, b.row_class, (size_t)rows));
  FX_HIP(get(out->row_xa, b.row_xa, (size_t)rows * 8));
  FX_HIP(get(out->list_desc, b.list_desc, (size_t)std::min(info->n_list, rows) * 4));
  FX_HIP(get(out->wave_desc, b.wave_desc, (size_t)std::min(info->n_wave, rows) * 4));
  for (uint32_t g = 0; g < FX_GROUP_CLASSES; ++g)
    FX_HIP(get(out->group_desc ? out->group_desc + (size_t)g * rows : nullptr, b.group_desc + (size_t)g * P.max_total_kp,
               (size_t)std::min(info->n_group[g], rows) * 4));
  FX_HIP(get(out->dense_rows, b.dense_rows, (size_t)std::min(info->n_dense, P.max_dense_rows) * 4));
  return FX_OK;
}

// Test hook: the device build of the cluster-order replay on caller-supplied size sequences.
fx_status fx_test_sort_replay_device(int device, const uint32_t *sizes, uint32_t n_seq, uint32_t n, uint32_t *perm_out) {
  if (!sizes || !perm_out) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (n > 192) return fail(FX_ERR_TOO_LARGE, "n > 192");
  if (!n_seq || !n) return FX_OK;
  FX_HIP(hipSetDevice(device));
  const size_t bytes = (size_t)n_seq * n * sizeof(uint32_t);
  uint32_t *d_in = nullptr, *d_out = nullptr;
  FX_HIP(hipMalloc((void **)&d_in, bytes));
  hipError_t e = hipMalloc((void **)&d_out, bytes);
  if (e == hipSuccess) e = hipMemcpy(d_in, sizes, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    fxk_test_sort_replay(nullptr, d_in, n_seq, n, d_out);
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(perm_out, d_out, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  FX_HIP(e);
  return FX_OK;
}

// Test hook: cc_order itself (the code the ring and merge kernels run) on caller-supplied size sequences.
fx_status fx_test_cc_order_device(int device, const uint32_t *sizes, uint32_t n_seq, uint32_t n, uint32_t min_sz, uint32_t max_sz,
                                  const uint32_t *ccap, uint32_t nt, int gs, uint32_t *perm_out, uint32_t *root_out, uint32_t *n_c_out,
                                  uint32_t *guard_bad_out) {
  if (!sizes || !ccap || !perm_out || !n_c_out || !guard_bad_out) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (nt != 64 && nt != 256 && nt != 1024) return fail(FX_ERR_INVALID_ARG, "nt: 64, 256 or 1024");
  if (n > 4096) return fail(FX_ERR_TOO_LARGE, "n > 4096");
  if (!n_seq || !n) return FX_OK;
  uint32_t ccap_max = 0;
  for (uint32_t q = 0; q < n_seq; ++q) ccap_max = std::max(ccap_max, ccap[q]);
  if (ccap_max > 4096) return fail(FX_ERR_TOO_LARGE, "ccap > 4096");  // (three arrays of it fit the LDS form)
  for (size_t i = 0; i < (size_t)n_seq * n; ++i)
    if (sizes[i] > 0xffffu) return fail(FX_ERR_INVALID_ARG, "a size above 65535 does not fit the sort record");
  FX_HIP(hipSetDevice(device));
  // one allocation: sizes | parent | ccaps | perm | roots | n_c | guard_bad | scratch (GS)
  const size_t w_seq = (size_t)n_seq * n, w_scratch = gs ? fxk_test_cc_order_scratch_words(n_seq, ccap_max) : 0;
  const size_t o_parent = w_seq, o_ccap = o_parent + n, o_perm = o_ccap + n_seq, o_root = o_perm + w_seq, o_nc = o_root + w_seq,
               o_bad = o_nc + n_seq, o_scratch = o_bad + n_seq, words = o_scratch + w_scratch;
  std::vector<uint32_t> iota(n);
  for (uint32_t i = 0; i < n; ++i) iota[i] = i;
  uint32_t *d = nullptr;
  FX_HIP(hipMalloc((void **)&d, words * 4));
  hipError_t e = hipMemset(d + o_perm, 0xff, (o_bad - o_perm) * 4);
  if (e == hipSuccess) e = hipMemset(d + o_bad, 0, (size_t)n_seq * 4);
  if (e == hipSuccess) e = hipMemcpy(d, sizes, w_seq * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + o_parent, iota.data(), (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + o_ccap, ccap, (size_t)n_seq * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess)
    e = fxk_test_cc_order(nullptr, nt, gs != 0, d, d + o_parent, n_seq, n, min_sz, max_sz, d + o_ccap, ccap_max, d + o_scratch, d + o_perm,
                          d + o_root, d + o_nc, d + o_bad);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(perm_out, d + o_perm, w_seq * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && root_out) e = hipMemcpy(root_out, d + o_root, w_seq * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(n_c_out, d + o_nc, (size_t)n_seq * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(guard_bad_out, d + o_bad, (size_t)n_seq * 4, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  FX_HIP(e);
  return FX_OK;
}

#endif  // FX_TEST_HOOKS

// Diagnostic: what the last completed batch left for the next one's tier grids (FxBuffers::tier_hint).
fx_status fx_debug_tier_hints(fx_ctx *c, uint32_t *out /* FX_N_HINTS = 8 words */) {
  if (!c || !out) return fail(FX_ERR_INVALID_ARG, "null argument");
  FX_HIP(hipSetDevice(c->device));
  FX_HIP(hipStreamSynchronize(c->stream));
  for (int i = 0; i < FX_N_HINTS; ++i) out[i] = c->tier_hint[i];
  return FX_OK;
}
// Diagnostic: 1 when the last batch went through the fused front kernel (k_front), 0 when through the separate kernels.
int fx_debug_front(fx_ctx *c) { return c && c->plan_state.front_last ? 1 : 0; }
// Diagnostic: the work-list counters of the last batch (rings / scans / keypoint rows deferred to larger tiers).
fx_status fx_debug_counters(fx_ctx *c, uint32_t *out8 /* 16 words */) {
  if (!c || !out8) return fail(FX_ERR_INVALID_ARG, "null argument");
  FX_HIP(hipSetDevice(c->device));
  FX_HIP(hipStreamSynchronize(c->stream));
  uint32_t all[FX_N_COUNTERS];
  FX_HIP(hipMemcpy(all, c->buf.counters, sizeof(all), hipMemcpyDeviceToHost));
  std::memcpy(out8, all, 16 * 4);
  out8[0] = out8[5] = 0;  // the rings handed on are counted per XCD class: 0 to the second run tier, 5 to the workgroup tier
  const bool runs2 = c->params.n_rings > 16;
  for (int k = 0; k < 8; ++k) {
    if (runs2) out8[0] += all[FX_CNT_LARGE + k];
    out8[5] += all[(runs2 ? FX_CNT_LARGE2 : FX_CNT_LARGE) + k];
  }
  return FX_OK;
}

// Diagnostic: the group rows of the last batch by size class (<= 16, <= 32, <= 64 support points; a dense row without room in the
// pools counts with the last).
fx_status fx_debug_group_classes(fx_ctx *c, uint32_t *out3 /* FX_GROUP_CLASSES words */) {
  if (!c || !out3) return fail(FX_ERR_INVALID_ARG, "null argument");
  FX_HIP(hipSetDevice(c->device));
  FX_HIP(hipStreamSynchronize(c->stream));
  FX_HIP(hipMemcpy(out3, c->buf.counters + FX_CNT_GROUP, FX_GROUP_CLASSES * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return FX_OK;
}

// Diagnostic (-DFX_STAMPS builds): cumulative per-phase cycle counters of the ring kernel.
fx_status fx_debug_stamps(fx_ctx *c, unsigned long long *out32 /* 64 words */) {
  if (!c || !out32) return fail(FX_ERR_INVALID_ARG, "null argument");
  FX_HIP(hipSetDevice(c->device));
  FX_HIP(hipStreamSynchronize(c->stream));
  std::vector<unsigned long long> all(64 * 64);
  FX_HIP(hipMemcpy(all.data(), c->buf.stamps, all.size() * 8, hipMemcpyDeviceToHost));
  for (int k = 0; k < 64; ++k) {
    out32[k] = 0;
    for (int w = 0; w < 64; ++w) out32[k] += all[(size_t)w * 64 + k];
  }
  return FX_OK;
}

// Diagnostic (-DFX_STAMPS builds): the raw stamp words (64 x 64).
fx_status fx_debug_stamps_raw(fx_ctx *c, unsigned long long *out4096) {
  if (!c || !out4096) return fail(FX_ERR_INVALID_ARG, "null argument");
  FX_HIP(hipSetDevice(c->device));
  FX_HIP(hipStreamSynchronize(c->stream));
  FX_HIP(hipMemcpy(out4096, c->buf.stamps, 64 * 64 * 8, hipMemcpyDeviceToHost));
  return FX_OK;
}

fx_status fx_pack_keypoint_records(fx_ctx *c, void *dst_device, uint32_t rec_keypoints) {
  if (!c || !dst_device || !rec_keypoints) return fail(FX_ERR_INVALID_ARG, "null argument");
  FX_HIP(hipSetDevice(c->device));
  if (c->plan_state.last_batch) fxk_pack_kp_records(c->stream, c->dp, c->buf, c->plan_state.last_batch, dst_device, rec_keypoints);
  FX_HIP(hipGetLastError());
  return FX_OK;
}

size_t fx_keypoint_block_bytes(uint32_t max_scans, uint32_t max_total_keypoints) { return fxk_kp_block_bytes(max_scans, max_total_keypoints); }

fx_status fx_pack_keypoint_block(fx_ctx *c, void *dst_device, uint32_t max_scans, uint32_t max_total_keypoints) {
  if (!c || !dst_device || !max_scans) return fail(FX_ERR_INVALID_ARG, "null argument");
  FX_HIP(hipSetDevice(c->device));
  // a workgroup a scan up to four a CU (the block's zero tail is dealt by stride; an empty batch — kp_offset[0] is 0 — gives
  // the empty block)
  const uint32_t grid = std::max(1u, std::min(c->plan_state.last_batch, 4u * c->plan_cfg.n_cu));
  fxk_pack_kp_block(c->stream, c->dp, c->buf, c->plan_state.last_batch, dst_device, max_scans, max_total_keypoints, grid);
  FX_HIP(hipGetLastError());
  return FX_OK;
}

size_t fx_descriptor_csr_bytes(uint32_t max_rows, uint32_t capacity) { return fxk_csr_bytes(max_rows, capacity); }

fx_status fx_pack_descriptors_csr(fx_ctx *c, void *dst_device, uint32_t max_rows, uint32_t capacity) {
  if (!c || !dst_device) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (((uintptr_t)dst_device % 16) != 0) return fail(FX_ERR_INVALID_ARG, "dst must be 16-byte aligned");
  if (!csr_pool_fits(c->lim)) return fail(FX_ERR_TOO_LARGE, "max_total_keypoints * 1989 exceeds 2^32 - 1");
  FX_HIP(hipSetDevice(c->device));
  return enqueue_csr(c, c->stream, dst_device, max_rows, capacity);
}

fx_status fx_splice_blocks(fx_ctx *c, const fx_splice_source *a, const fx_splice_source *b, void *dst_kp, uint32_t dst_max_scans,
                           uint32_t dst_max_total, void *dst_csr, uint32_t dst_max_rows, uint32_t dst_cap) {
  if (!c || !a || !b || !a->kp_block_device || !b->kp_block_device || !dst_kp) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (dst_csr && (!a->csr_block_device || !b->csr_block_device))
    return fail(FX_ERR_INVALID_ARG, "a destination CSR block needs both sources' CSR blocks");
  if (!a->max_scans || !b->max_scans || !dst_max_scans) return fail(FX_ERR_INVALID_ARG, "a keypoint block of no scans");
  // the blocks' byte ranges, as their layouts give them; the sources' CSR blocks are not looked at without a destination for them
  struct Range {
    const void *p;
    size_t bytes;
  };
  const Range src[4] = {{a->kp_block_device, fxk_kp_block_bytes(a->max_scans, a->max_total_keypoints)},
                        {b->kp_block_device, fxk_kp_block_bytes(b->max_scans, b->max_total_keypoints)},
                        {dst_csr ? a->csr_block_device : nullptr, fxk_csr_bytes(a->max_rows, a->capacity)},
                        {dst_csr ? b->csr_block_device : nullptr, fxk_csr_bytes(b->max_rows, b->capacity)}};
  const Range dst[2] = {{dst_kp, fxk_kp_block_bytes(dst_max_scans, dst_max_total)}, {dst_csr, fxk_csr_bytes(dst_max_rows, dst_cap)}};
  for (const Range &r : {src[0], src[1], src[2], src[3], dst[0], dst[1]})
    if (((uintptr_t)r.p % 16) != 0) return fail(FX_ERR_INVALID_ARG, "blocks must be 16-byte aligned");
  for (const Range &d : dst)
    for (const Range &s : src)
      if (d.p && s.p && (uintptr_t)d.p < (uintptr_t)s.p + s.bytes && (uintptr_t)s.p < (uintptr_t)d.p + d.bytes)
        return fail(FX_ERR_INVALID_ARG, "a destination block overlaps a source block");
  FX_HIP(hipSetDevice(c->device));
  FX_TRY(c->splice_scratch.reserve(c, FX_SPLICE_PLAN_WORDS * sizeof(uint32_t), "splice scratch"));
  auto view = [&](const fx_splice_source &x) {
    return FxSpliceSrc{(const uint32_t *)x.kp_block_device, x.max_scans, x.max_total_keypoints, dst_csr ? (const uint32_t *)x.csr_block_device : nullptr,
                       x.max_rows, x.capacity, x.scan0, x.n_scans};
  };
  FxSpliceArgs A{};
  A.a = view(*a), A.b = view(*b);
  A.dst_kp = (uint32_t *)dst_kp, A.dst_max_scans = dst_max_scans, A.dst_max_total = dst_max_total;
  A.dst_csr = (uint32_t *)dst_csr, A.dst_max_rows = dst_max_rows, A.dst_cap = dst_cap;
  A.plan = (uint32_t *)c->splice_scratch.d;
  FX_HIP(fxk_splice(c->stream, A, 8u * c->plan_cfg.n_cu));
  return FX_OK;
}

void fx_deskew_options_default(fx_deskew_options *o) {
  if (!o) return;
  o->start_turn = 0.5, o->ref_fraction = 1.0, o->sweep_fraction = 1.0;
  o->direction = -1;
  o->source = FX_DESKEW_LINKS, o->require_flags = FX_REG_VALID, o->reserved = 0u;
}

fx_status fx_deskew_keypoint_block(fx_ctx *c, const void *src, void *dst, uint32_t max_scans, uint32_t max_total, const fx_registration *motions,
                                   uint32_t n_scans, const fx_deskew_options *opt, fx_deskew_scan *out) {
  if (!c) return fail(FX_ERR_INVALID_ARG, "null argument");
  FX_TRY(query_check(max_scans, n_scans));
  fx_deskew_options o;
  fx_deskew_options_default(&o);
  if (opt) o = *opt;
  if (o.source != FX_DESKEW_LINKS && o.source != FX_DESKEW_PER_SCAN) return fail(FX_ERR_INVALID_ARG, "source must be FX_DESKEW_LINKS or FX_DESKEW_PER_SCAN");
  if (!src || !dst || !out || (!motions && !(o.source == FX_DESKEW_LINKS && n_scans == 1u))) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (!std::isfinite(o.start_turn)) return fail(FX_ERR_INVALID_ARG, "start_turn must be finite");
  if (!(o.ref_fraction >= 0.0 && o.ref_fraction <= 1.0)) return fail(FX_ERR_INVALID_ARG, "ref_fraction must be in [0, 1]");
  if (!(o.sweep_fraction > 0.0 && o.sweep_fraction <= 1.0)) return fail(FX_ERR_INVALID_ARG, "sweep_fraction must be in (0, 1]");
  if (o.direction != 1 && o.direction != -1) return fail(FX_ERR_INVALID_ARG, "direction must be +1 or -1");
  if (o.reserved) return fail(FX_ERR_INVALID_ARG, "reserved must be 0");
  if (((uintptr_t)src % 16) != 0 || ((uintptr_t)dst % 16) != 0 || ((uintptr_t)motions % 8) != 0 || ((uintptr_t)out % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "the keypoint blocks must be 16-byte, the motion records 8-byte, out 4-byte aligned");
  const size_t bytes = fxk_kp_block_bytes(max_scans, max_total);
  if (dst != src && (uintptr_t)dst < (uintptr_t)src + bytes && (uintptr_t)src < (uintptr_t)dst + bytes)
    return fail(FX_ERR_INVALID_ARG, "dst overlaps src without being src (in place: dst == src)");
  FX_HIP(hipSetDevice(c->device));
  FxDeskewArgs A{};
  A.src = (const uint32_t *)src, A.dst = (uint32_t *)dst, A.max_scans = max_scans, A.max_total = max_total;
  A.motions = motions, A.n_scans = n_scans;
  A.start_turn = o.start_turn, A.ref_fraction = o.ref_fraction, A.sweep_fraction = o.sweep_fraction, A.direction = (double)o.direction;
  A.source = o.source, A.require_flags = o.require_flags;
  A.out = out;
  FX_HIP(fxk_deskew(c->stream, A, 8u * c->plan_cfg.n_cu));
  return FX_OK;
}

fx_status fx_get_descriptors_csr(fx_ctx *c, fx_descriptor_csr_view *out) {
  if (!c || !out) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (!c->csr_valid) return fail(FX_ERR_INVALID_ARG, "the last batch was not FX_OUT_HOST | FX_OUT_DESC_CSR");
  const uint32_t R = c->lim.max_total_keypoints;
  const size_t col = csr_col_offset(R), val = csr_val_offset(R, c->csr_cap);
  out->rows = c->csr_rows;
  out->nnz = c->csr_nnz;
  out->h_row_ptr = (const uint32_t *)(c->h_csr + 16);
  out->h_col = (const uint32_t *)(c->h_csr + col);
  out->h_val = (const float *)(c->h_csr + val);
  out->d_row_ptr = (const uint32_t *)(c->d_csr + 16);
  out->d_col = (const uint32_t *)(c->d_csr + col);
  out->d_val = (const float *)(c->d_csr + val);
  return FX_OK;
}

fx_status fx_set_descriptor_csr_capacity(fx_ctx *c, uint32_t entries) {
  if (!c) return fail(FX_ERR_INVALID_ARG, "null ctx");
  c->csr_cap_want = entries;
  c->csr_resize = c->d_csr != nullptr;
  return FX_OK;
}

void fx_match_options_default(fx_match_options *o) {
  if (!o) return;
  o->azimuth_shifts = 12u;
  o->max_dist2 = std::numeric_limits<float>::infinity();
  o->max_ratio = 1.0f;
  o->mutual = 0u;
}

fx_status fx_match_descriptors_csr(fx_ctx *c, const void *q_block, uint32_t q_max_rows, uint32_t q_cap, const void *t_block, uint32_t t_max_rows,
                                   uint32_t t_cap, const fx_match_pair *pairs, uint32_t n_pairs, const fx_match_options *opt, fx_match *out) {
  if (!c || !q_block || !t_block || (n_pairs && !pairs) || (q_max_rows && !out)) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (((uintptr_t)q_block % 16) != 0 || ((uintptr_t)t_block % 16) != 0 || ((uintptr_t)out % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "blocks must be 16-byte aligned");
  fx_match_options o;
  fx_match_options_default(&o);
  if (opt) o = *opt;
  if (o.azimuth_shifts != 12u && o.azimuth_shifts != 1u) return fail(FX_ERR_INVALID_ARG, "azimuth_shifts must be 12 or 1");
  if (o.max_dist2 != o.max_dist2 || o.max_ratio != o.max_ratio) return fail(FX_ERR_INVALID_ARG, "NaN threshold");
  FX_TRY(query_ranges_disjoint(pairs, n_pairs));
  FX_HIP(hipSetDevice(c->device));
  // work list (pair, tile of query rows) from the ranges the layouts admit — the kernel clips them to rows_stored —, and each
  // pair's slots in the mutual table
  const uint32_t tile = fxk_match_tile_rows();
  uint64_t n_items = 0, mut_n = 0;
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const uint32_t q0 = std::min(pairs[p].q_row0, q_max_rows), t0 = std::min(pairs[p].t_row0, t_max_rows);
    n_items += (std::min(pairs[p].q_rows, q_max_rows - q0) + tile - 1u) / tile;
    if (o.mutual) mut_n += std::min(pairs[p].t_rows, t_max_rows - t0);
  }
  if (n_items > 0x7fffffffull || mut_n > 0xffffffffull) return fail(FX_ERR_TOO_LARGE, "too many query tiles / train rows in the pairs");
  const bool same = q_block == t_block && q_max_rows == t_max_rows && q_cap == t_cap;
  const size_t staged = (size_t)n_pairs * sizeof(FxMatchPairDev) + (size_t)n_items * sizeof(uint2);
  const size_t off_tn = (size_t)q_max_rows * 8u, off_mut = same ? off_tn : off_tn + (size_t)t_max_rows * 8u;  // (the query norms at 0)
  FX_TRY(c->match_stage.reserve(c, staged, "match pairs staging"));
  FX_TRY(c->match_scratch.reserve(c, off_mut + (size_t)mut_n * 8u, "match scratch"));
  if (staged) {
    FxMatchPairDev *hp = (FxMatchPairDev *)c->match_stage.h;
    uint2 *hi = (uint2 *)(c->match_stage.h + (size_t)n_pairs * sizeof(FxMatchPairDev));
    uint64_t m = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) {
      const uint32_t q0 = std::min(pairs[p].q_row0, q_max_rows), t0 = std::min(pairs[p].t_row0, t_max_rows);
      hp[p] = FxMatchPairDev{pairs[p].q_row0, pairs[p].q_rows, pairs[p].t_row0, pairs[p].t_rows, (uint32_t)m, {0u, 0u, 0u}};
      if (o.mutual) m += std::min(pairs[p].t_rows, t_max_rows - t0);
      const uint32_t tiles = (std::min(pairs[p].q_rows, q_max_rows - q0) + tile - 1u) / tile;
      for (uint32_t k = 0; k < tiles; ++k) *hi++ = make_uint2(p, k);
    }
    FX_TRY(c->match_stage.upload(c, staged));
  }
  FxMatchArgs A{};
  A.q_block = (const uint32_t *)q_block, A.t_block = (const uint32_t *)t_block;
  A.q_max_rows = q_max_rows, A.q_cap = q_cap, A.t_max_rows = t_max_rows, A.t_cap = t_cap;
  A.pairs = (const FxMatchPairDev *)c->match_stage.d;
  A.items = (const uint2 *)(c->match_stage.d + (size_t)n_pairs * sizeof(FxMatchPairDev));
  A.q_norm = (const double *)c->match_scratch.d, A.t_norm = same ? A.q_norm : (const double *)(c->match_scratch.d + off_tn);
  A.mut = (unsigned long long *)(c->match_scratch.d + off_mut);
  A.out = out;
  A.max_dist2 = o.max_dist2, A.max_ratio = o.max_ratio, A.mutual = o.mutual ? 1u : 0u;
  FX_HIP(fxk_match(c->stream, A, (uint32_t)n_items, (uint32_t)mut_n, o.azimuth_shifts));
  return FX_OK;
}

void fx_register_options_default(fx_register_options *o) {
  if (!o) return;
  o->inlier_dist = 0.30f;
  o->min_baseline = 2.0f;
  o->hyp_corr = 64u;
  o->min_inliers = 3u;
  o->require_flags = FX_MATCH_ACCEPTED;
}

fx_status fx_register_matches(fx_ctx *c, const void *q_kp, uint32_t q_max_scans, uint32_t q_max_total, const void *t_kp, uint32_t t_max_scans,
                              uint32_t t_max_total, const fx_match *matches, uint32_t q_max_rows, const fx_match_pair *pairs, uint32_t n_pairs,
                              const fx_register_options *opt, fx_registration *out, uint32_t *inlier) {
  if (!c || !q_kp || !t_kp || (q_max_rows && !matches) || (n_pairs && (!pairs || !out))) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (!q_max_scans || !t_max_scans) return fail(FX_ERR_INVALID_ARG, "a keypoint block of no scans");
  if (((uintptr_t)q_kp % 16) != 0 || ((uintptr_t)t_kp % 16) != 0 || ((uintptr_t)matches % 4) != 0 || ((uintptr_t)out % 8) != 0 ||
      ((uintptr_t)inlier % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "keypoint blocks must be 16-byte, the records 8-byte aligned");
  fx_register_options o;
  fx_register_options_default(&o);
  if (opt) o = *opt;
  if (!(o.inlier_dist > 0.f) || !std::isfinite(o.inlier_dist) || !(o.min_baseline > 0.f) || !std::isfinite(o.min_baseline))
    return fail(FX_ERR_INVALID_ARG, "inlier_dist and min_baseline must be finite and positive");
  if (o.hyp_corr < 2u || o.hyp_corr > 128u) return fail(FX_ERR_INVALID_ARG, "hyp_corr must be 2..128");
  if (o.min_inliers < 2u) return fail(FX_ERR_INVALID_ARG, "min_inliers must be at least 2");
  FX_TRY(query_ranges_disjoint(pairs, n_pairs));
  FX_HIP(hipSetDevice(c->device));
  const size_t staged = (size_t)n_pairs * sizeof(fx_match_pair);
  FX_TRY(c->reg_stage.reserve(c, staged, "register pairs staging"));
  if (staged) std::memcpy(c->reg_stage.h, pairs, staged);
  FX_TRY(c->reg_stage.upload(c, staged));
  FxRegisterArgs A{};
  A.q_kp = (const uint32_t *)q_kp, A.t_kp = (const uint32_t *)t_kp;
  A.q_max_scans = q_max_scans, A.q_max_total = q_max_total, A.t_max_scans = t_max_scans, A.t_max_total = t_max_total;
  A.matches = matches, A.q_max_rows = q_max_rows;
  A.pairs = c->reg_stage.d, A.out = out, A.inlier = inlier;
  A.inlier_dist = o.inlier_dist, A.min_baseline = o.min_baseline;
  A.hyp_corr = o.hyp_corr, A.min_inliers = o.min_inliers, A.require_flags = o.require_flags;
  FX_HIP(fxk_register(c->stream, A, n_pairs));
  return FX_OK;
}

void fx_track_options_default(fx_track_options *o) {
  if (!o) return;
  o->min_obs = 2u;
  o->reserved = 0u;
}

fx_status fx_track_landmarks(fx_ctx *c, const void *kp, uint32_t max_scans, uint32_t max_total, const fx_match *matches, const uint32_t *inlier,
                             uint32_t q_max_rows, const fx_registration *reg, uint32_t n_scans, const fx_pose *init, const fx_track_options *opt,
                             fx_pose *poses, int32_t *landmark_of_row, uint32_t *obs_row, fx_landmark *landmarks, uint32_t max_landmarks,
                             fx_track_header *header) {
  if (!c) return fail(FX_ERR_INVALID_ARG, "null argument");
  FX_TRY(query_check(max_scans, n_scans));
  if (!kp || !poses || !header || (q_max_rows && (!matches || !inlier || !landmark_of_row || !obs_row)) || (n_scans > 1u && !reg) ||
      (max_landmarks && !landmarks))
    return fail(FX_ERR_INVALID_ARG, "null argument");
  if (((uintptr_t)kp % 16) != 0 || ((uintptr_t)matches % 4) != 0 || ((uintptr_t)inlier % 4) != 0 || ((uintptr_t)reg % 8) != 0 ||
      ((uintptr_t)poses % 8) != 0 || ((uintptr_t)landmark_of_row % 4) != 0 || ((uintptr_t)obs_row % 4) != 0 || ((uintptr_t)landmarks % 8) != 0 ||
      ((uintptr_t)header % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "the keypoint block must be 16-byte, the records 8-byte, the words 4-byte aligned");
  fx_track_options o;
  fx_track_options_default(&o);
  if (opt) o = *opt;
  if (!o.min_obs) return fail(FX_ERR_INVALID_ARG, "min_obs must be at least 1");
  FxTrackArgs A{};
  A.init[0] = 1.0;
  if (init) {
    A.init[0] = init->c, A.init[1] = init->s, A.init[2] = init->tx, A.init[3] = init->ty, A.init[4] = init->tz;
    for (double v : A.init)
      if (!std::isfinite(v)) return fail(FX_ERR_INVALID_ARG, "init_pose must be finite");
  }
  FX_HIP(hipSetDevice(c->device));
  {  // the scratch arrays, [q_max_rows] each; the two (root, depth) buffers first: they are 8-byte words
    const size_t n = q_max_rows, n_blocks = (n + fxk_track_wg_rows() - 1) / fxk_track_wg_rows();
    FX_TRY(c->track_scratch.reserve(c, (11 * n + 2 * n_blocks + 4) * sizeof(uint32_t), "track scratch"));
    uint32_t *w = (uint32_t *)c->track_scratch.d;
    A.jump[0] = (uint2 *)w, A.jump[1] = (uint2 *)(w + 2 * n);
    w += 4 * n;
    A.scan_of = w, A.child = w + n, A.prop = (int32_t *)(w + 2 * n), A.len = w + 3 * n, A.lm_id = (int32_t *)(w + 4 * n), A.obs0 = w + 5 * n,
    A.lm_root = w + 6 * n;
    A.bsum = w + 7 * n;
    A.counters = A.bsum + 2 * n_blocks;
  }
  query_args(&A.K, kp, max_scans, max_total, n_scans, q_max_rows);
  A.matches = matches, A.inlier = inlier;
  A.reg = reg, A.min_obs = o.min_obs, A.max_landmarks = max_landmarks;
  A.poses = poses, A.landmark_of_row = landmark_of_row, A.obs_row = obs_row, A.landmarks = landmarks, A.header = header;
  FX_HIP(fxk_track(c->stream, A));
  return FX_OK;
}

fx_status fx_map_create(fx_ctx *c, uint32_t max_landmarks, uint32_t max_carry_rows, fx_map **out) {
  if (!c || !out) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (!max_landmarks) return fail(FX_ERR_INVALID_ARG, "max_landmarks must be at least 1");
  FX_HIP(hipSetDevice(c->device));
  // header (88 -> 96), state words, records, accumulators, the carry scan's rows, the carry table (its bytes rounded up to 16), the
  // alias table: all 16-byte aligned
  const size_t carry = std::max((size_t)max_carry_rows, (size_t)1);
  const size_t o_st = 96, o_rec = o_st + FX_MAP_ST_WORDS * 4, o_acc = o_rec + (size_t)max_landmarks * sizeof(fx_map_landmark),
               o_kp = o_acc + (size_t)max_landmarks * FX_MAP_ACC * sizeof(double), o_carry = o_kp + carry * 16, o_alias = o_carry + ((carry * 4 + 15) & ~(size_t)15),
               bytes = o_alias + (size_t)max_landmarks * 4;
  void *d = nullptr;
  hipError_t e = hipMalloc(&d, bytes);
  if (e != hipSuccess) return fail(FX_ERR_OOM, std::string("map (") + std::to_string(bytes) + "): " + hipGetErrorString(e));
  fx_map *m = new fx_map;
  m->ctx = c, m->device = c->device, m->d = (uint8_t *)d;
  m->a.header = m->d, m->a.st = (uint32_t *)(m->d + o_st), m->a.records = m->d + o_rec, m->a.acc = (double *)(m->d + o_acc);
  m->a.carry_kp = (uint4 *)(m->d + o_kp), m->a.carry = (int32_t *)(m->d + o_carry), m->a.alias = (int32_t *)(m->d + o_alias);
  m->a.cap = max_landmarks, m->a.max_carry = max_carry_rows;
  e = hipMemsetAsync(d, 0, bytes, c->stream);
  if (e == hipSuccess) e = fxk_map_reset(c->stream, m->a);
  if (e != hipSuccess) {
    (void)hipFree(d);
    delete m;
    return fail(FX_ERR_HIP, std::string("map reset: ") + hipGetErrorString(e));
  }
  *out = m;
  return FX_OK;
}

void fx_map_destroy(fx_map *m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  (void)hipFree(m->d);  // (waits for the device: nothing in flight reads the map afterwards)
  delete m;
}

fx_status fx_map_reset(fx_ctx *c, fx_map *m) {
  FX_TRY(map_call_check(c, m));
  FX_HIP(hipSetDevice(c->device));
  FX_HIP(fxk_map_reset(c->stream, m->a));
  return FX_OK;
}

fx_status fx_map_update(fx_ctx *c, fx_map *m, const void *kp, uint32_t max_scans, uint32_t max_total, const fx_pose *poses,
                        const int32_t *landmark_of_row, const uint32_t *obs_row, uint32_t q_max_rows, const fx_landmark *landmarks,
                        uint32_t max_landmarks, const fx_track_header *track_header, uint32_t flags, int32_t *map_id_of_row) {
  const bool tables = !(q_max_rows && (!landmark_of_row || !obs_row)) && !(max_landmarks && !landmarks);
  FX_TRY(map_call_check(c, m, kp && poses && track_header && tables));
  if (flags & ~FX_MAP_OVERLAP) return fail(FX_ERR_INVALID_ARG, "unknown flags (only FX_MAP_OVERLAP is defined)");
  if (((uintptr_t)kp % 16) != 0 || ((uintptr_t)poses % 8) != 0 || ((uintptr_t)landmark_of_row % 4) != 0 || ((uintptr_t)obs_row % 4) != 0 ||
      ((uintptr_t)landmarks % 8) != 0 || ((uintptr_t)track_header % 4) != 0 || ((uintptr_t)map_id_of_row % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "the keypoint block must be 16-byte, the records 8-byte, the words 4-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  const size_t n_blocks = ((size_t)max_landmarks + fxk_map_wg() - 1) / fxk_map_wg();
  FX_TRY(c->map_scratch.reserve(c, ((size_t)max_landmarks + 2 * n_blocks) * sizeof(uint32_t), "map scratch"));
  FxMapArgs A = m->a;
  A.id_of_lm = (int32_t *)c->map_scratch.d, A.bsum = (uint32_t *)c->map_scratch.d + max_landmarks;
  A.kp = (const uint32_t *)kp, A.max_scans = max_scans, A.max_total = max_total;
  A.poses = poses, A.landmark_of_row = landmark_of_row, A.obs_row = obs_row, A.q_max_rows = q_max_rows;
  A.landmarks = landmarks, A.max_landmarks = max_landmarks, A.track_header = track_header;
  A.flags = flags, A.map_id_of_row = map_id_of_row;
  FX_HIP(fxk_map_update(c->stream, A));
  return FX_OK;
}

fx_status fx_map_get(fx_map *m, const fx_map_header **header, const fx_map_landmark **landmarks) {
  if (!m) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (header) *header = (const fx_map_header *)m->a.header;
  if (landmarks) *landmarks = (const fx_map_landmark *)m->a.records;
  return FX_OK;
}

fx_status fx_map_read_header(fx_ctx *c, fx_map *m, fx_map_header *out) {
  FX_TRY(map_call_check(c, m, out != nullptr));
  FX_HIP(hipSetDevice(c->device));
  FX_HIP(hipMemcpyAsync(out, m->a.header, sizeof(fx_map_header), hipMemcpyDeviceToHost, c->stream));
  FX_HIP(hipStreamSynchronize(c->stream));
  return FX_OK;
}

fx_status fx_map_read_landmarks(fx_ctx *c, fx_map *m, uint32_t first, uint32_t count, fx_map_landmark *out) {
  FX_TRY(map_call_check(c, m, !count || out));
  if (first > m->a.cap || count > m->a.cap - first) return fail(FX_ERR_INVALID_ARG, "records outside the map's max_landmarks");
  FX_HIP(hipSetDevice(c->device));
  if (count)
    FX_HIP(hipMemcpyAsync(out, (const fx_map_landmark *)m->a.records + first, (size_t)count * sizeof(fx_map_landmark), hipMemcpyDeviceToHost,
                          c->stream));
  FX_HIP(hipStreamSynchronize(c->stream));
  return FX_OK;
}

void fx_map_merge_options_default(fx_map_merge_options *o) {
  if (!o) return;
  o->merge_dist = 0.30f;
  o->max_gap_scans = 64;
}

fx_status fx_map_merge(fx_ctx *c, fx_map *m, const fx_map_merge_options *opt, fx_map_merge_result *result) {
  FX_TRY(map_call_check(c, m));
  fx_map_merge_options o;
  fx_map_merge_options_default(&o);
  if (opt) o = *opt;
  if (!(std::isfinite(o.merge_dist) && o.merge_dist > 0.f)) return fail(FX_ERR_INVALID_ARG, "merge_dist must be finite and positive");
  if (!o.max_gap_scans) return fail(FX_ERR_INVALID_ARG, "max_gap_scans must be at least 1");
  if (((uintptr_t)result % 4) != 0) return fail(FX_ERR_INVALID_ARG, "the result must be 4-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  FxMapMergeArgs A{};
  map_grid_view(&A, m, (double)o.merge_dist);
  A.max_gap = o.max_gap_scans;
  A.result = (uint32_t *)result;
  FX_MAP_RUN(fxk_map_merge, "map merge scratch");
  return FX_OK;
}

void fx_localize_options_default(fx_localize_options *o) {
  if (!o) return;
  o->search_dist = 2.0f;
  o->inlier_dist = 0.30f;
  o->min_baseline = 2.0f;
  o->hyp_corr = 64u;
  o->min_inliers = 3u;
  o->min_landmark_obs = 2u;
  o->segment = FX_LOC_LAST_SEGMENT;
  o->reserved = 0u;
}

fx_status fx_map_localize(fx_ctx *c, fx_map *m, const void *kp, uint32_t max_scans, uint32_t max_total, const fx_pose *priors, uint32_t n_scans,
                          uint32_t q_max_rows, const fx_localize_options *opt, fx_localization *out, int32_t *map_id_of_row,
                          int32_t *nearest_of_row) {
  FX_TRY(map_call_check(c, m));
  FX_TRY(query_check(max_scans, n_scans));
  if (!kp || !priors || !out || (q_max_rows && !map_id_of_row)) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (((uintptr_t)kp % 16) != 0 || ((uintptr_t)priors % 8) != 0 || ((uintptr_t)out % 8) != 0 || ((uintptr_t)map_id_of_row % 4) != 0 ||
      ((uintptr_t)nearest_of_row % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "the keypoint block must be 16-byte, the records 8-byte, the words 4-byte aligned");
  fx_localize_options o;
  fx_localize_options_default(&o);
  if (opt) o = *opt;
  FX_TRY(consensus_options_check(o));
  if (o.reserved) return fail(FX_ERR_INVALID_ARG, "reserved must be 0");
  FX_HIP(hipSetDevice(c->device));
  FxMapLocalizeArgs A{};
  map_grid_view(&A.G, m, (double)o.search_dist);
  query_args(&A.K, kp, max_scans, max_total, n_scans, q_max_rows);
  A.priors = priors;
  A.inlier_dist = o.inlier_dist, A.min_baseline = o.min_baseline;
  A.hyp_corr = o.hyp_corr, A.min_inliers = o.min_inliers, A.min_landmark_obs = o.min_landmark_obs, A.segment = o.segment;
  A.out = out, A.map_id_of_row = map_id_of_row, A.nearest_of_row = nearest_of_row;
  FX_MAP_RUN(fxk_map_localize, "map localize scratch");
  return FX_OK;
}

void fx_follow_options_default(fx_follow_options *o) {
  if (!o) return;
  fx_localize_options_default(&o->loc);
  o->loc.segment = FX_LOC_ANY_SEGMENT;
  o->chain_scans = 0u, o->require_flags = FX_REG_VALID, o->max_lost = 5u, o->reserved = 0u;
}

fx_status fx_map_follow(fx_ctx *c, fx_map *m, const void *kp, uint32_t max_scans, uint32_t max_total, const fx_registration *links,
                        const fx_pose *starts, uint32_t n_scans, uint32_t q_max_rows, const fx_follow_options *opt, fx_localization *out,
                        fx_follow_scan *follow, fx_pose *poses, int32_t *map_id_of_row, int32_t *nearest_of_row) {
  FX_TRY(map_call_check(c, m));
  FX_TRY(query_check(max_scans, n_scans));
  fx_follow_options o;
  fx_follow_options_default(&o);
  if (opt) o = *opt;
  const uint32_t chain = o.chain_scans && o.chain_scans < n_scans ? o.chain_scans : n_scans;
  if (!kp || !starts || !out || !follow || (q_max_rows && !map_id_of_row) || (!links && chain > 1u)) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (((uintptr_t)kp % 16) != 0 || ((uintptr_t)links % 8) != 0 || ((uintptr_t)starts % 8) != 0 || ((uintptr_t)out % 8) != 0 ||
      ((uintptr_t)follow % 8) != 0 || ((uintptr_t)poses % 8) != 0 || ((uintptr_t)map_id_of_row % 4) != 0 || ((uintptr_t)nearest_of_row % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "the keypoint block must be 16-byte, the records 8-byte, the words 4-byte aligned");
  FX_TRY(consensus_options_check(o.loc));
  if (o.loc.reserved || o.reserved) return fail(FX_ERR_INVALID_ARG, "reserved must be 0");
  if (!o.max_lost) return fail(FX_ERR_INVALID_ARG, "max_lost must be at least 1");
  if (o.require_flags & ~(FX_REG_VALID | FX_REG_TRUNCATED | FX_REG_NO_HYPOTHESIS))
    return fail(FX_ERR_INVALID_ARG, "unknown require_flags bits (only the FX_REG_* flags are defined)");
  FX_HIP(hipSetDevice(c->device));
  FxMapFollowArgs A{};
  map_grid_view(&A.L.G, m, (double)o.loc.search_dist);
  query_args(&A.L.K, kp, max_scans, max_total, n_scans, q_max_rows);
  A.L.inlier_dist = o.loc.inlier_dist, A.L.min_baseline = o.loc.min_baseline;
  A.L.hyp_corr = o.loc.hyp_corr, A.L.min_inliers = o.loc.min_inliers, A.L.min_landmark_obs = o.loc.min_landmark_obs, A.L.segment = o.loc.segment;
  A.L.out = out, A.L.map_id_of_row = map_id_of_row, A.L.nearest_of_row = nearest_of_row;
  A.links = links, A.starts = starts;
  A.chain_scans = chain, A.n_chains = (n_scans + chain - 1u) / chain;
  A.require_flags = o.require_flags, A.max_lost = o.max_lost;
  A.follow = follow, A.poses = poses;
  FX_MAP_RUN(fxk_map_follow, "map follow scratch");
  return FX_OK;
}

void fx_relocalize_options_default(fx_relocalize_options *o) {
  if (!o) return;
  o->inlier_dist = 0.30f;
  o->pair_tol = 0.30f;
  o->min_baseline = 2.0f;
  o->max_baseline = 60.0f;
  o->max_seeds = 16u;
  o->min_inliers = 4u;
  o->min_margin = 1u;
  o->min_landmark_obs = 2u;
  o->segment = FX_LOC_ANY_SEGMENT;
  o->reserved = 0u;
}

fx_status fx_map_relocalize(fx_ctx *c, fx_map *m, const void *kp, uint32_t max_scans, uint32_t max_total, uint32_t n_scans, uint32_t q_max_rows,
                            const fx_relocalize_options *opt, fx_relocalization *out, int32_t *map_id_of_row) {
  FX_TRY(map_call_check(c, m));
  FX_TRY(query_check(max_scans, n_scans));
  if (!kp || !out || (q_max_rows && !map_id_of_row)) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (((uintptr_t)kp % 16) != 0 || ((uintptr_t)out % 8) != 0 || ((uintptr_t)map_id_of_row % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "the keypoint block must be 16-byte, the records 8-byte, the words 4-byte aligned");
  fx_relocalize_options o;
  fx_relocalize_options_default(&o);
  if (opt) o = *opt;
  FX_TRY(constellation_options_check(o));
  if (o.reserved) return fail(FX_ERR_INVALID_ARG, "reserved must be 0");
  FX_HIP(hipSetDevice(c->device));
  FxMapRelocalizeArgs A{};
  constellation_args(&A, m, o);
  query_args(&A.K, kp, max_scans, max_total, n_scans, q_max_rows);
  A.segment = o.segment;
  A.out = out, A.map_id_of_row = map_id_of_row;
  FX_MAP_RUN(fxk_map_relocalize, "map relocalize scratch");
  return FX_OK;
}

void fx_map_observe_options_default(fx_map_observe_options *o) {
  if (!o) return;
  o->gate_dist = 0.30f;
  o->require_flags = FX_LOC_VALID;
  o->mode = FX_OBS_APPLY;
  o->reserved = 0u;
}

fx_status fx_map_observe(fx_ctx *c, fx_map *m, const void *kp, uint32_t max_scans, uint32_t max_total, const fx_localization *loc, uint32_t n_scans,
                         const int32_t *map_id_of_row, uint32_t q_max_rows, const fx_map_observe_options *opt, fx_map_observe_result *result,
                         uint32_t *gained_of_landmark, int32_t *observed_id_of_row) {
  FX_TRY(map_call_check(c, m, kp && loc && !(q_max_rows && !map_id_of_row)));
  FX_TRY(query_check(max_scans, n_scans));
  fx_map_observe_options o;
  fx_map_observe_options_default(&o);
  if (opt) o = *opt;
  if (!(std::isfinite(o.gate_dist) && o.gate_dist > 0.f)) return fail(FX_ERR_INVALID_ARG, "gate_dist must be finite and positive");
  FX_TRY(loc_flags_check(o.require_flags));
  if (o.mode != FX_OBS_APPLY && o.mode != FX_OBS_DRY_RUN) return fail(FX_ERR_INVALID_ARG, "unknown mode (FX_OBS_APPLY or FX_OBS_DRY_RUN)");
  if (o.reserved) return fail(FX_ERR_INVALID_ARG, "reserved must be 0");
  if (((uintptr_t)kp % 16) != 0 || ((uintptr_t)loc % 8) != 0 || ((uintptr_t)map_id_of_row % 4) != 0 || ((uintptr_t)result % 4) != 0 ||
      ((uintptr_t)gained_of_landmark % 4) != 0 || ((uintptr_t)observed_id_of_row % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "the keypoint block must be 16-byte, the records 8-byte, the words 4-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  FxMapObserveArgs A{};
  A.header = m->a.header, A.records = m->a.records, A.acc = m->a.acc, A.alias = m->a.alias, A.cap = m->a.cap;
  query_args(&A.K, kp, max_scans, max_total, n_scans, q_max_rows);
  A.loc = loc, A.map_id_of_row = map_id_of_row;
  A.gd2 = (double)o.gate_dist * (double)o.gate_dist, A.require_flags = o.require_flags, A.mode = o.mode;
  A.result = (uint32_t *)result, A.gained = gained_of_landmark, A.observed = observed_id_of_row;
  FX_MAP_RUN(fxk_map_observe, "map observe scratch");
  return FX_OK;
}

void fx_map_expect_options_default(fx_map_expect_options *o) {
  if (!o) return;
  o->x_min = 1.f, o->x_max = 74.f, o->y_min = -29.f, o->y_max = 29.f;
  o->min_range = 2.0f, o->max_range = 60.0f;
  o->shadow_width = 0.5f;
  o->require_flags = FX_LOC_VALID;
  o->min_landmark_obs = 2u;
  o->segment = FX_LOC_ANY_SEGMENT;
  o->mode = FX_EXPECT_WRITE;
  o->reserved = 0u;
}

void fx_map_expect_options_from_params(const fx_params *p, float margin, fx_map_expect_options *o) {
  if (!o) return;
  fx_map_expect_options_default(o);
  if (!p) return;
  o->x_min = (float)p->x_min + margin, o->x_max = (float)p->x_max - margin;
  o->y_min = (float)p->y_min + margin, o->y_max = (float)p->y_max - margin;
}

fx_status fx_map_expect(fx_ctx *c, fx_map *m, const void *kp, uint32_t max_scans, uint32_t max_total, const fx_localization *loc, uint32_t n_scans,
                        const int32_t *map_id_of_row, uint32_t q_max_rows, const fx_map_expect_options *opt, fx_map_expect_result *result,
                        uint32_t *expected_of_landmark, uint32_t *seen_of_landmark) {
  FX_TRY(map_call_check(c, m, kp && loc && !(q_max_rows && !map_id_of_row) && expected_of_landmark && seen_of_landmark));
  FX_TRY(query_check(max_scans, n_scans));
  fx_map_expect_options o;
  fx_map_expect_options_default(&o);
  if (opt) o = *opt;
  if (!(o.x_min <= o.x_max) || !(o.y_min <= o.y_max)) return fail(FX_ERR_INVALID_ARG, "the box needs x_min <= x_max and y_min <= y_max, and no NaN");
  if (!(std::isfinite(o.min_range) && o.min_range >= 0.f)) return fail(FX_ERR_INVALID_ARG, "min_range must be finite and not negative");
  if (!(std::isfinite(o.max_range) && o.max_range > 0.f && o.max_range >= o.min_range))
    return fail(FX_ERR_INVALID_ARG, "max_range must be finite, positive and at least min_range");
  if (!(std::isfinite(o.shadow_width) && o.shadow_width >= 0.f)) return fail(FX_ERR_INVALID_ARG, "shadow_width must be finite and not negative");
  FX_TRY(loc_flags_check(o.require_flags));
  if (!o.min_landmark_obs) return fail(FX_ERR_INVALID_ARG, "min_landmark_obs must be at least 1");
  if (o.mode != FX_EXPECT_WRITE && o.mode != FX_EXPECT_ADD) return fail(FX_ERR_INVALID_ARG, "unknown mode (FX_EXPECT_WRITE or FX_EXPECT_ADD)");
  if (o.reserved) return fail(FX_ERR_INVALID_ARG, "reserved must be 0");
  if (((uintptr_t)kp % 16) != 0 || ((uintptr_t)loc % 8) != 0 || ((uintptr_t)map_id_of_row % 4) != 0 || ((uintptr_t)result % 4) != 0 ||
      ((uintptr_t)expected_of_landmark % 4) != 0 || ((uintptr_t)seen_of_landmark % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "the keypoint block must be 16-byte, the records 8-byte, the words 4-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  FxMapExpectArgs A{};
  map_grid_view(&A.G, m, (double)o.max_range);
  query_args(&A.K, kp, max_scans, max_total, n_scans, q_max_rows);
  A.loc = loc, A.map_id_of_row = map_id_of_row;
  A.x_min = (double)o.x_min, A.x_max = (double)o.x_max, A.y_min = (double)o.y_min, A.y_max = (double)o.y_max;
  A.lo2 = (double)o.min_range * (double)o.min_range, A.hi2 = (double)o.max_range * (double)o.max_range;
  A.w2 = (double)o.shadow_width * (double)o.shadow_width;
  A.require_flags = o.require_flags, A.min_landmark_obs = o.min_landmark_obs, A.segment = o.segment, A.mode = o.mode;
  A.result = (uint32_t *)result, A.expected = expected_of_landmark, A.seen = seen_of_landmark;
  FX_MAP_RUN(fxk_map_expect, "map expect scratch");
  return FX_OK;
}

void fx_map_discover_options_default(fx_map_discover_options *o) {
  if (!o) return;
  o->known_dist = 1.0f;
  o->join_dist = 0.30f;
  o->min_obs = 3u;
  o->require_flags = FX_LOC_VALID;
  o->segment = FX_LOC_LAST_SEGMENT;
  o->mode = FX_DISC_APPLY;
  o->reserved[0] = o->reserved[1] = 0u;
}

fx_status fx_map_discover(fx_ctx *c, fx_map *m, const void *kp, uint32_t max_scans, uint32_t max_total, const fx_localization *loc, uint32_t n_scans,
                          const int32_t *map_id_of_row, uint32_t q_max_rows, const fx_map_discover_options *opt, fx_map_discover_result *result,
                          int32_t *new_id_of_row) {
  FX_TRY(map_call_check(c, m, kp && loc && !(q_max_rows && !map_id_of_row)));
  FX_TRY(query_check(max_scans, n_scans));
  fx_map_discover_options o;
  fx_map_discover_options_default(&o);
  if (opt) o = *opt;
  if (!(std::isfinite(o.known_dist) && o.known_dist > 0.f)) return fail(FX_ERR_INVALID_ARG, "known_dist must be finite and positive");
  if (!(std::isfinite(o.join_dist) && o.join_dist > 0.f)) return fail(FX_ERR_INVALID_ARG, "join_dist must be finite and positive");
  if ((double)o.known_dist < 2.0 * (double)o.join_dist)
    return fail(FX_ERR_INVALID_ARG, "known_dist must be at least twice join_dist (a second call must find the rows of a new landmark known)");
  if (!o.min_obs) return fail(FX_ERR_INVALID_ARG, "min_obs must be at least 1");
  FX_TRY(loc_flags_check(o.require_flags));
  if (o.segment == FX_LOC_ANY_SEGMENT) return fail(FX_ERR_INVALID_ARG, "segment must be a segment number or FX_LOC_LAST_SEGMENT: a new landmark has one segment");
  if (o.mode != FX_DISC_APPLY && o.mode != FX_DISC_DRY_RUN) return fail(FX_ERR_INVALID_ARG, "unknown mode (FX_DISC_APPLY or FX_DISC_DRY_RUN)");
  if (o.reserved[0] || o.reserved[1]) return fail(FX_ERR_INVALID_ARG, "reserved must be 0");
  if (((uintptr_t)kp % 16) != 0 || ((uintptr_t)loc % 8) != 0 || ((uintptr_t)map_id_of_row % 4) != 0 || ((uintptr_t)result % 4) != 0 ||
      ((uintptr_t)new_id_of_row % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "the keypoint block must be 16-byte, the records 8-byte, the words 4-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  FxMapDiscoverArgs A{};
  map_grid_view(&A.G, m, (double)o.known_dist);
  // the grid over the free rows: no map behind it (the launches read the staged points), one item a row at the most
  const double jd = (double)o.join_dist;
  A.F.cap = q_max_rows, A.F.table = fxk_map_merge_table(q_max_rows);
  A.F.md2 = jd * jd, A.F.inv_edge = 1.0 / (jd * (1.0 + 1.0 / 256.0));
  A.header = m->a.header, A.records = m->a.records, A.acc = m->a.acc;
  query_args(&A.K, kp, max_scans, max_total, n_scans, q_max_rows);
  A.loc = loc, A.map_id_of_row = map_id_of_row;
  A.min_obs = o.min_obs, A.require_flags = o.require_flags, A.segment = o.segment, A.mode = o.mode;
  A.result = (uint32_t *)result, A.new_id = new_id_of_row;
  FX_MAP_RUN(fxk_map_discover, "map discover scratch");
  return FX_OK;
}

fx_status fx_map_get_alias(fx_map *m, const int32_t **alias) {
  if (!m || !alias) return fail(FX_ERR_INVALID_ARG, "null argument");
  *alias = m->a.alias;
  return FX_OK;
}

fx_status fx_map_read_alias(fx_ctx *c, fx_map *m, uint32_t first, uint32_t count, int32_t *out) {
  FX_TRY(map_call_check(c, m, !count || out));
  if (first > m->a.cap || count > m->a.cap - first) return fail(FX_ERR_INVALID_ARG, "entries outside the map's max_landmarks");
  FX_HIP(hipSetDevice(c->device));
  if (count) FX_HIP(hipMemcpyAsync(out, m->a.alias + first, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  FX_HIP(hipStreamSynchronize(c->stream));
  return FX_OK;
}

void fx_map_compact_options_default(fx_map_compact_options *o) {
  if (!o) return;
  o->min_obs = 1;
  o->min_age_scans = 64;
}

fx_status fx_map_compact(fx_ctx *c, fx_map *m, const fx_map_compact_options *opt, int32_t *remap, fx_map_compact_result *result) {
  FX_TRY(map_call_check(c, m));
  fx_map_compact_options o;
  fx_map_compact_options_default(&o);
  if (opt) o = *opt;
  if (!o.min_obs) return fail(FX_ERR_INVALID_ARG, "min_obs must be at least 1");
  if (((uintptr_t)remap % 4) != 0 || ((uintptr_t)result % 4) != 0) return fail(FX_ERR_INVALID_ARG, "remap and the result must be 4-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  FxMapCompactArgs A{};
  map_compact_view(&A, m);
  A.min_obs = o.min_obs, A.min_age = o.min_age_scans;
  A.remap = remap, A.result = (uint32_t *)result;
  FX_MAP_RUN(fxk_map_compact, "map compact scratch");
  return FX_OK;
}

void fx_map_retire_options_default(fx_map_retire_options *o) {
  if (!o) return;
  o->min_expected = 16u;
  o->seen_num = 1u, o->seen_den = 8u;
  o->mode = FX_RETIRE_APPLY;
  o->reserved[0] = o->reserved[1] = 0u;
}

fx_status fx_map_retire(fx_ctx *c, fx_map *m, uint32_t *expected_of_landmark, uint32_t *seen_of_landmark, const fx_map_retire_options *opt,
                        int32_t *remap, uint8_t *retired_of_landmark, fx_map_retire_result *result) {
  FX_TRY(map_call_check(c, m, expected_of_landmark && seen_of_landmark));
  fx_map_retire_options o;
  fx_map_retire_options_default(&o);
  if (opt) o = *opt;
  if (!o.min_expected) return fail(FX_ERR_INVALID_ARG, "min_expected must be at least 1");
  if (!o.seen_den || !o.seen_num || o.seen_num > o.seen_den) return fail(FX_ERR_INVALID_ARG, "the ratio needs 1 <= seen_num <= seen_den");
  if (o.mode != FX_RETIRE_APPLY && o.mode != FX_RETIRE_DRY_RUN) return fail(FX_ERR_INVALID_ARG, "unknown mode (FX_RETIRE_APPLY or FX_RETIRE_DRY_RUN)");
  if (o.reserved[0] || o.reserved[1]) return fail(FX_ERR_INVALID_ARG, "reserved must be 0");
  if (((uintptr_t)expected_of_landmark % 4) != 0 || ((uintptr_t)seen_of_landmark % 4) != 0 || ((uintptr_t)remap % 4) != 0 ||
      ((uintptr_t)result % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "the counters, remap and the result must be 4-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  fx_map_compact_options k;
  fx_map_compact_options_default(&k);  // min_obs 1: the compaction itself drops nothing live
  FxMapCompactArgs A{};
  map_compact_view(&A, m);
  A.min_obs = k.min_obs, A.min_age = k.min_age_scans;
  A.remap = remap, A.result = (uint32_t *)result;
  A.expected = expected_of_landmark, A.seen = seen_of_landmark;
  A.min_expected = o.min_expected, A.seen_num = o.seen_num, A.seen_den = o.seen_den, A.dry_run = o.mode == FX_RETIRE_DRY_RUN ? 1u : 0u;
  A.retired = retired_of_landmark;
  FX_MAP_RUN(fxk_map_compact, "map retire scratch");
  return FX_OK;
}

void fx_map_join_options_default(fx_map_join_options *o) {
  if (!o) return;
  o->search_dist = 2.0f;
  o->inlier_dist = 0.30f;
  o->min_baseline = 2.0f;
  o->hyp_corr = 64u;
  o->min_inliers = 3u;
  o->min_landmark_obs = 2u;
  o->mode = FX_JOIN_FIT;
  o->reserved = 0u;
}

fx_status fx_map_join_segments(fx_ctx *c, fx_map *m, uint32_t src, uint32_t dst, const fx_pose *prior_host, const double *prior_device,
                               const fx_map_join_options *opt, fx_map_join_result *result, int32_t *match_of_landmark) {
  FX_TRY(map_call_check(c, m));
  if (src == dst) return fail(FX_ERR_INVALID_ARG, "src_segment and dst_segment must differ (" + std::to_string(src) + ")");
  FX_TRY(prior_check(prior_host, prior_device));
  fx_map_join_options o;
  fx_map_join_options_default(&o);
  if (opt) o = *opt;
  FX_TRY(consensus_options_check(o));
  if (o.mode > FX_JOIN_DRY_RUN) return fail(FX_ERR_INVALID_ARG, "mode must be FX_JOIN_FIT, FX_JOIN_GIVEN or FX_JOIN_DRY_RUN");
  if (o.reserved) return fail(FX_ERR_INVALID_ARG, "reserved must be 0");
  if (((uintptr_t)prior_device % 8) != 0 || ((uintptr_t)result % 8) != 0 || ((uintptr_t)match_of_landmark % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "prior_device and the result must be 8-byte, match_of_landmark 4-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  FxMapJoinArgs A{};
  assoc_args(&A.S, m, o, prior_host, prior_device, match_of_landmark);
  A.src = src, A.dst = dst;
  A.result = result;
  FX_MAP_RUN(fxk_map_join, "map join scratch");
  return FX_OK;
}

void fx_map_loop_options_default(fx_map_loop_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->search_dist = 2.0f;
  o->inlier_dist = 0.30f;
  o->min_baseline = 2.0f;
  o->hyp_corr = 64u;
  o->min_inliers = 3u;
  o->min_landmark_obs = 2u;
  o->segment = FX_LOC_LAST_SEGMENT;
  o->min_loop_scans = 256u;
  o->recent_scans = 32u;
  o->mode = FX_LOOP_FIT;
}

fx_status fx_map_close_loop(fx_ctx *c, fx_map *m, const fx_pose *prior_host, const double *prior_device, const fx_map_loop_options *opt,
                            fx_map_loop_result *result, int32_t *match_of_landmark) {
  FX_TRY(map_call_check(c, m));
  FX_TRY(prior_check(prior_host, prior_device));
  fx_map_loop_options o;
  fx_map_loop_options_default(&o);
  if (opt) o = *opt;
  FX_TRY(consensus_options_check(o));
  if (o.recent_scans >= o.min_loop_scans) return fail(FX_ERR_INVALID_ARG, "recent_scans must be below min_loop_scans");
  if (o.segment == FX_LOC_ANY_SEGMENT) return fail(FX_ERR_INVALID_ARG, "segment must be one segment or FX_LOC_LAST_SEGMENT, not FX_LOC_ANY_SEGMENT");
  if (o.mode > FX_LOOP_DRY_RUN) return fail(FX_ERR_INVALID_ARG, "mode must be FX_LOOP_FIT, FX_LOOP_GIVEN or FX_LOOP_DRY_RUN");
  if (o.mode == FX_LOOP_GIVEN && o.loop_first_scan >= o.loop_last_scan)
    return fail(FX_ERR_INVALID_ARG, "loop_first_scan must be below loop_last_scan");
  if (o.mode == FX_LOOP_GIVEN && !(std::isfinite(o.pivot_x) && std::isfinite(o.pivot_y))) return fail(FX_ERR_INVALID_ARG, "the pivot must be finite");
  if (o.reserved) return fail(FX_ERR_INVALID_ARG, "reserved must be 0");
  if (((uintptr_t)prior_device % 8) != 0 || ((uintptr_t)result % 8) != 0 || ((uintptr_t)match_of_landmark % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "prior_device and the result must be 8-byte, match_of_landmark 4-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  FxMapLoopArgs A{};
  assoc_args(&A.S, m, o, prior_host, prior_device, match_of_landmark);
  A.segment = o.segment, A.min_loop_scans = o.min_loop_scans, A.recent_scans = o.recent_scans;
  A.given_s0 = o.loop_first_scan, A.given_s1 = o.loop_last_scan, A.given_px = o.pivot_x, A.given_py = o.pivot_y;
  A.result = result;
  FX_MAP_RUN(fxk_map_loop, "map loop scratch");
  return FX_OK;
}

fx_status fx_map_loop_correct_poses(fx_ctx *c, const fx_map_loop_result *result, fx_pose *poses, uint32_t first_global_scan, uint32_t n_poses) {
  if (!c || !result || !poses) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (((uintptr_t)result % 8) != 0 || ((uintptr_t)poses % 8) != 0) return fail(FX_ERR_INVALID_ARG, "the result and the poses must be 8-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  FX_HIP(fxk_map_loop_poses(c->stream, result, poses, first_global_scan, n_poses));
  return FX_OK;
}

void fx_map_find_loop_options_default(fx_map_find_loop_options *o) {
  if (!o) return;
  o->inlier_dist = 0.30f;
  o->pair_tol = 0.30f;
  o->min_baseline = 2.0f;
  o->max_baseline = 60.0f;
  o->max_seeds = 16u;
  o->min_inliers = 4u;
  o->min_margin = 1u;
  o->min_landmark_obs = 2u;
  o->segment = FX_LOC_LAST_SEGMENT;
  o->target_segment = FX_FIND_SAME_SEGMENT;
  o->min_loop_scans = 256u;
  o->recent_scans = 32u;
  o->reserved = 0u;
}

fx_status fx_map_find_loop(fx_ctx *c, fx_map *m, const fx_map_find_loop_options *opt, fx_map_loop_candidate *result, int32_t *match_of_landmark) {
  FX_TRY(map_call_check(c, m, result != nullptr));
  fx_map_find_loop_options o;
  fx_map_find_loop_options_default(&o);
  if (opt) o = *opt;
  FX_TRY(constellation_options_check(o));
  if (o.segment == FX_LOC_ANY_SEGMENT) return fail(FX_ERR_INVALID_ARG, "segment must be one segment or FX_LOC_LAST_SEGMENT, not FX_LOC_ANY_SEGMENT");
  if (o.target_segment == FX_LOC_ANY_SEGMENT)
    return fail(FX_ERR_INVALID_ARG, "target_segment must be one segment, FX_LOC_LAST_SEGMENT or FX_FIND_SAME_SEGMENT, not FX_LOC_ANY_SEGMENT");
  if (o.target_segment == FX_FIND_SAME_SEGMENT && o.recent_scans >= o.min_loop_scans)
    return fail(FX_ERR_INVALID_ARG, "recent_scans must be below min_loop_scans when the targets are the segment's own");
  if (o.reserved) return fail(FX_ERR_INVALID_ARG, "reserved must be 0");
  if (((uintptr_t)result % 8) != 0 || ((uintptr_t)match_of_landmark % 4) != 0)
    return fail(FX_ERR_INVALID_ARG, "the result must be 8-byte, match_of_landmark 4-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  FxMapFindLoopArgs A{};
  constellation_args(&A, m, o);
  A.segment = o.segment, A.target_segment = o.target_segment, A.min_loop_scans = o.min_loop_scans, A.recent_scans = o.recent_scans;
  A.result = result, A.match = match_of_landmark;
  FX_MAP_RUN(fxk_map_find_loop, "map find loop scratch");
  return FX_OK;
}

namespace {
// The snapshot (include/fx.h fx_map_export_host): a 64-byte block header, then the sections, each from a 16-byte boundary and sized
// by content: n landmarks, r carry rows.  This is the layout's one statement in the library (Python: capi.map_snapshot_pack).
constexpr uint32_t kSnapMagic = 0x504D5846u, kSnapFormat = 1u, kSnapHeader = 64u;
struct SnapLayout {
  size_t o_hdr, o_rec, o_acc, o_alias, o_carry, o_kp, total;
};
SnapLayout snap_layout(uint32_t n, uint32_t r) {
  auto up = [](size_t b) { return (b + 15u) & ~(size_t)15; };
  SnapLayout L;
  L.o_hdr = kSnapHeader;
  L.o_rec = L.o_hdr + up(sizeof(fx_map_header));
  L.o_acc = L.o_rec + (size_t)n * sizeof(fx_map_landmark);
  L.o_alias = L.o_acc + (size_t)n * FX_MAP_ACC * sizeof(double);
  L.o_carry = L.o_alias + up((size_t)n * 4);
  L.o_kp = L.o_carry + up((size_t)r * 4);
  L.total = L.o_kp + (size_t)r * 16;
  return L;
}
}  // namespace

fx_status fx_map_snapshot_check(const void *src, size_t bytes, uint32_t max_landmarks, uint32_t max_carry_rows) {
  if (!src) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (bytes < kSnapHeader) return fail(FX_ERR_INVALID_ARG, "snapshot: shorter than the 64-byte block header");
  const uint8_t *p = (const uint8_t *)src;
  uint32_t w[10];
  uint64_t total;
  memcpy(w, p, sizeof w), memcpy(&total, p + 40, 8);
  if (w[0] != kSnapMagic) return fail(FX_ERR_INVALID_ARG, "snapshot: wrong magic (not an fx_map snapshot)");
  if (w[1] != kSnapFormat) return fail(FX_ERR_INVALID_ARG, "snapshot: unknown format " + std::to_string(w[1]) + " (this library reads format 1)");
  if (w[3] != kSnapHeader || w[6] != sizeof(fx_map_header) || w[7] != sizeof(fx_map_landmark) || w[8] != FX_MAP_ACC)
    return fail(FX_ERR_INVALID_ARG, "snapshot: struct sizes differ (block header " + std::to_string(w[3]) + ", fx_map_header " + std::to_string(w[6]) +
                                        ", fx_map_landmark " + std::to_string(w[7]) + ", accumulators " + std::to_string(w[8]) + ")");
  const uint32_t n = w[4], r = w[5];
  const SnapLayout L = snap_layout(n, r);
  if (total != bytes) return fail(FX_ERR_INVALID_ARG, "snapshot: total bytes " + std::to_string(total) + " but " + std::to_string(bytes) + " given");
  if (total != L.total)
    return fail(FX_ERR_INVALID_ARG, "snapshot: total bytes " + std::to_string(total) + " but the sections sum to " + std::to_string(L.total));
  fx_map_header H;
  memcpy(&H, p + L.o_hdr, sizeof H);
  if (H.n_landmarks != n || H.carry_rows != r)
    return fail(FX_ERR_INVALID_ARG, "snapshot: the block's counts differ from its fx_map_header (n_landmarks " + std::to_string(H.n_landmarks) +
                                        ", carry_rows " + std::to_string(H.carry_rows) + ")");
  if (H.n_landmarks > H.n_needed) return fail(FX_ERR_INVALID_ARG, "snapshot: n_landmarks exceeds n_needed");
  if (n > max_landmarks) return fail(FX_ERR_TOO_LARGE, "snapshot: " + std::to_string(n) + " landmarks, max_landmarks " + std::to_string(max_landmarks));
  if (r > max_carry_rows) return fail(FX_ERR_TOO_LARGE, "snapshot: " + std::to_string(r) + " carry rows, max_carry_rows " + std::to_string(max_carry_rows));
  const uint8_t *alias = p + L.o_alias, *carry = p + L.o_carry;
  auto word = [](const uint8_t *q, size_t i) {
    int32_t v;
    memcpy(&v, q + 4 * i, 4);
    return v;
  };
  for (uint32_t i = 0; i < n; ++i) {
    const int32_t a = word(alias, i);
    if (a < -1 || (a >= 0 && (uint32_t)a >= n)) return fail(FX_ERR_INVALID_ARG, "snapshot: alias[" + std::to_string(i) + "] = " + std::to_string(a) + " is outside [-1, n)");
    if (a >= 0 && word(alias, (size_t)a) != -1)
      return fail(FX_ERR_INVALID_ARG, "snapshot: alias[" + std::to_string(i) + "] = " + std::to_string(a) + " is not resolved (a chain)");
  }
  for (uint32_t j = 0; j < r; ++j) {
    const int32_t v = word(carry, j);
    if (v < -1 || (v >= 0 && (uint32_t)v >= n)) return fail(FX_ERR_INVALID_ARG, "snapshot: carry[" + std::to_string(j) + "] = " + std::to_string(v) + " is outside [-1, n)");
  }
  if (H.n_needed > H.n_landmarks && max_landmarks != H.n_landmarks)
    return fail(FX_ERR_INVALID_ARG, "snapshot: the map overflowed (n_needed " + std::to_string(H.n_needed) + " > n_landmarks " + std::to_string(H.n_landmarks) +
                                        "): fx_map_compact it before taking it into a map of another max_landmarks");
  return FX_OK;
}

fx_status fx_map_export_host(fx_ctx *c, fx_map *m, void *dst, size_t capacity, size_t *bytes_out) {
  FX_TRY(map_call_check(c, m, dst || !capacity));
  FX_HIP(hipSetDevice(c->device));
  fx_map_header H;
  FX_HIP(hipMemcpyAsync(&H, m->a.header, sizeof H, hipMemcpyDeviceToHost, c->stream));
  FX_HIP(hipStreamSynchronize(c->stream));
  const uint32_t n = std::min(H.n_landmarks, m->a.cap), r = std::min(H.carry_rows, m->a.max_carry);
  const SnapLayout L = snap_layout(n, r);
  if (bytes_out) *bytes_out = L.total;
  if (!dst) return FX_OK;
  if (capacity < L.total) return fail(FX_ERR_TOO_LARGE, "snapshot: " + std::to_string(L.total) + " bytes, capacity " + std::to_string(capacity));
  uint8_t *p = (uint8_t *)dst;
  memset(p, 0, L.total);
  const uint32_t w[10] = {kSnapMagic, kSnapFormat, fx_version(), kSnapHeader, n, r, (uint32_t)sizeof(fx_map_header), (uint32_t)sizeof(fx_map_landmark), FX_MAP_ACC, 0u};
  const uint64_t total = L.total;
  memcpy(p, w, sizeof w), memcpy(p + 40, &total, 8);
  memcpy(p + L.o_hdr, &H, sizeof H);
  if (n) {
    FX_HIP(hipMemcpyAsync(p + L.o_rec, m->a.records, (size_t)n * sizeof(fx_map_landmark), hipMemcpyDeviceToHost, c->stream));
    FX_HIP(hipMemcpyAsync(p + L.o_acc, m->a.acc, (size_t)n * FX_MAP_ACC * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FX_HIP(hipMemcpyAsync(p + L.o_alias, m->a.alias, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (r) {
    FX_HIP(hipMemcpyAsync(p + L.o_carry, m->a.carry, (size_t)r * 4, hipMemcpyDeviceToHost, c->stream));
    FX_HIP(hipMemcpyAsync(p + L.o_kp, m->a.carry_kp, (size_t)r * 16, hipMemcpyDeviceToHost, c->stream));
  }
  FX_HIP(hipStreamSynchronize(c->stream));
  return FX_OK;
}

namespace {
// the snapshot's bytes into the context's pinned staging (fx_map_import_host, fx_map_append_host): free to write once the copies
// of the call before are done; the caller records snap_ev behind the copies it enqueues from it
fx_status snap_stage(fx_ctx *c, const void *src, size_t bytes) {
  if (!c->snap_ev) FX_HIP(hipEventCreateWithFlags(&c->snap_ev, hipEventDisableTiming));
  FX_HIP(hipEventSynchronize(c->snap_ev));
  if (bytes > c->snap_bytes) {
    if (c->snap_h) FX_HIP(hipHostFree(c->snap_h));
    c->snap_h = nullptr, c->snap_bytes = 0;
    const size_t want = std::max(bytes, (size_t)4096);
    void *q = nullptr;
    hipError_t e = hipHostMalloc(&q, want, hipHostMallocDefault);
    if (e != hipSuccess) return fail(FX_ERR_OOM, "snapshot staging hipHostMalloc(" + std::to_string(want) + "): " + hipGetErrorString(e));
    c->snap_h = (uint8_t *)q, c->snap_bytes = want;
  }
  memcpy(c->snap_h, src, bytes);
  return FX_OK;
}
// the target's part of an append's arguments
void append_target(FxMapAppendArgs *A, const fx_map *m, fx_map_append_result *result) {
  A->header = m->a.header, A->records = m->a.records, A->acc = m->a.acc, A->alias = m->a.alias, A->carry = m->a.carry, A->carry_kp = m->a.carry_kp;
  A->cap = m->a.cap, A->max_carry = m->a.max_carry;
  A->result = (uint32_t *)result;
}
}  // namespace

fx_status fx_map_import_host(fx_ctx *c, fx_map *m, const void *src, size_t bytes) {
  FX_TRY(map_call_check(c, m, src != nullptr));
  FX_TRY(fx_map_snapshot_check(src, bytes, m->a.cap, m->a.max_carry));
  FX_HIP(hipSetDevice(c->device));
  FX_TRY(snap_stage(c, src, bytes));
  const uint8_t *p = c->snap_h;
  uint32_t n, r;
  memcpy(&n, p + 16, 4), memcpy(&r, p + 20, 4);
  const SnapLayout L = snap_layout(n, r);
  FX_HIP(fxk_map_reset(c->stream, m->a));  // alias -1 everywhere, the state words 0
  FX_HIP(hipMemcpyAsync(m->a.header, p + L.o_hdr, sizeof(fx_map_header), hipMemcpyHostToDevice, c->stream));
  if (n) {
    FX_HIP(hipMemcpyAsync(m->a.records, p + L.o_rec, (size_t)n * sizeof(fx_map_landmark), hipMemcpyHostToDevice, c->stream));
    FX_HIP(hipMemcpyAsync(m->a.acc, p + L.o_acc, (size_t)n * FX_MAP_ACC * sizeof(double), hipMemcpyHostToDevice, c->stream));
    FX_HIP(hipMemcpyAsync(m->a.alias, p + L.o_alias, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  }
  if (r) {
    FX_HIP(hipMemcpyAsync(m->a.carry, p + L.o_carry, (size_t)r * 4, hipMemcpyHostToDevice, c->stream));
    FX_HIP(hipMemcpyAsync(m->a.carry_kp, p + L.o_kp, (size_t)r * 16, hipMemcpyHostToDevice, c->stream));
  }
  FX_HIP(hipEventRecord(c->snap_ev, c->stream));
  return FX_OK;
}

fx_status fx_map_append(fx_ctx *c, fx_map *dst, fx_map *src, fx_map_append_result *result) {
  if (!c || !dst || !src) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (dst == src) return fail(FX_ERR_INVALID_ARG, "dst and src are the same map");
  FX_TRY(map_call_check(c, dst));
  if (src->ctx != c) return fail(FX_ERR_INVALID_ARG, "the source map belongs to another context (go through the snapshot: fx_map_append_host)");
  if (((uintptr_t)result % 4) != 0) return fail(FX_ERR_INVALID_ARG, "the result must be 4-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  FxMapAppendArgs A{};
  append_target(&A, dst, result);
  A.src.header = src->a.header, A.src.records = src->a.records, A.src.acc = src->a.acc, A.src.alias = src->a.alias, A.src.carry = src->a.carry,
  A.src.carry_kp = src->a.carry_kp;
  A.src_cap = src->a.cap, A.src_max_carry = src->a.max_carry;
  FX_MAP_RUN(fxk_map_append, "map append scratch");
  return FX_OK;
}

fx_status fx_map_append_host(fx_ctx *c, fx_map *dst, const void *src, size_t bytes, fx_map_append_result *result) {
  FX_TRY(map_call_check(c, dst, src != nullptr));
  if (((uintptr_t)result % 4) != 0) return fail(FX_ERR_INVALID_ARG, "the result must be 4-byte aligned");
  FX_TRY(fx_map_snapshot_check(src, bytes, dst->a.cap, 0xffffffffu));
  FX_HIP(hipSetDevice(c->device));
  FxMapAppendArgs A{};
  append_target(&A, dst, result);
  A.stage_bytes = bytes;
  FX_TRY(c->merge_scratch.reserve(c, fxk_map_append_scratch(&A, nullptr), "map append scratch"));
  (void)fxk_map_append_scratch(&A, c->merge_scratch.d);
  FX_TRY(snap_stage(c, src, bytes));
  uint32_t n, r;
  memcpy(&n, c->snap_h + 16, 4), memcpy(&r, c->snap_h + 20, 4);
  const SnapLayout L = snap_layout(n, r);
  // the sections start 16-byte aligned in the block and the block does in the scratch: the kernels read them as vectors
  FX_HIP(hipMemcpyAsync(A.stage, c->snap_h, bytes, hipMemcpyHostToDevice, c->stream));
  FX_HIP(hipEventRecord(c->snap_ev, c->stream));
  A.src.header = A.stage + L.o_hdr, A.src.records = A.stage + L.o_rec, A.src.acc = (const double *)(A.stage + L.o_acc);
  A.src.alias = (const int32_t *)(A.stage + L.o_alias), A.src.carry = (const int32_t *)(A.stage + L.o_carry);
  A.src.carry_kp = (const uint4 *)(A.stage + L.o_kp);
  A.src_cap = n, A.src_max_carry = r;
  FX_HIP(fxk_map_append(c->stream, A));
  return FX_OK;
}

fx_status fx_unpack_pointcloud2(fx_ctx *c, const void *data_device, uint32_t n_points, const fx_pc2_layout *lay,
                                void *dst_device_xyzi) {
  if (!c || !lay || (n_points && (!data_device || !dst_device_xyzi))) return fail(FX_ERR_INVALID_ARG, "null argument");
  const uint32_t offs[3] = {lay->offset_x, lay->offset_y, lay->offset_z};
  for (uint32_t o : offs)
    if (o + 4 > lay->point_step) return fail(FX_ERR_INVALID_ARG, "field offset outside the point record");
  if (lay->offset_intensity != 0xffffffffu && lay->offset_intensity + 4 > lay->point_step)
    return fail(FX_ERR_INVALID_ARG, "intensity offset outside the point record");
  if (((uintptr_t)dst_device_xyzi % 16) != 0) return fail(FX_ERR_INVALID_ARG, "dst must be 16-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  if (n_points)
    fxk_unpack_pc2(c->stream, data_device, n_points, lay->point_step, lay->offset_x, lay->offset_y, lay->offset_z,
                   lay->offset_intensity, lay->is_bigendian, dst_device_xyzi, c->plan_cfg.n_cu * 8u);
  FX_HIP(hipGetLastError());
  return FX_OK;
}

fx_status fx_pack_pointxyzi(fx_ctx *c, uint32_t which, uint32_t scan, void *dst_device, uint32_t capacity_points,
                            uint32_t *n_points_out) {
  if (!c || !dst_device || !n_points_out) return fail(FX_ERR_INVALID_ARG, "null argument");
  if (scan >= c->plan_state.last_batch) return fail(FX_ERR_INVALID_ARG, "scan index outside the last batch");
  if (((uintptr_t)dst_device % 16) != 0) return fail(FX_ERR_INVALID_ARG, "dst must be 16-byte aligned");
  FX_HIP(hipSetDevice(c->device));
  const FxBuffers &B = c->buf;
  const fx_limits &L = c->lim;
  const float4 *src = nullptr;
  const uint32_t *cnt = nullptr;
  switch (which) {
    case FX_CLOUD_KEYPOINTS: src = B.keypoints + (size_t)scan * L.max_keypoints, cnt = B.n_kp + scan; break;
    case FX_CLOUD_FILTERED: src = B.filt + (size_t)scan * L.max_points, cnt = B.n_filt + scan; break;
    case FX_CLOUD_KEYPOINT_CLOUD: src = B.kpc + (size_t)scan * L.max_kpc_points, cnt = B.n_kpc + scan; break;
    default: return fail(FX_ERR_INVALID_ARG, "unknown cloud selector");
  }
  uint32_t n = 0;
  FX_HIP(hipMemcpyAsync(&n, cnt, 4, hipMemcpyDeviceToHost, c->stream));
  FX_HIP(hipStreamSynchronize(c->stream));
  if (n > capacity_points) return fail(FX_ERR_TOO_LARGE, "destination too small for the cloud");
  if (n) fxk_pack_xyzi32(c->stream, src, n, dst_device, c->plan_cfg.n_cu * 4u);
  FX_HIP(hipGetLastError());
  *n_points_out = n;
  return FX_OK;
}

fx_status fx_pack_features(fx_ctx *c, void *dst_device, uint32_t capacity_records) {
  if (!c || !dst_device) return fail(FX_ERR_INVALID_ARG, "null argument");
  FX_HIP(hipSetDevice(c->device));
  fxk_pack_features(c->stream, c->dp, c->buf, c->plan_state.last_batch, dst_device, capacity_records, c->plan_cfg.n_cu * 8u);
  FX_HIP(hipGetLastError());
  return FX_OK;
}

}  // extern "C"
