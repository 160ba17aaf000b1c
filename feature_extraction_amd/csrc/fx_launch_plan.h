// fx_launch_plan.h — which kernels a batch runs, with what grids and in how many slices: one host function, no HIP.
//
// fx_plan_batch decides; enqueue_stages (fx_api.cpp) and the launchers (fx_kernels.hip) only launch what the plan says.  The
// plan decides speed, never a result: every launch set here computes the same bits (tests/test_gpu_front.py, the fuzz's
// paths), so nothing but a timing can see a wrong grid on the device — csrc/fx_plan_selftest.cpp pins the policy on a CPU.
#ifndef FX_LAUNCH_PLAN_H_
#define FX_LAUNCH_PLAN_H_
#include <stdint.h>

// FxBuffers::tier_hint[]: what the last completed batch had for the rarely used tiers (k_slow's last workgroup and k_desc
// write them; pinned host memory).  0xffffffff: nothing known yet.
#define FX_N_HINTS 8
enum FxHint {
  FX_HINT_RINGS_FIRST = 0,   // rings the first run tier handed on — to the second run tier where there is one, else to the workgroup tier (largest XCD class)
  FX_HINT_RINGS_SECOND = 1,  // rings the second run tier handed to the workgroup tier (largest XCD class)
  FX_HINT_BIG_MERGES = 2,    // scans for the LDS merge tier
  FX_HINT_HUGE_MERGES = 3,   // scans for the large merge tier
  FX_HINT_DENSE_ROWS = 4,    // rows of the dense descriptor tier
  FX_HINT_DENSE_POINTS = 5,  // their support points
  FX_HINT_REDO_SCANS = 6,    // scans k_front handed to k_front_redo
  FX_HINT_SLOW_SCANS = 7,    // scans handed to the slow tier (k_slow)
};
#define FX_HINT_UNKNOWN 0xffffffffu

// what the tiers were handed lately: the largest count of the last FX_HINT_HOLD_BATCHES batches (a workload that alternates
// between batches with and without work for a tier keeps the tier's grid)
constexpr uint32_t FX_HINT_HOLD_BATCHES = 64;
// A batch that hands more than an eighth of its scans to k_front_redo sends the next FX_FRONT_RETRY batches through the
// separate kernels (k_prep ... k_merge_*), which are the fast way for large scans.
constexpr uint32_t FX_FRONT_RETRY = 64;
// batches that still get the dense tier's own kernels after the last one that needed them
constexpr uint32_t FX_DENSE_LINGER = 64;
// batches of up to this many scans run the front's streaming pass sliced (FX_FRONT_STREAMED)
constexpr uint32_t FX_FRONT_STREAM_MAX_BATCH = 8;
constexpr uint32_t FX_MERGE_CAP_SMALL = 512;  // candidates k_merge_small holds

// What is fixed for a context, or set by a setter.  The test hooks (FX_* in the environment of the TEST build) are read
// once, in fx_create.
struct FxPlanConfig {
  uint32_t n_cu = 256;
  uint32_t n_rings = 16;
  bool estimate_descriptors = true;
  // limits and caps
  uint32_t max_points = 0, max_keypoints = 0, max_total_keypoints = 0, max_candidates = 0, max_ring_points = 0;
  uint32_t merge_big_cap = 0;  // candidates the LDS merge tier holds as points (< max_candidates: the large merge tier exists)
  uint32_t list_cap = 0, dense_min = 0;
  uint32_t gs_slots = 0;   // k_slow's scratch regions: never more workgroups
  uint32_t gsd_slots = 0;  // the dense stand-in's scratch regions: never more workgroups
  bool merge_hp = false;    // FxBuffers::merge_hp is allocated: the large merge tier may run as three launches
  bool gather_cnt = false;  // FxBuffers::gather_cnt is allocated: the support gather may run counted
  // build constants of the kernels (fxk_* getters)
  uint32_t prep_slices_max = 16, merge_slices_max = 8, gather_counted_max = 16;
  uint32_t front_merge_cap = 512;    // candidates k_front merges itself
  uint32_t gather_kcap = 2048;       // keypoints the support gather's LDS tables hold
  uint32_t gather_slices_big = 1;    // workgroups a scan of k_gather from 64 scans on
  uint32_t dsort_per_cu = 4, ddens_per_cu = 3;  // workgroups a CU of k_dense_sort's / k_dense_density's full grids
  // setters and hooks
  uint32_t batches_in_flight = 1;  // fx_set_batches_in_flight: the caller's contexts busy on this device at a time
  uint32_t tier_min_grid = 8;      // FX_TIER_MIN_GRID: workgroups the rarely used tiers get at least (0: always the full grids)
  bool front_ok = false;           // sensor within k_front's ring capacity (and not FX_FRONT=0)
  uint32_t front_force = 0;        // FX_FRONT_FORCE: 1 k_front hands every scan to k_front_redo; 2: and that one every ring and merge to k_slow
  int front_stream = -1;           // FX_FRONT_STREAM: 1 always the sliced streaming pass + k_front_cd, 0 never; -1: batches of up to FX_FRONT_STREAM_MAX_BATCH scans
  int front_split = 0;             // FX_FRONT_SPLIT: 1 the two launches; 2 the same with k_front_cd's lean image; 0: the one fused launch
  int prep_slices = -1;            // FX_PREP_SLICES: workgroups a scan in the separate kernels' streaming pass and ring split
  int merge_slices = -1;           // FX_MERGE_SLICES: workgroups a scan in the large merge tier's pair loop (1: the one launch)
  int gather_slices = -1;          // FX_GATHER_COUNTED: workgroups a scan in the support gather's counted slices (1: one workgroup a scan)
  int gather_one = 0;              // FX_GATHER_ONE: 256 one k_gather workgroup a scan, 1024 k_gather_wide, at any batch size (0: by the batch)
  int dense_force = -1;            // FX_DENSE_SLOW: 1 always k_desc's stand-in workgroups, 0 always the tier's own kernels
  // FX_SKIP_EMPTY (experiment): bit 0 no k_front_redo, bit 1 no dense tier — only for workloads that need neither (a dense row
  // that does turn up is then neither computed NOR CLEARED: every tier clears its own rows, so such a row keeps what the last
  // batch left in it); bits 2 / 3: no k_dense_finish / k_dense_density (measurement: results wrong)
  uint32_t skip_mask = 0;
  uint32_t desc_wgs_per_cu = 0;  // FX_DESC_WGS_PER_CU: the group workgroups of k_desc's launch a CU (0: by batches_in_flight)
  uint32_t desc_grid_abs = 0;    // FX_DESC_GRID: the group workgroups of k_desc's launch, absolute
};

// What one batch leaves for the next.
struct FxPlanState {
  uint32_t hint_hold[FX_N_HINTS] = {}, hint_age[FX_N_HINTS] = {};
  uint32_t dense_fast_left = 0;  // batches that still get the dense tier's kernels
  uint32_t front_pause = 0;      // batches left on the separate kernels
  bool front_last = false;       // what the last batch ran
  uint32_t last_batch = 0;
  // after a failed batch (and with it, the device's hints set to unknown): nothing is known, nothing is paused
  void reset() {
    for (int i = 0; i < FX_N_HINTS; ++i) hint_hold[i] = FX_HINT_UNKNOWN, hint_age[i] = 0;
    front_pause = 0;
  }
};

enum FxFrontMode {
  FX_FRONT_FUSED,     // k_front
  FX_FRONT_TWO,       // k_front_ab, k_front_cd
  FX_FRONT_TWO_LEAN,  // k_front_ab, k_front_cdl
  FX_FRONT_STREAMED,  // k_prep_count, k_prep_sliced, k_bucket_sliced, k_front_cd
  FX_FRONT_SEPARATE,  // k_prep ... k_merge_*
};
enum FxGatherKind {
  FX_GATHER_PASSES,   // k_gather_passes, gather_n workgroups a scan
  FX_GATHER_COUNTED,  // k_gather_count + k_gather_scatter, gather_n workgroups a scan
  FX_GATHER_WIDE,     // k_gather_wide, one workgroup a scan
  FX_GATHER_SLICED,   // k_gather, gather_n workgroups a scan
};

// Everything enqueue_stages needs to issue a batch's launches.  Grids are workgroups.
struct FxLaunchPlan {
  uint32_t batch = 0;
  FxFrontMode front = FX_FRONT_SEPARATE;
  uint32_t prep_slices = 1;  // workgroups a scan of the streaming pass and the ring split (1: k_prep, k_bucket)
  bool many_rings = false;   // k_bucket_many
  // the front and what it hands on
  uint32_t front_merge_cap = 0;
  uint32_t force_redo = 0, force_slow = 0;
  uint32_t redo_grid = 0;  // 0: no k_front_redo (FX_SKIP_EMPTY bit 0)
  uint32_t slow_grid = 1;
  // the separate kernels
  uint32_t runs_grid = 0;
  uint32_t runs2_grid = 0;  // 0: no second run tier
  uint32_t large_grid = 0;
  uint32_t merge_small_cap = 0;
  uint32_t merge_big_grid = 0, merge_big_last = 0;
  uint32_t merge_huge_grid = 0;  // 0: no large merge tier
  uint32_t merge_huge_slices = 1;  // > 1: the three launches
  // descriptors
  bool descriptors = false;
  FxGatherKind gather = FX_GATHER_WIDE;
  uint32_t gather_n = 1;
  bool rng_ord = false;  // k_rng_ord follows (one workgroup a scan settles the RNG ordinals itself)
  uint32_t desc_cap = 0, desc_wg = 0, desc_wave = 0, desc_group = 0, desc_dslow = 0;
  bool dense = false;  // the dense tier's own kernels
  uint32_t dense_sort_grid = 0, dense_density_grid = 0, dense_finish_grid = 0;
  uint32_t dense_skip = 0;  // FX_SKIP_EMPTY bits 2 / 3
};

// The tiers behind the common ones (workgroup-per-ring, LDS-sized merges, the dense descriptor tier) take their work from
// lists by stride or ticket, so any grid computes the same; a launch that finds its list empty still has to place every
// workgroup, and these want most of a CU each.  Their grids follow what the context's previous batch handed them (twice
// that, at least tier_min_grid, at most the full grid; the full grid while nothing is known): a sparse batch costs
// eight workgroups a tier instead of 256, and a batch that is suddenly dense runs its tiers narrow once.
// (min_wg: the scans k_front hands on — k_front_redo, k_slow — get ONE workgroup when the last 64 batches handed on
//  nothing: an empty launch of eight k_front-shaped workgroups instead costs the headline 1 %, profiles/r05_experiments.md §9)
inline uint32_t fx_tier_grid(uint32_t tier_min_grid, uint32_t work, uint32_t full, uint32_t bound, uint32_t per = 1, uint32_t min_wg = 0) {
  uint32_t g = work > full / 2 ? full : 2 * work;  // (also: unknown)
  const uint32_t floor_wg = min_wg ? (min_wg < tier_min_grid ? min_wg : tier_min_grid) : tier_min_grid;
  if (g < (floor_wg + per - 1) / per) g = (floor_wg + per - 1) / per;
  if (g > bound) g = bound ? bound : 1;  // never more workgroups than the batch could have items for
  return g < full ? g : full;
}

// Front kernel or separate kernels: redo_hint is what the last COMPLETED batch of this context handed to k_front_redo (with
// batches in flight: an older batch's count, possibly of another size — this decides speed only, never a result).  Records
// what this batch runs for the next one's decision.
inline bool fx_plan_front(const FxPlanConfig &cfg, FxPlanState *st, uint32_t redo_hint, uint32_t batch) {
  bool front = cfg.front_ok;
  if (front && st->front_pause) {
    --st->front_pause;
    front = false;
  } else if (front && !cfg.front_force && st->front_last && redo_hint != FX_HINT_UNKNOWN && redo_hint > (st->last_batch + 7u) / 8u) {
    st->front_pause = FX_FRONT_RETRY;
    front = false;
  }
  st->front_last = front;
  st->last_batch = batch;
  return front;
}

// The plan of one batch.  Pure apart from *st, which it does not touch when `capture` is set: a captured graph is replayed
// for every later batch of its size, so its grids are the full ones, bounded by the batch, and its front is cfg.front_ok.
inline FxLaunchPlan fx_plan_batch(const FxPlanConfig &cfg, FxPlanState *st, const uint32_t raw_hints[FX_N_HINTS], uint32_t batch, bool capture) {
  auto umin = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
  auto umax = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
  FxLaunchPlan p;
  p.batch = batch;
  const bool live = !capture;
  const bool front = live ? fx_plan_front(cfg, st, raw_hints[FX_HINT_REDO_SCANS], batch) : cfg.front_ok;
  uint32_t hint[FX_N_HINTS];
  for (int i = 0; i < FX_N_HINTS; ++i) {
    hint[i] = FX_HINT_UNKNOWN;
    if (!live || !cfg.tier_min_grid) continue;
    hint[i] = raw_hints[i];
    // (held: the largest count of the last FX_HINT_HOLD_BATCHES batches; "nothing known yet" stays that only until something
    //  is known — held like a count it kept every rare tier at its full grid for the first 64 batches of a context, and
    //  after every reset)
    if (hint[i] == FX_HINT_UNKNOWN || st->hint_hold[i] == FX_HINT_UNKNOWN || hint[i] >= st->hint_hold[i] || ++st->hint_age[i] > FX_HINT_HOLD_BATCHES)
      st->hint_hold[i] = hint[i], st->hint_age[i] = 0;
    hint[i] = st->hint_hold[i];
  }
  if (!batch) return p;
  auto tier_grid = [&](uint32_t work, uint32_t full, uint32_t bound, uint32_t per = 1, uint32_t min_wg = 0) {
    return fx_tier_grid(cfg.tier_min_grid, work, full, bound, per, min_wg);
  };
  const uint32_t big_grid = cfg.n_cu;
  // (never more workgroups than k_slow has scratch regions)
  p.slow_grid = umax(1u, umin(tier_grid(hint[FX_HINT_SLOW_SCANS], big_grid, batch), cfg.gs_slots));
  if (front) {
    // stages 0-4 in three launches: k_front; k_front_redo — workgroups of k_front's shape, a few of them unless the
    // previous batch had work for it — for the scans that do not fit k_front's tables; and k_slow (256 threads, 9 KB of
    // LDS: an empty launch of it places anywhere) for what exceeds that shape's LDS too, on scratch in HBM.  All three go
    // with EVERY batch: the hints size grids, they never decide whether a scan gets what it needs.
    p.front_merge_cap = umin(cfg.front_merge_cap, cfg.max_candidates);
    // A handful of scans per call (the reference's own mode: one scan per callback, ref: node.cpp:72, :386): k_front's streaming
    // pass would be ONE workgroup a scan on a chip of 256 CUs — 0.036 of a scan's 0.093 ms in k_front.  So the streaming pass
    // and the ring split go out SLICED, sixteen workgroups a scan (the counting pass, k_prep_sliced, k_bucket_sliced: the
    // separate kernels' own, whose ring-major records are what k_front_ab writes), and k_front_cd clusters and merges in one.
    const bool stream = cfg.front_stream >= 0 ? cfg.front_stream != 0 : batch <= FX_FRONT_STREAM_MAX_BATCH;
    // k_front as TWO launches (k_front_ab: streaming pass + ring split, the ring-major records through HBM; k_front_cd:
    // clustering + merge).  Built, parity-green, and NOT the default: alone the two take what the one takes
    // (0.134 + 0.156 against 0.286 ms), with four batches in flight the headline is 3 % lower (profiles/r06_experiments.md §1).
    if (cfg.front_split)
      p.front = cfg.front_split >= 2 ? FX_FRONT_TWO_LEAN : FX_FRONT_TWO;
    else
      p.front = stream ? FX_FRONT_STREAMED : FX_FRONT_FUSED;
    if (p.front == FX_FRONT_STREAMED) p.prep_slices = cfg.prep_slices_max;
    p.force_redo = cfg.front_force >= 1u ? 1u : 0u;
    p.force_slow = cfg.front_force >= 2u ? 1u : 0u;
    // (the grid k_front_redo gets when the last 64 batches handed it nothing: ONE workgroup when the caller keeps four
    //  batches in flight — an empty launch of k_front-shaped workgroups waits for whole free CUs in the other batches' way:
    //  four of them cost the headline 0.6 %, eight 1.1 % —, four otherwise: a stream with the chip to itself pays nothing for
    //  them, and a batch that suddenly hands on many scans is not dealt through a single workgroup)
    const uint32_t redo_floor = cfg.batches_in_flight >= 4u ? 1u : 4u;
    if (!(cfg.skip_mask & 1u)) p.redo_grid = tier_grid(hint[FX_HINT_REDO_SCANS], 2 * big_grid, batch, 1, redo_floor);
  } else {
    p.front = FX_FRONT_SEPARATE;
    // one workgroup a scan when the batch fills the chip with that, several (a counting pass first) when it does not and the
    // scans are big enough to be worth a second read: 64 scans of 262 144 points are 64 workgroups on 256 CUs
    uint32_t slices = 1;
    if (cfg.prep_slices >= 0) {
      slices = (uint32_t)cfg.prep_slices;  // (test hook)
    } else if (4u * batch <= 2u * big_grid && cfg.max_points >= 65536u) {
      // (from four workgroups a scan on: with two — 256 scans of 131 072 points — the second read of the scan costs more
      //  than the wider grid gains: k_prep 0.15 -> 0.23 ms; with eight — 64 scans of 262 144 points — 0.23 -> 0.125 ms.
      //  Three workgroups a CU in all: what k_bucket_sliced's scalar registers (106: six wavefronts a SIMD) let be resident at once — 64 scans: the ring split
      //  0.092 / 0.065 / 0.109 ms with 8 / 12 / 16 a scan; 128 scans: 0.16 / 0.109 / 0.206 with 4 / 6 / 8,
      //  profiles/r06_experiments.md §12)
      slices = 3u * big_grid / batch;
    }
    p.prep_slices = umax(1u, umin(slices, cfg.prep_slices_max));
    p.many_rings = cfg.n_rings > 24;
    // one wavefront per (scan, ring): the hardware dispatcher balances the rings, whose costs differ a lot
    // (persistent wavefronts striding over the items: 0.18 ms instead of 0.14)
    const uint32_t n_items = batch * cfg.n_rings;
    p.runs_grid = (n_items + 7) / 8 * 8;
    // sensors of more than the reference's 16 rings: dense rings, many of which need longer run tables than the first tier's
    const bool runs2 = cfg.n_rings > 16;
    // (these two take the list of XCD class blockIdx % 8: grids are multiples of 8, the hints the longest class list)
    if (runs2) p.runs2_grid = 8 * tier_grid(hint[FX_HINT_RINGS_FIRST], (big_grid * 7 + 7) / 8, (n_items + 7) / 8, 8);  // (seven a CU: 21 KB of LDS each)
    p.large_grid = 8 * tier_grid(hint[runs2 ? FX_HINT_RINGS_SECOND : FX_HINT_RINGS_FIRST], (big_grid + 7) / 8, (n_items + 7) / 8, 8);
    p.merge_small_cap = umin(cfg.max_candidates, FX_MERGE_CAP_SMALL);
    p.merge_big_grid = tier_grid(hint[FX_HINT_BIG_MERGES], big_grid, batch);
    p.merge_big_last = cfg.merge_big_cap >= cfg.max_candidates ? 1u : 0u;
    if (cfg.merge_big_cap < cfg.max_candidates) {
      // one workgroup a scan in one launch — or, when the batches before had so few scans for this tier that those leave most
      // of the chip idle (64 scans of config 5 on 256 CUs), three launches with several workgroups a scan in the pair loop,
      // which is 97 % of the tier (merge_body's PHASE).  The hint decides speed, never a result.
      const uint32_t h = hint[FX_HINT_HUGE_MERGES];
      p.merge_huge_grid = tier_grid(h, big_grid, batch);
      uint32_t ms = 1;
      if (cfg.merge_slices >= 0)
        ms = (uint32_t)cfg.merge_slices;  // (test hook)
      else if (live && h != FX_HINT_UNKNOWN && h > 0 && 2u * h * cfg.batches_in_flight <= big_grid)
        ms = big_grid / (h * cfg.batches_in_flight);  // (the caller's other batches fill the chip as well: config 5 with four in flight 8.6e4 scans/s in one launch, 8.0e4 in three)
      ms = umin(ms, cfg.merge_slices_max);
      p.merge_huge_slices = ms > 1 && cfg.merge_hp ? ms : 1u;
    }
  }
  if (!cfg.estimate_descriptors) return p;
  p.descriptors = true;
  // one workgroup a scan — or, for batches of few big scans with the chip to themselves (64 scans of 262 144 points: 64
  // workgroups on 256 CUs), several a scan in two launches: a counting pass, then the scatter with every slice's list
  // positions known (from four a scan on: the near sectors are read and tested twice)
  uint32_t counted = 1;
  if (cfg.gather_slices >= 0)
    counted = (uint32_t)cfg.gather_slices;  // (test hook)
  else if (live && 10u * batch * cfg.batches_in_flight <= 3u * big_grid && cfg.max_points >= 65536u)
    // (256-thread workgroups, three a CU: all resident at once.  From ten a scan on: config 5 — 64 scans — 0.255 ms with one
    //  wide workgroup a scan, 0.405 / 0.246 / 0.197 / 0.273 with 4 / 8 / 12 / 16 counted slices, profiles/r06_experiments.md §4)
    counted = 3u * big_grid / (batch * cfg.batches_in_flight);
  // One workgroup per scan (the sole writer of the scan's lists: no global atomics) from 64 scans on — 256 threads when
  // the batch alone fills the GPU, 1024 (k_gather_wide) when it does not; only a handful of scans (streaming) is split
  // over several workgroups per scan.
  const uint32_t slices = batch >= 64u ? cfg.gather_slices_big : (batch >= 16u ? 4u : 16u);
  if (cfg.max_keypoints > cfg.gather_kcap) {  // (the wide workgroup, whatever the batch: its tables take most of a CU's LDS)
    p.gather = FX_GATHER_PASSES, p.gather_n = slices;
  } else if (cfg.gather_one == 256) {  // (test hook: the kind batches of 1024 scans and more take, at any batch size)
    p.gather = FX_GATHER_SLICED, p.gather_n = 1;
  } else if (cfg.gather_one == 1024) {  // (test hook: the kind batches of 64 to 1023 scans take)
    p.gather = FX_GATHER_WIDE, p.gather_n = 1;
  } else if (counted > 1u && cfg.gather_cnt) {
    p.gather = FX_GATHER_COUNTED, p.gather_n = umin(counted, cfg.gather_counted_max);
  } else if (slices == 1 && batch < 1024u) {
    p.gather = FX_GATHER_WIDE, p.gather_n = 1;
  } else {
    p.gather = FX_GATHER_SLICED, p.gather_n = slices;
  }
  p.rng_ord = p.gather_n > 1;
  // The dense tier (larger support sets and overflowed lists; nothing on sparse scans): its own three kernels, or a handful of
  // workgroups of k_desc's launch — the previous batches decide speed, never results.
  // (beside k_desc_mid, as it then was, on a second stream of the context: measured and dropped, profiles/r04_front_experiments.md)
  const uint32_t dense_rows = hint[FX_HINT_DENSE_ROWS], dense_points = hint[FX_HINT_DENSE_POINTS];
  bool fast = !live || dense_rows != 0u;  // (unknown: nothing known yet)
  if (fast && live && dense_rows != FX_HINT_UNKNOWN) st->dense_fast_left = FX_DENSE_LINGER;
  if (!fast && st->dense_fast_left) --st->dense_fast_left, fast = true;
  if (cfg.dense_force >= 0) fast = cfg.dense_force == 0;
  const bool skip_dense = (cfg.skip_mask & 2u) != 0u;
  // k_desc's group workgroups stride over the rows: ten a CU when the batch has the
  // chip to itself; with batches in flight fewer, longer-lived ones (measured, 1 / 2 / 3 / 4 batches in flight, scans/s with
  // 10 against 1 a CU: 1.64 / 1.47, 2.11 / 2.04, 2.25 / 2.27 — 2.29 with 3 —, 2.32 / 2.38e6: profiles/r05_experiments.md)
  const uint32_t desc_per_cu = cfg.desc_wgs_per_cu ? cfg.desc_wgs_per_cu : (cfg.batches_in_flight >= 4u ? 1u : (cfg.batches_in_flight == 3u ? 3u : 10u));
  // (never more workgroups than the batch can have rows for: sixteen rows a workgroup and trip — one scan per call launched
  //  2560 workgroups for its fifty rows)
  const uint64_t rows64 = (uint64_t)batch * cfg.max_keypoints;
  const uint32_t rows_bound = rows64 < cfg.max_total_keypoints ? (uint32_t)rows64 : cfg.max_total_keypoints;
  p.desc_group = umax(1u, umin(cfg.n_cu * desc_per_cu, (rows_bound + 15u) / 16u));
  if (cfg.desc_grid_abs) p.desc_group = cfg.desc_grid_abs;  // (test hook)
  // every tier in ONE launch: list rows (lists of up to dense_min entries, four keypoints per CU in flight), wave rows, the
  // group rows' striding workgroups, the dense stand-in (a scratch region each)
  p.desc_cap = umin(cfg.list_cap, cfg.dense_min);
  p.desc_wg = umax(1u, umin(big_grid * 4, rows_bound));
  p.desc_wave = umax(1u, umin(big_grid * 4, (rows_bound + 3u) / 4u));
  p.desc_dslow = umin(fast || skip_dense ? 0u : (cfg.tier_min_grid ? cfg.tier_min_grid : 8u), cfg.gsd_slots);
  p.dense = fast && !skip_dense;
  if (p.dense) {
    const uint32_t max_rows = batch * cfg.max_keypoints < cfg.max_total_keypoints ? batch * cfg.max_keypoints : cfg.max_total_keypoints;
    const uint32_t rows = tier_grid(dense_rows, 3 * big_grid, max_rows);
    // density items: 1024 queries each, at most one a row more than the support points fill
    const uint32_t items = dense_points == FX_HINT_UNKNOWN ? 3 * big_grid : tier_grid(dense_rows + dense_points / 1024u, 3 * big_grid, 0xffffffffu);
    // (rows and items are taken by ticket: any grid is correct; the full ones are what is resident at once)
    auto grid = [](uint32_t want, uint32_t full) { return want < full ? (want ? want : 1u) : full; };
    p.dense_sort_grid = grid(rows, cfg.n_cu * cfg.dsort_per_cu);
    p.dense_density_grid = grid(items, cfg.n_cu * cfg.ddens_per_cu);
    p.dense_finish_grid = grid(rows, cfg.n_cu);
    p.dense_skip = (cfg.skip_mask >> 2) & 3u;
  }
  return p;
}

#endif
