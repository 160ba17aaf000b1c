// fx_plan_selftest.cpp — the launch policy (fx_launch_plan.h) on a CPU: g++ -O2 -std=c++17 -Wall, no HIP, no GPU.
//
// Every expected value below was worked out by hand from the policy's expressions (for 256 CUs, tier_min_grid 8, one batch
// in flight and no hooks unless a case says otherwise), not by running fx_plan_batch: the policy decides speed only, so no
// parity test on the device can see a wrong grid — this is where one shows.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "fx_launch_plan.h"

static int g_failed = 0, g_checked = 0;
#define CHECK_EQ(got, want)                                                                                     \
  do {                                                                                                          \
    const long long g_ = (long long)(got), w_ = (long long)(want);                                              \
    ++g_checked;                                                                                                \
    if (g_ != w_) ++g_failed, printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g_, w_);     \
  } while (0)

static_assert(FX_N_HINTS == 8 && FX_HINT_RINGS_FIRST == 0 && FX_HINT_RINGS_SECOND == 1 && FX_HINT_BIG_MERGES == 2 && FX_HINT_HUGE_MERGES == 3 &&
                  FX_HINT_DENSE_ROWS == 4 && FX_HINT_DENSE_POINTS == 5 && FX_HINT_REDO_SCANS == 6 && FX_HINT_SLOW_SCANS == 7,
              "the slots the kernels write");

struct Hints {
  uint32_t v[FX_N_HINTS];
  explicit Hints(uint32_t all) {
    for (int i = 0; i < FX_N_HINTS; ++i) v[i] = all;
  }
  Hints &set(FxHint slot, uint32_t x) {
    v[slot] = x;
    return *this;
  }
};
static const uint32_t U = FX_HINT_UNKNOWN;

// a 16-ring sensor on 256 CUs: scans of 131 072 points, 50 keypoints a scan, room for everything
static FxPlanConfig base(bool front) {
  FxPlanConfig c;
  c.n_cu = 256, c.n_rings = 16, c.estimate_descriptors = true;
  c.max_points = 131072, c.max_keypoints = 50, c.max_total_keypoints = 50 * 1024, c.max_candidates = 4096, c.max_ring_points = 4096;
  c.merge_big_cap = 4096, c.list_cap = 4096, c.dense_min = 1024;
  c.gs_slots = 256, c.gsd_slots = 64;
  c.merge_hp = true, c.gather_cnt = true;
  c.prep_slices_max = 16, c.merge_slices_max = 8, c.gather_counted_max = 16, c.front_merge_cap = 512, c.gather_kcap = 2048, c.gather_slices_big = 1;
  c.dsort_per_cu = 4, c.ddens_per_cu = 3;
  c.batches_in_flight = 1, c.tier_min_grid = 8, c.front_ok = front;
  return c;
}
static FxLaunchPlan plan1(const FxPlanConfig &c, const Hints &h, uint32_t batch, bool capture = false) {
  FxPlanState st;
  return fx_plan_batch(c, &st, h.v, batch, capture);
}

static void test_desc_group_grid() {
  // rows_bound = min(batch * max_keypoints, max_total_keypoints); grid = max(1, min(n_cu * per, (rows_bound + 15) / 16))
  FxPlanConfig c = base(true);
  c.max_keypoints = 256, c.max_total_keypoints = 1024 * 256;  // (262144 + 15) / 16 = 16384 rows' worth: the CUs bound the grid
  const uint32_t per_cu[4] = {10, 10, 3, 1};
  for (uint32_t f = 1; f <= 4; ++f) {
    c.batches_in_flight = f;
    CHECK_EQ(plan1(c, Hints(0), 1024).desc_group, 256 * per_cu[f - 1]);
  }
  c.batches_in_flight = 7;
  CHECK_EQ(plan1(c, Hints(0), 1024).desc_group, 256);
  c = base(true);  // one scan of fifty rows: (50 + 15) / 16 = 4 workgroups, not 2560
  const FxLaunchPlan p = plan1(c, Hints(0), 1);
  CHECK_EQ(p.desc_group, 4);
  CHECK_EQ(p.desc_wg, 50);    // min(4 * 256, 50)
  CHECK_EQ(p.desc_wave, 13);  // min(4 * 256, (50 + 3) / 4)
  CHECK_EQ(p.desc_cap, 1024);
  c.max_total_keypoints = 1000;  // the pool bounds the rows: (1000 + 15) / 16 = 63
  CHECK_EQ(plan1(c, Hints(0), 1024).desc_group, 63);
  c.desc_wgs_per_cu = 2, c.max_total_keypoints = 1 << 20, c.max_keypoints = 1024;
  CHECK_EQ(plan1(c, Hints(0), 1024).desc_group, 512);
  c.desc_grid_abs = 77;
  CHECK_EQ(plan1(c, Hints(0), 1024).desc_group, 77);
}

static void test_redo_and_slow_grids() {
  FxPlanConfig c = base(true);
  // unknown: the full grid of 2 * 256, bounded by the batch
  CHECK_EQ(plan1(c, Hints(U), 1).redo_grid, 1);
  CHECK_EQ(plan1(c, Hints(U), 100).redo_grid, 100);
  CHECK_EQ(plan1(c, Hints(U), 1024).redo_grid, 512);
  // nothing handed on: four workgroups, one with four batches in flight
  CHECK_EQ(plan1(c, Hints(0), 1024).redo_grid, 4);
  CHECK_EQ(plan1(c, Hints(0), 3).redo_grid, 3);
  CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_REDO_SCANS, 3), 1024).redo_grid, 6);  // twice the count
  CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_REDO_SCANS, 257), 1024).redo_grid, 512);  // more than half the full grid: the full grid
  c.batches_in_flight = 4;
  CHECK_EQ(plan1(c, Hints(0), 1024).redo_grid, 1);
  c = base(true);
  c.skip_mask = 1;
  CHECK_EQ(plan1(c, Hints(0), 1024).redo_grid, 0);  // (no launch)
  // k_slow: eight, bounded by the batch, never above gs_slots — on both paths
  for (int front = 0; front < 2; ++front) {
    c = base(front != 0);
    CHECK_EQ(plan1(c, Hints(0), 1024).slow_grid, 8);
    CHECK_EQ(plan1(c, Hints(0), 3).slow_grid, 3);
    CHECK_EQ(plan1(c, Hints(U), 1024).slow_grid, 256);
    CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_SLOW_SCANS, 20), 1024).slow_grid, 40);
    c.gs_slots = 5;
    CHECK_EQ(plan1(c, Hints(0), 1024).slow_grid, 5);
    CHECK_EQ(plan1(c, Hints(U), 1024).slow_grid, 5);
    CHECK_EQ(plan1(c, Hints(U), 2).slow_grid, 2);
  }
  c = base(true);
  c.front_force = 1;
  CHECK_EQ(plan1(c, Hints(0), 9).force_redo, 1);
  CHECK_EQ(plan1(c, Hints(0), 9).force_slow, 0);
  c.front_force = 2;
  CHECK_EQ(plan1(c, Hints(0), 9).force_slow, 1);
}

static void test_separate_streaming_pass() {
  FxPlanConfig c = base(false);
  c.max_points = 65536;
  CHECK_EQ(plan1(c, Hints(0), 64).front, FX_FRONT_SEPARATE);
  CHECK_EQ(plan1(c, Hints(0), 64).prep_slices, 12);   // 3 * 256 / 64
  CHECK_EQ(plan1(c, Hints(0), 128).prep_slices, 6);   // 4 * 128 <= 2 * 256: 3 * 256 / 128
  CHECK_EQ(plan1(c, Hints(0), 129).prep_slices, 1);   // 516 > 512
  CHECK_EQ(plan1(c, Hints(0), 256).prep_slices, 1);
  CHECK_EQ(plan1(c, Hints(0), 1).prep_slices, 16);    // 768, the maximum is 16
  CHECK_EQ(plan1(c, Hints(0), 40).prep_slices, 16);   // 19
  c.max_points = 65535;
  CHECK_EQ(plan1(c, Hints(0), 64).prep_slices, 1);
  c.prep_slices = 40;
  CHECK_EQ(plan1(c, Hints(0), 1024).prep_slices, 16);
  c.prep_slices = 5;
  CHECK_EQ(plan1(c, Hints(0), 1024).prep_slices, 5);
  // the ring tiers: one wavefront a (scan, ring), grids in multiples of eight
  c = base(false);
  FxLaunchPlan p = plan1(c, Hints(0), 3);
  CHECK_EQ(p.runs_grid, 48);
  CHECK_EQ(p.runs2_grid, 0);
  CHECK_EQ(p.large_grid, 8);  // 8 * max(2 * 0, ceil(8 / 8)), the bound ceil(48 / 8) = 6
  CHECK_EQ(p.many_rings, 0);
  CHECK_EQ(p.merge_small_cap, 512);
  CHECK_EQ(p.merge_big_grid, 3);
  CHECK_EQ(p.merge_big_last, 1);
  CHECK_EQ(p.merge_huge_grid, 0);
  CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_RINGS_FIRST, 5), 1024).large_grid, 80);
  CHECK_EQ(plan1(c, Hints(U), 1024).large_grid, 256);  // 8 * ceil(256 / 8)
  CHECK_EQ(plan1(c, Hints(U), 1).large_grid, 16);      // 8 * ceil(16 / 8)
  // 32 rings: the second run tier takes the first tier's hint, the workgroup tier the second's; k_bucket_many
  c.n_rings = 32;
  p = plan1(c, Hints(0).set(FX_HINT_RINGS_FIRST, 5).set(FX_HINT_RINGS_SECOND, 3), 1024);
  CHECK_EQ(p.runs2_grid, 80);
  CHECK_EQ(p.large_grid, 48);
  CHECK_EQ(p.many_rings, 1);
  CHECK_EQ(p.runs_grid, 32768);
  CHECK_EQ(plan1(c, Hints(U), 1024).runs2_grid, 8 * 224);  // seven a CU: (256 * 7 + 7) / 8
  c.n_rings = 24;
  p = plan1(c, Hints(0), 1);
  CHECK_EQ(p.many_rings, 0);
  CHECK_EQ(p.runs_grid, 24);
  CHECK_EQ(p.runs2_grid, 8);
  c.max_candidates = 100;
  CHECK_EQ(plan1(c, Hints(0), 1).merge_small_cap, 100);
}

static void test_front_mode() {
  FxPlanConfig c = base(true);
  for (uint32_t b = 1; b <= 8; ++b) {
    CHECK_EQ(plan1(c, Hints(U), b).front, FX_FRONT_STREAMED);
    CHECK_EQ(plan1(c, Hints(U), b).prep_slices, 16);
  }
  CHECK_EQ(plan1(c, Hints(U), 9).front, FX_FRONT_FUSED);
  CHECK_EQ(plan1(c, Hints(U), 1024).front, FX_FRONT_FUSED);
  CHECK_EQ(plan1(c, Hints(U), 9).front_merge_cap, 512);
  c.max_candidates = 100;
  CHECK_EQ(plan1(c, Hints(U), 9).front_merge_cap, 100);
  c = base(true);
  c.front_stream = 0;
  CHECK_EQ(plan1(c, Hints(U), 1).front, FX_FRONT_FUSED);
  c.front_stream = 1;
  CHECK_EQ(plan1(c, Hints(U), 1000).front, FX_FRONT_STREAMED);
  c.front_split = 1;
  CHECK_EQ(plan1(c, Hints(U), 1).front, FX_FRONT_TWO);
  CHECK_EQ(plan1(c, Hints(U), 1000).front, FX_FRONT_TWO);
  c.front_split = 2;
  CHECK_EQ(plan1(c, Hints(U), 4).front, FX_FRONT_TWO_LEAN);
  c.front_ok = false;
  CHECK_EQ(plan1(c, Hints(U), 4).front, FX_FRONT_SEPARATE);
}

static void test_gather() {
  FxPlanConfig c = base(true);
  c.max_points = 65536;
  FxLaunchPlan p = plan1(c, Hints(0), 64);  // 10 * 64 <= 3 * 256: 768 / 64 = 12 counted slices
  CHECK_EQ(p.gather, FX_GATHER_COUNTED);
  CHECK_EQ(p.gather_n, 12);
  CHECK_EQ(p.rng_ord, 1);
  p = plan1(c, Hints(0), 76);  // 760 <= 768: 768 / 76 = 10
  CHECK_EQ(p.gather, FX_GATHER_COUNTED);
  CHECK_EQ(p.gather_n, 10);
  p = plan1(c, Hints(0), 77);  // 770 > 768: one wide workgroup a scan
  CHECK_EQ(p.gather, FX_GATHER_WIDE);
  CHECK_EQ(p.rng_ord, 0);
  p = plan1(c, Hints(0), 1);  // 768, the maximum is 16
  CHECK_EQ(p.gather, FX_GATHER_COUNTED);
  CHECK_EQ(p.gather_n, 16);
  c.batches_in_flight = 4;
  p = plan1(c, Hints(0), 64);
  CHECK_EQ(p.gather, FX_GATHER_WIDE);
  CHECK_EQ(p.gather_n, 1);
  CHECK_EQ(p.rng_ord, 0);
  c.batches_in_flight = 1;
  p = plan1(c, Hints(0), 64, true);  // under capture
  CHECK_EQ(p.gather, FX_GATHER_WIDE);
  CHECK_EQ(p.rng_ord, 0);
  c.gather_cnt = false;
  CHECK_EQ(plan1(c, Hints(0), 64).gather, FX_GATHER_WIDE);
  c.gather_cnt = true;
  c.max_points = 65535;  // small scans: by the batch alone — 16 workgroups a scan below 16 scans, 4 below 64, then one
  p = plan1(c, Hints(0), 15);
  CHECK_EQ(p.gather, FX_GATHER_SLICED);
  CHECK_EQ(p.gather_n, 16);
  CHECK_EQ(p.rng_ord, 1);
  p = plan1(c, Hints(0), 63);
  CHECK_EQ(p.gather, FX_GATHER_SLICED);
  CHECK_EQ(p.gather_n, 4);
  CHECK_EQ(plan1(c, Hints(0), 1023).gather, FX_GATHER_WIDE);
  p = plan1(c, Hints(0), 1024);  // the batch alone fills the chip: 256 threads a scan
  CHECK_EQ(p.gather, FX_GATHER_SLICED);
  CHECK_EQ(p.gather_n, 1);
  CHECK_EQ(p.rng_ord, 0);
  c.gather_slices = 7;  // the hook
  p = plan1(c, Hints(0), 1024, true);
  CHECK_EQ(p.gather, FX_GATHER_COUNTED);
  CHECK_EQ(p.gather_n, 7);
  // more keypoints than the LDS tables hold: passes, whatever else holds
  c.max_keypoints = 2049;
  p = plan1(c, Hints(0), 64);
  CHECK_EQ(p.gather, FX_GATHER_PASSES);
  CHECK_EQ(p.gather_n, 1);
  CHECK_EQ(p.rng_ord, 0);
  c.gather_slices = -1, c.max_points = 65536;
  p = plan1(c, Hints(0), 8);
  CHECK_EQ(p.gather, FX_GATHER_PASSES);
  CHECK_EQ(p.gather_n, 16);
  CHECK_EQ(p.rng_ord, 1);
  c.max_keypoints = 2048;
  CHECK_EQ(plan1(c, Hints(0), 8).gather, FX_GATHER_COUNTED);
  c.estimate_descriptors = false;
  CHECK_EQ(plan1(c, Hints(0), 8).descriptors, 0);
  // FX_GATHER_ONE: a one-workgroup kind at any batch size, also where the batch alone would pick counted slices or sixteen
  // staged workgroups a scan — but never beyond the LDS tables; unset (0), every plan above is what it was
  c = base(true);
  c.max_points = 65536;
  for (uint32_t batch : {1u, 3u, 16u, 64u, 1024u}) {
    for (int cap = 0; cap < 2; ++cap) {
      c.gather_one = 256;
      p = plan1(c, Hints(0), batch, cap != 0);
      CHECK_EQ(p.gather, FX_GATHER_SLICED);
      CHECK_EQ(p.gather_n, 1);
      CHECK_EQ(p.rng_ord, 0);
      c.gather_one = 1024;
      p = plan1(c, Hints(0), batch, cap != 0);
      CHECK_EQ(p.gather, FX_GATHER_WIDE);
      CHECK_EQ(p.gather_n, 1);
      CHECK_EQ(p.rng_ord, 0);
    }
  }
  c.gather_slices = 7;  // (it also beats the other hook)
  CHECK_EQ(plan1(c, Hints(0), 3).gather, FX_GATHER_WIDE);
  c.gather_slices = -1, c.max_keypoints = 2049;
  p = plan1(c, Hints(0), 3);
  CHECK_EQ(p.gather, FX_GATHER_PASSES);
  CHECK_EQ(p.gather_n, 16);
  c.gather_one = 256;
  CHECK_EQ(plan1(c, Hints(0), 64).gather, FX_GATHER_PASSES);
  c.gather_one = 0, c.max_keypoints = 50;
  CHECK_EQ(plan1(c, Hints(0), 3).gather, FX_GATHER_COUNTED);  // (768 / 3, the maximum is 16)
  CHECK_EQ(plan1(c, Hints(0), 3).gather_n, 16);
  CHECK_EQ(FxPlanConfig().gather_one, 0);
}

static void test_merge_huge() {
  FxPlanConfig c = base(false);
  c.merge_big_cap = 1024;  // below max_candidates: the large merge tier exists
  FxLaunchPlan p = plan1(c, Hints(0).set(FX_HINT_HUGE_MERGES, 4), 64);
  CHECK_EQ(p.merge_big_last, 0);
  CHECK_EQ(p.merge_huge_grid, 8);
  CHECK_EQ(p.merge_huge_slices, 8);  // 256 / 4 = 64, the maximum is 8
  CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_HUGE_MERGES, 64), 64).merge_huge_slices, 4);   // 2 * 64 <= 256: 256 / 64
  CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_HUGE_MERGES, 64), 64).merge_huge_grid, 64);    // 128, bounded by the batch
  CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_HUGE_MERGES, 129), 64).merge_huge_slices, 1);  // 258 > 256
  CHECK_EQ(plan1(c, Hints(U), 64).merge_huge_slices, 1);
  CHECK_EQ(plan1(c, Hints(U), 64).merge_huge_grid, 64);
  CHECK_EQ(plan1(c, Hints(0), 64).merge_huge_slices, 1);
  CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_HUGE_MERGES, 4), 64, true).merge_huge_slices, 1);
  c.batches_in_flight = 4;  // 256 / (4 * 4) = 16, the maximum is 8; 40 scans: 2 * 40 * 4 > 256
  CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_HUGE_MERGES, 4), 64).merge_huge_slices, 8);
  CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_HUGE_MERGES, 32), 64).merge_huge_slices, 2);
  CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_HUGE_MERGES, 40), 64).merge_huge_slices, 1);
  c.batches_in_flight = 1;
  c.merge_hp = false;
  CHECK_EQ(plan1(c, Hints(0).set(FX_HINT_HUGE_MERGES, 4), 64).merge_huge_slices, 1);
  c.merge_slices = 5;
  CHECK_EQ(plan1(c, Hints(0), 64).merge_huge_slices, 1);
  c.merge_hp = true;
  CHECK_EQ(plan1(c, Hints(0), 64, true).merge_huge_slices, 5);
  c.merge_slices = 40;
  CHECK_EQ(plan1(c, Hints(0), 64).merge_huge_slices, 8);
}

static void test_hint_hold() {
  // merge_big_grid = 2 * held count, at least 8, for a batch of 1024 scans
  const FxPlanConfig c = base(false);
  FxPlanState st;
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).set(FX_HINT_BIG_MERGES, 10).v, 1024, false).merge_big_grid, 20);
  for (int i = 1; i <= 64; ++i) CHECK_EQ(fx_plan_batch(c, &st, Hints(0).v, 1024, false).merge_big_grid, 20);
  CHECK_EQ(st.hint_hold[FX_HINT_BIG_MERGES], 10);
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).v, 1024, false).merge_big_grid, 8);  // the 65th
  CHECK_EQ(st.hint_hold[FX_HINT_BIG_MERGES], 0);
  // a larger count replaces a held one at once, and starts its own 64 batches
  st = FxPlanState();
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).set(FX_HINT_BIG_MERGES, 10).v, 1024, false).merge_big_grid, 20);
  for (int i = 0; i < 40; ++i) fx_plan_batch(c, &st, Hints(0).v, 1024, false);
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).set(FX_HINT_BIG_MERGES, 30).v, 1024, false).merge_big_grid, 60);
  for (int i = 1; i <= 64; ++i) CHECK_EQ(fx_plan_batch(c, &st, Hints(0).v, 1024, false).merge_big_grid, 60);
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).v, 1024, false).merge_big_grid, 8);
  // a held "unknown" is the full grid only until something is known
  st = FxPlanState();
  CHECK_EQ(fx_plan_batch(c, &st, Hints(U).v, 1024, false).merge_big_grid, 256);
  CHECK_EQ(fx_plan_batch(c, &st, Hints(U).set(FX_HINT_BIG_MERGES, 5).v, 1024, false).merge_big_grid, 10);
  CHECK_EQ(fx_plan_batch(c, &st, Hints(U).v, 1024, false).merge_big_grid, 256);  // (and unknown again replaces a count at once)
  st.reset();
  CHECK_EQ(st.hint_hold[FX_HINT_BIG_MERGES], U);
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).v, 1024, false).merge_big_grid, 8);
  // tier_min_grid 0: always the full grids, and nothing is held
  FxPlanConfig z = base(false);
  z.tier_min_grid = 0;
  st = FxPlanState();
  CHECK_EQ(fx_plan_batch(z, &st, Hints(0).set(FX_HINT_BIG_MERGES, 10).v, 1024, false).merge_big_grid, 256);
  CHECK_EQ(st.hint_hold[FX_HINT_BIG_MERGES], 0);
  // an empty batch launches nothing and still ages the holds
  st = FxPlanState();
  fx_plan_batch(c, &st, Hints(0).set(FX_HINT_BIG_MERGES, 10).v, 1024, false);
  fx_plan_batch(c, &st, Hints(0).v, 0, false);
  CHECK_EQ(st.hint_age[FX_HINT_BIG_MERGES], 1);
}

static void test_dense_tier() {
  FxPlanConfig c = base(true);
  FxPlanState st;
  // five rows of 5000 support points: the tier's kernels, 2 * 5 rows' workgroups, 2 * (5 + 5000 / 1024) density items
  FxLaunchPlan p = fx_plan_batch(c, &st, Hints(0).set(FX_HINT_DENSE_ROWS, 5).set(FX_HINT_DENSE_POINTS, 5000).v, 1024, false);
  CHECK_EQ(p.dense, 1);
  CHECK_EQ(p.desc_dslow, 0);
  CHECK_EQ(p.dense_sort_grid, 10);
  CHECK_EQ(p.dense_density_grid, 18);
  CHECK_EQ(p.dense_finish_grid, 10);
  CHECK_EQ(st.dense_fast_left, 64);
  // zeros: the count is held for 64 batches, then the kernels linger for 64 more on the floor of eight workgroups
  for (int i = 1; i <= 64; ++i) {
    p = fx_plan_batch(c, &st, Hints(0).v, 1024, false);
    CHECK_EQ(p.dense, 1);
    CHECK_EQ(p.dense_sort_grid, 10);
    CHECK_EQ(st.dense_fast_left, 64);
  }
  for (int i = 1; i <= 64; ++i) {
    p = fx_plan_batch(c, &st, Hints(0).v, 1024, false);
    CHECK_EQ(p.dense, 1);
    CHECK_EQ(p.desc_dslow, 0);
    CHECK_EQ(p.dense_sort_grid, 8);
    CHECK_EQ(p.dense_density_grid, 8);
    CHECK_EQ(p.dense_finish_grid, 8);
    CHECK_EQ(st.dense_fast_left, 64 - i);
  }
  p = fx_plan_batch(c, &st, Hints(0).v, 1024, false);  // after that: the stand-in in k_desc's launch
  CHECK_EQ(p.dense, 0);
  CHECK_EQ(p.desc_dslow, 8);
  // nothing known: the tier's kernels at their full grids (3 * 256 rows' worth, bounded by the rows the batch can have), no linger armed
  st = FxPlanState();
  p = fx_plan_batch(c, &st, Hints(U).v, 1024, false);
  CHECK_EQ(p.dense, 1);
  CHECK_EQ(p.dense_sort_grid, 768);     // of 256 * 4
  CHECK_EQ(p.dense_density_grid, 768);  // 256 * 3
  CHECK_EQ(p.dense_finish_grid, 256);
  CHECK_EQ(st.dense_fast_left, 0);
  CHECK_EQ(plan1(c, Hints(U), 2).dense_sort_grid, 100);  // two scans of fifty keypoints
  CHECK_EQ(plan1(c, Hints(U), 2).dense_density_grid, 768);
  // a context that never had a dense row: the stand-in from the first known count on, min(8, gsd_slots) workgroups
  CHECK_EQ(plan1(c, Hints(0), 1024).dense, 0);
  CHECK_EQ(plan1(c, Hints(0), 1024).desc_dslow, 8);
  c.gsd_slots = 4;
  CHECK_EQ(plan1(c, Hints(0), 1024).desc_dslow, 4);
  c.gsd_slots = 64, c.tier_min_grid = 16;
  CHECK_EQ(plan1(c, Hints(0), 1024).desc_dslow, 16);
  // the hooks
  c = base(true);
  c.dense_force = 1;
  p = plan1(c, Hints(0).set(FX_HINT_DENSE_ROWS, 5), 1024);
  CHECK_EQ(p.dense, 0);
  CHECK_EQ(p.desc_dslow, 8);
  c.dense_force = 0;
  p = plan1(c, Hints(0), 1024);
  CHECK_EQ(p.dense, 1);
  CHECK_EQ(p.desc_dslow, 0);
  c.dense_force = -1, c.skip_mask = 2;
  p = plan1(c, Hints(0).set(FX_HINT_DENSE_ROWS, 5), 1024);
  CHECK_EQ(p.dense, 0);
  CHECK_EQ(p.desc_dslow, 0);
  p = plan1(c, Hints(0), 1024);
  CHECK_EQ(p.dense, 0);
  CHECK_EQ(p.desc_dslow, 0);
  c.skip_mask = 4 | 8;
  CHECK_EQ(plan1(c, Hints(U), 1024).dense_skip, 3);
}

static void test_front_pause() {
  FxPlanConfig c = base(true);
  FxPlanState st;
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).v, 64, false).front, FX_FRONT_FUSED);
  CHECK_EQ(st.front_last, 1);
  CHECK_EQ(st.last_batch, 64);
  // 8 of 64 scans handed on is an eighth: no pause; 9 is more
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).set(FX_HINT_REDO_SCANS, 8).v, 64, false).front, FX_FRONT_FUSED);
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).set(FX_HINT_REDO_SCANS, 9).v, 64, false).front, FX_FRONT_SEPARATE);
  CHECK_EQ(st.front_pause, 64);
  CHECK_EQ(st.front_last, 0);
  for (int i = 1; i <= 64; ++i) {
    CHECK_EQ(fx_plan_batch(c, &st, Hints(0).set(FX_HINT_REDO_SCANS, 9).v, 64, false).front, FX_FRONT_SEPARATE);
    CHECK_EQ(st.front_pause, 64 - i);
  }
  // the 66th runs the front again, whatever the (stale) count says: the last batch did not run it
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).set(FX_HINT_REDO_SCANS, 9).v, 64, false).front, FX_FRONT_FUSED);
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).set(FX_HINT_REDO_SCANS, 9).v, 64, false).front, FX_FRONT_SEPARATE);  // and pauses again
  // the count is held against the LAST batch's size
  st = FxPlanState();
  fx_plan_batch(c, &st, Hints(0).v, 8, false);
  CHECK_EQ(fx_plan_batch(c, &st, Hints(0).set(FX_HINT_REDO_SCANS, 2).v, 1024, false).front, FX_FRONT_SEPARATE);  // 2 > (8 + 7) / 8
  st = FxPlanState();
  fx_plan_batch(c, &st, Hints(0).v, 1024, false);
  CHECK_EQ(fx_plan_batch(c, &st, Hints(U).v, 8, false).front, FX_FRONT_STREAMED);  // nothing known: no pause
  // FX_FRONT_FORCE: never paused
  c.front_force = 1;
  st = FxPlanState();
  for (int i = 0; i < 4; ++i) CHECK_EQ(fx_plan_batch(c, &st, Hints(0).set(FX_HINT_REDO_SCANS, 64).v, 64, false).front, FX_FRONT_FUSED);
  CHECK_EQ(st.front_pause, 0);
  // reset ends a pause
  c.front_force = 0;
  st = FxPlanState();
  fx_plan_batch(c, &st, Hints(0).v, 64, false);
  fx_plan_batch(c, &st, Hints(0).set(FX_HINT_REDO_SCANS, 64).v, 64, false);
  CHECK_EQ(st.front_pause, 64);
  st.reset();
  CHECK_EQ(fx_plan_batch(c, &st, Hints(U).v, 64, false).front, FX_FRONT_FUSED);
}

static void test_capture() {
  FxPlanConfig c = base(true);
  FxPlanState st;
  // some history first, so there is state a capture could disturb: held counts, a linger, a pause
  fx_plan_batch(c, &st, Hints(3).v, 64, false);
  fx_plan_batch(c, &st, Hints(40).v, 64, false);
  fx_plan_batch(c, &st, Hints(0).v, 64, false);
  CHECK_EQ(st.front_pause, 63);
  CHECK_EQ(st.dense_fast_left, 64);
  CHECK_EQ(st.hint_age[FX_HINT_BIG_MERGES], 1);
  FxPlanState before;
  memcpy(&before, &st, sizeof(st));
  const uint32_t batches[6] = {1, 9, 64, 100, 1024, 0};
  for (int front = 0; front < 2; ++front) {
    c.front_ok = front != 0;  // (a capture's front is the config's: the pause is the live batches')
    c.merge_big_cap = 1024;
    for (int i = 0; i < 6; ++i) {
      const uint32_t b = batches[i];
      const FxLaunchPlan p = fx_plan_batch(c, &st, Hints(1).v, b, true);
      CHECK_EQ(memcmp(&before, &st, sizeof(st)), 0);
      if (!b) continue;
      const uint32_t b256 = b < 256 ? b : 256, b512 = b < 512 ? b : 512;
      CHECK_EQ(p.slow_grid, b256);
      if (front) {
        CHECK_EQ(p.front, b <= 8 ? FX_FRONT_STREAMED : FX_FRONT_FUSED);
        CHECK_EQ(p.redo_grid, b512);
      } else {
        CHECK_EQ(p.front, FX_FRONT_SEPARATE);
        CHECK_EQ(p.merge_big_grid, b256);
        CHECK_EQ(p.merge_huge_grid, b256);
        CHECK_EQ(p.merge_huge_slices, 1);
        CHECK_EQ(p.large_grid, 2 * b < 32 ? 8 * 2 * b : 256);  // 16 rings: ceil(16 b / 8) lists' worth, at most 8 * 32
      }
      CHECK_EQ(p.dense, 1);
      CHECK_EQ(p.desc_dslow, 0);
      CHECK_EQ(p.dense_sort_grid, 50 * b < 768 ? 50 * b : 768);
      CHECK_EQ(p.dense_density_grid, 768);
      CHECK_EQ(p.dense_finish_grid, 50 * b < 256 ? 50 * b : 256);
    }
  }
}

int main() {
  test_desc_group_grid();
  test_redo_and_slow_grids();
  test_separate_streaming_pass();
  test_front_mode();
  test_gather();
  test_merge_huge();
  test_hint_hold();
  test_dense_tier();
  test_front_pause();
  test_capture();
  printf("%d checks, %d failed\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
