// fx_device.h — structures shared by the host driver and the gfx950 kernels.
#ifndef FX_DEVICE_H_
#define FX_DEVICE_H_
#include <stdint.h>

#include "../../include/fx.h"
#include "fx_launch_plan.h"  // FX_N_HINTS and the names of tier_hint[]'s slots (FxHint)

// One scan of the batch as the kernels see it.
struct FxScanMeta {
  const float *pts;   // device pointer, records of stride_f floats, x y z at 0 1 2
  uint32_t n;         // points in the scan
  uint32_t stride_f;  // record stride in floats (4 or 8)
  float R[9];         // rotateCloud matrix, row major (ref: node.cpp:161-165)
  uint32_t pad_;
};

// Per-context constants (narrowed exactly where PCL narrows them, see fx_api.cpp).
struct FxDevParams {
  // filterCloud limits as PassThrough stores them (float) (ref: node.cpp:169-183)
  float x_min, x_max, y_min, y_max, z_min, z_max;
  int32_t n_rings;
  // getCylinderSegments (ref: node.cpp:269-276, 314-316)
  float r2_cluster;
  uint32_t min_count, max_count;
  double gate_diameter;  // 2 * cluster_radius_threshold
  // secondary merge (ref: node.cpp:217, 222-229)
  double crt;
  float r2_merge;
  uint32_t ndc, secondary_max;
  // 3DSC (ref: node.cpp:350-352)
  float r2_search, r2_density, r2_support;
  int32_t estimate_descriptors;
  // capacities
  uint32_t max_points, max_ring_cands, max_candidates, max_keypoints, max_total_kp, max_kpc, max_neighbors,
      max_ring_points, list_cap, ring_slot_cap;
  uint32_t ring_list_cap;  // entries per XCD class of the deferred-ring lists
  uint32_t near_words;  // words of near bits per scan: one bit per 4 consecutive points = one 64-byte sector (k_prep -> k_gather)
  // dense tier (k_dense_*): support sets beyond dense_min points and lists that overflowed list_cap
  uint32_t dense_min;       // rows with more support points than this take the dense tier (1024)
  uint32_t ovf_cap;         // entries of a scan's overflow region (list entries beyond list_cap, any row of the scan)
  uint32_t dense_cap;       // entries of the sorted pool (and of the key pool) per batch
  uint32_t max_dense_rows;  // rows of the dense-row list / cell tables
  uint32_t dense_qcap;      // entries of the query pool (every cell's queries padded to four: up to 4 per support point)
  uint32_t dense_lds_keys;  // binned neighbours k_dense_finish sorts in LDS (14336; tests lower it to reach the key pool)
  uint32_t dense_won_points;  // support points of a row whose query marks k_dense_sort keeps as a bit map in LDS (65536; tests lower it)
  // slow tier (k_slow): scratch regions in HBM for what exceeds every LDS-sized tier
  uint32_t gs_slots;  // regions (= the largest grid k_slow is launched with)
  uint32_t gs_words;  // words per region
  uint32_t gsd_slots, gsd_words;  // the same for dense_slow_loop (the dense descriptor tier's rows without its four launches)
};

// 3DSC tables in device memory (built on the host by fx_sc3d_tables / fx_sc3d_xaxis).
struct FxScTables {
  float radii[16];
  float theta[12];
  float phi[13];
  float lut[165];  // [k*15 + j]; identical for every azimuth bin
};

// Every device buffer of a context.
#define FX_CLK_SLOTS 64
#define FX_N_COUNTERS 48  // counters k_prep / k_front clear for the batch
#define FX_CNT_REDO 48    // counters[48]: scans k_front hands to k_front_redo, [49]: scans handed to the slow tier, k_slow (cleared by k_offsets, after their readers)
#define FX_CNT_SLOW_TICKET 50  // counters[50]: workgroups of k_slow's launch that are done (the last one computes the batch's keypoint offsets and puts it back to 0)
#define FX_N_COUNTER_WORDS 56
#define FX_CNT_RUNS2_TICKET 40  // counters[40 + c]: next ring of XCD class c's list for k_rings_runs2
#define FX_CNT_GROUP 33  // counters[33 + c]: group rows of size class c (FxBuffers::group_desc; 0: <= 16 support points, 1: <= 32, 2: <= 64)
#define FX_GROUP_CLASSES 3
#define FX_ATAN_N 64      // table step of k_prep's arctangent: 1 / 64 over [0, 1]
#define FX_ATAN_DEG 6     // degree of the expansion about a table point (|offset| <= 1 / 128: truncation below 2^-51)
#define FX_ROW_DIRTY 0xffffffffu
// FxBuffers::row_class: which workgroups of k_desc own a row — clear it, compute it, record what they left in it
#define FX_ROW_GROUP 0u       // support sets of up to FX_GROUP_CAP points
#define FX_ROW_WAVE 1u        // up to FX_WAVE_CAP
#define FX_ROW_LIST 2u        // up to dense_min
#define FX_ROW_DENSE 3u       // beyond that, and every overflowed list: the dense tier (its own kernels or k_desc's stand-in workgroups)
#define FX_ROW_DENSE_FAIL 4u  // a dense row the pools have no room for: flagged, NaN-filled by the group workgroups
// CSR block of descriptor rows (include/fx.h fx_descriptor_csr_bytes): words of row_ptr[max_rows + 1] and of col / val[cap],
// each rounded up to 16 bytes; header 16 B, then row_ptr, col, val
__host__ __device__ inline size_t csr_rp_words(uint32_t max_rows) { return ((size_t)max_rows + 1u + 3u) & ~(size_t)3; }
__host__ __device__ inline size_t csr_cap_words(uint32_t cap) { return ((size_t)cap + 3u) & ~(size_t)3; }
// Compact keypoint block (include/fx.h fx_pack_keypoint_block; k_pack_kp_block writes it): float4 rows.  Row 0 the header words,
// then kp_offset[max_scans + 1] and flags[max_scans], four words a row each, then max_total (x, y, z, elevation) rows.  This is
// the layout's one definition on the device and in the host driver (Python: capi.keypoint_block_layout).
__host__ __device__ inline uint32_t kp_block_off_rows(uint32_t max_scans) { return (max_scans + 1u + 3u) / 4u; }
__host__ __device__ inline uint32_t kp_block_flag_rows(uint32_t max_scans) { return (max_scans + 3u) / 4u; }
__host__ __device__ inline uint32_t kp_block_first_row(uint32_t max_scans) { return 1u + kp_block_off_rows(max_scans) + kp_block_flag_rows(max_scans); }
__host__ __device__ inline size_t kp_block_bytes(uint32_t max_scans, uint32_t max_total) { return ((size_t)kp_block_first_row(max_scans) + max_total) * 16; }
// What the back end's kernels (fx_match / fx_register / fx_track / fx_map .hip) share.
// a block's kp_offset section and its keypoint rows, as float4 or as the uint4 words they are
__device__ __forceinline__ const uint32_t *kp_block_offsets(const uint32_t *block) { return block + 4; }
template <typename Row>
__device__ __forceinline__ const Row *kp_block_rows(const uint32_t *block, uint32_t max_scans) {
  return reinterpret_cast<const Row *>(block) + kp_block_first_row(max_scans);
}
__device__ __forceinline__ bool finite3(float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }
// the rows [row0, row0 + n) of a pair that lie below `stored`
__device__ __forceinline__ void clip_range(uint32_t row0, uint32_t n, uint32_t stored, uint32_t &lo, uint32_t &hi) {
  hi = (uint32_t)min((unsigned long long)row0 + n, (unsigned long long)stored);
  lo = min(row0, hi);
}
// The world-frame point of an observation: keypoint row p under the pose P of its scan, fp64, in exactly this operation order
// (the build's -ffp-contract=off keeps every operation its own rounding).  include/fx.h promises that the map equals one long
// track bit for bit: that holds because k_track_fuse and k_map_accumulate both take the point from here.
__device__ __forceinline__ void world_point(const fx_pose &P, float4 p, double &wx, double &wy, double &wz) {
  const double x = (double)p.x, y = (double)p.y;
  wx = (P.c * x - P.s * y) + P.tx;
  wy = (P.s * x + P.c * y) + P.ty;
  wz = (double)p.z + P.tz;
}
// The public record of a map landmark from its running sums (include/fx.h fx_map_update, "Records"): the means, and the spread
// about the mean through the anchor.  k_map_accumulate and fx_map_merge's fold both take the record from here.
__device__ __forceinline__ void map_record_from_sums(fx_map_landmark &R, double sx, double sy, double sz, double dsx, double dsy, double q) {
  const double dn = (double)R.n_obs;
  const double mx = dsx / dn, my = dsy / dn;
  const double var = q / dn - (mx * mx + my * my);
  R.x = sx / dn, R.y = sy / dn, R.z = sz / dn;
  R.rms_xy = (float)sqrt(var > 0.0 ? var : 0.0);
}
// exclusive prefix of (a, b) over the threads of a workgroup of NWAVE wavefronts, and the totals; s_w: [2][NWAVE] words of LDS
template <uint32_t NWAVE>
__device__ __forceinline__ void wg_scan2(uint32_t a, uint32_t b, uint32_t *s_w, uint32_t &ex_a, uint32_t &ex_b, uint32_t &tot_a, uint32_t &tot_b) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t ia = a, ib = b;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t ua = (uint32_t)__shfl_up((int)ia, o, 64), ub = (uint32_t)__shfl_up((int)ib, o, 64);
    if (lane >= (uint32_t)o) ia += ua, ib += ub;
  }
  __syncthreads();  // (s_w's readers of the call before)
  if (lane == 63u) s_w[wave] = ia, s_w[NWAVE + wave] = ib;
  __syncthreads();
  ex_a = ia - a, ex_b = ib - b, tot_a = tot_b = 0u;
#pragma unroll
  for (uint32_t w = 0; w < NWAVE; ++w) {
    const uint32_t na = s_w[w], nb = s_w[NWAVE + w];
    ex_a += w < wave ? na : 0u, ex_b += w < wave ? nb : 0u;
    tot_a += na, tot_b += nb;
  }
}
// one workgroup: the blocks' counts bsum[2][n_blocks] to their exclusive prefix, in place, and the totals
template <uint32_t NWAVE>
__device__ __forceinline__ void wg_scan2_blocks(uint32_t *bsum, uint32_t n_blocks, uint32_t *s_w, uint32_t &tot_a, uint32_t &tot_b) {
  uint32_t base_a = 0u, base_b = 0u;
  for (uint32_t i0 = 0u; i0 < n_blocks; i0 += NWAVE * 64u) {
    const uint32_t i = i0 + threadIdx.x;
    const uint32_t a = i < n_blocks ? bsum[i] : 0u, b = i < n_blocks ? bsum[n_blocks + i] : 0u;
    uint32_t ea, eb, ta, tb;
    wg_scan2<NWAVE>(a, b, s_w, ea, eb, ta, tb);
    if (i < n_blocks) bsum[i] = base_a + ea, bsum[n_blocks + i] = base_b + eb;
    base_a += ta, base_b += tb;
  }
  tot_a = base_a, tot_b = base_b;
}
// The carving of a call's arrays out of the context's scratch (the fxk_*_scratch functions; host only): take<T>(count) hands out the
// next `count` elements and steps to the next 16-byte boundary.  With base null only the bytes are counted.
struct FxCarve {
  uint8_t *base;
  size_t o;
  template <typename T>
  T *take(size_t count) {
    const size_t at = o;
    o += (count * sizeof(T) + 15u) & ~(size_t)15;
    return base ? reinterpret_cast<T *>(base + at) : nullptr;
  }
};
// fx_match_descriptors_csr (csrc/fx_match.hip): one pair of row ranges as the kernels see it, and a launch's arguments.
struct FxMatchPairDev {
  uint32_t q_row0, q_rows, t_row0, t_rows;
  uint32_t mut_off;  // first slot of the pair's train rows in the mutual table
  uint32_t pad_[3];
};
struct FxMatchArgs {
  const uint32_t *q_block, *t_block;  // CSR blocks (include/fx.h fx_descriptor_csr_bytes)
  uint32_t q_max_rows, q_cap, t_max_rows, t_cap;
  const FxMatchPairDev *pairs;
  const uint2 *items;          // work list: (pair, tile of query rows)
  const double *q_norm, *t_norm;  // squared norm of each stored row's bins; NaN: the row stores a NaN
  unsigned long long *mut;     // [sum of the pairs' train rows] (fp32 bits of dist2 << 32) | query row, atomic min
  void *out;                   // fx_match [q_max_rows]
  float max_dist2, max_ratio;
  uint32_t mutual;
};
// fx_register_matches (csrc/fx_register.hip): a launch's arguments.
struct FxRegisterArgs {
  const uint32_t *q_kp, *t_kp;  // keypoint blocks (include/fx.h fx_pack_keypoint_block)
  uint32_t q_max_scans, q_max_total, t_max_scans, t_max_total;
  const void *matches;          // fx_match [q_max_rows]
  uint32_t q_max_rows;
  const void *pairs;            // fx_match_pair [n_pairs], a workgroup each
  void *out;                    // fx_registration [n_pairs]
  uint32_t *inlier;             // [q_max_rows] or null
  float inlier_dist, min_baseline;
  uint32_t hyp_corr, min_inliers, require_flags;
};
// A keypoint block read as a query (csrc/fx_scan_query.h): the block, the sizes it was packed with, and the caller's scans and rows.
struct FxKpQuery {
  const uint32_t *kp;           // keypoint block (include/fx.h fx_pack_keypoint_block)
  uint32_t max_scans, max_total;
  uint32_t n_scans, q_max_rows;
};
// fx_track_landmarks (csrc/fx_track.hip): a launch set's arguments.  The scratch arrays are the context's, [q_max_rows] each.
struct FxTrackArgs {
  FxKpQuery K;
  const void *matches;          // fx_match [q_max_rows]
  const uint32_t *inlier;       // [q_max_rows]
  const void *reg;              // fx_registration [n_scans - 1]
  uint32_t min_obs, max_landmarks;
  double init[5];               // P_0: c, s, tx, ty, tz
  void *poses;                  // fx_pose [n_scans]
  int32_t *landmark_of_row;     // [q_max_rows]
  uint32_t *obs_row;            // [q_max_rows]
  void *landmarks;              // fx_landmark [max_landmarks]
  void *header;                 // fx_track_header
  // scratch
  uint32_t *scan_of;            // the row's scan, FX_TRACK_NONE: a non-row
  uint32_t *child;              // lowest proposer of the row as a parent (atomic min), FX_TRACK_NONE: none
  int32_t *prop;                // the parent the row proposes, -1: none
  uint2 *jump[2];               // (root so far, depth so far), ping-pong
  uint32_t *len;                // observations of the track rooted at the row
  int32_t *lm_id;               // landmark number of the track rooted at the row, -1: none
  uint32_t *obs0;               // first obs_row slot of the landmark rooted at the row
  uint32_t *lm_root;            // landmark number -> its first row
  uint32_t *bsum;               // [2][blocks of FXT_WG rows]: landmarks / observations that begin in the block
  uint32_t *counters;           // [0] conflicts, [1] gaps
};
// fx_map_update (csrc/fx_map.hip): a launch set's arguments.  The first group is the map's own memory (fx_map_create), the last
// the context's scratch, sized by the call's max_landmarks.
#define FX_MAP_ACC 8       // doubles of a landmark's private accumulators: Sx, Sy, Sz, ax, ay, Dx, Dy, Q
#define FX_MAP_ST_WORDS 8  // state words between the launches of one update: 0 the overlap scan differs, 1 overlap accepted,
                           // 2 scan_base, 3 seg_base, 4 new landmarks, 5 continued landmarks, 7 observations accumulated
struct FxMapArgs {
  void *header;                 // fx_map_header
  void *records;                // fx_map_landmark [cap]
  double *acc;                  // [cap][FX_MAP_ACC]
  int32_t *carry;               // [max_carry]: map id of local row j of the carry scan, -1: none
  uint4 *carry_kp;              // [max_carry]: the carry scan's rows as they were in the block
  uint32_t *st;                 // [FX_MAP_ST_WORDS]; words 0 and 7 are 0 between updates
  int32_t *alias;               // [cap]: -1 live, else the live landmark that absorbed it (fx_map_merge; the update never touches it)
  uint32_t cap, max_carry;
  const uint32_t *kp;           // keypoint block (include/fx.h fx_pack_keypoint_block)
  uint32_t max_scans, max_total;
  const void *poses;            // fx_pose [>= S]
  const int32_t *landmark_of_row;  // [q_max_rows]
  const uint32_t *obs_row;      // [q_max_rows]
  uint32_t q_max_rows;
  const void *landmarks;        // fx_landmark [max_landmarks]
  uint32_t max_landmarks;
  const void *track_header;     // fx_track_header
  uint32_t flags;
  int32_t *map_id_of_row;       // [q_max_rows] or null
  int32_t *id_of_lm;            // [max_landmarks]: k_map_join's verdict (>= 0 continues that id, -1 new, -2 not a landmark), then the map id or -1
  uint32_t *bsum;               // [2][blocks of FXMAP_WG landmarks]: new / continued landmarks of the block
};
// fx_map_merge (csrc/fx_map_merge.hip): a launch set's arguments.  The first group is the map's own memory, the last the context's
// scratch, sized by the map's max_landmarks (cap) and the hash table's `table` buckets (a power of two; bucket `table` is the far list).
#define FX_MAP_MERGE_ST_WORDS 4  // 0 proposals, 1 kept links, 2 live landmarks after the call, 3 landmarks in the grid
struct FxMapMergeCand {         // a landmark that takes part, as the search reads it: 32 B, in bucket order
  double x, y;
  uint32_t last_scan, segment, id, pad_;
};
struct FxMapMergeArgs {
  const void *header;           // fx_map_header (read only: ids are stable)
  void *records;                // fx_map_landmark [cap]
  double *acc;                  // [cap][FX_MAP_ACC]
  int32_t *carry;               // [max_carry]
  int32_t *alias;               // [cap]
  uint32_t cap, max_carry;
  double md2, inv_edge;         // the gate (double)merge_dist squared; 1 / the cell edge
  uint32_t max_gap, table;
  uint32_t *result;             // fx_map_merge_result or null
  uint32_t *st;                 // [FX_MAP_MERGE_ST_WORDS]
  uint32_t *count;              // [table + 1]: landmarks of the bucket (the scatter counts it down to 0)
  uint32_t *start;              // [table + 1]: the bucket's first slot within its block of buckets
  uint32_t *bsum;               // [2][blocks of buckets]: the block's landmarks, then its first slot (the second row is unused: 0)
  uint32_t *bucket;             // [cap]: the landmark's bucket, FX_TRACK_NONE: takes no part
  FxMapMergeCand *cand;         // [cap]
  int32_t *prop;                // [cap]: the g landmark h proposes, -1: none
  unsigned long long *keep;     // [cap]: (first_scan << 32) | h of g's proposers, atomic min
  int32_t *pred, *succ;         // [cap]: the kept link into / out of the landmark, -1: none
  // a grid over points that are no landmarks (fx_map_discover's free rows); points null: the grid is over the map's landmarks
  const double2 *points;        // [cap]: (x, y) of item i; every one takes part
  const uint32_t *n_points;     // how many there are, read on the device and clipped to cap
};
// fx_map_localize (csrc/fx_map_localize.hip): a launch set's arguments.  G describes the grid over the map (its gate is the
// search distance; the merge's per-landmark arrays are null); the last group is the context's scratch, [q_max_rows] each.
struct FxMapLocalizeArgs {
  FxMapMergeArgs G;
  FxKpQuery K;
  const void *priors;           // fx_pose [n_scans]
  float inlier_dist, min_baseline;
  uint32_t hyp_corr, min_inliers, min_landmark_obs, segment;
  void *out;                    // fx_localization [n_scans]
  int32_t *map_id_of_row;       // [q_max_rows]
  int32_t *nearest_of_row;      // [q_max_rows] or null
  int32_t *near;                // the row's landmark, -1: none
  unsigned long long *d2;       // its squared xy distance as bits
};
// fx_map_follow (csrc/fx_map_follow.hip): a launch set's arguments.  L is the localise's (L.priors is null: the chain forms its
// priors; L.out, the row arrays and the scratch as there); the options are fx.h's, checked, chain_scans resolved to >= 1.
struct FxMapFollowArgs {
  FxMapLocalizeArgs L;
  const void *links;            // fx_registration [n_scans - 1], or null when every chain is one scan
  const void *starts;           // fx_pose [n_chains]
  uint32_t chain_scans, n_chains;
  uint32_t require_flags, max_lost;
  void *follow;                 // fx_follow_scan [n_scans]
  void *poses;                  // fx_pose [n_scans] or null
};
// fx_map_observe (csrc/fx_map_observe.hip): a launch set's arguments.  The first group is the map's own memory, the last the
// context's scratch, sized by the map's max_landmarks (cap) and by q_max_rows.
#define FX_MAP_OBSERVE_ST_WORDS 8  // 0 scans_used, 1 proposed, 2 added, 3 duplicates, 4 gated, 5 stale, 6 landmarks_touched, 7 list entries
struct FxMapObserveArgs {
  void *header;                 // fx_map_header
  void *records;                // fx_map_landmark [cap]
  double *acc;                  // [cap][FX_MAP_ACC]
  const int32_t *alias;         // [cap]
  uint32_t cap;
  FxKpQuery K;
  const void *loc;              // fx_localization [n_scans]
  const int32_t *map_id_of_row; // [q_max_rows]
  double gd2;                   // the gate: (double)gate_dist squared
  uint32_t require_flags, mode;
  uint32_t *result;             // fx_map_observe_result or null
  uint32_t *gained;             // [cap] or null
  int32_t *observed;            // [q_max_rows] or null
  uint32_t *cnt;                // [cap]: entries of the landmark's list; cur and st follow it (one memset clears the three)
  uint32_t *cur;                // [cap]: the scatter's cursor into the list
  uint32_t *st;                 // [FX_MAP_OBSERVE_ST_WORDS]
  uint32_t *local;              // [cap]: the exclusive prefix of cnt within the block of 256
  uint32_t *bsum;               // [2][blocks of landmarks]: the block's entries, then their prefix (the second row is unused: 0)
  int32_t *tgt;                 // [q_max_rows]: the landmark the row's proposal passed the gate of, -1: none
  unsigned long long *d2;       // [q_max_rows]: its squared xy distance as bits
  uint4 *ent, *sorted;          // [q_max_rows] each: the lists as the scatter left them, and in ascending row; an entry is a proposal
                                // that passed the gate: x its row, y its scan, (w << 32) | z its d2 bits (one 16-byte vector: no struct copies)
};
// fx_map_relocalize (csrc/fx_map_relocalize.hip): a launch set's arguments.  P and Q describe the two grids over the map, alive
// together in the context's scratch (the merge's per-landmark arrays are null in both): P, the pair grid, finds the landmarks h
// whose distance from g can pass the length gate of a seed; Q, the score grid, the landmark a keypoint's image lands on.  The last
// group is the context's scratch.
#define FXR_CHUNK 256  // pair-grid slots a workgroup of the hypothesis kernel takes, a lane each
struct FxRelocPartial {         // the best hypothesis of one workgroup: 16 B
  uint32_t score, g, h, pad_;
};
struct FxRelocWinner {          // the winner of a scan: 48 B
  uint32_t score, seed, g, h;   // score 0: no winner
  double c, s, tx, ty;
};
struct FxMapRelocalizeArgs {
  FxMapMergeArgs P, Q;
  FxKpQuery K;
  float inlier_dist, pair_tol, min_baseline, max_baseline;
  uint32_t max_seeds, min_inliers, min_margin, min_landmark_obs, segment;
  uint32_t chunks;              // workgroups of the hypothesis kernel a (scan, seed): ceil(cap / FXR_CHUNK)
  uint32_t scan0;               // the hypothesis kernel's first scan (a launch takes 65535 scans)
  void *out;                    // fx_relocalization [n_scans]
  int32_t *map_id_of_row;       // [q_max_rows]
  uint8_t *elig;                // [cap]: 1, the landmark is eligible
  double *kq;                   // [n_scans][64][3]: the used keypoints of a scan, widened
  uint32_t *krow;               // [n_scans][64]: their rows
  uint32_t *meta;               // [n_scans][4]: n_kp, n_seeds, FX_RELOC_TRUNCATED or 0, 0
  uint32_t *seeds;              // [n_scans][64]: a | b << 8 of seed rank s
  unsigned long long *n_hyp;    // [n_scans]
  uint32_t *runner;             // [n_scans]: the best rival's score (atomic max)
  FxRelocPartial *partial;      // [n_scans][max_seeds][chunks]
  FxRelocWinner *win;           // [n_scans]
};
// fx_map_compact (csrc/fx_map_compact.hip): a launch set's arguments.  The first group is the map's own memory, the last the
// context's scratch, sized by the map's max_landmarks (cap).
// fx_map_retire runs the same launches with a rule (expected given): a landmark the counters condemn is not kept, and the counters
// move with the landmarks; fx_map_compact passes no rule.
#define FX_MAP_COMPACT_ST_WORDS 8  // 0 K: landmarks kept, 1 observations of the dropped live landmarks, 2 absorbed landmarks dropped,
                                   // 3 retired landmarks, 4 their observations, 5 protected by the carry (3 .. 5: fx_map_retire)
struct FxMapCompactArgs {
  void *header;                 // fx_map_header
  void *records;                // fx_map_landmark [cap]
  double *acc;                  // [cap][FX_MAP_ACC]
  int32_t *carry;               // [max_carry]
  int32_t *alias;               // [cap]
  uint32_t cap, max_carry;
  uint32_t min_obs, min_age;
  int32_t *remap;               // [cap] or null
  uint32_t *result;             // fx_map_compact_result or null
  uint32_t *mark;               // [cap]: 1: a carry entry resolves to the landmark; st follows it (one memset clears both)
  uint32_t *st;                 // [FX_MAP_COMPACT_ST_WORDS]
  int32_t *local;               // [cap]: a kept landmark's exclusive prefix within its block of 256, -1: dropped
  uint32_t *bsum;               // [2][blocks of landmarks]: the block's kept landmarks / dropped live observations, then their prefix
  uint4 *stage_rec, *stage_acc; // [cap][3], [cap][4]: the kept records and sums at their new ids, before they are copied back
  // fx_map_retire's rule; expected null: no rule (fx_map_compact), and nothing below is read
  uint32_t *expected, *seen;    // [cap]: the caller's counters, read by the rule and renumbered with the landmarks
  uint32_t min_expected, seen_num, seen_den, dry_run;
  uint8_t *retired;             // [cap] or null: 1 for a retired old id
  uint32_t *stage_cnt;          // [2][cap]: the kept landmarks' counters at their new ids
};
// fx_map_expect (csrc/fx_map_expect.hip): a launch set's arguments.  G describes the grid over the map (its gate is max_range; the
// merge's per-landmark arrays are null); the last group is the context's scratch, sized by the map's max_landmarks (G.cap) and by
// q_max_rows.
#define FX_MAP_EXPECT_ST_WORDS 8  // the words of fx_map_expect_result, in its order
struct FxMapExpectArgs {
  FxMapMergeArgs G;
  FxKpQuery K;
  const void *loc;              // fx_localization [n_scans]
  const int32_t *map_id_of_row; // [q_max_rows]
  double x_min, x_max, y_min, y_max;  // the options' floats widened
  double lo2, hi2, w2;          // (double)min_range, max_range and shadow_width squared
  uint32_t require_flags, min_landmark_obs, segment, mode;
  uint32_t *result;             // fx_map_expect_result or null
  uint32_t *expected, *seen;    // [cap]: the caller's arrays
  uint32_t *cnt_e;              // [cap]: this call's expected counts; cnt_s and st follow it (one memset clears the three)
  uint32_t *cnt_s;              // [cap]: ... seen counts
  uint32_t *st;                 // [FX_MAP_EXPECT_ST_WORDS]
  int32_t *tgt;                 // [q_max_rows]: the landmark the row names, -1: a finite row of a used scan that names none, -2: any other
};
// fx_map_discover (csrc/fx_map_discover.hip): a launch set's arguments.  G describes the grid over the map (its gate is known_dist;
// the merge's per-landmark arrays are null), F the grid over the free rows' world points (its gate is join_dist; it reads `pts`,
// not the map); the last group is the context's scratch, sized by the map's max_landmarks (G.cap) and by q_max_rows.  A free row
// is known by its number j in ascending row order from k_disc_stage on.
#define FX_MAP_DISCOVER_ST_WORDS 16  // 0 .. 13 the words of fx_map_discover_result up to `refused`, in its order; 14 confirmed leaders
#define FX_DISC_NONE 0xffffffffu
struct FxMapDiscoverArgs {
  FxMapMergeArgs G, F;
  void *header;                 // fx_map_header
  void *records;                // fx_map_landmark [cap]
  double *acc;                  // [cap][FX_MAP_ACC]
  FxKpQuery K;
  const void *loc;              // fx_localization [n_scans]
  const int32_t *map_id_of_row; // [q_max_rows]
  uint32_t min_obs, require_flags, segment, mode;
  uint32_t *result;             // fx_map_discover_result or null
  int32_t *new_id;              // [q_max_rows] or null
  uint32_t *st;                 // [FX_MAP_DISCOVER_ST_WORDS]; sup follows it (one memset clears both)
  uint32_t *sup;                // [q_max_rows]: kept rows attached to leader j, the scans that saw it
  int32_t *fidx;                // [q_max_rows]: row r is free row fidx[r]; -1: not free.  Until k_disc_stage: r's place among its block's free rows
  uint32_t *bsum_f, *bsum_c;    // [2][blocks of rows] each: the block's free rows / confirmed leaders, then their prefix (the second row is unused: 0)
  double2 *pts;                 // [q_max_rows]: the world (x, y) of free row j
  uint2 *src;                   // [q_max_rows]: (row, scan) of free row j
  uint32_t *lead;               // [q_max_rows]: 1: free row j is a leader
  uint32_t *att;                // [q_max_rows]: the leader free row j attaches to, FX_DISC_NONE: an orphan
  unsigned long long *ad2;      // [q_max_rows]: its squared xy distance from that leader as bits
  uint32_t *kept;               // [q_max_rows]: 1: free row j is its scan's observation of its leader
  uint32_t *rank_c;             // [q_max_rows]: a confirmed leader's place among its block's, FX_DISC_NONE: not one
};
// fx_map_append, fx_map_append_host (csrc/fx_map_append.hip): a launch set's arguments.  The source as the kernels read it is six
// pointers: a map's own buffers, or the sections of a snapshot staged in the context's scratch; the two look the same.
#define FX_MAP_APPEND_ST_WORDS 8  // 0 the result's flags, 1 N: the id base, 2 the scan base, 3 the segment base, 4 landmarks to move,
                                  // 5 carry rows to move (4 and 5: 0 on a refusal)
struct FxMapSrcView {
  const void *header;           // fx_map_header
  const void *records;          // fx_map_landmark [n_landmarks]
  const double *acc;            // [n_landmarks][FX_MAP_ACC]
  const int32_t *alias;         // [n_landmarks]
  const int32_t *carry;         // [carry_rows]
  const uint4 *carry_kp;        // [carry_rows]
};
struct FxMapAppendArgs {
  void *header;                 // the target: fx_map_header
  void *records;                // fx_map_landmark [cap]
  double *acc;                  // [cap][FX_MAP_ACC]
  int32_t *alias;               // [cap]
  int32_t *carry;               // [max_carry]
  uint4 *carry_kp;              // [max_carry]
  uint32_t cap, max_carry;
  FxMapSrcView src;
  uint32_t src_cap, src_max_carry;  // landmarks and carry rows the source's pointers hold at least: its header's counts are clipped to them
  uint32_t *result;             // fx_map_append_result or null
  size_t stage_bytes;           // bytes of a snapshot to stage (0: the source is a map)
  uint8_t *stage;               // [stage_bytes] of the context's scratch
  uint32_t *st;                 // [FX_MAP_APPEND_ST_WORDS]
};
// What fx_map_join_segments and fx_map_close_loop share (csrc/fx_map_assoc.h): the association of one set of landmarks with another
// under a prior and the consensus over it.  G describes the grid over the map (its gate is the search distance; the merge's
// per-landmark arrays are null) and carries the map's own memory; the last group is the context's scratch, sized by the map's
// max_landmarks (G.cap).
#define FX_MAP_ASSOC_ST_WORDS 4  // 0 queries, 1 queries with a target, 2 landmarks moved
struct FxMapAssocArgs {
  FxMapMergeArgs G;
  uint32_t mode;                // FX_JOIN_* / FX_LOOP_*: FIT, GIVEN or DRY_RUN
  double prior[5];              // c, s, tx, ty, tz: the host's prior, or the identity
  const double *prior_device;   // five doubles read on the device in its place, or null
  float inlier_dist, min_baseline;
  uint32_t hyp_corr, min_inliers, min_landmark_obs;
  int32_t *match;               // [cap] or null
  void *fit;                    // the call's result record: what the consensus decided, for the launches behind it
  uint32_t *st;                 // [FX_MAP_ASSOC_ST_WORDS]
  int32_t *near;                // [cap]: the query's target, -1: none or no query
  unsigned long long *d2;       // [cap]: its squared xy distance as bits
  uint32_t *local;              // [cap]: the exclusive prefix of the queries with a target within the block of 256
  uint32_t *bsum;               // [2][blocks of landmarks]: the block's queries / queries with a target, then their prefix
  uint32_t *corr;               // [FXC_MAP_MAX_CORR]: the queries of the correspondences, in ascending id
};
// fx_map_join_segments (csrc/fx_map_join.hip): a launch set's arguments.
struct FxMapJoinArgs {
  FxMapAssocArgs S;
  uint32_t src, dst;
  void *result;                 // fx_map_join_result or null
};
// fx_map_close_loop (csrc/fx_map_loop.hip): a launch set's arguments.
struct FxMapLoopArgs {
  FxMapAssocArgs S;
  uint32_t segment;             // the option's segment (FX_LOC_LAST_SEGMENT is resolved on the device)
  uint32_t min_loop_scans, recent_scans;
  uint32_t given_s0, given_s1;  // FX_LOOP_GIVEN: the loop's bounds and the pivot
  double given_px, given_py;
  void *result;                 // fx_map_loop_result or null
};
// fx_map_find_loop (csrc/fx_map_find_loop.hip): a launch set's arguments.  P and Q are fx_map_relocalize's two grids (the search
// is csrc/fx_map_constellation.h's, with the loop's queries in the place of a scan's keypoints); the last group is the context's
// scratch.
#define FX_FIND_ST_WORDS 8  // 0 n_targets, 1 the best rival's score (atomic max), 2 n_query, 3 n_seeds, 4 FX_FIND_TRUNCATED or 0,
                            // 5 qseg, 6 tseg (resolved; 0xffffffff: FX_LOC_LAST_SEGMENT in a map of no segment), 7 FX_FIND_BAD_SEGMENT or 0
struct FxMapFindLoopArgs {
  FxMapMergeArgs P, Q;
  float inlier_dist, pair_tol, min_baseline, max_baseline;
  uint32_t max_seeds, min_inliers, min_margin, min_landmark_obs;
  uint32_t segment, target_segment;  // the options' (FX_LOC_LAST_SEGMENT and FX_FIND_SAME_SEGMENT are resolved on the device)
  uint32_t min_loop_scans, recent_scans;
  uint32_t chunks;              // workgroups of the hypothesis kernel a seed: ceil(cap / FXR_CHUNK)
  void *result;                 // fx_map_loop_candidate
  int32_t *match;               // [cap] or null
  unsigned long long *n_hyp;    // [1]; st follows it (one memset clears both)
  uint32_t *st;                 // [FX_FIND_ST_WORDS]
  uint8_t *elig;                // [cap]: 0 neither, 1 target, 2 query
  double *kq;                   // [64][3]: the queries' x, y, z, in descending id
  uint32_t *kid;                // [64]: their ids
  uint32_t *seeds;              // [64]: a | b << 8 of seed rank s
  FxRelocPartial *partial;      // [max_seeds][chunks]
  FxRelocWinner *win;           // [1]
};
// fx_splice_blocks (csrc/fx_splice.hip): a launch set's arguments.  A source is fx.h's fx_splice_source with its blocks as words; the
// plan words are the context's scratch.
#define FX_SPLICE_PLAN_WORDS 32  // what k_splice_plan resolves from the two sources' headers for the launch behind it (fx_splice.hip names them)
struct FxSpliceSrc {
  const uint32_t *kp;           // keypoint block (include/fx.h fx_pack_keypoint_block)
  uint32_t max_scans, max_total;
  const uint32_t *csr;          // CSR block (include/fx.h fx_descriptor_csr_bytes); not read when the destination has none
  uint32_t max_rows, cap;
  uint32_t scan0, n_scans;
};
struct FxSpliceArgs {
  FxSpliceSrc a, b;
  uint32_t *dst_kp;
  uint32_t dst_max_scans, dst_max_total;
  uint32_t *dst_csr;            // or null: keypoints only
  uint32_t dst_max_rows, dst_cap;
  uint32_t *plan;               // [FX_SPLICE_PLAN_WORDS]
};
// fx_deskew_keypoint_block (csrc/fx_deskew.hip): the launch's arguments.  dst may be src itself; the options are fx.h's, checked.
struct FxDeskewArgs {
  const uint32_t *src;          // keypoint block (include/fx.h fx_pack_keypoint_block)
  uint32_t *dst;                // a block of the same layout
  uint32_t max_scans, max_total;
  const void *motions;          // fx_registration [n_scans - 1] (LINKS) or [n_scans] (PER_SCAN)
  uint32_t n_scans;
  double start_turn, ref_fraction, sweep_fraction, direction;  // (direction: +1.0 or -1.0)
  uint32_t source, require_flags;
  void *out;                    // fx_deskew_scan [n_scans], zeroed in front of the launch
};
#define FX_TRACK_NONE 0xffffffffu
#define FX_CNT_QPOOL 32   // counters[32]: entries of the dense tier's query pool in use
#define FX_CNT_LARGE2 16  // counters[16 + c]: rings of XCD class c the second run tier hands to the workgroup tier
#define FX_CNT_LARGE 24  // counters[24 + c]: ... to the large tier
struct FxBuffers {
  const FxScanMeta *meta;
  const float2 *ring_win;  // [n_rings] (lo, hi) as float, inclusive
  const double *atan_tab;  // [FX_ATAN_N + 1][FX_ATAN_DEG + 1]: Taylor coefficients of atan about i / FX_ATAN_N (k_prep's elevation)
  const FxScTables *tables;
  const float2 *xaxis;  // [max_keypoints]
  // stage 1
  float4 *filt;          // [B][max_points]
  uint32_t *n_filt;      // [B]
  uint32_t *near_bits;   // [B][near_words]  bit: some point of that sector (4 points) is within the descriptor stage's reach of the filter box
  uint32_t *prep_cnt;       // [B][S]     survivors of slice s of the scan (k_prep_count; S workgroups a scan: small batches of big scans)
  uint32_t *prep_ring_cnt;  // [B][S][n_rings]  their ring counts (k_prep_sliced -> k_bucket_sliced)
  // stage 2a: ring-major copy of the filtered cloud
  float4 *ring_pts;         // [B][ring_slot_cap]
  uint32_t *ring_off;       // [B][n_rings]
  uint32_t *ring_cnt;       // [B][n_rings]
  // stage 2b
  float4 *ring_cand;        // [B][n_rings][max_ring_cands]
  uint32_t *ring_cand_size; // same shape
  uint32_t *ring_cand_cnt;  // [B][n_rings]
  float4 *kpc_pool;         // [B][ring_slot_cap]  ring r's members start at ring_off[r]
  uint32_t *kpc_pool_cand;  // [B][ring_slot_cap]  ring-local candidate slot
  uint32_t *kpc_ring_cnt;   // [B][n_rings]
  // stage 3
  float4 *cand;           // [B][max_candidates]
  uint32_t *cand_size;    // [B][max_candidates]
  int32_t *cand_kp;       // [B][max_candidates]
  uint32_t *n_cand;       // [B]
  float4 *keypoints;      // [B][max_keypoints]
  uint32_t *kp_size;      // [B][max_keypoints]
  uint32_t *kp_nbrs;      // [B][max_keypoints]
  uint32_t *n_kp;         // [B]
  uint32_t *kp_offset;    // [B+1]
  float4 *kpc;            // [B][max_kpc]
  uint32_t *kpc_cand;     // [B][max_kpc]
  uint32_t *n_kpc;        // [B]
  // stage 5
  float *desc;            // [max_total_kp][1989]
  // What the previous batches left in each descriptor row (rows outlive a batch: the buffer is zeroed when the context is
  // made, and a row is cleared by un-writing what was written to it): the number of non-zero bins a group workgroup of k_desc wrote, or
  // FX_ROW_DIRTY when another tier (or a NaN fill) wrote the row — such a row is cleared whole.
  uint32_t *desc_nbins;   // [max_total_kp]
  uint16_t *desc_bins;    // [max_total_kp][FX_GROUP_CAP]: those bins
  uint8_t *row_class;     // [max_total_kp]  FX_ROW_*: the tier that computes the row in this batch (the support gather classifies every row)
  uint32_t *flags;        // [B]
  // work lists for the large-capacity tiers
  uint32_t *huge_rings;   // [B*n_rings]  rings for the workgroup tier (k_rings_large), by XCD class
  uint32_t *huge_rings2;  // [B*n_rings]  rings the second run tier hands to the workgroup tier, by XCD class
  uint32_t *big_merge;    // [B]
  uint32_t *huge_merge;   // [B]  scans with more candidates than the LDS merge tiers hold
  uint32_t *front_n;      // [B]  k_front_ab -> k_front_cd: the scan's ring-major entries; 0: none (empty results written); FX_NONE: handed to k_front_redo
  uint32_t *redo;         // [B]  scans that do not fit k_front's LDS tables: k_front_redo runs the general kernels' bodies on them
  uint32_t *slow;         // [B]  scans with work for the slow tier (k_slow): rings or merges beyond every LDS-sized tier
  uint32_t *slow_state;   // [B]  1 while the scan is listed (k_slow clears it)
  uint32_t *ring_pending; // [B][(n_rings + 31) / 32]  bit r: ring r of the scan waits for k_slow (which clears it)
  uint32_t *gs_pool;      // [gs_slots][gs_words]  k_slow's scratch: the LDS tiers' per-point / per-cluster arrays, in HBM
  uint32_t *gsd_pool;     // [gsd_slots][gsd_words]  dense_slow_loop's scratch: a support set of up to max_points points
  uint32_t *merge_hp;     // [B][merge_hp_words]  the large merge tier as three launches (batches of few scans): a scan's slices' roots, its bin table, its state (null: not allocated — the one launch)
  float4 *merge_sorted;   // [B][max_candidates] (x, y, pseudo z, id) in bin order: k_merge_huge's pair tests (allocated only when that tier exists)
  uint32_t *list_desc;    // [max_total_kp]  rows whose list is too long for one wavefront (257 .. dense_min support points)
  uint32_t *wave_desc;    // [max_total_kp]  rows with 65..256 support points (one wavefront each)
  uint32_t *group_desc;   // [FX_GROUP_CLASSES][max_total_kp]  group rows by size class (16 / 8 / 4 rows a wavefront of k_desc's group workgroups); FX_ROW_DENSE_FAIL rows ride in the widest class's list
  // dense tier (k_dense_*)
  uint32_t *dense_rows;   // [max_dense_rows]  rows of the tier (FX_NONE: no room in the pools, flagged)
  uint32_t *dense_order;  // [4][max_dense_rows]  slots by size class (largest rows first)
  uint32_t *dense_off;    // [max_dense_rows]  the row's region of dense_pts / dense_q
  uint32_t *dense_koff;   // [max_dense_rows]  the row's region of dense_key (rows whose keys do not fit LDS)
  uint32_t *dense_qoff;   // [max_dense_rows]  the row's region of dense_q
  uint32_t *dense_nq;     // [max_dense_rows]  queries (densities this row computes)
  uint32_t *dense_nm;     // [max_dense_rows]  binned neighbours (FX_NONE: failed row)
  uint32_t *dense_cells;  // [max_dense_rows][25 * 25 * 7]  end of every cell in the row's sorted region
  uint2 *dense_items;     // work items of k_dense_density: (slot, first query)
  float4 *dense_pts;      // [dense_cap]  support sets sorted by cell (x, y, z rotated, point index as bits)
  uint32_t *dense_q;      // [dense_qcap]  query lists (positions in the row's sorted region, cell by cell, padded to four)
  unsigned long long *dense_key;   // [dense_cap]  (bin, d2, index) keys of rows too large for the LDS sort
  unsigned long long *dens_cache;  // [B][max_points]  batch tag << 21 | local point density of the point (k_dense_density)
  unsigned long long *seq;         // [1]  batches processed (device side), the cache's tag
  float4 *ovf_pts;        // [B][ovf_cap]  list entries beyond list_cap, unordered (k_gather)
  uint32_t *ovf_kp;       // [B][ovf_cap]  keypoint ordinal of each
  uint32_t *ovf_cnt;      // [B]
  uint32_t *gather_cnt;   // [B][16][max_keypoints]  k_gather_count -> k_gather_scatter: a slice's entries per keypoint (several workgroups a scan: batches of few big scans)
  // per-keypoint support lists written by k_gather
  float4 *s_pts;          // [max_total_kp][list_cap]  (x, y, z rotated, point index as bits)
  uint32_t *s_cnt;        // [max_total_kp]
  uint2 *row_map;         // [max_total_kp]  (scan, keypoint ordinal) of each descriptor row
  float4 *row_kp;         // [max_total_kp]  the row's keypoint and its 3DSC x-axis (first-pass ordinal), so that the
  float2 *row_xa;         //                 per-keypoint kernels fetch everything a row needs in one round trip
  unsigned long long *clk;     // [FX_CLK_SLOTS][2] k_prep's first start / last end on the device's constant-rate clock, by batch
  unsigned long long *stamps;  // [32] diagnostic build only (-DFX_STAMPS)
  uint32_t *tier_hint;    // [FX_N_HINTS], pinned HOST memory: the batch's counts of work for the rarely used tiers, which the host sizes the next batch's launches of those tiers by (k_offsets, k_desc write them; grid sizes only — never what is computed)
  uint32_t *counters;     // [FX_N_COUNTER_WORDS]: 16.. / 24.. rings handed on per XCD class; 1 big_merge, 4 list_desc, 6 dense rows (2 / 3 / 7 / 10: by size class), 8 wave_desc, 33 / 34 / 35 group_desc by size class, 9 huge_merge, 12 key pool used, 13 sorted pool used, 14 density items, 15 / 11 / 5 / 0 tickets of k_dense_density / sort / finish_s / finish_l
};

#endif
