// fx_launch.h — the launchers and getters the .hip files define for the host driver (fx_api.cpp), declared once: the files
// that define them include this header too, so an argument list that drifts is a compile error, not a call that links and runs.
// A launcher computes its LDS bytes from its file's constants and launches with the grid it is given; what to launch is
// csrc/fx_launch_plan.h's decision.
#ifndef FX_LAUNCH_H_
#define FX_LAUNCH_H_
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_device.h"
#include "fx_launch_plan.h"

extern "C" {
// ---- fx_kernels.hip: sizes and build constants
size_t fxk_ring_large_lds_bytes(uint32_t cap, uint32_t ccap);
size_t fxk_ring_runs_lds_bytes(void);
size_t fxk_merge_lds_bytes(uint32_t cap, uint32_t n_rings);
size_t fxk_merge_huge_lds_bytes(uint32_t cap, uint32_t ccap, uint32_t n_rings);
size_t fxk_merge_hp_words(uint32_t cap);
size_t fxk_desc_lds_bytes(uint32_t cap);
size_t fxk_gather_lds_bytes(uint32_t max_keypoints);
size_t fxk_dense_finish_lds_bytes(void);
size_t fxk_dense_slow_words(uint32_t max_points);
size_t fxk_slow_words(uint32_t max_ring_points, uint32_t max_candidates, uint32_t huge_ccap);
size_t fxk_kp_block_bytes(uint32_t max_scans, uint32_t max_total);
size_t fxk_csr_bytes(uint32_t max_rows, uint32_t cap);
uint32_t fxk_near_words(uint32_t max_points);
uint32_t fxk_dense_cells(void);
uint32_t fxk_group_cap(void);
uint32_t fxk_dfin_k(void);
uint32_t fxk_front_max_rings(void);
// (what FxPlanConfig takes from the build)
uint32_t fxk_prep_slices_max(void);
uint32_t fxk_merge_slices_max(void);
uint32_t fxk_front_merge_cap(void);
uint32_t fxk_gather_counted_max(void);
uint32_t fxk_gather_kcap(void);
uint32_t fxk_gather_slices_big(void);
uint32_t fxk_dsort_per_cu(void);
uint32_t fxk_ddens_per_cu(void);
hipError_t fxk_configure(size_t ring_big, size_t merge_big, size_t merge_huge, size_t desc_big, size_t gather);
hipError_t fxk_configure_front(void);
// ---- fx_kernels.hip: the stages of a batch
void fxk_prep(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, float near_margin, float el0, float inv_step,
              uint32_t clk_slot);
void fxk_bucket(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, float el0, float inv_step, uint32_t clk_next,
                uint32_t many_rings);
void fxk_prep_sliced(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, uint32_t slices, float near_margin, float el0, float inv_step,
                     uint32_t clk_slot);
void fxk_bucket_sliced(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, uint32_t slices, float el0, float inv_step,
                       uint32_t clk_next);
void fxk_rings_runs(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, uint32_t max_pts, uint32_t grid);
void fxk_rings_runs2(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t max_pts, uint32_t grid);
void fxk_rings_large(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t cap, uint32_t ccap, uint32_t grid,
                     uint32_t after_runs2);
void fxk_merge_small(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, uint32_t cap);
void fxk_merge_big(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t cap, uint32_t grid, uint32_t last);
void fxk_merge_huge(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t cap, uint32_t ccap, uint32_t grid);
void fxk_merge_huge_split(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t cap, uint32_t ccap, uint32_t grid, uint32_t slices);
void fxk_front(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, float near_margin, float el0, float inv_step,
               uint32_t clk_slot, uint32_t merge_cap, uint32_t force_redo);
void fxk_front_ab(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, float near_margin, float el0, float inv_step,
                  uint32_t clk_slot, uint32_t force_redo);
void fxk_front_cd(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, uint32_t clk_slot, uint32_t merge_cap, uint32_t lean,
                  uint32_t self_n, uint32_t force_redo);
void fxk_front_redo(hipStream_t s, const FxDevParams &P, const FxBuffers &B, float el0, float inv_step, uint32_t huge_ccap, uint32_t force_slow,
                    uint32_t grid);
void fxk_slow(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t huge_ccap, uint32_t grid, uint32_t batch, uint32_t clk_next);
void fxk_gather(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, float box_margin, FxGatherKind kind, uint32_t per_scan);
void fxk_rng_ord(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch);
void fxk_desc(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, uint32_t cap, uint32_t n_wg, uint32_t n_wave, uint32_t n_group,
              uint32_t n_dslow);
void fxk_dense(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t sort_grid, uint32_t density_grid, uint32_t finish_grid, uint32_t skip);
// ---- fx_kernels.hip: results and inputs
void fxk_pack_kp_records(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, void *dst,
                         uint32_t rec_kp);
void fxk_pack_kp_block(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, void *dst, uint32_t max_scans, uint32_t max_total,
                       uint32_t grid);
hipError_t fxk_pack_csr(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, void *dst, uint32_t max_rows, uint32_t cap,
                        uint32_t grid, uint32_t full_rows);
void fxk_unpack_pc2(hipStream_t s, const void *src, uint32_t n, uint32_t point_step, uint32_t ox, uint32_t oy, uint32_t oz,
                    uint32_t oi, uint32_t big_endian, void *dst, uint32_t grid);
void fxk_pack_xyzi32(hipStream_t s, const void *src, uint32_t n, void *dst, uint32_t grid);
void fxk_pack_features(hipStream_t s, const FxDevParams &P, const FxBuffers &B, uint32_t batch, void *dst,
                       uint32_t capacity, uint32_t grid);
#ifdef FX_TEST_HOOKS
void fxk_test_sort_replay(hipStream_t s, const uint32_t *sizes, uint32_t n_seq, uint32_t n, uint32_t *perm);
size_t fxk_test_cc_order_scratch_words(uint32_t n_seq, uint32_t ccap_max);
hipError_t fxk_test_cc_order(hipStream_t s, uint32_t nt, bool gs, const uint32_t *sizes, const uint32_t *parent, uint32_t n_seq, uint32_t n,
                             uint32_t min_sz, uint32_t max_sz, const uint32_t *ccaps, uint32_t ccap_max, uint32_t *scratch, uint32_t *perm,
                             uint32_t *roots, uint32_t *n_c, uint32_t *guard_bad);
void fxk_test_elevation(hipStream_t s, const float *xyz, uint32_t n, const double *tab, float *fast, uint8_t *ok, float *exact);
void fxk_test_within(hipStream_t s, const float4 *sp, uint32_t n, const float4 *queries, uint32_t nq, float r2, uint32_t *packed, uint32_t *plain);
#endif
// ---- fx_match.hip, fx_register.hip, fx_track.hip, fx_splice.hip, fx_deskew.hip
hipError_t fxk_deskew(hipStream_t s, const FxDeskewArgs &A, uint32_t max_grid);
hipError_t fxk_match(hipStream_t s, const FxMatchArgs &A, uint32_t n_items, uint32_t mut_n, uint32_t shifts);
uint32_t fxk_match_tile_rows(void);
hipError_t fxk_register(hipStream_t s, const FxRegisterArgs &A, uint32_t n_pairs);
hipError_t fxk_track(hipStream_t s, const FxTrackArgs &A);
uint32_t fxk_track_wg_rows(void);
hipError_t fxk_splice(hipStream_t s, const FxSpliceArgs &A, uint32_t max_grid);
// ---- fx_map*.hip (a *_scratch with base == nullptr returns the bytes the call needs; with a base it carves A's pointers)
hipError_t fxk_map_reset(hipStream_t s, const FxMapArgs &A);
hipError_t fxk_map_update(hipStream_t s, const FxMapArgs &A);
uint32_t fxk_map_wg(void);
hipError_t fxk_map_grid_build(hipStream_t s, const FxMapMergeArgs &A);
uint32_t fxk_map_merge_table(uint32_t cap);
hipError_t fxk_map_merge(hipStream_t s, const FxMapMergeArgs &A);
size_t fxk_map_merge_scratch(FxMapMergeArgs *A, uint8_t *base);
uint32_t fxk_map_merge_wg(void);
hipError_t fxk_map_localize(hipStream_t s, const FxMapLocalizeArgs &A);
size_t fxk_map_localize_scratch(FxMapLocalizeArgs *A, uint8_t *base);
hipError_t fxk_map_follow(hipStream_t s, const FxMapFollowArgs &A);
size_t fxk_map_follow_scratch(FxMapFollowArgs *A, uint8_t *base);
hipError_t fxk_map_relocalize(hipStream_t s, const FxMapRelocalizeArgs &A);
size_t fxk_map_relocalize_scratch(FxMapRelocalizeArgs *A, uint8_t *base);
hipError_t fxk_map_observe(hipStream_t s, const FxMapObserveArgs &A);
size_t fxk_map_observe_scratch(FxMapObserveArgs *A, uint8_t *base);
hipError_t fxk_map_expect(hipStream_t s, const FxMapExpectArgs &A);
size_t fxk_map_expect_scratch(FxMapExpectArgs *A, uint8_t *base);
hipError_t fxk_map_discover(hipStream_t s, const FxMapDiscoverArgs &A);
size_t fxk_map_discover_scratch(FxMapDiscoverArgs *A, uint8_t *base);
hipError_t fxk_map_find_loop(hipStream_t s, const FxMapFindLoopArgs &A);
size_t fxk_map_find_loop_scratch(FxMapFindLoopArgs *A, uint8_t *base);
hipError_t fxk_map_compact(hipStream_t s, const FxMapCompactArgs &A);
size_t fxk_map_compact_scratch(FxMapCompactArgs *A, uint8_t *base);
hipError_t fxk_map_append(hipStream_t s, const FxMapAppendArgs &A);
size_t fxk_map_append_scratch(FxMapAppendArgs *A, uint8_t *base);
void fxk_map_assoc_rank(hipStream_t s, const FxMapAssocArgs &S, uint32_t n_blocks);
size_t fxk_map_assoc_scratch(FxMapAssocArgs *S, uint8_t *base, size_t fit_bytes);
hipError_t fxk_map_join(hipStream_t s, const FxMapJoinArgs &A);
size_t fxk_map_join_scratch(FxMapJoinArgs *A, uint8_t *base);
hipError_t fxk_map_loop(hipStream_t s, const FxMapLoopArgs &A);
hipError_t fxk_map_loop_poses(hipStream_t s, const void *result, void *poses, uint32_t first, uint32_t n);
size_t fxk_map_loop_scratch(FxMapLoopArgs *A, uint8_t *base);
}  // extern "C"

#endif
