// fx_map_assoc.hip — the launches of csrc/fx_map_assoc.h that have no per-call part: the rank of the queries with a target
// (k_ma_top, k_ma_gather: fx_map_join_segments and fx_map_close_loop both run them behind their own search kernel), and the carving
// of the shared scratch.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_map_assoc.h"


extern "C" __global__ __launch_bounds__(FXA_WG) void k_ma_top(FxMapAssocArgs S, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXA_NWAVE];
  uint32_t tot_a, tot_b;
  wg_scan2_blocks<FXA_NWAVE>(S.bsum, n_blocks, s_w, tot_a, tot_b);
  if (threadIdx.x == 0u) S.st[0] = tot_a, S.st[1] = tot_b;
}

extern "C" __global__ __launch_bounds__(FXA_WG) void k_ma_gather(FxMapAssocArgs S, uint32_t n_blocks) {
  const uint32_t i = blockIdx.x * FXA_WG + threadIdx.x;
  if (i >= S.G.cap || S.near[i] < 0) return;
  const uint32_t slot = S.bsum[n_blocks + blockIdx.x] + S.local[i];
  if (slot < FXC_MAP_MAX_CORR) S.corr[slot] = i;
}

extern "C" void fxk_map_assoc_rank(hipStream_t s, const FxMapAssocArgs &S, uint32_t n_blocks) {
  hipLaunchKernelGGL(k_ma_top, dim3(1), dim3(FXA_WG), 0, s, S, n_blocks);
  hipLaunchKernelGGL(k_ma_gather, dim3(n_blocks), dim3(FXA_WG), 0, s, S, n_blocks);
}

// bytes of the context's scratch for a map of S->G.cap landmarks, and the pointers carved out of it: the grid's part of the merge's
// layout first (the map calls share the buffer: they are ordered on one stream), then the call's result record of fit_bytes and
// the association's arrays
extern "C" size_t fxk_map_assoc_scratch(FxMapAssocArgs *S, uint8_t *base, size_t fit_bytes) {
  FxCarve C{base, fxk_map_merge_scratch(&S->G, base)};
  S->G.prop = S->G.pred = S->G.succ = nullptr, S->G.keep = nullptr;  // (the grid's mark leaves the merge's words alone)
  const size_t cap = S->G.cap, nb = (cap + FXA_WG - 1u) / FXA_WG;
  S->fit = C.take<uint8_t>(fit_bytes);
  S->st = C.take<uint32_t>(FX_MAP_ASSOC_ST_WORDS);
  S->d2 = C.take<unsigned long long>(cap);
  S->near = C.take<int32_t>(cap);
  S->local = C.take<uint32_t>(cap);
  S->bsum = C.take<uint32_t>(2u * nb);
  S->corr = C.take<uint32_t>(FXC_MAP_MAX_CORR);
  return C.o;
}
