// fx_track.hip — poses and landmark tracks of one batch of consecutive scans (include/fx.h fx_track_landmarks).
//
// The pairwise motions of fx_register_matches are folded into poses, the inlier rows are chained from scan to scan into tracks,
// and each track of enough observations is averaged in the common frame.  Every decision is an integer (atomicMin on the child
// word, an atomicAdd of conflict counts: both order-free), every fp64 value is an ordered chain of correctly rounded operations
// on one lane (the build's -ffp-contract=off): the same bytes from run to run and with any number of contexts in flight.
//
// Launches, in stream order (FXT_WG = 256 rows a workgroup everywhere a thread is a row):
//   k_track_init     a thread a row: the row's scan (fx_scan_query.h scan_of_row), child = none, the two row outputs to their
//                    "nothing" words
//   k_track_poses    one workgroup, tiles of FXT_WG links: the records and their good flags into LDS; one lane folds (c, s),
//                    every thread forms its link's rotated translation from the (c, s) before it, three lanes of three
//                    wavefronts fold tx, ty, tz (one add a step each) while a fourth counts segments; all threads write the tile
//   k_track_link     a thread a row: validate the proposal, atomicMin(child[t], r)
//   k_track_parent   a thread a row: kept iff child[t] == r; (root, depth) starts as (t, 1) or (r, 0); conflicts are counted a
//                    wavefront at a time
//   k_track_jump     ceil(log2 n_scans) launches, ping-pong: (root, depth) <- (root of root, depth + depth of root); a pure
//                    function of the round before
//   k_track_len      the leaf of a track (the row nobody kept as a parent) stores depth + 1 at its root: one writer a track
//   k_track_sums / k_track_top / k_track_number   the integer scan over rows: landmarks and observations that begin in each
//                    block of FXT_WG rows, their exclusive prefix (one workgroup, which also writes the header), and the number
//                    and first obs_row slot of every landmark at its first row
//   k_track_scatter  a thread a row: landmark_of_row, obs_row[obs0 + depth] = r
//   k_track_fuse     a lane a landmark: two sequential passes over its contiguous obs_row segment
// The block's layout, the workgroup scan and the world-frame point of an observation are fx_device.h's (kp_block_*, wg_scan2,
// world_point): fx_map.hip uses the same ones.  The block read as a query (the scans and rows that take part, a row's scan) is
// fx_scan_query.h's, as in the map's calls that read scans.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "fx_scan_query.h"
#include "fx_launch.h"
#include "../../include/fx.h"

#define FXT_WG 256
#define FXT_NWAVE (FXT_WG / 64)

static_assert(sizeof(fx_pose) == 48 && sizeof(fx_landmark) == 48 && sizeof(fx_track_header) == 32 && sizeof(fx_track_options) == 8, "include/fx.h");

namespace {
__device__ __forceinline__ bool good_link(const fx_registration &r) {
  return (r.flags & FX_REG_VALID) && isfinite(r.c) && isfinite(r.s) && isfinite(r.tx) && isfinite(r.ty) && isfinite(r.tz);
}
// is row r the first row of a landmark, and of how many observations
__device__ __forceinline__ uint32_t landmark_len(const FxTrackArgs &A, const uint2 *jump, uint32_t r) {
  if (r >= A.K.q_max_rows || A.scan_of[r] == FX_TRACK_NONE || jump[r].x != r) return 0u;
  const uint32_t n = A.len[r];
  return n >= A.min_obs ? n : 0u;
}
}  // namespace

extern "C" __global__ __launch_bounds__(FXT_WG) void k_track_init(FxTrackArgs A) {
  const uint32_t r = blockIdx.x * FXT_WG + threadIdx.x;
  if (r == 0u) A.counters[0] = 0u;
  if (r >= A.K.q_max_rows) return;
  const KpView B = query_view(A.K);
  uint32_t b;
  A.scan_of[r] = r < B.rows && B.S && scan_of_row(B.off, B.S, r, b) ? b : FX_TRACK_NONE;
  A.child[r] = FX_TRACK_NONE;
  A.landmark_of_row[r] = -1;
  A.obs_row[r] = FX_TRACK_NONE;
}

extern "C" __global__ __launch_bounds__(FXT_WG) void k_track_poses(FxTrackArgs A) {
  __shared__ double s_r[5][FXT_WG];      // the tile's records: c, s, tx, ty, tz
  __shared__ double s_c[FXT_WG + 1], s_s[FXT_WG + 1];  // (c, s) of the pose before the tile and of the tile's poses
  __shared__ double s_t[3][FXT_WG + 1];  // rotated translations of the links, then tx, ty, tz of the poses (slot 0: before the tile)
  __shared__ uint32_t s_kind[FXT_WG];    // 1 good link, 0 bad link, 2 beyond the block's scans
  __shared__ uint32_t s_seg[FXT_WG + 1];
  __shared__ uint32_t s_gaps;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t S = query_scans(A.K);
  const fx_registration *reg = reinterpret_cast<const fx_registration *>(A.reg);
  fx_pose *poses = reinterpret_cast<fx_pose *>(A.poses);
  if (tid == 0u) {
    s_c[0] = A.init[0], s_s[0] = A.init[1], s_t[0][0] = A.init[2], s_t[1][0] = A.init[3], s_t[2][0] = A.init[4];
    s_seg[0] = 0u, s_gaps = 0u;
    fx_pose p;
    p.c = A.init[0], p.s = A.init[1], p.tx = A.init[2], p.ty = A.init[3], p.tz = A.init[4];
    p.segment = 0u, p.flags = S ? 0u : FX_POSE_NO_SCAN;
    poses[0] = p;
  }
  for (uint32_t b0 = 1u; b0 < A.K.n_scans; b0 += FXT_WG) {  // the tile's poses are b0 + i, their links b0 + i - 1
    const uint32_t n = min((uint32_t)FXT_WG, A.K.n_scans - b0);
    __syncthreads();  // (the tile before is written out, its carry is in slot 0)
    if (tid < n) {
      const uint32_t b = b0 + tid;
      uint32_t kind = 2u;
      double rc = 1.0, rs = 0.0, rx = 0.0, ry = 0.0, rz = 0.0;
      if (b < S) {
        const fx_registration r = reg[b - 1u];
        kind = good_link(r) ? 1u : 0u;
        if (kind) rc = r.c, rs = r.s, rx = r.tx, ry = r.ty, rz = r.tz;
      }
      s_kind[tid] = kind;
      s_r[0][tid] = rc, s_r[1][tid] = rs, s_r[2][tid] = rx, s_r[3][tid] = ry, s_r[4][tid] = rz;
    }
    __syncthreads();
#ifndef FXT_SKIP_CS_FOLD  // (measurement builds of tools/track_pose_phases.py leave a phase out: wrong poses, the other phases' time)
    if (tid == 0u) {  // the (c, s) fold: two dependent fp64 operations a step
      double pc = s_c[0], ps = s_s[0];
      for (uint32_t i = 0; i < n; ++i) {
        const double rc = s_r[0][i], rs = s_r[1][i];
        const double c = pc * rc - ps * rs, s = ps * rc + pc * rs;
        const bool good = s_kind[i] == 1u;
        pc = good ? c : pc, ps = good ? s : ps;
        s_c[i + 1u] = pc, s_s[i + 1u] = ps;
      }
    }
#endif
    __syncthreads();
    if (tid < n) {  // the link's translation in the common frame, under the pose before it
      const double pc = s_c[tid], ps = s_s[tid], rx = s_r[2][tid], ry = s_r[3][tid];
      s_t[0][tid + 1u] = pc * rx - ps * ry;
      s_t[1][tid + 1u] = ps * rx + pc * ry;
      s_t[2][tid + 1u] = s_r[4][tid];
    }
    __syncthreads();
#ifndef FXT_SKIP_T_FOLD
    if (lane == 0u) {
      if (wave < 3u) {  // tx, ty, tz: one add a step, a wavefront each
        double *t = s_t[wave];
        double acc = t[0];
        for (uint32_t i = 0; i < n; ++i) {
          const double sum = acc + t[i + 1u];
          acc = s_kind[i] == 1u ? sum : acc;
          t[i + 1u] = acc;
        }
      } else {
        uint32_t seg = s_seg[0], gaps = s_gaps;
        for (uint32_t i = 0; i < n; ++i) {
          const uint32_t bad = s_kind[i] == 0u ? 1u : 0u;
          seg += bad, gaps += bad;
          s_seg[i + 1u] = seg;
        }
        s_gaps = gaps;
      }
    }
#endif
    __syncthreads();
    if (tid < n) {
      fx_pose p;
      p.c = s_c[tid + 1u], p.s = s_s[tid + 1u], p.tx = s_t[0][tid + 1u], p.ty = s_t[1][tid + 1u], p.tz = s_t[2][tid + 1u];
      p.segment = s_seg[tid + 1u];
      p.flags = s_kind[tid] == 1u ? 0u : s_kind[tid] == 0u ? FX_POSE_GAP : FX_POSE_NO_SCAN;
      poses[b0 + tid] = p;
    }
    __syncthreads();
    if (tid == 0u) s_c[0] = s_c[n], s_s[0] = s_s[n], s_t[0][0] = s_t[0][n], s_t[1][0] = s_t[1][n], s_t[2][0] = s_t[2][n], s_seg[0] = s_seg[n];
  }
  __syncthreads();
  if (tid == 0u) A.counters[1] = s_gaps;
}

extern "C" __global__ __launch_bounds__(FXT_WG) void k_track_link(FxTrackArgs A) {
  const uint32_t r = blockIdx.x * FXT_WG + threadIdx.x;
  if (r >= A.K.q_max_rows) return;
  const KpView B = query_view(A.K);
  const uint32_t b = A.scan_of[r];
  int32_t prop = -1;
  if (b != FX_TRACK_NONE && b >= 1u && A.inlier[r] == 1u) {
    const fx_match m = reinterpret_cast<const fx_match *>(A.matches)[r];
    const uint32_t t = (uint32_t)m.train_row;
    if (m.pair == b - 1u && m.train_row >= 0 && t >= B.off[b - 1u] && t < B.off[b] && t < B.rows &&
        good_link(reinterpret_cast<const fx_registration *>(A.reg)[b - 1u]) && finite3(B.kp[r]) && finite3(B.kp[t])) {
      prop = m.train_row;
      atomicMin(&A.child[t], r);
    }
  }
  A.prop[r] = prop;
}

extern "C" __global__ __launch_bounds__(FXT_WG) void k_track_parent(FxTrackArgs A) {
  const uint32_t r = blockIdx.x * FXT_WG + threadIdx.x;
  bool lost = false;
  if (r < A.K.q_max_rows) {
    const int32_t t = A.prop[r];
    const bool kept = t >= 0 && A.child[t] == r;
    lost = t >= 0 && !kept;
    A.jump[0][r] = kept ? make_uint2((uint32_t)t, 1u) : make_uint2(r, 0u);
    A.len[r] = 0u;
  }
  count_wave(lost, &A.counters[0]);
}

extern "C" __global__ __launch_bounds__(FXT_WG) void k_track_jump(const uint2 *src, uint2 *dst, uint32_t n) {
  const uint32_t r = blockIdx.x * FXT_WG + threadIdx.x;
  if (r >= n) return;
  const uint2 a = src[r];
  const uint2 b = src[a.x];
  dst[r] = make_uint2(b.x, a.y + b.y);
}

extern "C" __global__ __launch_bounds__(FXT_WG) void k_track_len(FxTrackArgs A, const uint2 *jump) {
  const uint32_t r = blockIdx.x * FXT_WG + threadIdx.x;
  if (r >= A.K.q_max_rows || A.scan_of[r] == FX_TRACK_NONE || A.child[r] != FX_TRACK_NONE) return;
  const uint2 j = jump[r];  // a leaf: the one row of its track nobody kept as a parent
  A.len[j.x] = j.y + 1u;
}

extern "C" __global__ __launch_bounds__(FXT_WG) void k_track_sums(FxTrackArgs A, const uint2 *jump, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXT_NWAVE];
  const uint32_t n = landmark_len(A, jump, blockIdx.x * FXT_WG + threadIdx.x);
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXT_NWAVE>(n ? 1u : 0u, n, s_w, ea, eb, ta, tb);
  if (threadIdx.x == 0u) A.bsum[blockIdx.x] = ta, A.bsum[n_blocks + blockIdx.x] = tb;
}

extern "C" __global__ __launch_bounds__(FXT_WG) void k_track_top(FxTrackArgs A, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXT_NWAVE];
  uint32_t base_a, base_b;
  wg_scan2_blocks<FXT_NWAVE>(A.bsum, n_blocks, s_w, base_a, base_b);
  if (threadIdx.x == 0u) {
    const KpView B = query_view(A.K);
    fx_track_header h;
    h.scans = B.S, h.rows = B.rows;
    h.n_landmarks = base_a, h.n_obs = base_b, h.n_conflicts = A.counters[0], h.n_gaps = A.counters[1];
    h.reserved[0] = h.reserved[1] = 0u;
    *reinterpret_cast<fx_track_header *>(A.header) = h;
  }
}

extern "C" __global__ __launch_bounds__(FXT_WG) void k_track_number(FxTrackArgs A, const uint2 *jump, uint32_t n_blocks) {
  __shared__ uint32_t s_w[2 * FXT_NWAVE];
  const uint32_t r = blockIdx.x * FXT_WG + threadIdx.x;
  const uint32_t n = landmark_len(A, jump, r);
  uint32_t ea, eb, ta, tb;
  wg_scan2<FXT_NWAVE>(n ? 1u : 0u, n, s_w, ea, eb, ta, tb);
  if (r >= A.K.q_max_rows) return;
  if (n) {
    const uint32_t id = A.bsum[blockIdx.x] + ea;
    A.lm_id[r] = (int32_t)id;
    A.obs0[r] = A.bsum[n_blocks + blockIdx.x] + eb;
    A.lm_root[id] = r;
  } else {
    A.lm_id[r] = -1;
  }
}

extern "C" __global__ __launch_bounds__(FXT_WG) void k_track_scatter(FxTrackArgs A, const uint2 *jump) {
  const uint32_t r = blockIdx.x * FXT_WG + threadIdx.x;
  if (r >= A.K.q_max_rows || A.scan_of[r] == FX_TRACK_NONE) return;
  const uint2 j = jump[r];
  const int32_t id = A.lm_id[j.x];
  if (id < 0) return;
  A.landmark_of_row[r] = id;
  A.obs_row[A.obs0[j.x] + j.y] = r;
}

extern "C" __global__ __launch_bounds__(FXT_WG) void k_track_fuse(FxTrackArgs A) {
  const uint32_t i = blockIdx.x * FXT_WG + threadIdx.x;
  const fx_track_header *h = reinterpret_cast<const fx_track_header *>(A.header);
  if (i >= A.max_landmarks || i >= h->n_landmarks) return;
  const KpView B = query_view(A.K);
  const fx_pose *poses = reinterpret_cast<const fx_pose *>(A.poses);
  const uint32_t root = A.lm_root[i], n = A.len[root], o = A.obs0[root], first_scan = A.scan_of[root];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (uint32_t k = 0; k < n; ++k) {
    double wx, wy, wz;
    const float4 p = B.kp[A.obs_row[o + k]];
    world_point(poses[first_scan + k], p, wx, wy, wz);
    sx += wx, sy += wy, sz += wz;
  }
  const double dn = (double)n;
  const double mx = sx / dn, my = sy / dn, mz = sz / dn;
  double acc = 0.0;
  for (uint32_t k = 0; k < n; ++k) {
    double wx, wy, wz;
    const float4 p = B.kp[A.obs_row[o + k]];
    world_point(poses[first_scan + k], p, wx, wy, wz);
    const double dx = wx - mx, dy = wy - my;
    acc += (dx * dx + dy * dy);
  }
  fx_landmark L;
  L.x = mx, L.y = my, L.z = mz;
  L.rms_xy = (float)sqrt(acc / dn);
  L.n_obs = n, L.obs0 = o, L.first_row = root, L.first_scan = first_scan, L.last_scan = first_scan + n - 1u;
  reinterpret_cast<fx_landmark *>(A.landmarks)[i] = L;
}

extern "C" hipError_t fxk_track(hipStream_t s, const FxTrackArgs &A) {
  const uint32_t R = A.K.q_max_rows, nb = (R + FXT_WG - 1u) / FXT_WG;
  const dim3 wg(FXT_WG), grid(nb);
  if (nb) hipLaunchKernelGGL(k_track_init, grid, wg, 0, s, A);
  else (void)hipMemsetAsync(A.counters, 0, sizeof(uint32_t), s);
#ifndef FXT_SKIP_POSES
  hipLaunchKernelGGL(k_track_poses, dim3(1), wg, 0, s, A);
#endif
  uint32_t cur = 0u;
  if (nb) {
    hipLaunchKernelGGL(k_track_link, grid, wg, 0, s, A);
    hipLaunchKernelGGL(k_track_parent, grid, wg, 0, s, A);
    for (uint32_t span = 1u; span < A.K.n_scans; span <<= 1, cur ^= 1u)  // a chain has at most n_scans - 1 links
      hipLaunchKernelGGL(k_track_jump, grid, wg, 0, s, A.jump[cur], A.jump[cur ^ 1u], R);
    hipLaunchKernelGGL(k_track_len, grid, wg, 0, s, A, A.jump[cur]);
    hipLaunchKernelGGL(k_track_sums, grid, wg, 0, s, A, A.jump[cur], nb);
  }
  hipLaunchKernelGGL(k_track_top, dim3(1), wg, 0, s, A, nb);
  if (nb) {
    hipLaunchKernelGGL(k_track_number, grid, wg, 0, s, A, A.jump[cur], nb);
    hipLaunchKernelGGL(k_track_scatter, grid, wg, 0, s, A, A.jump[cur]);
    const uint32_t nl = R < A.max_landmarks ? R : A.max_landmarks;
    if (nl) hipLaunchKernelGGL(k_track_fuse, dim3((nl + FXT_WG - 1u) / FXT_WG), wg, 0, s, A);
  }
  return hipGetLastError();
}

extern "C" uint32_t fxk_track_wg_rows(void) { return FXT_WG; }
