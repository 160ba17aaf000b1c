// fx_map_append.hip — one landmark map appended to another: the source's landmarks behind the target's under new ids, its scans
// and segments numbered on from the target's, its carry in the place of the target's (include/fx.h fx_map_append).
//
// Every decision is an integer and no floating-point operation occurs: records and sums move as 16-byte vectors, 3 + 4 a landmark
// (as fx_map_compact.hip moves them), and only integer words are patched.  The same bytes from run to run and with any number of
// contexts in flight.  Counts come from the two headers on the device; the grid is sized by the smaller of the two capacities and
// exits early.
//
// The source is a view of six pointers (FxMapSrcView): a map's own buffers for fx_map_append, the sections of a snapshot staged in the
// context's scratch for fx_map_append_host.  It is only read.  Nothing of the target below its n_landmarks is written: the source's
// landmark i goes to id N + i, so nothing moves, nothing races and no second set of buffers is needed.
//
// Launches, in stream order (FXMA_WG = 256 threads a workgroup; N, M = the two headers' n_landmarks):
//   k_ma_decide  one lane: refusal or apply from the two headers; the state words st[] = the flags, N, the scan and segment bases, the
//                landmarks and carry rows to move (0 and 0 on a refusal).  The launch behind it reads the counts from these words
//                only, never from the target's header, which its last lane rewrites.
//   k_ma_apply   a thread a 16-byte vector: the M records (the thread that holds a record's integer words patches first_scan,
//                last_scan and segment), then the M sums; a thread an alias word and a carry row; one lane: the header and the result.
//                No thread reads a word that another thread of the launch writes.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "fx_device.h"
#include "fx_launch.h"
#include "../../include/fx.h"

#define FXMA_WG 256
#define FXMA_REC_V 3u  // 16-byte vectors of an fx_map_landmark
#define FXMA_ACC_V 4u  // ... of a landmark's FX_MAP_ACC doubles
#define FXMA_V (FXMA_REC_V + FXMA_ACC_V)

static_assert(sizeof(fx_map_landmark) == FXMA_REC_V * 16 && FX_MAP_ACC * sizeof(double) == FXMA_ACC_V * 16 && sizeof(fx_map_header) == 88 &&
                  sizeof(fx_map_append_result) == 32 && sizeof(fx_pose) == 48,
              "include/fx.h");
// the record's last vector holds exactly its integer words: first_scan, last_scan, segment, flags
static_assert(offsetof(fx_map_landmark, first_scan) == 32 && offsetof(fx_map_landmark, last_scan) == 36 && offsetof(fx_map_landmark, segment) == 40 &&
                  offsetof(fx_map_landmark, flags) == 44,
              "include/fx.h");

enum { ST_FLAGS = 0, ST_N, ST_SCANS, ST_SEGS, ST_M, ST_CARRY };  // the state words (FX_MAP_APPEND_ST_WORDS of them)

extern "C" __global__ void k_ma_decide(FxMapAppendArgs A) {
  if (blockIdx.x || threadIdx.x) return;
  const fx_map_header *D = reinterpret_cast<const fx_map_header *>(A.header);
  const fx_map_header *S = reinterpret_cast<const fx_map_header *>(A.src.header);
  const uint32_t N = min(D->n_landmarks, A.cap), M = min(S->n_landmarks, A.src_cap), r = min(S->carry_rows, A.src_max_carry);
  const uint64_t top = 0xffffffffull;
  uint32_t flags = 0u;
  if (S->scans == 0u) flags |= FX_APPEND_EMPTY;
  if (D->n_needed > D->n_landmarks || S->n_needed > S->n_landmarks) flags |= FX_APPEND_OVERFLOWED;
  if ((uint64_t)N + M > (uint64_t)A.cap) flags |= FX_APPEND_NO_ROOM;
  if ((uint64_t)D->scans + S->scans > top || (uint64_t)D->segments + S->segments > top || (uint64_t)D->batches + S->batches > top ||
      (uint64_t)D->n_obs + S->n_obs > top)
    flags |= FX_APPEND_TOO_LONG;
  const bool apply = flags == 0u;
  if (apply) flags = FX_APPEND_APPLIED | (r > A.max_carry ? FX_APPEND_CARRY_DROPPED : 0u);
  A.st[ST_FLAGS] = flags, A.st[ST_N] = N, A.st[ST_SCANS] = D->scans, A.st[ST_SEGS] = D->segments;
  A.st[ST_M] = apply ? M : 0u;
  A.st[ST_CARRY] = apply && r <= A.max_carry ? r : 0u;
}

extern "C" __global__ __launch_bounds__(FXMA_WG) void k_ma_apply(FxMapAppendArgs A) {
  const size_t t = (size_t)blockIdx.x * FXMA_WG + threadIdx.x;
  // (N + M <= cap, M <= src_cap, r <= min(max_carry, src_max_carry): k_ma_decide saw to it)
  const uint32_t N = A.st[ST_N], M = A.st[ST_M], r = A.st[ST_CARRY];
  const size_t n_rec = (size_t)M * FXMA_REC_V, n_acc = (size_t)M * FXMA_ACC_V;
  if (t < n_rec) {
    uint4 q = reinterpret_cast<const uint4 *>(A.src.records)[t];
    if (t % FXMA_REC_V == FXMA_REC_V - 1u) q.x += A.st[ST_SCANS], q.y += A.st[ST_SCANS], q.z += A.st[ST_SEGS];
    reinterpret_cast<uint4 *>(A.records)[(size_t)N * FXMA_REC_V + t] = q;
  } else if (t - n_rec < n_acc) {
    const size_t u = t - n_rec;
    reinterpret_cast<uint4 *>(A.acc)[(size_t)N * FXMA_ACC_V + u] = reinterpret_cast<const uint4 *>(A.src.acc)[u];
  }
  if (t < M) {
    const int32_t a = A.src.alias[t];
    A.alias[(size_t)N + t] = a >= 0 ? (int32_t)((uint32_t)a + N) : -1;
  }
  if (t < r) {
    const int32_t c = A.src.carry[t];
    A.carry[t] = c >= 0 ? (int32_t)((uint32_t)c + N) : -1;
    A.carry_kp[t] = A.src.carry_kp[t];
  }
  if (t) return;
  // (no other thread of this launch reads the target's header)
  fx_map_header *D = reinterpret_cast<fx_map_header *>(A.header);
  const fx_map_header *S = reinterpret_cast<const fx_map_header *>(A.src.header);
  const uint32_t flags = A.st[ST_FLAGS];
  if (flags & FX_APPEND_APPLIED) {
    D->n_landmarks = D->n_needed = N + M;
    D->n_obs += S->n_obs, D->scans += S->scans, D->batches += S->batches, D->segments += S->segments;
    D->flags |= S->flags;
    D->carry_rows = r;
    D->last_joined = S->last_joined, D->last_new = S->last_new;
    // last_pose as words: the bytes move, nothing is computed
    const uint32_t *sp = reinterpret_cast<const uint32_t *>(&S->last_pose);
    uint32_t *dp = reinterpret_cast<uint32_t *>(&D->last_pose);
    for (uint32_t k = 0; k < sizeof(fx_pose) / 4u; ++k) dp[k] = sp[k];
  }
  if (A.result) {
    A.result[0] = N, A.result[1] = A.st[ST_SCANS], A.result[2] = A.st[ST_SEGS], A.result[3] = M;
    A.result[4] = flags, A.result[5] = D->carry_rows, A.result[6] = A.result[7] = 0u;
  }
}

extern "C" hipError_t fxk_map_append(hipStream_t s, const FxMapAppendArgs &A) {
  const size_t lm = A.cap < A.src_cap ? A.cap : A.src_cap;
  const size_t rows = A.max_carry < A.src_max_carry ? A.max_carry : A.src_max_carry;
  size_t threads = lm * FXMA_V > rows ? lm * FXMA_V : rows;
  if (!threads) threads = 1;  // (the lane that writes the header and the result)
  hipLaunchKernelGGL(k_ma_decide, dim3(1), dim3(64), 0, s, A);
  hipLaunchKernelGGL(k_ma_apply, dim3((uint32_t)((threads + FXMA_WG - 1u) / FXMA_WG)), dim3(FXMA_WG), 0, s, A);
  return hipGetLastError();
}

// bytes of the context's scratch for an append that stages `stage_bytes` of a snapshot, and the pointers carved out of it
extern "C" size_t fxk_map_append_scratch(FxMapAppendArgs *A, uint8_t *base) {
  FxCarve C{base, 0};
  A->stage = C.take<uint8_t>(A->stage_bytes);
  A->st = C.take<uint32_t>(FX_MAP_APPEND_ST_WORDS);
  return C.o;
}
