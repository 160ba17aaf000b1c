"""Device time of folding a batch's landmark tracks into the persistent map (fx_map_update), next to the fx_track_landmarks call
that precedes it, on a run fed as overlapping batches.

  timeout -k 10 600 python tools/map_times.py [--scans 1024] [--batch 128] [--warmup 1] [--repeats 5] [--out profiles/map.json]

The two workloads of tools/track_times.py (profiles/track.json): `scenes` (independent scenes: links mostly bad, tracks short) and
`rotated` (one scan and its rotated copies: every link good, a pole followed through the run), --scans VLP-16 scans each, launch
preset, fx_limits_sparse, the scans resident on the device, one context.  The run is cut into batches of --batch scans that
overlap by one scan; every batch goes process -> pack block + CSR -> match (mutual) -> register -> track -> map with the map's
last_pose as the next init_pose.  The track call and the map update of every batch each sit between their own pair of HIP events
on the context's stream (the events are read after the run: nothing waits inside it); the run is repeated --repeats times after
--warmup runs, the map reset in between.  Reported per workload: the median over all batches and repeats of track_ms and map_ms,
the same for the first batch (nothing to join) and the later ones, and what the map held at the end.  No target is set: both are
a handful of small launches and are expected to be launch-bound.  Writes one JSON object.

  timeout -k 10 600 python tools/map_times.py --merge [--sizes 1000,100000,1000000] [--warmup 1] [--repeats 5] [--out profiles/map_merge_times.txt]

times fx_map_merge instead: for every size N a map of N landmarks laid out like a world, 1 pole per 250 m^2 in a square, two thirds
of the landmarks the first fragment of a pole (scans 0-1) and one third a second fragment of one of those poles (scans 2-3, up to
0.2 m off), built by ONE track -> fx_map_update of a synthetic four-scan block.  Every repeat resets the map, updates it, merges
(the call that does the work: N / 3 proposals, links and folds) and merges again (the fixpoint: the grid and the search, nothing to
fold); each call sits between its own pair of HIP events.  Reported per size: the medians, and the ratio of the merge time to the
size before; the requirement is time(10^6) <= 15 x time(10^5).

  timeout -k 10 600 python tools/map_times.py --compact [--sizes 1000,100000,1000000] [--warmup 1] [--repeats 5] [--out profiles/map_compact_times.txt]

times fx_map_compact on the same synthetic maps after their one merge (a third of the landmarks absorbed).  Every repeat resets the
map, updates it, merges, merges again on the fixpoint (timed: the grid and the search over N records, a third of them dead),
compacts (timed: one pair of HIP events around the call) and merges once more on the compacted map (timed: the same grid and search
over the 2 N / 3 live records).  Reported per size: the medians, the ratio of the compaction time to the size before (the merge's
requirement applies: time(10^6) <= 15 x time(10^5)) and the fixpoint merge after over before.

  timeout -k 10 600 python tools/map_times.py --relocalize [--sizes 10000,100000] [--warmup 1] [--repeats 3] [--out profiles/map_relocalize_times.txt]

times fx_map_relocalize on the same synthetic maps (built by one update, not merged: every landmark live): 8 scans a call, each of
the 64 poles nearest to a random position inside the map, seen from a random pose there; default options (16 seeds).  One pair of
HIP events around the call.  Reported per size: the median time of a call, the time per scan, how many scans came back VALID and
the mean n_hyp of a scan.  No target is set.
  timeout -k 10 600 python tools/map_times.py --join [--sizes 1000,100000,1000000] [--warmup 1] [--repeats 5] [--out profiles/map_join_times.txt]

times fx_map_join_segments on the same synthetic maps with the link between scans 1 and 2 made unusable: the first fragments (two
thirds of the landmarks) are segment 0, the second fragments (a third, up to 0.2 m beside their poles) segment 1, in one frame
(the motions are the identity), so the identity prior associates every second fragment.  Every repeat resets the map, updates it,
localises 8 scans of 64 keypoints against it (timed: fx_map_localize on the same map, any segment, the true poses as priors) and
joins segment 1 into segment 0 (timed: one pair of HIP events around the call: the grid, N / 3 queries, the consensus over the
first 1024 correspondences, N / 3 landmarks moved, N relabelled).  Reported per size: the medians and the join's result.  No
target is set.
  timeout -k 10 600 python tools/map_times.py --observe [--sizes 1000,100000,1000000] [--warmup 1] [--repeats 5] [--out profiles/map_observe.md]

times fx_map_observe on the synthetic maps of --join (the link left usable: one segment): every repeat resets the map, updates it,
localises 8 scans of 64 keypoints against it (timed: fx_map_localize, any segment, the true poses as priors) and folds the inlier
rows into their landmarks (timed: fx_map_observe reading the localise's records and table where they are: the memset, the seven
launches).  One pair of HIP events around each call.  Reported per size: the medians and the observe's result.  No target is set.
  timeout -k 10 600 python tools/map_times.py --expect [--sizes 1000,100000,1000000] [--warmup 1] [--repeats 5] [--out profiles/map_expect.md]

times fx_map_expect and fx_map_retire on the synthetic maps of --join (one segment): every repeat resets the map, updates and merges
it, localises 128 scans of 64 keypoints against it (timed: fx_map_localize, any segment, the true poses as priors), counts expected
and seen from the localise's device outputs (timed: fx_map_expect, FX_EXPECT_ADD into zeroed counters, a box and a range of 80 m
so that landmarks beyond the 64 a scan sees are expected: the grid build, the memset, the three launches) and retires on those
counters (timed: fx_map_retire, min_expected 1, seen / expected below 1 / 2); then it resets, updates and merges again and compacts
(timed: fx_map_compact, the same launches without the rule).  One pair of HIP events around each call.  No target is set.
  timeout -k 10 600 python tools/map_times.py --discover [--sizes 1000,100000,1000000] [--warmup 1] [--repeats 5] [--out profiles/map_discover_times.txt]

times fx_map_discover next to fx_map_observe on the synthetic maps of --observe, with room for 8 more landmarks: the 8 scans are taken
at one place, each 64 keypoints on the map's poles and 8 on poles the map does not hold (2 cm of jitter).  Every repeat resets the map,
updates it, localises (timed), observes (timed: the yardstick, on the same inputs) and discovers (timed: fx_map_discover with its
defaults reading the localise's records and table where they are: the two grid builds, the memset, the ten launches).  One pair of
HIP events around each call.  Reported per size: the medians and both results.  No target is set.
  timeout -k 10 600 python tools/map_times.py --loop [--sizes 1000,100000,1000000] [--warmup 1] [--repeats 5] [--out profiles/map_loop_times.txt]

times fx_map_close_loop on the same synthetic maps as one segment: the first fragments (scans 0-1) are the old landmarks, the second
fragments (scans 2-3, a third, up to 0.2 m beside their poles) the recent ones (min_loop_scans 2, recent_scans 1), under the identity
prior.  Every repeat resets the map, updates it and closes (timed: one pair of HIP events around the call: the grid, N / 3 queries,
the consensus over the first 1024 correspondences, N / 3 landmarks moved), then corrects 1024 poses (timed).  The join of --join is
timed on the same maps in the same run for the column beside it.  Reported per size: the medians and the closure's result.  No target
is set.
  timeout -k 10 600 python tools/map_times.py --find-loop [--sizes 10000,100000,1000000] [--warmup 1] [--repeats 5] [--out profiles/map_find_loop_times.txt]

times fx_map_find_loop: for every size N a map of one segment taken in as a snapshot: N - 40 old landmarks uniform in a square at the
loop world's density (1 pole per 160 m^2, scans 0-5) and 40 recent ones (scans 395-400, the highest ids): twins of the 40 poles
nearest to a random position, moved by a drift of 0.13 rad and 7.8 m with 1 cm of noise.  Timed with one pair of HIP events each:
fx_map_find_loop with default options (40 queries, 16 seeds), and on the same map fx_map_relocalize of one scan holding the same 40
points as float keypoints (any segment: it sees both copies), whose walk the new call shares.  Reported per size: the medians, their
ratio and the result.  No target is set.
  timeout -k 10 600 python tools/map_times.py --append [--sizes 1000,100000,1000000] [--warmup 1] [--repeats 5] [--out profiles/map_append.md]

times fx_map_append: for every size N a map of N landmarks (every landmark live, a carry scan of 16 rows) taken in as a snapshot
into a target of 2 N landmarks and into a source of N.  Every repeat imports the snapshot into the target (timed: fx_map_import_host,
the reset and the six copies from pinned memory), appends the source map (timed: fx_map_append of M = N landmarks into a map of N),
imports again, appends the same snapshot from the host (timed: fx_map_append_host, the copy of the staged block and the same
launches; the call's wall time with the staging memcpy is reported beside it) and copies 116 N bytes from one device buffer to
another with one hipMemcpyAsync (timed: what moving the bytes costs).  One pair of HIP events around each.  Reported per size: the
medians, the append over the plain copy, and the requirement the merge and the compaction meet: time(10^6) <= 15 x time(10^5).
  timeout -k 10 600 python tools/map_times.py --splice [--steps 200] [--warmup 1] [--repeats 5] [--out profiles/splice.md]

times fx_splice_blocks.  (1) One new scan a call, host to host (time.perf_counter around the calls and the wait for the stream),
the two routes to a block pair of [the scan before, the new scan] alternating over --steps VLP-16 scans resident on the device, one
context of two scans: `twice`, fx_process_batch of both scans and the two packs; `once`, fx_process_batch of the new scan, the two
packs and the splice behind the last scan of the block pair before.  Medians; the two routes' blocks are compared at every step.
(2) 1 + 1023 scans: synthetic block pairs (54 rows a scan, 40 entries a row), the splice of (previous, last, 1) with (current, 0,
1023) between one pair of HIP events, alternating with one hipMemcpyAsync, device to device, of the bytes the splice defines.
  timeout -k 10 600 python tools/map_times.py --follow [--sizes 10000,1000000] [--scans 1024] [--warmup 1] [--repeats 5] [--out profiles/map_follow_times.txt]

times fx_map_follow: a drive of --scans scans of 54 keypoints, 0.5 m apart on a gentle arc through the synthetic map, with links 2 %
long.  Timed with one pair of HIP events each: one chain of all the scans from the true first pose; chains of 16 scans from the true
poses; a chain of one scan (the grid build, the fill and one turn of the loop: what a call costs before its chains run); and
fx_map_localize over the same scans under the true poses (the parallel call the follow replaces when no good priors exist).  The
records of every call are asserted equal across repeats.  Reported per size: the medians with min and max, and the VALID scans.
No target is set.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feature_extraction_amd import capi  # noqa: E402
from tools.track_times import rotated  # noqa: E402


def measure(ctx, scans, roll, pitch, batch, warmup, repeats):
    import torch
    n, N = scans.shape[0], scans.shape[1]
    dev = torch.from_numpy(scans).cuda()
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    starts = list(range(0, n - batch + 1, batch - 1))
    B, R, cap = batch, ctx.limits.max_total_keypoints, ctx.limits.max_total_keypoints * 128
    buf = torch.empty(int(ctx.lib.fx_descriptor_csr_bytes(R, cap)), dtype=torch.uint8, device="cuda")
    kp = torch.empty(int(ctx.lib.fx_keypoint_block_bytes(B, R)), dtype=torch.uint8, device="cuda")
    match_t = torch.empty((R, 8), dtype=torch.int32, device="cuda")
    reg_t = torch.empty((B, 8), dtype=torch.float64, device="cuda")
    inl_t = torch.empty((R,), dtype=torch.int32, device="cuda")
    outs = (torch.empty((B, 6), dtype=torch.float64, device="cuda"), torch.empty((R,), dtype=torch.int32, device="cuda"),
            torch.empty((R,), dtype=torch.int32, device="cuda"), torch.empty((R, 6), dtype=torch.float64, device="cuda"),
            torch.empty((8,), dtype=torch.int32, device="cuda"))
    ids = torch.empty((R,), dtype=torch.int32, device="cuda")
    mp = ctx.map_create(n * ctx.limits.max_keypoints, ctx.limits.max_keypoints)
    mopt = capi.FxMatchOptions()
    ctx.lib.fx_match_options_default(C.byref(mopt))
    mopt.mutual = 1
    ropt = capi.FxRegisterOptions()
    ctx.lib.fx_register_options_default(C.byref(ropt))
    topt = capi.FxTrackOptions()
    ctx.lib.fx_track_options_default(C.byref(topt))
    P = C.c_void_p
    torch.cuda.synchronize()
    track_ms, map_ms, hdr = [], [], None
    for rep in range(warmup + repeats):
        mp.reset()
        pose, evs = None, []
        for k, a in enumerate(starts):
            descs = ctx.make_descs([dev.data_ptr() + (a + b) * N * 16 for b in range(B)], [N] * B, 16, roll, pitch)
            v = ctx.process_raw(descs, B, capi.FX_IN_DEVICE | capi.FX_OUT_HOST)
            off = capi._np(v.h_kp_offset, (B + 1,), np.uint32).astype(np.int64)
            pairs = capi.pairs_consecutive(off)
            arr = (capi.FxMatchPair * max(len(pairs), 1))(*[capi.FxMatchPair(*p) for p in pairs])
            ctx.pack_keypoint_block(kp.data_ptr(), B, R)
            ctx.pack_descriptors_csr(buf.data_ptr(), R, cap)
            capi.check(ctx.lib.fx_match_descriptors_csr(ctx.handle, P(buf.data_ptr()), R, cap, P(buf.data_ptr()), R, cap, arr, len(pairs),
                                                        C.byref(mopt), P(match_t.data_ptr())))
            capi.check(ctx.lib.fx_register_matches(ctx.handle, P(kp.data_ptr()), B, R, P(kp.data_ptr()), B, R, P(match_t.data_ptr()), R, arr,
                                                   len(pairs), C.byref(ropt), P(reg_t.data_ptr()), P(inl_t.data_ptr())))
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record(stream)
            capi.check(ctx.lib.fx_track_landmarks(ctx.handle, P(kp.data_ptr()), B, R, P(match_t.data_ptr()), P(inl_t.data_ptr()), R, P(reg_t.data_ptr()),
                                                  B, C.byref(pose) if pose is not None else None, C.byref(topt), P(outs[0].data_ptr()),
                                                  P(outs[1].data_ptr()), P(outs[2].data_ptr()), P(outs[3].data_ptr()), R, P(outs[4].data_ptr())))
            e[1].record(stream)
            e[2].record(stream)
            capi.check(ctx.lib.fx_map_update(ctx.handle, mp.handle, P(kp.data_ptr()), B, R, P(outs[0].data_ptr()), P(outs[1].data_ptr()),
                                             P(outs[2].data_ptr()), R, P(outs[3].data_ptr()), R, P(outs[4].data_ptr()),
                                             capi.FX_MAP_OVERLAP if k else 0, P(ids.data_ptr())))
            e[3].record(stream)
            evs.append(e)
            # the next batch's init_pose (a streaming caller reads it here too: the next process_batch waits for its outputs anyway)
            h = capi.FxMapHeader()
            capi.check(ctx.lib.fx_map_read_header(ctx.handle, mp.handle, C.byref(h)))
            pose = h.last_pose
        ctx.synchronize()
        if rep >= warmup:
            track_ms.append([e[0].elapsed_time(e[1]) for e in evs])
            map_ms.append([e[2].elapsed_time(e[3]) for e in evs])
        hdr = mp.header()
    mp.close()

    def stat(rows, sel):
        v = [x for r in rows for x in r[sel]]
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": len(v)} if v else None
    out = {"batches": len(starts), "scans_a_batch": B, "map": {k: hdr[k] for k in capi.MAP_HEADER_FIELDS}}
    for name, rows in (("track_ms", track_ms), ("map_ms", map_ms)):
        out[name] = stat(rows, slice(None))["median"]
        out[name + "_detail"] = {"all": stat(rows, slice(None)), "first_batch": stat(rows, slice(0, 1)), "later_batches": stat(rows, slice(1, None))}
    out["map_over_track"] = out["map_ms"] / out["track_ms"]
    return out


def merge_case(n, rng):
    """The four-scan block, match records, inlier words and registrations whose track holds n landmarks: roots in scans 0-1, members
    (a third) in scans 2-3.  Host arrays."""
    M = n // 3
    R = n - M
    side = (R * 250.0) ** 0.5
    roots = rng.uniform(0.0, side, (R, 2))
    of = rng.permutation(R)[:M]
    r, a = rng.uniform(0.0, 0.2, M), rng.uniform(0.0, 2 * np.pi, M)
    members = roots[of] + np.stack([r * np.cos(a), r * np.sin(a)], axis=1)
    off = np.array([0, R, 2 * R, 2 * R + M, 2 * R + 2 * M], np.uint32)
    rows = np.zeros((int(off[-1]), 4), np.float32)
    rows[:R, :2] = rows[R:2 * R, :2] = roots
    rows[2 * R:2 * R + M, :2] = rows[2 * R + M:, :2] = members
    rows[:, 2] = 1.0
    m = np.zeros(len(rows), capi.MATCH_DTYPE)
    m["train_row"], m["second_row"], m["dist2"], m["dist2_second"], m["pair"] = -1, -1, np.inf, np.inf, capi.FX_MATCH_NO_PAIR
    inl = np.zeros(len(rows), np.int32)
    for b, (lo, hi) in enumerate(zip(off[1:-1], off[2:]), start=1):
        m["pair"][lo:hi] = b - 1
    for lo, n_rows, src in ((R, R, 0), (2 * R + M, M, 2 * R)):
        m["train_row"][lo:lo + n_rows], m["flags"][lo:lo + n_rows], m["dist2"][lo:lo + n_rows], inl[lo:lo + n_rows] = np.arange(src, src + n_rows), capi.FX_MATCH_ACCEPTED, 1.0, 1
    reg = np.zeros(3, capi.REG_DTYPE)
    reg[:] = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 10, 10, capi.FX_REG_VALID, 0, 1)
    S, T = 4, len(rows)
    k0, n_blk = capi.keypoint_block_layout(S, T)
    blk = np.zeros((n_blk, 4), np.float32)
    u = blk.view(np.uint32).reshape(-1)
    u[:4] = (S, T, 0, T)
    u[4:4 + S + 1] = off
    u[4 + S + 1:capi.keypoint_block_layout(S, T).f0] = off[-1]
    blk[k0:k0 + T] = rows
    return blk.view(np.uint8).reshape(-1), (S, T), m, inl, reg, M


def measure_merge(ctx, n, warmup, repeats):
    import torch
    blk, (S, T), m, inl, reg, M = merge_case(n, np.random.default_rng(n))
    kp = (torch.from_numpy(blk).cuda(), S, T)
    md, inl_t = torch.from_numpy(m.view(np.int32).reshape(-1, 8).copy()).cuda(), torch.from_numpy(inl).cuda()
    reg_t = torch.from_numpy(reg.view(np.float64).reshape(-1, 8).copy()).cuda()
    out = ctx.track_landmarks(kp, md, inl_t, reg_t, S, max_landmarks=n)
    mp = ctx.map_create(n, 16)
    res = torch.zeros((4,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    t = {"update_ms": [], "merge_ms": [], "merge_fixpoint_ms": []}
    first = None
    for rep in range(warmup + repeats):
        mp.reset()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        e[0].record(stream)
        mp.update(kp, out, overlap=False, row_ids=False)
        e[1].record(stream), e[2].record(stream)
        mp.merge(result=res)
        e[3].record(stream)
        ctx.synchronize()
        got = res.cpu().numpy().tolist()
        e[4].record(stream)
        mp.merge(result=res)
        e[5].record(stream)
        ctx.synchronize()
        first = first or got
        assert got == first, (got, first)  # (merged may differ from M by a few: two poles may lie within the gate of one fragment)
        if rep >= warmup:
            for k, (a, b) in zip(t, ((0, 1), (2, 3), (4, 5))):
                t[k].append(e[a].elapsed_time(e[b]))
    hdr = mp.header()
    mp.close()
    out = {"landmarks": hdr["n_landmarks"], "mergeable": M, "result": dict(zip(capi.MAP_MERGE_RESULT_FIELDS, first))}
    for k, v in t.items():
        out[k] = statistics.median(v)
        out[k + "_min_max"] = [min(v), max(v)]
    return out


def measure_compact(ctx, n, warmup, repeats):
    import torch
    blk, (S, T), m, inl, reg, M = merge_case(n, np.random.default_rng(n))
    kp = (torch.from_numpy(blk).cuda(), S, T)
    md, inl_t = torch.from_numpy(m.view(np.int32).reshape(-1, 8).copy()).cuda(), torch.from_numpy(inl).cuda()
    reg_t = torch.from_numpy(reg.view(np.float64).reshape(-1, 8).copy()).cuda()
    out = ctx.track_landmarks(kp, md, inl_t, reg_t, S, max_landmarks=n)
    mp = ctx.map_create(n, 16)
    res, cres = (torch.zeros((4,), dtype=torch.int32, device="cuda") for _ in range(2))
    remap = torch.empty((n,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    t = {"fixpoint_before_ms": [], "compact_ms": [], "fixpoint_after_ms": []}
    first = None
    for rep in range(warmup + repeats):
        mp.reset()
        mp.update(kp, out, overlap=False, row_ids=False)
        mp.merge(result=res)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        e[0].record(stream)
        mp.merge(result=res)
        e[1].record(stream), e[2].record(stream)
        mp.compact(remap=remap, result=cres)
        e[3].record(stream), e[4].record(stream)
        mp.merge(result=res)
        e[5].record(stream)
        ctx.synchronize()
        got = cres.cpu().numpy().tolist() + res.cpu().numpy().tolist()
        first = first or got
        assert got == first and got[5] == 0 and got[1] == got[6], (got, first)  # (nothing merges on the fixpoint; live == kept)
        if rep >= warmup:
            for k, (a, b) in zip(t, ((0, 1), (2, 3), (4, 5))):
                t[k].append(e[a].elapsed_time(e[b]))
    hdr = mp.header()
    mp.close()
    out = {"landmarks": n, "after": hdr["n_landmarks"], "result": dict(zip(capi.MAP_COMPACT_RESULT_FIELDS, first[:4]))}
    for k, v in t.items():
        out[k] = statistics.median(v)
        out[k + "_min_max"] = [min(v), max(v)]
    return out


def measure_relocalize(ctx, n, warmup, repeats, n_scans=8):
    import torch
    blk, (S, T), m, inl, reg, M = merge_case(n, np.random.default_rng(n))
    kp = (torch.from_numpy(blk).cuda(), S, T)
    md, inl_t = torch.from_numpy(m.view(np.int32).reshape(-1, 8).copy()).cuda(), torch.from_numpy(inl).cuda()
    reg_t = torch.from_numpy(reg.view(np.float64).reshape(-1, 8).copy()).cuda()
    out = ctx.track_landmarks(kp, md, inl_t, reg_t, S, max_landmarks=n)
    mp = ctx.map_create(n, 16)
    mp.update(kp, out, overlap=False, row_ids=False)
    lm = mp.landmarks(0, mp.header()["n_landmarks"])
    xy = np.stack([lm["x"], lm["y"]], axis=1)
    rng = np.random.default_rng(n + 1)
    rows = np.zeros((n_scans * capi.FX_RELOC_MAX_KP, 4), np.float32)
    for b in range(n_scans):
        at, yaw = xy[rng.integers(len(xy))] + rng.uniform(-5.0, 5.0, 2), rng.uniform(-np.pi, np.pi)
        near = np.argsort(((xy - at) ** 2).sum(axis=1))[:capi.FX_RELOC_MAX_KP]
        d = xy[near] - at
        c, s = np.cos(yaw), np.sin(yaw)
        rows[b * 64:(b + 1) * 64, 0], rows[b * 64:(b + 1) * 64, 1], rows[b * 64:(b + 1) * 64, 2] = c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], 1.0
    T2 = len(rows)
    k0, n_blk = capi.keypoint_block_layout(n_scans, T2)
    sb = np.zeros((n_blk, 4), np.float32)
    u = sb.view(np.uint32).reshape(-1)
    u[:4] = (n_scans, T2, 0, T2)
    u[4:4 + n_scans + 1] = np.arange(n_scans + 1) * 64
    sb[k0:k0 + T2] = rows
    skp = (torch.from_numpy(sb.view(np.uint8).reshape(-1)).cuda(), n_scans, T2)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    ms, rec = [], None
    for rep in range(warmup + repeats):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record(stream)
        recs, _ = mp.relocalize(skp, n_scans)
        e[1].record(stream)
        ctx.synchronize()
        rec = capi.relocalize_records(recs)
        if rep >= warmup:
            ms.append(e[0].elapsed_time(e[1]))
    mp.close()
    return {"landmarks": int(len(xy)), "scans": n_scans, "call_ms": statistics.median(ms), "call_ms_min_max": [min(ms), max(ms)],
            "valid": int((rec["flags"] & capi.FX_RELOC_VALID != 0).sum()), "n_hyp_mean": float(rec["n_hyp"].mean()), "n_seeds": rec["n_seeds"].tolist()}


def localize_scene(ctx, n, n_scans, cut_link, new_poles=0):
    """What --join and --observe localise against: merge_case(n) through one track and one update into a map of n landmarks
    (cut_link: the link scan 2 -> scan 1 made unusable, the second fragments a segment of their own), and n_scans scans of the 64
    poles nearest to a random position inside the map, seen from a random pose there, with the true poses as priors.  new_poles
    (--discover): the map has room for that many more landmarks, every scan is taken at ONE position (another yaw each) and ends in
    that many rows on poles the map does not hold, within 30 m of the position and 2 cm of jitter.  Returns (the map, the batch's
    block, the track's outputs, the scans' block, the priors): device tensors."""
    import torch
    blk, (S, T), m, inl, reg, M = merge_case(n, np.random.default_rng(n))
    if cut_link:
        reg["flags"][1] = 0
    kp = (torch.from_numpy(blk).cuda(), S, T)
    md, inl_t = torch.from_numpy(m.view(np.int32).reshape(-1, 8).copy()).cuda(), torch.from_numpy(inl).cuda()
    reg_t = torch.from_numpy(reg.view(np.float64).reshape(-1, 8).copy()).cuda()
    out = ctx.track_landmarks(kp, md, inl_t, reg_t, S, max_landmarks=n)
    mp = ctx.map_create(n + new_poles, 16)
    mp.update(kp, out, overlap=False, row_ids=False)
    lm = mp.landmarks(0, mp.header()["n_landmarks"])
    xy = np.stack([lm["x"], lm["y"]], axis=1)
    rng = np.random.default_rng(n + 1)
    K = capi.FX_RELOC_MAX_KP
    per = K + new_poles
    rows, pri = np.zeros((n_scans * per, 4), np.float32), np.zeros(n_scans, capi.POSE_DTYPE)
    one_place = xy[rng.integers(len(xy))] + rng.uniform(-5.0, 5.0, 2) if new_poles else None
    new_xy = one_place + rng.uniform(-30.0, 30.0, (new_poles, 2)) if new_poles else None
    for b in range(n_scans):
        at, yaw = xy[rng.integers(len(xy))] + rng.uniform(-5.0, 5.0, 2), rng.uniform(-np.pi, np.pi)
        if new_poles:
            at = one_place
        near = np.argsort(((xy - at) ** 2).sum(axis=1))[:K]
        d = xy[near] - at
        if new_poles:
            d = np.concatenate([d, new_xy + rng.normal(0.0, 0.02, new_xy.shape) - at])
        c, s = np.cos(yaw), np.sin(yaw)
        rows[b * per:(b + 1) * per, 0], rows[b * per:(b + 1) * per, 1], rows[b * per:(b + 1) * per, 2] = c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], 1.0
        pri[b] = (c, s, at[0], at[1], 0.0, 0, 0)
    T2 = len(rows)
    k0, n_blk = capi.keypoint_block_layout(n_scans, T2)
    sb = np.zeros((n_blk, 4), np.float32)
    u = sb.view(np.uint32).reshape(-1)
    u[:4] = (n_scans, T2, 0, T2)
    u[4:4 + n_scans + 1] = np.arange(n_scans + 1) * per
    sb[k0:k0 + T2] = rows
    skp = (torch.from_numpy(sb.view(np.uint8).reshape(-1)).cuda(), n_scans, T2)
    pri_t = torch.from_numpy(pri.view(np.float64).reshape(-1, 6).copy()).cuda()
    return mp, kp, out, skp, pri_t


def measure_join(ctx, n, warmup, repeats, n_scans=8):
    import torch
    mp, kp, out, skp, pri_t = localize_scene(ctx, n, n_scans, cut_link=True)
    res = torch.zeros((capi.JOIN_DTYPE.itemsize // 8,), dtype=torch.float64, device="cuda")
    match = torch.empty((n,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    t = {"localize_ms": [], "join_ms": []}
    first, valid = None, 0
    for rep in range(warmup + repeats):
        mp.reset()
        mp.update(kp, out, overlap=False, row_ids=False)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(stream)
        recs, _, _ = mp.localize(skp, pri_t, n_scans, nearest=False, segment=capi.FX_LOC_ANY_SEGMENT)
        e[1].record(stream), e[2].record(stream)
        mp.join_segments(1, 0, result=res, match=match)
        e[3].record(stream)
        ctx.synchronize()
        got = capi.join_records(res)[0]
        valid = int((capi.localize_records(recs)["flags"] & capi.FX_LOC_VALID != 0).sum())
        first = got if first is None else first
        assert got.tobytes() == first.tobytes() and got["flags"] & capi.FX_JOIN_APPLIED, (got, first)
        if rep >= warmup:
            for k, (a, b) in zip(t, ((0, 1), (2, 3))):
                t[k].append(e[a].elapsed_time(e[b]))
    hdr = mp.header()
    mp.close()
    out = {"landmarks": n, "segments_after": hdr["segments"], "localize_valid": valid,
           "result": {k: (float(first[k]) if first[k].dtype.kind == "f" else int(first[k])) for k in capi.JOIN_DTYPE.names}}
    for k, v in t.items():
        out[k] = statistics.median(v)
        out[k + "_min_max"] = [min(v), max(v)]
    return out


def measure_observe(ctx, n, warmup, repeats, n_scans=8):
    import torch
    mp, kp, out, skp, pri_t = localize_scene(ctx, n, n_scans, cut_link=False)
    res = torch.zeros((8,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    t = {"localize_ms": [], "observe_ms": []}
    first, valid = None, 0
    for rep in range(warmup + repeats):
        mp.reset()
        mp.update(kp, out, overlap=False, row_ids=False)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(stream)
        recs, ids, _ = mp.localize(skp, pri_t, n_scans, nearest=False, segment=capi.FX_LOC_ANY_SEGMENT)
        e[1].record(stream), e[2].record(stream)
        mp.observe(skp, recs, n_scans, ids, out=res, gained=False, observed=False)
        e[3].record(stream)
        ctx.synchronize()
        got = capi.observe_records(res)
        valid = int((capi.localize_records(recs)["flags"] & capi.FX_LOC_VALID != 0).sum())
        first = got if first is None else first
        assert got == first and got["added"] > 0, (got, first)
        if rep >= warmup:
            for k, (a, b) in zip(t, ((0, 1), (2, 3))):
                t[k].append(e[a].elapsed_time(e[b]))
    mp.close()
    out = {"landmarks": n, "localize_valid": valid, "result": first}
    for k, v in t.items():
        out[k] = statistics.median(v)
        out[k + "_min_max"] = [min(v), max(v)]
    return out


def measure_discover(ctx, n, warmup, repeats, n_scans=8, new_poles=8):
    import torch
    mp, kp, out, skp, pri_t = localize_scene(ctx, n, n_scans, cut_link=False, new_poles=new_poles)
    ores = torch.zeros((8,), dtype=torch.int32, device="cuda")
    dres = torch.zeros((16,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    t = {"localize_ms": [], "observe_ms": [], "discover_ms": []}
    first = None
    for rep in range(warmup + repeats):
        mp.reset()
        mp.update(kp, out, overlap=False, row_ids=False)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        e[0].record(stream)
        recs, ids, _ = mp.localize(skp, pri_t, n_scans, nearest=False, segment=capi.FX_LOC_ANY_SEGMENT)
        e[1].record(stream), e[2].record(stream)
        mp.observe(skp, recs, n_scans, ids, out=ores, gained=False, observed=False)
        e[3].record(stream), e[4].record(stream)
        mp.discover(skp, recs, n_scans, ids, out=dres, new_id=False)
        e[5].record(stream)
        ctx.synchronize()
        got = (capi.discover_records(dres), capi.observe_records(ores))
        first = got if first is None else first
        assert got == first and got[0]["created"] > 0, (got, first)
        if rep >= warmup:
            for k, (a, b) in zip(t, ((0, 1), (2, 3), (4, 5))):
                t[k].append(e[a].elapsed_time(e[b]))
    mp.close()
    out = {"landmarks": n, "scans": n_scans, "discover": first[0], "observe": first[1]}
    for k, v in t.items():
        out[k] = statistics.median(v)
        out[k + "_min_max"] = [min(v), max(v)]
    return out


def main_discover(a):
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    rows = [measure_discover(ctx, n, a.warmup, a.repeats) for n in sizes]
    ctx.close()
    lines = [f"fx_map_discover next to fx_map_observe, both behind one fx_map_localize, on synthetic maps (tools/map_times.py --discover): 1 pole",
             f"per 250 m^2, one segment; a call: 8 scans taken at one place, 64 keypoints on the map's poles and 8 on poles it does not hold each,",
             f"localised (any segment, the true poses as priors), then observed and then discovered from the localise's device outputs (default",
             f"options); one context, HIP events around each call, median of {a.repeats} after {a.warmup} warm-up; ms",
             f"{'landmarks':>10} {'used':>5} {'unmatched':>10} {'known':>6} {'free':>5} {'leaders':>8} {'dup':>4} {'weak':>5} {'added':>6} {'created':>8} "
             f"{'discover':>9} {'min':>8} {'max':>8} {'observe':>9} {'min':>8} {'max':>8} {'localize':>9}"]
    for r in rows:
        q = r["discover"]
        lines.append(f"{r['landmarks']:>10} {q['scans_used']:>5} {q['unmatched']:>10} {q['known']:>6} {q['free_rows']:>5} {q['leaders']:>8} {q['duplicates']:>4} "
                     f"{q['weak']:>5} {q['added']:>6} {q['created']:>8} {r['discover_ms']:>9.3f} {r['discover_ms_min_max'][0]:>8.3f} {r['discover_ms_min_max'][1]:>8.3f} "
                     f"{r['observe_ms']:>9.3f} {r['observe_ms_min_max'][0]:>8.3f} {r['observe_ms_min_max'][1]:>8.3f} {r['localize_ms']:>9.3f}")
    s = "\n".join(lines)
    print(s)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


EXPECT_OPTS = dict(x_min=-80.0, x_max=80.0, y_min=-80.0, y_max=80.0, min_range=0.0, max_range=80.0)


def measure_expect(ctx, n, warmup, repeats, n_scans=128):
    import torch
    mp, kp, out, skp, pri_t = localize_scene(ctx, n, n_scans, cut_link=False)
    res, rres = (torch.zeros((8,), dtype=torch.int32, device="cuda") for _ in range(2))
    cres, mres = (torch.zeros((4,), dtype=torch.int32, device="cuda") for _ in range(2))
    counters = [torch.zeros((n,), dtype=torch.int32, device="cuda") for _ in range(2)]
    remap = torch.empty((n,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    t = {"localize_ms": [], "expect_ms": [], "retire_ms": [], "compact_ms": []}
    first = None
    for rep in range(warmup + repeats):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        mp.reset()
        mp.update(kp, out, overlap=False, row_ids=False)
        mp.merge(result=mres)
        for c in counters:
            c.zero_()
        e[0].record(stream)
        recs, ids, _ = mp.localize(skp, pri_t, n_scans, nearest=False, segment=capi.FX_LOC_ANY_SEGMENT)
        e[1].record(stream), e[2].record(stream)
        mp.expect(skp, recs, n_scans, ids, out=res, expected=counters[0], seen=counters[1], mode=capi.FX_EXPECT_ADD, **EXPECT_OPTS)
        e[3].record(stream), e[4].record(stream)
        mp.retire(counters[0], counters[1], remap=remap, retired=False, result=rres, min_expected=1, seen_num=1, seen_den=2)
        e[5].record(stream)
        mp.reset()
        mp.update(kp, out, overlap=False, row_ids=False)
        mp.merge(result=mres)
        e[6].record(stream)
        mp.compact(remap=remap, result=cres)
        e[7].record(stream)
        ctx.synchronize()
        got = (capi.expect_records(res), capi.retire_records(rres), cres.cpu().numpy().tolist())
        first = got if first is None else first
        assert got == first and got[0]["seen"] > 0 and got[1]["before"] == got[2][0] and got[1]["dropped_absorbed"] == got[2][2], (got, first)
        if rep >= warmup:
            for k, (a, b) in zip(t, ((0, 1), (2, 3), (4, 5), (6, 7))):
                t[k].append(e[a].elapsed_time(e[b]))
    mp.close()
    out = {"landmarks": n, "scans": n_scans, "expect": first[0], "retire": first[1], "compact": dict(zip(capi.MAP_COMPACT_RESULT_FIELDS, first[2]))}
    for k, v in t.items():
        out[k] = statistics.median(v)
        out[k + "_min_max"] = [min(v), max(v)]
    return out


def main_expect(a):
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    rows = [measure_expect(ctx, n, a.warmup, a.repeats) for n in sizes]
    ctx.close()
    lines = [f"fx_map_expect behind fx_map_localize, and fx_map_retire next to fx_map_compact, on synthetic maps (tools/map_times.py --expect):",
             f"1 pole per 250 m^2, one segment, merged; a call: 128 scans of 64 keypoints localised (any segment, the true poses as priors), then",
             f"expected / seen counted from the localise's device outputs (box and range 80 m, adding), then retired (min_expected 1, seen /",
             f"expected < 1 / 2); the compaction on the same merged map; one context, HIP events around each call, median of {a.repeats} after",
             f"{a.warmup} warm-up; ms",
             f"{'landmarks':>10} {'used':>5} {'in_range':>9} {'shadowed':>9} {'expected':>9} {'seen':>7} {'lm_exp':>7} {'retired':>8} {'absorbed':>9} "
             f"{'expect':>8} {'min':>7} {'max':>7} {'localize':>9} {'retire':>8} {'min':>7} {'max':>7} {'compact':>8} {'min':>7} {'max':>7}"]
    for r in rows:
        q, v = r["expect"], r["retire"]
        lines.append(f"{r['landmarks']:>10} {q['scans_used']:>5} {q['in_range']:>9} {q['shadowed']:>9} {q['expected']:>9} {q['seen']:>7} {q['landmarks_expected']:>7} "
                     f"{v['retired']:>8} {v['dropped_absorbed']:>9} {r['expect_ms']:>8.3f} {r['expect_ms_min_max'][0]:>7.3f} {r['expect_ms_min_max'][1]:>7.3f} "
                     f"{r['localize_ms']:>9.3f} {r['retire_ms']:>8.3f} {r['retire_ms_min_max'][0]:>7.3f} {r['retire_ms_min_max'][1]:>7.3f} "
                     f"{r['compact_ms']:>8.3f} {r['compact_ms_min_max'][0]:>7.3f} {r['compact_ms_min_max'][1]:>7.3f}")
    s = "\n".join(lines)
    print(s)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


def follow_scene(ctx, n, n_scans, per=54, step=0.5):
    """What --follow drives through: merge_case(n) through one track and one update into a map of n landmarks, and a drive of
    n_scans scans, `step` metres apart on a gentle arc from the map's middle, each the `per` poles nearest to the sensor.  Returns
    (the map, the scans' block, the links between consecutive scans, the true poses): device tensors, the poses also as records."""
    import torch
    blk, (S, T), m, inl, reg, M = merge_case(n, np.random.default_rng(n))
    kp = (torch.from_numpy(blk).cuda(), S, T)
    md, inl_t = torch.from_numpy(m.view(np.int32).reshape(-1, 8).copy()).cuda(), torch.from_numpy(inl).cuda()
    reg_t = torch.from_numpy(reg.view(np.float64).reshape(-1, 8).copy()).cuda()
    mp = ctx.map_create(n, 16)
    mp.update(kp, ctx.track_landmarks(kp, md, inl_t, reg_t, S, max_landmarks=n), overlap=False, row_ids=False)
    lm = mp.landmarks(0, mp.header()["n_landmarks"])
    xy = np.stack([lm["x"], lm["y"]], axis=1)
    yaw = 0.3 + 0.0005 * np.arange(n_scans)
    at = np.median(xy, axis=0) + np.concatenate([[[0.0, 0.0]], np.cumsum(step * np.stack([np.cos(yaw[:-1]), np.sin(yaw[:-1])], axis=1), axis=0)])
    box = xy[(np.abs(xy - (at.min(axis=0) + at.max(axis=0)) / 2) <= np.ptp(at, axis=0) / 2 + 150.0).all(axis=1)]  # (the poles the drive can see)
    assert len(box) >= per, "the map is too small for the drive"
    rows, poses, links = np.zeros((n_scans * per, 4), np.float32), np.zeros(n_scans, capi.POSE_DTYPE), np.zeros(max(n_scans - 1, 1), capi.REG_DTYPE)
    for b in range(n_scans):
        d = box[np.argpartition(((box - at[b]) ** 2).sum(axis=1), per - 1)[:per]] - at[b]
        c, s = np.cos(yaw[b]), np.sin(yaw[b])
        rows[b * per:(b + 1) * per, 0], rows[b * per:(b + 1) * per, 1], rows[b * per:(b + 1) * per, 2] = c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], 1.0
        poses[b] = (c, s, at[b, 0], at[b, 1], 0.0, 0, 0)
        if b:  # scan b -> scan b - 1, 2 % long: the odometry's bias
            c0, s0, dx, dy, dyaw = np.cos(yaw[b - 1]), np.sin(yaw[b - 1]), *(at[b] - at[b - 1]), yaw[b] - yaw[b - 1]
            links[b - 1] = (np.cos(dyaw), np.sin(dyaw), 1.02 * (c0 * dx + s0 * dy), 1.02 * (-s0 * dx + c0 * dy), 0.0, 0.0, per, per, capi.FX_REG_VALID, 0, 1)
    T2 = len(rows)
    k0, n_blk = capi.keypoint_block_layout(n_scans, T2)
    sb = np.zeros((n_blk, 4), np.float32)
    u = sb.view(np.uint32).reshape(-1)
    u[:4] = (n_scans, T2, 0, T2)
    u[4:4 + n_scans + 1] = np.arange(n_scans + 1) * per
    sb[k0:k0 + T2] = rows
    skp = (torch.from_numpy(sb.view(np.uint8).reshape(-1)).cuda(), n_scans, T2)
    dev = lambda a, w: torch.from_numpy(a.view(np.float64).reshape(-1, w).copy()).cuda()
    return mp, skp, dev(links, 8), dev(poses, 6), poses


def measure_follow(ctx, n, warmup, repeats, n_scans=1024, chain=16):
    import torch
    mp, skp, links, poses_t, poses = follow_scene(ctx, n, n_scans)
    starts = torch.from_numpy(poses[::chain].copy().view(np.float64).reshape(-1, 6).copy()).cuda()
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    calls = {"one_chain_ms": lambda: mp.follow(skp, links, poses_t, n_scans, nearest=False)[0],
             "chains_ms": lambda: mp.follow(skp, links, starts, n_scans, nearest=False, chain_scans=chain)[0],
             "one_scan_ms": lambda: mp.follow(skp, None, poses_t, 1, nearest=False)[0],
             "localize_ms": lambda: mp.localize(skp, poses_t, n_scans, nearest=False, segment=capi.FX_LOC_ANY_SEGMENT)[0]}
    torch.cuda.synchronize()
    t, first, valid = {k: [] for k in calls}, {}, {}
    for rep in range(warmup + repeats):
        for k, call in calls.items():
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record(stream)
            recs = call()
            e[1].record(stream)
            ctx.synchronize()
            got = capi.localize_records(recs)
            assert first.setdefault(k, got.tobytes()) == got.tobytes(), f"{k}: other bytes in repeat {rep}"
            valid[k] = int((got["flags"] & capi.FX_LOC_VALID != 0).sum())
            if rep >= warmup:
                t[k].append(e[0].elapsed_time(e[1]))
    mp.close()
    out = {"landmarks": n, "scans": n_scans, "chain_scans": chain, "valid": valid}
    for k, v in t.items():
        out[k] = statistics.median(v)
        out[k + "_min_max"] = [min(v), max(v)]
    return out


def main_follow(a):
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    rows = [measure_follow(ctx, n, a.warmup, a.repeats, a.scans) for n in sizes]
    ctx.close()
    lines = [f"fx_map_follow next to fx_map_localize on synthetic maps (tools/map_times.py --follow): 1 pole per 250 m^2, one segment; a drive of",
             f"{a.scans} scans of 54 keypoints, 0.5 m apart, links 2 % long; one chain of all scans, chains of 16 scans from the true poses, a chain",
             f"of 1 scan (the grid build, the fill and one turn), and fx_map_localize over the same scans under the true poses; one context,",
             f"HIP events around each call, median of {a.repeats} after {a.warmup} warm-up; ms (min .. max); valid: scans FX_LOC_VALID",
             f"{'landmarks':>10} {'one chain':>24} {'valid':>6} {'chains of 16':>24} {'valid':>6} {'one scan':>24} {'localize':>24} {'valid':>6}"]
    cell = lambda r, k: f"{r[k]:>9.3f} ({r[k + '_min_max'][0]:.3f} .. {r[k + '_min_max'][1]:.3f})".rjust(24)
    for r in rows:
        lines.append(f"{r['landmarks']:>10} {cell(r, 'one_chain_ms')} {r['valid']['one_chain_ms']:>6} {cell(r, 'chains_ms')} {r['valid']['chains_ms']:>6} "
                     f"{cell(r, 'one_scan_ms')} {cell(r, 'localize_ms')} {r['valid']['localize_ms']:>6}")
    s = "\n".join(lines)
    print(s)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


def main_observe(a):
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    rows = [measure_observe(ctx, n, a.warmup, a.repeats) for n in sizes]
    ctx.close()
    lines = [f"fx_map_observe behind fx_map_localize on synthetic maps (tools/map_times.py --observe): 1 pole per 250 m^2, one segment; a call:",
             f"8 scans of 64 keypoints localised (any segment, the true poses as priors), then observed from the localise's device outputs; one",
             f"context, HIP events around each call, median of {a.repeats} after {a.warmup} warm-up; ms",
             f"{'landmarks':>10} {'used':>5} {'proposed':>9} {'added':>6} {'dup':>4} {'gated':>6} {'stale':>6} {'touched':>8} {'observe':>9} {'min':>8} {'max':>8} {'localize':>9} {'valid':>6}"]
    for r in rows:
        q = r["result"]
        lines.append(f"{r['landmarks']:>10} {q['scans_used']:>5} {q['proposed']:>9} {q['added']:>6} {q['duplicates']:>4} {q['gated']:>6} {q['stale']:>6} "
                     f"{q['landmarks_touched']:>8} {r['observe_ms']:>9.3f} {r['observe_ms_min_max'][0]:>8.3f} {r['observe_ms_min_max'][1]:>8.3f} "
                     f"{r['localize_ms']:>9.3f} {r['localize_valid']:>6}")
    s = "\n".join(lines)
    print(s)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


def main_join(a):
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    rows = [measure_join(ctx, n, a.warmup, a.repeats) for n in sizes]
    ctx.close()
    lines = [f"fx_map_join_segments next to fx_map_localize on synthetic maps (tools/map_times.py --join): 1 pole per 250 m^2, a third of the",
             f"landmarks second fragments in a segment of their own (segment 1 joined into segment 0 under the identity prior); localize: 8 scans",
             f"of 64 keypoints, any segment; one context, HIP events around each call, median of {a.repeats} after {a.warmup} warm-up; ms",
             f"{'landmarks':>10} {'queries':>8} {'corr':>6} {'inliers':>8} {'moved':>8} {'flags':>6} {'join':>9} {'join / size before':>19} {'localize':>9} {'valid':>6}"]
    for k, r in enumerate(rows):
        ratio = f"{r['join_ms'] / rows[k - 1]['join_ms']:.2f}" if k else "-"
        q = r["result"]
        lines.append(f"{r['landmarks']:>10} {q['n_src']:>8} {q['n_corr']:>6} {q['n_inliers']:>8} {q['moved']:>8} {q['flags']:>#6x} {r['join_ms']:>9.3f} {ratio:>19} "
                     f"{r['localize_ms']:>9.3f} {r['localize_valid']:>6}")
    s = "\n".join(lines)
    print(s)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


def measure_loop(ctx, n, warmup, repeats, n_poses=1024):
    import torch
    blk, (S, T), m, inl, reg, M = merge_case(n, np.random.default_rng(n))
    kp = (torch.from_numpy(blk).cuda(), S, T)
    md, inl_t = torch.from_numpy(m.view(np.int32).reshape(-1, 8).copy()).cuda(), torch.from_numpy(inl).cuda()
    reg_t = torch.from_numpy(reg.view(np.float64).reshape(-1, 8).copy()).cuda()
    out = ctx.track_landmarks(kp, md, inl_t, reg_t, S, max_landmarks=n)
    mp = ctx.map_create(n, 16)
    res = torch.zeros((capi.LOOP_DTYPE.itemsize // 8,), dtype=torch.float64, device="cuda")
    match = torch.empty((n,), dtype=torch.int32, device="cuda")
    poses0 = np.zeros(n_poses, capi.POSE_DTYPE)
    poses0["c"] = 1.0
    poses_h = torch.from_numpy(poses0.view(np.float64).reshape(-1, 6).copy()).cuda()
    poses = poses_h.clone()
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    t = {"loop_ms": [], "poses_ms": []}
    first = None
    for rep in range(warmup + repeats):
        mp.reset()
        mp.update(kp, out, overlap=False, row_ids=False)
        poses.copy_(poses_h)
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(stream)
        mp.close_loop(result=res, match=match, min_loop_scans=2, recent_scans=1)
        e[1].record(stream), e[2].record(stream)
        mp.loop_correct_poses(res, poses, 0)
        e[3].record(stream)
        ctx.synchronize()
        got = capi.loop_records(res)[0]
        first = got if first is None else first
        assert got.tobytes() == first.tobytes() and got["flags"] & capi.FX_LOOP_APPLIED, (got, first)
        if rep >= warmup:
            for k, (a, b) in zip(t, ((0, 1), (2, 3))):
                t[k].append(e[a].elapsed_time(e[b]))
    mp.close()
    out = {"landmarks": n, "result": {k: (float(first[k]) if first[k].dtype.kind == "f" else int(first[k])) for k in capi.LOOP_DTYPE.names}}
    for k, v in t.items():
        out[k] = statistics.median(v)
        out[k + "_min_max"] = [min(v), max(v)]
    return out


def main_loop(a):
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    rows = [dict(measure_loop(ctx, n, a.warmup, a.repeats), join_ms=measure_join(ctx, n, a.warmup, a.repeats)["join_ms"]) for n in sizes]
    ctx.close()
    lines = [f"fx_map_close_loop next to fx_map_join_segments on synthetic maps (tools/map_times.py --loop): 1 pole per 250 m^2, a third of the",
             f"landmarks second fragments two scans later (the recent ones, closed onto the first under the identity prior; for the join they are",
             f"a segment of their own); poses: fx_map_loop_correct_poses on 1024 poses; one context, HIP events around each call, median of",
             f"{a.repeats} after {a.warmup} warm-up; ms",
             f"{'landmarks':>10} {'queries':>8} {'corr':>6} {'inliers':>8} {'moved':>8} {'flags':>6} {'loop':>9} {'loop / size before':>19} {'poses':>9} {'join':>9}"]
    for k, r in enumerate(rows):
        ratio = f"{r['loop_ms'] / rows[k - 1]['loop_ms']:.2f}" if k else "-"
        q = r["result"]
        lines.append(f"{r['landmarks']:>10} {q['n_query']:>8} {q['n_corr']:>6} {q['n_inliers']:>8} {q['moved']:>8} {q['flags']:>#6x} {r['loop_ms']:>9.3f} {ratio:>19} "
                     f"{r['poses_ms']:>9.3f} {r['join_ms']:>9.3f}")
    s = "\n".join(lines)
    print(s)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


def find_loop_case(n, rng, n_recent=40):
    """(the snapshot of a one-segment map of n landmarks, the recent ones' x, y, z): n - n_recent old landmarks of two observations at 1
    pole per 160 m^2 and n_recent recent twins of the poles nearest to a random position, drifted."""
    n_old = n - n_recent
    side = (n_old * 160.0) ** 0.5
    old = np.concatenate([rng.uniform(0.0, side, (n_old, 2)), rng.uniform(0.0, 2.0, (n_old, 1))], axis=1).astype(np.float32).astype(np.float64)
    at = rng.uniform(0.25 * side, 0.75 * side, 2)
    near = np.argsort(((old[:, :2] - at) ** 2).sum(axis=1))[:n_recent]
    yaw, t = 0.13, np.array([7.75, 0.53])
    c, s = np.cos(yaw), np.sin(yaw)
    d = old[near, :2] - t
    rec = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], old[near, 2]], axis=1) + 0.01 * rng.standard_normal((n_recent, 3))
    rec = rec.astype(np.float32).astype(np.float64)
    xyz = np.concatenate([old, rec])
    scans = [(0, 5)] * n_old + [(395, 400)] * n_recent
    st = capi.map_state(n, 16)
    st["landmarks"] = [dict(x=float(p[0]), y=float(p[1]), z=float(p[2]), rms_xy=np.float32(0.0), n_obs=2, first_scan=a, last_scan=b, segment=0, flags=0)
                       for p, (a, b) in zip(xyz, scans)]
    st["acc"] = np.concatenate([2.0 * xyz, xyz[:, :2], np.zeros((n, 3))], axis=1).tolist()
    st["header"] = dict(st["header"], n_landmarks=n, n_needed=n, n_obs=2 * n, scans=401, batches=1, segments=1)
    return capi.map_snapshot_pack(st), rec


def measure_find_loop(ctx, n, warmup, repeats):
    import torch
    blob, rec = find_loop_case(n, np.random.default_rng(n))
    mp = ctx.map_create(n, 16)
    mp.import_state(blob)
    K = len(rec)
    k0, n_blk = capi.keypoint_block_layout(1, K)
    sb = np.zeros((n_blk, 4), np.float32)
    u = sb.view(np.uint32).reshape(-1)
    u[:4] = (1, K, 0, K)
    u[4:6] = (0, K)
    sb[k0:k0 + K, :3] = rec
    skp = (torch.from_numpy(sb.view(np.uint8).reshape(-1)).cuda(), 1, K)
    res = torch.zeros((capi.FIND_DTYPE.itemsize // 8,), dtype=torch.float64, device="cuda")
    match = torch.empty((n,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    t = {"find_ms": [], "relocalize_ms": []}
    first = reloc = None
    for rep in range(warmup + repeats):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(stream)
        mp.find_loop(result=res, match=match)
        e[1].record(stream), e[2].record(stream)
        recs, _ = mp.relocalize(skp, 1)
        e[3].record(stream)
        ctx.synchronize()
        got, reloc = capi.find_loop_records(res), capi.relocalize_records(recs)[0]
        first = got if first is None else first
        assert got.tobytes() == first.tobytes(), (got, first)
        if rep >= warmup:
            for k, (a, b) in zip(t, ((0, 1), (2, 3))):
                t[k].append(e[a].elapsed_time(e[b]))
    mp.close()
    out = {"landmarks": n, "result": {k: (float(first[k]) if first[k].dtype.kind == "f" else int(first[k])) for k in capi.FIND_DTYPE.names},
           "relocalize": {k: int(reloc[k]) for k in ("n_hyp", "n_kp", "n_seeds", "score", "runner_up", "flags")}}
    for k, v in t.items():
        out[k] = statistics.median(v)
        out[k + "_min_max"] = [min(v), max(v)]
    return out


def main_find_loop(a):
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    rows = [measure_find_loop(ctx, n, a.warmup, a.repeats) for n in sizes]
    ctx.close()
    lines = [f"fx_map_find_loop next to fx_map_relocalize on synthetic maps (tools/map_times.py --find-loop): 1 pole per 160 m^2, one segment, 40",
             f"recent landmarks that are drifted twins of 40 old ones; find: default options (40 queries, 16 seeds); relocalize: one scan of the",
             f"same 40 points, any segment; one context, HIP events around each call, median of {a.repeats} after {a.warmup} warm-up; ms",
             f"{'landmarks':>10} {'targets':>8} {'n_hyp':>9} {'score':>6} {'runner':>7} {'flags':>6} {'find':>9} {'find / size before':>19} {'relocalize':>11} {'its n_hyp':>10} "
             f"{'find / relocalize':>18}"]
    for k, r in enumerate(rows):
        ratio = f"{r['find_ms'] / rows[k - 1]['find_ms']:.2f}" if k else "-"
        q = r["result"]
        lines.append(f"{r['landmarks']:>10} {q['n_targets']:>8} {q['n_hyp']:>9} {q['score']:>6} {q['runner_up']:>7} {q['flags']:>#6x} {r['find_ms']:>9.3f} {ratio:>19} "
                     f"{r['relocalize_ms']:>11.3f} {r['relocalize']['n_hyp']:>10} {r['find_ms'] / r['relocalize_ms']:>18.2f}")
    s = "\n".join(lines)
    print(s)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


def append_case(n, rng, r=16):
    """The snapshot of a one-segment map of n live landmarks of two observations with a carry scan of r rows, built as arrays (the
    layout is capi.map_snapshot_pack's)."""
    import struct
    xyz = np.concatenate([rng.uniform(0.0, (n * 250.0) ** 0.5, (n, 2)), rng.uniform(0.0, 2.0, (n, 1))], axis=1).astype(np.float32).astype(np.float64)
    rec = np.zeros(n, capi.MAP_LANDMARK_DTYPE)
    rec["x"], rec["y"], rec["z"], rec["n_obs"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 2
    rec["first_scan"] = np.arange(n) % 4
    rec["last_scan"] = rec["first_scan"] + 1
    acc = np.concatenate([2.0 * xyz, xyz[:, :2], np.zeros((n, 3))], axis=1)
    r = min(r, n)
    H = dict(n_landmarks=n, n_needed=n, n_obs=2 * n, scans=5, batches=1, segments=1, flags=0, carry_rows=r, last_joined=0, last_new=n)
    hdr = struct.pack("<10I", *(H[k] for k in capi.MAP_HEADER_FIELDS)) + struct.pack("<5d2I", 1.0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    body = [capi._pad16(hdr), rec.tobytes(), acc.astype("<f8").tobytes(), capi._pad16(np.full(n, -1, "<i4").tobytes()),
            capi._pad16(np.arange(n - r, n, dtype="<i4").tobytes()), rng.integers(0, 1 << 32, (r, 4), dtype=np.uint64).astype("<u4").tobytes()]
    total = capi.FX_MAP_SNAPSHOT_HEADER_BYTES + sum(len(b) for b in body)
    head = struct.pack("<10IQ", capi.FX_MAP_SNAPSHOT_MAGIC, capi.FX_MAP_SNAPSHOT_FORMAT, capi.FX_HEADER_VERSION, capi.FX_MAP_SNAPSHOT_HEADER_BYTES, n, r,
                       C.sizeof(capi.FxMapHeader), C.sizeof(capi.FxMapLandmark), capi.FX_MAP_ACC, 0, total)
    return head + b"\0" * (capi.FX_MAP_SNAPSHOT_HEADER_BYTES - len(head)) + b"".join(body)


def measure_append(ctx, n, warmup, repeats):
    import time
    import torch
    blob = append_case(n, np.random.default_rng(n))
    dst, src = ctx.map_create(2 * n, 16), ctx.map_create(n, 16)
    src.import_state(blob)
    res = torch.zeros((8,), dtype=torch.int32, device="cuda")
    plain = torch.empty((2, 116 * n), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    t = {"import_ms": [], "append_ms": [], "import2_ms": [], "append_host_ms": [], "copy_ms": []}
    wall, first = [], None
    for rep in range(warmup + repeats):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(10)]
        e[0].record(stream)
        dst.import_state(blob)
        e[1].record(stream), e[2].record(stream)
        dst.append(src, result=res)
        e[3].record(stream)
        ctx.synchronize()
        got = capi.append_records(res).copy()
        assert int(got["flags"]) == capi.FX_APPEND_APPLIED and int(got["appended"]) == n == int(got["id_base"]), got
        state = dst.export_state() if n <= 100000 else None
        e[4].record(stream)
        dst.import_state(blob)
        e[5].record(stream)
        ctx.synchronize()
        t0 = time.perf_counter()
        e[6].record(stream)
        dst.append_state(blob, result=res)
        e[7].record(stream)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        assert capi.append_records(res).tobytes() == got.tobytes()
        if state is not None:
            assert dst.export_state() == state, "fx_map_append_host and fx_map_append leave the same map"
        first = got if first is None else first
        with torch.cuda.stream(stream):
            e[8].record(stream)
            plain[1].copy_(plain[0], non_blocking=True)
            e[9].record(stream)
        ctx.synchronize()
        if rep >= warmup:
            for k, (a, b) in zip(t, ((0, 1), (2, 3), (4, 5), (6, 7), (8, 9))):
                t[k].append(e[a].elapsed_time(e[b]))
    dst.close(), src.close()
    out = {"landmarks": n, "snapshot_bytes": len(blob), "result": {k: int(first[k]) for k in ("id_base", "scan_base", "segment_base", "appended", "flags", "carry_rows")},
           "append_host_wall_ms": statistics.median(wall[warmup:])}
    for k, v in t.items():
        out[k] = statistics.median(v)
        out[k + "_min_max"] = [min(v), max(v)]
    return out


def main_append(a):
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    rows = [measure_append(ctx, n, a.warmup, a.repeats) for n in sizes]
    ctx.close()
    lines = ["# fx_map_append: device times", "",
             "tools/map_times.py --append: a map of M = N landmarks (all live, 16 carry rows) appended to a map of N; one context, one pair of",
             f"HIP events around each call, median of {a.repeats} after {a.warmup} warm-up; ms.  append: fx_map_append of the source map; append_host:",
             "fx_map_append_host of its snapshot (events: the copy of the staged block and the launches; wall: the call and the wait for it,",
             "the staging memcpy included); import: fx_map_import_host of the same snapshot; copy: one hipMemcpyAsync of 116 N bytes, device to device.",
             "", "```",
             f"{'landmarks':>10} {'append':>9} {'append / size before':>21} {'append_host':>12} {'its wall':>9} {'import':>9} {'copy':>9} {'append / copy':>14}"]
    for k, r in enumerate(rows):
        ratio = f"{r['append_ms'] / rows[k - 1]['append_ms']:.2f}" if k else "-"
        lines.append(f"{r['landmarks']:>10} {r['append_ms']:>9.4f} {ratio:>21} {r['append_host_ms']:>12.4f} {r['append_host_wall_ms']:>9.3f} {r['import_ms']:>9.4f} "
                     f"{r['copy_ms']:>9.4f} {r['append_ms'] / r['copy_ms']:>14.2f}")
    lines.append("```")
    by = {r["landmarks"]: r for r in rows}
    if 100000 in by and 1000000 in by:
        ratio = by[1000000]["append_ms"] / by[100000]["append_ms"]
        lines += ["", f"requirement: append(10^6) <= 15 x append(10^5): {ratio:.2f} x, {'met' if ratio <= 15.0 else 'NOT met'}"]
    s = "\n".join(lines)
    print(s)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


def splice_source(kp, csr, scan0, n_scans):
    """An fx_splice_source from (kp tensor, max_scans, max_total) and (CSR tensor, max_rows, capacity)."""
    return capi.FxSpliceSource(kp[0].data_ptr(), kp[1], kp[2], csr[0].data_ptr(), csr[1], csr[2], scan0, n_scans)


def measure_splice_one_scan(steps, warmup):
    """One new scan a call: `twice` against `once`, alternating, host to host."""
    import time
    import torch
    N = 28800
    ctx = capi.Context(capi.params("launch"), capi.limits(2, N, sparse=True))
    dev = torch.from_numpy(np.stack([capi.synth_scan(capi.synth_cfg(1000 + b)) for b in range(steps + 1)])).cuda()
    S, R = 2, ctx.limits.max_total_keypoints
    cap = R * 128
    nk, nc = int(ctx.lib.fx_keypoint_block_bytes(S, R)), int(ctx.lib.fx_descriptor_csr_bytes(R, cap))
    pair = lambda: ((torch.zeros(nk, dtype=torch.uint8, device="cuda"), S, R), (torch.zeros(nc, dtype=torch.uint8, device="cuda"), R, cap))
    twice, cur, ring = pair(), pair(), [pair(), pair()]
    P = C.c_void_p

    def process(first, n):
        descs = ctx.make_descs([dev.data_ptr() + (first + b) * N * 16 for b in range(n)], [N] * n, 16, 0.02, -0.015)
        ctx.process_raw(descs, n, capi.FX_IN_DEVICE | capi.FX_OUT_HOST)

    def packs(dst):
        ctx.pack_keypoint_block(dst[0][0].data_ptr(), S, R)
        ctx.pack_descriptors_csr(dst[1][0].data_ptr(), R, cap)
    process(0, 1), packs(ring[0])  # the block pair "before" of step 1: scan 0 alone
    ctx.synchronize()
    t_twice, t_once = [], []
    for k in range(1, steps + 1):
        prev, dst = ring[(k - 1) % 2], ring[k % 2]
        t0 = time.perf_counter()
        process(k - 1, 2), packs(twice)
        ctx.synchronize()
        t1 = time.perf_counter()
        process(k, 1), packs(cur)
        a, b = splice_source(*prev, capi.FX_SPLICE_LAST_SCAN, 1), splice_source(*cur, 0, 1)
        capi.check(ctx.lib.fx_splice_blocks(ctx.handle, C.byref(a), C.byref(b), P(dst[0][0].data_ptr()), S, R, P(dst[1][0].data_ptr()), R, cap))
        ctx.synchronize()
        t2 = time.perf_counter()
        if k > warmup:
            t_twice.append((t1 - t0) * 1e3), t_once.append((t2 - t1) * 1e3)
        assert torch.equal(twice[0][0], dst[0][0]), f"step {k}: the keypoint blocks of the two routes differ"
        g, w = capi.csr_parse(dst[1][0].cpu().numpy(), R, cap), capi.csr_parse(twice[1][0].cpu().numpy(), R, cap)
        assert all(np.array_equal(g[f].view(np.uint32) if f == "val" else g[f], w[f].view(np.uint32) if f == "val" else w[f]) for f in g), f"step {k}: the CSR blocks differ"
    ctx.close()
    return {"steps": len(t_twice), "twice_ms": statistics.median(t_twice), "once_ms": statistics.median(t_once),
            "twice_min_max": [min(t_twice), max(t_twice)], "once_min_max": [min(t_once), max(t_once)]}


def splice_blocks_synthetic(rng, scans, rows_a_scan=54, entries_a_row=40):
    """A block pair of `scans` scans as host arrays, built section by section (no dense rows): (kp bytes, max_scans, max_total), (CSR
    bytes, max_rows, capacity), the layouts exactly what the content needs."""
    n = scans * rows_a_scan
    nnz = n * entries_a_row
    lay = capi.keypoint_block_layout(scans, n)
    kp = np.zeros(4 * lay.n_rows, np.uint32)
    kp[:4] = (scans, n, 0, n)
    kp[4:lay.f0] = np.minimum(np.arange(lay.f0 - 4), scans) * rows_a_scan
    kp[4 * lay.k0:] = rng.integers(0, 1 << 32, 4 * n, dtype=np.uint64).astype(np.uint32)
    o_rp, o_col, o_val, end = capi.csr_layout(n, nnz)
    csr = np.zeros(end // 4, np.uint32)
    csr[:4] = (n, nnz, nnz, n)
    csr[4:4 + n + 1] = np.arange(n + 1) * entries_a_row
    csr[o_col // 4:o_col // 4 + nnz] = np.tile(np.sort(rng.choice(capi.FX_DESC_FLOATS, entries_a_row, replace=False)), n)
    csr[o_val // 4:o_val // 4 + nnz] = rng.integers(1, 1 << 32, nnz, dtype=np.uint64).astype(np.uint32)
    return (kp.view(np.uint8), scans, n), (csr.view(np.uint8), n, nnz)


def measure_splice_large(warmup, repeats, scans=1024):
    """(previous, last, 1) spliced with (current, 0, scans - 1) against one copy of the bytes the splice defines."""
    import torch
    rng = np.random.default_rng(scans)
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    up = lambda blk: (torch.from_numpy(blk[0]).cuda(), blk[1], blk[2])
    prev, cur = [tuple(up(b) for b in splice_blocks_synthetic(rng, s)) for s in (scans, scans - 1)]
    whole_h = splice_blocks_synthetic(rng, scans)
    (_, S, R), (_, _, cap) = whole_h
    dk = torch.zeros(len(whole_h[0][0]), dtype=torch.uint8, device="cuda")
    dc = torch.zeros(len(whole_h[1][0]), dtype=torch.uint8, device="cuda")
    a, b = splice_source(*prev, capi.FX_SPLICE_LAST_SCAN, 1), splice_source(*cur, 0, scans - 1)
    defined = len(whole_h[0][0]) + 16 + 4 * (R + 1) + 8 * cap
    plain = torch.empty((2, defined), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    P = C.c_void_p
    torch.cuda.synchronize()
    t_splice, t_copy = [], []
    for rep in range(warmup + repeats):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(stream)
        capi.check(ctx.lib.fx_splice_blocks(ctx.handle, C.byref(a), C.byref(b), P(dk.data_ptr()), S, R, P(dc.data_ptr()), R, cap))
        e[1].record(stream)
        with torch.cuda.stream(stream):
            e[2].record(stream)
            plain[1].copy_(plain[0], non_blocking=True)
            e[3].record(stream)
        ctx.synchronize()
        if rep >= warmup:
            t_splice.append(e[0].elapsed_time(e[1])), t_copy.append(e[2].elapsed_time(e[3]))
    # what was timed is the splice: against the reference's statement of it on the first and the last scans' sections
    hdr = dc[:16].view(torch.int32).cpu().tolist()
    assert hdr == [R, cap, cap, R] and dk[:16].view(torch.int32).cpu().tolist() == [S, R, 0, R], (hdr, S, R, cap)
    ctx.close()
    return {"scans": scans, "rows": R, "entries": cap, "bytes": defined, "splice_ms": statistics.median(t_splice), "copy_ms": statistics.median(t_copy),
            "splice_min_max": [min(t_splice), max(t_splice)], "copy_min_max": [min(t_copy), max(t_copy)]}


def main_splice(a):
    one = measure_splice_one_scan(a.steps, max(a.warmup, 4))
    big = measure_splice_large(a.warmup, a.repeats)
    lines = ["# fx_splice_blocks: times", "",
             "tools/map_times.py --splice, one run on one MI355X.", "",
             "## One new scan a call, host to host", "",
             f"VLP-16 scans resident on the device, a context of two scans (launch preset, fx_limits_sparse); the two routes alternate over {one['steps']}",
             "steps, time.perf_counter around the calls and the wait for the stream, medians (min .. max); ms.  twice: fx_process_batch of [the",
             "scan before, the new scan], fx_pack_keypoint_block, fx_pack_descriptors_csr.  once: fx_process_batch of the new scan, the two",
             "packs, fx_splice_blocks behind the last scan of the block pair before.  Both with FX_OUT_HOST; the two routes' blocks are equal at",
             "every step (asserted).", "", "```",
             f"{'route':>6} {'median':>8} {'min':>8} {'max':>8}",
             f"{'twice':>6} {one['twice_ms']:>8.4f} {one['twice_min_max'][0]:>8.4f} {one['twice_min_max'][1]:>8.4f}",
             f"{'once':>6} {one['once_ms']:>8.4f} {one['once_min_max'][0]:>8.4f} {one['once_min_max'][1]:>8.4f}",
             f"once / twice: {one['once_ms'] / one['twice_ms']:.3f}", "```", "",
             f"## 1 + {big['scans'] - 1} scans", "",
             f"Synthetic block pairs (54 rows a scan, 40 entries a row): (previous, last, 1) spliced with (current, 0, {big['scans'] - 1}) into {big['rows']} rows and",
             f"{big['entries']} entries; one pair of HIP events around the call, alternating with one hipMemcpyAsync, device to device, of the {big['bytes']} bytes the",
             f"splice defines; median of {a.repeats} after {a.warmup} warm-up (min .. max); ms.", "", "```",
             f"{'':>7} {'median':>8} {'min':>8} {'max':>8}",
             f"{'splice':>7} {big['splice_ms']:>8.4f} {big['splice_min_max'][0]:>8.4f} {big['splice_min_max'][1]:>8.4f}",
             f"{'copy':>7} {big['copy_ms']:>8.4f} {big['copy_min_max'][0]:>8.4f} {big['copy_min_max'][1]:>8.4f}",
             f"splice / copy: {big['splice_ms'] / big['copy_ms']:.2f}", "```"]
    s = "\n".join(lines)
    print(s)
    print(json.dumps({"one_scan": one, "large": big}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


def main_relocalize(a):
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    rows = [measure_relocalize(ctx, n, a.warmup, a.repeats) for n in sizes]
    ctx.close()
    lines = [f"fx_map_relocalize on synthetic maps (tools/map_times.py --relocalize): 1 pole per 250 m^2 (a third of them a second landmark up to",
             f"0.2 m off), 8 scans of 64 keypoints a call, default options (16 seeds); one context, HIP events around the call, median of",
             f"{a.repeats} after {a.warmup} warm-up; ms",
             f"{'landmarks':>10} {'scans':>6} {'call':>10} {'a scan':>10} {'valid':>6} {'n_hyp a scan':>14}"]
    for r in rows:
        lines.append(f"{r['landmarks']:>10} {r['scans']:>6} {r['call_ms']:>10.3f} {r['call_ms'] / r['scans']:>10.3f} {r['valid']:>6} {r['n_hyp_mean']:>14.0f}")
    s = "\n".join(lines)
    print(s)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


def main_compact(a):
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    rows = [measure_compact(ctx, n, a.warmup, a.repeats) for n in sizes]
    ctx.close()
    lines = [f"fx_map_compact on synthetic maps after one fx_map_merge (tools/map_times.py --compact): 1 pole per 250 m^2, a third of the",
             f"landmarks absorbed; one context, HIP events around each call, median of {a.repeats} after {a.warmup} warm-up; ms.  fixpoint: fx_map_merge on",
             f"the merged map (nothing left to merge: the grid build and the search), before and after the compaction",
             f"{'landmarks':>10} {'kept':>8} {'absorbed':>9} {'compact':>9} {'compact / size before':>21} {'fixpoint before':>16} {'fixpoint after':>15} {'after / before':>15}"]
    for k, r in enumerate(rows):
        ratio = f"{r['compact_ms'] / rows[k - 1]['compact_ms']:.2f}" if k else "-"
        lines.append(f"{r['landmarks']:>10} {r['result']['kept']:>8} {r['result']['dropped_absorbed']:>9} {r['compact_ms']:>9.3f} {ratio:>21} "
                     f"{r['fixpoint_before_ms']:>16.3f} {r['fixpoint_after_ms']:>15.3f} {r['fixpoint_after_ms'] / r['fixpoint_before_ms']:>15.2f}")
    by = {r["landmarks"]: r for r in rows}
    if 100000 in by and 1000000 in by:
        ratio = by[1000000]["compact_ms"] / by[100000]["compact_ms"]
        lines.append(f"requirement: compact(10^6) <= 15 x compact(10^5): {ratio:.2f} x, {'met' if ratio <= 15.0 else 'NOT met'}")
    s = "\n".join(lines)
    print(s)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


def main_merge(a):
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    rows = [measure_merge(ctx, n, a.warmup, a.repeats) for n in sizes]
    ctx.close()
    lines = [f"fx_map_merge next to fx_map_update on synthetic maps (tools/map_times.py --merge): 1 pole per 250 m^2, a third of the landmarks",
             f"the second fragment of a pole; one context, HIP events around each call, median of {a.repeats} after {a.warmup} warm-up; ms",
             f"{'landmarks':>10} {'merged':>8} {'live':>8} {'update':>9} {'merge':>9} {'fixpoint':>9} {'merge / size before':>19}"]
    for k, r in enumerate(rows):
        ratio = f"{r['merge_ms'] / rows[k - 1]['merge_ms']:.2f}" if k else "-"
        lines.append(f"{r['landmarks']:>10} {r['result']['merged']:>8} {r['result']['live']:>8} {r['update_ms']:>9.3f} {r['merge_ms']:>9.3f} {r['merge_fixpoint_ms']:>9.3f} {ratio:>19}")
    s = "\n".join(lines)
    print(s)
    print(json.dumps(rows))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", action="store_true", help="time fx_map_merge on synthetic maps instead")
    ap.add_argument("--compact", action="store_true", help="time fx_map_compact on the merged synthetic maps instead")
    ap.add_argument("--relocalize", action="store_true", help="time fx_map_relocalize on the synthetic maps instead (pass --sizes 10000,100000)")
    ap.add_argument("--join", action="store_true", help="time fx_map_join_segments on two-segment synthetic maps instead")
    ap.add_argument("--observe", action="store_true", help="time fx_map_observe behind fx_map_localize on the synthetic maps of --join instead")
    ap.add_argument("--expect", action="store_true", help="time fx_map_expect behind fx_map_localize and fx_map_retire next to fx_map_compact on the synthetic maps of --join instead")
    ap.add_argument("--discover", action="store_true", help="time fx_map_discover next to fx_map_observe behind fx_map_localize on the synthetic maps of --join instead")
    ap.add_argument("--loop", action="store_true", help="time fx_map_close_loop on the synthetic maps taken as one loop instead")
    ap.add_argument("--find-loop", action="store_true", help="time fx_map_find_loop next to fx_map_relocalize on one-segment synthetic maps instead")
    ap.add_argument("--append", action="store_true", help="time fx_map_append and fx_map_append_host next to fx_map_import_host and a plain copy instead")
    ap.add_argument("--splice", action="store_true", help="time fx_splice_blocks instead: one new scan a call against processing two, and 1 + 1023 scans against a plain copy")
    ap.add_argument("--follow", action="store_true", help="time fx_map_follow (one chain, chains of 16, one scan) next to fx_map_localize over a drive of --scans scans (pass --sizes 10000,1000000)")
    ap.add_argument("--steps", type=int, default=200, help="--splice: scans of the one-scan-a-call comparison")
    ap.add_argument("--sizes", default="1000,100000,1000000")
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: device times are measured on the GPU or not at all")
    if a.merge:
        return main_merge(a)
    if a.compact:
        return main_compact(a)
    if a.relocalize:
        return main_relocalize(a)
    if a.join:
        return main_join(a)
    if a.observe:
        return main_observe(a)
    if a.expect:
        return main_expect(a)
    if a.discover:
        return main_discover(a)
    if a.loop:
        return main_loop(a)
    if a.find_loop:
        return main_find_loop(a)
    if a.append:
        return main_append(a)
    if a.splice:
        return main_splice(a)
    if a.follow:
        return main_follow(a)
    N = 28800
    ctx = capi.Context(capi.params("launch"), capi.limits(a.batch, N, sparse=True))
    scenes = np.stack([capi.synth_scan(capi.synth_cfg(1000 + b)) for b in range(a.scans)])
    out = {"config": f"{a.scans} VLP-16 scans as batches of {a.batch} with one-scan overlap, launch preset, fx_limits_sparse, device-resident input, "
                     f"one context; in-batch pairs_consecutive, 12 shifts, mutual on; default register and track options; one pair of HIP events "
                     f"around each batch's fx_track_landmarks and fx_map_update, median over the batches of {a.repeats} runs after {a.warmup} warm-up",
           "scenes": measure(ctx, scenes, 0.02, -0.015, a.batch, a.warmup, a.repeats),
           "rotated": measure(ctx, rotated(scenes[0], a.scans), 0.0, 0.0, a.batch, a.warmup, a.repeats)}
    ctx.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
