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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: device times are measured on the GPU or not at all")
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
