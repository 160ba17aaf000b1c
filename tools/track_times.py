"""Device time of chaining a batch's motions and inliers into poses and landmark tracks (fx_track_landmarks), next to the
batch, the match and the register it follows.

  timeout -k 10 600 python tools/track_times.py [--batch 1024] [--warmup 5] [--repeats 30] [--out profiles/track.json] [--trace DIR]

One context, the method of tools/register_times.py (HIP events on the context's stream, one pair of events a repeat, the median
of the repeats after the warm-up), two workloads of --batch VLP-16 scans in the same process (launch preset, fx_limits_sparse,
the scans resident on the device):
  scenes   seeds 1000 + b, roll 0.02, pitch -0.015: independent scenes, so links are mostly bad or carry few inliers and tracks
           are short (the workload of profiles/register.json)
  rotated  scan seed 1000 and its copies, each 3 degrees further about z than the last, no levelling: every link is good and a
           pole is followed through the whole batch
Per workload: batch_ms, match_ms, register_ms, track_ms (fx_track_landmarks alone) and chain_ms (pack block + pack CSR + match +
register + track), and what the track found.  Writes one JSON object.
--trace DIR first runs this script again — a fresh child process, a run of its own — under `rocprofv3 --kernel-trace --stats`
with a short repeat count and adds the per-kernel averages of the k_track_* kernels (both workloads together) to the JSON; each
GPU step runs under its own `timeout`, the steps chained with `&&`.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feature_extraction_amd import capi  # noqa: E402
from tools.match_times import kernel_trace, timed  # noqa: E402


def rotated(scan, n, step_deg=3.0):
    x, y = scan[:, 0].astype(np.float64), scan[:, 1].astype(np.float64)
    out = np.repeat(scan[None], n, axis=0)
    for k in range(n):
        th = math.radians(step_deg * k)
        out[k, :, 0], out[k, :, 1] = math.cos(th) * x - math.sin(th) * y, math.sin(th) * x + math.cos(th) * y
    return out


def measure(ctx, scans, roll, pitch, warmup, repeats):
    import ctypes as C
    import torch
    B, N = scans.shape[0], scans.shape[1]
    dev = torch.from_numpy(scans).cuda()
    descs = ctx.make_descs([dev.data_ptr() + b * N * 16 for b in range(B)], [N] * B, 16, roll, pitch)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    v = ctx.process_raw(descs, B, capi.FX_IN_DEVICE | capi.FX_OUT_HOST)
    off = capi._np(v.h_kp_offset, (B + 1,), np.uint32).astype(np.int64)
    pairs = capi.pairs_consecutive(off)
    R, cap = ctx.limits.max_total_keypoints, ctx.limits.max_total_keypoints * 128
    buf = torch.empty(int(ctx.lib.fx_descriptor_csr_bytes(R, cap)), dtype=torch.uint8, device="cuda")
    kp = torch.empty(int(ctx.lib.fx_keypoint_block_bytes(B, R)), dtype=torch.uint8, device="cuda")
    match_t = torch.empty((R, 8), dtype=torch.int32, device="cuda")
    reg_t = torch.empty((max(len(pairs), 1), 8), dtype=torch.float64, device="cuda")
    inl_t = torch.empty((R,), dtype=torch.int32, device="cuda")
    outs = (torch.empty((B, 6), dtype=torch.float64, device="cuda"), torch.empty((R,), dtype=torch.int32, device="cuda"),
            torch.empty((R,), dtype=torch.int32, device="cuda"), torch.empty((R, 6), dtype=torch.float64, device="cuda"),
            torch.empty((8,), dtype=torch.int32, device="cuda"))
    _, hdr = ctx.descriptors_csr(buf, R, cap)
    assert hdr["rows_stored"] == hdr["rows"] == int(off[-1]), hdr

    # (the C calls with their arguments built once: the events must not span Python building 1023 pairs)
    arr = (capi.FxMatchPair * max(len(pairs), 1))(*[capi.FxMatchPair(*p) for p in pairs])
    mopt = capi.FxMatchOptions()
    ctx.lib.fx_match_options_default(C.byref(mopt))
    mopt.mutual = 1
    ropt = capi.FxRegisterOptions()
    ctx.lib.fx_register_options_default(C.byref(ropt))
    topt = capi.FxTrackOptions()
    ctx.lib.fx_track_options_default(C.byref(topt))
    P = C.c_void_p

    def batch():
        ctx.process_raw(descs, B, capi.FX_IN_DEVICE)

    def match():
        capi.check(ctx.lib.fx_match_descriptors_csr(ctx.handle, P(buf.data_ptr()), R, cap, P(buf.data_ptr()), R, cap, arr, len(pairs), C.byref(mopt),
                                                    P(match_t.data_ptr())))

    def register():
        capi.check(ctx.lib.fx_register_matches(ctx.handle, P(kp.data_ptr()), B, R, P(kp.data_ptr()), B, R, P(match_t.data_ptr()), R, arr, len(pairs),
                                               C.byref(ropt), P(reg_t.data_ptr()), P(inl_t.data_ptr())))

    def track():
        capi.check(ctx.lib.fx_track_landmarks(ctx.handle, P(kp.data_ptr()), B, R, P(match_t.data_ptr()), P(inl_t.data_ptr()), R, P(reg_t.data_ptr()), B,
                                              None, C.byref(topt), P(outs[0].data_ptr()), P(outs[1].data_ptr()), P(outs[2].data_ptr()),
                                              P(outs[3].data_ptr()), R, P(outs[4].data_ptr())))

    def chain():
        ctx.pack_keypoint_block(kp.data_ptr(), B, R)
        ctx.pack_descriptors_csr(buf.data_ptr(), R, cap)
        match()
        register()
        track()

    chain()
    ctx.synchronize()
    res = {}
    for name, fn in (("batch_ms", batch), ("chain_ms", chain), ("match_ms", match), ("register_ms", register), ("track_ms", track)):
        ms = timed(stream, fn, warmup, repeats)
        res[name] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "repeats": len(ms)}
    tr = capi.track_records(*outs)
    rec = capi.register_records(reg_t)[:len(pairs)]
    n = tr["landmarks"]["n_obs"]
    out = {"rows": int(off[-1]), "links": len(pairs), "valid_links": int(((rec["flags"] & capi.FX_REG_VALID) != 0).sum()),
           "inlier_rows": int(rec["n_inliers"].sum()), "header": tr["header"], "longest_track": int(n.max()) if len(n) else 0,
           "mean_track": float(n.mean()) if len(n) else 0.0, "segments": int(tr["poses"]["segment"][-1]) + 1,
           "worst_rms_xy": float(tr["landmarks"]["rms_xy"].max()) if len(n) else 0.0, "timings": res}
    for k in ("batch_ms", "match_ms", "register_ms", "track_ms", "chain_ms"):
        out[k] = res[k]["median"]
    out["track_over_register"] = out["track_ms"] / out["register_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out")
    ap.add_argument("--trace")
    a = ap.parse_args()
    trace = kernel_trace(__file__, a.trace, a.batch, "k_track", 300) if a.trace else None  # (the child runs before this process opens the GPU)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: device times are measured on the GPU or not at all")
    B, N = a.batch, 28800
    ctx = capi.Context(capi.params("launch"), capi.limits(B, N, sparse=True))
    scenes = np.stack([capi.synth_scan(capi.synth_cfg(1000 + b)) for b in range(B)])
    out = {"config": f"{B} VLP-16 scans, launch preset, fx_limits_sparse, device-resident input, one context; in-batch pairs_consecutive, "
                     f"12 shifts, mutual on; default register and track options; HIP events, median of {a.repeats} after {a.warmup} warm-up",
           "scenes": measure(ctx, scenes, 0.02, -0.015, a.warmup, a.repeats),
           "rotated": measure(ctx, rotated(scenes[0], B), 0.0, 0.0, a.warmup, a.repeats)}
    if trace is not None:
        out["kernel_trace"] = trace
    ctx.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
