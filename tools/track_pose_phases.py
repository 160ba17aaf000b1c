"""Where k_track_poses (csrc/fx_track.hip) spends its time: fx_track_landmarks timed with the product library and with four
measurement builds that leave one part of the pose kernel out (wrong poses, the time of what remains):

  timeout -k 10 600 python tools/track_pose_phases.py [--scans 1024] [--rows 54] [--warmup 5] [--repeats 30] [--out profiles/track_pose_phases.json]

  product      the library as shipped
  no_cs_fold   -DFXT_SKIP_CS_FOLD: without the one-lane (c, s) fold
  no_t_fold    -DFXT_SKIP_T_FOLD: without the three one-lane folds of tx, ty, tz and the segment count
  no_folds     both left out: the loads, the rotated translations, the barriers and the write-out remain
  no_poses     -DFXT_SKIP_POSES: k_track_poses is not launched at all
Input: --scans scans of --rows random keypoints, every row of a scan >= 1 an inlier claiming a random row of the scan before with
probability 0.7, every link valid (no batch is processed).  HIP events on the context's stream around the one call, the median of
the repeats after the warm-up; every variant in a fresh child process under its own `timeout` (a process loads one library).
--build only compiles the variants (they are built where there is a compiler, not on GPU time).
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feature_extraction_amd import build, capi  # noqa: E402

VARIANTS = {"product": None, "no_cs_fold": ["-DFXT_SKIP_CS_FOLD"], "no_t_fold": ["-DFXT_SKIP_T_FOLD"],
            "no_folds": ["-DFXT_SKIP_CS_FOLD", "-DFXT_SKIP_T_FOLD"], "no_poses": ["-DFXT_SKIP_POSES"]}


def lib_of(name):
    return build.LIB if VARIANTS[name] is None else build.build_variant("track_" + name, VARIANTS[name])


def child(name, S, K, warmup, repeats):
    import ctypes as C
    import torch
    from tools.match_times import timed
    capi.LIB_PATH = lib_of(name)
    rng = np.random.default_rng(5)
    N = S * K
    k0, n_rows = capi.keypoint_block_layout(S, N)
    blk = np.zeros((n_rows, 4), np.float32)
    u = blk.view(np.uint32).reshape(-1)
    u[:4] = (S, N, 0, N)
    u[4:4 + S + 1] = np.arange(S + 1) * K
    blk[k0:, :3] = rng.uniform(-40, 40, (N, 3))
    m = np.zeros(N, capi.MATCH_DTYPE)
    scan = np.arange(N) // K
    pick = (rng.random(N) < 0.7) & (scan >= 1)
    m["train_row"] = np.where(pick, (scan - 1) * K + rng.integers(0, K, N), -1)
    m["pair"] = np.where(scan >= 1, scan - 1, capi.FX_MATCH_NO_PAIR).astype(np.uint32)
    reg = np.zeros(S, capi.REG_DTYPE)
    yaw = rng.uniform(-0.1, 0.1, S)
    reg["c"], reg["s"], reg["tx"], reg["ty"], reg["tz"] = np.cos(yaw), np.sin(yaw), rng.uniform(-2, 2, S), rng.uniform(-2, 2, S), rng.uniform(-0.1, 0.1, S)
    reg["flags"] = capi.FX_REG_VALID
    ctx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    d = [torch.from_numpy(a).cuda() for a in (blk.view(np.uint8).reshape(-1), m.view(np.int32).reshape(-1, 8).copy(), pick.astype(np.int32),
                                               reg.view(np.float64).reshape(-1, 8).copy())]
    outs = (torch.empty((S, 6), dtype=torch.float64, device="cuda"), torch.empty((N,), dtype=torch.int32, device="cuda"),
            torch.empty((N,), dtype=torch.int32, device="cuda"), torch.empty((N, 6), dtype=torch.float64, device="cuda"),
            torch.empty((8,), dtype=torch.int32, device="cuda"))
    opt = capi.FxTrackOptions()
    ctx.lib.fx_track_options_default(C.byref(opt))
    P = C.c_void_p

    def track():
        capi.check(ctx.lib.fx_track_landmarks(ctx.handle, P(d[0].data_ptr()), S, N, P(d[1].data_ptr()), P(d[2].data_ptr()), N, P(d[3].data_ptr()), S, None,
                                              C.byref(opt), P(outs[0].data_ptr()), P(outs[1].data_ptr()), P(outs[2].data_ptr()), P(outs[3].data_ptr()), N,
                                              P(outs[4].data_ptr())))
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    torch.cuda.synchronize()
    ms = timed(stream, track, warmup, repeats)
    hdr = capi.track_records(*outs)["header"]
    ctx.close()
    print("RESULT " + json.dumps({"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "header": hdr}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=54)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out")
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.scans, a.rows, a.warmup, a.repeats)
    for name in VARIANTS:
        lib_of(name)
    if a.build:
        return
    res = {}
    for name in VARIANTS:  # (a step that fails ends the run: nothing more is started on the GPU)
        out = subprocess.check_output(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child", name, "--scans", str(a.scans),
                                       "--rows", str(a.rows), "--warmup", str(a.warmup), "--repeats", str(a.repeats)], cwd=ROOT, text=True)
        res[name] = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
    t = {k: v["median_ms"] * 1e3 for k, v in res.items()}
    out = {"config": f"{a.scans} scans of {a.rows} rows, every link valid, one context; fx_track_landmarks alone, HIP events, median of {a.repeats} "
                     f"after {a.warmup} warm-up, a process a variant",
           "variants": res,
           "us": {"track": t["product"], "k_track_poses_in_the_call": t["product"] - t["no_poses"], "cs_fold": t["product"] - t["no_cs_fold"],
                  "t_folds": t["product"] - t["no_t_fold"], "both_folds": t["product"] - t["no_folds"],
                  "rest_of_k_track_poses": t["no_folds"] - t["no_poses"], "other_launches": t["no_poses"]}}
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
