"""Device time of registering a batch's consecutive scans (fx_register_matches), next to the batch and the match it follows.

  python tools/register_times.py [--batch 1024] [--warmup 5] [--repeats 30] [--out profiles/register.json] [--trace DIR]

One context, one batch of VLP-16 scans (seeds 1000 + b, launch preset, roll 0.02, pitch -0.015, fx_limits_sparse, the scans
resident on the device), the method of tools/match_times.py: HIP events on the context's stream, one pair of events a repeat,
the median of the repeats after the warm-up:
  batch_ms     fx_process_batch(FX_IN_DEVICE)
  match_ms     fx_match_descriptors_csr over pairs_consecutive (the block against itself, 12 shifts, mutual)
  register_ms  fx_register_matches alone, the same pairs
  chain_ms     fx_pack_keypoint_block + fx_pack_descriptors_csr + match + register
Also counts the work of the registration: samples formed and (sample, correspondence) agreement tests.  Writes one JSON object.
--trace DIR first runs this script again — a fresh child process, a run of its own — under `rocprofv3 --kernel-trace --stats`
with a short repeat count and adds the per-kernel averages of k_register / k_register_init to the JSON; each GPU step runs
under its own `timeout`, the steps chained with `&&`.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feature_extraction_amd import capi  # noqa: E402
from tools.match_times import kernel_trace, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out")
    ap.add_argument("--trace")
    a = ap.parse_args()
    trace = kernel_trace(__file__, a.trace, a.batch, "k_register", 240) if a.trace else None  # (the child runs before this process opens the GPU)
    import ctypes as C
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: device times are measured on the GPU or not at all")
    B, N = a.batch, 28800
    dev = torch.from_numpy(np.stack([capi.synth_scan(capi.synth_cfg(1000 + b)) for b in range(B)])).cuda()
    ctx = capi.Context(capi.params("launch"), capi.limits(B, N, sparse=True))
    descs = ctx.make_descs([dev.data_ptr() + b * N * 16 for b in range(B)], [N] * B, 16, 0.02, -0.015)
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
    _, hdr = ctx.descriptors_csr(buf, R, cap)
    assert hdr["rows_stored"] == hdr["rows"] == int(off[-1]), hdr

    # (the C calls with their arguments built once: the events must not span Python building 1023 pairs)
    arr = (capi.FxMatchPair * max(len(pairs), 1))(*[capi.FxMatchPair(*p) for p in pairs])
    mopt = capi.FxMatchOptions()
    ctx.lib.fx_match_options_default(C.byref(mopt))
    mopt.mutual = 1
    ropt = capi.FxRegisterOptions()
    ctx.lib.fx_register_options_default(C.byref(ropt))
    P = C.c_void_p

    def batch():
        ctx.process_raw(descs, B, capi.FX_IN_DEVICE)

    def match():
        capi.check(ctx.lib.fx_match_descriptors_csr(ctx.handle, P(buf.data_ptr()), R, cap, P(buf.data_ptr()), R, cap, arr, len(pairs), C.byref(mopt),
                                                    P(match_t.data_ptr())))

    def register():
        capi.check(ctx.lib.fx_register_matches(ctx.handle, P(kp.data_ptr()), B, R, P(kp.data_ptr()), B, R, P(match_t.data_ptr()), R, arr, len(pairs),
                                               C.byref(ropt), P(reg_t.data_ptr()), P(inl_t.data_ptr())))

    def chain():
        ctx.pack_keypoint_block(kp.data_ptr(), B, R)
        ctx.pack_descriptors_csr(buf.data_ptr(), R, cap)
        match()
        register()

    chain()
    ctx.synchronize()
    res = {}
    for name, fn in (("batch_ms", batch), ("chain_ms", chain), ("match_ms", match), ("register_ms", register), ("batch_ms_again", batch)):
        ms = timed(stream, fn, a.warmup, a.repeats)
        res[name] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "repeats": len(ms)}
    rec = capi.register_records(reg_t)[:len(pairs)]
    H = np.minimum(rec["n_corr"], ropt.hyp_corr).astype(np.int64)
    samples = H * (H - 1) // 2
    batch_ms = statistics.median([res["batch_ms"]["median"], res["batch_ms_again"]["median"]])
    yaw = np.degrees(capi.register_yaw(rec))
    out = {"config": f"{B} VLP-16 scans, launch preset, fx_limits_sparse, device-resident input, one context; in-batch pairs_consecutive, "
                     f"12 shifts, mutual on; default fx_register_options; HIP events, median of {a.repeats} after {a.warmup} warm-up",
           "rows": int(off[-1]), "pairs": len(pairs), "correspondences": int(rec["n_corr"].sum()), "inlier_rows": int(rec["n_inliers"].sum()),
           "valid_pairs": int(((rec["flags"] & capi.FX_REG_VALID) != 0).sum()),
           "no_hypothesis_pairs": int(((rec["flags"] & capi.FX_REG_NO_HYPOTHESIS) != 0).sum()),
           "samples": int(samples.sum()), "agreement_tests_upper_bound": int((samples * rec["n_corr"]).sum()),
           "median_abs_yaw_deg": float(np.median(np.abs(yaw))) if len(yaw) else 0.0,
           "timings": res, "batch_ms": batch_ms, "match_ms": res["match_ms"]["median"], "register_ms": res["register_ms"]["median"],
           "chain_ms": res["chain_ms"]["median"], "register_over_match": res["register_ms"]["median"] / res["match_ms"]["median"],
           "chain_over_batch": res["chain_ms"]["median"] / batch_ms}
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
