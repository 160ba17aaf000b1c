"""Device time of matching a batch's scans against each other, next to the batch itself.

  python tools/match_times.py [--batch 1024] [--warmup 5] [--repeats 30] [--out profiles/match.json]

One context, one batch of VLP-16 scans (seeds 1000 + b, launch preset, roll 0.02, pitch -0.015, fx_limits_sparse, the scans
resident on the device).  Timed with HIP events on the context's stream, one pair of events a repeat, the median of the
repeats after the warm-up:
  batch_ms       fx_process_batch(FX_IN_DEVICE)
  pack_match_ms  fx_pack_descriptors_csr into a caller's block + fx_match_descriptors_csr over pairs_consecutive (scan b + 1's
                 rows against scan b's, the block against itself, all 12 shifts)
  match_ms       fx_match_descriptors_csr alone, the same pairs
and their ratio.  Also counts the work the match does: (query row, train row) comparisons and the train entries they walk,
each entry being 12 LDS reads and 12 fp64 multiply-adds.  Writes one JSON object.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feature_extraction_amd import capi  # noqa: E402


def timed(stream, fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def kernel_trace(script, trace_dir, batch, prefix, limit_s):
    """{kernel: {calls, avg_us, min_us, max_us}} of the kernels whose names begin with `prefix`, from a rocprofv3 run of `script`
    (one of the *_times.py tools, with a short repeat count) in a fresh child process under its own time limit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = (f"timeout -k 10 {limit_s} rocprofv3 --kernel-trace --stats -d {trace_dir} -o trace --output-format csv -- "
           f"{sys.executable} {os.path.abspath(script)} --batch {batch} --warmup 2 --repeats 5 > {trace_dir}/child.log 2>&1")
    os.makedirs(trace_dir, exist_ok=True)
    subprocess.check_call(["bash", "-c", cmd], cwd=root)
    out = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if row["Name"].startswith(prefix):
                out[row["Name"].split("(")[0]] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                                                 "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--mutual", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
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
    out_t = torch.empty((R, 8), dtype=torch.int32, device="cuda")
    t_csr, hdr = ctx.descriptors_csr(buf, R, cap)
    assert hdr["rows_stored"] == hdr["rows"] == int(off[-1]), hdr
    rp = t_csr.crow_indices().cpu().numpy().astype(np.int64)

    def batch():
        ctx.process_raw(descs, B, capi.FX_IN_DEVICE)

    # (the C call itself with its arguments built once: the events must not span Python building 1023 pairs)
    import ctypes as C
    arr = (capi.FxMatchPair * len(pairs))(*[capi.FxMatchPair(*p) for p in pairs])
    opt = capi.FxMatchOptions()
    ctx.lib.fx_match_options_default(C.byref(opt))
    opt.mutual = int(a.mutual)

    def match():
        capi.check(ctx.lib.fx_match_descriptors_csr(ctx.handle, C.c_void_p(buf.data_ptr()), R, cap, C.c_void_p(buf.data_ptr()), R, cap, arr,
                                                    len(pairs), C.byref(opt), C.c_void_p(out_t.data_ptr())))

    def pack_match():
        ctx.pack_descriptors_csr(buf.data_ptr(), R, cap)
        match()

    res = {}
    for name, fn in (("batch_ms", batch), ("pack_match_ms", pack_match), ("match_ms", match), ("batch_ms_again", batch)):
        ms = timed(stream, fn, a.warmup, a.repeats)
        res[name] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "repeats": len(ms)}
    rec = capi.match_records(out_t)[:int(off[-1])]
    # the work: every query row of a pair meets every train row of it, walking that train row's entries
    comparisons = sum(qn * tn for _, qn, _, tn in pairs)
    entries = sum(qn * int(rp[t0 + tn] - rp[t0]) for _, qn, t0, tn in pairs)
    batch_ms = statistics.median([res["batch_ms"]["median"], res["batch_ms_again"]["median"]])
    out = {"config": f"{B} VLP-16 scans, launch preset, fx_limits_sparse, device-resident input, one context; in-batch "
                     f"pairs_consecutive, 12 shifts, mutual {'on' if a.mutual else 'off'}; HIP events, median of {a.repeats} after {a.warmup} warm-up",
           "rows": int(off[-1]), "nnz": int(rp[-1]), "pairs": len(pairs), "row_comparisons": comparisons, "train_entries_walked": entries,
           "lds_reads": 12 * entries, "fp64_fma": 12 * entries,
           "matched_rows": int((rec["train_row"] >= 0).sum()), "timings": res,
           "batch_ms": batch_ms, "pack_match_ms": res["pack_match_ms"]["median"], "match_ms": res["match_ms"]["median"],
           "pack_match_over_batch": res["pack_match_ms"]["median"] / batch_ms,
           "match_lds_reads_per_s": 12 * entries / (res["match_ms"]["median"] * 1e-3)}
    ctx.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
