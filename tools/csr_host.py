"""Host-to-host rate and streaming latency with the descriptor rows as dense rows (FX_OUT_HOST) against compressed rows
(FX_OUT_HOST | FX_OUT_DESC_CSR), alternating the two in the same process.

  python tools/csr_host.py [--batch 1024] [--steps 4] [--rounds 3] [--contexts 1,4] [--calls 200] [--out FILE]
  python tools/csr_host.py --profile [--batch 1024]     (one batch, then 20 fx_pack_descriptors_csr calls: for a kernel trace)

Headline configuration: VLP-16 scans (seeds 1000 + b), launch preset, roll 0.02, pitch -0.015, fx_limits_sparse, scans in
pinned host memory.  The throughput part follows bench.py's host_to_host: one host thread per context, each context on its
own stream, every thread issuing `steps` batches.  The latency part is one scan per fx_process_batch call on a warm context,
blocks of `calls` calls of each kind in turn.  Prints one JSON object.
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feature_extraction_amd import capi  # noqa: E402

MODES = {"dense": capi.FX_OUT_HOST, "csr": capi.FX_OUT_HOST | capi.FX_OUT_DESC_CSR}


def host_rate(ctxs, descs, B, flags, steps):
    err = []

    def worker(c):
        try:
            for _ in range(steps):
                c.process_raw(descs, B, flags)
        except Exception as e:  # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=worker, args=(c,)) for c in ctxs]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    if err:
        raise err[0]
    return B * steps * len(ctxs) / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--contexts", default="1,4")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    B, N = a.batch, 28800
    p = capi.params("launch")
    host = np.stack([capi.synth_scan(capi.synth_cfg(1000 + b)) for b in range(B)])
    pinned = torch.from_numpy(host).pin_memory()
    base = pinned.data_ptr()
    out = {"config": f"{B} VLP-16 scans a batch, launch preset, fx_limits_sparse, pinned host input"}

    if a.profile:
        ctx = capi.Context(p, capi.limits(B, N, sparse=True))
        descs = ctx.make_descs([base + b * N * 16 for b in range(B)], [N] * B, 16, 0.02, -0.015)
        ctx.process_raw(descs, B, MODES["csr"])
        R = ctx.limits.max_total_keypoints
        cap = R * 128
        buf = torch.zeros(int(ctx.lib.fx_descriptor_csr_bytes(R, cap)), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(20):
            ctx.pack_descriptors_csr(buf.data_ptr(), R, cap)
        ctx.synchronize()
        hdr = buf[:16].view(torch.int32).cpu().tolist()
        out["profile_header"] = {"rows": hdr[0], "nnz_stored": hdr[1], "nnz_needed": hdr[2], "rows_stored": hdr[3]}
        ctx.close()
        print(json.dumps(out))
        return

    # ---- what crosses the link for one headline batch
    ctx = capi.Context(p, capi.limits(B, N, sparse=True))
    descs = ctx.make_descs([base + b * N * 16 for b in range(B)], [N] * B, 16, 0.02, -0.015)
    v = ctx.process_raw(descs, B, MODES["csr"])
    rp, col, val = ctx.descriptors_csr_host()
    rows, nnz = len(rp) - 1, len(col)
    dense_b, csr_b = rows * capi.FX_DESC_FLOATS * 4, 4 * (rows + 1) + 8 * nnz
    out["descriptor_bytes"] = {"rows": rows, "nnz": nnz, "nnz_per_row": nnz / max(rows, 1), "dense_bytes": dense_b, "csr_bytes": csr_b,
                               "ratio": dense_b / max(csr_b, 1), "input_bytes": B * N * 16}
    ctx.close()

    # ---- host-to-host throughput, the two kinds alternating
    out["host_to_host_scans_per_s"] = {}
    for n_ctx in (int(x) for x in a.contexts.split(",")):
        ctxs = [capi.Context(p, capi.limits(B, N, sparse=True)) for _ in range(n_ctx)]
        for c in ctxs:
            c.set_batches_in_flight(n_ctx)
            for f in MODES.values():  # (first calls allocate the pinned mirrors and the CSR block)
                c.process_raw(descs, B, f)
        res = {m: [] for m in MODES}
        for r in range(a.rounds):
            for m in (MODES if r % 2 == 0 else reversed(list(MODES))):
                res[m].append(host_rate(ctxs, descs, B, MODES[m], a.steps))
        out["host_to_host_scans_per_s"][f"{n_ctx}_contexts"] = {m: {"median": statistics.median(x), "runs": x} for m, x in res.items()}
        for c in ctxs:
            c.close()

    # ---- one scan per call (streaming mode), the two kinds in alternating blocks
    ctx = capi.Context(p, capi.limits(1, N))
    one = [ctx.make_descs([base + b * N * 16], [N], 16, 0.02, -0.015) for b in range(16)]
    lat = {m: [] for m in MODES}
    for f in MODES.values():
        for w in range(20):
            ctx.process_raw(one[w % 16], 1, f)
    for r in range(2 * a.rounds):
        m = list(MODES)[r % 2]
        for i in range(a.calls):
            t0 = time.perf_counter()
            ctx.process_raw(one[i % 16], 1, MODES[m])
            lat[m].append((time.perf_counter() - t0) * 1e3)
    out["one_scan_per_call_ms"] = {m: {"p50": float(np.percentile(x, 50)), "p90": float(np.percentile(x, 90)), "p99": float(np.percentile(x, 99)),
                                       "calls": len(x)} for m, x in lat.items()}
    ctx.close()
    s = json.dumps(out)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
