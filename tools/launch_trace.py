"""Diagnostic: six batches of one size through a context of the TEST build (its environment hooks: FX_FRONT, FX_FRONT_SPLIT,
...), each with FX_OUT_HOST so that a batch's tier hints have landed before the next batch is planned.  Run it under
`rocprofv3 --kernel-trace` (alone: no counters, no other tracing) to list a shape's launches — kernel, grid, workgroup, LDS —
in order; two builds launch alike iff their listings are equal (profiles/launch_plan.md).
  python tools/launch_trace.py [batch=1] [preset=launch|rings32]
FX_LIB: another build's file name under feature_extraction_amd/lib (A/B runs)."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feature_extraction_amd import capi

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1
preset = sys.argv[2] if len(sys.argv) > 2 else "launch"
capi.LIB_PATH = os.path.join(os.path.dirname(capi.LIB_PATH), os.environ.get("FX_LIB", os.path.basename(capi.TEST_LIB_PATH)))
capi.load()
if preset == "rings32":  # more than 16 rings: the second run tier; more than 24: the many-rings ring split
    sensor = dict(n_rings=32, el0_deg=-15.0, el_step_deg=1.0)
    p = capi.params("launch", secondary_max=32, **sensor)
else:
    sensor = {}
    p = capi.params(preset)
scans = [capi.synth_scan(capi.synth_cfg(1000 + b, **sensor)) for b in range(min(B, 16))]
ctx = capi.Context(p, capi.limits(B, max(len(s) for s in scans)))
part = [scans[b % len(scans)] for b in range(B)]
descs = ctx.make_descs([s.ctypes.data for s in part], [len(s) for s in part], 16, 0.02, -0.015)
ctx.lib.fx_debug_front.argtypes = [ctypes.c_void_p]
for i in range(6):
    v = ctx.process_raw(descs, B, capi.FX_OUT_HOST)
    print(f"batch {i}: {B} scans, {int(v.total_keypoints)} keypoints, front {ctx.lib.fx_debug_front(ctx.handle)}")
