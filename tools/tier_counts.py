"""Diagnostic: how many rings / scans / keypoint rows each larger tier received in one batch."""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from feature_extraction_amd import capi
if len(sys.argv) > 3:  # an alternative build under feature_extraction_amd/lib
    capi.LIB_PATH = os.path.join(os.path.dirname(capi.LIB_PATH), sys.argv[3])
lib = capi.load()
preset = sys.argv[1] if len(sys.argv) > 1 else "launch"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 256
scans = [capi.synth_scan(capi.synth_cfg(1000 + b)) for b in range(B)]
ctx = capi.Context(capi.params(preset), capi.limits(B, 28800))
descs = ctx.make_descs([s.ctypes.data for s in scans], [len(s) for s in scans], 16, 0.02, -0.015)
v = ctx.process_raw(descs, B, capi.FX_OUT_HOST)
out = (C.c_uint32 * 16)()
lib.fx_debug_counters.argtypes = [C.c_void_p, C.c_void_p]
capi.check(lib.fx_debug_counters(ctx.handle, out))
names = ["rings -> second run tier", "scans -> big merge", "-", "-", "rows -> list tier",
         "rings -> workgroup tier", "rows -> dense tier", "-", "rows -> wavefront tier", "scans -> huge merge", "-", "-",
         "key-pool entries", "sorted-pool entries", "density work items", "-"]
print(f"batch {B} scans, {v.total_keypoints} keypoint rows, {B * 16} rings")
for n, c in zip(names, out):
    print(f"  {n:28s} {c}")
if hasattr(lib, "fx_debug_group_classes"):  # (an older build under lib/ has no size classes)
    cls = (C.c_uint32 * 3)()
    lib.fx_debug_group_classes.argtypes = [C.c_void_p, C.c_void_p]
    capi.check(lib.fx_debug_group_classes(ctx.handle, cls))
    for cap, c in zip((16, 32, 64), cls):
        print(f"  {'group rows, <= %d support points' % cap:28s} {c}  ({100.0 * c / max(1, v.total_keypoints):.1f} % of the rows)")
hints = (C.c_uint32 * 8)()
lib.fx_debug_tier_hints.argtypes = [C.c_void_p, C.c_void_p]
capi.check(lib.fx_debug_tier_hints(ctx.handle, hints))
print("tier hints (second run tier, workgroup ring tier [largest XCD class], big merges, huge merges, dense rows, dense points):", list(hints)[:6])
