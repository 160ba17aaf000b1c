"""The launch policy (csrc/fx_launch_plan.h: which kernels a batch runs, with what grids and in how many slices) on a CPU:
csrc/fx_plan_selftest.cpp pins grids, slice counts, the front and gather kinds, the hint hold, the dense tier's linger, the
front's pause and the capture rule at values worked out by hand.  The policy decides speed only, never a result, so the
parity tests on the device cannot see a wrong grid; this one can."""
import subprocess

from feature_extraction_amd import build


def test_launch_plan_selftest():
    exe = build.build_plan_selftest()
    pr = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 0, pr.stdout + pr.stderr
    assert " 0 failed" in pr.stdout, pr.stdout
