"""capi.map_loop_reference and capi.loop_correct_poses_reference, the executable statements of fx_map_close_loop and
fx_map_loop_correct_poses (include/fx.h), on the CPU: the declarations, what the call is for (a drifted loop brought together so
that the merge can fuse the twins), the weights at their edges, the modes, the refusals and the poses."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_join_util as ju
from tests import map_loop_util as lu
from tests import map_merge_util as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, T_, NH, BP, BS, F, TF = (capi.FX_LOOP_APPLIED, capi.FX_LOOP_TRUNCATED, capi.FX_LOOP_NO_HYPOTHESIS, capi.FX_LOOP_BAD_PRIOR,
                            capi.FX_LOOP_BAD_SEGMENT, capi.FX_LOOP_FITTED, capi.FX_LOOP_TOO_FAR)
GIVEN, DRY = capi.FX_LOOP_GIVEN, capi.FX_LOOP_DRY_RUN
pack = capi.map_snapshot_pack


# ---- 1. declarations
def test_names_declared_exported_and_listed(fxlib):
    text = open(os.path.join(ROOT, "include", "fx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in ("fx_map_loop_options", "fx_map_loop_result"):
        assert re.search(r"typedef struct %s\s*\{[^}]*\}\s*%s;" % (n, n), src), n
    for n in ("fx_map_loop_options_default", "fx_map_close_loop", "fx_map_loop_correct_poses"):
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(fxlib, n) and n in capi.EXPORTS, n
    assert "#define FX_VERSION_MINOR 7" in src and fxlib.fx_version() == 7  # added symbols only
    # the sizes the header's comments state
    sizes = {n: int(re.search(r"typedef struct %s \{\s*/\* (\d+) B \*/" % n, text).group(1)) for n in ("fx_map_loop_options", "fx_map_loop_result")}
    assert sizes == {"fx_map_loop_options": C.sizeof(capi.FxMapLoopOptions), "fx_map_loop_result": C.sizeof(capi.FxMapLoopResult)}
    assert C.sizeof(capi.FxMapLoopResult) == capi.LOOP_DTYPE.itemsize == 144 and C.sizeof(capi.FxMapLoopOptions) == 72
    assert [n for n, _ in capi.FxMapLoopResult._fields_] == list(capi.LOOP_DTYPE.names)
    assert all(getattr(capi.FxMapLoopResult, n).offset == capi.LOOP_DTYPE.fields[n][1] for n in capi.LOOP_DTYPE.names)
    o, j = capi.FxMapLoopOptions(), capi.FxMapJoinOptions()
    C.memset(C.byref(o), 0xff, C.sizeof(o))
    fxlib.fx_map_loop_options_default(C.byref(o)), fxlib.fx_map_join_options_default(C.byref(j))
    got = {k: getattr(o, k) for k in capi.LOOP_DEFAULTS}
    assert got == {k: (float(np.float32(v)) if k.endswith(("dist", "baseline")) else v) for k, v in capi.LOOP_DEFAULTS.items()} and o.reserved == 0
    assert all(getattr(o, k) == getattr(j, k) for k in ("search_dist", "inlier_dist", "min_baseline", "hyp_corr", "min_inliers", "min_landmark_obs"))
    assert o.segment == capi.FX_LOC_LAST_SEGMENT and o.min_loop_scans == 256 and o.recent_scans == 32 and o.mode == capi.FX_LOOP_FIT
    for name, v in (("MAX_CORR", 1024), ("FIT", 0), ("GIVEN", 1), ("DRY_RUN", 2), ("APPLIED", 1), ("TRUNCATED", 2), ("NO_HYPOTHESIS", 4),
                    ("BAD_PRIOR", 8), ("BAD_SEGMENT", 0x10), ("FITTED", 0x20), ("TOO_FAR", 0x40)):
        assert getattr(capi, "FX_LOOP_" + name) == v, name
        assert re.search(r"#define FX_LOOP_%s (0x%xu|%du)\s" % (name, v, v), src), name
    assert "fx_map_loop.hip" in __import__("feature_extraction_amd.build", fromlist=["SOURCES"]).SOURCES


# ---- 2. the loop world
@pytest.fixture(scope="module")
def loop():
    w, pieces = lu.loop_world()
    st, pole = lu.run(w, pieces)
    new, res, match = capi.map_loop_reference(st, **lu.OPTS)
    return w, st, pole, new, res, match


def test_a_drifted_loop_is_brought_together(loop):
    """Measured (seed 0, 3e-4 rad and 3 mm a link, 80 scans): the figures are in tests/map_loop_util.py's MEASURED and DESIGN.md
    3.4j; the test prints them."""
    w, st, pole, new, res, match = loop
    n_scans = lu.WORLD["n_scans"]
    assert st["header"]["segments"] == 1 and st["header"]["scans"] == n_scans
    before = pack(st)
    again = capi.map_loop_reference(st, **lu.OPTS)
    assert pack(st) == before and pack(again[0]) == pack(new), "the input is not modified, the call is a function of it"
    d_before, d_after = lu.spread(st, pole), lu.spread(new, pole)
    q = np.flatnonzero(match >= 0)
    lms = new["landmarks"]
    worst = max(math.hypot(lms[i]["x"] - lms[match[i]]["x"], lms[i]["y"] - lms[match[i]]["y"]) for i in q)
    print(f"loop world: {len(st['landmarks'])} landmarks, n_query {res['n_query']}, n_corr {res['n_corr']}, n_inliers {res['n_inliers']}, rms {res['rms']:.4f} m, "
          f"s0 {res['loop_first_scan']}, s1 {res['loop_last_scan']}, moved {res['moved']}; spread before {d_before:.4f} m, after {d_after:.4f} m; "
          f"worst inlier pair after {worst:.4f} m; T yaw {math.atan2(res['s'], res['c']):.5f} rad, t ({res['tx']:.3f}, {res['ty']:.3f})")
    # spread before: beyond what a merge could join
    assert d_before > 1.0
    # close
    assert res["flags"] == F | A and res["n_inliers"] >= 3 == capi.LOOP_DEFAULTS["min_inliers"] and len(q) == res["n_inliers"]
    assert res["loop_first_scan"] < res["loop_last_scan"] and res["segment"] == 0
    # inlier pairs: exact but for the recomputation of the record from the moved sums
    assert worst <= float(np.float32(0.30)) * (1.0 + 2.0 ** -30)
    # targets keep every byte; so does everything at or before s0
    recs_b, recs_a = capi.map_state_records(st)["landmarks"], capi.map_state_records(new)["landmarks"]
    for g in set(int(v) for v in match[q]):
        assert recs_b[g].tobytes() == recs_a[g].tobytes() and st["acc"][g] == new["acc"][g], g
    # spread after: twice the measured value, and that below half the spread before
    bound = 2.0 * lu.MEASURED["d_after"]
    assert bound < d_before / 2.0 and d_after <= bound, (d_before, d_after, bound)
    # last_pose = T o the old one
    T = lu.transform_of(res)
    lp, jp = st["header"]["last_pose"], new["header"]["last_pose"]
    want = capi._rigid_compose(T, tuple(float(v) for v in lp[:5]))
    assert [float(v).hex() for v in jp[:5]] == [float(v).hex() for v in want] and tuple(jp[5:]) == tuple(lp[5:])
    assert {k: v for k, v in new["header"].items() if k != "last_pose"} == {k: v for k, v in st["header"].items() if k != "last_pose"}
    assert new["carry"] == st["carry"] and (new["carry_kp"] == st["carry_kp"]).all() and new["alias"] == [-1] * len(lms)
    assert all((a["n_obs"], a["first_scan"], a["last_scan"], a["segment"]) == (b["n_obs"], b["first_scan"], b["last_scan"], b["segment"])
               for a, b in zip(lms, st["landmarks"]))


def test_the_merge_fuses_the_twins_of_the_closed_map_only(loop):
    w, st, pole, new, res, match = loop
    q = np.flatnonzero(match >= 0)
    n_scans = lu.WORLD["n_scans"]
    closed, _ = mm.merge_to_fixpoint(new, max_calls=16, max_gap_scans=n_scans)
    unclosed, _ = mm.merge_to_fixpoint(st, max_calls=16, max_gap_scans=n_scans)
    rc, ru = lu.roots(closed), lu.roots(unclosed)
    shared = [int(i) for i in q if rc[i] == rc[match[i]]]
    print(f"merge of the closed map: {len(shared)} of {len(q)} inlier pairs share a root")
    assert len(shared) >= 1
    assert not any(ru[i] == ru[match[i]] for i in q), "without the closure the merge joins none of them"


# ---- 3. hand-built states
def _line(scans, segs=None):
    """Landmarks 8 m apart on a line, two observations each, with the scans given."""
    st = lu.timed([(8.0 * k, 2.0) for k in range(len(scans))], scans)
    return st if segs is None else ju.set_segments(st, segs)


def test_weights_at_the_edges_of_the_loop():
    """A pure translation by small integers about a dyadic pivot, s1 - s0 = 8: every step is exact, so the landmark moves by
    alpha t to the bit."""
    s0, s1 = 10, 18
    scans = [(10, 10), (10, 11), (17, 18), (18, 18), (3, 4), (30, 40), (12, 16)]
    alphas = [0.0, 1.0 / 16.0, 15.0 / 16.0, 1.0, 0.0, 1.0, 0.5]
    st = _line(scans)
    T = (1.0, 0.0, 16.0, -32.0, 8.0)
    new, res, match = capi.map_loop_reference(st, prior=T, mode=GIVEN, loop_first_scan=s0, loop_last_scan=s1, pivot_x=4.0, pivot_y=-2.0)
    assert res["flags"] == A and res["moved"] == 5 and (match == -1).all() and (res["px"], res["py"]) == (4.0, -2.0)
    assert (res["loop_first_scan"], res["loop_last_scan"], res["n_query"], res["n_corr"], res["n_inliers"]) == (s0, s1, 0, 0, 0)
    assert lu.transform_of(res) == T and (res["dc"], res["ds"], res["dtx"], res["dty"], res["dtz"]) == (1.0, 0.0, 0.0, 0.0, 0.0) and np.isinf(res["rms"])
    for k, a in enumerate(alphas):
        assert capi._loop_weight(sum(scans[k]), s0, s1) == a
        b, n = st["landmarks"][k], new["landmarks"][k]
        assert (n["x"], n["y"], n["z"]) == (b["x"] + a * 16.0, b["y"] - a * 32.0, b["z"] + a * 8.0) and n["rms_xy"] == b["rms_xy"], k
        if a == 0.0:
            assert n == b and new["acc"][k] == st["acc"][k], "alpha 0: nothing is touched"
    # s1 = s0 + 1: the one interior weight is a half
    assert [capi._loop_weight(t2, 10, 11) for t2 in (20, 21, 22)] == [0.0, 0.5, 1.0]
    # alpha 1 is T itself, bit for bit, and a rotation: against the join's Apply formulas written out
    R = (0.8, 0.6, 3.25, -1.5, 0.125)
    new, res, _ = capi.map_loop_reference(st, prior=R, mode=GIVEN, loop_first_scan=s0, loop_last_scan=s1, pivot_x=1.0, pivot_y=7.0)
    assert capi._loop_transform(R, 1.0, 7.0, 1.0) is R
    c, s, tx, ty, tz = R
    for k in (3, 5):
        a0, a1 = st["acc"][k], new["acc"][k]
        assert a1[:7] == [(c * a0[0] - s * a0[1]) + 2.0 * tx, (s * a0[0] + c * a0[1]) + 2.0 * ty, a0[2] + 2.0 * tz, (c * a0[3] - s * a0[4]) + tx,
                          (s * a0[3] + c * a0[4]) + ty, c * a0[5] - s * a0[6], s * a0[5] + c * a0[6]] and a1[7] == a0[7]
    # an interior weight of a rotation: a rotation (unit c, s) that leaves the pivot on the straight line between its two ends
    ca, sa, txa, tya, tza = capi._loop_transform(R, 1.0, 7.0, 0.5)
    assert abs(ca * ca + sa * sa - 1.0) <= 4 * 2.0 ** -52 and 0.8 < ca < 1.0 and tza == 0.0625
    g = ((c * 1.0 - s * 7.0) + tx, (s * 1.0 + c * 7.0) + ty)
    h = ((ca * 1.0 - sa * 7.0) + txa, (sa * 1.0 + ca * 7.0) + tya)
    assert math.hypot(h[0] - (1.0 + 0.5 * (g[0] - 1.0)), h[1] - (7.0 + 0.5 * (g[1] - 7.0))) <= 64 * 2.0 ** -52


def test_absorbed_landmarks_move_and_other_segments_keep_every_byte():
    scans = [(0, 1), (20, 21), (20, 21), (20, 21)]
    st = _line(scans, segs=[0, 0, 1, 0])
    st["alias"] = [-1, -1, -1, 1]  # 3 is absorbed by 1: it moves with its segment
    st["header"]["last_pose"] = (0.8, 0.6, 3.0, -4.0, 0.5, 1, 0)
    T = (0.6, 0.8, 10.0, -20.0, 0.25)
    kw = dict(prior=T, mode=GIVEN, loop_first_scan=5, loop_last_scan=15, pivot_x=0.0, pivot_y=0.0)
    new, res, _ = capi.map_loop_reference(st, segment=0, **kw)
    assert res["flags"] == A and res["moved"] == 2 and res["segment"] == 0 and new["alias"] == st["alias"]
    assert new["landmarks"][0] == st["landmarks"][0] and new["landmarks"][2] == st["landmarks"][2] and new["acc"][2] == st["acc"][2]
    assert new["acc"][3] != st["acc"][3] and new["landmarks"][3]["x"] != st["landmarks"][3]["x"] and new["acc"][1] != st["acc"][1]
    assert new["header"] == st["header"], "segment 0 is not the current segment: last_pose stays"
    # the current segment: last_pose moves by T (alpha at 2 last = 42 >= 2 s1), segment and flags kept
    new, res, _ = capi.map_loop_reference(st, **kw)
    assert res["flags"] == A and res["moved"] == 1 and res["segment"] == 1
    assert new["header"]["last_pose"] == capi._rigid_compose(T, (0.8, 0.6, 3.0, -4.0, 0.5)) + (1, 0)
    assert [new["landmarks"][k] == st["landmarks"][k] for k in range(4)] == [True, True, False, True]


def test_too_far_dry_run_and_a_failed_fit_change_no_byte():
    st = _line([(0, 1), (20, 21)])
    before = pack(st)
    new, res, _ = capi.map_loop_reference(st, prior=(0.0, 1.0, 0.0, 0.0, 0.0), mode=GIVEN, loop_first_scan=5, loop_last_scan=15)
    assert res["flags"] == TF and res["moved"] == 0 and pack(new) == before, "an exact quarter turn is no drift"
    st = lu.old_and_recent(12, 12)
    before = pack(st)
    full, ref, match = capi.map_loop_reference(st)
    assert ref["flags"] == F | A and ref["n_query"] == 12 == ref["n_corr"] == ref["n_inliers"] and pack(full) != before
    new, res, m2 = capi.map_loop_reference(st, mode=DRY)
    assert pack(new) == before and res["flags"] == F and res["moved"] == 0 and (m2 == match).all()
    assert all(res[k] == ref[k] for k in capi.LOOP_DTYPE.names if k not in ("flags", "moved"))
    new, res, _ = capi.map_loop_reference(st, min_inliers=int(ref["n_inliers"]) + 1)
    assert pack(new) == before and res["flags"] == 0 and res["n_inliers"] == ref["n_inliers"] and res["dtx"] == ref["dtx"]
    assert lu.transform_of(res) == (1.0, 0.0, 0.0, 0.0, 0.0) and res["loop_first_scan"] == res["loop_last_scan"] == capi.FX_LOOP_NONE
    # a fitted quarter turn: the recent landmarks are the old ones turned by 100 degrees about the origin
    th = math.radians(-100.0)
    old = [(8.0 * (k % 4) + 3.0, 8.0 * (k // 4) + 2.0) for k in range(8)]
    rec = [(math.cos(th) * x - math.sin(th) * y, math.sin(th) * x + math.cos(th) * y) for x, y in old]
    st = lu.timed(old + rec, [(0, 1)] * 8 + [(395, 400)] * 8)
    before = pack(st)
    prior = (math.cos(-th), math.sin(-th), 0.0, 0.0, 0.0)
    new, res, _ = capi.map_loop_reference(st, prior=prior)
    assert res["flags"] == F | TF and res["n_inliers"] == 8 and res["c"] < 0 and pack(new) == before


def test_device_refusals_leave_the_state_and_report_the_prior():
    st = lu.old_and_recent(6, 6)
    before = pack(st)
    for kw, flags, seg in ((dict(segment=1), BS, 1), (dict(prior=(1.0, 0.0, float("nan"), 0.0, 0.0)), BP, 0),
                           (dict(segment=7, prior=(float("inf"), 0.0, 0.0, 0.0, 0.0), mode=GIVEN, loop_first_scan=1, loop_last_scan=2), BS | BP, 7)):
        new, res, match = capi.map_loop_reference(st, **kw)
        assert pack(new) == before and res["flags"] == flags and res["segment"] == seg and (match == -1).all()
        assert (res["dc"], res["ds"], res["dtx"], res["dty"], res["dtz"], res["px"], res["py"]) == (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0) and np.isinf(res["rms"])
        assert (res["n_query"], res["n_corr"], res["n_inliers"], res["moved"]) == (0, 0, 0, 0)
        assert all(res[k] == capi.FX_LOOP_NONE for k in ("loop_first_scan", "loop_last_scan", "hyp_a", "hyp_b"))
        P = kw.get("prior", (1.0, 0.0, 0.0, 0.0, 0.0))
        assert [float(v).hex() for v in lu.transform_of(res)] == [float(v).hex() for v in P], "T is the prior as it is"
    # a map of no scans
    empty = capi.map_state(8, 8)
    new, res, _ = capi.map_loop_reference(empty)
    assert res["flags"] == BS and res["segment"] == capi.FX_LOOP_NONE and pack(new) == pack(empty)


@pytest.mark.parametrize("kw", [dict(recent_scans=256), dict(recent_scans=300), dict(segment=capi.FX_LOC_ANY_SEGMENT), dict(mode=3),
                                dict(mode=GIVEN, loop_first_scan=5, loop_last_scan=5), dict(mode=GIVEN, loop_first_scan=6, loop_last_scan=5),
                                dict(mode=GIVEN, loop_first_scan=1, loop_last_scan=5, pivot_x=float("nan")),
                                dict(mode=GIVEN, loop_first_scan=1, loop_last_scan=5, pivot_y=float("inf")), dict(search_dist=0.0),
                                dict(inlier_dist=float("inf")), dict(min_baseline=-1.0), dict(hyp_corr=1), dict(hyp_corr=129), dict(min_inliers=1),
                                dict(min_landmark_obs=0)])
def test_host_refusals_raise(kw):
    with pytest.raises(ValueError):
        capi.map_loop_reference(lu.old_and_recent(4, 4), **kw)


def test_unknown_options_raise():
    with pytest.raises(TypeError):
        capi.map_loop_reference(lu.old_and_recent(4, 4), reserved=1)


def test_a_second_fit_on_the_closed_map_and_its_merge():
    st = lu.old_and_recent(12, 12, n_between=5)
    one, r1, m1 = capi.map_loop_reference(st)
    two, r2, m2 = capi.map_loop_reference(one)
    assert r1["flags"] == r2["flags"] == F | A and (m1 == m2).all() and r2["n_inliers"] == 12
    # the second closure has little left to do: its T is the identity within the first fit's residual
    assert r2["c"] > 1.0 - 1e-6 and math.hypot(r2["tx"], r2["ty"]) <= 2.0 * float(r1["rms"]) + 1e-9 and r2["rms"] <= r1["rms"] * (1.0 + 1e-9)
    q = np.flatnonzero(m1 >= 0)
    for s in (one, two):
        merged, _ = mm.merge_to_fixpoint(s, max_calls=16, max_gap_scans=400)
        r = lu.roots(merged)
        assert all(r[i] == r[m1[i]] for i in q), "every twin is within merge_dist of its old landmark"
    unclosed, _ = mm.merge_to_fixpoint(st, max_calls=16, max_gap_scans=400)
    r = lu.roots(unclosed)
    assert not any(r[i] == r[m1[i]] for i in q), "0.56 m apart: beyond merge_dist"


# ---- 4. poses
def test_poses_follow_the_landmarks():
    s0, s1 = 10, 18
    T = (0.96, 0.28, 3.0, -2.0, 0.5)
    # one landmark of one observation a scan, at the pose's origin
    n = 24
    poses = np.zeros(n, capi.POSE_DTYPE)
    for b in range(n):
        a = 0.05 * b
        poses[b] = (math.cos(a), math.sin(a), 1.5 * b + 0.1, 40.0 - 0.7 * b, 0.01 * b, 0, b & 1)
    st = lu.timed([(float(poses["tx"][b]), float(poses["ty"][b])) for b in range(n)], [(b, b) for b in range(n)])
    for b, (R, acc) in enumerate(zip(st["landmarks"], st["acc"])):
        R["n_obs"] = 1
        R["x"], R["y"], R["z"] = float(poses["tx"][b]), float(poses["ty"][b]), float(poses["tz"][b])
        acc[:] = [R["x"], R["y"], R["z"], R["x"], R["y"], 0.0, 0.0, 0.0]
    new, res, _ = capi.map_loop_reference(st, prior=T, mode=GIVEN, loop_first_scan=s0, loop_last_scan=s1, pivot_x=20.0, pivot_y=30.0)
    assert res["flags"] == A and res["moved"] == n - (s0 + 1)
    out = capi.loop_correct_poses_reference(res, poses, 0)
    assert out[:s0 + 1].tobytes() == poses[:s0 + 1].tobytes(), "alpha 0: the bits stay"
    for b in range(s1, n):
        want = capi._rigid_compose(T, tuple(float(poses[k][b]) for k in ("c", "s", "tx", "ty", "tz")))
        assert tuple(float(out[k][b]) for k in ("c", "s", "tx", "ty", "tz")) == want, "alpha 1: T o pose"
    assert (out["segment"] == poses["segment"]).all() and (out["flags"] == poses["flags"]).all()
    for b in range(n):
        R = new["landmarks"][b]
        assert (float(out["tx"][b]), float(out["ty"][b]), float(out["tz"][b])) == (R["x"], R["y"], R["z"]), f"scan {b}: the pose lands where its landmark does"
    # a window that begins inside the loop
    part = capi.loop_correct_poses_reference(res, poses[12:], 12)
    assert part.tobytes() == out[12:].tobytes()
    # without APPLIED nothing is written
    _, dry, _ = capi.map_loop_reference(st, prior=(0.0, 1.0, 0.0, 0.0, 0.0), mode=GIVEN, loop_first_scan=s0, loop_last_scan=s1)
    assert dry["flags"] == TF and capi.loop_correct_poses_reference(dry, poses, 0).tobytes() == poses.tobytes()
