"""capi.map_join_reference, the executable statement of fx_map_join_segments (include/fx.h), on the CPU: the declarations, what the
call is for (a run cut by one bad link made one map again), the label arithmetic, last_pose, the run going on after a join, and
the modes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_join_util as ju
from tests import map_merge_util as mm
from tests import map_util as mu
from tests import track_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = capi


def test_names_declared_exported_and_listed(fxlib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fx.h")).read(), flags=re.S)
    for n in ("fx_map_join_options", "fx_map_join_result"):
        assert re.search(r"typedef struct %s\s*\{[^}]*\}\s*%s;" % (n, n), src), n
    for n in ("fx_map_join_options_default", "fx_map_join_segments"):
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(fxlib, n) and n in capi.EXPORTS, n
    assert "#define FX_VERSION_MINOR 7" in src and fxlib.fx_version() == 7  # added symbols only
    assert C.sizeof(capi.FxMapJoinOptions) == 32 and C.sizeof(capi.FxMapJoinResult) == 120 == capi.JOIN_DTYPE.itemsize
    o, l = capi.FxMapJoinOptions(), capi.FxLocalizeOptions()
    fxlib.fx_map_join_options_default(C.byref(o)), fxlib.fx_localize_options_default(C.byref(l))
    got = {k: getattr(o, k) for k in capi.JOIN_DEFAULTS}
    assert got == {k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in capi.JOIN_DEFAULTS.items()} and o.reserved == 0
    assert all(getattr(o, k) == getattr(l, k) for k in ("search_dist", "inlier_dist", "min_baseline", "hyp_corr", "min_inliers", "min_landmark_obs"))
    for name, v in (("MAX_CORR", 1024), ("FIT", 0), ("GIVEN", 1), ("DRY_RUN", 2), ("APPLIED", 1), ("TRUNCATED", 2), ("NO_HYPOTHESIS", 4),
                    ("BAD_PRIOR", 8), ("BAD_SEGMENT", 0x10), ("FITTED", 0x20)):
        assert getattr(capi, "FX_JOIN_" + name) == v and re.search(r"#define FX_JOIN_%s (0x)?%xu\b" % (name, v), src) or \
            re.search(r"#define FX_JOIN_%s %du\b" % (name, v), src), name
    assert "fx_map_join.hip" in __import__("feature_extraction_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.fixture(scope="module")
def runs():
    f = ju.WORLD
    w, broken, whole = ju.world()
    stb, _, idb = mu.run_reference(broken, f["cap"], f["carry"])
    stw, _, idw = mu.run_reference(whole, f["cap"], f["carry"])
    return w, broken, whole, stb, idb, stw, idw


def test_a_run_cut_by_one_bad_link_is_one_map_again(runs):
    """Measured (seed 10, link 12 bad): 24 queries, 5 correspondences, 4 inliers; after the join and the merge's fixpoint every
    landmark lies within 0.0148 m of the unbroken run's landmark of its pole (bound: inlier_dist 0.30 m), the yaw of T is within
    2.9e-4 rad of the true step."""
    w, broken, whole, stb, idb, stw, idw = runs
    assert stb["header"]["segments"] == 2 and stw["header"]["segments"] == 1
    before = capi.map_snapshot_pack(stb)
    st, res, match = capi.map_join_reference(stb, 1, 0)
    assert capi.map_snapshot_pack(stb) == before, "the input is not modified"
    assert res["flags"] == capi.FX_JOIN_APPLIED | capi.FX_JOIN_FITTED and res["label"] == 0 and res["segments"] == 1 == st["header"]["segments"]
    seg = np.array([r["segment"] for r in stb["landmarks"]])
    assert res["moved"] == (seg == 1).sum() > 0 and all(r["segment"] == 0 for r in st["landmarks"])
    assert res["n_inliers"] >= 3 and (match >= 0).sum() == res["n_inliers"] and (seg[match[match >= 0]] == 0).all() and (seg[np.flatnonzero(match >= 0)] == 1).all()
    # T against the truth: the held pose is scan BAD's, so T is the true motion scan BAD + 1 -> scan BAD seen in the map's frame
    b = ju.WORLD["bad"]
    yaw_err = tu.yaw_err(math.atan2(res["s"], res["c"]), w["truth"][b + 1][0] - w["truth"][b][0])
    st, _ = mm.merge_to_fixpoint(st, max_calls=8)
    stw, _ = mm.merge_to_fixpoint(stw, max_calls=8)
    pb, pw = ju.poles_of(w, broken, idb, len(stb["landmarks"])), ju.poles_of(w, whole, idw, len(stw["landmarks"]))
    both = set(pb[seg == 0].tolist()) & set(pb[seg == 1].tolist())
    lv, lw = ju.live(st), ju.live(stw)
    count = {}
    for i in lv:
        count[int(pb[i])] = count.get(int(pb[i]), 0) + 1
    assert len(both) >= 10 and all(count.get(k, 0) == 1 for k in both), {k: count.get(k, 0) for k in both}
    worst = 0.0
    for i in lv:
        twins = [j for j in lw if pw[j] == pb[i]]
        assert twins, f"pole {pb[i]} has no landmark in the unbroken run"
        worst = max(worst, min(math.hypot(st["landmarks"][i]["x"] - stw["landmarks"][j]["x"], st["landmarks"][i]["y"] - stw["landmarks"][j]["y"]) for j in twins))
    print(f"join of the broken world: n_src {res['n_src']}, n_corr {res['n_corr']}, n_inliers {res['n_inliers']}, rms {res['rms']:.4f} m; "
          f"worst distance to the unbroken run {worst:.4f} m, yaw error of T {yaw_err:.2e} rad; {len(both)} poles on both sides")
    assert worst <= float(np.float32(0.30))
    # a second join of the joined map: one segment is left
    st2, res2, match2 = capi.map_join_reference(st, 1, 0)
    assert res2["flags"] == capi.FX_JOIN_BAD_SEGMENT and res2["moved"] == 0 and (match2 == -1).all()
    assert capi.map_snapshot_pack(st2) == capi.map_snapshot_pack(st)


def test_the_run_goes_on_in_the_joined_segment():
    """The bad link inside the last batch but one: the current segment takes part, the next overlap continues its landmarks."""
    f = ju.WORLD
    w, broken, _ = ju.world(bad=17)  # (inside the piece of scans 15 .. 20; the last piece is 20 .. 23)
    st, _, _ = mu.run_reference(broken[:-1], f["cap"], f["carry"])
    assert st["header"]["segments"] == 2 and st["header"]["last_pose"][5] == 1
    joined, res, _ = capi.map_join_reference(st, 1, 0, search_dist=2.0)
    if not res["flags"] & capi.FX_JOIN_APPLIED:  # (what the association finds under the identity is not this test's subject)
        b = 17
        yaw = w["truth"][b + 1][0] - w["truth"][b][0]
        joined, res, _ = capi.map_join_reference(st, 1, 0, prior=(math.cos(yaw), math.sin(yaw), 0.0, 0.0, 0.0), search_dist=8.0)
    assert res["flags"] & capi.FX_JOIN_APPLIED and joined["header"]["segments"] == 1
    T = tuple(float(res[k]) for k in ("c", "s", "tx", "ty", "tz"))
    lp, jp = st["header"]["last_pose"], joined["header"]["last_pose"]
    want = (T[0] * lp[0] - T[1] * lp[1], T[1] * lp[0] + T[0] * lp[1], (T[0] * lp[2] - T[1] * lp[3]) + T[2], (T[1] * lp[2] + T[0] * lp[3]) + T[3], lp[4] + T[4])
    assert [float(v).hex() for v in jp[:5]] == [float(v).hex() for v in want] and tuple(jp[5:]) == tuple(lp[5:]), "last_pose = T o last_pose"
    assert joined["carry"] == st["carry"] and (joined["carry_kp"] == st["carry_kp"]).all() and joined["alias"] == [-1] * len(st["landmarks"])
    p = broken[-1]
    tr = tu.reference(p, init_pose=jp[:5])
    nxt, ids = capi.map_reference(joined, p["off"], p["rows"], tr, overlap=True)
    H = nxt["header"]
    assert H["last_joined"] > 0 and H["last_new"] > 0 and not H["flags"] & capi.FX_MAP_OVERLAP_MISMATCH and H["segments"] == 1
    assert all(r["segment"] == H["segments"] - 1 for r in nxt["landmarks"][joined["header"]["n_landmarks"]:])
    # and the pose is dst's frame again: the last pose against the truth
    yaw_err = tu.yaw_err(math.atan2(H["last_pose"][1], H["last_pose"][0]), w["truth"][-1][0])
    assert math.hypot(H["last_pose"][2] - w["truth"][-1][1], H["last_pose"][3] - w["truth"][-1][2]) <= 0.30 and yaw_err <= 0.01


def _three():
    """9 landmarks of three segments (0 1 2 0 1 2 ...), 100 m apart by segment so that nothing associates; last_pose in segment 2."""
    frags = [(0, ju.F32(100.0 * (k % 3) + 5.0 * (k // 3)), ju.F32(7.0 * (k // 3))) for k in range(9)]
    st, _ = mm.reference_of(mm.fragments(frags, 3), cap=12, carry=8)
    st = ju.set_segments(st, [k % 3 for k in range(9)])
    st["header"]["last_pose"] = (0.8, 0.6, 3.0, -4.0, 0.5, 2, 0)
    return st


@pytest.mark.parametrize("src,dst", [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)])
def test_label_arithmetic_on_three_segments(src, dst):
    st = _three()
    T = (0.6, 0.8, 10.0, -20.0, 0.25)
    out, res, match = capi.map_join_reference(st, src, dst, prior=T, mode=capi.FX_JOIN_GIVEN)
    lo, hi = min(src, dst), max(src, dst)
    relabel = lambda s: hi - 1 if s == lo else (s - 1 if s > lo else s)
    assert [r["segment"] for r in out["landmarks"]] == [relabel(k % 3) for k in range(9)]
    assert res["flags"] == capi.FX_JOIN_APPLIED and res["label"] == hi - 1 and res["segments"] == 2 == out["header"]["segments"] and res["moved"] == 3
    assert (res["n_src"], res["n_corr"], res["n_inliers"], res["hyp_a"], res["hyp_b"]) == (0, 0, 0, capi.FX_JOIN_NONE, capi.FX_JOIN_NONE) and (match == -1).all()
    assert np.isinf(res["rms"]) and tuple(float(res[k]) for k in ("c", "s", "tx", "ty", "tz")) == T and (res["dc"], res["ds"], res["dtx"]) == (1.0, 0.0, 0.0)
    lp = st["header"]["last_pose"]
    if src == 2:  # the current segment moved: last_pose with it
        want = (T[0] * lp[0] - T[1] * lp[1], T[1] * lp[0] + T[0] * lp[1], (T[0] * lp[2] - T[1] * lp[3]) + T[2], (T[1] * lp[2] + T[0] * lp[3]) + T[3], lp[4] + T[4])
        assert out["header"]["last_pose"] == want + (2, 0)
    else:
        assert out["header"]["last_pose"] == lp
    for k in range(9):
        if k % 3 != src:
            assert out["landmarks"][k] == dict(st["landmarks"][k], segment=relabel(k % 3)) and out["acc"][k] == st["acc"][k], k
    assert {k: v for k, v in out["header"].items() if k not in ("segments", "last_pose")} == {k: v for k, v in st["header"].items() if k not in ("segments", "last_pose")}


def test_given_reproduces_hand_computed_sums():
    """A quarter turn and a shift of small integers: every product and sum is exact."""
    st = ju.two_segments(2, 2)
    i = next(k for k, r in enumerate(st["landmarks"]) if r["segment"] == 1)
    st["acc"][i] = [6.0, 10.0, 4.0, 3.0, 5.0, 0.5, -0.25, 0.125]  # Sx Sy Sz ax ay Dx Dy Q, n_obs 2
    out, res, _ = capi.map_join_reference(st, 1, 0, prior=(0.0, 1.0, 7.0, -2.0, 1.5), mode=capi.FX_JOIN_GIVEN)
    # c = 0, s = 1: (x, y) -> (-y, x) + (7, -2); sums carry n = 2 translations
    assert out["acc"][i] == [-10.0 + 14.0, 6.0 - 4.0, 4.0 + 3.0, -5.0 + 7.0, 3.0 - 2.0, 0.25, 0.5, 0.125]
    R = out["landmarks"][i]
    var = 0.125 / 2.0 - (0.125 * 0.125 + 0.25 * 0.25)
    assert (R["x"], R["y"], R["z"]) == (2.0, 1.0, 3.5) and R["rms_xy"] == np.float32(math.sqrt(var if var > 0 else 0.0)) and R["segment"] == 0
    assert res["moved"] == 2 and res["flags"] == capi.FX_JOIN_APPLIED
    # absorbed landmarks of src move too
    st2 = dict(st, alias=[-1] * len(st["landmarks"]))
    j = next(k for k, r in enumerate(st["landmarks"]) if r["segment"] == 1 and k != i)
    st2["alias"][i] = j
    out2, res2, _ = capi.map_join_reference(st2, 1, 0, prior=(0.0, 1.0, 7.0, -2.0, 1.5), mode=capi.FX_JOIN_GIVEN)
    assert out2["acc"][i] == out["acc"][i] and out2["alias"] == st2["alias"] and res2["moved"] == 2


def test_a_dry_run_and_a_fit_below_min_inliers_change_no_byte(runs):
    stb = runs[3]
    before = capi.map_snapshot_pack(stb)
    full, ref, _ = capi.map_join_reference(stb, 1, 0)
    out, res, match = capi.map_join_reference(stb, 1, 0, mode=capi.FX_JOIN_DRY_RUN)
    assert capi.map_snapshot_pack(out) == before and res["flags"] == capi.FX_JOIN_FITTED and res["moved"] == 0 and res["label"] == capi.FX_JOIN_NONE
    assert res["segments"] == 2 and all(res[k] == ref[k] for k in ("c", "s", "tx", "ty", "tz", "dc", "ds", "dtx", "dty", "dtz", "rms", "n_inliers", "hyp_a", "hyp_b"))
    assert (match >= 0).sum() == res["n_inliers"]
    out, res, _ = capi.map_join_reference(stb, 1, 0, min_inliers=int(ref["n_inliers"]) + 1)
    assert capi.map_snapshot_pack(out) == before and res["flags"] == 0 and res["n_inliers"] == ref["n_inliers"] and res["dc"] == ref["dc"]
    assert [float(res[k]) for k in ("c", "s", "tx", "ty", "tz")] == [1.0, 0.0, 0.0, 0.0, 0.0], "without a fit T is the prior"
    # the device refusals: a prior that is not finite, a segment that is not there
    out, res, _ = capi.map_join_reference(stb, 1, 0, prior=(1.0, 0.0, float("nan"), 0.0, 0.0))
    assert capi.map_snapshot_pack(out) == before and res["flags"] == capi.FX_JOIN_BAD_PRIOR and np.isnan(res["tx"])
    out, res, _ = capi.map_join_reference(stb, 2, 0, prior=(1.0, 0.0, float("inf"), 0.0, 0.0))
    assert capi.map_snapshot_pack(out) == before and res["flags"] == capi.FX_JOIN_BAD_PRIOR | capi.FX_JOIN_BAD_SEGMENT
    with pytest.raises(ValueError):
        capi.map_join_reference(stb, 1, 1)
    with pytest.raises(ValueError):
        capi.map_join_reference(stb, 1, 0, mode=3)
