"""fx_map_close_loop and fx_map_loop_correct_poses on the GPU.  Every call is compared with capi.map_loop_reference — an all-pairs
statement of include/fx.h's definition in numpy float64 that knows nothing of the grid — bit for bit: the map's snapshot
(Map.export_state against map_snapshot_pack of the reference state), the result record and all max_landmarks words of
match_of_landmark; the poses against capi.loop_correct_poses_reference.  The guard words about the outputs must be untouched."""
import ctypes as C
import math

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_join_util as ju
from tests import map_localize_util as llu
from tests import map_loop_util as lu
from tests.test_gpu_map_compact import _compact, _same_state
from tests.test_gpu_map_localize import _device, _localize
from tests.test_gpu_map_merge import _merge_to_fixpoint
from tests.test_gpu_track import FILL, GUARD

pytestmark = pytest.mark.gpu
REC_WORDS = capi.LOOP_DTYPE.itemsize // 4
POSE_WORDS = capi.POSE_DTYPE.itemsize // 4
A, T_, NH, BP, BS, F, TF = (capi.FX_LOOP_APPLIED, capi.FX_LOOP_TRUNCATED, capi.FX_LOOP_NO_HYPOTHESIS, capi.FX_LOOP_BAD_PRIOR,
                            capi.FX_LOOP_BAD_SEGMENT, capi.FX_LOOP_FITTED, capi.FX_LOOP_TOO_FAR)
GIVEN, DRY = capi.FX_LOOP_GIVEN, capi.FX_LOOP_DRY_RUN


@pytest.fixture
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def _map_of(ctx, st):
    mp = ctx.map_create(st["max_landmarks"], st["max_carry_rows"])
    mp.import_state(capi.map_snapshot_pack(st))
    return mp


def _close(ctx, mp, st, what, prior=None, prior_device=None, prior_ref=None, keep=None, **opts):
    """One fx_map_close_loop into guarded outputs against one map_loop_reference call.  keep: a dict that receives the device's
    result tensor.  Returns (the reference's new state, its result, match_of_landmark)."""
    import torch
    dev, cap = f"cuda:{ctx.device}", mp.max_landmarks
    res = torch.full((GUARD + REC_WORDS + GUARD,), FILL, dtype=torch.int32, device=dev)
    match = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.int32, device=dev)
    assert GUARD % 2 == 0
    mp.close_loop(prior=prior, prior_device=prior_device, result=res[GUARD:GUARD + REC_WORDS], match=match[GUARD:GUARD + cap], **opts)
    ctx.synchronize()
    for t, n, name in ((res, REC_WORDS, "the result"), (match, cap, "match_of_landmark")):
        assert (t[:GUARD] == FILL).all().item() and (t[GUARD + n:] == FILL).all().item(), f"{what}: the guards about {name}"
    new, ref, ref_match = capi.map_loop_reference(st, prior=prior if prior_ref is None else prior_ref, **opts)
    lu.assert_result(capi.loop_records(res[GUARD:GUARD + REC_WORDS])[0], ref, what)
    got = match[GUARD:GUARD + cap].cpu().numpy()
    bad = np.flatnonzero(got != ref_match)
    assert not len(bad), f"{what}: match_of_landmark differs at {bad[:8].tolist()}: got {got[bad[:8]]}, reference {ref_match[bad[:8]]}"
    _same_state(mp, new, what)
    if keep is not None:
        keep["result"] = res[GUARD:GUARD + REC_WORDS]
    return new, ref, ref_match


def _given(res):
    return dict(prior=lu.transform_of(res), mode=GIVEN, loop_first_scan=int(res["loop_first_scan"]), loop_last_scan=int(res["loop_last_scan"]),
                pivot_x=float(res["px"]), pivot_y=float(res["py"]))


@pytest.fixture(scope="module")
def loop():
    w, pieces = lu.loop_world()
    st, pole = lu.run(w, pieces)
    return w, pieces, st


def test_a_the_loop_world_in_the_three_modes_and_twice(ctx, loop):
    _, _, st = loop
    mp = _map_of(ctx, st)
    blob = mp.export_state()
    _, dry, _ = _close(ctx, mp, st, "(a) dry run", mode=DRY, **lu.OPTS)
    assert dry["flags"] == F and mp.export_state() == blob
    new, res, match = _close(ctx, mp, st, "(a) fit", **lu.OPTS)
    assert res["flags"] == A | F and res["n_inliers"] >= 3 and res["moved"] > res["n_query"]
    closed = mp.export_state()
    # the same call on the same bytes: the same bytes
    mp.import_state(blob)
    _close(ctx, mp, st, "(a) again", **lu.OPTS)
    assert mp.export_state() == closed
    # GIVEN the fitted T, bounds and pivot: the same map
    mp.import_state(blob)
    _close(ctx, mp, st, "(a) given", **_given(res))
    assert mp.export_state() == closed
    # a second closure of the closed map
    _close(ctx, mp, new, "(a) closed already", **lu.OPTS)
    mp.close()


def test_b_after_a_close_the_map_calls_go_on(ctx, loop):
    """fx_map_localize, fx_map_merge and fx_map_compact after a close, against their references on the reference's closed state."""
    w, pieces, st = loop
    mp = _map_of(ctx, st)
    st, res, match = _close(ctx, mp, st, "(b) close", **lu.OPTS)
    assert res["flags"] == A | F
    b = lu.WORLD["n_scans"] - 1
    off, rows = llu.scans([[tuple(r[:3]) for r in w["rows"][int(w["off"][b]):int(w["off"][b + 1])]]])
    lp = st["header"]["last_pose"]
    pri = llu.identity(1, c=lp[0], s=lp[1], tx=lp[2], ty=lp[3], tz=lp[4])
    got, ref = _localize(ctx, mp, st, off, rows, pri, "(b) localize")
    assert (ref["rec"]["flags"] & capi.FX_LOC_VALID).all()
    st, results = _merge_to_fixpoint(ctx, mp, st, "(b) merge", max_calls=16, max_gap_scans=lu.WORLD["n_scans"])
    q = np.flatnonzero(match >= 0)
    r = lu.roots(st)
    assert any(r[i] == r[match[i]] for i in q), "twins of the loop's two ends are merged"
    st, _, _ = _compact(ctx, mp, st, "(b) compact")
    _same_state(mp, st, "(b) at the end")
    mp.close()


@pytest.mark.parametrize("n", [255, 256, 257])
def test_c_interleaved_ids_across_the_workgroups_edge(ctx, n):
    k = n // 3
    st = lu.old_and_recent(k, k, n - 2 * k)
    assert len(st["landmarks"]) == n
    mp = _map_of(ctx, st)
    new, res, match = _close(ctx, mp, st, f"(c) {n}")
    assert res["flags"] == A | F and res["n_query"] == k == res["n_corr"] == res["n_inliers"] == (match >= 0).sum()
    assert res["moved"] == n - k, "the old landmarks stay, those in between move by their part"
    mp.close()


@pytest.mark.parametrize("n_recent,flags", [(1023, A | F), (1024, A | F), (1025, A | F | T_)])
def test_d_1023_1024_and_1025_correspondences(ctx, n_recent, flags):
    st = lu.old_and_recent(1030, n_recent, pitch=6.0)
    mp = _map_of(ctx, st)
    new, res, match = _close(ctx, mp, st, f"(d) {n_recent}")
    assert res["flags"] == flags and res["n_query"] == n_recent == res["moved"] and res["n_corr"] == min(n_recent, 1024)
    mp.close()


def test_e_three_segments_the_middle_one_closed(ctx):
    st = lu.old_and_recent(8, 8, 8)
    kinds = [k % 3 for k in range(24)]  # old, recent, between interleaved
    st = ju.set_segments(st, [1 if kind < 2 else (0 if k % 2 else 2) for k, kind in enumerate(kinds)], segments=3)
    st["header"]["last_pose"] = (0.8, 0.6, 3.0, -4.0, 0.5, 2, 0)
    mp = _map_of(ctx, st)
    new, res, match = _close(ctx, mp, st, "(e) segment 1 of 3", segment=1)
    assert res["flags"] == A | F and res["moved"] == 8 and res["segment"] == 1 and new["header"] == st["header"]
    for k, (a, b) in enumerate(zip(new["landmarks"], st["landmarks"])):
        assert (a == b) == (b["segment"] != 1 or kinds[k] == 0), k
    _, res, _ = _close(ctx, mp, new, "(e) the last segment holds nothing old", min_inliers=2)
    assert res["flags"] == NH and res["segment"] == 2
    mp.close()


def test_f_hand_built_edges(ctx):
    from tests.test_map_loop_reference import _line
    # the weights at the loop's two ends, s1 = s0 + 1, a rotation
    scans = [(10, 10), (10, 11), (17, 18), (18, 18), (3, 4), (30, 40), (12, 16)]
    st = _line(scans)
    mp = _map_of(ctx, st)
    blob = mp.export_state()
    for T, s0, s1, moved in (((1.0, 0.0, 16.0, -32.0, 8.0), 10, 18, 5), ((0.8, 0.6, 3.25, -1.5, 0.125), 10, 18, 5), ((0.8, 0.6, 3.25, -1.5, 0.125), 10, 11, 5),
                             ((0.28, -0.96, -7.0, 2.0, 0.0), 0, 0xfffffffe, 7)):
        mp.import_state(blob)
        _, res, _ = _close(ctx, mp, st, f"(f) given {T} {s0} {s1}", prior=T, mode=GIVEN, loop_first_scan=s0, loop_last_scan=s1, pivot_x=4.0, pivot_y=-2.0)
        assert res["flags"] == A and res["moved"] == moved
    # a quarter turn given: too far
    mp.import_state(blob)
    _, res, _ = _close(ctx, mp, st, "(f) too far", prior=(0.0, 1.0, 0.0, 0.0, 0.0), mode=GIVEN, loop_first_scan=5, loop_last_scan=15)
    assert res["flags"] == TF and mp.export_state() == blob
    mp.close()
    # an absorbed landmark moves, another segment's keeps every byte, last_pose with the current segment
    st = _line([(0, 1), (20, 21), (20, 21), (20, 21)], segs=[0, 0, 1, 0])
    st["alias"] = [-1, -1, -1, 1]
    st["header"]["last_pose"] = (0.8, 0.6, 3.0, -4.0, 0.5, 1, 0)
    kw = dict(prior=(0.6, 0.8, 10.0, -20.0, 0.25), mode=GIVEN, loop_first_scan=5, loop_last_scan=15)
    mp = _map_of(ctx, st)
    one, res, _ = _close(ctx, mp, st, "(f) segment 0", segment=0, **kw)
    assert res["moved"] == 2
    _, res, _ = _close(ctx, mp, one, "(f) the current segment", **kw)
    assert res["moved"] == 1 and res["segment"] == 1
    mp.close()
    # a failed fit, a fitted quarter turn, not finite and few observations, the equidistant targets
    st = lu.old_and_recent(12, 12)
    lms = st["landmarks"]
    old, rec = [i for i in range(24) if i % 2 == 0], [i for i in range(24) if i % 2 == 1]
    st["alias"] = [-1] * 24
    st["alias"][rec[1]] = rec[0]        # an absorbed recent landmark: no query, but it moves
    st["alias"][old[2]] = old[0]        # an absorbed target: query rec[2] finds nothing (the lattice's pitch is beyond search_dist)
    lms[rec[3]]["x"] = float("nan")     # records that are not finite: no query, no target (their sums are: they move)
    lms[old[4]]["z"] = float("inf")
    lms[rec[5]]["n_obs"] = 1            # below min_landmark_obs = 2
    lms[old[6]]["n_obs"] = 1
    q, t = lms[rec[7]], lms[old[7]]
    lms[old[8]] = dict(lms[old[8]], x=2.0 * q["x"] - t["x"], y=2.0 * q["y"] - t["y"])  # the mirror image of old[7] about query rec[7]
    assert (lms[old[8]]["x"] - q["x"], lms[old[8]]["y"] - q["y"]) == (q["x"] - t["x"], q["y"] - t["y"]), "exactly as far"
    mp = _map_of(ctx, st)
    blob = mp.export_state()
    _, dry, match = _close(ctx, mp, st, "(f) dry", mode=DRY)
    assert dry["n_query"] == 12 - 3 and match[rec[7]] == old[7] < old[8] and all(match[rec[k]] == -1 for k in (1, 2, 3, 5))
    _, res, _ = _close(ctx, mp, st, "(f) a failed fit", min_inliers=int(dry["n_inliers"]) + 1)
    assert res["flags"] == 0 and mp.export_state() == blob
    new, res, _ = _close(ctx, mp, st, "(f) fit")
    assert res["flags"] == A | F and res["moved"] == 12 and math.isfinite(new["landmarks"][rec[3]]["x"])
    mp.close()
    th = math.radians(-100.0)
    pts = [(8.0 * (k % 4) + 3.0, 8.0 * (k // 4) + 2.0) for k in range(8)]
    st = lu.timed(pts + [(math.cos(th) * x - math.sin(th) * y, math.sin(th) * x + math.cos(th) * y) for x, y in pts], [(0, 1)] * 8 + [(395, 400)] * 8)
    mp = _map_of(ctx, st)
    blob = mp.export_state()
    _, res, _ = _close(ctx, mp, st, "(f) a fitted quarter turn", prior=(math.cos(-th), math.sin(-th), 0.0, 0.0, 0.0))
    assert res["flags"] == F | TF and mp.export_state() == blob
    mp.close()
    # a map of no scans
    empty = capi.map_state(8, 8)
    mp = ctx.map_create(8, 8)
    _, res, _ = _close(ctx, mp, empty, "(f) an empty map")
    assert res["flags"] == BS and res["segment"] == capi.FX_LOOP_NONE
    _, res, _ = _close(ctx, mp, empty, "(f) an empty map, given", prior=(1.0, 0.0, 1.0, 0.0, 0.0), mode=GIVEN, loop_first_scan=0, loop_last_scan=1, segment=0)
    assert res["flags"] == BS and res["segment"] == 0
    mp.close()


def test_g_a_device_prior_from_a_localization(ctx, loop):
    """The run's last scan localised under last_pose: the record's D, read on the device, is the closure's prior."""
    import torch
    w, pieces, st = loop
    mp = _map_of(ctx, st)
    b = lu.WORLD["n_scans"] - 1
    off, rows = llu.scans([[tuple(r[:3]) for r in w["rows"][int(w["off"][b]):int(w["off"][b + 1])]]])
    lp = st["header"]["last_pose"]
    held = llu.identity(1, c=lp[0], s=lp[1], tx=lp[2], ty=lp[3], tz=lp[4])
    kp, pri = _device(ctx, off, rows, held, 3, len(rows) + 9)
    recs, _, _ = mp.localize(kp, pri, 1, q_max_rows=len(rows))
    ctx.synchronize()
    loc = capi.localize_records(recs)
    assert loc["flags"][0] & capi.FX_LOC_VALID
    D = tuple(float(loc[k][0]) for k in ("dc", "ds", "dtx", "dty", "dtz"))
    d_ptr = recs.data_ptr() + capi.LOC_DTYPE.fields["dc"][1]
    new, res, _ = _close(ctx, mp, st, "(g) the prior on the device", prior_device=d_ptr, prior_ref=D, **lu.OPTS)
    assert res["flags"] == A | F and lu.transform_of(res) != D
    # a device prior that is not finite and a segment that is not there: reported, nothing changed
    bad = torch.tensor([1.0, 0.0, float("nan"), 0.0, 0.0], dtype=torch.float64, device=f"cuda:{ctx.device}")
    _, res, _ = _close(ctx, mp, new, "(g) NaN", prior_device=bad, prior_ref=(1.0, 0.0, float("nan"), 0.0, 0.0), **lu.OPTS)
    assert res["flags"] == BP
    _, res, _ = _close(ctx, mp, new, "(g) NaN and segment 5", prior_device=bad, prior_ref=(1.0, 0.0, float("nan"), 0.0, 0.0), segment=5)
    assert res["flags"] == BP | BS and res["segment"] == 5
    mp.close()


@pytest.mark.parametrize("n,first", [(1, 14), (64, 0), (65, 3)])
def test_h_poses_across_the_loops_two_ends(ctx, n, first):
    import torch
    from tests.test_map_loop_reference import _line
    dev = f"cuda:{ctx.device}"
    st = _line([(0, 1), (70, 71)])
    mp = _map_of(ctx, st)
    poses = np.zeros(n, capi.POSE_DTYPE)
    for b in range(n):
        a = 0.05 * (first + b)
        poses[b] = (math.cos(a), math.sin(a), 1.5 * b + 0.1, 40.0 - 0.7 * b, 0.01 * b, 0, b & 1)
    keep = {}
    st, res, _ = _close(ctx, mp, st, "(h) given", keep=keep, prior=(0.96, 0.28, 3.0, -2.0, 0.5), mode=GIVEN, loop_first_scan=10, loop_last_scan=18,
                       pivot_x=20.0, pivot_y=30.0)
    assert res["flags"] == A
    buf = torch.full((GUARD + n * POSE_WORDS + GUARD,), FILL, dtype=torch.int32, device=dev)
    body = buf[GUARD:GUARD + n * POSE_WORDS]
    body.copy_(torch.from_numpy(poses.view(np.int32).copy()).to(dev))
    mp.loop_correct_poses(keep["result"], body, first)
    ctx.synchronize()
    assert (buf[:GUARD] == FILL).all().item() and (buf[GUARD + n * POSE_WORDS:] == FILL).all().item(), "the guards about the poses"
    want = capi.loop_correct_poses_reference(res, poses, first)
    got = body.cpu().numpy().view(capi.POSE_DTYPE)
    assert got.tobytes() == want.tobytes(), np.flatnonzero([g.tobytes() != r.tobytes() for g, r in zip(got, want)])[:8]
    assert n == 1 or got.tobytes() != poses.tobytes()
    # twice from the same state: the same bytes; fewer poses than the tensor holds: the rest stays
    body.copy_(torch.from_numpy(poses.view(np.int32).copy()).to(dev))
    mp.loop_correct_poses(keep["result"], body, first, n_poses=n - 1)
    ctx.synchronize()
    got = body.cpu().numpy().view(capi.POSE_DTYPE)
    assert got[:n - 1].tobytes() == want[:n - 1].tobytes() and got[n - 1:].tobytes() == poses[n - 1:].tobytes()
    # a result without APPLIED: nothing is written
    _, res, _ = _close(ctx, mp, st, "(h) too far", keep=keep, prior=(0.0, 1.0, 0.0, 0.0, 0.0), mode=GIVEN, loop_first_scan=10, loop_last_scan=18)
    assert res["flags"] == TF
    body.copy_(torch.from_numpy(poses.view(np.int32).copy()).to(dev))
    mp.loop_correct_poses(keep["result"], body, first)
    ctx.synchronize()
    assert body.cpu().numpy().tobytes() == poses.tobytes()
    mp.close()


def test_i_host_refusals_touch_nothing(ctx, fxlib):
    import torch
    st = lu.old_and_recent(6, 6)
    mp = _map_of(ctx, st)
    other = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    blob = mp.export_state()
    dev = f"cuda:{ctx.device}"
    res = torch.full((REC_WORDS + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    match = torch.full((mp.max_landmarks + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    poses = torch.full((4 * POSE_WORDS + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    pd = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev)
    P = C.c_void_p
    r, m, ps = res.data_ptr() + 4 * GUARD, match.data_ptr() + 4 * GUARD, poses.data_ptr() + 4 * GUARD

    def opt(**kw):
        o = capi.FxMapLoopOptions()
        fxlib.fx_map_loop_options_default(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    nan = capi.FxPose(1.0, 0.0, float("nan"), 0.0, 0.0, 0, 0)
    ok = capi.FxPose(1.0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    h, mh = ctx.handle, mp.handle
    given = dict(mode=GIVEN, loop_first_scan=1, loop_last_scan=5)
    cases = [("null ctx", (None, mh, None, None, None, P(r), P(m)), b"null"),
             ("null map", (h, None, None, None, None, P(r), P(m)), b"null"),
             ("another context's map", (other.handle, mh, None, None, None, P(r), P(m)), b"another context"),
             ("both priors", (h, mh, C.byref(ok), P(pd.data_ptr()), None, P(r), P(m)), b"not both"),
             ("prior_host not finite", (h, mh, C.byref(nan), None, None, P(r), P(m)), b"finite"),
             ("search_dist", (h, mh, None, None, opt(search_dist=0.0), P(r), P(m)), b"search_dist"),
             ("inlier_dist", (h, mh, None, None, opt(inlier_dist=float("inf")), P(r), P(m)), b"inlier_dist"),
             ("min_baseline", (h, mh, None, None, opt(min_baseline=-1.0), P(r), P(m)), b"min_baseline"),
             ("hyp_corr 1", (h, mh, None, None, opt(hyp_corr=1), P(r), P(m)), b"hyp_corr"),
             ("hyp_corr 129", (h, mh, None, None, opt(hyp_corr=129), P(r), P(m)), b"hyp_corr"),
             ("min_inliers", (h, mh, None, None, opt(min_inliers=1), P(r), P(m)), b"min_inliers"),
             ("min_landmark_obs", (h, mh, None, None, opt(min_landmark_obs=0), P(r), P(m)), b"min_landmark_obs"),
             ("recent_scans == min_loop_scans", (h, mh, None, None, opt(recent_scans=256), P(r), P(m)), b"recent_scans"),
             ("recent_scans above", (h, mh, None, None, opt(min_loop_scans=8), P(r), P(m)), b"recent_scans"),
             ("any segment", (h, mh, None, None, opt(segment=capi.FX_LOC_ANY_SEGMENT), P(r), P(m)), b"FX_LOC_ANY_SEGMENT"),
             ("mode", (h, mh, None, None, opt(mode=3), P(r), P(m)), b"mode"),
             ("given, s0 == s1", (h, mh, None, None, opt(mode=GIVEN, loop_first_scan=5, loop_last_scan=5), P(r), P(m)), b"loop_first_scan"),
             ("given, s0 > s1", (h, mh, None, None, opt(mode=GIVEN, loop_first_scan=6, loop_last_scan=5), P(r), P(m)), b"loop_first_scan"),
             ("given, pivot_x", (h, mh, None, None, opt(pivot_x=float("nan"), **given), P(r), P(m)), b"pivot"),
             ("given, pivot_y", (h, mh, None, None, opt(pivot_y=float("-inf"), **given), P(r), P(m)), b"pivot"),
             ("reserved", (h, mh, None, None, opt(reserved=1), P(r), P(m)), b"reserved"),
             ("prior_device alignment", (h, mh, None, P(pd.data_ptr() + 4), None, P(r), P(m)), b"aligned"),
             ("result alignment", (h, mh, None, None, None, P(r + 4), P(m)), b"aligned"),
             ("match alignment", (h, mh, None, None, None, P(r), P(m + 2)), b"aligned")]
    for name, args, word in cases:
        assert fxlib.fx_map_close_loop(*args) == capi.FX_ERR_INVALID_ARG and word in fxlib.fx_last_error(), (name, fxlib.fx_last_error())
    for name, args, word in [("null ctx", (None, P(r), P(ps), 0, 4), b"null"), ("null result", (h, None, P(ps), 0, 4), b"null"),
                             ("null poses", (h, P(r), None, 0, 4), b"null"), ("result alignment", (h, P(r + 4), P(ps), 0, 4), b"aligned"),
                             ("poses alignment", (h, P(r), P(ps + 4), 0, 3), b"aligned")]:
        assert fxlib.fx_map_loop_correct_poses(*args) == capi.FX_ERR_INVALID_ARG and word in fxlib.fx_last_error(), (name, fxlib.fx_last_error())
    ctx.synchronize()
    assert (res == FILL).all().item() and (match == FILL).all().item() and (poses == FILL).all().item() and mp.export_state() == blob
    # a pivot that is not finite is no refusal outside FX_LOOP_GIVEN, NULL outputs are none at all, and no pose is no launch
    new, _, _ = capi.map_loop_reference(st)
    assert mp.close_loop(result=False, match=False, pivot_x=float("nan")) == (None, None)
    _same_state(mp, new, "(i) without outputs")
    assert fxlib.fx_map_loop_correct_poses(h, P(r), P(ps), 0, 0) == 0
    ctx.synchronize()
    assert (poses == FILL).all().item()
    mp.close(), other.close()
