"""fx_map_join_segments on the GPU.  Every call is compared with capi.map_join_reference — an all-pairs statement of include/fx.h's
definition in numpy float64 that knows nothing of the grid — bit for bit: the map's snapshot (Map.export_state against
map_snapshot_pack of the reference state), the result record and all max_landmarks words of match_of_landmark.  The guard words
about the two outputs must be untouched."""
import ctypes as C
import math

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_join_util as ju
from tests import map_localize_util as lu
from tests import map_util as mu
from tests.test_gpu_map import _step
from tests.test_gpu_map_compact import _compact, _same_state
from tests.test_gpu_map_localize import _localize
from tests.test_gpu_map_merge import _merge_to_fixpoint
from tests.test_gpu_track import FILL, GUARD

pytestmark = pytest.mark.gpu
REC_WORDS = capi.JOIN_DTYPE.itemsize // 4
A, T_, NH, BP, BS, F = (capi.FX_JOIN_APPLIED, capi.FX_JOIN_TRUNCATED, capi.FX_JOIN_NO_HYPOTHESIS, capi.FX_JOIN_BAD_PRIOR, capi.FX_JOIN_BAD_SEGMENT,
                        capi.FX_JOIN_FITTED)


@pytest.fixture
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def _map_of(ctx, st):
    mp = ctx.map_create(st["max_landmarks"], st["max_carry_rows"])
    mp.import_state(capi.map_snapshot_pack(st))
    return mp


def _join(ctx, mp, st, src, dst, what, prior=None, prior_device=None, prior_ref=None, **opts):
    """One fx_map_join_segments into guarded outputs against one map_join_reference call.  Returns (the reference's new state, its
    result, match_of_landmark)."""
    import torch
    dev, cap = f"cuda:{ctx.device}", mp.max_landmarks
    res = torch.full((GUARD + REC_WORDS + GUARD,), FILL, dtype=torch.int32, device=dev)
    match = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.int32, device=dev)
    assert GUARD % 2 == 0
    mp.join_segments(src, dst, prior=prior, prior_device=prior_device, result=res[GUARD:GUARD + REC_WORDS], match=match[GUARD:GUARD + cap], **opts)
    ctx.synchronize()
    for t, n, name in ((res, REC_WORDS, "the result"), (match, cap, "match_of_landmark")):
        assert (t[:GUARD] == FILL).all().item() and (t[GUARD + n:] == FILL).all().item(), f"{what}: the guards about {name}"
    new, ref, ref_match = capi.map_join_reference(st, src, dst, prior=prior if prior_ref is None else prior_ref, **opts)
    ju.assert_result(capi.join_records(res[GUARD:GUARD + REC_WORDS])[0], ref, what)
    got = match[GUARD:GUARD + cap].cpu().numpy()
    bad = np.flatnonzero(got != ref_match)
    assert not len(bad), f"{what}: match_of_landmark differs at {bad[:8].tolist()}: got {got[bad[:8]]}, reference {ref_match[bad[:8]]}"
    _same_state(mp, new, what)
    return new, ref, ref_match


@pytest.fixture(scope="module")
def broken():
    f = ju.WORLD
    w, pieces, _ = ju.world()
    st, _, _ = mu.run_reference(pieces, f["cap"], f["carry"])
    return w, pieces, st


def test_a_the_broken_world_in_the_three_modes_and_twice(ctx, broken):
    _, _, st = broken
    mp = _map_of(ctx, st)
    blob = mp.export_state()
    _, dry, _ = _join(ctx, mp, st, 1, 0, "(a) dry run", mode=capi.FX_JOIN_DRY_RUN)
    assert dry["flags"] == F and mp.export_state() == blob
    new, res, match = _join(ctx, mp, st, 1, 0, "(a) fit")
    assert res["flags"] == A | F and res["n_inliers"] >= 3 and new["header"]["segments"] == 1
    joined = mp.export_state()
    _join(ctx, mp, new, 1, 0, "(a) joined already")  # BAD_SEGMENT: one segment is left
    assert mp.export_state() == joined
    # the same call on the same bytes: the same bytes
    mp.import_state(blob)
    _join(ctx, mp, st, 1, 0, "(a) again")
    assert mp.export_state() == joined
    # GIVEN the fitted T: the same map
    mp.import_state(blob)
    T = tuple(float(res[k]) for k in ("c", "s", "tx", "ty", "tz"))
    given, _, _ = _join(ctx, mp, st, 1, 0, "(a) given", prior=T, mode=capi.FX_JOIN_GIVEN)
    assert mp.export_state() == joined
    # the other direction: dst's landmarks move, the label is the same
    mp.import_state(blob)
    _, back, _ = _join(ctx, mp, st, 0, 1, "(a) 0 into 1")
    assert back["flags"] == A | F and back["label"] == 0
    mp.close()


def test_b_after_a_join_the_run_goes_on(ctx):
    """Update with overlap, merge, compact, localize with the new label, export / import into a second map."""
    f = ju.WORLD
    w, pieces, _ = ju.world(bad=17)
    st, _, _ = mu.run_reference(pieces[:-1], f["cap"], f["carry"])
    mp = _map_of(ctx, st)
    b = 17
    yaw = w["truth"][b + 1][0] - w["truth"][b][0]
    st, res, _ = _join(ctx, mp, st, 1, 0, "(b) join", prior=(math.cos(yaw), math.sin(yaw), 0.0, 0.0, 0.0), search_dist=8.0)
    assert res["flags"] & A and st["header"]["segments"] == 1
    other = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    dst = other.map_create(f["cap"] + 5, f["carry"] + 1)
    dst.import_state(mp.export_state())
    p = pieces[-1]
    outs = []
    for c, m in ((ctx, mp), (other, dst)):
        s = dict(st, max_landmarks=m.max_landmarks, max_carry_rows=m.max_carry_rows)
        s, tr, ids = _step(c, m, s, p, True, "(b) the next batch")
        assert s["header"]["last_joined"] > 0 and not s["header"]["flags"] & capi.FX_MAP_OVERLAP_MISMATCH
        s, _ = _merge_to_fixpoint(c, m, s, "(b) merge", max_calls=8)
        assert any(a >= 0 for a in s["alias"]), "the twins of the two segments are merged"
        got, ref = _localize(c, m, s, p["off"], p["rows"], tr["poses"], "(b) localize", segment=0)
        assert (ref["rec"]["flags"] & capi.FX_LOC_VALID).all()
        s, _, _ = _compact(c, m, s, "(b) compact")
        _same_state(m, s, "(b) at the end")
        outs.append(m.export_state()[64:])  # (behind the block header: the two maps differ in nothing it does not size)
    assert outs[0] == outs[1]
    mp.close(), dst.close(), other.close()


@pytest.mark.parametrize("n", [255, 256, 257])
def test_c_interleaved_ids_across_the_workgroups_edge(ctx, n):
    st = ju.two_segments(n // 2, n - n // 2, jitter=0.01)
    assert len(st["landmarks"]) == n
    mp = _map_of(ctx, st)
    new, res, match = _join(ctx, mp, st, 1, 0, f"(c) {n}")
    assert res["flags"] == A | F and res["n_src"] == n // 2 == res["n_corr"] == res["moved"] and (match >= 0).sum() == res["n_inliers"] == n // 2
    mp.close()


@pytest.mark.parametrize("n_src,flags", [(1024, A | F), (1025, A | F | T_)])
def test_d_1024_and_1025_correspondences(ctx, n_src, flags):
    st = ju.two_segments(n_src, 1030, pitch=6.0, jitter=0.01)
    mp = _map_of(ctx, st)
    new, res, match = _join(ctx, mp, st, 1, 0, f"(d) {n_src}")
    assert res["flags"] == flags and res["n_src"] == n_src == res["moved"] and res["n_corr"] == 1024
    mp.close()


def test_e_absorbed_nan_few_observations_and_the_id_tie(ctx):
    st = ju.two_segments(12, 12, jitter=0.01)
    lms = st["landmarks"]
    src = [i for i, r in enumerate(lms) if r["segment"] == 1]
    dst = [i for i, r in enumerate(lms) if r["segment"] == 0]
    st["alias"] = [-1] * len(lms)
    st["alias"][src[1]] = src[0]        # an absorbed landmark of src: no query, but it moves
    st["alias"][dst[2]] = dst[0]        # an absorbed target: query src[2] finds nothing
    lms[src[3]]["x"] = float("nan")     # records that are not finite: no query, no target (their sums are: they move)
    lms[dst[4]]["z"] = float("inf")
    lms[src[5]]["n_obs"] = 1            # below min_landmark_obs = 2
    lms[dst[6]]["n_obs"] = 1
    # a query with two equidistant targets: dst[8] laid as the mirror image of dst[7] about query src[7]
    q, t = lms[src[7]], lms[dst[7]]
    mirror = dict(lms[dst[8]], x=2.0 * q["x"] - t["x"], y=2.0 * q["y"] - t["y"])
    assert (mirror["x"] - q["x"], mirror["y"] - q["y"]) == (q["x"] - t["x"], q["y"] - t["y"]), "exactly as far"
    lms[dst[8]] = mirror
    mp = _map_of(ctx, st)
    _, dry, match = _join(ctx, mp, st, 1, 0, "(e) dry", mode=capi.FX_JOIN_DRY_RUN)
    assert dry["n_src"] == 12 - 3 and match[src[7]] == dst[7] < dst[8] and all(match[src[k]] == -1 for k in (1, 2, 3, 5))
    _, one, _ = _join(ctx, mp, st, 1, 0, "(e) min_landmark_obs 1", mode=capi.FX_JOIN_DRY_RUN, min_landmark_obs=1)
    assert one["n_src"] == dry["n_src"] + 1 and one["n_corr"] == dry["n_corr"] + 2
    new, res, _ = _join(ctx, mp, st, 1, 0, "(e) fit")
    assert res["flags"] == A | F and res["moved"] == 12 and math.isfinite(new["landmarks"][src[3]]["x"])
    mp.close()


@pytest.mark.parametrize("src,dst", [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)])
def test_f_three_segments(ctx, src, dst):
    from tests.test_map_join_reference import _three
    st = _three()
    mp = _map_of(ctx, st)
    new, res, _ = _join(ctx, mp, st, src, dst, f"(f) {src} into {dst}", prior=(0.6, 0.8, 10.0, -20.0, 0.25), mode=capi.FX_JOIN_GIVEN)
    assert res["flags"] == A and res["moved"] == 3 and res["segments"] == 2
    new, res, _ = _join(ctx, mp, new, 1, 0, "(f) and the two that are left", mode=capi.FX_JOIN_GIVEN)
    assert res["segments"] == 1 and all(r["segment"] == 0 for r in new["landmarks"])
    mp.close()


def test_g_a_device_prior_from_a_localization(ctx, broken):
    """Scan BAD + 1 localised against segment 0 under its held pose: the record's D, read on the device, is the join's prior."""
    import torch
    w, pieces, st = broken
    b = ju.WORLD["bad"]
    mp = _map_of(ctx, st)
    off, rows = lu.scans([[tuple(r[:3]) for r in w["rows"][int(w["off"][b + 1]):int(w["off"][b + 2])]]])
    t = w["truth"][b]
    held = lu.identity(1, c=math.cos(t[0]), s=math.sin(t[0]), tx=t[1], ty=t[2], tz=t[3])
    opts = dict(search_dist=8.0, segment=0)
    kp, pri = __import__("tests.test_gpu_map_localize", fromlist=["_device"])._device(ctx, off, rows, held, 3, len(rows) + 9)
    recs, _, _ = mp.localize(kp, pri, 1, q_max_rows=len(rows), **opts)
    ctx.synchronize()
    loc = capi.localize_records(recs)
    assert loc["flags"][0] & capi.FX_LOC_VALID
    D = tuple(float(loc[k][0]) for k in ("dc", "ds", "dtx", "dty", "dtz"))
    d_ptr = recs.data_ptr() + capi.LOC_DTYPE.fields["dc"][1]
    new, res, _ = _join(ctx, mp, st, 1, 0, "(g) the prior on the device", prior_device=d_ptr, prior_ref=D, search_dist=0.5)
    assert res["flags"] == A | F and res["n_inliers"] > 4, "under D every twin is in reach, not only those about the centre"
    # a device prior that is not finite: reported, nothing changed
    bad = torch.tensor([1.0, 0.0, float("nan"), 0.0, 0.0], dtype=torch.float64, device=f"cuda:{ctx.device}")
    _, res, _ = _join(ctx, mp, new, 0, 0 + 5, "(g) NaN and a segment that is not there", prior_device=bad, prior_ref=(1.0, 0.0, float("nan"), 0.0, 0.0))
    assert res["flags"] == BP | BS
    mp.close()


def test_h_host_refusals_touch_nothing(ctx, fxlib, broken):
    import torch
    _, _, st = broken
    mp = _map_of(ctx, st)
    other = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    blob = mp.export_state()
    dev = f"cuda:{ctx.device}"
    res = torch.full((REC_WORDS + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    match = torch.full((mp.max_landmarks + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    pd = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev)
    P = C.c_void_p
    r, m = res.data_ptr() + 4 * GUARD, match.data_ptr() + 4 * GUARD

    def opt(**kw):
        o = capi.FxMapJoinOptions()
        fxlib.fx_map_join_options_default(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    nan = capi.FxPose(1.0, 0.0, float("nan"), 0.0, 0.0, 0, 0)
    ok = capi.FxPose(1.0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    cases = [("null ctx", (None, mp.handle, 1, 0, None, None, None, P(r), P(m)), b"null"),
             ("null map", (ctx.handle, None, 1, 0, None, None, None, P(r), P(m)), b"null"),
             ("another context's map", (other.handle, mp.handle, 1, 0, None, None, None, P(r), P(m)), b"another context"),
             ("src == dst", (ctx.handle, mp.handle, 1, 1, None, None, None, P(r), P(m)), b"differ"),
             ("both priors", (ctx.handle, mp.handle, 1, 0, C.byref(ok), P(pd.data_ptr()), None, P(r), P(m)), b"not both"),
             ("prior_host not finite", (ctx.handle, mp.handle, 1, 0, C.byref(nan), None, None, P(r), P(m)), b"finite"),
             ("search_dist", (ctx.handle, mp.handle, 1, 0, None, None, opt(search_dist=0.0), P(r), P(m)), b"search_dist"),
             ("inlier_dist", (ctx.handle, mp.handle, 1, 0, None, None, opt(inlier_dist=float("inf")), P(r), P(m)), b"inlier_dist"),
             ("min_baseline", (ctx.handle, mp.handle, 1, 0, None, None, opt(min_baseline=-1.0), P(r), P(m)), b"min_baseline"),
             ("hyp_corr 1", (ctx.handle, mp.handle, 1, 0, None, None, opt(hyp_corr=1), P(r), P(m)), b"hyp_corr"),
             ("hyp_corr 129", (ctx.handle, mp.handle, 1, 0, None, None, opt(hyp_corr=129), P(r), P(m)), b"hyp_corr"),
             ("min_inliers", (ctx.handle, mp.handle, 1, 0, None, None, opt(min_inliers=1), P(r), P(m)), b"min_inliers"),
             ("min_landmark_obs", (ctx.handle, mp.handle, 1, 0, None, None, opt(min_landmark_obs=0), P(r), P(m)), b"min_landmark_obs"),
             ("mode", (ctx.handle, mp.handle, 1, 0, None, None, opt(mode=3), P(r), P(m)), b"mode"),
             ("reserved", (ctx.handle, mp.handle, 1, 0, None, None, opt(reserved=1), P(r), P(m)), b"reserved"),
             ("prior_device alignment", (ctx.handle, mp.handle, 1, 0, None, P(pd.data_ptr() + 4), None, P(r), P(m)), b"aligned"),
             ("result alignment", (ctx.handle, mp.handle, 1, 0, None, None, None, P(r + 4), P(m)), b"aligned"),
             ("match alignment", (ctx.handle, mp.handle, 1, 0, None, None, None, P(r), P(m + 2)), b"aligned")]
    for name, args, word in cases:
        assert fxlib.fx_map_join_segments(*args) == capi.FX_ERR_INVALID_ARG and word in fxlib.fx_last_error(), (name, fxlib.fx_last_error())
    ctx.synchronize()
    assert (res == FILL).all().item() and (match == FILL).all().item() and mp.export_state() == blob
    # NULL outputs are no refusal
    new, _, _ = capi.map_join_reference(st, 1, 0)
    assert mp.join_segments(1, 0, result=False, match=False) == (None, None)
    _same_state(mp, new, "(h) without outputs")
    mp.close(), other.close()
