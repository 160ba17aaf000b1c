"""fx_map_find_loop on the GPU.  Every call is compared with capi.map_find_loop_reference — an all-pairs statement of
include/fx.h's definition in numpy float64 that knows nothing of the grids — bit for bit: the result record (doubles as bit
patterns) and all max_landmarks words of match_of_landmark; the map's snapshot must be what it was and the guard words about the
outputs untouched.  The chained calls (fx_map_close_loop, fx_map_join_segments with the result as prior_device) are held to their
own references under the reference's transform."""
import ctypes as C
import math

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_find_loop_util as fu
from tests import map_join_util as ju
from tests import map_localize_util as llu
from tests import map_loop_util as lu
from tests import map_relocalize_util as ru
from tests import map_util as mu
from tests.test_gpu_map_compact import _compact, _same_state
from tests.test_gpu_map_join import _join
from tests.test_gpu_map_loop import _close
from tests.test_gpu_map_merge import _merge_to_fixpoint
from tests.test_gpu_track import FILL, GUARD

pytestmark = pytest.mark.gpu
REC_WORDS = capi.FIND_DTYPE.itemsize // 4
NAN5 = (float("nan"),) * 5


@pytest.fixture
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def _map_of(ctx, st):
    mp = ctx.map_create(st["max_landmarks"], st["max_carry_rows"])
    mp.import_state(capi.map_snapshot_pack(st))
    return mp


def _find(ctx, mp, st, what, keep=None, **opts):
    """One fx_map_find_loop into guarded outputs against one map_find_loop_reference call; the map's snapshot stays.  keep: a dict
    that receives the device's result tensor and the output bytes.  Returns the reference's {"rec", "match_of_landmark", "hyp"}."""
    import torch
    dev, cap = f"cuda:{ctx.device}", mp.max_landmarks
    res = torch.full((GUARD + REC_WORDS + GUARD,), FILL, dtype=torch.int32, device=dev)
    match = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.int32, device=dev)
    assert GUARD % 2 == 0
    before = mp.export_state()
    mp.find_loop(result=res[GUARD:GUARD + REC_WORDS], match=match[GUARD:GUARD + cap], **opts)
    ctx.synchronize()
    for t, n, name in ((res, REC_WORDS, "the result"), (match, cap, "match_of_landmark")):
        assert (t[:GUARD] == FILL).all().item() and (t[GUARD + n:] == FILL).all().item(), f"{what}: the guards about {name}"
    ref = capi.map_find_loop_reference(st, **opts)
    fu.assert_result(capi.find_loop_records(res[GUARD:GUARD + REC_WORDS]), ref["rec"], what)
    got = match[GUARD:GUARD + cap].cpu().numpy()
    bad = np.flatnonzero(got != ref["match_of_landmark"])
    assert not len(bad), f"{what}: match_of_landmark differs at {bad[:8].tolist()}: got {got[bad[:8]]}, reference {ref['match_of_landmark'][bad[:8]]}"
    assert mp.export_state() == before, f"{what}: the map was written"
    if keep is not None:
        keep["result"] = res[GUARD:GUARD + REC_WORDS]
        keep["bytes"] = res.cpu().numpy().tobytes() + match.cpu().numpy().tobytes()
    return ref


def _hand(ctx, st, what, **opts):
    mp = _map_of(ctx, st)
    ref = _find(ctx, mp, st, what, **opts)
    mp.close()
    return ref["rec"], ref["match_of_landmark"]


# ---- (1) the loop worlds and the chains
@pytest.fixture(scope="module")
def worlds():
    return {b: fu.world(b) for b in fu.BIASES}


@pytest.mark.parametrize("bias", fu.BIASES)
def test_a_the_loop_worlds(ctx, worlds, bias):
    st, _ = worlds[bias]
    mp = _map_of(ctx, st)
    rec = _find(ctx, mp, st, f"(a) {bias}", **lu.OPTS)["rec"]
    assert rec["flags"] == fu.VALID and rec["score"] >= 35 and int(rec["score"]) - int(rec["runner_up"]) >= 10
    mp.close()


def test_a_find_then_close_then_merge_and_compact_with_no_host_read(ctx, worlds):
    st, pole = worlds[fu.BIASES[1]]
    mp = _map_of(ctx, st)
    keep = {}
    ref = _find(ctx, mp, st, "(a) find", keep=keep, **lu.OPTS)
    T = fu.transform_of(ref["rec"])
    st, res, match = _close(ctx, mp, st, "(a) close on the result", prior_device=keep["result"], prior_ref=T, search_dist=0.6, **lu.OPTS)
    assert res["flags"] == capi.FX_LOOP_FITTED | capi.FX_LOOP_APPLIED and res["n_inliers"] >= 35 and lu.spread(st, pole) < 0.30
    st, _ = _merge_to_fixpoint(ctx, mp, st, "(a) merge", max_calls=16, max_gap_scans=lu.WORLD["n_scans"])
    q = np.flatnonzero(match >= 0)
    r = lu.roots(st)
    assert any(r[i] == r[match[i]] for i in q), "twins of the loop's two ends are merged"
    st, _, _ = _compact(ctx, mp, st, "(a) compact")
    _same_state(mp, st, "(a) at the end")
    mp.close()


def test_a_a_loop_that_is_not_found_cannot_move_the_map(ctx, worlds):
    st, _ = worlds[fu.BIASES[1]]
    mp = _map_of(ctx, st)
    blob = mp.export_state()
    keep = {}
    rec = _find(ctx, mp, st, "(a) no seed", keep=keep, max_baseline=2.0, **lu.OPTS)["rec"]
    assert rec["flags"] == fu.NOHYP and rec["n_seeds"] == 0 and fu.head_bits(rec) == [capi.FX_FIND_NAN_BITS] * 5
    _, res, _ = _close(ctx, mp, st, "(a) close on no result", prior_device=keep["result"], prior_ref=NAN5, search_dist=0.6, **lu.OPTS)
    assert res["flags"] == capi.FX_LOOP_BAD_PRIOR and mp.export_state() == blob
    mp.close()


# ---- (2) the windows
def _window_points(last, min_loop, recent):
    base = fu.random_field(14, 3)
    tw = fu.moved(base, 0.4, 30.0, -20.0)
    old = [(x, y, last - min_loop - 9, last - min_loop) for x, y in base[:6]] + [base[6] + (last - min_loop - 9, last - min_loop + 1)]
    rec = [(x, y, last - recent, last) for x, y in tw[:6]] + [tw[6] + (last - recent - 1, last)]
    # neither old nor recent: 32-bit sums of its scans and the windows wrap when `last` is near 2^32
    mid = [base[7] + (last - min_loop + 1, last - 10), tw[7] + (last - min_loop + 1, last - 10)]
    return old + rec + mid


@pytest.mark.parametrize("last", [400, 0xfffffffe])
def test_b_window_edges(ctx, last):
    """last_scan + min_loop_scans == last is a target and one scan later is not; first_scan + recent_scans == last is a query and
    one scan earlier is not; near 2^32 the sums need 64 bits."""
    st = fu.state(_window_points(last, 256, 100))
    rec, match = _hand(ctx, st, f"(b) last {last:#x}", recent_scans=100)
    assert (rec["n_targets"], rec["n_query"], rec["score"], rec["flags"]) == (6, 6, 6, fu.VALID)
    assert np.flatnonzero(match >= 0).tolist() == list(range(7, 13)) and match[7:13].tolist() == list(range(6))


def test_b_the_whole_segment_as_queries(ctx):
    pts = _window_points(400, 256, 100)
    st = fu.state([p + (0 if k < 7 or k == 14 else 1,) for k, p in enumerate(pts)])
    rec, _ = _hand(ctx, st, "(b) recent_scans 32", segment=1, target_segment=0)
    assert (rec["n_targets"], rec["n_query"]) == (8, 0) and rec["flags"] == fu.NOHYP
    rec, _ = _hand(ctx, st, "(b) recent_scans 0xffffffff", segment=1, target_segment=0, recent_scans=0xffffffff)
    assert (rec["n_targets"], rec["n_query"], rec["score"], rec["flags"]) == (8, 8, 8, fu.VALID)


# ---- (3) the query cut
def _laced(n_twins, n_base=70, seed=4):
    base = fu.random_field(n_base, seed)
    tw = fu.moved(base, -0.3, 5.0, 80.0)
    pts = []
    for k in range(n_base):
        pts.append(base[k] + fu.OLD)
        if k < n_twins:
            pts.append(tw[k] + fu.RECENT)
    st = fu.state(pts)
    st["header"]["scans"] = fu.LAST_SCAN + 1  # (without a recent landmark too)
    return st


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65])
def test_c_the_query_cut(ctx, n):
    rec, match = _hand(ctx, _laced(n), f"(c) {n} candidate queries", max_baseline=200.0)
    want = fu.NOHYP if n < 2 else 0 if n == 2 else fu.VALID | (fu.TRUNC if n > 64 else 0)  # (a score of 2 is below min_inliers)
    assert (rec["n_query"], rec["n_targets"], rec["flags"]) == (min(n, 64), 70, want)
    if n >= 2:
        assert rec["score"] == min(n, 64)
        assert np.flatnonzero(match >= 0).tolist() == ([2 * k + 1 for k in range(n)][-64:] if want & fu.VALID else [])


# ---- (4) the hypothesis kernel's workgroup edges
@pytest.mark.parametrize("n", [255, 256, 257])
@pytest.mark.parametrize("which", ["last", "straddle"])
def test_d_targets_at_the_workgroups_edge(ctx, n, which):
    """255 / 256 / 257 targets.  The hypothesis kernel takes 256 SLOTS of the pair grid a workgroup, and a landmark's slot follows
    the grid's bucket hash, not its id: the grid holds the targets and the queries, so a second workgroup exists at all three sizes,
    and where the winning (g, h) falls among the slots is NOT controlled here.  The queries are twins of the highest ids or of ids
    on both sides of 256, so that the winning pair differs between the runs; a workgroup whose partial was lost or counted twice
    would show in n_hyp and in the winner, which are compared with the all-pairs reference bit for bit."""
    base = fu.random_field(n, 94 + n)
    ids = [n - 1, n - 2, n - 3, n - 5, n - 8] if which == "last" else [0, 100, 254, n - 1, n - 2, 200, 101]
    tw = fu.moved([base[k] for k in ids], 2.0, 120.0, 130.0)
    st = fu.state([p + fu.OLD for p in base] + [p + fu.RECENT for p in tw])
    rec, match = _hand(ctx, st, f"(d) {n} targets, {which}", max_baseline=300.0, max_seeds=8)
    assert rec["flags"] == fu.VALID and rec["score"] == len(ids) and match[n:n + len(ids)].tolist() == ids


# ---- (5) ties
@pytest.mark.parametrize("extra", [False, True])
def test_e_a_lattice_ties_and_one_pole_decides(ctx, extra):
    """Hypotheses of equal score from different seeds and from different (g, h) of one seed: the lowest (s, g, h) wins."""
    st = fu.lattice_case(extra)
    ref = _find(ctx, (mp := _map_of(ctx, st)), st, f"(e) lattice, extra {extra}")
    mp.close()
    rec, h = ref["rec"], ref["hyp"]
    top = np.flatnonzero(h["score"] == h["score"].max())
    assert (rec["flags"], rec["score"], rec["runner_up"]) == ((fu.VALID, 5, 4) if extra else (fu.AMBIG, 4, 4))
    if not extra:
        assert len(set(h["s"][top].tolist())) > 1 and len(top) > len(set(h["s"][top].tolist())), "ties across seeds and within one"
        assert (rec["lm_a"], rec["lm_b"]) == (h["g"][top[0]], h["h"][top[0]]) and fu.head_bits(rec) == [capi.FX_FIND_NAN_BITS] * 5


def test_e_identical_targets_and_two_queries_on_one_target(ctx):
    base = [(0.0, 0.0), (3.0, 4.0), (8.0, 0.0), (8.0, 0.0), (20.0, 5.0)]  # targets 2 and 3 at one xy
    tw = [(x + 50.0, y) for x, y in base[:3]] + [(58.125, 0.0), (70.0, 5.0)]  # queries 2 and 3 both land on target 2
    st = fu.state([p + fu.OLD for p in base] + [p + fu.RECENT for p in tw])
    rec, match = _hand(ctx, st, "(e) identical xy", min_inliers=3)
    assert rec["score"] == 5 and match[5:10].tolist() == [0, 1, 2, 2, 4]


# ---- (6) the gates: fx_map_relocalize's constructions, a scan's rows as the queries
def _from_reloc(frags, rows):
    return fu.state([(x, y) + fu.OLD for _, x, y in frags] + [(x, y) + fu.RECENT for x, y, _ in rows][::-1])  # (query k = row k)


@pytest.mark.parametrize("name", sorted(ru.edge_cases()))
def test_f_gates_at_their_edges(ctx, name):
    frags, rows_by_scan, opts, expect = ru.edge_cases()[name]
    for b, rows in enumerate(rows_by_scan):
        ref = _find(ctx, (mp := _map_of(ctx, st := _from_reloc(frags, rows))), st, f"(f) {name}, scan {b}", **opts)
        mp.close()
        for f, want in expect.items():
            if f == "hyp":
                got = sorted(zip(ref["hyp"]["s"].tolist(), ref["hyp"]["g"].tolist(), ref["hyp"]["h"].tolist()))
                assert got == sorted(want[b]), f"{name}: hypotheses {got}"
            else:
                assert ref["rec"][f] == want[b], f"{name}, scan {b}: {f} {ref['rec'][f]}, expected {want[b]}"


def test_f_the_far_bucket_and_a_crowded_cell(ctx):
    frags = llu.lattice(9, pitch=8.0) + [(0, fu.F32(1e13), fu.F32(-1e13)), (0, fu.F32(1e30), fu.F32(1e30))]
    rec, match = _hand(ctx, _from_reloc(frags, [(x, y, 1.0) for _, x, y in frags]), "(f) the far bucket", min_inliers=3)
    assert rec["score"] == 11 and sorted(match[11:22].tolist()) == list(range(11))
    crowd = [(0, fu.F32(40.0 + 0.01 * (k % 7)), fu.F32(40.0 + 0.01 * (k // 7))) for k in range(49)]  # 49 targets within 7 cm
    frags = llu.lattice(9, pitch=8.0) + crowd
    rows = [(x, y, 1.0) for _, x, y in frags[:9]] + [(40.0, 40.0, 1.0)]
    rec, match = _hand(ctx, _from_reloc(frags, rows), "(f) a crowded cell", min_inliers=3)
    assert rec["score"] == 10 and rec["n_targets"] == 58


# ---- (7) eligibility
def test_g_who_takes_part(ctx):
    """Absorbed landmarks, landmarks of too few observations and those with an x, y or z that is not finite are neither queries nor
    targets; a third segment's landmarks are ignored."""
    base = fu.random_field(10, 11)
    tw = fu.moved(base, 0.25, -12.0, 7.0)
    pts = [p + fu.OLD for p in base] + [p + fu.RECENT for p in tw] + [base[0] + fu.OLD + (1,), tw[0] + fu.RECENT + (1,)]
    st = fu.state(pts, segments=1)  # (segment 0 is the last one by the header: the two of "segment 1" are beyond it)
    st["alias"] = list(st.get("alias", [])) + [-1] * (len(st["landmarks"]) - len(st.get("alias", [])))
    st["alias"][1], st["alias"][11] = 0, 10  # target 1 and query 11 absorbed
    st["landmarks"][2]["n_obs"] = st["landmarks"][12]["n_obs"] = 1
    st["landmarks"][3]["x"], st["landmarks"][13]["y"] = math.inf, math.nan
    st["landmarks"][4]["z"], st["landmarks"][14]["z"] = math.nan, -math.inf
    rec, match = _hand(ctx, st, "(g) eligibility")
    assert (rec["n_targets"], rec["n_query"], rec["score"], rec["flags"]) == (6, 6, 6, fu.VALID)
    assert np.flatnonzero(match >= 0).tolist() == [10, 15, 16, 17, 18, 19]
    rec, _ = _hand(ctx, st, "(g) min_landmark_obs 3", min_landmark_obs=3)
    assert (rec["n_targets"], rec["n_query"], rec["flags"]) == (0, 0, fu.NOHYP)
    three = ju.set_segments(st, [r["segment"] for r in st["landmarks"][:20]] + [2, 2])
    rec, _ = _hand(ctx, three, "(g) a third segment", segment=0)
    assert (rec["n_targets"], rec["n_query"], rec["score"]) == (6, 6, 6)


# ---- (8) two segments
def _displaced(st, seg, yaw, tx, ty):
    """The state with every landmark of segment seg moved by (yaw, tx, ty): sums, anchor and record, as fx_map_join_segments moves."""
    c, s = math.cos(yaw), math.sin(yaw)
    st = dict(st, landmarks=[dict(r) for r in st["landmarks"]], acc=[list(a) for a in st["acc"]])
    for R, A in zip(st["landmarks"], st["acc"]):
        if int(R["segment"]) != seg:
            continue
        n = float(R["n_obs"])
        A[:7] = [(c * A[0] - s * A[1]) + n * tx, (s * A[0] + c * A[1]) + n * ty, A[2], (c * A[3] - s * A[4]) + tx, (s * A[3] + c * A[4]) + ty,
                 c * A[5] - s * A[6], s * A[5] + c * A[6]]
        if int(R["n_obs"]):
            capi._map_record_from_sums(R, A)
    return st


def test_h_find_then_join_with_no_host_read(ctx):
    f = ju.WORLD
    _, pieces, _ = ju.world()
    st, _, _ = mu.run_reference(pieces, f["cap"], f["carry"])
    st = _displaced(st, 1, 0.2, 8.0, -6.0)
    mp = _map_of(ctx, st)
    opts = dict(segment=1, target_segment=0, recent_scans=0xffffffff)
    keep = {}
    rec = _find(ctx, mp, st, "(h) find", keep=keep, **opts)["rec"]
    assert rec["flags"] == fu.VALID and (rec["segment"], rec["target_segment"]) == (1, 0)
    _, plain, _ = capi.map_join_reference(st, 1, 0, mode=capi.FX_JOIN_DRY_RUN)
    assert not plain["flags"] & capi.FX_JOIN_FITTED, "the identity prior joins nothing this far apart"
    new, res, _ = _join(ctx, mp, st, 1, 0, "(h) join on the result", prior_device=keep["result"], prior_ref=fu.transform_of(rec), search_dist=0.6)
    assert res["flags"] == capi.FX_JOIN_APPLIED | capi.FX_JOIN_FITTED and new["header"]["segments"] == 1
    # an explicit target_segment that names the query segment
    for o in (dict(segment=0, target_segment=0), dict(target_segment=capi.FX_LOC_LAST_SEGMENT)):
        rec = _find(ctx, mp, new, f"(h) {o}", **o)["rec"]
        assert rec["flags"] == fu.BADSEG
    mp.close()


# ---- (9) refusals
def test_i_device_refusals(ctx):
    st = fu.lattice_case(True)
    mp = _map_of(ctx, st)
    for o, segs in ((dict(segment=1), (1, 1)), (dict(target_segment=7), (0, 7)), (dict(segment=5, target_segment=0), (5, 0))):
        ref = _find(ctx, mp, st, f"(i) {o}", **o)
        rec = ref["rec"]
        assert rec["flags"] == fu.BADSEG and (rec["segment"], rec["target_segment"]) == segs and (ref["match_of_landmark"] == -1).all()
        assert [int(rec[k]) for k in ("n_hyp", "n_query", "n_targets", "n_seeds", "score", "runner_up")] == [0] * 6
        assert fu.head_bits(rec) == [capi.FX_FIND_NAN_BITS] * 5 and rec["wc"] == 1.0
    mp.close()
    no_scans = dict(st, header=dict(st["header"], scans=0))
    rec, _ = _hand(ctx, no_scans, "(i) a map of no scans")
    assert rec["flags"] == fu.BADSEG and (rec["segment"], rec["target_segment"]) == (0, 0)
    mp = ctx.map_create(8, 8)
    rec = _find(ctx, mp, capi.map_state(8, 8), "(i) an empty map")["rec"]
    assert rec["flags"] == fu.BADSEG and (rec["segment"], rec["target_segment"]) == (fu.NONE, fu.NONE)
    mp.close()


def test_i_host_refusals_touch_nothing(ctx, fxlib):
    import torch
    st = fu.lattice_case(True)
    mp = _map_of(ctx, st)
    other = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    blob = mp.export_state()
    dev = f"cuda:{ctx.device}"
    res = torch.full((REC_WORDS + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    match = torch.full((mp.max_landmarks + 2 * GUARD,), FILL, dtype=torch.int32, device=dev)
    P = C.c_void_p
    r, m = res.data_ptr() + 4 * GUARD, match.data_ptr() + 4 * GUARD

    def opt(**kw):
        o = capi.FxMapFindLoopOptions()
        fxlib.fx_map_find_loop_options_default(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    h, mh = ctx.handle, mp.handle
    ANY = capi.FX_LOC_ANY_SEGMENT
    cases = [("null ctx", (None, mh, None, P(r), P(m)), b"null"),
             ("null map", (h, None, None, P(r), P(m)), b"null"),
             ("null result", (h, mh, None, None, P(m)), b"null"),
             ("another context's map", (other.handle, mh, None, P(r), P(m)), b"another context"),
             ("inlier_dist", (h, mh, opt(inlier_dist=0.0), P(r), P(m)), b"inlier_dist"),
             ("inlier_dist inf", (h, mh, opt(inlier_dist=float("inf")), P(r), P(m)), b"inlier_dist"),
             ("pair_tol", (h, mh, opt(pair_tol=float("nan")), P(r), P(m)), b"pair_tol"),
             ("min_baseline", (h, mh, opt(min_baseline=-1.0), P(r), P(m)), b"min_baseline"),
             ("max_baseline below", (h, mh, opt(max_baseline=1.0), P(r), P(m)), b"max_baseline"),
             ("max_baseline inf", (h, mh, opt(max_baseline=float("inf")), P(r), P(m)), b"max_baseline"),
             ("max_seeds 0", (h, mh, opt(max_seeds=0), P(r), P(m)), b"max_seeds"),
             ("max_seeds 65", (h, mh, opt(max_seeds=65), P(r), P(m)), b"max_seeds"),
             ("min_inliers", (h, mh, opt(min_inliers=2), P(r), P(m)), b"min_inliers"),
             ("min_margin", (h, mh, opt(min_margin=0), P(r), P(m)), b"min_margin"),
             ("min_landmark_obs", (h, mh, opt(min_landmark_obs=0), P(r), P(m)), b"min_landmark_obs"),
             ("any segment", (h, mh, opt(segment=ANY), P(r), P(m)), b"FX_LOC_ANY_SEGMENT"),
             ("any target segment", (h, mh, opt(target_segment=ANY), P(r), P(m)), b"target_segment"),
             ("recent_scans == min_loop_scans", (h, mh, opt(recent_scans=256), P(r), P(m)), b"recent_scans"),
             ("recent_scans above", (h, mh, opt(min_loop_scans=8), P(r), P(m)), b"recent_scans"),
             ("reserved", (h, mh, opt(reserved=1), P(r), P(m)), b"reserved"),
             ("result alignment", (h, mh, None, P(r + 4), P(m)), b"aligned"),
             ("match alignment", (h, mh, None, P(r), P(m + 2)), b"aligned")]
    for name, args, word in cases:
        assert fxlib.fx_map_find_loop(*args) == capi.FX_ERR_INVALID_ARG and word in fxlib.fx_last_error(), (name, fxlib.fx_last_error())
    ctx.synchronize()
    assert (res == FILL).all().item() and (match == FILL).all().item() and mp.export_state() == blob
    # recent_scans >= min_loop_scans is no refusal with another segment's targets, and a NULL match_of_landmark none at all
    assert fxlib.fx_map_find_loop(h, mh, opt(recent_scans=300, target_segment=1), P(r), None) == capi.FX_OK
    ctx.synchronize()
    assert capi.find_loop_records(res[GUARD:GUARD + REC_WORDS])["flags"] == fu.BADSEG and (match == FILL).all().item()
    other.close()
    mp.close()


# ---- (10) the same bytes
def test_j_the_same_call_twice_gives_the_same_bytes(ctx, worlds):
    st, _ = worlds[fu.BIASES[2]]
    mp = _map_of(ctx, st)
    a, b = {}, {}
    _find(ctx, mp, st, "(j) once", keep=a, **lu.OPTS)
    _find(ctx, mp, st, "(j) twice", keep=b, **lu.OPTS)
    assert a["bytes"] == b["bytes"]
    mp.close()
