"""fx_map_merge, the part that needs no GPU: the C-ABI's new names, and capi.map_merge_reference — the executable statement of
include/fx.h's definition — held to what the call exists for: under detector flicker the map ends with ONE live landmark a pole,
holding every observation of the pole's tracks, and a map that is updated after a merge continues the merged landmarks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_merge_util as mm
from tests import map_util as mu
from tests import track_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABS, MRG, CONT = capi.FX_MAP_LM_ABSORBED, capi.FX_MAP_LM_MERGED, capi.FX_MAP_LM_CONTINUED


def test_names_declared_exported_and_listed(fxlib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fx.h")).read(), flags=re.S)
    for n in ("fx_map_merge_options", "fx_map_merge_result"):
        assert re.search(r"typedef struct %s\s*\{[^}]*\}\s*%s;" % (n, n), src), n
    for n in ("fx_map_merge_options_default", "fx_map_merge", "fx_map_get_alias", "fx_map_read_alias"):
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(fxlib, n) and n in capi.EXPORTS, n
    assert "#define FX_VERSION_MINOR 7" in src and fxlib.fx_version() == 7  # added symbols only
    assert re.search(r"#define FX_MAP_LM_ABSORBED 0x2u", src) and re.search(r"#define FX_MAP_LM_MERGED\s+0x4u", src)
    assert C.sizeof(capi.FxMapMergeOptions) == 8 and C.sizeof(capi.FxMapMergeResult) == 16 and C.sizeof(capi.FxMapLandmark) == 48 and C.sizeof(capi.FxMapHeader) == 88
    o = capi.FxMapMergeOptions()
    fxlib.fx_map_merge_options_default(C.byref(o))
    assert o.merge_dist == np.float32(0.30) and o.max_gap_scans == 64
    r = capi.FxRegisterOptions()
    fxlib.fx_register_options_default(C.byref(r))
    assert o.merge_dist == r.inlier_dist


@pytest.fixture(scope="module")
def world():
    w, pieces, poles = mm.flicker()
    whole = tu.reference(w)
    return w, pieces, poles, whole


def _world_points(w, whole):
    """The world-frame point of every row, fp64, in fx_track_landmarks's operation order."""
    P, off = whole["poses"], [int(x) for x in w["off"]]
    b = np.repeat(np.arange(len(off) - 1), np.diff(off))
    x, y, z = (w["rows"][:, k].astype(np.float64) for k in range(3))
    return np.stack([(P["c"][b] * x - P["s"][b] * y) + P["tx"][b], (P["s"][b] * x + P["c"][b] * y) + P["ty"][b], z + P["tz"][b]], axis=1)


def _check_one_landmark_a_pole(w, whole, st, row_ids_by_piece, pieces, what):
    """The checks of the flicker world on a merged state."""
    runs = mm.long_runs(w)
    L, alias = capi.map_state_records(st)["landmarks"], np.array(st["alias"], np.int32)
    live = np.flatnonzero(alias == -1)
    assert len(live) == len(runs), f"{what}: {len(live)} live landmarks, {len(runs)} poles with a track"
    absorbed = np.flatnonzero(alias >= 0)
    assert (alias[alias[absorbed]] == -1).all() and ((L["flags"][absorbed] & ABS) != 0).all() and not (L["flags"][live] & ABS).any(), what
    # rows -> live id -> one pole
    pole_of = {}
    for p, ids in zip(pieces, row_ids_by_piece):
        res = mm.resolve(ids[:len(p["rows"])], alias)
        for r in np.flatnonzero(res >= 0):
            pole_of.setdefault(int(res[r]), set()).add(int(w["pole"][p["row0"] + r]))
    assert set(pole_of) == set(live.tolist()) and all(len(v) == 1 for v in pole_of.values()), what
    W = _world_points(w, whole)
    worst = [0.0, 0.0]
    for lid, ks in pole_of.items():
        rows = runs[next(iter(ks))]
        n = len(rows)
        assert L["n_obs"][lid] == n, (what, lid, L["n_obs"][lid], n)
        for k, f in enumerate(("x", "y", "z")):
            s = 0.0
            for v in W[rows, k].tolist():  # the sequential fp64 mean
                s += v
            # two association orders of the same n terms differ by at most 2 (n - 1) 2^-53 sum |w_i|; divided by n
            bound = 2 * (n - 1) * 2.0 ** -53 * np.abs(W[rows, k]).sum() / n
            err = abs(L[f][lid] - s / n)
            worst[0] = max(worst[0], err / bound if bound else 0.0)
            assert err <= bound, (what, lid, f, err, bound)
        # rms_xy against a two-pass value: tests/test_map_reference.py's bound
        wx, wy = W[rows, 0], W[rows, 1]
        ref = np.sqrt(np.mean((wx - wx.mean()) ** 2 + (wy - wy.mean()) ** 2))
        bound = 4 * float(np.spacing(np.float32(ref))) + 2.0 ** -46 * max(np.abs(wx).max(), np.abs(wy).max())
        err = abs(float(L["rms_xy"][lid]) - ref)
        worst[1] = max(worst[1], err / bound)
        assert err <= bound, (what, lid, err, bound)
    print(f"{what}: {len(L)} landmarks -> {len(live)} live; worst mean error {worst[0]:.3f} of its bound, worst rms_xy error {worst[1]:.3f} of its bound")


def test_flicker_world_one_live_landmark_a_pole(world):
    w, pieces, poles, whole = world
    d = np.hypot(*(poles[:, None, :] - poles[None, :, :]).transpose(2, 0, 1))
    assert d[np.triu_indices(len(poles), 1)].min() >= 3.26 > 2 * 0.30
    f = mm.FLICKER
    st, _, ids = mu.run_reference(pieces, f["cap"], f["carry"])
    assert st["header"]["n_landmarks"] == 54 == st["header"]["n_needed"] and len(set(int(k) for k in w["pole"])) == 35
    before = capi.map_state_records(st)
    merged, results = mm.merge_to_fixpoint(st, max_gap_scans=24)
    assert len(results) <= mm.MAX_CALLS and results[-1]["merged"] == 0 and results[-1]["proposals"] == 0
    print("calls:", results)
    assert results[0]["merged"] > 0 and sum(r["merged"] for r in results) == 54 - results[-1]["live"]
    assert mm.state_bytes(st) and capi.map_state_records(st)["landmarks"].tobytes() == before["landmarks"].tobytes() and "alias" not in st  # (not modified)
    assert merged["header"] == st["header"]  # ids are stable, the header is untouched
    _check_one_landmark_a_pole(w, whole, merged, ids, pieces, "flicker")
    # a root keeps first_scan, segment and anchor; absorbed records are frozen but for the flag
    L0, L1 = before["landmarks"], capi.map_state_records(merged)["landmarks"]
    alias = np.array(merged["alias"])
    for i in range(len(L0)):
        if alias[i] >= 0:
            a, b = L0[i].copy(), L1[i].copy()
            assert b["flags"] == a["flags"] | ABS
            b["flags"] = a["flags"]
            assert a.tobytes() == b.tobytes() and merged["acc"][i] == st["acc"][i]
        else:
            assert all(L0[k][i] == L1[k][i] for k in ("first_scan", "segment")) and merged["acc"][i][3:5] == st["acc"][i][3:5]
            assert bool(L1["flags"][i] & MRG) == bool((alias == i).any())


@pytest.mark.parametrize("k", [1, 3])
def test_update_after_merge_continues_the_roots(world, k):
    w, pieces, poles, whole = world
    f = mm.FLICKER
    st = capi.map_state(f["cap"], f["carry"])
    ids, frozen = [], None
    for j, p in enumerate(pieces):
        tr = tu.reference(p, init_pose=st["header"]["last_pose"][:5])
        st, row_ids = capi.map_reference(st, p["off"], p["rows"], tr, overlap=j > 0)
        ids.append(row_ids)
        if frozen is not None:
            alias = np.array(frozen[0] + [-1] * (len(st["landmarks"]) - len(frozen[0])))
            assert st["alias"] == frozen[0], "fx_map_update never touches the alias table"
            assert (alias[row_ids[row_ids >= 0]] == -1).all(), "a row of a later batch reports an absorbed id"
            L = capi.map_state_records(st)["landmarks"]
            assert L[:len(frozen[1])][alias[:len(frozen[1])] >= 0].tobytes() == frozen[1][alias[:len(frozen[1])] >= 0].tobytes(), "an absorbed record changed"
        if j == k:
            unmerged_carry = list(st["carry"])
            st, results = mm.merge_to_fixpoint(st, max_gap_scans=24)
            assert results[0]["merged"] > 0
            a = st["alias"]
            assert st["carry"] == [c if c < 0 or a[c] < 0 else a[c] for c in unmerged_carry] and all(c < 0 or a[c] == -1 for c in st["carry"])
            frozen = (list(a), capi.map_state_records(st)["landmarks"])
    assert (capi.map_state_records(st)["landmarks"]["flags"] & (MRG | CONT) == (MRG | CONT)).any()  # a merged root that was continued
    st, _ = mm.merge_to_fixpoint(st, max_gap_scans=24)
    _check_one_landmark_a_pole(w, whole, st, ids, pieces, f"merge after piece {k}, then at the end")


def _merge(frags, n_scans, bad=(), **kw):
    w = mm.fragments(frags, n_scans, bad)
    st, lm = mm.reference_of(w)
    out, res = capi.map_merge_reference(st, **kw)
    return st, out, res, lm


NEXT = float(np.nextafter(np.float32(0.25), np.float32(1.0)))


def test_hand_the_distance_gate_is_inclusive():
    for x, merges in ((0.25, True), (NEXT, False)):
        _, out, res, (a, b) = _merge([(0, 0.0, 2.0), (3, x, 2.0)], 5, merge_dist=0.25)
        assert (res["merged"], res["proposals"], res["live"]) == ((1, 1, 1) if merges else (0, 0, 2)), (x, res)
        assert out["alias"] == ([-1, a] if merges else [-1, -1])
    # the gate is the float the options hold, taken to double: 0.3 is float32(0.3), which is above 0.3
    _, out, res, _ = _merge([(0, 0.0, 2.0), (3, float(np.float32(0.3)), 2.0)], 5, merge_dist=0.3)
    assert res["merged"] == 1


def test_hand_the_gap_gate_segments_and_touching_ranges():
    frags = [(0, 1.0, 1.0), (7, 1.0, 1.0)]  # last_scan 1, first_scan 7
    assert _merge(frags, 9, max_gap_scans=6)[2]["merged"] == 1
    assert _merge(frags, 9, max_gap_scans=5)[2]["merged"] == 0
    st, out, res, lm = _merge(frags, 9, bad=(4,), max_gap_scans=64)  # a bad link in between: two segments
    L = capi.map_state_records(st)["landmarks"]
    assert L["segment"].tolist() == [0, 1] and res["merged"] == 0 and res["live"] == 2
    st, out, res, lm = _merge([(0, 1.0, 1.0), (1, 1.0, 1.0), (2, 1.0, 1.0)], 4)  # scans 0-1, 1-2, 2-3: only the outer two are disjoint
    assert res["merged"] == 1 and out["alias"] == [-1, -1, 0]


def test_hand_proposal_order_most_recent_then_nearest_then_lowest_id():
    # the older one is nearer: the more recent one is proposed (the two are too far apart to merge themselves)
    st, out, res, (old, new, h) = _merge([(0, -0.25, 0.0), (2, 0.25, 0.0), (5, -0.125, 0.0)], 7, merge_dist=0.375)
    assert out["alias"][h] == new and out["alias"][old] == -1 and res["merged"] == 1
    # equal last_scan: the nearer one, whatever its id
    st, out, res, (g1, g2, h) = _merge([(0, 0.125, 0.0), (0, -0.0625, 0.0), (3, 0.0, 0.0)], 5)
    assert g1 < g2 and out["alias"][h] == g2
    # equal last_scan and equal d2: the lower id
    st, out, res, (g1, g2, h) = _merge([(0, 0.125, 0.0), (0, -0.125, 0.0), (3, 0.0, 0.0)], 5)
    assert g1 < g2 and out["alias"][h] == g1 and res["proposals"] == 1


def test_hand_acceptance_lowest_first_scan_then_lowest_id_and_the_loser_merges_next_call():
    # two proposers of one first_scan: the lower id is kept; the other was seen in the same scans and stays live for good
    st, out, res, (g, h1, h2) = _merge([(0, 0.0, 0.0), (3, 0.25, 0.0), (3, -0.25, 0.0)], 5, merge_dist=0.375)
    assert h1 < h2 and res["proposals"] == 2 and res["merged"] == 1 and out["alias"] == [-1, g, -1]
    assert capi.map_merge_reference(out, merge_dist=0.375)[1]["merged"] == 0
    # the later proposer loses, and merges on the second call: g = 0, h1 = 0.25, h2 = -0.3125 (h1 and h2 0.5625 apart)
    st, out, res, (g, h1, h2) = _merge([(0, 0.0, 0.0), (3, 0.25, 0.0), (6, -0.3125, 0.0)], 8, merge_dist=0.5)
    assert res["proposals"] == 2 and res["merged"] == 1 and res["live"] == 2 and out["alias"] == [-1, g, -1]
    assert out["landmarks"][g]["x"] == 0.125 and out["landmarks"][g]["last_scan"] == 4
    out2, res2 = capi.map_merge_reference(out, merge_dist=0.5)
    assert res2["merged"] == 1 and res2["live"] == 1 and out2["alias"] == [-1, g, g] and out2["landmarks"][g]["n_obs"] == 6
    assert out2["landmarks"][g]["x"] == (0.0 + 0.0 + 0.25 + 0.25 - 0.3125 - 0.3125) / 6


def test_hand_three_fragments_fold_as_one_chain_in_order_and_a_fixpoint_is_stable():
    xs = [float(np.float32(v)) for v in (10.01, 10.07, 9.96)]
    ys = [float(np.float32(v)) for v in (-3.02, -3.11, -2.95)]
    st, out, res, (a, b, c) = _merge([(0, xs[0], ys[0]), (3, xs[1], ys[1]), (6, xs[2], ys[2])], 8)
    assert (res["proposals"], res["merged"], res["live"]) == (2, 2, 1) and out["alias"] == [-1, a, a]
    A = list(st["acc"][a])
    for m in (b, c):  # the fold of include/fx.h, A then B then C
        B, nm = st["acc"][m], 2.0
        ex, ey = B[3] - A[3], B[4] - A[4]
        A[0], A[1], A[2] = A[0] + B[0], A[1] + B[1], A[2] + B[2]
        A[7] += ((B[7] + 2.0 * (ex * B[5] + ey * B[6])) + nm * (ex * ex + ey * ey))
        A[5], A[6] = A[5] + (B[5] + nm * ex), A[6] + (B[6] + nm * ey)
    assert [v.hex() for v in out["acc"][a]] == [v.hex() for v in A]
    R = out["landmarks"][a]
    assert R["n_obs"] == 6 and R["last_scan"] == 7 and R["first_scan"] == 0 and R["flags"] == MRG and R["x"] == A[0] / 6.0
    # the spread about the mean of six points, two at each place
    ref = np.sqrt(np.mean((np.repeat(xs, 2) - np.mean(np.repeat(xs, 2))) ** 2 + (np.repeat(ys, 2) - np.mean(np.repeat(ys, 2))) ** 2))
    assert abs(float(R["rms_xy"]) - ref) <= 4 * float(np.spacing(np.float32(ref))) + 2.0 ** -46 * 10.07
    again, res2 = capi.map_merge_reference(out)
    assert res2 == {"proposals": 0, "merged": 0, "live": 1, "reserved": 0} and mm.state_bytes(again) == mm.state_bytes(out)


def test_refusals_of_the_reference():
    st = capi.map_state(4, 4)
    for kw in (dict(merge_dist=0.0), dict(merge_dist=float("nan")), dict(merge_dist=float("inf")), dict(merge_dist=-1.0), dict(max_gap_scans=0)):
        with pytest.raises(ValueError):
            capi.map_merge_reference(st, **kw)
    out, res = capi.map_merge_reference(st)
    assert res == {"proposals": 0, "merged": 0, "live": 0, "reserved": 0} and out["alias"] == []
