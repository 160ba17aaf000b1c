"""capi.map_expect_reference and capi.map_retire_reference — the numpy statements of include/fx.h's fx_map_expect and fx_map_retire
that the GPU tests compare the device with bit for bit — held to answers worked out by hand, not to themselves."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_expect_util as eu
from tests import map_localize_util as lu
from tests import map_merge_util as mm
from tests import map_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(c, **over):
    res, e, s = eu.reference(eu.state_of(c), c, **over)
    return res, e.tolist(), s.tolist()


def test_the_header_states_the_constants_the_binding_mirrors():
    src = open(os.path.join(ROOT, "include", "fx.h")).read()
    for name, value in (("FX_EXPECT_WRITE", 0), ("FX_EXPECT_ADD", 1), ("FX_RETIRE_APPLY", 0), ("FX_RETIRE_DRY_RUN", 1)):
        assert re.search(rf"#define {name} {value}u", src) and getattr(capi, name) == value
    assert [C.sizeof(t) for t in (capi.FxMapExpectOptions, capi.FxMapExpectResult, capi.FxMapRetireOptions, capi.FxMapRetireResult)] == [48, 32, 24, 32]
    for size, name in ((48, "fx_map_expect_options"), (32, "fx_map_expect_result"), (24, "fx_map_retire_options"), (32, "fx_map_retire_result")):
        assert re.search(rf"typedef struct {name} \{{\s*/\* {size} B \*/", src), name
    assert re.search(r"#define FX_VERSION_MINOR 7\b", src), "added symbols only"
    assert "fx_map_expect (below) counts" in src and "fx_map_retire (below) runs this same compaction" in src, "the Limits point at the new calls"
    d = capi.EXPECT_DEFAULTS
    assert (d["x_min"], d["x_max"], d["y_min"], d["y_max"], d["min_range"], d["max_range"], d["shadow_width"]) == (1, 74, -29, 29, 2, 60, 0.5)
    assert (d["require_flags"], d["min_landmark_obs"], d["segment"], d["mode"]) == (capi.FX_LOC_VALID, 2, capi.FX_LOC_ANY_SEGMENT, 0)
    assert capi.RETIRE_DEFAULTS == dict(min_expected=16, seen_num=1, seen_den=8, mode=0)


def test_four_landmarks_and_two_scans_by_hand():
    """Landmarks 0 (10, 0), 1 (20, 5), 2 (30, 0), 3 (-10, 0); the default box 1 .. 74 x -29 .. 29, range 2 .. 60, shadow 0.5.
    Scan 0, the identity, one row (10, 0) named 0:
      0 seen; 1 in box, unseen, the row is 50 off its ray (crs = 10 * 5 - 0 * 20): expected; 2 behind the row on the same ray
      (k2 = 100 < 900, along = 300, crs = 0): shadowed; 3 at lx = -10 outside the box: not expected.
    Scan 1, c = 0, s = 1 (lx = dy, ly = -dx), one row (0, -10) named 0:
      0 at (0, -10) outside the box but seen: expected; 1 at (5, -20) in box, crs = 0 * -20 - -10 * 5 = 50: expected; 2 at (0, -30)
      and 3 at (0, 10) outside the box."""
    res, e, s = _counts(eu.hand4())
    assert e == [2, 2, 0, 0] and s == [2, 0, 0, 0]
    assert res == dict(scans_used=2, in_range=8, in_box=4, shadowed=1, expected=4, seen=2, stale=0, landmarks_expected=2)


def test_the_three_gates_of_the_shadow_at_their_edges():
    """tests/map_expect_util.shadow_gates: the landmark (16, 0) is expected in scans 0, 1, 3 and 5 and shadowed in 2 and 4; the far
    landmark at 500 m is out of range throughout."""
    c = eu.shadow_gates()
    res, e, s = _counts(c)
    assert e == [4, 0] and s == [0, 0] and (res["in_range"], res["in_box"], res["shadowed"], res["expected"]) == (6, 6, 2, 4)
    for b, want in enumerate((1, 1, 0, 1, 0, 1)):
        one = dict(c, off=c["off"][b:b + 2] - c["off"][b], rows=c["rows"][b:b + 1], loc=c["loc"][b:b + 1], ids=c["ids"][b:b + 1])
        assert _counts(one)[1] == [want, 0], f"scan {b}"
    res, e, _ = _counts(c, shadow_width=0.0)
    assert e == [6, 0] and res["shadowed"] == 0, "shadow_width 0: no shadows"


def test_the_range_and_the_box_at_their_edges():
    c = eu.edges()
    per_scan = []
    for b in range(6):
        one = dict(c, off=np.array([0, 0], np.uint32), loc=c["loc"][b:b + 1])
        res, e, _ = _counts(one)
        per_scan.append((res["in_range"], res["in_box"], e[0]))
    #                   d2 == lo2  d2 == hi2  beyond     inside lo2 lx == x_min  below x_min
    assert per_scan == [(1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0), (1, 1, 1), (1, 0, 0)]
    assert _counts(c)[1] == [3]


def test_a_seen_landmark_outside_the_box_is_expected_and_one_out_of_range_is_neither():
    res, e, s = _counts(eu.seen_outside())
    assert e == [0, 1] and s == [0, 1] and (res["in_range"], res["in_box"], res["stale"]) == (1, 0, 0)


def test_two_ids_of_one_root_name_one_landmark_once_a_scan():
    c = eu.twins()
    st = eu.state_of(c)
    assert st["alias"] == [-1, -1, 0] and st["landmarks"][0]["x"] == 0.0625
    res, e, s = eu.reference(st, c)
    # landmark 0 is named by rows 0 and 1 of scan 0 (ids 0 and 2) and by scan 1's row; landmark 1 is seen in scan 0 and, in box and
    # with the only other keypoint at the sensor itself (along = 0), expected in scan 1; the absorbed landmark 2 counts nowhere
    assert e.tolist() == [2, 2, 0] and s.tolist() == [2, 1, 0] and res["stale"] == 0 and res["seen"] == 3


def test_stale_targets_and_ids_that_propose_nothing():
    res, e, s = _counts(eu.stale())
    assert res["stale"] == 1 and s == [1, 0, 0] and e == [1, 0, 1]
    assert res["in_range"] == 2, "the landmark of a z that is not finite is not eligible"


def test_require_flags_and_poses_that_are_not_finite():
    assert _counts(eu.filters())[0]["scans_used"] == 2
    assert _counts(eu.filters(require_flags=0))[0]["scans_used"] == 5
    assert _counts(eu.filters(), require_flags=capi.FX_LOC_VALID | capi.FX_LOC_TRUNCATED)[0]["scans_used"] == 1
    for bad in (dict(require_flags=0x20), dict(min_landmark_obs=0), dict(mode=2), dict(x_min=2.0, x_max=1.0), dict(y_min=float("nan")),
                dict(min_range=-1.0), dict(max_range=0.0), dict(min_range=3.0, max_range=2.0), dict(shadow_width=float("inf"))):
        with pytest.raises(ValueError):
            _counts(eu.hand4(), **bad)


def test_add_mode_two_calls_equal_one_write_of_both_and_untouched_words_keep_their_bytes():
    c = eu.CPU_CASES["n255"]()
    st = eu.state_of(c)
    cut = int(c["off"][2])
    first = dict(c, off=c["off"][:3], rows=c["rows"][:cut], loc=c["loc"][:2], ids=c["ids"][:cut])
    second = dict(c, off=c["off"][2:] - c["off"][2], rows=c["rows"][cut:], loc=c["loc"][2:], ids=c["ids"][cut:])
    whole, e, s = eu.reference(st, c)
    assert whole["expected"] > whole["seen"] > 0 and (s <= e).all()
    sentinel = 0xdeadbeef
    e0, s0 = np.full(255, sentinel, np.uint32), np.full(255, sentinel, np.uint32)
    r1, e1, s1 = eu.reference(st, first, expected=e0, seen=s0, mode=capi.FX_EXPECT_ADD)
    r2, e2, s2 = eu.reference(st, second, expected=e1, seen=s1, mode=capi.FX_EXPECT_ADD)
    assert (e0 == sentinel).all(), "the arrays given are not modified"
    assert ((e2 - np.uint32(sentinel)) == e).all() and ((s2 - np.uint32(sentinel)) == s).all(), "uint32, wrapping"
    assert (e2[e == 0] == sentinel).all() and (e == 0).any()
    for k in ("scans_used", "in_range", "in_box", "shadowed", "expected", "seen", "stale"):
        assert r1[k] + r2[k] == whole[k], k


# ---- the retire rule
def _world():
    """The clean world of the localise tests after its run: 40 poles, a carry of the last scan's landmarks."""
    w, pieces = lu.clean_world(0, 0.01)
    st, _, _ = mu.run_reference(pieces, lu.WORLD["cap"], lu.WORLD["carry"])
    return st


def test_the_ratio_and_min_expected_at_their_edges():
    st = eu.state_of(eu.hand4())
    e = np.array([16, 16, 15, 2 ** 32 - 1], np.uint32)
    s = np.array([2, 1, 0, 2 ** 29 - 1], np.uint32)
    new, remap, mask, res, ne, ns = capi.map_retire_reference(st, e, s)
    # 2 * 8 == 16 * 1 stays; 1 * 8 < 16 goes; expected 15 < min_expected stays; (2^29 - 1) * 8 < 2^32 - 1 goes: a 32-bit product would wrap
    assert mask.tolist() == [0, 1, 0, 1] and remap.tolist() == [0, -1, 1, -1] and res["retired"] == 2 and res["retired_obs"] == 4
    assert ne.tolist() == [16, 15, 0, 0] and ns.tolist() == [2, 0, 0, 0], "the counters follow remap, zeros behind K"
    assert new["header"]["n_landmarks"] == 2 == res["kept"] and new["header"]["n_obs"] == st["header"]["n_obs"] - 4
    assert [r["x"] for r in new["landmarks"]] == [10.0, 30.0]
    for bad in (dict(min_expected=0), dict(seen_num=0), dict(seen_den=0), dict(seen_num=3, seen_den=2)):
        with pytest.raises(ValueError):
            capi.map_retire_reference(st, e, s, **bad)


def test_the_carry_protects_and_a_dry_run_changes_nothing():
    c = eu.carried()
    st = eu.state_of(c)
    assert [k for k in st["carry"][:st["header"]["carry_rows"]] if k >= 0] == [2]
    res, e, s = eu.accumulated(st, c)
    assert e.tolist() == [2, 2, 2] and not s.any()
    new, remap, mask, out, ne, ns = capi.map_retire_reference(st, e, s, **c["retire"])
    assert out == dict(before=3, kept=1, dropped_absorbed=0, retired=2, retired_obs=4, protected_by_carry=1)
    assert mask.tolist() == [1, 1, 0] and remap.tolist() == [-1, -1, 0] and new["carry"][:new["header"]["carry_rows"]].count(0) == 1
    assert ne.tolist() == [2, 0, 0]
    dry = capi.map_retire_reference(st, e, s, dry_run=True, **c["retire"])
    assert dry[0] is st and (dry[1] == remap).all() and (dry[2] == mask).all() and dry[3] == out and (dry[4] == e).all() and (dry[5] == s).all()


def test_a_call_that_retires_nothing_is_the_compaction_and_the_snapshot_checks():
    st = mm.merge_to_fixpoint(_world())[0]
    cap = st["max_landmarks"]
    zeros = np.zeros(cap, np.uint32)
    packed, remap_c, res_c = capi.map_compact_reference(st, min_obs=1)
    new, remap, mask, res, _, _ = capi.map_retire_reference(st, zeros, zeros)
    assert set(new) == set(packed) and all(repr(new[k]) == repr(packed[k]) for k in new if k != "carry_kp")
    assert (new["carry_kp"] == packed["carry_kp"]).all() and (remap == remap_c).all() and not mask.any()
    assert res["retired"] == 0 and (res["before"], res["kept"], res["dropped_absorbed"]) == (res_c["before"], res_c["kept"], res_c["dropped_absorbed"])
    again = capi.map_retire_reference(new, zeros, zeros)
    assert mm.state_bytes(again[0]) == mm.state_bytes(new), "a second call changes no byte"
    # every landmark condemned: the carried ones stay, and the result is a map every other call accepts
    full = np.full(cap, 100, np.uint32)
    new, remap, mask, res, ne, ns = capi.map_retire_reference(st, full, zeros)
    assert res["retired"] > 0 and res["protected_by_carry"] > 0 and res["kept"] == res["protected_by_carry"]
    assert res["retired_obs"] == st["header"]["n_obs"] - new["header"]["n_obs"]
    blob = capi.map_snapshot_pack(new)
    back = capi.map_snapshot_parse(blob, cap, st["max_carry_rows"])
    assert mm.state_bytes(back) == mm.state_bytes(new)
    lib = capi.load()
    assert lib.fx_map_snapshot_check(blob, len(blob), cap, st["max_carry_rows"]) == capi.FX_OK


def test_the_chained_use_forgets_the_poles_that_were_cut_down():
    """localize -> expect -> observe -> expect (adding) -> retire -> localize again, through the references alone: the landmarks of
    the two poles that left the scans are retired, nothing else that a pole still stands on is, and the new table names none."""
    w, pieces, rows, left = eu.cut_world()
    f = mm.FLICKER
    S = f["n_scans"]
    st, _, _ = mu.run_reference(pieces, f["cap"], f["carry"])
    st = mm.merge_to_fixpoint(st, **eu.CHAIN["merge"])[0]
    priors = lu.poses_of(w["truth"], seed=1072)
    loc = capi.map_localize_reference(st, w["off"], rows, priors, S, segment=capi.FX_LOC_ANY_SEGMENT)
    args = (w["off"], rows, loc["rec"], loc["map_id_of_row"], S)
    zeros = np.zeros(f["cap"], np.uint32)
    _, e, s = capi.map_expect_reference(st, *args, expected=zeros, seen=zeros, mode=capi.FX_EXPECT_ADD, **eu.CHAIN["expect"])
    st1 = capi.map_observe_reference(st, *args)[0]
    res, e, s = capi.map_expect_reference(st1, *args, expected=e, seen=s, mode=capi.FX_EXPECT_ADD, **eu.CHAIN["expect"])
    new, remap, mask, out, ne, ns = capi.map_retire_reference(st1, e, s, **eu.CHAIN["retire"])
    doomed = eu.doomed_landmarks(st1, w, left, priors)
    assert doomed and all(mask[i] for i in doomed) and not s[doomed].any() and (e[doomed] >= 4).all()
    standing = [i for i in np.flatnonzero(mask).tolist() if i not in doomed]
    assert all(int(s[i]) * 8 < int(e[i]) for i in standing) and out["retired"] == len(doomed) + len(standing)
    assert (remap[doomed] == -1).all() and out["kept"] == out["before"] - out["dropped_absorbed"] - out["retired"]
    again = capi.map_localize_reference(new, w["off"], rows, priors, S, segment=capi.FX_LOC_ANY_SEGMENT)
    table = again["map_id_of_row"]
    assert (table < out["kept"]).all() and (table >= 0).sum() > 5 * S
    assert (again["rec"]["flags"] & capi.FX_LOC_VALID).sum() == (loc["rec"]["flags"] & capi.FX_LOC_VALID).sum()


# ---- every case the GPU file runs
@pytest.mark.parametrize("name", sorted(eu.CPU_CASES))
def test_seen_never_exceeds_expected_and_the_result_adds_up(name):
    c = eu.CPU_CASES[name]()
    st = eu.state_of(c)
    res, e, s = eu.reference(st, c)
    assert (s <= e).all() and int(e.sum()) == res["expected"] and int(s.sum()) == res["seen"] and int((e > 0).sum()) == res["landmarks_expected"]
    assert res["seen"] <= res["expected"] <= res["in_range"] and res["in_box"] <= res["in_range"] and res["shadowed"] <= res["in_box"]
    assert mm.state_bytes(eu.state_of(c)) == mm.state_bytes(st), "the map is only read"


def test_the_cases_meet_their_own_census():
    """The GPU file runs these cases: every clause must be at work in at least one of them."""
    met = {k: 0 for k in ("in_box", "shadowed", "stale", "retired", "protected_by_carry", "expected_not_seen", "two_chunks", "three_rounds",
                          "none_in_range", "retired_and_kept")}
    for name, make in eu.CPU_CASES.items():
        c = make()
        st = eu.state_of(c)
        res, e, s = eu.accumulated(st, c)
        out = capi.map_retire_reference(st, e, s, **c["retire"])[3]
        for k in ("in_box", "shadowed", "stale"):
            met[k] += res[k] != 0
        for k in ("retired", "protected_by_carry"):
            met[k] += out[k] != 0
        met["expected_not_seen"] += res["expected"] > res["seen"]
        met["two_chunks"] += int(np.diff(c["off"].astype(np.int64)).max(initial=0)) > eu.CHUNK
        met["three_rounds"] += res["in_range"] > 2 * eu.WG * res["scans_used"]
        met["none_in_range"] += res["in_range"] == 0 and res["scans_used"] > 0
        met["retired_and_kept"] += out["retired"] > 0 and out["kept"] > 0
    assert all(met.values()), met
    assert _counts(eu.CPU_CASES["one_in_range"]())[0]["in_range"] == 2 and _counts(eu.CPU_CASES["far"]())[0]["in_range"] == 1
