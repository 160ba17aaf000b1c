"""capi.map_discover_reference — the all-pairs numpy statement of include/fx.h's fx_map_discover that the GPU tests compare the device
with bit for bit — held to answers worked out by hand, not to itself."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_discover_util as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = capi.FX_MAP_FULL


def _same(a, b):
    """Two states hold the same bytes."""
    return capi.map_snapshot_pack(a) == capi.map_snapshot_pack(b)


def test_the_header_states_what_the_binding_mirrors():
    src = open(os.path.join(ROOT, "include", "fx.h")).read()
    for text in (r"#define FX_MAP_LM_DISCOVERED 0x10u", r"#define FX_DISC_APPLY 0u", r"#define FX_DISC_DRY_RUN 1u", r"#define FX_VERSION_MINOR 7\b",
                 r"typedef struct fx_map_discover_options \{ +/\* 32 B \*/", r"typedef struct fx_map_discover_result \{ +/\* 64 B \*/"):
        assert re.search(text, src), text
    assert (capi.FX_MAP_LM_DISCOVERED, capi.FX_DISC_APPLY, capi.FX_DISC_DRY_RUN) == (0x10, 0, 1)
    assert C.sizeof(capi.FxMapDiscoverOptions) == 32 and C.sizeof(capi.FxMapDiscoverResult) == 64
    assert capi.FX_HEADER_VERSION == 7
    assert capi.DISCOVER_DEFAULTS == dict(known_dist=1.0, join_dist=0.30, min_obs=3, require_flags=capi.FX_LOC_VALID,
                                          segment=capi.FX_LOC_LAST_SEGMENT, mode=capi.FX_DISC_APPLY)
    for word in ("default 1.0", "default 0.30", "default 3", "default FX_LOC_VALID", "FX_LOC_LAST_SEGMENT (default)", "FX_DISC_APPLY (default)"):
        assert word in src[src.index("typedef struct fx_map_discover_options"):src.index("} fx_map_discover_options")], word
    assert "fx_map_discover (below fx_map_expect) does" in src, "fx_map_observe's Limits point at the new call"
    assert "the call creates no landmark: unmatched rows are ignored" in src and "fx_map_expect (below) counts" in src


def test_the_library_states_the_same_defaults(fxlib):
    o = capi.FxMapDiscoverOptions()
    fxlib.fx_map_discover_options_default(C.byref(o))
    assert (o.known_dist, o.join_dist) == (1.0, float(np.float32(0.30))) and list(o.reserved) == [0, 0]
    assert (o.min_obs, o.require_flags, o.segment, o.mode) == (3, capi.FX_LOC_VALID, capi.FX_LOC_LAST_SEGMENT, capi.FX_DISC_APPLY)


def test_null_arguments_are_refused_without_a_device(fxlib):
    """A context needs a device, so only the clauses that come before it can be met here; tests/test_gpu_map_discover.py meets them all."""
    assert fxlib.fx_map_discover(None, None, None, 1, 1, None, 1, None, 0, None, None, None) == 1 and b"null" in fxlib.fx_last_error()


def test_two_landmarks_three_scans_by_hand():
    """Landmarks 0 and 1 at (0, 0) and (10, 0) in segment 0, a map of 7 scans.  Scan 0 under the identity, scan 1 under tx = 1, scan 2
    under a quarter turn ((x, y) -> (-y, x)), all VALID: scans_used = 3.
      row 0 (0, 0)        id 0: matched, not unmatched
      row 1 (10.5, 0)     0.5 m from landmark 1: known
      row 2 (5, 5)        free; the first free row: a leader, id 2
      row 3 (-5, 5)       free; a leader; seen in scans 0 and 1 only: weak
      row 4 (4.125, 5)    world (5.125, 5): attaches to row 2 at 0.125
      row 5 (-6, 5)       world (-5, 5): attaches to row 3 at 0
      row 6 (5.25, -5)    world (5, 5.25): attaches to row 2 at 0.25
    unmatched 6 = known 1 + free 5; leaders 2; free 5 = weak 2 + added 3.  Landmark 2 holds (5, 5, 1), (5.125, 5, 2), (5, 5.25, 3):
    the mean is the sums / 3, the anchor (5, 5), Dx = 0.125, Dy = 0.25, Q = 0.125^2 + 0.25^2."""
    c = du.hand()
    st, res, new_id = du.reference(c)
    assert du.values(res) == (3, 6, 1, 5, 2, 0, 0, 2, 3, 0, 1, 0, 2, 0)
    assert new_id.tolist() == [-1, -1, 2, -1, 2, -1, 2]
    L = st["landmarks"][2]
    assert (L["n_obs"], L["first_scan"], L["last_scan"], L["segment"], L["flags"]) == (3, 6, 6, 0, 0x10)
    assert (L["x"], L["y"], L["z"]) == (15.125 / 3.0, 15.25 / 3.0, 2.0)
    mx, my = 0.125 / 3.0, 0.25 / 3.0
    assert L["rms_xy"] == np.float32(math.sqrt(0.078125 / 3.0 - (mx * mx + my * my)))
    assert st["acc"][2] == [15.125, 15.25, 6.0, 5.0, 5.0, 0.125, 0.25, 0.078125]
    H0, H = c["st"]["header"], st["header"]
    assert (H["n_landmarks"], H["n_needed"], H["n_obs"], H["flags"]) == (3, 3, H0["n_obs"] + 3, 0)
    assert {k: v for k, v in H.items() if k not in ("n_landmarks", "n_needed", "n_obs")} == {k: v for k, v in H0.items() if k not in ("n_landmarks", "n_needed", "n_obs")}
    assert st["landmarks"][:2] == c["st"]["landmarks"] and st["acc"][:2] == c["st"]["acc"] and st["carry"] == c["st"]["carry"]


def test_leader_attached_orphan_and_the_orphan_leads_in_the_next_call():
    c = du.chain()
    st, res, new_id = du.reference(c)
    # per scan: (0, 0) the leader's place, (0.25, 0) attached, a duplicate of its scan, (0.5, 0) within jd of the non-leader only
    assert du.values(res) == (3, 9, 0, 9, 1, 3, 3, 0, 3, 0, 1, 0, 1, 0) and new_id.tolist() == [1, -1, -1] * 3
    # on the map that learnt the pole the orphans are within known_dist of it
    _, again, _ = du.reference(c, st=st)
    assert (again["known"], again["free_rows"], again["created"]) == (9, 0, 0)
    # a caller whose first call created nothing (min_obs 4) marks the first two rows of every scan matched: the orphans lead
    st4, res4, _ = du.reference(c, min_obs=4)
    assert (res4["weak"], res4["orphans"], res4["created"]) == (3, 3, 0) and _same(st4, c["st"])
    nxt = dict(c, ids=np.array([0, 0, -1] * 3, np.int32))
    st2, res2, new2 = du.reference(nxt, st=st4)
    assert du.values(res2) == (3, 3, 0, 3, 1, 0, 0, 0, 3, 0, 1, 0, 1, 0) and new2.tolist() == [-1, -1, 1] * 3
    assert (st2["landmarks"][1]["x"], st2["landmarks"][1]["y"]) == (0.5, 0.0)


def test_the_gates_at_their_edges():
    _, res, new_id = du.reference(du.join_edge())  # world x: 0, 0.5 (d2 == jd jd: attaches), -(0.5 + 1 ulp) (does not: it leads)
    assert (res["leaders"], res["orphans"], res["created"]) == (2, 0, 2) and new_id.tolist() == [1, 1, 2]
    _, res, new_id = du.reference(du.known_edge())  # world x: 1.0 (d2 == kd kd: known), -(1 + 1 ulp) (free)
    assert (res["known"], res["free_rows"]) == (1, 1) and new_id.tolist() == [-1, 1]
    c = du.two_poles()
    _, res, _ = du.reference(c, known_dist=0.5, join_dist=0.25)
    assert res["created"] == 2
    with pytest.raises(ValueError):
        du.reference(c, known_dist=float(np.nextafter(np.float32(0.5), np.float32(0.0))), join_dist=0.25)
    for bad in (dict(known_dist=0.0), dict(join_dist=float("nan")), dict(known_dist=float("inf")), dict(min_obs=0), dict(require_flags=0x20),
                dict(segment=capi.FX_LOC_ANY_SEGMENT), dict(n_scans=0)):
        with pytest.raises(ValueError):
            du.reference(c, **bad)
    with pytest.raises(TypeError):
        du.reference(c, gate_dist=0.3)


def test_one_observation_a_scan_a_leader():
    _, res, new_id = du.reference(du.two_in_a_scan())
    assert new_id.tolist() == [1, -1, 1, -1, 1, -1] and (res["duplicates"], res["added"], res["created"]) == (3, 3, 1)


def test_min_obs_and_the_order_of_the_ids():
    _, res, new_id = du.reference(du.two_poles(n_scans=2))
    assert (res["weak"], res["created"], res["leaders"]) == (4, 0, 2) and (new_id == -1).all()
    st, res, new_id = du.reference(du.two_poles(n_scans=3))
    assert (res["weak"], res["created"], res["added"]) == (0, 2, 6) and new_id.tolist() == [1, 2, 2, 1, 2, 1]
    assert [(L["x"], L["y"]) for L in st["landmarks"][1:]] == [(20.0, 0.0), (0.0, 20.0)]
    _, res, _ = du.reference(du.two_poles(n_scans=2), min_obs=2)
    assert res["created"] == 2


def test_a_map_that_fills_and_one_that_has_overflowed():
    c = du.two_poles(cap=2)
    st, res, new_id = du.reference(c)
    assert (res["added"], res["lost"], res["created"], res["not_stored"], res["first_id"]) == (3, 3, 1, 1, 1)
    assert new_id.tolist() == [1, -1, -1, 1, -1, 1]
    H = st["header"]
    assert (H["n_landmarks"], H["n_needed"], H["flags"] & FULL, H["n_obs"]) == (2, 3, FULL, c["st"]["header"]["n_obs"] + 3) and len(st["landmarks"]) == 2
    c = du.two_poles(cap=1, n_needed=3)
    st, res, new_id = du.reference(c)
    assert (res["added"], res["lost"], res["created"], res["not_stored"], res["first_id"]) == (0, 6, 0, 2, 3) and (new_id == -1).all()
    assert (st["header"]["n_landmarks"], st["header"]["n_needed"], st["header"]["flags"] & FULL) == (1, 5, FULL) and st["landmarks"] == c["st"]["landmarks"]


def test_segments_aliases_and_the_refused_calls():
    c = du.segments_and_aliases()
    st, res, new_id = du.reference(c)
    assert (res["known"], res["free_rows"], res["created"]) == (6, 6, 2) and new_id.tolist() == [4, -1, 5, -1] * 3
    assert [L["segment"] for L in st["landmarks"][4:]] == [1, 1] and st["alias"] == [-1, -1, 3, -1, -1, -1]
    _, res, new_id = du.reference(c, segment=0)  # in segment 0 only landmark 0 explains
    assert (res["known"], res["created"]) == (3, 3) and new_id.tolist() == [-1, 4, 5, 6] * 3
    for seg in (2, 7, 0xfffffffd):
        st, res, new_id = du.reference(c, segment=seg)
        assert du.values(res) == (0,) * 12 + (4, 1) and (new_id == -1).all() and _same(st, c["st"])
    empty = dict(c, st=capi.map_state(8, 8))
    st, res, new_id = du.reference(empty)
    assert du.values(res) == (0,) * 12 + (0, 1) and (new_id == -1).all() and _same(st, empty["st"])


def test_filters_bad_rows_and_sizes():
    c = du.filters()
    _, res, new_id = du.reference(c)
    # used: scans 0, 6 and 7; scan 0: rows 0 and 2; scan 6: its one good row is matched; scan 7: the row at the origin alone is finite
    assert (res["scans_used"], res["unmatched"], res["created"]) == (3, 3, 3) and new_id.reshape(8, 3).tolist()[0] == [1, -1, 2]
    assert np.flatnonzero(new_id >= 0).tolist() == [0, 2, 21]
    _, res, new_id = du.reference(du.filters(require_flags=0))
    assert res["scans_used"] == 6 and (new_id.reshape(8, 3)[4:6] == -1).all() and new_id[[3, 9, 19]].tolist() == [-1, -1, -1]
    _, res, _ = du.reference(c, require_flags=capi.FX_LOC_VALID | capi.FX_LOC_TRUNCATED)
    assert res["scans_used"] == 1
    _, res, _ = du.reference(c, n_scans=11)  # beyond the block
    assert res["scans_used"] == 3
    _, res, new_id = du.reference(c, q_max_rows=2)  # scan 0 is cut after its second row
    assert res["unmatched"] == 1 and new_id.tolist() == [1, -1]
    _, res, new_id = du.reference(c, q_max_rows=30)
    assert res["unmatched"] == 3 and len(new_id) == 30
    _, res, _ = du.reference(c, stored=2)
    assert res["unmatched"] == 1
    _, res, new_id = du.reference(c, q_max_rows=0)
    assert du.values(res) == (3,) + (0,) * 11 + (1, 0) and len(new_id) == 0


@pytest.mark.parametrize("name", sorted(du.CASES))
def test_identities_the_dry_run_and_the_second_call(name):
    c = du.CASES[name]()
    st, res, new_id = du.reference(c)
    du.assert_identities(res, name)
    dry_st, dry, dry_id = du.reference(c, dry_run=True)
    assert dry == res and dry_id.tobytes() == new_id.tobytes() and _same(dry_st, c["st"])
    assert (res["created"] > 0) == (not _same(st, c["st"])) or res["not_stored"] > 0
    st2, again, new2 = du.reference(c, st=st)
    du.assert_identities(again, name + ", again")
    if not res["not_stored"]:
        assert again["created"] == 0 and (new2 == -1).all(), "no twin"
        assert again["known"] >= res["known"] + res["added"], "every formerly kept row is known"


@pytest.mark.parametrize("seed", du.SEEDS)
def test_the_seeded_worlds_meet_the_census(seed):
    c = du.world(seed)
    S = len(c["off"]) - 1
    assert 5 <= S <= 40 and len(c["st"]["landmarks"]) <= 40
    st, res, new_id = du.reference(c)
    du.assert_identities(res, f"seed {seed}")
    assert du.census(res) and res["created"] <= 6, res
    _, again, _ = du.reference(c, st=st)
    assert again["created"] == 0 and again["known"] >= res["known"] + res["added"]
    for L in st["landmarks"][res["first_id"]:]:
        assert L["flags"] == 0x10 and L["n_obs"] >= 3 and L["rms_xy"] < 0.15
