"""capi.map_observe_reference — the all-pairs numpy statement of include/fx.h's fx_map_observe that the GPU tests compare the device
with bit for bit — held to answers worked out by hand and to properties that do not go through its own anchor algebra."""
import math
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_compact_util as mc
from tests import map_localize_util as lu
from tests import map_merge_util as mm
from tests import map_observe_util as ou
from tests import map_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_states_the_constants_the_binding_mirrors():
    src = open(os.path.join(ROOT, "include", "fx.h")).read()
    assert re.search(r"#define FX_MAP_LM_OBSERVED 0x8u", src) and re.search(r"#define FX_OBS_APPLY 0u", src) and re.search(r"#define FX_OBS_DRY_RUN 1u", src)
    assert (capi.FX_MAP_LM_OBSERVED, capi.FX_OBS_APPLY, capi.FX_OBS_DRY_RUN) == (8, 0, 1)
    import ctypes as C
    assert C.sizeof(capi.FxMapObserveOptions) == 16 and C.sizeof(capi.FxMapObserveResult) == 32
    assert re.search(r"re-estimates no landmark \(fx_map_observe, below, does", src), "fx_map_localize's Limits point at the new call"


def test_three_landmarks_and_six_rows_by_hand():
    """Landmarks 0, 1, 2 at x = 0, 10, 20 (y = 0, two observations each); landmark 2's record is made NaN.  Scan 0 under the
    identity, scan 1 under tx = 0.125, both VALID: scans_used = 2.
      row 0 (0.1, 0)   id 0: passes, d = 0.1           -> the duplicate of row 1
      row 1 (0.05, 0)  id 0: passes, d = 0.05          -> kept (the lowest d2 of scan 0 on landmark 0)
      row 2 (10.5, 0)  id 1: d = 0.5 > 0.30            -> gated
      row 3 (0, 0)     id 0: world x = 0.125, passes   -> kept (scan 1's one observation of landmark 0)
      row 4 (20, 0)    id 7 >= N = 3                   -> no proposal
      row 5 (20, 0)    id 2: the record is not finite  -> stale
    proposed = 5 = added 2 + duplicates 1 + gated 1 + stale 1, one landmark touched.  Landmark 0 then holds 4 observations at
    x = 0, 0, 0.05f, 0.125: the mean is their sum / 4; the anchor is 0, so Q = 0.05f^2 + 0.125^2 and rms follows."""
    c = ou.hand3()
    st0 = ou.state_of(c)
    st, res, gained, observed = ou.reference(st0, c)
    assert tuple(res[k] for k in ou.RESULT) == (2, 5, 2, 1, 1, 1, 1) and res["reserved"] == 0
    assert gained.tolist() == [2, 0, 0] and observed.tolist() == [-1, 0, -1, 0, -1, -1]
    x1 = float(np.float32(0.05))
    L = st["landmarks"][0]
    assert L["n_obs"] == 4 and L["x"] == (x1 + 0.125) / 4.0 and L["y"] == 0.0 and L["z"] == 1.0 and L["flags"] == capi.FX_MAP_LM_OBSERVED
    mean = (x1 + 0.125) / 4.0
    assert L["rms_xy"] == np.float32(math.sqrt((x1 * x1 + 0.125 * 0.125) / 4.0 - mean * mean))
    assert (L["first_scan"], L["last_scan"], L["segment"]) == tuple(st0["landmarks"][0][k] for k in ("first_scan", "last_scan", "segment"))
    assert st["header"]["n_obs"] == st0["header"]["n_obs"] + 2
    assert {k: v for k, v in st["header"].items() if k != "n_obs"} == {k: v for k, v in st0["header"].items() if k != "n_obs"}
    assert st["landmarks"][1] == st0["landmarks"][1] and st["acc"][1:] == st0["acc"][1:] and st["carry"] == st0["carry"]


def test_ties_ids_the_gate_and_the_filters_by_hand():
    c = ou.duplicates()
    _, res, gained, observed = ou.reference(ou.state_of(c), c)
    # scan 0: landmark 0 rows 0, 2 (row 2 nearer), landmark 1 rows 1, 3, 5 (row 3 nearest), landmark 2 rows 4, 6 (equal bits: row 4)
    assert observed.tolist() == [-1, -1, 0, 1, 2, -1, -1, 5, 2, -1, 0, 1] and gained[:6].tolist() == [2, 2, 2, 0, 0, 1]
    assert (res["added"], res["duplicates"], res["landmarks_touched"]) == (7, 5, 4)
    c = ou.garbage_ids()
    _, res, _, observed = ou.reference(ou.state_of(c), c)
    assert res["proposed"] == 1 == res["added"] and observed.tolist() == [-1] * 6 + [6, -1]
    c = ou.gate_edge()
    st, res, gained, observed = ou.reference(ou.state_of(c), c)
    assert observed.tolist() == [0, -1, 0, -1, 0] and (res["added"], res["gated"]) == (3, 2) and st["landmarks"][0]["x"] == 0.0
    c = ou.filters()
    _, res, _, observed = ou.reference(ou.state_of(c), c)
    assert res["scans_used"] == 2 and observed.reshape(7, 3).tolist() == [[0, -1, 8]] + [[-1] * 3] * 5 + [[-1, 10, -1]]
    c = ou.filters(require_flags=0)
    _, res, _, observed = ou.reference(ou.state_of(c), c)
    assert res["scans_used"] == 5 and (observed.reshape(7, 3)[1:4] >= 0).all() and (observed.reshape(7, 3)[4:6] == -1).all()


def test_two_ids_of_one_root_are_one_landmark():
    c = ou.merged_twins()
    st0, results = mm.merge_to_fixpoint(ou.state_of(c))
    assert st0["alias"] == [-1, -1, 0] and st0["landmarks"][0]["x"] == 0.0625
    st, res, gained, observed = ou.reference(st0, c)
    assert observed.tolist() == [0, -1, 1, 0] and gained.tolist() == [2, 1, 0]
    assert tuple(res[k] for k in ou.RESULT) == (2, 4, 3, 1, 0, 0, 2)
    assert st["landmarks"][2] == st0["landmarks"][2] and st["acc"][2] == st0["acc"][2], "the absorbed record stays frozen"


def test_sizes_as_in_the_localise():
    c = ou.filters(require_flags=0)
    st = ou.state_of(c)
    full = ou.reference(st, c)[3]
    for q in (0, 5, 20, 21, 40):
        _, res, gained, observed = ou.reference(st, c, q_max_rows=q)
        assert len(observed) == q and (observed[:min(q, 21)] == full[:min(q, 21)]).all() and (observed[21:] == -1).all()
        ou.assert_sums_to_proposed(res)
    _, res, _, observed = ou.reference(st, c, n_scans=2)
    assert (observed[6:] == -1).all() and res["scans_used"] == 2
    _, res, _, observed = ou.reference(st, c, stored=7)
    assert (observed[7:] == -1).all() and (observed[:7] == full[:7]).all()
    empty = capi.map_state(8, 8)
    _, res, gained, observed = ou.reference(empty, c)
    assert res["proposed"] == 0 and res["scans_used"] == 5 and not gained.any() and (observed == -1).all()


@pytest.mark.parametrize("name", sorted(ou.CPU_CASES))
def test_counts_add_up_and_the_mean_is_the_weighted_mean(name):
    """proposed = added + duplicates + gated + stale; for every touched landmark the new mean is (n0 old mean + the sum of its kept
    world points) / (n0 + k) within 1e-9 m: at most 2048 fp64 additions of coordinates below 1024 m, 2048 * 2^-53 * 1024 m = 2.3e-10 m.
    The check knows nothing of the anchor."""
    c = ou.CPU_CASES[name]()
    st0 = ou.state_of(c)
    st, res, gained, observed = ou.reference(st0, c)
    ou.assert_sums_to_proposed(res, name)
    assert int(gained.sum()) == res["added"] == int((observed >= 0).sum()) and int((gained > 0).sum()) == res["landmarks_touched"]
    W = ou.world_points(c)
    for g in np.flatnonzero(gained).tolist():
        old, new = st0["landmarks"][g], st["landmarks"][g]
        mine = np.flatnonzero(observed == g)
        k, n0 = len(mine), old["n_obs"]
        assert k == gained[g] and new["n_obs"] == n0 + k and new["flags"] & capi.FX_MAP_LM_OBSERVED
        for j, f in enumerate("xyz"):
            want = (n0 * old[f] + math.fsum(W[mine, j].tolist())) / (n0 + k)
            assert abs(new[f] - want) <= 1e-9, (name, g, f, new[f], want)
    for g in np.flatnonzero(gained == 0).tolist()[:len(st0["landmarks"])]:
        if g < len(st0["landmarks"]):
            assert st["landmarks"][g] == st0["landmarks"][g] and st["acc"][g] == st0["acc"][g]
    # a dry run reports the same and returns the state unchanged
    dry, res_d, gained_d, observed_d = ou.reference(st0, c, dry_run=True)
    assert res_d == res and (gained_d == gained).all() and (observed_d == observed).all()
    assert mm.state_bytes(dry) == mm.state_bytes(st0) and dry["header"] == st0["header"]


def test_the_cases_meet_their_own_census():
    seen = {k: 0 for k in ou.RESULT}
    for name, make in ou.CPU_CASES.items():
        c = make()
        res = ou.reference(ou.state_of(c), c)[1]
        for k in ou.RESULT:
            seen[k] += res[k] != 0
    assert all(seen.values()), seen
    c = ou.lists()
    assert ou.reference(ou.state_of(c), c)[2][:len(ou.COUNTS)].tolist() == ou.COUNTS


def test_a_merge_and_a_compaction_since_the_localise():
    """The flicker world: the table of a localise BEFORE the merge.  After the merge the absorbed ids resolve to their roots and two
    ids of one root are one landmark (duplicates appear that the unmerged map does not have); after a compaction without remap the
    same table is stale ids and ids of other landmarks: nothing but counts and gates, and no landmark beyond N is touched."""
    w, pieces, _ = mm.flicker()
    f = mm.FLICKER
    st0, _, _ = mu.run_reference(pieces, f["cap"], f["carry"])
    priors = lu.poses_of(w["truth"], seed=1072)
    loc = capi.map_localize_reference(st0, w["off"], w["rows"], priors, f["n_scans"], segment=capi.FX_LOC_ANY_SEGMENT)
    args = (w["off"], w["rows"], loc["rec"], loc["map_id_of_row"], f["n_scans"])
    _, before, _, _ = capi.map_observe_reference(st0, *args)
    merged, _ = mm.merge_to_fixpoint(st0, max_gap_scans=mc.GAP)
    st, after, gained, observed = capi.map_observe_reference(merged, *args)
    ou.assert_sums_to_proposed(before), ou.assert_sums_to_proposed(after)
    assert after["proposed"] == before["proposed"] > 0 and after["stale"] == 0
    alias = np.array(merged["alias"])
    assert (alias[observed[observed >= 0]] == -1).all() and not gained[np.flatnonzero(alias >= 0)].any()
    assert after["landmarks_touched"] < before["landmarks_touched"]
    packed, _, _ = capi.map_compact_reference(merged)
    N = packed["header"]["n_landmarks"]
    st, res, gained, observed = capi.map_observe_reference(packed, *args)
    ou.assert_sums_to_proposed(res)
    assert res["proposed"] < after["proposed"] and (observed < N).all() and not gained[N:].any()
