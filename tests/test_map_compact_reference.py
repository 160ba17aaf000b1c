"""fx_map_compact, the part that needs no GPU: the C-ABI's new names, and capi.map_compact_reference — the executable statement of
include/fx.h's definition — held to what the call exists for: the dead records leave, every kept landmark keeps its bytes, and the
run goes on exactly as it would have."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_compact_util as mc
from tests import map_merge_util as mm
from tests import map_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_declared_exported_and_listed(fxlib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fx.h")).read(), flags=re.S)
    for n in ("fx_map_compact_options", "fx_map_compact_result"):
        assert re.search(r"typedef struct %s\s*\{[^}]*\}\s*%s;" % (n, n), src), n
    for n in ("fx_map_compact_options_default", "fx_map_compact", "fx_map_export_host", "fx_map_import_host", "fx_map_snapshot_check"):
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(fxlib, n) and n in capi.EXPORTS, n
    assert "#define FX_VERSION_MINOR 7" in src and fxlib.fx_version() == 7  # added symbols only
    assert C.sizeof(capi.FxMapCompactOptions) == 8 and C.sizeof(capi.FxMapCompactResult) == 16
    o, m = capi.FxMapCompactOptions(), capi.FxMapMergeOptions()
    fxlib.fx_map_compact_options_default(C.byref(o)), fxlib.fx_map_merge_options_default(C.byref(m))
    assert o.min_obs == 1 and o.min_age_scans == 64 == m.max_gap_scans
    assert "fx_map_compact.hip" in __import__("feature_extraction_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.fixture(scope="module")
def merged():
    w, pieces, _ = mm.flicker()
    f = mm.FLICKER
    st, tracks, ids = mu.run_reference(pieces, f["cap"], f["carry"])
    st, _ = mm.merge_to_fixpoint(st, max_gap_scans=mc.GAP)
    return w, pieces, st, ids, tracks


def test_flicker_world_only_the_live_landmarks_stay(merged):
    w, pieces, st, ids, _ = merged
    before = mm.state_bytes(st)
    out, remap, res = capi.map_compact_reference(st)
    assert mm.state_bytes(st) == before, "the input is not modified"
    H = out["header"]
    assert len(out["landmarks"]) == H["n_landmarks"] == H["n_needed"] == res["kept"] == mc.FLICKER_LIVE == len(mm.long_runs(w))
    assert res == {"before": 54, "kept": 33, "dropped_absorbed": 21, "dropped_live": 0}
    assert H["n_obs"] == st["header"]["n_obs"] and out["alias"] == [-1] * 33
    assert {k: v for k, v in H.items() if k not in ("n_landmarks", "n_needed")} == {k: v for k, v in st["header"].items() if k not in ("n_landmarks", "n_needed")}
    mc.assert_moved(st, out, remap, "flicker")
    # remap alone does what the alias table and the ranks of the live landmarks do together
    rank = mc.rank_of_live(st["alias"])
    assert len(remap) == st["max_landmarks"] and (remap[54:] == -1).all()
    for p, row_ids in zip(pieces, ids):
        assert (mc.through(remap, row_ids) == mc.through(rank, mm.resolve(row_ids, st["alias"]))).all()
    assert sorted(remap[:54][np.array(st["alias"]) == -1].tolist()) == list(range(33))  # order kept, no gap
    assert (np.diff(remap[:54][np.array(st["alias"]) == -1]) == 1).all()
    # the carry points at the same landmarks
    assert out["carry"] == [int(remap[c]) if c >= 0 else c for c in st["carry"]] and any(c >= 0 for c in out["carry"])


def test_compaction_commutes_with_the_run():
    r = mc.flicker_runs(k=2)
    n0, k0 = r["result"]["before"], r["result"]["kept"]
    assert r["result"]["dropped_absorbed"] > 0 and r["result"]["dropped_live"] == 0
    A, B = r["plain"], r["compacted"]
    assert not (A["header"]["flags"] | B["header"]["flags"]) & capi.FX_MAP_OVERLAP_MISMATCH
    m = mc.id_mapping(r["remap"], n0, k0, A["header"]["n_landmarks"])
    for (ia, ha), (ib, hb) in zip(r["plain_tail"], r["compacted_tail"]):
        assert (mc.through(m, ia) == ib).all(), "the same rows continue the same landmarks"
        assert ha["last_joined"] == hb["last_joined"] > 0 and ha["last_new"] == hb["last_new"]
    dropped = n0 - k0
    assert B["header"]["n_landmarks"] == A["header"]["n_landmarks"] - dropped == len(B["landmarks"])
    assert B["header"]["n_obs"] == A["header"]["n_obs"] and B["header"]["scans"] == A["header"]["scans"]
    mc.assert_moved(dict(A, alias=list(r["before"]["alias"])), B, m, "after the remaining pieces")
    # and the merge at the end finds the same fragments
    A2, ra = mm.merge_to_fixpoint(A, max_gap_scans=mc.GAP)
    B2, rb = mm.merge_to_fixpoint(B, max_gap_scans=mc.GAP)
    assert [x["merged"] for x in ra] == [x["merged"] for x in rb] and ra[-1]["live"] == rb[-1]["live"] == mc.FLICKER_LIVE


def test_localize_gives_the_same_records_on_the_compacted_map(merged):
    w, pieces, st, ids, tracks = merged
    out, remap, _ = capi.map_compact_reference(st)
    p, prior = pieces[-1], tracks[-1]["poses"].copy()
    prior["tx"] += 0.25  # (priors a little off the map's frame)
    prior["ty"] -= 0.125
    kw = dict(segment=capi.FX_LOC_ANY_SEGMENT, min_landmark_obs=1)
    a = capi.map_localize_reference(st, p["off"], p["rows"], prior, p["n_scans"], **kw)
    b = capi.map_localize_reference(out, p["off"], p["rows"], prior, p["n_scans"], **kw)
    assert a["rec"].tobytes() == b["rec"].tobytes() and (a["rec"]["flags"] & capi.FX_LOC_VALID).any()
    for k in ("map_id_of_row", "nearest_of_row"):
        assert (mc.through(remap, a[k]) == b[k]).all() and (a[k] >= 0).any(), k


def _aged():
    """8 scans, tracks of min_obs = 1.  Ids in order: an old long landmark (scans 0-2), a short one last seen at scan 4 (age 3), a
    short one last seen at scan 5 (age 2), a short one in the last scan (in the carry), a long one in scans 6-7."""
    w = mc.fragments([(0, 3, 1.0, 1.0), (4, 1, 11.0, 1.0), (5, 1, 21.0, 1.0), (6, 2, 41.0, 1.0), (7, 1, 31.0, 1.0)], 8)
    st, _, ids = mu.run_reference([w], 16, 16, min_obs=1)
    lm = mm.ids_of(w, ids[0])
    assert lm == [0, 1, 2, 3, 4] and st["header"]["n_obs"] == 8 and st["header"]["scans"] == 8
    return st, lm


def test_min_obs_and_min_age_scans():
    st, (long_old, age3, age2, long_new, carried) = _aged()
    assert carried in st["carry"] and long_new in st["carry"]
    out, remap, res = capi.map_compact_reference(st, min_obs=2, min_age_scans=3)
    assert remap[:5].tolist() == [0, -1, 1, 2, 3] and res == {"before": 5, "kept": 4, "dropped_absorbed": 0, "dropped_live": 1}
    assert out["header"]["n_obs"] == 8 - 1 and out["header"]["n_landmarks"] == out["header"]["n_needed"] == 4
    mc.assert_moved(st, out, remap, "age")
    # age is the only thing that keeps the one of age min_age_scans - 1: one scan less and it goes too
    out, remap, res = capi.map_compact_reference(st, min_obs=2, min_age_scans=2)
    assert remap[:5].tolist() == [0, -1, -1, 1, 2] and res["dropped_live"] == 2 and out["header"]["n_obs"] == 6
    # min_age_scans = 0: nothing is young; the short landmark of the last scan stays because the carry refers to it
    out, remap, res = capi.map_compact_reference(st, min_obs=2, min_age_scans=0)
    assert remap[:5].tolist() == [0, -1, -1, 1, 2] and out["carry"] == [int(remap[c]) if c >= 0 else c for c in st["carry"]]
    assert all(c >= 0 for c in out["carry"]) and out["header"]["n_obs"] == 6
    # without a carry it goes as well
    bare = dict(st, carry=[-1] * len(st["carry"]))
    out, remap, res = capi.map_compact_reference(bare, min_obs=2, min_age_scans=0)
    assert remap[:5].tolist() == [0, -1, -1, 1, -1] and out["header"]["n_obs"] == 5
    # min_obs = 3 takes the two-observation landmark when it is old enough, never the default
    out, remap, res = capi.map_compact_reference(bare, min_obs=3, min_age_scans=0)
    assert remap[:5].tolist() == [0, -1, -1, -1, -1]
    assert capi.map_compact_reference(st)[2]["dropped_live"] == 0
    with pytest.raises(ValueError):
        capi.map_compact_reference(st, min_obs=0)


def test_identity_idempotence_and_the_empty_map(merged):
    st, _ = _aged()
    out, remap, res = capi.map_compact_reference(st)
    assert mm.state_bytes(dict(out, alias=[])) == mm.state_bytes(st) and remap[:5].tolist() == list(range(5)) and (remap[5:] == -1).all()
    assert res == {"before": 5, "kept": 5, "dropped_absorbed": 0, "dropped_live": 0}
    for state, kw in ((merged[2], {}), (st, dict(min_obs=2, min_age_scans=2))):
        once, _, _ = capi.map_compact_reference(state, **kw)
        twice, remap, res = capi.map_compact_reference(once, **kw)
        n = once["header"]["n_landmarks"]
        assert mm.state_bytes(twice) == mm.state_bytes(once) and remap[:n].tolist() == list(range(n)) and res["kept"] == res["before"] == n
    out, remap, res = capi.map_compact_reference(capi.map_state(4, 4))
    assert res == {"before": 0, "kept": 0, "dropped_absorbed": 0, "dropped_live": 0} and remap.tolist() == [-1] * 4 and out["landmarks"] == []
