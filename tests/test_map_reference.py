"""The persistent landmark map, the part that needs no GPU: the C-ABI's new names and struct layouts, and capi.map_reference — the
numpy statement of include/fx.h's definition — held to the property the map exists for: however a run is cut into batches that
overlap by one scan, track -> map over the pieces gives what ONE track over the whole run gives, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_util as mu
from tests import track_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SCANS = 37


def test_names_declared_exported_and_listed(fxlib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fx.h")).read(), flags=re.S)
    for n in ("fx_map_landmark", "fx_map_header"):
        assert re.search(r"typedef struct %s\s*\{[^}]*\}\s*%s;" % (n, n), src), n
    for n in ("fx_map_create", "fx_map_destroy", "fx_map_reset", "fx_map_update", "fx_map_get", "fx_map_read_header", "fx_map_read_landmarks"):
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(fxlib, n), n
        assert n in capi.EXPORTS, n
    assert "#define FX_VERSION_MINOR 7" in src and fxlib.fx_version() == 7  # added symbols only


def test_struct_layouts():
    assert C.sizeof(capi.FxMapLandmark) == 48 == capi.MAP_LANDMARK_DTYPE.itemsize and C.sizeof(capi.FxMapHeader) == 88
    assert [f[0] for f in capi.FxMapLandmark._fields_] == list(capi.MAP_LANDMARK_DTYPE.names)
    assert [getattr(capi.FxMapLandmark, n).offset for n in capi.MAP_LANDMARK_DTYPE.names] == [capi.MAP_LANDMARK_DTYPE.fields[n][1] for n in capi.MAP_LANDMARK_DTYPE.names]
    assert [f[0] for f in capi.FxMapHeader._fields_[:10]] == list(capi.MAP_HEADER_FIELDS) and capi.FxMapHeader.last_pose.offset == 40


@pytest.fixture(scope="module")
def run():
    """37 scans, 15 % dropout, centimetre noise, two bad links; the whole run's track is computed once."""
    w = tu.world(np.random.default_rng(41), 80, N_SCANS, dropout=0.15, sigma=0.01)
    w["reg"]["flags"][[11, 25]] = 0
    whole = tu.reference(w)
    assert whole["header"]["n_gaps"] == 2 and whole["header"]["n_landmarks"] > 100 and whole["landmarks"]["n_obs"].max() >= 8
    return w, whole


@pytest.mark.parametrize("name,edges", [("every scan", mu.every(N_SCANS, 1)), ("every 5", mu.every(N_SCANS, 5)),
                                        ("uneven", [0, 1, 2, 9, 11, 12, 26, 27, 33, 36])])
def test_any_cut_gives_the_whole_runs_landmarks_bit_for_bit(run, name, edges):
    w, whole = run
    pieces = mu.split(w, edges)
    assert pieces[0]["scan0"] == 0 and edges[-1] == N_SCANS - 1
    st, tracks, ids = mu.run_reference(pieces, len(w["rows"]), 200)
    recs = capi.map_state_records(st)
    mu.assert_whole(recs, whole, name)
    mu.assert_rows_map_to_whole(pieces, ids, whole, name)
    for p, tr in zip(pieces, tracks):  # the poses: every piece's are the whole run's, bit for bit (segments re-based)
        a, n = p["scan0"], p["n_scans"]
        for f in ("c", "s", "tx", "ty", "tz"):
            assert (tu.bits(tr["poses"][f]) == tu.bits(whole["poses"][f][a:a + n])).all(), (name, a, f)
        assert (tr["poses"]["segment"] + whole["poses"]["segment"][a] == whole["poses"]["segment"][a:a + n]).all()
    H = recs["header"]
    assert H["batches"] == len(pieces) and H["flags"] == 0 and H["segments"] == 3
    assert [float(v).hex() for v in H["last_pose"][:5]] == [float(whole["poses"][f][-1]).hex() for f in ("c", "s", "tx", "ty", "tz")]
    # rms_xy is the spread about the mean through an anchor, not the track's two-pass value: held to an independent fp64 two-pass
    # computation over the same observations.  Bound: 4 ulp of float32 (the fp64 errors of both are orders below one), plus what
    # the two-pass mean's own rounding can leave when the spread is (nearly) zero: n 2^-53 |w| <= 2^-46 |w|.
    ref, mag = mu.independent_rms(w, whole)
    got = recs["landmarks"]["rms_xy"].astype(np.float64)
    err = np.abs(got - ref)
    bound = 4 * np.spacing(ref.astype(np.float32)).astype(np.float64) + 2.0 ** -46 * mag
    print(f"{name}: {len(pieces)} pieces, {len(ref)} landmarks, rms_xy worst error {err.max():.2e} of bound {bound[err.argmax()]:.2e}, last_joined {H['last_joined']}")
    assert (err <= bound).all(), (err.max(), bound[err.argmax()])
    assert (recs["landmarks"]["flags"] & capi.FX_MAP_LM_CONTINUED).any() and np.abs(got - whole["landmarks"]["rms_xy"]).max() < 1e-6


def _two_batches(rng, lens=(3, 3), through_first=True):
    """Two hand-built batches that overlap by one scan: chain A through both, chain B ending at the overlap scan (before or after
    A in row order), chain C starting there, and a stray row a scan.  Returns the whole case and its pieces."""
    n = lens[0] + lens[1] - 1
    h = tu.Hand(n)
    e = lens[0] - 1
    if through_first:
        h.chain(0, n), h.chain(0, e + 1)
    else:
        h.chain(0, e + 1), h.chain(0, n)
    h.chain(e, n - e)
    for b in range(n):
        h.new(b)
    w = h.finish(rng)
    return w, mu.split(w, [0, e, n - 1])


def test_overlap_mismatch_and_a_batch_without_the_flag():
    w, pieces = _two_batches(np.random.default_rng(42))
    whole = tu.reference(w)
    st, _, _ = mu.run_reference(pieces, 64, 64)
    mu.assert_whole(capi.map_state_records(st), whole, "two batches")
    assert st["header"]["last_joined"] == 1 and st["header"]["last_new"] == 1 and st["header"]["scans"] == 5
    # without the flag: the second batch's tracks are all new, its scans and its segment follow on
    st2, _, _ = mu.run_reference(pieces, 64, 64, overlap=False)
    H = st2["header"]
    assert H["flags"] == 0 and H["last_joined"] == 0 and H["last_new"] == 2 and H["n_needed"] == 4 and H["scans"] == 6 and H["segments"] == 2
    L = capi.map_state_records(st2)["landmarks"]
    assert L["first_scan"].tolist() == [0, 0, 3, 3] and L["segment"].tolist() == [0, 0, 1, 1] and L["n_obs"].tolist() == [3, 3, 3, 3]
    # the flag, and one bit of the overlap scan's elevation word altered: a mismatch, taken as without the flag
    first = capi.map_state(64, 64)
    tr0 = tu.reference(pieces[0])
    first, _ = capi.map_reference(first, pieces[0]["off"], pieces[0]["rows"], tr0, overlap=True)
    assert first["header"]["flags"] == capi.FX_MAP_OVERLAP_MISMATCH and first["header"]["scans"] == 3  # (a first batch has nothing to overlap)
    first["header"]["flags"] = 0
    p = dict(pieces[1], rows=pieces[1]["rows"].copy())
    p["rows"].view(np.uint32)[1, 3] ^= 1
    tr = tu.reference(p, init_pose=first["header"]["last_pose"][:5])
    bad, ids = capi.map_reference(first, p["off"], p["rows"], tr, overlap=True)
    assert bad["header"]["flags"] == capi.FX_MAP_OVERLAP_MISMATCH and bad["header"]["last_joined"] == 0 and bad["header"]["scans"] == 6
    assert first["header"]["flags"] == 0 and first["header"]["scans"] == 3  # (the state passed in is not modified)
    # a different row count in scan 0 is a mismatch as well
    q = dict(pieces[1])
    q["off"] = np.array([0, 2, 4, 7, 10], np.uint32)  # (the same rows as one scan more: scan 0 of two rows, not four)
    q["n_scans"], q["reg"] = 4, np.concatenate([q["reg"][:1], q["reg"]])
    q["m"] = tu.match_rows(q["off"])
    q["inlier"] = np.zeros(10, np.int32)
    bad, _ = capi.map_reference(first, q["off"], q["rows"], tu.reference(q), overlap=True)
    assert bad["header"]["flags"] == capi.FX_MAP_OVERLAP_MISMATCH


def test_a_batch_of_only_the_overlap_scan_changes_nothing():
    w, pieces = _two_batches(np.random.default_rng(43))
    e = pieces[1]["scan0"]
    with_single = mu.split(w, [0, e, e, w["n_scans"] - 1])
    assert with_single[1]["n_scans"] == 1
    for min_obs in (2, 1):
        a, _, _ = mu.run_reference(pieces, 64, 64, min_obs=min_obs)
        b, _, ids = mu.run_reference(with_single, 64, 64, min_obs=min_obs)
        ra, rb = capi.map_state_records(a), capi.map_state_records(b)
        assert rb["header"].pop("batches") == ra["header"].pop("batches") + 1
        mu.assert_equal(rb, ra, f"S == 1, min_obs {min_obs}")
        assert a["carry"] == b["carry"]
    assert len(ids[1]) == 4 and (ids[1] >= 0).all()  # (min_obs 1: every row of the overlap scan is a landmark and keeps its id)


def test_capacity_of_the_map_and_of_the_carry():
    w, pieces = _two_batches(np.random.default_rng(44), lens=(4, 4))
    whole = tu.reference(w)
    assert whole["header"]["n_landmarks"] == 3
    # map capacity 2 of 3 needed: batch 0 stores A and B; C (new in batch 1) is counted and not stored
    st, _, ids = mu.run_reference(pieces, 2, 64)
    H = st["header"]
    assert H["n_needed"] == 3 and H["n_landmarks"] == 2 and H["flags"] == capi.FX_MAP_FULL and len(st["landmarks"]) == 2 and H["last_new"] == 1
    assert set(ids[1].tolist()) == {-1, 0}  # chain A's rows; C's report -1
    # capacity 1, with B before A in row order: A is counted and not stored in batch 0, so its continuation in batch 1 is new AGAIN
    _, other = _two_batches(np.random.default_rng(44), lens=(4, 4), through_first=False)
    st, _, ids = mu.run_reference(other, 1, 64)
    H = st["header"]
    assert H["n_needed"] == 2 + 2 and H["n_landmarks"] == 1 and H["last_joined"] == 0 and H["last_new"] == 2 and st["landmarks"][0]["n_obs"] == 4
    assert (ids[1] == -1).all()
    # the track's own output truncated to 1 landmark a batch
    s = capi.map_state(64, 64)
    for k, p in enumerate(pieces):
        tr = tu.reference(p, init_pose=s["header"]["last_pose"][:5])
        s, row_ids = capi.map_reference(s, p["off"], p["rows"], tr, overlap=k > 0, track_max_landmarks=1)
        assert (row_ids >= 0).sum() == tr["landmarks"]["n_obs"][0]
    assert s["header"]["flags"] == capi.FX_MAP_TRACK_TRUNCATED and s["header"]["n_needed"] == 1 and s["landmarks"][0]["n_obs"] == 7
    # a carry table too small for the overlap scan: nothing is carried, the next overlap is a mismatch
    n_e = int(np.diff(pieces[0]["off"])[-1])
    st, _, _ = mu.run_reference(pieces, 64, n_e - 1)
    assert st["header"]["flags"] == capi.FX_MAP_OVERLAP_MISMATCH and st["header"]["last_joined"] == 0 and st["header"]["scans"] == 8
    st, _, _ = mu.run_reference(pieces, 64, n_e)
    assert st["header"]["flags"] == 0 and st["header"]["last_joined"] == 1 and st["header"]["carry_rows"] == int(np.diff(pieces[1]["off"])[-1])
