"""Helpers of the map tests (tests/test_map_reference.py, tests/test_gpu_map.py): cutting a track_util case into batches that
overlap by one scan, running track -> map over the pieces on the CPU (capi.track_reference, capi.map_reference), and the
comparisons: a map against another bit for bit, and a map against ONE track over the whole run."""
import numpy as np

from feature_extraction_amd import capi
from tests import track_util as tu


def split(w, edges):
    """Cuts a track_util case dict into overlapping sub-cases: piece k holds the scans edges[k] .. edges[k + 1] inclusive, so a
    piece's first scan is the last scan of the piece before.  Rows, train_row and pair are re-based; the first scan's rows get no
    pair (and no inlier word), as a match over pairs_consecutive of the piece leaves them; reg is sliced."""
    off = [int(x) for x in w["off"]]
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        assert 0 <= a <= b < w["n_scans"]
        r0, r1 = off[a], off[b + 1]
        o = np.array(off[a:b + 2], np.uint32) - np.uint32(r0)
        m, inl = w["m"][r0:r1].copy(), w["inlier"][r0:r1].copy()
        first = int(o[1])
        m[:first], inl[:first] = tu.match_rows(o)[:first], 0
        has = m["train_row"] >= 0
        m["train_row"][has] -= r0
        paired = m["pair"] != capi.FX_MATCH_NO_PAIR
        m["pair"][paired] -= a
        out.append(dict(off=o, rows=w["rows"][r0:r1].copy(), m=m, inlier=inl, reg=w["reg"][a:b].copy(), n_scans=b - a + 1, row0=r0, scan0=a))
    return out


def every(n_scans, step):
    """Edges every `step` scans over a run of n_scans, the last piece ending at the last scan."""
    e = list(range(0, n_scans - 1, step)) + [n_scans - 1]
    return e if len(e) > 1 else [0, n_scans - 1]


def run_reference(pieces, max_landmarks, max_carry_rows, overlap=True, **kw):
    """track_reference -> map_reference over the pieces, each piece's last pose the next one's init_pose.  Returns (state, [the
    piece's track], [its map_id_of_row])."""
    st = capi.map_state(max_landmarks, max_carry_rows)
    tracks, ids = [], []
    for k, p in enumerate(pieces):
        tr = tu.reference(p, init_pose=st["header"]["last_pose"][:5], **kw)
        st, row_ids = capi.map_reference(st, p["off"], p["rows"], tr, overlap=overlap and k > 0)
        tracks.append(tr), ids.append(row_ids)
    return st, tracks, ids


def _bits(a):
    return tu.bits(a) if a.dtype.kind == "f" else a


def assert_equal(got, ref, what=""):
    """Map.records()'s dict `got` against map_state_records' `ref`: integers equal, doubles and rms_xy bit for bit."""
    g, r = dict(got["header"]), dict(ref["header"])
    gp, rp = g.pop("last_pose"), r.pop("last_pose")
    assert g == r, f"{what}: header {g} != {r}"
    assert [float(v).hex() for v in gp[:5]] == [float(v).hex() for v in rp[:5]] and tuple(gp[5:]) == tuple(rp[5:]), f"{what}: last_pose {gp} != {rp}"
    assert got["landmarks"].shape == ref["landmarks"].shape, f"{what}: {got['landmarks'].shape} != {ref['landmarks'].shape}"
    for f in capi.MAP_LANDMARK_DTYPE.names:
        bad = np.flatnonzero(_bits(got["landmarks"][f]) != _bits(ref["landmarks"][f]))
        assert not len(bad), f"{what}: landmarks.{f} differs at {bad[:8].tolist()}: got {got['landmarks'][bad[:4]]}, reference {ref['landmarks'][bad[:4]]}"


def assert_whole(recs, whole, what=""):
    """A map's records against ONE track over the whole run (track_records' / track_reference's dict): the same landmarks in the
    same order, n_obs and the global scans equal, x, y, z bit for bit."""
    L, W = recs["landmarks"], whole["landmarks"]
    assert recs["header"]["n_landmarks"] == recs["header"]["n_needed"] == len(L) == len(W) == whole["header"]["n_landmarks"], (what, len(L), len(W))
    assert recs["header"]["n_obs"] == whole["header"]["n_obs"] and recs["header"]["scans"] == whole["header"]["scans"], what
    for f in ("n_obs", "first_scan", "last_scan", "x", "y", "z"):
        bad = np.flatnonzero(_bits(L[f]) != _bits(W[f]))
        assert not len(bad), f"{what}: {f} differs from the whole run's at {bad[:8].tolist()}: {L[bad[:4]]} against {W[bad[:4]]}"
    seg = whole["poses"]["segment"]
    assert (L["segment"] == seg[W["first_scan"]]).all() and recs["header"]["segments"] == int(seg[whole["header"]["scans"] - 1]) + 1, what


def assert_rows_map_to_whole(pieces, ids, whole, what="", min_obs=2):
    """map_id_of_row of every piece against landmark_of_row of the whole run: ids are the whole run's landmark numbers.  A row
    whose landmark has fewer than min_obs observations inside the piece (a track that starts at the piece's last scan or ends at
    its first) is in no landmark of that batch and reports -1 there; every landmark row gets its id in at least one piece."""
    L = whole["landmarks"]
    seen = np.zeros(len(whole["landmark_of_row"]), bool)
    for p, row_ids in zip(pieces, ids):
        a, b, r0, n = p["scan0"], p["scan0"] + p["n_scans"] - 1, p["row0"], len(p["rows"])
        want = whole["landmark_of_row"][r0:r0 + n].copy()
        lm = np.flatnonzero(want >= 0)
        inside = np.minimum(L["last_scan"][want[lm]].astype(np.int64), b) - np.maximum(L["first_scan"][want[lm]].astype(np.int64), a) + 1
        want[lm[inside < min_obs]] = -1
        bad = np.flatnonzero(row_ids[:n] != want)
        assert not len(bad) and (row_ids[n:] == -1).all(), f"{what}: piece at scan {a}: rows {bad[:8].tolist()} give {row_ids[bad[:8]]}, the whole run {want[bad[:8]]}"
        seen[r0:r0 + n] |= want >= 0
    assert (seen == (whole["landmark_of_row"] >= 0)).all(), what


def independent_rms(w, whole):
    """rms_xy of the whole run's landmarks by a two-pass fp64 numpy computation over the same observations, and the magnitude of
    their coordinates."""
    P, off = whole["poses"], [int(x) for x in w["off"]]
    scan = np.repeat(np.arange(len(off) - 1), np.diff(off))
    out, mag = [], []
    for lm in whole["landmarks"]:
        q = whole["obs_row"][lm["obs0"]:lm["obs0"] + lm["n_obs"]].astype(np.int64)
        b = scan[q]
        x, y = w["rows"][q, 0].astype(np.float64), w["rows"][q, 1].astype(np.float64)
        wx, wy = (P["c"][b] * x - P["s"][b] * y) + P["tx"][b], (P["s"][b] * x + P["c"][b] * y) + P["ty"][b]
        out.append(np.sqrt(np.mean((wx - wx.mean()) ** 2 + (wy - wy.mean()) ** 2)))
        mag.append(max(np.abs(wx).max(), np.abs(wy).max()))
    return np.array(out), np.array(mag)
