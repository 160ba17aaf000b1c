"""Helpers of the map compaction and snapshot tests (tests/test_map_compact_reference.py, tests/test_map_snapshot.py and their GPU
twins): hand-built fragments of chosen lengths, the flicker world run with a compaction in the middle, and the id mapping a
compaction leaves between a compacted run and an uncompacted one."""
import numpy as np

from feature_extraction_amd import capi
from tests import map_merge_util as mm
from tests import track_util as tu

GAP = 24  # max_gap_scans of the flicker world's merges (tests/test_map_merge_reference.py)
FLICKER_LIVE = 33  # live landmarks of the flicker world after the merge's fixpoint (checked on the CPU)


def fragments(frags, n_scans, seed=7):
    """map_merge_util.fragments with a length a fragment: frags = [(first_scan, length, x, y)].  Tracks of one observation are
    landmarks only for a track run with min_obs = 1."""
    h = tu.Hand(n_scans)
    chains = [h.chain(int(fs), int(n)) for fs, n, _, _ in frags]
    w = h.finish(np.random.default_rng(seed), motions=[(0.0, 0.0, 0.0, 0.0)] * (n_scans - 1))
    for (_, _, x, y), ch in zip(frags, chains):
        for r in ch:
            w["rows"][w["at"](r), :3] = (x, y, 1.0)
    w["chains"] = chains
    return w


def alternating(n, spacing=5.0, apart=0.1):
    """mm.fragments case of n landmarks in which one merge absorbs every second one: pair k is a root in scans 2 k, 2 k + 1 at
    (spacing k, 0) and a member in scans 2 k + 2, 2 k + 3 `apart` beside it.  Member k and root k + 1 begin at the same scan and ids
    follow (first_scan, order given): root 0, member 0, root 1, member 1, ...; an odd n ends with a single landmark."""
    P = n // 2
    F32 = lambda v: float(np.float32(v))
    frags = []
    for k in range(P):
        frags += ([(2 * k, F32(spacing * (k - 1) + apart), 0.0)] if k else []) + [(2 * k, F32(spacing * k), 0.0)]
    if P:
        frags.append((2 * P, F32(spacing * (P - 1) + apart), 0.0))
    if n % 2:
        frags.append((2 * P, F32(spacing * P), 0.0))
    return mm.fragments(frags, 2 * P + 2)


def kept_last(n_old=300, n_young=40):
    """A case for a track of min_obs = 1: n_old landmarks of one observation in scan 0 and n_young of two in scans 3-4, 5 m apart.
    compact(min_obs=2, min_age_scans=2) keeps the young ones only: all of them in the map's last workgroup of 256."""
    F32 = lambda v: float(np.float32(v))
    return fragments([(0, 1, F32(5.0 * k), 0.0) for k in range(n_old)] + [(3, 2, F32(5.0 * k), 50.0) for k in range(n_young)], 5)


def rank_of_live(alias):
    """old id -> new id of a compaction that drops exactly the absorbed landmarks: the number of live ones below (-1: absorbed)."""
    a = np.asarray(alias, np.int64)
    live = a == -1
    return np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)


def through(remap, ids):
    """map_id_of_row words through a remap array."""
    ids = np.asarray(ids).astype(np.int64)
    out = np.full(len(ids), -1, np.int32)
    has = ids >= 0
    out[has] = np.asarray(remap)[ids[has]]
    return out


def assert_moved(old, new, remap, what=""):
    """Every kept landmark of state `old` is, bit for bit, landmark remap[i] of state `new`: record and sums."""
    L0, L1 = capi.map_state_records(old)["landmarks"], capi.map_state_records(new)["landmarks"]
    alias = list(old.get("alias", [])) + [-1] * (len(L0) - len(old.get("alias", [])))
    kept = 0
    for i in range(len(L0)):
        if alias[i] != -1 or remap[i] < 0:
            continue
        k = int(remap[i])
        assert L0[i].tobytes() == L1[k].tobytes(), f"{what}: record {i} -> {k}"
        assert [float(v).hex() for v in old["acc"][i]] == [float(v).hex() for v in new["acc"][k]], f"{what}: sums {i} -> {k}"
        kept += 1
    assert kept == len(L1), f"{what}: {kept} landmarks moved, {len(L1)} stored"


def flicker_runs(k=2):
    """The flicker world run twice on the CPU: pieces 0 .. k, the merge's fixpoint, then the remaining pieces — once as it is and
    once with a compaction behind the merge.  Returns a dict: pieces, the two final states, the two lists of map_id_of_row, remap,
    the states before and after the compaction, N0 and K0 there."""
    w, pieces, _ = mm.flicker()
    f = mm.FLICKER
    st = capi.map_state(f["cap"], f["carry"])
    ids = []
    for j, p in enumerate(pieces[:k + 1]):
        tr = tu.reference(p, init_pose=st["header"]["last_pose"][:5])
        st, row_ids = capi.map_reference(st, p["off"], p["rows"], tr, overlap=j > 0)
        ids.append(row_ids)
    st, _ = mm.merge_to_fixpoint(st, max_gap_scans=GAP)
    cst, remap, res = capi.map_compact_reference(st)
    out = dict(w=w, pieces=pieces, before=st, after=cst, remap=remap, result=res, ids_head=ids)
    for name, s in (("plain", st), ("compacted", cst)):
        tail = []
        for j, p in enumerate(pieces[k + 1:], start=k + 1):
            tr = tu.reference(p, init_pose=s["header"]["last_pose"][:5])
            s, row_ids = capi.map_reference(s, p["off"], p["rows"], tr, overlap=True)
            tail.append((row_ids, dict(s["header"])))
        out[name], out[name + "_tail"] = s, tail
    return out


def id_mapping(remap, n0, k0, n_final):
    """old id -> id in the compacted run for a run that went on after the compaction: remap below n0, and the landmarks made
    afterwards keep their order behind the k0 kept ones."""
    m = np.full(n_final, -1, np.int32)
    m[:n0] = remap[:n0]
    m[n0:] = k0 + np.arange(n_final - n0)
    return m
