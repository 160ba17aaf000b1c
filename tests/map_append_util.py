"""Helpers of the map append tests (tests/test_map_append_reference.py, tests/test_gpu_map_append.py): a run fed to a map in two
sessions (each with a fresh state; the second starts where the first ended), whole states compared through their snapshots,
hand-built states of chosen sizes, and the comparison of a device append with capi.map_append_reference."""
import math

import numpy as np

from feature_extraction_amd import capi
from tests import map_find_loop_util as fu
from tests import map_join_util as ju
from tests import map_merge_util as mm
from tests import map_util as mu
from tests import track_util as tu

A, CD, EMPTY, OVER, NOROOM, LONG = (capi.FX_APPEND_APPLIED, capi.FX_APPEND_CARRY_DROPPED, capi.FX_APPEND_EMPTY, capi.FX_APPEND_OVERFLOWED,
                                    capi.FX_APPEND_NO_ROOM, capi.FX_APPEND_TOO_LONG)
TOP = 0xffffffff
# the chain's second session: the join world seen again with fresh noise, cut elsewhere, from another start
CHAIN = dict(sigma=0.02, seed=99, step=7, init_pose=(math.cos(0.7), math.sin(0.7), 40.0, -25.0, 0.5))


def fresh(cap, carry, init_pose=None):
    """The state of a fresh map whose first track starts at init_pose (default: the identity): feed() hands a state's last_pose to
    the next track, and the first update overwrites it."""
    st = capi.map_state(cap, carry)
    if init_pose is not None:
        st["header"]["last_pose"] = tuple(float(v) for v in tuple(init_pose)[:5]) + (0, 0)
    return st


def feed(st, pieces, flags=None, **kw):
    """track_reference -> map_reference over the pieces into the state st, each track's init pose the state's last_pose; flags[k]:
    FX_MAP_OVERLAP of piece k (default: all but the first).  Returns (the new state, [the piece's map_id_of_row])."""
    ids = []
    for k, p in enumerate(pieces):
        tr = tu.reference(p, init_pose=st["header"]["last_pose"][:5], **kw)
        st, row_ids = capi.map_reference(st, p["off"], p["rows"], tr, overlap=(k > 0) if flags is None else flags[k])
        ids.append(row_ids)
    return st, ids


def two_sessions(pieces, cut, cap, carry):
    """The run in two sessions cut before piece `cut`, and in one.  Returns (A: pieces[:cut] into a fresh map, B: pieces[cut:] into
    another fresh map from A's last_pose, the one run over all pieces with piece `cut` fed without FX_MAP_OVERLAP)."""
    a, _ = feed(fresh(cap, carry), pieces[:cut])
    b, _ = feed(fresh(cap, carry, a["header"]["last_pose"]), pieces[cut:])
    one, _ = feed(fresh(cap, carry), pieces, flags=[k > 0 and k != cut for k in range(len(pieces))])
    return a, b, one


def cuts(pieces):
    return list(range(1, len(pieces)))


def same(a, b):
    """Two states hold the same map: their snapshots are the same bytes (records, sums, alias, carry, the carry scan, the header)."""
    return capi.map_snapshot_pack(a) == capi.map_snapshot_pack(b)


def with_caps(st, cap=None, carry=None):
    """The state in a map of other capacities."""
    return dict(st, max_landmarks=st["max_landmarks"] if cap is None else int(cap), max_carry_rows=st["max_carry_rows"] if carry is None else int(carry))


def with_header(st, **words):
    st = dict(st, header=dict(st["header"]))
    st["header"].update(words)
    return st


def hand(n, salt=0, cap=None, carry=8):
    """A hand-built state of n landmarks, each of its own bytes: positions, scans and segments differ from landmark to landmark and
    with `salt`.  n == 0: a run of three scans that found nothing (scans > 0)."""
    if n == 0:
        st = with_header(capi.map_state(1, carry), scans=3, batches=1, segments=1)
    else:
        st = fu.state([(ju.F32(1.5 * k + salt), ju.F32(0.25 * k - salt), (k + salt) % 7, (k + salt) % 7 + 3, k % 3) for k in range(n)])
    return with_caps(st, max(n, 1) if cap is None else cap, carry)


def flicker_sessions():
    """The flicker world in two sessions cut in the middle: (A, B, the one run), B with a carry scan of several rows."""
    f = mm.FLICKER
    _, pieces, _ = mm.flicker()
    return two_sessions(pieces, 2, f["cap"], f["carry"])


def merged_flicker():
    """The flicker world's whole run merged to the fixpoint: alias holds roots (-1) and absorbed landmarks."""
    f = mm.FLICKER
    _, pieces, _ = mm.flicker()
    st, _ = feed(fresh(f["cap"], f["carry"]), pieces)
    st, _ = mm.merge_to_fixpoint(st, max_gap_scans=64)
    assert any(a >= 0 for a in st["alias"]) and any(a < 0 for a in st["alias"])
    return st


def chain_sessions():
    """The two sessions of the chain: A, the join world's unbroken run from the identity; B, the same world with CHAIN's fresh noise
    on the rows' x, y, z, cut every 7 scans, from CHAIN's init pose.  Both in maps of the join world's capacities."""
    f, c = ju.WORLD, CHAIN
    w, _, whole = ju.world()
    a, _ = feed(fresh(f["cap"], f["carry"]), whole)
    w2 = dict(w, rows=w["rows"].copy())
    w2["rows"][:, :3] += (c["sigma"] * np.random.default_rng(c["seed"]).standard_normal((len(w2["rows"]), 3))).astype(np.float32)
    b, _ = feed(fresh(f["cap"], f["carry"], c["init_pose"]), mu.split(w2, mu.every(f["n_scans"], c["step"])))
    return a, b


def chain_reference(a, b):
    """append -> find -> join -> merge to the fixpoint -> compact with the references alone.  Returns every step's (state, result)."""
    st, app = capi.map_append_reference(a, b)
    find = capi.map_find_loop_reference(st, segment=fu.LAST, target_segment=0, recent_scans=TOP)
    T = fu.transform_of(find["rec"])
    joined, join, _ = capi.map_join_reference(st, 1, 0, prior=T, search_dist=0.6)
    merged, merges = mm.merge_to_fixpoint(joined, max_gap_scans=1 << 20)
    compacted, _, comp = capi.map_compact_reference(merged)
    return dict(appended=(st, app), find=find, joined=(joined, join), merged=(merged, merges), compacted=(compacted, comp))


def assert_result(got, ref, what=""):
    """A device result record (capi.append_records) against the reference's dict, word for word."""
    g = {k: int(got[k]) for k in ref if k != "reserved"}
    g["reserved"] = int(np.asarray(got["reserved"]).any())
    assert g == ref, f"{what}: result {g}, reference {ref}"


def _append(ctx, dst, dst_st, src_st, what, src=None, data=None):
    """One fx_map_append (src: the source Map, in src_st's state) or fx_map_append_host (data: a snapshot of src_st) into a guarded
    result against one map_append_reference call: the result word for word, dst's snapshot byte for byte, the source and the guard
    words untouched.  Returns (the reference's new state, its result)."""
    import torch
    from tests.test_gpu_map_compact import _same_state
    from tests.test_gpu_track import FILL, GUARD
    res = torch.full((GUARD + 8 + GUARD,), FILL, dtype=torch.int32, device=f"cuda:{ctx.device}")
    out = res[GUARD:GUARD + 8]
    if src is not None:
        before = src.export_state()
        dst.append(src, result=out)
    else:
        dst.append_state(data, result=out)
    ctx.synchronize()
    new, ref = capi.map_append_reference(dst_st, src_st)
    assert (res[:GUARD] == FILL).all().item() and (res[GUARD + 8:] == FILL).all().item(), f"{what}: the guards about the result"
    assert_result(capi.append_records(out), ref, what)
    _same_state(dst, new, what)
    if src is not None:
        assert src.export_state() == before, f"{what}: the source was written"
    return new, ref
