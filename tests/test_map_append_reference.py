"""fx_map_append without a GPU: the new symbols and their host refusals, and capi.map_append_reference, the executable statement
of include/fx.h's clauses.  The yardstick that does not come from the append's own code: a run fed to a map in two sessions and
appended equals, snapshot byte for snapshot byte, ONE reference run over all pieces in which the second session's first piece is
fed without FX_MAP_OVERLAP (fx_map_update's promise that the cut of a run into batches does not show)."""
import ctypes as C

from feature_extraction_amd import build, capi
from tests import map_append_util as au
from tests import map_join_util as ju
from tests import map_merge_util as mm

A, CD, EMPTY, OVER, NOROOM, LONG, TOP = au.A, au.CD, au.EMPTY, au.OVER, au.NOROOM, au.LONG, au.TOP


# ---- the symbols and the host refusals
def test_symbols_sizes_and_version(fxlib):
    for name in ("fx_map_append", "fx_map_append_host"):
        assert name in capi.EXPORTS and hasattr(fxlib, name), name
    assert C.sizeof(capi.FxMapAppendResult) == 32 == capi.APPEND_DTYPE.itemsize
    assert fxlib.fx_version() == 7, "added symbols only: the minor version stays"
    assert "fx_map_append.hip" in build.SOURCES
    assert (A, CD, EMPTY, OVER, NOROOM, LONG) == (0x1, 0x2, 0x4, 0x8, 0x10, 0x20)


def test_null_arguments_and_the_same_map_are_refused_without_a_device(fxlib):
    # (the handles are never read: the refusals come before anything looks at them)
    room = C.create_string_buffer(256)
    h = [C.addressof(room) + 64 * k for k in range(3)]
    snap = capi.map_snapshot_pack(au.hand(2))
    for args in ((None, h[1], h[2], None), (h[0], None, h[2], None), (h[0], h[1], None, None)):
        assert fxlib.fx_map_append(*args) == capi.FX_ERR_INVALID_ARG and b"null" in fxlib.fx_last_error(), args
    assert fxlib.fx_map_append(h[0], h[1], h[1], None) == capi.FX_ERR_INVALID_ARG and b"same map" in fxlib.fx_last_error()
    for args in ((None, h[1], snap, len(snap), None), (h[0], None, snap, len(snap), None), (h[0], h[1], None, len(snap), None)):
        assert fxlib.fx_map_append_host(*args) == capi.FX_ERR_INVALID_ARG and b"null" in fxlib.fx_last_error(), args


# ---- equal to one run
def _worlds():
    return [("flicker", mm.flicker()[1], mm.FLICKER), ("join", ju.world()[1], ju.WORLD)]


def test_a_run_in_two_sessions_appended_equals_the_one_run():
    n = 0
    for name, pieces, f in _worlds():
        for cut in au.cuts(pieces):
            a, b, one = au.two_sessions(pieces, cut, f["cap"], f["carry"])
            before = (capi.map_snapshot_pack(a), capi.map_snapshot_pack(b))
            st, res = capi.map_append_reference(a, b)
            assert capi.map_snapshot_pack(st) == capi.map_snapshot_pack(one), f"{name}, cut before piece {cut}"
            assert res == dict(id_base=a["header"]["n_landmarks"], scan_base=a["header"]["scans"], segment_base=a["header"]["segments"],
                               appended=b["header"]["n_landmarks"], flags=A, carry_rows=b["header"]["carry_rows"], reserved=0)
            assert (capi.map_snapshot_pack(a), capi.map_snapshot_pack(b)) == before, "neither state is modified"
            n += 1
        if name == "join":
            assert one["header"]["segments"] == 3, "the broken run: the bad link and the cut each start a segment"
    assert n == 8


# ---- the clauses on hand-built states
def _records(st):
    return capi.map_state_records(st)["landmarks"]


def test_a_merged_source_has_its_alias_words_offset():
    src, dst = au.merged_flicker(), au.hand(5, cap=128)
    st, res = capi.map_append_reference(dst, src)
    N, M = 5, len(src["landmarks"])
    assert res["flags"] == A and res["id_base"] == N and res["appended"] == M
    roots = [i for i in range(M) if src["alias"][i] < 0]
    absorbed = [i for i in range(M) if src["alias"][i] >= 0]
    assert roots and absorbed
    assert all(st["alias"][N + i] == -1 for i in roots) and all(st["alias"][N + i] == src["alias"][i] + N for i in absorbed)
    assert st["alias"][:N] == [-1] * N
    got, ref = _records(st), _records(src)
    for f in ("x", "y", "z", "rms_xy", "n_obs", "flags"):
        assert got[f][N:].tobytes() == ref[f].tobytes(), f
    Sd, Gd = dst["header"]["scans"], dst["header"]["segments"]
    assert (got["first_scan"][N:] == ref["first_scan"] + Sd).all() and (got["last_scan"][N:] == ref["last_scan"] + Sd).all()
    assert (got["segment"][N:] == ref["segment"] + Gd).all()
    assert st["acc"][N:] == src["acc"]
    assert st["carry"] == [c + N if c >= 0 else -1 for c in src["carry"]] and any(c >= 0 for c in src["carry"])


def test_a_merged_target_is_untouched_below_n():
    dst, src = au.merged_flicker(), au.hand(7, salt=3)
    st, res = capi.map_append_reference(dst, src)
    N = len(dst["landmarks"])
    assert res["flags"] == A and st["header"]["n_landmarks"] == N + 7
    assert st["alias"][:N] == dst["alias"] and st["landmarks"][:N] == dst["landmarks"] and st["acc"][:N] == dst["acc"]
    assert st["alias"][N:] == [-1] * 7
    assert st["header"]["flags"] == dst["header"]["flags"] | src["header"]["flags"]
    assert st["header"]["carry_rows"] == 0 and st["carry"] == [], "the target's former carry is gone: its run has ended"


def test_the_carry_fits_exactly_or_is_dropped():
    _, b, _ = au.flicker_sessions()
    r = b["header"]["carry_rows"]
    assert r > 1
    fits, res = capi.map_append_reference(au.hand(3, cap=128, carry=r), b)
    assert res["flags"] == A and res["carry_rows"] == r == fits["header"]["carry_rows"]
    assert fits["carry"] == [c + 3 if c >= 0 else -1 for c in b["carry"]] and (fits["carry_kp"] == b["carry_kp"]).all()
    drop, res = capi.map_append_reference(au.hand(3, cap=128, carry=r - 1), b)
    assert res["flags"] == A | CD and res["carry_rows"] == 0 == drop["header"]["carry_rows"] and drop["carry"] == [] and len(drop["carry_kp"]) == 0
    assert drop["landmarks"] == fits["landmarks"] and drop["header"]["scans"] == fits["header"]["scans"]


def test_a_source_of_no_landmarks_and_a_target_of_none():
    dst, none = au.hand(4), au.hand(0)
    st, res = capi.map_append_reference(dst, none)
    assert res == dict(id_base=4, scan_base=dst["header"]["scans"], segment_base=dst["header"]["segments"], appended=0, flags=A, carry_rows=0, reserved=0)
    assert st["landmarks"] == dst["landmarks"] and st["header"]["scans"] == dst["header"]["scans"] + 3
    assert st["header"]["segments"] == dst["header"]["segments"] + 1 and st["header"]["batches"] == dst["header"]["batches"] + 1
    # N == 0: the imported source apart from the capacities
    src = au.merged_flicker()
    st, res = capi.map_append_reference(capi.map_state(200, 99), src)
    assert res["flags"] == A and (res["id_base"], res["scan_base"], res["segment_base"]) == (0, 0, 0)
    assert capi.map_snapshot_pack(st) == capi.map_snapshot_pack(src) and (st["max_landmarks"], st["max_carry_rows"]) == (200, 99)


def _refused(dst, src, flags):
    st, res = capi.map_append_reference(dst, src)
    H = dst["header"]
    assert res == dict(id_base=H["n_landmarks"], scan_base=H["scans"], segment_base=H["segments"], appended=0, flags=flags,
                       carry_rows=H["carry_rows"], reserved=0)
    assert capi.map_snapshot_pack(st) == capi.map_snapshot_pack(dst), "a refusal leaves the target bit for bit unchanged"


def test_the_four_refusals():
    dst, src = au.hand(4, cap=16), au.hand(3, salt=2)
    _refused(dst, capi.map_state(4, 4), EMPTY)
    full = au.with_header(src, n_needed=5)
    _refused(dst, full, OVER)
    _refused(au.with_header(dst, n_needed=9), src, OVER)
    assert capi.map_append_reference(au.with_caps(dst, cap=7), src)[1]["flags"] == A, "N + M == max_landmarks fits"
    _refused(au.with_caps(dst, cap=6), src, NOROOM)
    s = src["header"]
    for k in ("scans", "segments", "batches", "n_obs"):
        edge = au.with_header(dst, **{k: TOP - s[k]})
        st, res = capi.map_append_reference(edge, src)
        assert res["flags"] == A and st["header"][k] == TOP, k
        _refused(au.with_header(dst, **{k: TOP - s[k] + 1}), src, LONG)
    _refused(au.with_header(dst, n_needed=9), capi.map_state(4, 4), EMPTY | OVER)
    _refused(au.with_caps(au.with_header(dst, scans=TOP), cap=6), full, OVER | NOROOM | LONG)


def test_an_append_of_an_append():
    a, b, c = au.hand(3, cap=64), au.hand(4, salt=1), au.hand(5, salt=2)
    ab, r1 = capi.map_append_reference(a, b)
    abc, r2 = capi.map_append_reference(ab, c)
    assert (r2["id_base"], r2["scan_base"], r2["segment_base"]) == (7, a["header"]["scans"] + b["header"]["scans"], a["header"]["segments"] + b["header"]["segments"])
    bc, r3 = capi.map_append_reference(au.with_caps(b, cap=64), c)
    other, r4 = capi.map_append_reference(a, bc)
    assert capi.map_snapshot_pack(abc) == capi.map_snapshot_pack(other), "(a + b) + c and a + (b + c) are one map"
    assert r4["appended"] == 9 and abc["header"]["n_landmarks"] == 12


# ---- the chain: two sessions of one place brought into one frame
def test_the_chain_brings_two_sessions_into_one_map():
    a, b = au.chain_sessions()
    assert (len(a["landmarks"]), len(b["landmarks"])) == (41, 41)
    c = au.chain_reference(a, b)
    st, app = c["appended"]
    assert app["flags"] == A and app["segment_base"] == 1 and st["header"]["segments"] == 2
    rec = c["find"]["rec"]
    assert (int(rec["flags"]), int(rec["score"]), int(rec["runner_up"])) == (capi.FX_FIND_VALID, 41, 8)
    join = c["joined"][1]
    assert int(join["flags"]) == 0x21 and int(join["n_inliers"]) == 41 and round(float(join["rms"]), 4) == 0.0105
    merges = c["merged"][1]
    assert len(ju.live(st)) == 82 and merges[-2]["live"] == 38
    alone, _ = mm.merge_to_fixpoint(a, max_gap_scans=1 << 20)
    alone = capi.map_compact_reference(alone)[2]
    comp = c["compacted"][1]
    assert comp["kept"] == 38 == alone["kept"], "the merged, compacted map has as many live landmarks as session A alone"
    assert c["compacted"][0]["header"]["segments"] == 1 and c["compacted"][0]["header"]["n_landmarks"] == 38
