"""The map's snapshot, the part that needs no GPU: capi.map_snapshot_pack / map_snapshot_parse — the layout of include/fx.h's
"The snapshot" clause in Python — and the library's host-only fx_map_snapshot_check on blocks packed here and then damaged."""
import struct

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_compact_util as mc
from tests import map_merge_util as mm
from tests import map_util as mu

OK, INVALID, TOO_LARGE = capi.FX_OK, capi.FX_ERR_INVALID_ARG, capi.FX_ERR_TOO_LARGE


@pytest.fixture(scope="module")
def merged():
    """The flicker world after piece 3 and a merge to the fixpoint: alias entries >= 0 and a carry that continues landmarks."""
    w, pieces, _ = mm.flicker()
    f = mm.FLICKER
    st, _, _ = mu.run_reference(pieces[:4], f["cap"], f["carry"])
    st, _ = mm.merge_to_fixpoint(st, max_gap_scans=mc.GAP)
    assert any(a >= 0 for a in st["alias"]) and any(c >= 0 for c in st["carry"]) and st["header"]["carry_rows"] == len(st["carry"]) > 0
    return st


def _offsets(n, r):
    up = lambda b: (b + 15) & ~15
    o_rec = 64 + 96
    o_acc = o_rec + 48 * n
    o_alias = o_acc + 64 * n
    o_carry = o_alias + up(4 * n)
    o_kp = o_carry + up(4 * r)
    return dict(hdr=64, rec=o_rec, acc=o_acc, alias=o_alias, carry=o_carry, kp=o_kp, total=o_kp + 16 * r)


def test_layout_word_for_word(merged):
    st = merged
    blob = capi.map_snapshot_pack(st)
    n, r = st["header"]["n_landmarks"], st["header"]["carry_rows"]
    o = _offsets(n, r)
    assert len(blob) == o["total"] and len(blob) % 16 == 0
    assert struct.unpack_from("<10IQ", blob) == (0x504D5846, 1, capi.FX_HEADER_VERSION, 64, n, r, 88, 48, 8, 0, len(blob))
    assert blob[:4] == b"FXMP" and blob[48:64] == bytes(16) and blob[64 + 88:64 + 96] == bytes(8)
    assert struct.unpack_from("<10I", blob, 64) == tuple(st["header"][k] for k in capi.MAP_HEADER_FIELDS)
    assert blob[o["rec"]:o["acc"]] == capi.map_state_records(st)["landmarks"].tobytes()
    assert blob[o["acc"]:o["alias"]] == np.array(st["acc"], "<f8").tobytes()
    assert np.frombuffer(blob, "<i4", n, o["alias"]).tolist() == st["alias"] and blob[o["alias"] + 4 * n:o["carry"]] == bytes(-4 * n % 16)
    assert np.frombuffer(blob, "<i4", r, o["carry"]).tolist() == st["carry"] and blob[o["carry"] + 4 * r:o["kp"]] == bytes(-4 * r % 16)
    assert blob[o["kp"]:] == st["carry_kp"].tobytes()


def test_parse_round_trips_the_state(merged):
    for st in (merged, capi.map_compact_reference(merged)[0], capi.map_state(8, 8)):
        blob = capi.map_snapshot_pack(st)
        back = capi.map_snapshot_parse(blob, st["max_landmarks"], st["max_carry_rows"])
        n = st["header"]["n_landmarks"]
        assert back["header"] == st["header"] and back["carry"] == list(st["carry"]) and (back["carry_kp"] == st["carry_kp"]).all()
        assert back["alias"] == (list(st.get("alias", [])) + [-1] * n)[:n] and (back["max_landmarks"], back["max_carry_rows"]) == (st["max_landmarks"], st["max_carry_rows"])
        assert mm.state_bytes(back) == mm.state_bytes(dict(st, alias=back["alias"])) and capi.map_snapshot_pack(back) == blob
    # the references go on from a parsed state as from the original
    a, ra = capi.map_compact_reference(merged)[0], capi.map_compact_reference(merged)[2]
    b, _, rb = capi.map_compact_reference(capi.map_snapshot_parse(capi.map_snapshot_pack(merged), merged["max_landmarks"], merged["max_carry_rows"]))
    assert mm.state_bytes(a) == mm.state_bytes(b) and ra == rb
    with pytest.raises(ValueError):
        capi.map_snapshot_parse(capi.map_snapshot_pack(merged)[:-1])
    with pytest.raises(ValueError):
        capi.map_snapshot_pack(dict(merged, carry=merged["carry"][:-1]))


def _check(fxlib, blob, cap, carry):
    status = fxlib.fx_map_snapshot_check(bytes(blob), len(blob), cap, carry)
    return status, fxlib.fx_last_error().decode() if status else ""


def test_check_accepts_and_refuses_each_with_its_reason(fxlib, merged):
    st = merged
    f = mm.FLICKER
    blob = capi.map_snapshot_pack(st)
    n, r = st["header"]["n_landmarks"], st["header"]["carry_rows"]
    o = _offsets(n, r)
    assert _check(fxlib, blob, f["cap"], f["carry"]) == (OK, "") and _check(fxlib, blob, n, r) == (OK, "")
    assert _check(fxlib, capi.map_snapshot_pack(capi.map_state(8, 8)), 1, 0) == (OK, "")

    def damaged(at, fmt, value):
        b = bytearray(blob)
        struct.pack_into(fmt, b, at, value)
        return b
    absorbed = next(i for i, a in enumerate(st["alias"]) if a >= 0)
    live = [i for i, a in enumerate(st["alias"]) if a == -1]
    chain = bytearray(damaged(o["alias"] + 4 * live[0], "<i", live[1]))  # alias[a] = b, alias[b] = c
    struct.pack_into("<i", chain, o["alias"] + 4 * live[1], live[2])
    cases = [("wrong magic", damaged(0, "<I", 0x504D5847), INVALID, "magic"),
             ("wrong format", damaged(4, "<I", 2), INVALID, "format 2"),
             ("a struct size", damaged(28, "<I", 56), INVALID, "struct sizes"),
             ("one byte short", blob[:-1], INVALID, f"{len(blob) - 1} given"),
             ("total against the sections", damaged(40, "<Q", len(blob) + 16) + bytes(16), INVALID, "sections sum"),
             ("n against the header", damaged(64, "<I", n - 1), INVALID, "counts differ"),
             ("alias == n", damaged(o["alias"] + 4 * absorbed, "<i", n), INVALID, f"alias[{absorbed}] = {n} is outside"),
             ("alias below -1", damaged(o["alias"], "<i", -2), INVALID, "alias[0] = -2 is outside"),
             ("alias chain", chain, INVALID, f"alias[{live[0]}] = {live[1]} is not resolved"),
             ("carry == n", damaged(o["carry"], "<i", n), INVALID, f"carry[0] = {n} is outside"),
             ("n_landmarks above n_needed", damaged(64 + 4, "<I", n - 1), INVALID, "exceeds n_needed")]
    reasons = set()
    for name, b, status, word in cases:
        got = _check(fxlib, b, f["cap"], f["carry"])
        assert got[0] == status and word in got[1], (name, got)
        reasons.add(got[1])
    assert len(reasons) == len(cases), "each refusal has its own reason"
    got = _check(fxlib, blob, n - 1, f["carry"])
    assert got[0] == TOO_LARGE and f"{n} landmarks, max_landmarks {n - 1}" in got[1], got
    got = _check(fxlib, blob, f["cap"], r - 1)
    assert got[0] == TOO_LARGE and f"{r} carry rows, max_carry_rows {r - 1}" in got[1], got
    assert fxlib.fx_map_snapshot_check(None, 64, 1, 1) == INVALID and _check(fxlib, blob[:63], 1, 1)[0] == INVALID
    # a map that overflowed goes into a map of the same max_landmarks only
    over = damaged(64 + 4, "<I", n + 5)
    assert _check(fxlib, over, n, f["carry"]) == (OK, "")
    got = _check(fxlib, over, f["cap"], f["carry"])
    assert got[0] == INVALID and "fx_map_compact" in got[1] and f"n_needed {n + 5}" in got[1], got
