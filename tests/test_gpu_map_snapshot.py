"""fx_map_export_host / fx_map_import_host on the GPU: a map's snapshot against capi.map_snapshot_pack of the reference state, byte
for byte; a map imported into another context (and a larger map) goes on exactly as its source; a refused import changes nothing."""
import ctypes as C
import struct

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_compact_util as mc
from tests import map_merge_util as mm
from tests.test_gpu_map import _run, _step
from tests.test_gpu_map_compact import _same_state
from tests.test_gpu_map_localize import _call as _localize
from tests.test_gpu_map_merge import _merge_to_fixpoint
from tests.test_gpu_track import _upload

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def test_a_fresh_map_a_used_one_and_after_a_reset(ctx, fxlib):
    f = mm.FLICKER
    mp = ctx.map_create(f["cap"], f["carry"])
    fresh = capi.map_snapshot_pack(capi.map_state(f["cap"], f["carry"]))
    assert mp.export_state() == fresh and len(fresh) == 64 + 96
    _, pieces, _ = mm.flicker()
    st, _, _, _ = _run(ctx, pieces[:2], "(a)", f["cap"], f["carry"], mp=mp)
    _same_state(mp, st, "(a) after two batches")  # (the sums and the carry scan, which no other call shows)
    blob = mp.export_state()
    # the size query, a capacity that is too small, NULL arguments
    n = C.c_size_t(0)
    assert fxlib.fx_map_export_host(ctx.handle, mp.handle, None, 0, C.byref(n)) == capi.FX_OK and n.value == len(blob)
    buf = C.create_string_buffer(b"\x5a" * len(blob), len(blob))
    n = C.c_size_t(0)
    assert fxlib.fx_map_export_host(ctx.handle, mp.handle, buf, len(blob) - 1, C.byref(n)) == capi.FX_ERR_TOO_LARGE
    assert n.value == len(blob) and buf.raw == b"\x5a" * len(blob) and b"capacity" in fxlib.fx_last_error()
    assert fxlib.fx_map_export_host(ctx.handle, mp.handle, None, 8, C.byref(n)) == capi.FX_ERR_INVALID_ARG
    assert fxlib.fx_map_export_host(None, mp.handle, buf, len(blob), C.byref(n)) == capi.FX_ERR_INVALID_ARG
    assert fxlib.fx_map_import_host(ctx.handle, mp.handle, None, 0) == capi.FX_ERR_INVALID_ARG
    mp.reset()
    assert mp.export_state() == fresh
    mp.close()


def test_b_an_imported_map_goes_on_as_its_source(ctx):
    f = mm.FLICKER
    _, pieces, _ = mm.flicker()
    src = ctx.map_create(f["cap"], f["carry"])
    st, _, _, _ = _run(ctx, pieces[:3], "(b)", f["cap"], f["carry"], mp=src)
    st, _ = _merge_to_fixpoint(ctx, src, st, "(b)", max_gap_scans=mc.GAP)
    blob = src.export_state()
    assert blob == capi.map_snapshot_pack(st) and any(a >= 0 for a in st["alias"]) and any(c >= 0 for c in st["carry"])
    other = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    dst = other.map_create(2 * f["cap"] + 1, f["carry"] + 3)
    data = bytearray(blob)
    dst.import_state(data)
    data[:] = bytes(len(data))  # (the caller's bytes are free once the call returns)
    assert dst.export_state() == blob
    assert (dst.alias()[st["header"]["n_landmarks"]:] == -1).all()
    # the same next batch with overlap, a merge round, a localisation: everything byte-equal
    p = pieces[3]
    dev_in = _upload(p, p["n_scans"] + 2, len(p["rows"]) + 9)
    outs = []
    for c, mp in ((ctx, src), (other, dst)):
        s, tr, ids = _step(c, mp, dict(st, max_landmarks=mp.max_landmarks, max_carry_rows=mp.max_carry_rows), p, True, "(b) the next batch", dev_in=dev_in)
        assert s["header"]["last_joined"] > 0 and not s["header"]["flags"] & capi.FX_MAP_OVERLAP_MISMATCH, "the overlap is accepted"
        s, _ = _merge_to_fixpoint(c, mp, s, "(b) merge", max_gap_scans=mc.GAP)
        import torch
        pri = torch.from_numpy(np.ascontiguousarray(tr["poses"]).view(np.float64).reshape(-1, 6).copy()).to(f"cuda:{c.device}")
        loc = _localize(c, mp, dev_in[0], pri, p["n_scans"], len(p["rows"]), segment=capi.FX_LOC_ANY_SEGMENT)
        assert (loc["rec"]["flags"] & capi.FX_LOC_VALID).any()
        s, remap, _ = capi.map_compact_reference(s)
        rm, _ = mp.compact(result=False)
        c.synchronize()
        outs.append((mp.export_state(), ids.tobytes(), loc["rec"].tobytes(), loc["map_id_of_row"].tobytes(), loc["nearest_of_row"].tobytes(),
                     rm.cpu().numpy()[:f["cap"]].tobytes()))
        assert outs[-1][0] == capi.map_snapshot_pack(s)
    assert outs[0] == outs[1]
    src.close(), dst.close(), other.close()


def test_c_a_refused_import_leaves_the_target_unchanged(ctx, fxlib):
    f = mm.FLICKER
    _, pieces, _ = mm.flicker()
    src = ctx.map_create(f["cap"], f["carry"])
    st, _, _, _ = _run(ctx, pieces[:2], "(c)", f["cap"], f["carry"], mp=src)
    st, _ = _merge_to_fixpoint(ctx, src, st, "(c)", max_gap_scans=mc.GAP)
    blob = src.export_state()
    n, r = st["header"]["n_landmarks"], st["header"]["carry_rows"]
    small = ctx.map_create(n - 1, f["carry"])
    few = ctx.map_create(f["cap"], r - 1)
    other = mm.fragments([(0, 1.0, 2.0), (3, 1.0, 2.0)], 5)
    for mp in (small, few):
        mine, _, _ = _step(ctx, mp, capi.map_state(mp.max_landmarks, mp.max_carry_rows), other, False, "(c) the target's own state")
        before = mp.export_state()
        with pytest.raises(capi.FxError, match="status 5"):
            mp.import_state(blob)
        assert b"snapshot:" in fxlib.fx_last_error() and (b"max_landmarks" if mp is small else b"max_carry_rows") in fxlib.fx_last_error()
        assert mp.export_state() == before
    # a corrupted alias word: into the map the snapshot came from
    absorbed = next(i for i, a in enumerate(st["alias"]) if a >= 0)
    o_alias = 64 + 96 + 48 * n + 64 * n
    bad = bytearray(blob)
    struct.pack_into("<i", bad, o_alias + 4 * absorbed, n)
    with pytest.raises(capi.FxError, match="status 1"):
        src.import_state(bad)
    assert f"alias[{absorbed}] = {n} is outside".encode() in fxlib.fx_last_error() and src.export_state() == blob
    with pytest.raises(capi.FxError, match="status 1"):
        src.import_state(blob[:-16])
    assert src.export_state() == blob
    # and the block itself goes back in
    src.reset()
    src.import_state(blob)
    assert src.export_state() == blob
    src.close(), small.close(), few.close()
