"""fx_map_compact on the GPU.  Every call is compared with capi.map_compact_reference word for word — remap, the result — and the
device map's whole private state with the reference's through the snapshot: Map.export_state() against capi.map_snapshot_pack, byte
for byte (records, sums, alias, carry, the carry scan, the header).  The guard words behind remap and the result must be untouched."""
import ctypes as C

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_compact_util as mc
from tests import map_merge_util as mm
from tests.test_gpu_map import _run, _step
from tests.test_gpu_map_merge import _merge, _merge_to_fixpoint, _one_batch
from tests.test_gpu_track import FILL, GUARD

pytestmark = pytest.mark.gpu
WG = 256  # csrc/fx_map_compact.hip: FXMC_WG landmarks a workgroup, one block of the prefix


@pytest.fixture
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def _same_state(mp, st, what):
    got, ref = mp.export_state(), capi.map_snapshot_pack(st)
    if got != ref:
        g, r = capi.map_snapshot_parse(got), capi.map_snapshot_parse(ref)
        diff = [k for k in ("header", "alias", "carry") if g[k] != r[k]]
        diff += [f"landmark {i}" for i, (a, b) in enumerate(zip(g["landmarks"], r["landmarks"])) if a != b][:4]
        diff += [f"sums {i}" for i, (a, b) in enumerate(zip(g["acc"], r["acc"])) if a != b][:4]
        raise AssertionError(f"{what}: the device's snapshot differs from the reference's: {diff} ({len(got)} and {len(ref)} bytes)")


def _compact(ctx, mp, st, what, **kw):
    """One fx_map_compact into guarded outputs against one map_compact_reference call.  Returns (the new state, remap, result)."""
    import torch
    cap = mp.max_landmarks
    raw = torch.full((cap + GUARD,), FILL, dtype=torch.int32, device=f"cuda:{ctx.device}")
    res = torch.full((4 + GUARD,), FILL, dtype=torch.int32, device=f"cuda:{ctx.device}")
    mp.compact(remap=raw[:cap], result=res[:4], **kw)
    ctx.synchronize()
    st, ref_remap, ref = capi.map_compact_reference(st, **kw)
    assert (raw[cap:] == FILL).all().item() and (res[4:] == FILL).all().item(), f"{what}: the guards behind remap and the result"
    got = dict(zip(capi.MAP_COMPACT_RESULT_FIELDS, res[:4].cpu().numpy().astype(np.uint32).tolist()))
    assert got == ref, f"{what}: result {got}, reference {ref}"
    remap = raw[:cap].cpu().numpy()
    bad = np.flatnonzero(remap != ref_remap)
    assert not len(bad), f"{what}: remap differs at {bad[:8].tolist()}: got {remap[bad[:8]]}, reference {ref_remap[bad[:8]]}"
    _same_state(mp, st, what)
    assert (mp.alias() == -1).all(), f"{what}: the whole alias table is -1"
    return st, remap, got


# ---- (a) the reference's cases on the device
def test_a1_flicker_world_and_equal_bytes_from_run_to_run(ctx):
    w, pieces, _ = mm.flicker()
    f = mm.FLICKER

    def once():
        mp = ctx.map_create(f["cap"], f["carry"])
        pointers = (mp.device_pointers(), mp.alias_device_pointer())
        st, _, _, _ = _run(ctx, pieces, "(a1)", f["cap"], f["carry"], mp=mp)
        st, _ = _merge_to_fixpoint(ctx, mp, st, "(a1)", max_gap_scans=mc.GAP)
        _same_state(mp, st, "(a1) before the compaction: the merged map's private state")
        st, remap, res = _compact(ctx, mp, st, "(a1)")
        assert res == {"before": 54, "kept": mc.FLICKER_LIVE, "dropped_absorbed": 21, "dropped_live": 0}
        assert (mp.device_pointers(), mp.alias_device_pointer()) == pointers, "the map's addresses are stable"
        out = mp.export_state() + remap.tobytes()
        mp.close()
        return out
    assert once() == once()


def test_a2_compaction_commutes_with_the_run(ctx):
    r = mc.flicker_runs(k=2)
    f = mm.FLICKER
    mp, st = ctx.map_create(f["cap"], f["carry"]), capi.map_state(f["cap"], f["carry"])
    for k, p in enumerate(r["pieces"]):
        st, _, ids = _step(ctx, mp, st, p, k > 0, f"(a2) batch {k}")
        if k == 2:
            st, _ = _merge_to_fixpoint(ctx, mp, st, "(a2)", max_gap_scans=mc.GAP)
            st, remap, res = _compact(ctx, mp, st, "(a2)")
            assert (remap == r["remap"]).all() and res == r["result"]
        if k > 2:
            assert (ids == r["compacted_tail"][k - 3][0]).all(), f"(a2) batch {k}: the rows continue what the CPU run's continue"
    assert not st["header"]["flags"] & capi.FX_MAP_OVERLAP_MISMATCH
    _same_state(mp, st, "(a2) at the end")
    assert mm.state_bytes(st) == mm.state_bytes(r["compacted"])
    mp.close()


AGED = [(0, 3, 1.0, 1.0), (4, 1, 11.0, 1.0), (5, 1, 21.0, 1.0), (6, 2, 41.0, 1.0), (7, 1, 31.0, 1.0)]  # tests/test_map_compact_reference.py's _aged


@pytest.mark.parametrize("kw,want,n_obs", [(dict(min_obs=2, min_age_scans=3), [0, -1, 1, 2, 3], 7), (dict(min_obs=2, min_age_scans=2), [0, -1, -1, 1, 2], 6),
                                           (dict(min_obs=2, min_age_scans=0), [0, -1, -1, 1, 2], 6), (dict(min_obs=4, min_age_scans=0), [-1, -1, -1, 0, 1], 3),
                                           ({}, [0, 1, 2, 3, 4], 8)])
def test_a4_min_obs_min_age_scans_and_the_carry(ctx, kw, want, n_obs):
    w = mc.fragments(AGED, 8)
    mp = ctx.map_create(16, 16)
    st, _, _ = _step(ctx, mp, capi.map_state(16, 16), w, False, "(a4)", min_obs=1)
    assert st["header"]["n_obs"] == 8 and st["header"]["n_landmarks"] == 5
    before = mp.export_state()
    st, remap, res = _compact(ctx, mp, st, f"(a4) {kw}", **kw)
    assert remap[:5].tolist() == want and st["header"]["n_obs"] == n_obs and res["dropped_live"] == want.count(-1)
    if not kw:
        assert mp.export_state() == before, "a map with nothing to drop is left bit for bit as it was"
    once = mp.export_state()
    st, remap, res = _compact(ctx, mp, st, f"(a4) {kw}, again", **kw)
    assert mp.export_state() == once and remap[:res["kept"]].tolist() == list(range(res["kept"])), "a second call changes no byte"
    mp.close()


def test_a5_an_empty_map(ctx):
    mp = ctx.map_create(4, 4)
    st, remap, res = _compact(ctx, mp, capi.map_state(4, 4), "(a5) N = 0")
    assert res == {"before": 0, "kept": 0, "dropped_absorbed": 0, "dropped_live": 0} and remap.tolist() == [-1] * 4
    mp.close()


# ---- (b) block edges of the prefix
@pytest.mark.parametrize("n", [WG - 1, WG, WG + 1, 2 * WG + 1])
def test_b_every_second_landmark_absorbed(ctx, n):
    w = mc.alternating(n)
    mp, st = _one_batch(ctx, w, f"(b) {n}", cap=n, carry=8)
    assert st["header"]["n_landmarks"] == n
    st, res = _merge(ctx, mp, st, f"(b) {n}")
    assert res["merged"] == n // 2 and st["alias"][:4] == [-1, 0, -1, 2]
    old = st
    st, remap, res = _compact(ctx, mp, st, f"(b) {n}")
    assert res == {"before": n, "kept": n - n // 2, "dropped_absorbed": n // 2, "dropped_live": 0}
    mc.assert_moved(old, st, remap, f"(b) {n}")
    mp.close()


def test_b_the_kept_landmarks_all_in_the_last_workgroup(ctx):
    w = mc.kept_last(300, 40)
    mp = ctx.map_create(340, 8)
    st, _, _ = _step(ctx, mp, capi.map_state(340, 8), w, False, "(b) last workgroup", min_obs=1)
    assert st["header"]["n_landmarks"] == 340
    st, remap, res = _compact(ctx, mp, st, "(b) last workgroup", min_obs=2, min_age_scans=2)
    assert res == {"before": 340, "kept": 40, "dropped_absorbed": 0, "dropped_live": 300} and remap[300:340].tolist() == list(range(40))
    assert (remap[:300] == -1).all() and st["header"]["n_obs"] == 80
    mp.close()


# ---- (c) a full map recovers
def test_c_a_full_map_takes_new_landmarks_again(ctx):
    mp, st = _one_batch(ctx, mc.alternating(12), "(c) 12 into 8", cap=8, carry=8)
    H = st["header"]
    assert H["flags"] & capi.FX_MAP_FULL and H["n_needed"] == 12 and H["n_landmarks"] == 8
    st, res = _merge(ctx, mp, st, "(c)")
    assert res["merged"] >= 3
    st, remap, res = _compact(ctx, mp, st, "(c)")
    K = res["kept"]
    assert K == 8 - res["dropped_absorbed"] <= 5 and st["header"]["n_landmarks"] == st["header"]["n_needed"] == K
    assert st["header"]["flags"] & capi.FX_MAP_FULL, "FX_MAP_FULL is sticky"
    more = mm.fragments([(0, 100.0, 7.0), (0, 110.0, 7.0), (1, 120.0, 7.0)], 3)
    st, _, ids = _step(ctx, mp, st, more, False, "(c) the next update")
    assert mm.ids_of(more, ids) == [K, K + 1, K + 2] and st["header"]["n_landmarks"] == K + 3 == st["header"]["n_needed"]
    _same_state(mp, st, "(c) after the next update")
    mp.close()


# ---- (d) refusals
def test_d_host_refusals_launch_nothing(ctx, fxlib):
    import torch
    mp, st = _one_batch(ctx, mc.alternating(6), "(d)")
    st, _ = _merge(ctx, mp, st, "(d)")
    other = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    theirs = other.map_create(8, 8)
    out = torch.full((mp.max_landmarks + 4 + GUARD,), FILL, dtype=torch.int32, device=f"cuda:{ctx.device}")
    remap, res = out.data_ptr(), out.data_ptr() + 4 * mp.max_landmarks
    before = mp.export_state()
    O = capi.FxMapCompactOptions
    ok = O(1, 64)
    for args, word in [((None, mp.handle, C.byref(ok), remap, res), b"null"), ((ctx.handle, None, C.byref(ok), remap, res), b"null"),
                       ((ctx.handle, theirs.handle, C.byref(ok), remap, res), b"another context"),
                       ((other.handle, mp.handle, C.byref(ok), remap, res), b"another context"),
                       ((ctx.handle, mp.handle, C.byref(O(0, 64)), remap, res), b"min_obs"),
                       ((ctx.handle, mp.handle, C.byref(ok), remap + 2, res), b"aligned"),
                       ((ctx.handle, mp.handle, C.byref(ok), remap, res + 1), b"aligned")]:
        assert fxlib.fx_map_compact(*args) == capi.FX_ERR_INVALID_ARG and word in fxlib.fx_last_error(), (word, fxlib.fx_last_error())
    ctx.synchronize()
    assert (out == FILL).all().item() and mp.export_state() == before
    # opt == NULL: the defaults; remap_device == result_device == NULL: nothing is reported
    assert fxlib.fx_map_compact(ctx.handle, mp.handle, None, None, None) == capi.FX_OK
    ctx.synchronize()
    st, _, ref = capi.map_compact_reference(st)
    assert ref["kept"] == 3 and (out == FILL).all().item()
    _same_state(mp, st, "(d) defaults")
    theirs.close(), other.close(), mp.close()
