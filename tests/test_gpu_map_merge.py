"""fx_map_merge on the GPU.  Every call of every case is compared with capi.map_merge_reference — an all-pairs statement of
include/fx.h's definition that knows nothing of the grid — bit for bit: every record field, the whole alias table, the result
words, and the carry table as the next fx_map_update's map_id_of_row shows it.  The guard words behind the result and the records
past the ones stored must be untouched."""
import ctypes as C
import threading

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_merge_util as mm
from tests import map_util as mu
from tests import track_util as tu
from tests.test_gpu_map import _run, _step
from tests.test_gpu_track import FILL, GUARD, _batch as _process

pytestmark = pytest.mark.gpu
# csrc/fx_map_merge.hip: FXMM_WG landmarks (or buckets) a workgroup, one block of the bucket scan; k_mm_top scans FXMM_WG blocks a round
WG = 256
E = float(np.float32(0.30)) * (1.0 + 2.0 ** -8)  # the grid's cell edge at the default gate
F32 = lambda v: float(np.float32(v))


@pytest.fixture
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def _merge(ctx, mp, st, what, shrunk=False, **kw):
    """One fx_map_merge into a guarded result against one map_merge_reference call.  Returns (the new state, the result dict).
    The records past the ones stored stay what they were, and are zero unless `shrunk`: a map that was compacted, reset or imported
    into holds unspecified records there (include/fx.h)."""
    import torch
    tail = mp.landmarks(st["header"]["n_landmarks"]).tobytes()
    raw = torch.full((4 + GUARD,), FILL, dtype=torch.int32, device=f"cuda:{ctx.device}")
    mp.merge(result=raw[:4], **kw)
    ctx.synchronize()
    st, ref = capi.map_merge_reference(st, **kw)
    got = dict(zip(capi.MAP_MERGE_RESULT_FIELDS, raw[:4].cpu().numpy().astype(np.uint32).tolist()))
    assert (raw[4:] == FILL).all().item(), f"{what}: the guard behind the result"
    assert got == ref, f"{what}: result {got}, reference {ref}"
    mu.assert_equal(mp.records(), capi.map_state_records(st), what)
    mm.assert_alias(mp.alias(), st, what)
    n = st["header"]["n_landmarks"]
    past = mp.landmarks(n)
    assert past.tobytes() == tail and (shrunk or not past.view(np.uint8).any()), f"{what}: records past the ones stored"
    return st, got


def _merge_to_fixpoint(ctx, mp, st, what, max_calls=mm.MAX_CALLS, **kw):
    results = []
    for k in range(max_calls + 1):
        st, res = _merge(ctx, mp, st, f"{what}, call {k}", **kw)
        results.append(res)
        if res["merged"] == 0:
            return st, results
    raise AssertionError(f"{what}: no fixpoint after {max_calls + 1} calls: {results}")


def _one_batch(ctx, w, what, cap=None, carry=None):
    """A fragments() case through track -> map on the device (compared with the reference on the way).  Returns (map, state)."""
    n = len(w["rows"])
    cap, carry = cap or max(n, 1), carry or max(n, 1)
    mp = ctx.map_create(cap, carry)
    st, _, _ = _step(ctx, mp, capi.map_state(cap, carry), w, False, what)
    return mp, st


# ---- (a) the reference's cases on the device
def test_a1_flicker_world(ctx):
    w, pieces, _ = mm.flicker()
    f = mm.FLICKER
    mp = ctx.map_create(f["cap"], f["carry"])
    st, got, _, _ = _run(ctx, pieces, "(a1)", f["cap"], f["carry"], mp=mp)
    assert got["header"]["n_landmarks"] == 54
    st, results = _merge_to_fixpoint(ctx, mp, st, "(a1)", max_gap_scans=24)
    assert results[-1]["live"] == len(mm.long_runs(w)) and sum(r["merged"] for r in results) == 54 - results[-1]["live"]
    before = mp.landmarks().tobytes() + mp.alias().tobytes()
    mp.merge(max_gap_scans=24, result=False)
    ctx.synchronize()
    assert mp.landmarks().tobytes() + mp.alias().tobytes() == before, "a call on a fixpoint changes no byte"
    print("(a1)", results)
    mp.close()


def test_a2_update_after_merge_continues_the_roots(ctx):
    w, pieces, _ = mm.flicker()
    f = mm.FLICKER
    mp, st = ctx.map_create(f["cap"], f["carry"]), capi.map_state(f["cap"], f["carry"])
    merged = 0
    for k, p in enumerate(pieces):
        st, _, ids = _step(ctx, mp, st, p, k > 0, f"(a2) batch {k}")  # (map_id_of_row shows the carry the merge re-pointed)
        mm.assert_alias(mp.alias(), st, f"(a2) batch {k}: the update leaves the alias table alone")
        if k in (1, 3):
            st, results = _merge_to_fixpoint(ctx, mp, st, f"(a2) after batch {k}", max_gap_scans=24)
            merged += sum(r["merged"] for r in results)
    st, results = _merge_to_fixpoint(ctx, mp, st, "(a2) at the end", max_gap_scans=24)
    assert merged > 0 and results[-1]["live"] == len(mm.long_runs(w))
    L = mp.records()["landmarks"]
    both = capi.FX_MAP_LM_MERGED | capi.FX_MAP_LM_CONTINUED
    assert (L["flags"] & both == both).any()
    mp.close()


HAND = {
    "gate exact": ([(0, 0.0, 2.0), (3, 0.25, 2.0)], 5, (), dict(merge_dist=0.25), [1]),
    "gate next float": ([(0, 0.0, 2.0), (3, float(np.nextafter(np.float32(0.25), np.float32(1.0))), 2.0)], 5, (), dict(merge_dist=0.25), [0]),
    "gap exact": ([(0, 1.0, 1.0), (7, 1.0, 1.0)], 9, (), dict(max_gap_scans=6), [1]),
    "gap one short": ([(0, 1.0, 1.0), (7, 1.0, 1.0)], 9, (), dict(max_gap_scans=5), [0]),
    "segments": ([(0, 1.0, 1.0), (7, 1.0, 1.0)], 9, (4,), {}, [0]),
    "touching ranges": ([(0, 1.0, 1.0), (1, 1.0, 1.0), (2, 1.0, 1.0)], 4, (), {}, [1, 0]),
    "most recent": ([(0, -0.25, 0.0), (2, 0.25, 0.0), (5, -0.125, 0.0)], 7, (), dict(merge_dist=0.375), [1]),
    "nearest": ([(0, 0.125, 0.0), (0, -0.0625, 0.0), (3, 0.0, 0.0)], 5, (), {}, [1]),
    "lowest id": ([(0, 0.125, 0.0), (0, -0.125, 0.0), (3, 0.0, 0.0)], 5, (), {}, [1]),
    "acceptance tie": ([(0, 0.0, 0.0), (3, 0.25, 0.0), (3, -0.25, 0.0)], 5, (), dict(merge_dist=0.375), [1, 0]),
    "loser next call": ([(0, 0.0, 0.0), (3, 0.25, 0.0), (6, -0.3125, 0.0)], 8, (), dict(merge_dist=0.5), [1, 1, 0]),
    "chain of three": ([(0, F32(10.01), F32(-3.02)), (3, F32(10.07), F32(-3.11)), (6, F32(9.96), F32(-2.95))], 8, (), {}, [2, 0]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_a3_hand_built(ctx, name):
    frags, n_scans, bad, kw, merged = HAND[name]
    mp, st = _one_batch(ctx, mm.fragments(frags, n_scans, bad), f"(a3) {name}")
    for k, want in enumerate(merged):
        st, res = _merge(ctx, mp, st, f"(a3) {name}, call {k}", **kw)
        assert res["merged"] == want, (name, k, res)
    mp.close()


# ---- (b) sizes at the launch edges
def _pairs(n, seed=61, slot=64):
    """n landmarks as n // 2 pairs (and a single one when n is odd) on a 2 m lattice about the origin, root and member up to 0.25 m
    apart.  Pair k lives in scans 2 j, 2 j + 1 (its root) and 2 j + 2, 2 j + 3 (its member), j = k // slot, and the landmarks that
    begin at one scan are created members and roots in turn: ids follow (first scan, order of creation), so but for the first
    `slot` roots and the last `slot` members every run of ids holds both, and so does every workgroup."""
    rng = np.random.default_rng(seed)
    P = n // 2
    side = int(np.ceil(np.sqrt(max(P, 1))))
    roots, members = [], []
    for k in range(P):
        cx, cy = 2.0 * (k % side - side // 2) + rng.uniform(-0.3, 0.3), 2.0 * (k // side - side // 2) + rng.uniform(-0.3, 0.3)
        r, a = rng.uniform(0.0, 0.25), rng.uniform(0.0, 2 * np.pi)
        t = 2 * (k // slot)
        roots.append((t, F32(cx), F32(cy))), members.append((t + 2, F32(cx + r * np.cos(a)), F32(cy + r * np.sin(a))))
    frags = []
    for k in range(P + slot):  # the root of pair k, then the member of the pair one slot earlier: both begin at the same scan
        frags += roots[k:k + 1] + (members[k - slot:k - slot + 1] if k >= slot else [])
    if n % 2:
        frags.append((0, F32(2.0 * side + 5.0), 0.0))
    return mm.fragments(frags, 2 * ((P + slot - 1) // slot) + 2), P


@pytest.mark.parametrize("n", [WG - 1, WG, WG + 1, 2 * WG + 1, 2 * WG * 64 + 1])
def test_b_landmarks_at_the_workgroup_and_scan_tile_edges(ctx, n):
    w, P = _pairs(n)
    mp, st = _one_batch(ctx, w, f"(b) {n} landmarks", cap=n, carry=8)
    assert st["header"]["n_landmarks"] == n
    st, res = _merge(ctx, mp, st, f"(b) {n} landmarks")
    assert res == {"proposals": P, "merged": P, "live": n - P, "reserved": 0}
    a = np.array(st["alias"])
    for lo in range(0, n - 1, WG):  # roots and members in every workgroup (of more than one landmark)
        assert (a[lo:lo + WG] >= 0).any() and (a[lo:lo + WG] < 0).any(), lo
    if n <= 2 * WG + 1:  # (the all-pairs reference takes seconds at the largest size: once is enough there)
        st, res = _merge(ctx, mp, st, f"(b) {n} landmarks, again")
        assert res["merged"] == 0
    mp.close()


# ---- (c) grid edges
def test_c_pairs_across_cell_borders_far_from_the_origin_and_beyond_the_table(ctx):
    frags, want = [], 0

    def pair(x0, y0, x1, y1, merges=True):
        nonlocal want
        frags.extend([(0, F32(x0), F32(y0)), (3, F32(x1), F32(y1))])
        want += bool(merges)
    for k in (7, -7, 0):  # borders at positive and negative coordinates and across 0 (floor, not truncation)
        b = k * E
        pair(b - 0.1, 50.0 + k, b + 0.1, 50.0 + k)            # in x
        pair(60.0 + k, b - 0.1, 60.0 + k, b + 0.1)            # in y
        pair(b - 0.1, b - 3.1 * E - 0.1, b + 0.1, b - 3.1 * E + 0.1)  # diagonally (3.1 cells off the x = y diagonal: other places)
        pair(b - 0.25, 70.0 + k, b + 0.25, 70.0 + k, merges=False)  # one cell apart and beyond the gate
    pair(1e6, 1e6, 1e6 + 0.25, 1e6)                   # float32 steps of 1 / 16 m
    pair(-1e6, 1e6, -1e6, 1e6 + 0.3125, merges=False)
    pair(1e13, -1e13, 1e13, -1e13)                    # beyond 2^39 cells: the far list
    pair(1e13, 2e13, 1e13, 2e13)
    pair(1e30, 1e30, 1e30, 1e30)                      # beyond any cell number
    pair(3e38, 3e38, -3e38, 3e38, merges=False)       # the ends of float32's range
    w = mm.fragments(frags, 5)
    mp, st = _one_batch(ctx, w, "(c) borders")
    st, res = _merge(ctx, mp, st, "(c) borders")
    assert res["merged"] == want == res["proposals"], (res, want)
    mp.close()


def test_c_three_hundred_fragments_in_one_cell(ctx):
    rng = np.random.default_rng(62)
    frags = [(2 * k, F32(12.3 + rng.uniform(-0.04, 0.04)), F32(-45.6 + rng.uniform(-0.04, 0.04))) for k in range(300)]
    mp, st = _one_batch(ctx, mm.fragments(frags, 600), "(c) 300 fragments")
    st, res = _merge(ctx, mp, st, "(c) 300 fragments")
    assert res == {"proposals": 299, "merged": 299, "live": 1, "reserved": 0} and st["landmarks"][0]["n_obs"] == 600
    mp.close()


@pytest.mark.parametrize("merging", [False, True])
def test_c_a_map_of_eight_small_table_and_collisions(ctx, merging):
    if merging:
        w, _ = _pairs(8, seed=63)
    else:
        w = mm.fragments([(2 * (k % 2), F32(37.0 * k - 100.0), F32(-53.0 * k + 90.0)) for k in range(8)], 5)
    mp, st = _one_batch(ctx, w, "(c) map of 8", cap=8, carry=4)
    assert st["header"]["n_landmarks"] == 8 and st["header"]["flags"] == 0
    st, res = _merge(ctx, mp, st, "(c) map of 8")
    assert res["merged"] == (4 if merging else 0) and res["live"] == 8 - res["merged"]
    mp.close()


# ---- (d) refusals
def test_d_host_refusals_launch_nothing(ctx, fxlib):
    import torch
    w = mm.fragments(HAND["chain of three"][0], 8)
    mp, st = _one_batch(ctx, w, "(d)")
    other = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    theirs = other.map_create(8, 8)
    res = torch.full((4 + GUARD,), FILL, dtype=torch.int32, device=f"cuda:{ctx.device}")
    before = (mp.header(), mp.landmarks().tobytes(), mp.alias().tobytes())
    O = capi.FxMapMergeOptions
    ok = O(0.3, 64)
    for args, word in [((None, mp.handle, C.byref(ok), res.data_ptr()), b"null"), ((ctx.handle, None, C.byref(ok), res.data_ptr()), b"null"),
                       ((ctx.handle, theirs.handle, C.byref(ok), res.data_ptr()), b"another context"),
                       ((other.handle, mp.handle, C.byref(ok), res.data_ptr()), b"another context"),
                       ((ctx.handle, mp.handle, C.byref(O(0.0, 64)), res.data_ptr()), b"merge_dist"),
                       ((ctx.handle, mp.handle, C.byref(O(-1.0, 64)), res.data_ptr()), b"merge_dist"),
                       ((ctx.handle, mp.handle, C.byref(O(float("nan"), 64)), res.data_ptr()), b"merge_dist"),
                       ((ctx.handle, mp.handle, C.byref(O(float("inf"), 64)), res.data_ptr()), b"merge_dist"),
                       ((ctx.handle, mp.handle, C.byref(O(0.3, 0)), res.data_ptr()), b"max_gap_scans"),
                       ((ctx.handle, mp.handle, C.byref(ok), res.data_ptr() + 2), b"aligned")]:
        assert fxlib.fx_map_merge(*args) == 1 and word in fxlib.fx_last_error(), (word, fxlib.fx_last_error())
    a = C.c_void_p()
    assert fxlib.fx_map_get_alias(None, C.byref(a)) == 1 and fxlib.fx_map_get_alias(mp.handle, None) == 1
    assert fxlib.fx_map_read_alias(other.handle, mp.handle, 0, 1, C.c_void_p(np.zeros(1, np.int32).ctypes.data)) == 1
    assert fxlib.fx_map_read_alias(ctx.handle, mp.handle, mp.max_landmarks, 1, None) == 1
    assert mp.alias_device_pointer() and len(mp.alias(mp.max_landmarks)) == 0
    ctx.synchronize()
    assert (res == FILL).all().item() and (mp.header(), mp.landmarks().tobytes(), mp.alias().tobytes()) == before
    # opt == NULL: the defaults; result_device == NULL: nothing is reported
    assert fxlib.fx_map_merge(ctx.handle, mp.handle, None, None) == capi.FX_OK
    ctx.synchronize()
    st, ref = capi.map_merge_reference(st)
    assert ref["merged"] == 2 and (res == FILL).all().item()
    mu.assert_equal(mp.records(), capi.map_state_records(st), "(d) defaults")
    mm.assert_alias(mp.alias(), st, "(d) defaults")
    theirs.close(), other.close(), mp.close()


# ---- (e) the same bytes from run to run, across contexts, after a reset
def test_e_identical_bytes_across_contexts_and_after_a_reset(ctx):
    w, pieces, _ = mm.flicker()
    f = mm.FLICKER

    def once(c, mp=None):
        own = mp is None
        mp = mp or c.map_create(f["cap"], f["carry"])
        st, _, _, ids = _run(c, pieces, "(e)", f["cap"], f["carry"], mp=mp)
        st, results = _merge_to_fixpoint(c, mp, st, "(e)", max_gap_scans=24)
        out = repr(results).encode() + mp.landmarks().tobytes() + mp.alias().tobytes()
        if own:
            mp.close()
        return out
    first = once(ctx)
    mp = ctx.map_create(f["cap"], f["carry"])
    for _ in range(2):
        assert once(ctx, mp) == first
        mp.reset()
        ctx.synchronize()
        assert (mp.alias() == -1).all(), "a reset fills the alias table with -1"
    mp.close()
    res, errs = {}, []

    def run(i):
        try:
            c = capi.Context(capi.params("launch"), capi.limits(2, 1024))
            c.set_batches_in_flight(4)
            res[i] = once(c)
            c.close()
        except Exception as e:  # (reported below)
            errs.append(e)
    ths = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    [x.start() for x in ths]
    [x.join() for x in ths]
    assert not errs, errs
    assert all(res[i] == first for i in range(4))


# ---- (f) end to end on real kernels
def test_f_nine_rotated_copies_with_the_middle_scan_withheld(fxlib):
    """process -> pack -> match (mutual) -> register on nine rotated copies; the track is handed a block in which scan 4 has no
    rows (its rows are counted to scan 3, where their match records belong to another pair and link nothing, and the rows of
    scan 5 find their partners in the wrong scan): every track breaks at scan 4, the poses still chain through all nine scans in
    one segment.  The map then holds every pole that lived through both halves twice; the merge makes it one."""
    import torch
    c = capi.Context(capi.params("launch"), capi.limits(9, 28800))
    scans = tu.rotated_copies(9)
    off, blk, kp, csr = _process(c, scans, 0.0, 0.0)
    pairs = capi.pairs_consecutive(off)
    md = c.match_descriptors(csr, csr, pairs, mutual=True)
    reg, inl = c.register_matches(kp, kp, md, pairs)
    unbroken = capi.track_records(*c.track_landmarks(kp, md, inl, reg, 9))
    host = kp[0].cpu().numpy().copy()
    host.view(np.uint32)[4 + 4] = int(off[5])  # kp_offset[4] = kp_offset[5]: scan 4 is empty
    cut = (torch.from_numpy(host).to(kp[0].device), kp[1], kp[2])
    cap, carry = len(blk["rows"]), int(np.diff(off).max()) * 2
    mp = c.map_create(cap, carry)
    piece = dict(off=capi.keypoint_block_parse(host, kp[1], kp[2])["kp_offset"], rows=blk["rows"], n_scans=9)
    st, tr, ids = _step(c, mp, capi.map_state(cap, carry), piece, False, "(f) the cut run", dev_in=(cut, md, inl, reg))
    L = tr["landmarks"]
    assert st["header"]["segments"] == 1 and len(L) > 10 and not ((L["first_scan"] <= 4) & (L["last_scan"] >= 4)).any(), "a track crosses scan 4"
    st, results = _merge_to_fixpoint(c, mp, st, "(f)")
    alias, M = np.array(st["alias"]), capi.map_state_records(st)["landmarks"]
    twice = np.flatnonzero(alias >= 0)
    assert len(twice) >= 5 and (M["last_scan"][alias[twice]] >= 5).all() and (M["first_scan"][alias[twice]] <= 3).all()
    assert (M["n_obs"][alias[twice]] >= 4).all() and results[-1]["live"] == len(M) - len(twice)
    print(f"(f) {len(M)} landmarks of the cut run, {results[-1]['live']} live after {results}; the unbroken run has {unbroken['header']['n_landmarks']}")
    mp.close(), c.close()
