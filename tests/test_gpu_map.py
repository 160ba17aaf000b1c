"""fx_map_update on the GPU.  Every batch of every case goes track -> map on the device and is compared with capi.map_reference fed
the device's own track output: every header field and every record field, integers equal, the doubles and rms_xy bit for bit
(the definition uses only integers and ordered, correctly rounded operations: there is no tolerance).  The guard words behind
map_id_of_row and behind the track's outputs (which the map only reads) must be untouched."""
import ctypes as C
import threading

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_util as mu
from tests import track_util as tu
from tests.test_gpu_track import FILL, GUARD, _batch as _process, _guarded, _upload

pytestmark = pytest.mark.gpu
# the tile sizes of csrc/fx_map.hip: FXMAP_WG landmarks (or rows) a workgroup, which is also the elements of one block of the integer
# scan over the batch's landmarks; k_map_top scans FXMAP_WG blocks, 65536 landmarks, a round
LM_WG = ROWS_WG = SCAN_BLOCK = 256
TOP_TILE_LMS = 256 * 256


@pytest.fixture
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def _step(ctx, mp, state, p, overlap, what, min_obs=2, max_landmarks=None, dev_in=None):
    """One batch: track into guarded outputs, map update into a guarded map_id_of_row, everything against the reference.  Returns
    (the reference's new state, the device's track records, map_id_of_row)."""
    import torch
    kp, md, inl, reg = dev_in or _upload(p, p["n_scans"] + 2, len(p["rows"]) + 9)
    n_rows = int(md.shape[0])
    max_landmarks = n_rows if max_landmarks is None else max_landmarks
    raw, words, out = _guarded(f"cuda:{ctx.device}", p["n_scans"], n_rows, max_landmarks)
    ids_raw = torch.full((n_rows + GUARD,), FILL, dtype=torch.int32, device=f"cuda:{ctx.device}")
    ctx.track_landmarks(kp, md, inl, reg, p["n_scans"], init_pose=state["header"]["last_pose"][:5], min_obs=min_obs, max_landmarks=max_landmarks, out=out)
    before = [r.clone() for r in raw]
    mp.update(kp, out, overlap=overlap, row_ids=ids_raw[:n_rows])
    ctx.synchronize()
    assert (ids_raw[n_rows:] == FILL).all().item(), f"{what}: the guard behind map_id_of_row"
    assert all((a == b).all().item() for a, b in zip(raw, before)), f"{what}: the track's outputs are read only"
    tr = capi.track_records(*out)
    blk = capi.keypoint_block_parse(kp[0].cpu().numpy(), kp[1], kp[2])
    state, ref_ids = capi.map_reference(state, blk["kp_offset"], blk["rows"], tr, overlap=overlap, track_max_landmarks=max_landmarks)
    ids = ids_raw[:n_rows].cpu().numpy()
    bad = np.flatnonzero(ids != ref_ids)
    assert not len(bad), f"{what}: map_id_of_row differs at {bad[:8].tolist()}: got {ids[bad[:8]]}, reference {ref_ids[bad[:8]]}"
    mu.assert_equal(mp.records(), capi.map_state_records(state), what)
    return state, tr, ids


def _run(ctx, pieces, what, cap, carry, flags=None, mp=None, **kw):
    """The pieces through one map (made here unless given); flags[k]: FX_MAP_OVERLAP of piece k (default: all but the first)."""
    own = mp is None
    mp = mp or ctx.map_create(cap, carry)
    st, trs, ids = capi.map_state(cap, carry), [], []
    for k, p in enumerate(pieces):
        st, tr, row_ids = _step(ctx, mp, st, p, (k > 0) if flags is None else flags[k], f"{what}, batch {k}", **kw)
        trs.append(tr), ids.append(row_ids)
    got = mp.records()
    if own:
        mp.close()
    return st, got, trs, ids


def _case_a(rng):
    """12 scans: a chain through all of them, one ending exactly at scan 3, one starting there, a singleton there, strays, a link
    that is not VALID inside the second batch; cut at 3, 6, 6 (a batch of one scan), 9."""
    h = tu.Hand(12)
    h.chain(0, 12), h.chain(0, 4), h.chain(3, 3), h.new(3), h.chain(5, 5), h.chain(6, 2)
    for b in range(12):
        h.new(b)
    w = h.finish(rng)
    w["reg"]["flags"][4] = 0
    return w, mu.split(w, [0, 3, 6, 6, 9, 11])


@pytest.mark.parametrize("min_obs", [2, 1])
def test_a_every_special_case_in_one_sequence(ctx, min_obs):
    w, pieces = _case_a(np.random.default_rng(51))
    altered = dict(pieces[4], rows=pieces[4]["rows"].copy())
    altered["rows"].view(np.uint32)[1, 3] ^= 1  # one bit of the overlap scan's elevation word: a mismatch
    empty = tu.random_case(np.random.default_rng(52), [0, 0])
    seq = pieces[:4] + [altered, empty, pieces[4]]
    st, got, trs, ids = _run(ctx, seq, f"(a) min_obs {min_obs}", 64, 16, flags=[False, True, True, True, True, False, True], min_obs=min_obs)
    H = got["header"]
    assert H["batches"] == 7 and H["flags"] == capi.FX_MAP_OVERLAP_MISMATCH and H["scans"] == 10 + 3 + 2 + 3
    assert H["segments"] == 2 + 1 + 1 + 1  # (the bad link; the mismatch, the empty batch and the batch after it start segments)
    # up to the mismatch the map is the whole run's track over scans 0 .. 9
    whole = tu.reference(dict(w, off=w["off"][:11], n_scans=10, reg=w["reg"][:9]), min_obs=min_obs)
    part, part_got, _, part_ids = _run(ctx, pieces[:4], "(a) the first four", 64, 16, min_obs=min_obs)
    mu.assert_whole(part_got, whole, "(a) against one batch of scans 0 .. 9")
    # scan 6 holds four rows: two chains that are landmarks of the batch before, one that starts there, a stray
    assert part["header"]["last_joined"] == (2 if min_obs == 2 else 4) and (part_ids[2] >= 0).sum() == (0 if min_obs == 2 else 4) and len(part_ids[2]) == 4
    assert (part_got["landmarks"]["flags"][0] & capi.FX_MAP_LM_CONTINUED) and part_got["landmarks"]["n_obs"][0] == 5  # (scans 0 .. 4: up to the bad link)
    assert len(ids[5]) == 0


@pytest.mark.parametrize("n", [LM_WG - 1, LM_WG, LM_WG + 1, 2 * SCAN_BLOCK + 1, TOP_TILE_LMS + 1])
def test_b_landmarks_and_carry_rows_at_the_workgroup_and_scan_tile_edges(ctx, n):
    """n chains through three scans cut at the middle one: n batch landmarks, n rows in the carry scan, a carry table and a map of
    exactly n, every landmark continued; strays in the outer scans move the chains' rows off the same places."""
    rng = np.random.default_rng(53)
    h = tu.Hand(3)
    [h.new(0) for _ in range(5)], [h.new(2) for _ in range(3)]
    for _ in range(n):
        h.chain(0, 3)
    [h.new(0) for _ in range(2)]
    w = h.finish(rng)
    pieces = mu.split(w, [0, 1, 2])
    assert int(np.diff(pieces[0]["off"])[-1]) == n
    st, got, trs, ids = _run(ctx, pieces, f"(b) {n} landmarks", n, n)
    assert got["header"]["last_joined"] == n and got["header"]["last_new"] == 0 and got["header"]["n_landmarks"] == n and got["header"]["flags"] == 0
    assert trs[1]["header"]["n_landmarks"] == n and (got["landmarks"]["n_obs"] == 3).sum() == n
    if n <= 2 * SCAN_BLOCK + 1:
        mu.assert_whole(got, tu.reference(w), f"(b) {n} landmarks against one batch")


def _two_batches(rng, lens=(4, 4), through_first=True):
    n, e = lens[0] + lens[1] - 1, lens[0] - 1
    h = tu.Hand(n)
    if through_first:
        h.chain(0, n), h.chain(0, e + 1)
    else:
        h.chain(0, e + 1), h.chain(0, n)
    h.chain(e, n - e), h.chain(e + 1, n - e - 1)
    for b in range(n):
        h.new(b)
    w = h.finish(rng)
    return w, mu.split(w, [0, e, n - 1])


def test_c_capacity_of_the_map_the_track_and_the_carry(ctx):
    w, pieces = _two_batches(np.random.default_rng(54))
    needed = tu.reference(w)["header"]["n_landmarks"]
    assert needed == 4
    for cap in (needed - 1, needed, needed + 3):
        mp = ctx.map_create(cap, 16)
        st, got, _, ids = _run(ctx, pieces, f"(c) map of {cap}", cap, 16, mp=mp)
        assert got["header"]["n_needed"] == needed and got["header"]["n_landmarks"] == min(cap, needed)
        assert got["header"]["flags"] == (capi.FX_MAP_FULL if cap < needed else 0)
        assert not mp.landmarks(min(cap, needed)).view(np.uint8).any(), "records past the ones stored"
        mp.close()
    # a landmark that was counted and not stored is new AGAIN when it continues (B before A in row order: A is the second id)
    _, other = _two_batches(np.random.default_rng(54), through_first=False)
    st, got, _, ids = _run(ctx, other, "(c) map of 1", 1, 16)
    assert got["header"]["n_needed"] == 2 + 3 and got["header"]["last_joined"] == 0 and got["landmarks"]["n_obs"].tolist() == [4] and (ids[1] == -1).all()
    # the track's records cut to one landmark a batch; a carry table one row too small for the overlap scan, and just large enough
    st, got, _, _ = _run(ctx, pieces, "(c) track of 1", 8, 16, max_landmarks=1)
    assert got["header"]["flags"] == capi.FX_MAP_TRACK_TRUNCATED and got["header"]["n_needed"] == 1 and got["landmarks"]["n_obs"].tolist() == [7]
    n_e = int(np.diff(pieces[0]["off"])[-1])
    st, got, _, _ = _run(ctx, pieces, "(c) carry too small", 8, n_e - 1)
    assert got["header"]["flags"] == capi.FX_MAP_OVERLAP_MISMATCH and got["header"]["last_joined"] == 0 and got["header"]["scans"] == 8
    st, got, _, _ = _run(ctx, pieces, "(c) carry exact", 8, n_e)
    assert got["header"]["flags"] == 0 and got["header"]["last_joined"] == 1


def test_d_host_refusals_launch_nothing(ctx, fxlib):
    import torch
    w, pieces = _two_batches(np.random.default_rng(55))
    mp = ctx.map_create(8, 16)
    st, _, _ = _step(ctx, mp, capi.map_state(8, 16), pieces[0], False, "(d) first batch")
    p = pieces[1]
    kp, md, inl, reg = _upload(p, p["n_scans"] + 2, len(p["rows"]) + 9)
    n_rows = int(md.shape[0])
    raw, words, out = _guarded(f"cuda:{ctx.device}", p["n_scans"], n_rows, n_rows)
    ctx.track_landmarks(kp, md, inl, reg, p["n_scans"], init_pose=st["header"]["last_pose"][:5], out=out)
    ids = torch.full((n_rows + GUARD,), FILL, dtype=torch.int32, device=f"cuda:{ctx.device}")
    before = (mp.header(), mp.landmarks().tobytes())
    other = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    theirs = other.map_create(8, 16)
    args = [ctx.handle, mp.handle, kp[0].data_ptr(), kp[1], kp[2], out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), n_rows,
            out[3].data_ptr(), n_rows, out[4].data_ptr(), capi.FX_MAP_OVERLAP, ids.data_ptr()]
    for i, repl, word in [(i, None, b"null") for i in (0, 1, 2, 5, 6, 7, 9, 11)] + [(1, theirs.handle, b"another context"), (0, other.handle, b"another context"),
                          (12, 3, b"flags"), (2, kp[0].data_ptr() + 8, b"aligned"), (5, out[0].data_ptr() + 4, b"aligned"), (9, out[3].data_ptr() + 4, b"aligned"),
                          (13, ids.data_ptr() + 2, b"aligned")]:
        a = list(args)
        a[i] = repl
        assert fxlib.fx_map_update(*a) == 1 and word in fxlib.fx_last_error(), (i, fxlib.fx_last_error())
    h = C.c_void_p()
    assert fxlib.fx_map_create(ctx.handle, 0, 16, C.byref(h)) == 1 and b"max_landmarks" in fxlib.fx_last_error() and not h.value
    assert fxlib.fx_map_reset(other.handle, mp.handle) == 1 and fxlib.fx_map_read_header(other.handle, mp.handle, C.byref(capi.FxMapHeader())) == 1
    assert fxlib.fx_map_read_landmarks(ctx.handle, mp.handle, 8, 1, None) == 1
    ctx.synchronize()
    assert (ids == FILL).all().item() and (mp.header(), mp.landmarks().tobytes()) == before
    assert fxlib.fx_map_update(*args) == capi.FX_OK  # (the same arguments, none missing)
    ctx.synchronize()
    assert not (ids[:n_rows] == FILL).any().item() and mp.header()["batches"] == 2 and mp.header()["last_joined"] == 1
    theirs.close(), other.close(), mp.close()


def test_e_identical_bytes_from_run_to_run_across_contexts_and_after_a_reset(ctx):
    rng = np.random.default_rng(56)
    w = tu.world(rng, 60, 13, dropout=0.1, sigma=0.01)
    w["reg"]["flags"][5] = 0
    pieces = mu.split(w, [0, 3, 4, 4, 9, 12])
    mu.assert_whole(_run(ctx, pieces, "(e)", 400, 64)[1], tu.reference(w), "(e) against one batch")

    def once(c, mp=None):
        st, got, trs, ids = _run(c, pieces, "(e)", 400, 64, mp=mp)
        return repr(got["header"]).encode() + got["landmarks"].tobytes() + b"".join(i.tobytes() for i in ids)
    first = once(ctx)
    mp = ctx.map_create(400, 64)
    for _ in range(4):
        assert once(ctx, mp) == first
        mp.reset()
    mp.close()
    res, errs = {}, []

    def run(i):
        try:
            c = capi.Context(capi.params("launch"), capi.limits(2, 1024))
            c.set_batches_in_flight(4)
            for _ in range(2):
                res[i] = once(c)
            c.close()
        except Exception as e:  # (reported below)
            errs.append(e)
    ths = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    [x.start() for x in ths]
    [x.join() for x in ths]
    assert not errs, errs
    assert all(res[i] == first for i in range(4))


def test_f_end_to_end_nine_rotated_copies_in_batches_of_three(fxlib):
    """One batch of nine scans against batches of three with one-scan overlap, both through process -> pack -> match (mutual) ->
    register -> track on the device, the batches also through the map: the same landmarks and the same poses, bit for bit."""
    c = capi.Context(capi.params("launch"), capi.limits(9, 28800))
    scans = tu.rotated_copies(9)

    def chain(part, init, what):
        off, blk, kp, csr = _process(c, part, 0.0, 0.0)
        pairs = capi.pairs_consecutive(off)
        md = c.match_descriptors(csr, csr, pairs, mutual=True)
        reg, inl = c.register_matches(kp, kp, md, pairs)
        return dict(off=blk["kp_offset"], rows=blk["rows"], n_scans=len(part)), (kp, md, inl, reg)
    p, dev_in = chain(scans, None, "(f) one batch")
    out = c.track_landmarks(*dev_in, len(scans))
    c.synchronize()
    whole = capi.track_records(*out)
    assert whole["header"]["scans"] == 9 and whole["header"]["n_landmarks"] > 10 and whole["landmarks"]["n_obs"].max() == 9
    cap, carry = len(p["rows"]), int(np.diff(p["off"]).max())
    mp, st = c.map_create(cap, carry), capi.map_state(cap, carry)
    for k, a in enumerate((0, 2, 4, 6)):
        piece, dev_in = chain(scans[a:a + 3], None, f"(f) batch {k}")
        st, tr, ids = _step(c, mp, st, piece, k > 0, f"(f) batch {k}", dev_in=dev_in)
        for f in ("c", "s", "tx", "ty", "tz"):
            assert (tu.bits(tr["poses"][f]) == tu.bits(whole["poses"][f][a:a + 3])).all(), (k, f)
    got = mp.records()
    mu.assert_whole(got, whole, "(f) the map against one batch of nine")
    print(f"(f) {got['header']}")
    mp.close(), c.close()
