"""fx_track_landmarks on the GPU.  Every case checks that every field of every record equals capi.track_reference on the same
inputs — integers equal, the doubles and rms_xy bit for bit (the definition uses only integers and ordered, correctly rounded
operations: there is no tolerance) — and that the guard words behind all five outputs, and the landmark records past the ones
the call may write, are untouched."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import track_util as tu

pytestmark = pytest.mark.gpu
GUARD = 1024  # int32 words behind each output that the call must leave alone
FILL = 0x5A5A5A5A
NONE = capi.FX_TRACK_NO_ROW
# the tile sizes of csrc/fx_track.hip: FXT_WG rows a workgroup, which is also the elements of one block of the integer scan and the
# links of one tile of k_track_poses; k_track_top scans FXT_WG blocks, 65536 rows, a round
ROWS_WG = SCAN_BLOCK = POSE_TILE = 256
TOP_TILE_ROWS = 256 * 256
HDL64 = dict(n_rings=64, n_az=2048, el0_deg=-24.8, el_step_deg=26.8 / 63, n_poles=256)


@pytest.fixture
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def _guarded(dev, n_scans, n_rows, max_landmarks):
    import torch
    words = (n_scans * 12, n_rows, n_rows, max_landmarks * 12, 8)
    raw = [torch.full((n + GUARD,), FILL, dtype=torch.int32, device=dev) for n in words]
    out = (raw[0][:words[0]].view(torch.float64).view(n_scans, 6), raw[1][:n_rows], raw[2][:n_rows],
           raw[3][:words[3]].view(torch.float64).view(max_landmarks, 6), raw[4][:8])
    return raw, words, out


def _call(ctx, kp, md, inl, reg, n_scans, max_landmarks=None, **kw):
    """Context.track_landmarks into guarded outputs -> track_records' dict."""
    import torch
    n_rows = int(md.shape[0])
    max_landmarks = n_rows if max_landmarks is None else max_landmarks
    raw, words, out = _guarded(f"cuda:{ctx.device}", n_scans, n_rows, max_landmarks)
    torch.cuda.synchronize()
    ctx.track_landmarks(kp, md, inl, reg, n_scans, max_landmarks=max_landmarks, out=out, **kw)
    ctx.synchronize()
    for r, n, name in zip(raw, words, ("poses", "landmark_of_row", "obs_row", "landmarks", "header")):
        assert (r[n:] == FILL).all().item(), f"the guard behind {name}"
    got = capi.track_records(*out)
    written = min(got["header"]["n_landmarks"], max_landmarks)
    assert (raw[3][written * 12:] == FILL).all().item(), "landmark records past the ones written"
    return got


def _upload(w, max_scans, max_total, q_max_rows=None, stored=None, n_reg=None, blk=None):
    import torch
    blk = tu.block(w["off"], w["rows"], max_scans, max_total, stored) if blk is None else blk
    m, inl = tu.padded(w, q_max_rows)
    reg = np.zeros(max(len(w["reg"]), n_reg or 0, 1), capi.REG_DTYPE)
    reg.view(np.uint8)[:] = 0xA5  # (records beyond the block's links: never read)
    reg[:len(w["reg"])] = w["reg"]
    return ((torch.from_numpy(blk).cuda(), max_scans, max_total), torch.from_numpy(m.view(np.int32).reshape(-1, 8).copy()).cuda(),
            torch.from_numpy(inl.copy()).cuda(), torch.from_numpy(reg.view(np.float64).reshape(-1, 8).copy()).cuda())


def _run(ctx, w, what, n_scans=None, q_max_rows=None, stored=None, max_scans=None, max_total=None, max_landmarks=None, edge=None, **kw):
    """A case dict of track_util on the device (its block laid out for max_scans / max_total, storing `stored` rows), compared with
    the reference.  edge: one of tu.edge_blocks(w["rows"]) in the place of the block (the per-row inputs stay w's)."""
    n_scans = w["n_scans"] if n_scans is None else n_scans
    max_scans = max(w["n_scans"], n_scans) + 2 if max_scans is None else max_scans
    max_total = len(w["rows"]) + 9 if max_total is None else max_total
    if edge:
        max_scans, max_total, q_max_rows = edge["max_scans"], edge["max_total"], len(w["m"])
    kp, md, inl, reg = _upload(w, max_scans, max_total, q_max_rows, stored, n_scans - 1, edge and edge["blk"])
    got = _call(ctx, kp, md, inl, reg, n_scans, max_landmarks, **kw)
    ref = tu.reference(dict(w, off=edge["off"], rows=edge["rows"]) if edge else w, n_scans=n_scans, q_max_rows=q_max_rows, stored=stored, **kw)
    tu.assert_equal(got, ref, what, max_landmarks)
    n = ref["landmarks"]["n_obs"]
    print(f"{what}: {ref['header']}, longest track {int(n.max()) if len(n) else 0}")
    return got, ref


def _case_a(rng):
    """66 scans of chains (scans 0 .. 65: scan 0 behind a link that is not VALID, then 65 scans joined by good links), a link
    with a NaN tx, a scan of no keypoints, and two scans for the special rows."""
    h = tu.Hand(70)
    first = [h.new(0) for _ in range(3)]
    lens = [65, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64]
    chains = {}
    for n in lens:
        chains[n] = h.chain(1 if n == 65 else 2 if n == 64 else int(rng.integers(1, 67 - n)), n)
        h.new(int(rng.integers(1, 66)))  # (a stray row, so that chains do not sit at the same place in every scan)
    over_bad = h.child(first[1])             # scan 1 -> scan 0 over the link that is not VALID
    over_nan = h.child(chains[65][-1])       # scan 66 -> scan 65 over the link with a NaN tx
    assert over_nan[0] == 66 and h.count[67] == 0
    par = [h.new(68) for _ in range(16)]
    kids = [h.child(p) for p in (par[0], par[0], par[1], par[1], par[1])] + [h.child(p) for p in par[2:]]
    w = h.finish(rng)
    at, m, inl, rows = w["at"], w["m"], w["inlier"], w["rows"]
    N = len(rows)
    k = [at(x) for x in kids[5:]]  # children of par[2 ..]
    m["train_row"][k[0]] = at(chains[65][0])  # a row of the wrong scan
    m["train_row"][k[1]] = -1
    m["train_row"][k[2]] = N + 5              # beyond the rows
    m["train_row"][k[3]] = 0x7fffffff
    m["pair"][k[4]] = 3                       # a record of another pair
    inl[k[5]], inl[k[6]] = 0, 2
    rows[k[7], 0] = np.nan
    rows[at(par[10]), 1] = np.inf             # (k[8]'s parent)
    rows[k[9], 3] = np.nan                    # elevation: not a coordinate, the link is kept
    rows[at(par[13]), 3] = np.inf             # (k[11]'s parent: kept as well)
    rows[k[10], 2] = -np.inf
    w["reg"]["flags"][0] = capi.FX_REG_NO_HYPOTHESIS
    w["reg"]["tx"][65] = np.nan
    w["special"] = dict(k=k, kids=[at(x) for x in kids], par=[at(x) for x in par], over_bad=at(over_bad), over_nan=at(over_nan), lens=lens)
    return w


def test_a_every_special_case_in_one_block(ctx):
    w = _case_a(np.random.default_rng(31))
    N, sp = len(w["rows"]), w["special"]
    got, ref = _run(ctx, w, "(a) all 70 scans")
    L, lor = ref["landmarks"], ref["landmark_of_row"]
    assert sorted(L["n_obs"].tolist()) == sorted([n for n in sp["lens"] if n >= 2] + [2] * 6) and ref["header"]["n_conflicts"] == 3
    assert ref["header"]["n_gaps"] == 2 and ref["poses"]["segment"][[0, 1, 65, 66, 69]].tolist() == [0, 1, 1, 2, 2]
    assert lor[sp["over_bad"]] == -1 and lor[sp["over_nan"]] == -1
    kept = [sp["kids"][0], sp["kids"][2], sp["k"][9], sp["k"][11], sp["k"][12], sp["k"][13]]  # lowest of two / three, NaN / inf elevation, plain
    assert (lor[kept] >= 0).all() and (lor[[x for x in sp["kids"] if x not in kept]] == -1).all()
    assert got["header"]["scans"] == 70 and got["header"]["rows"] == N
    # fewer scans than the block has; poses asked beyond the block's scans
    got, ref = _run(ctx, w, "(a) n_scans 66", n_scans=66)
    assert ref["header"]["scans"] == 66 and (ref["landmark_of_row"][w["off"][66]:] == -1).all() and ref["landmarks"]["n_obs"].max() == 65
    got, ref = _run(ctx, w, "(a) n_scans 72", n_scans=72)
    assert ref["header"]["scans"] == 70 and ref["poses"]["flags"][70:].tolist() == [capi.FX_POSE_NO_SCAN] * 2
    assert ref["poses"][71].tobytes()[:40] == ref["poses"][69].tobytes()[:40]
    # q_max_rows below and above the rows stored; a block that stores fewer rows than its offsets say
    got, ref = _run(ctx, w, "(a) q_max_rows N - 3", q_max_rows=N - 3)
    assert ref["header"]["rows"] == N - 3
    got, ref = _run(ctx, w, "(a) q_max_rows N + 7", q_max_rows=N + 7)
    assert ref["header"]["rows"] == N and (ref["landmark_of_row"][N:] == -1).all()
    got, ref = _run(ctx, w, "(a) stored N - 2", stored=N - 2)
    assert ref["header"]["rows"] == N - 2
    _run(ctx, w, "(a) exact layout", max_scans=70, max_total=N)
    # the edges only a hand-made block reaches: three scans of 2, 0 and 3 rows whose records all propose (none may be kept: the scan
    # before is empty); with min_obs 1 every row that has a scan is a landmark of its own, so the scan of every row shows
    h = tu.Hand(3)
    first, last = [h.new(0) for _ in range(2)], [h.new(2) for _ in range(3)]
    e = h.finish(np.random.default_rng(32))
    for k, r in enumerate(last):
        e["m"]["pair"][e["at"](r)], e["m"]["train_row"][e["at"](r)], e["inlier"][e["at"](r)] = 1, k % 2, 1
    assert tuple(e["off"]) == tu.EDGE_OFF
    for edge in tu.edge_blocks(e["rows"]):
        got, ref = _run(ctx, e, f"(a) {edge['what']}", edge=edge, min_obs=1)
        assert ref["header"]["scans"] == 3 and ref["header"]["rows"] == len(edge["rows"]) == ref["header"]["n_landmarks"]


@pytest.mark.parametrize("rows", [ROWS_WG - 1, ROWS_WG, ROWS_WG + 1, 2 * SCAN_BLOCK + 1])
def test_b_rows_at_the_workgroup_and_scan_block_edges(ctx, rows):
    rng = np.random.default_rng(32)
    w = tu.random_case(rng, [rows - 3 * (rows // 4)] + [rows // 4] * 3, p_link=0.8)
    assert len(w["rows"]) == rows
    _run(ctx, w, f"(b) {rows} rows", max_total=rows)


@pytest.mark.parametrize("n_scans", [POSE_TILE, POSE_TILE + 1, POSE_TILE + 2, 2 * POSE_TILE, 2 * POSE_TILE + 1, 2 * POSE_TILE + 2])
def test_b_scans_at_the_pose_tile_edges(ctx, n_scans):
    """POSE_TILE - 1, POSE_TILE and POSE_TILE + 1 links, and the same three at the end of the second tile; 1 to 2 keypoints a scan."""
    rng = np.random.default_rng(33)
    w = tu.random_case(rng, rng.integers(1, 3, n_scans).tolist(), p_link=0.95)
    w["reg"]["flags"][[n_scans // 3, n_scans - 3]] = 0  # (two bad links, one in the last tile)
    got, ref = _run(ctx, w, f"(b) {n_scans} scans", max_scans=n_scans)
    assert ref["landmarks"]["n_obs"].max() > 16 and ref["header"]["n_gaps"] == 2  # (chains that take several jumping rounds)


@pytest.mark.parametrize("rows", [TOP_TILE_ROWS - ROWS_WG, TOP_TILE_ROWS, TOP_TILE_ROWS + 1])
def test_b_blocks_at_the_top_scan_tile_edges(ctx, rows):
    """255, 256 and 257 blocks of the integer scan: one round of k_track_top less one block, exactly one round, one block more."""
    rng = np.random.default_rng(34)
    w = tu.random_case(rng, [rows - 7 * (rows // 8)] + [rows // 8] * 7, p_link=0.5)
    got, ref = _run(ctx, w, f"(b) {rows} rows")
    assert ref["header"]["n_conflicts"] > 1000 and ref["header"]["n_landmarks"] > 1000


def test_c_options_and_capacity(ctx):
    rng = np.random.default_rng(35)
    w = tu.random_case(rng, [40] * 8, p_link=0.9)
    needed = {}
    for k in (1, 2, 3, 7, 100):
        got, ref = _run(ctx, w, f"(c) min_obs {k}", min_obs=k)
        needed[k] = ref["header"]["n_landmarks"]
    assert needed[1] > needed[2] > needed[3] > needed[7] >= 0 == needed[100]
    for cap in (0, needed[2] - 1, needed[2]):
        got, ref = _run(ctx, w, f"(c) max_landmarks {cap}", max_landmarks=cap)
        assert len(got["landmarks"]) == cap and got["header"]["n_landmarks"] == needed[2]
    got, ref = _run(ctx, w, "(c) init_pose", init_pose=(math.cos(2.0), math.sin(2.0), -30.5, 12.25, 1.5))
    assert got["poses"]["tx"][0] == -30.5 and got["poses"]["c"][0] == math.cos(2.0)


def test_d_host_refusals_launch_nothing(ctx):
    rng = np.random.default_rng(36)
    w = tu.random_case(rng, [20] * 3)
    kp, md, inl, reg = _upload(w, 3, 60, n_reg=3)
    raw, words, out = _guarded(f"cuda:{ctx.device}", 3, 60, 60)
    for kw, word in [(dict(min_obs=0), "min_obs"), (dict(init_pose=(math.nan, 0, 0, 0, 0)), "init_pose"),
                     (dict(init_pose=(1, 0, math.inf, 0, 0)), "init_pose"), (dict(init_pose=(1, 0, 0, 0, -math.inf)), "init_pose")]:
        with pytest.raises(capi.FxError, match="status 1") as e:
            ctx.track_landmarks(kp, md, inl, reg, 3, out=out, **kw)
        assert word in str(e.value) and word in ctx.lib.fx_last_error().decode(), (kw, str(e.value))
    # through the C entry point, into the same guarded outputs: n_scans 0 and beyond max_scans, then a NULL required pointer, one
    # at a time (the binding never passes one)
    opt = capi.FxTrackOptions(2, 0)
    args = [ctx.handle, kp[0].data_ptr(), 3, 60, md.data_ptr(), inl.data_ptr(), 60, reg.data_ptr(), 3, None, C.byref(opt)] + \
           [t.data_ptr() for t in out[:4]] + [60, out[4].data_ptr()]
    for n in (0, 4):
        a = list(args)
        a[8] = n
        assert ctx.lib.fx_track_landmarks(*a) == 1 and b"n_scans" in ctx.lib.fx_last_error(), n
    for i in (0, 1, 4, 5, 7, 11, 12, 13, 14, 16):
        a = list(args)
        a[i] = None
        assert ctx.lib.fx_track_landmarks(*a) == 1 and b"null" in ctx.lib.fx_last_error(), i
    ctx.synchronize()
    for r in raw:
        assert (r == FILL).all().item()
    assert ctx.lib.fx_track_landmarks(*args) == capi.FX_OK  # (the same arguments, none missing)
    ctx.synchronize()
    assert not (raw[4][:8] == FILL).any().item()


def test_e_identical_bytes_from_run_to_run_and_across_contexts(ctx):
    rng = np.random.default_rng(37)
    w = tu.random_case(rng, rng.integers(0, 60, 70).tolist(), p_link=0.9, p_bad=0.05)
    ref = tu.reference(w)

    def once(c):
        got = _call(c, *_upload(w, 70, len(w["rows"])), 70)
        return b"".join(got[k].tobytes() for k in ("poses", "landmark_of_row", "obs_row", "landmarks")) + repr(got["header"]).encode()
    first = once(ctx)
    assert first == b"".join(ref[k].tobytes() for k in ("poses", "landmark_of_row", "obs_row", "landmarks")) + repr(ref["header"]).encode()
    for _ in range(4):
        assert once(ctx) == first
    res, errs = {}, []

    def run(i):
        try:
            c = capi.Context(capi.params("launch"), capi.limits(2, 1024))
            c.set_batches_in_flight(4)
            for _ in range(4):
                res[i] = once(c)
            c.close()
        except Exception as e:  # (reported below)
            errs.append(e)
    ths = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    [x.start() for x in ths]
    [x.join() for x in ths]
    assert not errs, errs
    assert all(res[i] == first for i in range(4))
    # a smaller call on the context that has just held a larger one: nothing stale in its scratch
    small = tu.random_case(rng, [5, 0, 7, 7, 3], p_link=0.9)
    _run(ctx, small, "(e) smaller second call")
    _run(ctx, tu.random_case(rng, [4], p_link=0.9), "(e) one scan", min_obs=1)
    _run(ctx, tu.random_case(rng, [0, 0], p_link=0.9), "(e) no rows")


def _batch(c, scans, roll, pitch):
    """One batch: (kp_offset, keypoint rows on the host, the keypoint block on the device, the CSR block on the device)."""
    import torch
    scans = [np.ascontiguousarray(s, dtype=np.float32) for s in scans]
    descs = c.make_descs([s.ctypes.data for s in scans], [len(s) for s in scans], 16, roll, pitch)
    v = c.process_raw(descs, len(scans), capi.FX_OUT_HOST)
    off = capi._np(v.h_kp_offset, (len(scans) + 1,), np.uint32)
    S, R, cap = c.limits.max_batch, c.limits.max_total_keypoints, c.limits.max_total_keypoints * 128
    kp = torch.full((int(c.lib.fx_keypoint_block_bytes(S, R)),), 0xA5, dtype=torch.uint8, device=f"cuda:{c.device}")
    ext, cur = torch.cuda.ExternalStream(c.stream_ptr()), torch.cuda.current_stream()
    ext.wait_stream(cur)
    c.pack_keypoint_block(kp.data_ptr(), S, R)
    cur.wait_stream(ext)
    buf = torch.empty(int(c.lib.fx_descriptor_csr_bytes(R, cap)), dtype=torch.uint8, device=f"cuda:{c.device}")
    c.descriptors_csr(buf, R, cap)
    blk = capi.keypoint_block_parse(kp.cpu().numpy(), S, R)
    assert blk["kp_offset"].tolist() == off.tolist()
    return off, blk, (kp, S, R), (buf, R, cap)


def _chain(c, scans, what, roll=0.0, pitch=0.0):
    """process -> pack block + CSR -> match (mutual) -> register -> track on the device; the track compared bit for bit with the
    reference fed the device's own match and register records."""
    off, blk, kp, csr = _batch(c, scans, roll, pitch)
    pairs = capi.pairs_consecutive(off)
    md = c.match_descriptors(csr, csr, pairs, mutual=True)
    reg, inl = c.register_matches(kp, kp, md, pairs)
    got = _call(c, kp, md, inl, reg, len(scans))
    rg = capi.register_records(reg)
    ref = capi.track_reference(blk["kp_offset"], blk["rows"], capi.match_records(md), inl.cpu().numpy(), rg, len(scans))
    tu.assert_equal(got, ref, what)
    return got, rg, off


def test_f_end_to_end_five_rotated_copies(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(8, 28800))
    got, rg, off = _chain(c, tu.rotated_copies(), "(f) rotated copies")  # (no levelling: the clouds differ by exactly the rotations)
    err, full, rms = tu.chain_checks(got, rg, int(off[1]))
    print(f"(f) keypoints {np.diff(off).tolist()}, inliers {rg['n_inliers'].tolist()}, final pose error at 50 m + translation {err:.2e} m, "
          f"{got['header']['n_landmarks']} landmarks, {full} of 5 observations, worst rms_xy {rms:.2e} m")
    c.close()


def test_f_end_to_end_config3_batch(fxlib):
    p = capi.params("launch", n_rings=64, el0_deg=-24.8, el_step_deg=26.8 / 63, secondary_max=64)
    lim = capi.limits(4, 64 * 2048, max_candidates=4096, max_kpc_points=32768, max_keypoints=512, max_total_keypoints=4 * 256)
    c = capi.Context(p, lim)
    got, rg, off = _chain(c, [capi.synth_scan(capi.synth_cfg(10 + b, **HDL64)) for b in range(4)], "(f) config3", roll=0.02, pitch=-0.015)
    print(f"(f) config3: keypoints {np.diff(off).tolist()}, {got['header']}")
    assert got["header"]["scans"] == 4 and got["header"]["rows"] == int(off[-1])
    c.close()
