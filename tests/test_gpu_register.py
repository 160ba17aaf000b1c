"""fx_register_matches on the GPU.  Every case checks four things: the integer fields and the inlier words equal
capi.register_reference on the same inputs, the five doubles and rms equal it bit for bit (the definition uses only ordered,
correctly rounded operations: there is no tolerance), and the guard regions behind `out` and behind the inlier words are
untouched."""
import math
import threading

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import register_util as ru
from tests import util

pytestmark = pytest.mark.gpu
GUARD = 1024  # int32 words behind each output that the call must leave alone
FILL = 0x5A5A5A5A
HDL64 = dict(n_rings=64, n_az=2048, el0_deg=-24.8, el_step_deg=26.8 / 63, n_poles=256)
ACC, MUT = capi.FX_MATCH_ACCEPTED, capi.FX_MATCH_MUTUAL
VALID, TRUNC, NOHYP = capi.FX_REG_VALID, capi.FX_REG_TRUNCATED, capi.FX_REG_NO_HYPOTHESIS


@pytest.fixture
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def _register(ctx, q_kp, t_kp, matches, pairs, inliers=True, **opts):
    """Context.register_matches into guarded outputs: (REG_DTYPE records, inlier words or None)."""
    import torch
    dev = f"cuda:{ctx.device}"
    n_rows, n_pairs = int(matches.shape[0]), len(pairs)
    raw_o = torch.full((n_pairs * 16 + GUARD,), FILL, dtype=torch.int32, device=dev)
    raw_i = torch.full((n_rows + GUARD,), FILL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    out, inl = ctx.register_matches(q_kp, t_kp, matches, pairs, out=raw_o[:n_pairs * 16].view(torch.float64).view(n_pairs, 8),
                                    inliers=raw_i[:n_rows] if inliers else False, **opts)
    ctx.synchronize()
    assert (raw_o[n_pairs * 16:] == FILL).all().item(), "the guard behind the records"
    assert (raw_i[n_rows if inliers else 0:] == FILL).all().item(), "the guard behind the inlier words"
    return capi.register_records(out), (inl.cpu().numpy() if inliers else None)


def _dev_block(rows, max_scans, max_total):
    import torch
    blk, s, t = capi.keypoint_block_from_rows(rows, max_scans, max_total)
    return (torch.from_numpy(blk).cuda(), s, t)


def _dev_matches(m, q_max_rows):
    import torch
    full = ru.records(q_max_rows, -1, np.inf, flags=0, pair=capi.FX_MATCH_NO_PAIR)
    full[:len(m)] = m
    return torch.from_numpy(full.view(np.int32).reshape(-1, 8).copy()).cuda(), full


def _run(ctx, q, t, m, pairs, what, q_stored=None, t_stored=None, q_max_rows=None, inliers=True, **opts):
    """Host rows -> device blocks storing the first *_stored rows (laid out for more), the records padded to q_max_rows with
    no-pair sentinels; registered on the GPU and compared with the reference."""
    qs, ts = len(q) if q_stored is None else q_stored, len(t) if t_stored is None else t_stored
    q_kp, t_kp = _dev_block(q[:qs], 3, len(q) + 5), _dev_block(t[:ts], 1, len(t))
    md, full = _dev_matches(m, len(m) if q_max_rows is None else q_max_rows)
    got, inl = _register(ctx, q_kp, t_kp, md, pairs, inliers=inliers, **opts)
    ref = capi.register_reference(q[:qs], t[:ts], full, pairs, **opts)
    ru.assert_equal(got, inl, ref, what)
    f = ref["rec"]["flags"]
    print(f"{what}: {len(pairs)} pairs, {int(((f & VALID) != 0).sum())} valid, {int(((f & NOHYP) != 0).sum())} without a hypothesis, "
          f"{int(((f & TRUNC) != 0).sum())} truncated, {int(ref['inlier'].sum())} inlier rows of {int(ref['rec']['n_corr'].sum())} correspondences")
    return got, inl, ref


def test_a_many_pairs_of_varied_sizes_and_every_special_case(ctx):
    rng = np.random.default_rng(21)
    sizes = [0, 1, 2, 54, 512, 1100, 3, 4, 1024, 1025] + [int(x) for x in rng.integers(0, 90, 290)]
    q, t, m, pairs = ru.multi_pair_case(rng, sizes, gap=2)
    # special rows inside ordinary pairs: non-finite coordinates, two queries on one train row, records that are not accepted,
    # a record of another pair, a train row beyond the block
    q0 = pairs[3][0]
    q[q0 + 5, 0], q[q0 + 9, 2] = np.nan, np.inf
    t[m["train_row"][q0 + 11], 1] = -np.inf
    m["train_row"][q0 + 20] = m["train_row"][q0 + 21]
    m["flags"][q0 + 30] = 0
    m["pair"][q0 + 31] = 4
    m["train_row"][q0 + 32] = len(t) + 7
    m["train_row"][q0 + 33] = -1
    q1 = pairs[4][0]
    q[q1:q1 + 512:7, 3] = np.nan  # (elevation: not a coordinate)
    # a pair too small in extent for min_baseline
    q6, n6 = pairs[11][:2]
    q[q6:q6 + n6, :2] *= 0.001
    # clipped ranges and empty sides
    last = len(pairs) - 1
    pairs[last] = (pairs[last][0], pairs[last][1] + 45, pairs[last][2], pairs[last][3])  # beyond q_max_rows: clipped
    pairs += [(len(m) + 50, 10, 0, 10), (0xfffffff0, 0x40, 0xfffffff0, 0x40), (len(m) + 1, 0, 0, 0)]
    got, inl, ref = _run(ctx, q, t, m, pairs, "(a)", q_stored=len(q) - 3, t_stored=len(t) - 2, q_max_rows=len(m) + 40)
    r = ref["rec"]
    assert r["n_corr"][:6].tolist() == [0, 1, 2, 54 - 7, 512, 1024] and r["n_corr"][8:10].tolist() == [1024, 1024]
    assert (r["flags"][[0, 1]] == NOHYP).all() and r["flags"][5] == VALID | TRUNC and r["flags"][8] == VALID and r["flags"][9] == VALID | TRUNC
    assert (r["flags"][-3:] == NOHYP).all() and r["flags"][11] & NOHYP
    assert ((r["flags"] & VALID) != 0).sum() > 250 and inl[len(m):].sum() == 0


@pytest.mark.parametrize("opts", [dict(hyp_corr=2), dict(hyp_corr=7), dict(hyp_corr=128), dict(inlier_dist=0.05), dict(inlier_dist=2.0),
                                  dict(require_flags=ACC | MUT), dict(min_baseline=30.0, min_inliers=10),
                                  dict(hyp_corr=128, inlier_dist=0.1, min_baseline=0.5, min_inliers=2, require_flags=0)],
                         ids=["hyp2", "hyp7", "hyp128", "tight", "wide", "mutual", "baseline", "all"])
def test_b_options(ctx, opts):
    rng = np.random.default_rng(22)
    q, t, m, pairs = ru.multi_pair_case(rng, [200, 54, 30, 7, 3, 150, 0, 129, 128], outlier_share=0.4, sigma=0.04)
    m["flags"][rng.random(len(m)) < 0.6] |= MUT
    m["flags"][rng.random(len(m)) < 0.1] &= ~np.uint32(ACC)
    got, _, ref = _run(ctx, q, t, m, pairs, f"(b) {opts}", **opts)
    assert (got["flags"] & VALID).any()
    if opts.get("hyp_corr") == 2:
        assert (got["flags"] & NOHYP).any()  # (one sample: it may well be a wrong one)


def test_c_host_refusals_launch_nothing(ctx):
    import torch
    rng = np.random.default_rng(23)
    q, t, m, pairs = ru.multi_pair_case(rng, [20, 20])
    q_kp, t_kp = _dev_block(q, 1, len(q)), _dev_block(t, 1, len(t))
    md, _ = _dev_matches(m, len(m))
    out = torch.full((2, 8), -7.25, dtype=torch.float64, device="cuda")
    inl = torch.full((len(m),), FILL, dtype=torch.int32, device="cuda")
    bad = [dict(pairs=[(0, 20, 0, 20), (19, 5, 0, 20)]), dict(hyp_corr=1), dict(hyp_corr=129), dict(min_inliers=1), dict(min_inliers=0),
           dict(inlier_dist=0.0), dict(inlier_dist=-1.0), dict(inlier_dist=math.inf), dict(inlier_dist=math.nan), dict(min_baseline=0.0),
           dict(min_baseline=math.inf), dict(min_baseline=math.nan)]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(capi.FxError, match="status 1"):
            ctx.register_matches(q_kp, t_kp, md, kw.pop("pairs", pairs), out=out, inliers=inl, **kw)
    ctx.synchronize()
    assert (out == -7.25).all().item() and (inl == FILL).all().item()
    ctx.register_matches(q_kp, t_kp, md, [(0, 20, 0, 20), (20, 20, 0, 5), (10, 0, 0, 5)], out=torch.empty((3, 8), dtype=torch.float64, device="cuda"))


def _config(name, B):
    if name == "vlp16":
        return capi.params("launch"), capi.limits(B, 28800), [util.vlp16_scan(1000 + b) for b in range(B)]
    p = capi.params("launch", n_rings=64, el0_deg=-24.8, el_step_deg=26.8 / 63, secondary_max=64)
    lim = capi.limits(B, 64 * 2048, max_candidates=4096, max_kpc_points=32768, max_keypoints=512, max_total_keypoints=B * 256)
    return p, lim, [capi.synth_scan(capi.synth_cfg(10 + b, **HDL64)) for b in range(B)]


def _batch(c, scans, roll=0.02, pitch=-0.015):
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
    _, hdr = c.descriptors_csr(buf, R, cap)
    blk = capi.keypoint_block_parse(kp.cpu().numpy(), S, R)
    assert hdr["rows_stored"] == hdr["rows"] == blk["keypoints"] == int(off[-1]) and blk["kp_offset"].tolist() == off.tolist()
    return off, blk["rows"], (kp, S, R), (buf, R, cap)


def _chain(c, q, t, pairs, what, **opts):
    """match (mutual) + register on the device, q / t = _batch results; compared with the reference fed the downloaded keypoint
    rows and the GPU's own match records."""
    md = c.match_descriptors(q[3], t[3], pairs, mutual=True)
    got, inl = _register(c, q[2], t[2], md, pairs, **opts)
    ref = capi.register_reference(q[1], t[1], capi.match_records(md), pairs, **opts)
    ru.assert_equal(got, inl, ref, what)
    print(f"{what}: " + "; ".join(f"{r['n_inliers']}/{r['n_corr']} flags {r['flags']:#x} yaw {math.degrees(math.atan2(r['s'], r['c'])):.3f} deg "
                                  f"t ({r['tx']:.3f}, {r['ty']:.3f}, {r['tz']:.3f}) rms {r['rms']:.4f}" for r in got[:6]))
    return got, inl


@pytest.mark.parametrize("name,B", [("vlp16", 16), ("config3", 4)])
def test_d_end_to_end_in_batch_pairs_consecutive(fxlib, name, B):
    p, lim, scans = _config(name, B)
    c = capi.Context(p, lim)
    b = _batch(c, scans)
    pairs = capi.pairs_consecutive(b[0])
    assert len(pairs) == B - 1 and len(b[1]) > B
    got, inl = _chain(c, b, b, pairs, name)
    assert (got["n_corr"] > 0).all() and inl[:b[0][1]].sum() == 0  # scan 0 is nobody's query
    _chain(c, b, b, pairs, name + " mutual only", require_flags=ACC | MUT, min_baseline=1.0)
    c.close()


def test_e_a_scan_its_copy_and_its_rotated_copy(fxlib):
    A = util.vlp16_scan(1000)
    th = math.radians(3.0)
    Bs = A.copy()
    x, y = A[:, 0].astype(np.float64), A[:, 1].astype(np.float64)
    Bs[:, 0], Bs[:, 1] = (math.cos(th) * x - math.sin(th) * y).astype(np.float32), (math.sin(th) * x + math.cos(th) * y).astype(np.float32)
    c = capi.Context(capi.params("launch"), capi.limits(4, 28800))
    b = _batch(c, [A, A, Bs], roll=0.0, pitch=0.0)  # (no levelling: the clouds differ by exactly the rotation)
    off = b[0]
    K = int(off[1])
    assert K > 10 and off[2] == 2 * K and (util.bits(b[1][:K]) == util.bits(b[1][K:2 * K])).all()
    got, inl = _chain(c, b, b, capi.pairs_consecutive(off), "(e)")
    same, rot = got[0], got[1]
    # a scan against itself: exactly the identity
    assert same["flags"] == VALID and 2 * same["n_inliers"] >= same["n_corr"] > 10
    for f, v in (("c", 1.0), ("s", 0.0), ("tx", 0.0), ("ty", 0.0), ("tz", 0.0), ("rms", 0.0)):
        assert same[f] == v, (f, same[f])
    # the rotated copy is the query: the motion back onto the scan is the opposite rotation, no translation
    err = abs(math.atan2(rot["s"], rot["c"]) + th) * 50.0 + math.hypot(rot["tx"], rot["ty"])
    print(f"(e) rotated copy: error at 50 m + translation {err:.5f} m")
    assert rot["flags"] & VALID and err <= 0.30 and 2 * rot["n_inliers"] >= rot["n_corr"]
    c.close()


def test_f_kept_blocks_of_one_batch_against_the_next(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(4, 28800))
    b1 = _batch(c, [util.vlp16_scan(1000 + b) for b in range(3)])
    b2 = _batch(c, [util.vlp16_scan(1001 + b) for b in range(3)])  # (scan b of this one is scan b + 1 of the last)
    off1, off2 = b1[0], b2[0]
    pairs = [(int(off2[b]), int(off2[b + 1] - off2[b]), int(off1[b]), int(off1[b + 1] - off1[b])) for b in range(3)]
    got, _ = _chain(c, b2, b1, pairs, "(f)")
    assert (got["n_corr"] > 0).all()
    back = [(t0, tn, q0, qn) for q0, qn, t0, tn in pairs]
    _chain(c, b1, b2, back, "(f) reversed")
    c.close()


def test_g_identical_bytes_from_run_to_run_and_across_contexts(ctx):
    rng = np.random.default_rng(24)
    q, t, m, pairs = ru.multi_pair_case(rng, [300, 54, 54, 20, 1100, 9] + [int(x) for x in rng.integers(10, 70, 60)], outlier_share=0.5)
    qh, th_ = capi.keypoint_block_from_rows(q, 2, len(q)), capi.keypoint_block_from_rows(t, 2, len(t))
    mh = m.view(np.int32).reshape(-1, 8).copy()

    def once(c):
        import torch
        got, inl = _register(c, (torch.from_numpy(qh[0]).cuda(), 2, len(q)), (torch.from_numpy(th_[0]).cuda(), 2, len(t)),
                             torch.from_numpy(mh).cuda(), pairs)
        return got.tobytes() + inl.tobytes()
    first = once(ctx)
    assert once(ctx) == first
    ref = capi.register_reference(q, t, m, pairs)
    assert first == ref["rec"].tobytes() + ref["inlier"].astype(np.int32).tobytes()
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


def test_h_smaller_second_call_and_no_inlier_words(ctx):
    rng = np.random.default_rng(25)
    q, t, m, pairs = ru.multi_pair_case(rng, [60] * 40)
    _run(ctx, q, t, m, pairs, "(h) first")
    q2, t2, m2, pairs2 = ru.multi_pair_case(rng, [5, 33])
    got, inl, ref = _run(ctx, q2, t2, m2, pairs2, "(h) second")
    assert len(got) == 2 and len(inl) == 38 and got["flags"][1] == VALID
    got3, none, _ = _run(ctx, q2, t2, m2, pairs2, "(h) no inlier words", inliers=False)
    assert none is None and got3.tobytes() == got.tobytes()
    # no pairs: nothing but zeroed inlier words; no rows at all
    got, inl, _ = _run(ctx, q2, t2, m2, [], "(h) no pairs")
    assert len(got) == 0 and not inl.any()
    got, inl, _ = _run(ctx, q2, t2, m2[:0], [(0, 5, 0, 5)], "(h) no rows")
    assert got["flags"][0] == NOHYP and len(inl) == 0
