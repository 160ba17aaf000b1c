"""fx_deskew_keypoint_block on the GPU.  Every case is held to capi.deskew_reference without tolerance: every byte of the destination
block, every field of every record (max_shift bit for bit), the guard bytes behind both outputs, and every byte of the source when
the call is not in place."""
import ctypes as C
import threading

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import deskew_util as du
from tests import register_util as ru
from tests import track_util as tu

pytestmark = pytest.mark.gpu
GUARD = 1024  # bytes behind each output that the call must leave alone
FILL = 0x5A
LINKS, PER_SCAN = capi.FX_DESKEW_LINKS, capi.FX_DESKEW_PER_SCAN


@pytest.fixture(scope="module")
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wd():
    return du.world(15.0, 0.3)


def _motions(m, need):
    """REG_DTYPE records as the device tensor the call takes: at least `need` records, the ones behind them a pattern nobody may read."""
    import torch
    if m is None:
        return None
    buf = np.zeros(max(len(m), need, 1), capi.REG_DTYPE)
    buf.view(np.uint8)[:] = 0xA5
    buf[:len(m)] = m
    return torch.from_numpy(buf.view(np.float64).reshape(-1, 8).copy()).cuda()


def _deskew(ctx, what, blk, S, K, m, n_scans, in_place=False, compare=True, **opts):
    """The block uploaded, de-skewed into a destination filled with a pattern (or in place) and compared with the reference.
    Returns (the destination block's bytes, the records)."""
    import torch
    dev = f"cuda:{ctx.device}"
    nbytes = len(blk)
    assert nbytes == int(ctx.lib.fx_keypoint_block_bytes(S, K))
    src = torch.from_numpy(blk.copy()).cuda()
    raw = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    if in_place:
        raw[:nbytes] = src
    out_raw = torch.full((n_scans * 4 + GUARD // 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    need = n_scans if opts.get("source", LINKS) == PER_SCAN else n_scans - 1
    torch.cuda.synchronize()
    ctx.deskew_keypoint_block((raw[:nbytes] if in_place else src, S, K), _motions(m, need), n_scans, dst=raw[:nbytes],
                              out=out_raw[:n_scans * 4].view(n_scans, 4), **opts)
    ctx.synchronize()
    got, rec = raw.cpu().numpy(), capi.deskew_records(out_raw[:n_scans * 4])
    assert (got[nbytes:] == FILL).all() and (out_raw[n_scans * 4:] == 0x5A5A5A5A).all().item(), f"{what}: the guard bytes behind the outputs"
    assert in_place or (src.cpu().numpy() == blk).all(), f"{what}: the source block was written"
    if compare:
        ref_blk, ref_rec = capi.deskew_reference(blk, S, K, m, n_scans, **opts)
        du.assert_equal(got[:nbytes], rec, ref_blk, ref_rec, what)
    return got[:nbytes], rec


@pytest.mark.parametrize("source", [LINKS, PER_SCAN])
def test_the_moving_world_under_every_option(ctx, wd, source):
    blk, S, K = du.block(wd)
    m = du.link_motions(wd) if source == LINKS else du.per_scan_motions(wd)
    moved = 0
    for direction in (-1, 1):
        for ref in (0.0, 0.5, 1.0):
            for sweep in (0.5, 1.0):
                for start in (0.5, 0.0):
                    opts = dict(source=source, direction=direction, ref_fraction=ref, sweep_fraction=sweep, start_turn=start)
                    _, rec = _deskew(ctx, f"{opts}", blk, S, K, m, wd["n_scans"], **opts)
                    moved += int(rec["rows_moved"].sum())
    assert moved > 20 * len(wd["rows"])
    # the defaults put every row on its pole to within the arcs' bound, as the reference does
    got, rec = _deskew(ctx, "defaults", blk, S, K, m, wd["n_scans"], source=source)
    rows = du.block_rows(got, S, K, len(wd["rows"]))
    ex = du.exact_rows(wd)
    assert np.hypot(rows[:, 0] - ex[:, 0], rows[:, 1] - ex[:, 1]).max() <= du.ARC_BOUND and int(rec["rows_moved"].sum()) == len(rows)


def test_estimated_links_with_noise(ctx):
    wn = du.world(30.0, 0.0, sigma=0.02)
    r1 = du.register(wn, wn["rows"])
    blk, S, K = du.block(wn)
    got, _ = _deskew(ctx, "estimated links", blk, S, K, r1["rec"], wn["n_scans"])
    err, share = du.pose_fits(wn, du.block_rows(got, S, K, len(wn["rows"]))[:, :2])
    assert err <= du.POSE_BOUND and share == 1.0, (err, share)


@pytest.mark.parametrize("source", [LINKS, PER_SCAN])
def test_edge_blocks_with_special_rows(ctx, source):
    """tu.edge_blocks (three scans, five rows, the middle one empty; a header of more scans than max_scans, fewer rows than stored,
    offsets that fall) with rows on the axes and diagonals, at +-0, denormal, at 1e30, NaN and infinite."""
    rng = np.random.default_rng(61)
    sp = du.special_rows(rng)
    for k in range(0, 30, 5):
        for e in tu.edge_blocks(sp[k:k + 5]):
            for n_scans in (1, 2, 3):
                m = du.random_motions(rng, 3)
                _deskew(ctx, f"rows {k}.., {e['what']}, {n_scans} scans", e["blk"], e["max_scans"], e["max_total"], m, n_scans, source=source)
                _deskew(ctx, f"rows {k}.., {e['what']}, {n_scans} scans, in place", e["blk"], e["max_scans"], e["max_total"], m, n_scans, in_place=True,
                        source=source, ref_fraction=0.5, sweep_fraction=0.5, direction=1)


def test_special_rows_link_choice_and_the_rows_that_stay(ctx):
    rng = np.random.default_rng(7)
    blk, S, K, off, rows = du.hand_case(rng)
    for what, m, n_scans, opts, flags in du.link_cases(rng):
        _, rec = _deskew(ctx, what, blk, S, K, m, n_scans, **opts)
        assert rec["flags"].tolist() == flags, (what, rec["flags"].tolist())
    lo = int(off[2])  # (the special rows: (10, 0) at lo, (-10, 0) at lo + 1)
    m = du.random_motions(rng, 5)
    for ref, row in ((0.5, lo), (0.0, lo + 1)):  # phi == ref_fraction: the row keeps its bytes
        got, rec = _deskew(ctx, f"ref_fraction {ref}", blk, S, K, m, 5, source=PER_SCAN, ref_fraction=ref)
        g = du.block_rows(got, S, K, len(rows))
        assert (tu.bits(g[row]) == tu.bits(rows[row])).all() and (tu.bits(g[row + 2, :2]) != tu.bits(rows[row + 2, :2])).any()
    # w == 1: the row behind the sensor under the defaults moves by the whole inverse, bit for bit
    got, rec = _deskew(ctx, "w == 1", blk, S, K, m, 5, source=PER_SCAN)
    c, s, tx, ty, tz = (float(m[f][2]) for f in ("c", "s", "tx", "ty", "tz"))
    x, y, z = (float(v) for v in rows[lo + 1, :3])
    want = np.array([(c * x - -s * y) + -(c * tx + s * ty), (-s * x + c * y) + (s * tx - c * ty), z + -tz], np.float64).astype(np.float32)
    assert (tu.bits(du.block_rows(got, S, K, len(rows))[lo + 1, :3]) == tu.bits(want)).all()
    assert rec["rows_moved"].tolist() == [7, 0, 27, 5, 6]
    _deskew(ctx, "phi rounds to 1", blk, S, K, m, 5, source=PER_SCAN, start_turn=1e-20, direction=1)


def test_n_scans_above_and_below_the_blocks(ctx, wd):
    blk, S, K = du.block(wd)
    m = du.random_motions(np.random.default_rng(9), S)
    for source in (LINKS, PER_SCAN):
        _, rec = _deskew(ctx, "n_scans above", blk, S, K, m, S, source=source)
        assert rec["flags"][9:].tolist() == [8, 8]
        for n in (1, 4, 8):
            _deskew(ctx, f"n_scans {n}", blk, S, K, m, n, source=source)
    # a block whose layout holds more than 256 rows and whose scans cross the workgroups
    rng = np.random.default_rng(10)
    big = tu.random_case(rng, [0, 255, 1, 257, 300, 0])
    b = tu.block(big["off"], big["rows"], 6, len(big["rows"]) + 3)
    _deskew(ctx, "813 rows", b, 6, len(big["rows"]) + 3, du.random_motions(rng, 6), 6)
    _deskew(ctx, "813 rows, fewer stored", tu.block(big["off"], big["rows"], 6, len(big["rows"]) + 3, stored=500), 6, len(big["rows"]) + 3,
            du.random_motions(rng, 6), 6, source=PER_SCAN)


def test_in_place_run_to_run_and_two_contexts(ctx, wd):
    blk, S, K = du.block(wd)
    m = du.link_motions(wd)
    first = _deskew(ctx, "out of place", blk, S, K, m, wd["n_scans"])
    again = _deskew(ctx, "in place", blk, S, K, m, wd["n_scans"], in_place=True)
    assert (first[0] == again[0]).all() and first[1].tobytes() == again[1].tobytes()
    for _ in range(3):
        again = _deskew(ctx, "again", blk, S, K, m, wd["n_scans"], compare=False)
        assert (first[0] == again[0]).all() and first[1].tobytes() == again[1].tobytes()
    res, errs = {}, []

    def run(i):
        try:
            c = capi.Context(capi.params("launch"), capi.limits(2, 1024))
            for _ in range(4):
                res[i] = _deskew(c, f"context {i}", blk, S, K, m, wd["n_scans"], compare=False)
            c.close()
        except Exception as e:  # (reported below)
            errs.append(e)
    ths = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, errs
    assert all((res[i][0] == first[0]).all() and res[i][1].tobytes() == first[1].tobytes() for i in range(2))


def test_register_deskew_register_on_the_device(ctx):
    """The intended chain with no host read between the calls: fx_register_matches -> fx_deskew_keypoint_block (LINKS, reading the
    records where the register left them) -> fx_register_matches on the corrected block with the same matches; equal to the
    references chained the same way."""
    import torch
    wn = du.world(15.0, 0.3, sigma=0.02)
    blk, S, K = du.block(wn)
    pairs = capi.pairs_consecutive(wn["off"])
    kp = (torch.from_numpy(blk.copy()).cuda(), S, K)
    md = torch.from_numpy(wn["m"].view(np.int32).reshape(-1, 8).copy()).cuda()
    torch.cuda.synchronize()
    reg1, inl1 = ctx.register_matches(kp, kp, md, pairs)
    kp2, out = ctx.deskew_keypoint_block(kp, reg1, wn["n_scans"])
    reg2, inl2 = ctx.register_matches(kp2, kp2, md, pairs)
    ctx.synchronize()
    r1 = du.register(wn, wn["rows"])
    ru.assert_equal(capi.register_records(reg1), inl1.cpu().numpy(), r1, "the first register")
    ref_blk, ref_rec = capi.deskew_reference(blk, S, K, r1["rec"], wn["n_scans"])
    du.assert_equal(kp2[0].cpu().numpy(), capi.deskew_records(out), ref_blk, ref_rec, "the de-skew behind the register")
    r2 = du.register(wn, du.block_rows(ref_blk, S, K, len(wn["rows"])))
    ru.assert_equal(capi.register_records(reg2), inl2.cpu().numpy(), r2, "the second register")
    err, share = du.pose_fits(wn, du.block_rows(kp2[0].cpu().numpy(), S, K, len(wn["rows"]))[:, :2])
    assert err <= du.POSE_BOUND and share == 1.0 and (ref_rec["flags"] & capi.FX_DESKEW_MOVED).all()


def test_host_refusals_launch_nothing(ctx, fxlib, wd):
    import torch
    blk, S, K = du.block(wd)
    n, nbytes = wd["n_scans"], len(blk)
    dev = f"cuda:{ctx.device}"
    src = torch.from_numpy(blk.copy()).cuda()
    dst = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
    big = torch.full((2 * nbytes + 64,), FILL, dtype=torch.uint8, device=dev)  # (a source inside it, destinations over its ends)
    big[32:32 + nbytes] = src
    out = torch.full((4 * S + 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    mot = _motions(du.link_motions(wd), S)
    torch.cuda.synchronize()

    def call(ctx_h=ctx.handle, s=src.data_ptr(), d=dst.data_ptr(), kp=(S, K), m=mot.data_ptr(), n_scans=n, o=out.data_ptr(), null_opt=False, **kw):
        opt = capi.FxDeskewOptions()
        fxlib.fx_deskew_options_default(C.byref(opt))
        for k, v in kw.items():
            setattr(opt, k, v)
        st = fxlib.fx_deskew_keypoint_block(ctx_h, s, d, kp[0], kp[1], m, n_scans, None if null_opt else C.byref(opt), o)
        return st, fxlib.fx_last_error()
    bad = [(dict(ctx_h=None), b"null"), (dict(s=None), b"null"), (dict(d=None), b"null"), (dict(o=None), b"null"), (dict(m=None), b"null"),
           (dict(m=None, n_scans=1, source=PER_SCAN), b"null"), (dict(m=None, n_scans=2), b"null"),
           (dict(n_scans=0), b"n_scans"), (dict(n_scans=S + 1), b"n_scans"),
           (dict(start_turn=float("nan")), b"start_turn"), (dict(start_turn=float("inf")), b"start_turn"),
           (dict(ref_fraction=-1e-9), b"ref_fraction"), (dict(ref_fraction=1.0 + 1e-9), b"ref_fraction"), (dict(ref_fraction=float("nan")), b"ref_fraction"),
           (dict(sweep_fraction=0.0), b"sweep_fraction"), (dict(sweep_fraction=1.0 + 1e-9), b"sweep_fraction"), (dict(sweep_fraction=float("nan")), b"sweep_fraction"),
           (dict(direction=0), b"direction"), (dict(direction=2), b"direction"), (dict(source=2), b"source"), (dict(reserved=1), b"reserved"),
           (dict(s=src.data_ptr() + 8), b"aligned"), (dict(d=dst.data_ptr() + 4), b"aligned"), (dict(m=mot.data_ptr() + 4), b"aligned"),
           (dict(o=out.data_ptr() + 2), b"aligned"),
           (dict(s=big.data_ptr() + 32, d=big.data_ptr()), b"overlaps"), (dict(s=big.data_ptr() + 32, d=big.data_ptr() + 48), b"overlaps"),
           (dict(s=big.data_ptr() + 32, d=big.data_ptr() + 16 + nbytes), b"overlaps")]
    for kw, word in bad:
        st, err = call(**kw)
        assert st == capi.FX_ERR_INVALID_ARG and word in err, (kw, st, err)
    ctx.synchronize()
    assert (dst == FILL).all().item() and (out == 0x5A5A5A5A).all().item() and (src.cpu().numpy() == blk).all()
    assert (big[:32] == FILL).all().item() and (big[32 + nbytes:] == FILL).all().item() and (big[32:32 + nbytes] == src).all().item()
    # the same arguments, none wrong, run: a destination that touches the source's end, in place, with the options, with NULL for
    # the defaults, and one scan without records
    ref_blk, ref_rec = capi.deskew_reference(blk, S, K, du.link_motions(wd), n)
    for kw in (dict(s=big.data_ptr() + 32, d=big.data_ptr() + 32 + nbytes), dict(s=big.data_ptr() + 32, d=big.data_ptr() + 32), dict(), dict(null_opt=True)):
        assert call(**kw)[0] == capi.FX_OK, kw
    ctx.synchronize()
    du.assert_equal(dst[:nbytes].cpu().numpy(), capi.deskew_records(out[:4 * n]), ref_blk, ref_rec, "after the refusals")
    assert (dst[nbytes:] == FILL).all().item() and (out[4 * n:] == 0x5A5A5A5A).all().item()
    assert call(m=None, n_scans=1)[0] == capi.FX_OK
    ctx.synchronize()
    assert capi.deskew_records(out[:4])["flags"].tolist() == [capi.FX_DESKEW_NO_MOTION]
