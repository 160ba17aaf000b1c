"""fx_splice_blocks on the GPU.  Hand-built block pairs are uploaded, spliced into destinations filled with a byte pattern, and
compared with capi.splice_reference byte for byte, without tolerance: the whole keypoint block, the CSR header, all max_rows + 1
words of row_ptr, col / val below nnz_stored, the fill pattern wherever the call defines nothing (the sections' padding, col / val
from nnz_stored on), the guard bytes behind both destination blocks, and every byte of the sources.  Then the premise — a scan's
blocks do not depend on its batch — on processed scans, and the purpose: the map fed every scan once."""
import ctypes as C

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_util as mu
from tests import splice_util as su
from tests import track_util as tu
from tests import util

pytestmark = pytest.mark.gpu
GUARD = 1024  # bytes behind each destination block that the call must leave alone
PLAN_WG = 1024  # csrc/fx_splice.hip: rows a round of k_splice_plan's count


@pytest.fixture(scope="module")
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def _filled(ctx, nbytes):
    import torch
    return torch.full((nbytes + GUARD,), su.FILL, dtype=torch.uint8, device=f"cuda:{ctx.device}")


def _splice(ctx, what, a, b, dst_kp, dst_csr):
    """The sources (as capi.splice_reference takes them) uploaded — one upload a distinct array, so a == b stays one block —, spliced,
    and everything compared with the reference.  Returns the destination's bytes (keypoint block, CSR block or None)."""
    import torch
    up = {}

    def dev(arr):
        if id(arr) not in up:
            up[id(arr)] = (arr, torch.from_numpy(arr.copy()).cuda())
        return up[id(arr)][1]

    def src(s):
        (kb, scans, total), csr, scan0, n_scans = s
        return ((dev(kb), scans, total), None if csr is None else (dev(csr[0]), csr[1], csr[2]), scan0, n_scans)
    nk = int(ctx.lib.fx_keypoint_block_bytes(*dst_kp))
    nc = int(ctx.lib.fx_descriptor_csr_bytes(*dst_csr)) if dst_csr is not None else 0
    dk, dc = _filled(ctx, nk), _filled(ctx, nc)
    torch.cuda.synchronize()
    ctx.splice_blocks(src(a), src(b), (dk[:nk], *dst_kp), (dc[:nc], *dst_csr) if dst_csr is not None else None)
    ctx.synchronize()
    gk, gc = dk.cpu().numpy(), dc.cpu().numpy()
    ref_kp, ref_csr = capi.splice_reference(a, b, dst_kp, dst_csr)
    su.assert_blocks(gk[:nk], gc[:nc] if dst_csr is not None else None, ref_kp, None if ref_csr is None else su.csr_image(ref_csr, *dst_csr), what)
    assert (gk[nk:] == su.FILL).all() and (gc[nc:] == su.FILL).all(), f"{what}: the guard bytes behind the destination"
    for arr, t in up.values():
        assert (t.cpu().numpy() == arr).all(), f"{what}: a source block was written"
    return gk[:nk], gc[:nc] if dst_csr is not None else None


def test_the_hand_built_cases_of_the_reference_test(ctx):
    cases = su.cases(np.random.default_rng(71))
    for what, a, b, parts, dst_kp, dst_csr in cases:
        gk, gc = _splice(ctx, what, a, b, dst_kp, dst_csr)
        want_kp, want_csr = su.expected(parts, dst_kp, dst_csr)  # (the independent construction as well)
        su.assert_blocks(gk, gc, want_kp, want_csr, f"{what}, by hand")
    # the same bytes from run to run
    what, a, b, parts, dst_kp, dst_csr = cases[0]
    first = _splice(ctx, what, a, b, dst_kp, dst_csr)
    for _ in range(3):
        again = _splice(ctx, what, a, b, dst_kp, dst_csr)
        assert (again[0] == first[0]).all() and (again[1] == first[1]).all()


@pytest.mark.parametrize("src_word", [0, 1, 2, 3])
def test_runs_at_every_alignment_of_source_and_destination(ctx, src_word):
    """b's entries begin at word src_word (mod 4) of its col / val and land at word dst_word (mod 4) of the destination's, for
    every pair of the two and runs of 0 .. 257 entries; a's run begins at src_word as well and lands at word 0."""
    rng = np.random.default_rng(73 + src_word)
    for dst_word in range(4):
        for run in (0, 1, 3, 4, 5, 63, 64, 65, 257):
            A = su.Source(rng, (1, 1), nnz=[4 + src_word, 8 + dst_word])
            B = su.Source(rng, (1, 1), nnz=[4 + src_word, run], special=run >= 3)
            assert int(A.csr.view(np.uint32)[5]) % 4 == src_word and int(B.csr.view(np.uint32)[5]) % 4 == src_word  # row_ptr[1]
            parts = [(A, 1, 2), (B, 1, 2)]
            for cap in (0, 3):  # the last vector of col / val full or not, whatever the run
                dst_kp, dst_csr = su.room(parts, cap=cap)
                assert (dst_csr[1] - cap - run) % 4 == dst_word
                _splice(ctx, f"source word {src_word}, destination word {dst_word}, {run} entries, {cap} to spare", A.src(su.LAST, 1), B.src(1, 1), dst_kp, dst_csr)


@pytest.mark.parametrize("n", [255, 256, 257, PLAN_WG + 1])
def test_rows_and_scans_at_the_tile_edges(ctx, n):
    rng = np.random.default_rng(77 + n)
    A = su.Source(rng, (2, 3), special=True)
    B = su.Source(rng, (1, n), special=True)
    parts = [(A, 1, 2), (B, 0, 2)]
    _splice(ctx, f"{n} rows", A.src(su.LAST, 1), B.src(0, su.ALL), *su.room(parts))
    (dk, dc) = su.room(parts)
    _splice(ctx, f"{n} rows, cut in b", A.src(su.LAST, 1), B.src(0, su.ALL), dk, (dc[0] - 2, dc[1] - 40))
    if n > 257:
        return
    Cs = su.Source(rng, rng.integers(0, 3, n))
    parts = [(A, 1, 2), (Cs, 0, n)]
    _splice(ctx, f"{n} scans", A.src(su.LAST, 1), Cs.src(0, su.ALL), *su.room(parts))
    _splice(ctx, f"{n} scans behind {n} scans", Cs.src(0, su.ALL), Cs.src(0, su.ALL), *su.room([(Cs, 0, n), (Cs, 0, n)]))


@pytest.mark.parametrize("max_scans", [1, 3, 4, 5])
def test_destination_scan_sections_of_every_padding(ctx, max_scans):
    """The offset and the flag section hold four words a row: max_scans + 1 and max_scans words at every remainder, with n below, at
    and above max_scans."""
    rng = np.random.default_rng(79 + max_scans)
    A, B = su.Source(rng, (2, 0, 3), flags=[8, 16, 64]), su.Source(rng, (1, 4, 2), flags=[32, 8, 1])
    for a_sel, b_sel, parts in (((su.LAST, 1), (0, 0), [(A, 2, 3)]), ((1, 2), (0, 1), [(A, 1, 3), (B, 0, 1)]), ((0, su.ALL), (0, su.ALL), [(A, 0, 3), (B, 0, 3)])):
        _, dst_csr = su.room(parts)
        gk, _ = _splice(ctx, f"max_scans {max_scans}, {sum(p[2] - p[1] for p in parts)} scans", A.src(*a_sel), B.src(*b_sel), (max_scans, 20), dst_csr)
        su.assert_blocks(gk, None, su.expected(parts, (max_scans, 20))[0], None, "by hand")


def test_host_refusals_launch_nothing(ctx, fxlib):
    import torch
    rng = np.random.default_rng(81)
    A, B = su.Source(rng, (2, 3)), su.Source(rng, (1, 4))
    parts = [(A, 1, 2), (B, 0, 2)]
    dst_kp, dst_csr = su.room(parts)
    t = {k: torch.from_numpy(v.copy()).cuda() for k, v in (("ak", A.kp), ("ac", A.csr), ("bk", B.kp), ("bc", B.csr))}
    nk, nc = int(fxlib.fx_keypoint_block_bytes(*dst_kp)), int(fxlib.fx_descriptor_csr_bytes(*dst_csr))
    dk, dc = _filled(ctx, nk), _filled(ctx, nc)
    big = torch.zeros(len(A.kp) + 64, dtype=torch.uint8, device=dk.device)  # (a source inside it, a destination over its start)
    big[32:32 + len(A.kp)] = t["ak"]

    def call(ctx_h=ctx.handle, a=None, b=None, dkp=dk.data_ptr(), dcp=dc.data_ptr(), kp=dst_kp, **kw):
        sa = capi.FxSpliceSource(t["ak"].data_ptr(), A.max_scans, A.max_total, t["ac"].data_ptr(), A.max_rows, A.cap, su.LAST, 1)
        sb = capi.FxSpliceSource(t["bk"].data_ptr(), B.max_scans, B.max_total, t["bc"].data_ptr(), B.max_rows, B.cap, 0, su.ALL)
        for name, v in kw.items():
            setattr(sa if name.startswith("a_") else sb, name[2:], v)
        pa, pb = (None if a is False else C.byref(sa)), (None if b is False else C.byref(sb))
        st = fxlib.fx_splice_blocks(ctx_h, pa, pb, dkp, kp[0], kp[1], dcp, dst_csr[0], dst_csr[1])
        return st, fxlib.fx_last_error()
    bad = [(dict(ctx_h=None), b"null"), (dict(a=False), b"null"), (dict(b=False), b"null"), (dict(dkp=None), b"null"),
           (dict(a_kp_block_device=None), b"null"), (dict(b_kp_block_device=None), b"null"),
           (dict(a_csr_block_device=None), b"both sources"), (dict(b_csr_block_device=None), b"both sources"),
           (dict(dkp=dk.data_ptr() + 8), b"aligned"), (dict(dcp=dc.data_ptr() + 4), b"aligned"), (dict(a_kp_block_device=t["ak"].data_ptr() + 4), b"aligned"),
           (dict(b_csr_block_device=t["bc"].data_ptr() + 8), b"aligned"),
           (dict(a_max_scans=0), b"no scans"), (dict(b_max_scans=0), b"no scans"), (dict(kp=(0, dst_kp[1])), b"no scans"),
           (dict(dkp=t["ak"].data_ptr()), b"overlaps"), (dict(dcp=t["bc"].data_ptr()), b"overlaps"), (dict(dkp=t["bc"].data_ptr()), b"overlaps"),
           (dict(a_kp_block_device=big.data_ptr() + 32, dkp=big.data_ptr()), b"overlaps"),
           (dict(b_csr_block_device=dc.data_ptr() + 16 * ((nc - 1) // 16)), b"overlaps")]
    before = {k: v.clone() for k, v in t.items()}
    for kw, word in bad:
        st, err = call(**kw)
        assert st == 1 and word in err, (kw, st, err)
    ctx.synchronize()
    assert (dk == su.FILL).all().item() and (dc == su.FILL).all().item() and not big[:32].any().item()
    assert all((t[k] == before[k]).all().item() for k in t)
    # a source CSR pointer is not looked at without a destination for it; the same arguments, none missing, run
    assert call(dcp=None, a_csr_block_device=4, b_csr_block_device=None)[0] == capi.FX_OK
    assert call()[0] == capi.FX_OK
    ctx.synchronize()
    ref_kp, ref_csr = capi.splice_reference(A.src(su.LAST, 1), B.src(0, su.ALL), dst_kp, dst_csr)
    su.assert_blocks(dk[:nk].cpu().numpy(), dc[:nc].cpu().numpy(), ref_kp, su.csr_image(ref_csr, *dst_csr), "after the refusals")


def test_a_scan_gives_the_same_blocks_in_any_batch(fxlib):
    """The premise.  [s0, s1] and [s2] are processed and packed; (first, LAST, 1) spliced with (second, 0, 1) must be the block pair
    of [s1, s2] processed as one batch: the keypoint blocks byte for byte, the CSR blocks in every word the pack defines."""
    import torch
    from tests.test_gpu_track import _batch
    c = capi.Context(capi.params("launch"), capi.limits(2, 28800))
    s = [util.vlp16_scan(seed) for seed in su.PREMISE_SEEDS]
    _, _, kp1, csr1 = _batch(c, s[:2], 0.02, -0.015)
    _, _, kp2, csr2 = _batch(c, s[2:], 0.02, -0.015)
    (_, S, R), (_, _, cap) = kp1, csr1
    nk, nc = int(fxlib.fx_keypoint_block_bytes(S, R)), int(fxlib.fx_descriptor_csr_bytes(R, cap))
    dk, dc = _filled(c, nk), _filled(c, nc)
    c.splice_blocks((kp1, csr1, su.LAST, 1), (kp2, csr2, 0, 1), (dk[:nk], S, R), (dc[:nc], R, cap))
    c.synchronize()
    off, blk, kp3, csr3 = _batch(c, s[1:], 0.02, -0.015)
    assert len(off) == 3 and min(np.diff(off.astype(np.int64))) >= 2, off
    got, want = dk.cpu().numpy(), kp3[0].cpu().numpy()
    assert (got[nk:] == su.FILL).all() and (dc[nc:] == su.FILL).all().item()
    su.assert_blocks(got[:nk], None, want[:nk], None, "the keypoint block of [s1, s2]")
    g, w = capi.csr_parse(dc[:nc].cpu().numpy(), R, cap), capi.csr_parse(csr3[0].cpu().numpy(), R, cap)
    assert w["rows"] == int(off[2]) and w["rows_stored"] == w["rows"] and w["nnz_stored"] > w["rows"], w
    for k in ("rows", "nnz_stored", "nnz_needed", "rows_stored"):
        assert g[k] == w[k], (k, g[k], w[k])
    for k in ("row_ptr_all", "col", "val"):
        assert (util.bits(g[k]) == util.bits(w[k])).all() if k == "val" else (g[k] == w[k]).all(), k
    c.close()


def test_the_map_fed_every_scan_once(ctx):
    """The purpose.  tests/test_gpu_map.py's world (a), every piece uploaded WITHOUT its overlap scan and spliced behind the last scan
    of the block before: the spliced block is the overlapping piece's block, and track -> fx_map_update on it gives the reference's
    map as it does today."""
    import torch
    from tests.test_gpu_map import _case_a, _step
    from tests.test_gpu_track import _upload
    w, pieces = _case_a(np.random.default_rng(51))
    mp, st = ctx.map_create(64, 16), capi.map_state(64, 16)
    prev = None
    for k, p in enumerate(pieces):
        S, K = p["n_scans"] + 2, len(p["rows"]) + 9  # (the layout _step gives a piece)
        kp, md, inl, reg = _upload(p, S, K)
        if k:
            first = int(p["off"][1])
            cur = tu.block(p["off"][1:] - p["off"][1], p["rows"][first:], S, K)
            dst = _filled(ctx, len(cur))
            ctx.splice_blocks((prev, None, su.LAST, 1), ((torch.from_numpy(cur).cuda(), S, K), None, 0, su.ALL), (dst[:len(cur)], S, K))
            ctx.synchronize()
            got = dst.cpu().numpy()
            want = su.kp_block(np.diff(p["off"].astype(np.int64)).tolist(), p["rows"], [0] * p["n_scans"], S, K)
            su.assert_blocks(got[:len(cur)], None, want, None, f"piece {k} spliced")
            stored = 16 * (capi.keypoint_block_layout(S, K).k0 + len(p["rows"]))
            assert (got[:stored] == kp[0].cpu().numpy()[:stored]).all() and (got[len(cur):] == su.FILL).all(), f"piece {k}: the uploaded piece's block"
            kp = (dst[:len(cur)], S, K)
        st, _, _ = _step(ctx, mp, st, p, k > 0, f"every scan once, piece {k}", dev_in=(kp, md, inl, reg))
        prev = kp
    assert st["header"]["n_landmarks"] > 0 and st["header"]["scans"] == 12, st["header"]
    mu.assert_equal(mp.records(), capi.map_state_records(st), "every scan once")
    mp.close()
