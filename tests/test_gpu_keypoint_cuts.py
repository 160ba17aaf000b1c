"""Keypoint-pool cuts end to end (include/fx.h "Cuts").  Batches of keypoint-heavy synthetic scenes (256 and 512 poles: some
140-220 keypoints a scan, beyond the default pool's average of 64) with max_total_keypoints placed exactly at, one short of,
inside and at the first row of a scan, and short enough to leave later scans with nothing; a 1024-scan batch whose cut falls
in the second FX_WG chunk of the offsets pass.  Every scan's detector outputs must stay the oracle's bit for bit, every row
the pool holds must be the oracle's row of the same keypoint, the flags must follow the stated rule, and every way results
leave the library must report the same held rows.  The per-scan cuts (max_keypoints, max_kpc_points) are checked the same way."""
import ctypes as C

import numpy as np
import pytest

from feature_extraction_amd import capi, sharding
from tests import util

pytestmark = pytest.mark.gpu

ROLL, PITCH = 0.02, -0.015
TOTAL, KPC = 0x10, 0x20  # FX_FLAG_TOTAL_KP_OVERFLOW, FX_FLAG_KPC_OVERFLOW
EMPTY = np.zeros((0, 4), np.float32)
# the cut batch: keypoint-heavy scenes, a plain VLP-16 one and two empty scans (one inside the batch, one at its end — past
# every cut below but the control)
SCENES = [(100, 256), (101, 512), (102, None), None, (103, 256), (104, 512), None]

_ORA = {}


def _scene(key):
    if key is None:
        return EMPTY
    seed, poles = key
    return util.vlp16_scan(seed) if poles is None else util.vlp16_scan(seed, n_poles=poles)


def _oracle(oracle, key):
    if key not in _ORA:  # (launch preset throughout)
        _ORA[key] = oracle.run(capi.params("launch"), _scene(key), roll=ROLL, pitch=PITCH)
    return _ORA[key]


def _held(off, K, M):
    """Rows of a scan the pool holds (include/fx.h "Cuts"): its leading ones, [off, off + K) clipped to [0, M)."""
    return max(0, min(off + K, M) - min(off, M))


def _run(ctx, scans):
    """process_host's dicts plus the view's total_keypoints and the unclamped offsets."""
    scans = [np.ascontiguousarray(s, np.float32) for s in scans]
    descs = ctx.make_descs([s.ctypes.data for s in scans], [s.shape[0] for s in scans], 16, ROLL, PITCH)
    v = ctx.process_raw(descs, len(scans), capi.FX_OUT_HOST | capi.FX_OUT_CLOUDS | capi.FX_OUT_DEBUG)
    got = ctx.unpack(v, True)
    off = capi._np(v.h_kp_offset, (v.batch + 1,), np.uint32).astype(np.int64)
    return got, int(v.total_keypoints), off


def _check_descriptors(d, o, rows, tag):
    """Rows [0, rows) of the scan against the oracle's rows of the same keypoints: NaN pattern equal, within DESC_TOL."""
    g, o = d["descriptors"], o["descriptors"][:rows]
    assert g.shape == o.shape == (rows, capi.FX_DESC_FLOATS), f"{tag}: rows {g.shape} vs {o.shape}"
    if not rows:
        return
    assert (np.isnan(g) == np.isnan(o)).all(), f"{tag}: NaN pattern of the held rows differs"
    diff = np.abs(np.where(np.isnan(g), 0, g) - np.where(np.isnan(o), 0, o))
    assert diff.max() <= util.DESC_TOL, f"{tag}: held rows max |diff| {diff.max()}"
    assert (g[:, capi.FX_DESC_BINS:] == 0).all(), f"{tag}: rf must be zero"


def check_cut(got, total, off, oras, M, tag):
    """Every clause of the pool-cut rule for one batch: offsets unclamped, detector outputs complete, flags exactly on the
    scans that lose rows, the leading rows held and the oracle's, nothing beyond the pool."""
    B = len(oras)
    Ks = [int(o["n_keypoints"]) for o in oras]
    want_off = np.concatenate([[0], np.cumsum(Ks)])
    util.assert_bit_equal(off, want_off, f"{tag}: kp_offset (exclusive prefix of n_keypoints, not clamped to the pool)")
    assert total == min(int(want_off[-1]), M), f"{tag}: total_keypoints {total} vs min({want_off[-1]}, {M})"
    n_rows = 0
    for b in range(B):
        d, o, t = got[b], oras[b], f"{tag} scan {b}"
        rows = _held(int(want_off[b]), Ks[b], M)
        assert d["flags"] == (TOTAL if rows < Ks[b] else 0), f"{t}: flags {d['flags']:#x}, holds {rows} of {Ks[b]} rows"
        # the detector half: keypoints, membership, ~cloud, ~keypoint_cloud do not live in the pool
        util.compare_scan(dict(d, flags=0), o, estimate_descriptors=False, tag=t)
        assert d["rows"] == rows, f"{t}: {d['rows']} rows reported, the pool holds {rows}"
        _check_descriptors(d, o, rows, t)
        util.assert_bit_equal(d["kp_neighbors"][:rows], o["kp_neighbors"][:rows], f"{t}: neighbour counts of the held rows")
        n_rows += rows
    assert n_rows == total <= M, f"{tag}: {n_rows} rows reported, total_keypoints {total}, pool {M}"


def cut_points(Ks):
    """(name, M) of the cuts of a batch with per-scan keypoint counts Ks (the first two scans are keypoint-heavy)."""
    S = np.concatenate([[0], np.cumsum(Ks)]).astype(int)
    return [("control: the pool ends at the batch's end", int(S[-1])),
            ("one row short of the batch's end", int(S[-1]) - 1),
            ("one row short of a scan boundary", int(S[2]) - 1),
            ("the middle of a scan", int(S[1]) + Ks[1] // 2),
            ("the first row of a scan", int(S[1]) + 1),
            ("at a scan boundary: every later scan gets nothing", int(S[1]))]


LAUNCH_SETS = {"default": ({}, {}), "separate": (dict(FX_FRONT=0), {}), "front-fused": (dict(FX_FRONT_STREAM=0), {}),
               "gather-counted": (dict(FX_GATHER_COUNTED=1), {}), "dense-tier": ({}, dict(max_neighbors=32)),
               "dense-slow": (dict(FX_DENSE_SLOW=1), dict(max_neighbors=32))}


@pytest.fixture
def launch(request, fxlib, monkeypatch):
    env, lim = LAUNCH_SETS[request.param]
    if not env:
        yield lim
        return
    with capi.test_hooks():
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        yield lim


@pytest.mark.parametrize("launch", list(LAUNCH_SETS), indirect=True)
def test_pool_cuts_hold_the_leading_rows_and_flag_the_scans_that_lose_rows(launch, oracle):
    p = capi.params("launch")
    scans = [_scene(k) for k in SCENES]
    oras = [_oracle(oracle, k) for k in SCENES]
    Ks = [int(o["n_keypoints"]) for o in oras]
    assert Ks[0] > 64 and Ks[1] > 64 and Ks[3] == 0 and Ks[-1] == 0, Ks
    for name, M in cut_points(Ks):
        ctx = capi.Context(p, capi.limits(len(scans), 28800, max_keypoints=512, max_total_keypoints=M, **launch))
        got, total, off = _run(ctx, scans)
        ctx.close()
        check_cut(got, total, off, oras, M, name)
        if "control" in name:
            assert all(d["flags"] == 0 for d in got)
        if "nothing" in name:  # (the empty scans past the cut lose nothing and are not flagged)
            assert [d["flags"] != 0 for d in got] == [False, True, True, False, True, True, False]


def test_a_cut_in_the_second_offsets_chunk_of_a_1024_scan_batch(fxlib, oracle):
    """The real case: 1024 scans under the default pool (64 a scan).  Keypoint-heavy scenes put the cut past scan 256, in the
    second FX_WG chunk of the offsets pass.  The scenes repeat, so every scan is checked against its scene's oracle run."""
    keys = [(200 + i, 256 if i % 2 else 512) for i in range(12)]
    oras = [_oracle(oracle, k) for k in keys]
    B = 1024
    scene_of = [(b * 7) % len(keys) for b in range(B)]
    base = [_scene(k) for k in keys]
    p = capi.params("launch")
    ctx = capi.Context(p, capi.limits(B, 28800, sparse=True))
    M = ctx.limits.max_total_keypoints
    assert M == 64 * B
    got, total, off = _run(ctx, [base[i] for i in scene_of])
    ctx.close()
    all_oras = [oras[i] for i in scene_of]
    cut_scan = int(np.searchsorted(np.cumsum([o["n_keypoints"] for o in all_oras]), M, side="right"))
    assert 256 <= cut_scan < 512, cut_scan
    check_cut(got, total, off, all_oras, M, "1024 scans, default pool")


def _cut_batch(oracle, M_from=lambda Ks: int(np.cumsum(Ks)[1]) + Ks[2] // 2):
    scans = [_scene(k) for k in SCENES]
    oras = [_oracle(oracle, k) for k in SCENES]
    Ks = [int(o["n_keypoints"]) for o in oras]
    return scans, oras, Ks, M_from(Ks)


def test_every_output_of_a_cut_batch(fxlib, oracle):
    """The held rows as every egress reports them: the dense host rows, the CSR block (host and device), the PointDescriptor
    records, the fixed-stride keypoint records and the compact keypoint block."""
    import torch
    scans, oras, Ks, M = _cut_batch(oracle)
    S = np.concatenate([[0], np.cumsum(Ks)]).astype(int)
    rows = [_held(int(S[b]), Ks[b], M) for b in range(len(Ks))]
    assert 0 < rows[2] < Ks[2] and sum(rows) == M
    p = capi.params("launch")
    ctx = capi.Context(p, capi.limits(len(scans), 28800, max_keypoints=512, max_total_keypoints=M))
    got, total, off = _run(ctx, scans)
    check_cut(got, total, off, oras, M, "egress: dense host rows")
    dense = np.concatenate([d["descriptors"] for d in got])
    dev = torch.device("cuda", 0)

    # the CSR block through FX_OUT_DESC_CSR: the same rows, bit for bit, per scan and as one block
    csr = ctx.process_host(scans, roll=ROLL, pitch=PITCH, descriptors="csr")
    rp, col, val = ctx.descriptors_csr_host()
    assert len(rp) == total + 1
    util.assert_bit_equal(capi.dense_from_csr(rp, col, val), dense, "CSR host block vs dense rows")
    for b, d in enumerate(csr):
        assert d["rows"] == rows[b] and d["flags"] == got[b]["flags"]
        util.assert_bit_equal(capi.dense_from_csr(*d["desc_csr"]), got[b]["descriptors"], f"CSR rows of scan {b}")
    # ... and packed on the device (fx_pack_descriptors_csr)
    t, hdr = ctx.descriptors_csr()
    assert hdr["rows"] == hdr["rows_stored"] == total
    util.assert_bit_equal(t.to_dense().cpu().numpy(), dense, "device CSR block vs dense rows")

    # fx_pack_features: total_keypoints records (keypoint + its row), nothing past the capacity
    # (every buffer below is filled on torch's stream and packed on the context's: the fill must be done before the pack starts)
    R = capi.FX_FEATURE_RECORD_BYTES
    for cap in (total, total - 3):
        buf = torch.full(((total + 2) * R,), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        capi.check(ctx.lib.fx_pack_features(ctx.handle, C.c_void_p(buf.data_ptr()), cap))
        ctx.synchronize()
        raw = buf.cpu().numpy()
        assert (raw[cap * R:] == 0xAB).all(), f"fx_pack_features wrote past capacity {cap}"
        rec = raw[:cap * R].view(np.float32).reshape(cap, R // 4)
        kp = np.concatenate([d["keypoints"][:rows[b]] for b, d in enumerate(got)])[:cap]
        util.assert_bit_equal(rec[:, [0, 1, 2, 4]], kp, f"feature records' keypoints (capacity {cap})")
        assert (rec[:, 3] == 1.0).all() and (rec[:, 5 + capi.FX_DESC_FLOATS:] == 0).all()
        util.assert_bit_equal(rec[:, 5:5 + capi.FX_DESC_FLOATS], dense[:cap], f"feature records' rows (capacity {cap})")

    # fx_pack_keypoint_records: keypoints complete up to the record's own cut, flags as include/fx.h says
    for rec_kp in (512, 100):
        buf = torch.zeros((len(scans) * (1 + rec_kp), 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.pack_keypoint_records(buf.data_ptr(), rec_kp)
        ctx.synchronize()
        r = buf.cpu().numpy().reshape(len(scans), 1 + rec_kp, 4)
        for b, d in enumerate(got):
            n, f = (int(x) for x in r[b, 0].view(np.uint32)[:2])
            K = Ks[b]
            assert n == min(K, rec_kp) and f == d["flags"] | (0x4 if K > rec_kp else 0), (rec_kp, b, n, hex(f))
            util.assert_bit_equal(r[b, 1:1 + n], oras[b]["keypoints"][:n], f"keypoint records of scan {b} ({rec_kp})")
            assert (r[b, 1 + n:] == 0).all()

    # fx_pack_keypoint_block: at the pool's size it cuts where the pool does; larger, it holds every keypoint
    for max_total in (M, int(S[-1]) + 10, M - 5):
        buf = torch.zeros((sharding.block_rows(len(scans), max_total), 4), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.pack_keypoint_block(buf.data_ptr(), len(scans), max_total)
        ctx.synchronize()
        hdr, per_scan = sharding.unpack_block(buf.cpu().numpy(), len(scans))
        held = [_held(int(S[b]), Ks[b], max_total) for b in range(len(Ks))]
        assert hdr["keypoints"] == sum(held) == min(int(S[-1]), max_total)
        for b, (n, f, kp) in enumerate(per_scan):
            assert n == held[b] and f == got[b]["flags"] | (0x4 if held[b] < Ks[b] else 0), (max_total, b, n, hex(f))
            util.assert_bit_equal(kp, oras[b]["keypoints"][:n], f"keypoint block scan {b} ({max_total})")
        if max_total == M:  # (the block's cut is the pool's: its scans lose exactly the rows the pool lost)
            assert [n for n, _, _ in per_scan] == rows
    ctx.close()


def test_rows_are_clean_across_cut_and_uncut_batches(fxlib, oracle):
    """Row reuse across a cut: a cut batch, an uncut batch of other scenes that ends inside the rows the cut batch filled, the
    cut batch again — every result bit-identical to a fresh context's and the oracle's."""
    scans, oras, Ks, M = _cut_batch(oracle)
    p = capi.params("launch")
    lim = capi.limits(len(scans), 28800, max_keypoints=512, max_total_keypoints=M)
    other_keys = [(300 + i, None) for i in range(3)] + [(303, 256)]
    other = [_scene(k) for k in other_keys]
    other_oras = [_oracle(oracle, k) for k in other_keys]
    assert sum(o["n_keypoints"] for o in other_oras) <= M

    def fresh(batch):
        c = capi.Context(p, lim)
        r = _run(c, batch)
        c.close()
        return r

    ctx = capi.Context(p, lim)
    for i, (batch, ora) in enumerate(((scans, oras), (other, other_oras), (scans, oras))):
        got, total, off = _run(ctx, batch)
        check_cut(got, total, off, ora, M, f"step {i}")
        ref, _, _ = fresh(batch)
        for b in range(len(batch)):
            for key in ("flags", "n_keypoints", "rows"):
                assert got[b][key] == ref[b][key], (i, b, key)
            for key in ("keypoints", "descriptors", "kp_neighbors", "kpc", "filtered"):
                util.assert_bit_equal(got[b][key], ref[b][key], f"step {i} scan {b} {key} vs a fresh context")
    ctx.close()


@pytest.mark.parametrize("front", ["default", "separate"])
def test_per_scan_keypoint_cut_keeps_the_leading_keypoints(fx_hooks, oracle, front):
    """max_keypoints: a scan keeps its first max_keypoints keypoints in the oracle's order, with the oracle's descriptors;
    candidates merged into a dropped keypoint map to -1; FX_FLAG_KP_OVERFLOW iff a keypoint was dropped."""
    fx_hooks(**({} if front == "default" else dict(FX_FRONT=0)))
    key = (100, 256)
    s, ora = _scene(key), _oracle(oracle, key)
    K = int(ora["n_keypoints"])
    assert K > 100
    p = capi.params("launch")
    for m in (8, 64, K - 1, K):
        ctx = capi.Context(p, capi.limits(2, 28800, max_keypoints=m, max_total_keypoints=1024))
        got, total, _ = _run(ctx, [s, s])
        ctx.close()
        n = min(K, m)
        assert total == 2 * n
        for b, d in enumerate(got):
            t = f"max_keypoints {m} scan {b}"
            assert d["flags"] == (0x4 if K > m else 0), f"{t}: flags {d['flags']:#x}"
            assert d["n_keypoints"] == n and d["rows"] == n
            trunc = dict(ora, n_keypoints=n, keypoints=ora["keypoints"][:n], kp_size=ora["kp_size"][:n],
                         kp_neighbors=ora["kp_neighbors"][:n], descriptors=ora["descriptors"][:n],
                         cand_keypoint=np.where(ora["cand_keypoint"] >= n, -1, ora["cand_keypoint"]).astype(np.int32))
            util.compare_scan(dict(d, flags=0), trunc, tag=t)


def test_keypoint_cloud_cut_empties_it_and_keeps_everything_else(fxlib, oracle):
    """max_kpc_points: a scan whose ~keypoint_cloud does not fit gets none of it and FX_FLAG_KPC_OVERFLOW; its keypoints and
    descriptors, and every other scan, stay the oracle's."""
    keys = [(100, 256), (102, None)]
    scans, oras = [_scene(k) for k in keys], [_oracle(oracle, k) for k in keys]
    n0, n1 = len(oras[0]["kpc"]), len(oras[1]["kpc"])
    assert n0 > n1
    p = capi.params("launch")
    for m in (n0, n0 - 1, n1):
        ctx = capi.Context(p, capi.limits(2, 28800, max_keypoints=512, max_total_keypoints=1024, max_kpc_points=m))
        got = ctx.process_host(scans, roll=ROLL, pitch=PITCH)
        ctx.close()
        for b, (d, o) in enumerate(zip(got, oras)):
            t = f"max_kpc_points {m} scan {b}"
            if len(o["kpc"]) > m:
                assert d["flags"] == KPC and len(d["kpc"]) == 0 and len(d["kpc_cand"]) == 0, (t, hex(d["flags"]))
                o = dict(o, kpc=o["kpc"][:0], kpc_cand=o["kpc_cand"][:0])
            util.compare_scan(dict(d, flags=0) if d["flags"] == KPC else d, o, tag=t)
