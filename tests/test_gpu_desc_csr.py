"""Descriptor rows as compressed rows (CSR) on the GPU: fx_pack_descriptors_csr's block, the FX_OUT_HOST | FX_OUT_DESC_CSR host
path, Context.descriptors_csr()'s torch.sparse_csr_tensor and fx_batcher_cli --csr all expand into the dense rows bit for bit
(every one of the 1989 words, -0.0 and NaN included), on every path a batch can take."""
import glob
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

from feature_extraction_amd import build, capi
from tests import desc_rows_util as rows
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096  # bytes behind a block that the pack must leave alone

HDL64 = dict(n_rings=64, n_az=2048, el0_deg=-24.8, el_step_deg=26.8 / 63, n_poles=256)
DENSE = dict(n_rings=128, n_az=2048, el0_deg=-25.0, el_step_deg=40.0 / 127, n_poles=256)


def _config(name, B):
    """(params, limits, scans) of a multi-scan batch: the VLP-16 launch scene, config 3 (64 x 2048), config 5 (128 x 2048)."""
    if name == "vlp16":
        return capi.params("launch"), capi.limits(B, 28800), [util.vlp16_scan(1000 + b) for b in range(B)]
    if name == "config3":
        p = capi.params("launch", n_rings=64, el0_deg=-24.8, el_step_deg=26.8 / 63, secondary_max=64)
        lim = capi.limits(B, 64 * 2048, max_candidates=4096, max_kpc_points=32768, max_keypoints=512, max_total_keypoints=B * 256)
        return p, lim, [capi.synth_scan(capi.synth_cfg(10 + b, **HDL64)) for b in range(B)]
    p = capi.params("launch", n_rings=128, el0_deg=-25.0, el_step_deg=40.0 / 127, secondary_max=128, descriptor_radius=2.0)
    lim = capi.limits(B, 128 * 2048, max_candidates=8192, max_kpc_points=65536, max_keypoints=512, max_total_keypoints=B * 256)
    return p, lim, [capi.synth_scan(capi.synth_cfg(50 + b, **DENSE)) for b in range(B)]


def _dense(ctx, scans, roll=0.02, pitch=-0.015, flags=0, descs=None):
    """One batch with FX_OUT_HOST: (view, the batch's dense descriptor rows as a host copy)."""
    if descs is None:
        scans = [np.ascontiguousarray(s, dtype=np.float32) for s in scans]
        descs = ctx.make_descs([s.ctypes.data for s in scans], [len(s) for s in scans], 16, roll, pitch)
    v = ctx.process_raw(descs, len(scans), capi.FX_OUT_HOST | flags)
    rows = capi._np(v.h_descriptors, (v.total_keypoints, capi.FX_DESC_FLOATS), np.float32) if v.h_descriptors else None
    return v, rows


def _pack(ctx, max_rows=None, capacity=None):
    """fx_pack_descriptors_csr into a zeroed device buffer with a guard region behind it: (parsed block, raw bytes, guard intact)."""
    import torch
    max_rows = ctx.limits.max_total_keypoints if max_rows is None else max_rows
    capacity = max_rows * capi.FX_DESC_FLOATS if capacity is None else capacity
    n = int(ctx.lib.fx_descriptor_csr_bytes(max_rows, capacity))
    buf = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=f"cuda:{ctx.device}")
    buf[:n].zero_()
    torch.cuda.synchronize()
    ctx.pack_descriptors_csr(buf.data_ptr(), max_rows, capacity)
    ctx.synchronize()
    raw = buf.cpu().numpy()
    return capi.csr_parse(raw[:n], max_rows, capacity), raw[:n].copy(), bool((raw[n:] == 0xA5).all())


def _check_structure(rp, col, val):
    rp64 = rp.astype(np.int64)
    assert rp64[0] == 0 and (np.diff(rp64) >= 0).all()
    assert len(col) == len(val) == rp64[-1]
    for r in range(len(rp) - 1):
        c = col[rp64[r]:rp64[r + 1]].astype(np.int64)
        assert (np.diff(c) > 0).all() and (c < capi.FX_DESC_FLOATS).all(), f"row {r}"
    assert (util.bits(val) != 0).all(), "a stored word with zero bits"


def _equal_bits(rows_csr, rows_dense, what):
    assert rows_csr.shape == rows_dense.shape, what
    bad = util.bits(rows_csr) != util.bits(rows_dense)
    assert not bad.any(), f"{what}: {int(bad.sum())} words differ, first at {np.argwhere(bad)[:3].tolist()}"


def _check_block(blk, dense, what):
    """A block with room for every row: structure, header, and every word against the dense rows."""
    rows = len(dense)
    nnz = int((util.bits(dense) != 0).sum())
    assert (blk["rows"], blk["rows_stored"], blk["nnz_stored"], blk["nnz_needed"]) == (rows, rows, nnz, nnz), what
    _check_structure(blk["row_ptr"], blk["col"], blk["val"])
    assert (blk["row_ptr_all"][rows:] == nnz).all()
    _equal_bits(capi.dense_from_csr(blk["row_ptr"], blk["col"], blk["val"]), dense, what)
    ref = capi.csr_from_dense(dense)
    assert all((a == b).all() for a, b in zip((blk["row_ptr"], blk["col"], util.bits(blk["val"])), (ref[0], ref[1], util.bits(ref[2]))))


def _check_host_csr(ctx, got, dense, off, what):
    """process_host(descriptors="csr")'s per-scan records against the dense rows of the same batch."""
    rp, col, val = ctx.descriptors_csr_host()
    _check_structure(rp, col, val)
    _equal_bits(capi.dense_from_csr(rp, col, val), dense, what)
    for b, d in enumerate(got):
        r, c, v = d["desc_csr"]
        K = d["n_keypoints"]
        _equal_bits(capi.dense_from_csr(r, c, v), dense[off[b]:off[b] + K], f"{what} scan {b}")


def test_golden_fixtures_dense_equivalence_and_oracle(fxlib, oracle):
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    assert len(files) >= 5
    for f in files:
        name = os.path.basename(f)
        p, lim, pts, roll, pitch = util.golden_case(np.load(f), name)
        ctx = capi.Context(p, lim)
        v, dense = _dense(ctx, [pts], roll, pitch)
        assert len(dense) > 0, name
        blk, _, guard = _pack(ctx)
        assert guard
        _check_block(blk, dense, name)
        got = ctx.process_host([pts], roll=roll, pitch=pitch, descriptors="csr")
        _check_host_csr(ctx, got, dense, [0], name)
        d = dict(got[0])
        d["descriptors"] = capi.dense_from_csr(*d["desc_csr"])
        util.compare_scan(d, oracle.run(p, pts, roll=roll, pitch=pitch), tag=f"{name} through CSR")
        ctx.close()


@pytest.mark.parametrize("name,B", [("vlp16", 16), ("config3", 8), ("config5", 4)])
def test_multi_scan_batches(fxlib, oracle, name, B):
    p, lim, scans = _config(name, B)
    ctx = capi.Context(p, lim)
    v, dense = _dense(ctx, scans)
    off = capi._np(v.h_kp_offset, (B + 1,), np.uint32)
    blk, _, guard = _pack(ctx)
    assert guard
    _check_block(blk, dense, name)
    got = ctx.process_host(scans, roll=0.02, pitch=-0.015, descriptors="csr")
    _check_host_csr(ctx, got, dense, off, name)
    for b in (0, B - 1):
        d = dict(got[b])
        d["descriptors"] = capi.dense_from_csr(*d["desc_csr"])
        util.compare_scan(d, oracle.run(p, scans[b], roll=0.02, pitch=-0.015), tag=f"{name} scan {b} through CSR")
    nnz = np.diff(blk["row_ptr"].astype(np.int64))
    print(f"{name}: {len(dense)} rows, {nnz.mean():.1f} non-zero words a row (max {nnz.max()}), "
          f"{blk['nnz_stored'] * 8 + 4 * (len(dense) + 1)} B of CSR against {dense.nbytes} B dense")
    ctx.close()


def test_nan_rows_of_an_exhausted_dense_pool(fxlib):
    s = util.vlp16_scan(1000, n_poles=8, x_lo=3.0, x_hi=8.0, y_lo=-4.0, y_hi=4.0)
    p = capi.params("default", descriptor_radius=4.0)
    ctx = capi.Context(p, capi.limits(1, 28800, max_dense_points=4096))
    v, dense = _dense(ctx, [s], 0.0, 0.0)
    assert capi._np(v.h_flags, (1,), np.uint32)[0] & capi.FX_FLAG_NBR_OVERFLOW
    nan_rows = np.isnan(dense[:, :capi.FX_DESC_BINS]).all(axis=1)
    assert nan_rows.any()
    blk, _, guard = _pack(ctx)
    assert guard
    _check_block(blk, dense, "NaN rows")
    # (which rows an exhausted pool fails depends on the order the rows drew their slots in: another batch of the same scan
    #  may fail others — so the host path's rows are held against the block packed from the SAME batch)
    got = ctx.process_host([s], descriptors="csr")
    rp, col, val = ctx.descriptors_csr_host()
    same, _, guard = _pack(ctx)
    assert guard and (rp == same["row_ptr"]).all() and (col == same["col"]).all() and (util.bits(val) == util.bits(same["val"])).all()
    _check_structure(rp, col, val)
    back = capi.dense_from_csr(*got[0]["desc_csr"])
    assert back.shape == dense.shape
    assert np.isnan(back[:, :capi.FX_DESC_BINS]).all(axis=1).sum() > 0 and got[0]["flags"] & capi.FX_FLAG_NBR_OVERFLOW
    ctx.close()


def test_capacity_cut_stores_whole_leading_rows_and_nothing_past_it(fxlib):
    p, lim, scans = _config("vlp16", 4)
    ctx = capi.Context(p, lim)
    v, dense = _dense(ctx, scans)
    ref_rp, ref_col, ref_val = capi.csr_from_dense(dense)
    nnz, rows = int(ref_rp[-1]), len(dense)
    for cap in (0, 1, int(ref_rp[1]), int(ref_rp[1]) + 1, nnz // 2, nnz - 1):
        blk, raw, guard = _pack(ctx, capacity=cap)
        assert guard, cap
        want = int(np.searchsorted(ref_rp, cap, side="right")) - 1  # leading rows whose end is within cap
        assert (blk["rows"], blk["rows_stored"], blk["nnz_needed"]) == (rows, want, nnz), cap
        assert blk["nnz_stored"] == ref_rp[want] <= cap
        assert (blk["row_ptr_all"][:want + 1] == ref_rp[:want + 1]).all() and (blk["row_ptr_all"][want:] == ref_rp[want]).all()
        assert (blk["col"] == ref_col[:ref_rp[want]]).all() and (util.bits(blk["val"]) == util.bits(ref_val[:ref_rp[want]])).all()
        _, col_o, val_o, end = capi.csr_layout(lim.max_total_keypoints, cap)
        assert not raw[col_o + 4 * blk["nnz_stored"]:val_o].any() and not raw[val_o + 4 * blk["nnz_stored"]:end].any()
    # fewer rows than the batch has: the first max_rows, the rest reported as cut
    blk, _, guard = _pack(ctx, max_rows=rows // 2)
    assert guard and (blk["rows"], blk["rows_stored"], blk["nnz_needed"]) == (rows, rows // 2, nnz)
    _equal_bits(capi.dense_from_csr(blk["row_ptr"], blk["col"], blk["val"]), dense[:rows // 2], "max_rows cut")
    ctx.close()


def test_host_path_grows_its_block(fxlib):
    p, lim, scans = _config("vlp16", 8)
    ctx = capi.Context(p, lim)
    v, dense = _dense(ctx, scans)
    off = capi._np(v.h_kp_offset, (9,), np.uint32)
    ctx.set_descriptor_csr_capacity(1)
    for _ in range(2):  # (the second call finds the grown block)
        got = ctx.process_host(scans, roll=0.02, pitch=-0.015, descriptors="csr")
        _check_host_csr(ctx, got, dense, off, "grown")
    ctx.set_descriptor_csr_capacity(0)
    got = ctx.process_host(scans, roll=0.02, pitch=-0.015, descriptors="csr")
    _check_host_csr(ctx, got, dense, off, "default capacity")
    # the dense host path is still there, and a CSR view only after a CSR batch
    v2, dense2 = _dense(ctx, scans)
    _equal_bits(dense2, dense, "dense after CSR")
    with pytest.raises(capi.FxError):
        ctx.descriptors_csr_host()
    ctx.close()


def test_edges_empty_batch_empty_scans_and_no_descriptors(fxlib):
    p = capi.params("launch")
    ctx = capi.Context(p, capi.limits(4, 28800))
    v = ctx.process_raw(None, 0, capi.FX_OUT_HOST | capi.FX_OUT_DESC_CSR)
    assert v.total_keypoints == 0 and not v.h_descriptors
    rp, col, val = ctx.descriptors_csr_host()
    assert list(rp) == [0] and len(col) == len(val) == 0
    blk, _, guard = _pack(ctx, max_rows=8, capacity=16)
    assert guard and (blk["rows"], blk["nnz_stored"], blk["nnz_needed"], blk["rows_stored"]) == (0, 0, 0, 0)
    assert not blk["row_ptr_all"].any()
    # scans with K = 0 (empty, everything filtered out) between real ones
    far = np.full((500, 4), 1000.0, np.float32)
    scans = [np.zeros((0, 4), np.float32), util.vlp16_scan(1000), far, util.vlp16_scan(1001)]
    v, dense = _dense(ctx, scans)
    off = capi._np(v.h_kp_offset, (5,), np.uint32)
    got = ctx.process_host(scans, roll=0.02, pitch=-0.015, descriptors="csr")
    assert got[0]["n_keypoints"] == 0 == got[2]["n_keypoints"]
    assert len(got[0]["desc_csr"][0]) == 1 and len(got[2]["desc_csr"][1]) == 0
    _check_host_csr(ctx, got, dense, off, "K = 0 scans")
    _check_block(_pack(ctx)[0], dense, "K = 0 scans")
    ctx.close()
    ctx = capi.Context(capi.params("launch", estimate_descriptors=0), capi.limits(2, 28800))
    got = ctx.process_host([util.vlp16_scan(1000)], roll=0.02, pitch=-0.015, descriptors="csr")
    assert got[0]["n_keypoints"] > 0 and len(got[0]["desc_csr"][1]) == 0
    assert list(ctx.descriptors_csr_host()[0]) == [0]
    blk, _, guard = _pack(ctx, max_rows=64, capacity=64)
    assert guard and (blk["rows"], blk["nnz_needed"]) == (0, 0)
    ctx.close()


def test_paths_give_the_identical_block(fxlib):
    """Graph replay, device-resident input, several contexts in flight and a second run: the same bytes."""
    import torch
    p, lim, scans = _config("vlp16", 8)
    ctx = capi.Context(p, lim)
    v, dense = _dense(ctx, scans)
    blk, ref, _ = _pack(ctx)
    _check_block(blk, dense, "plain")
    _dense(ctx, scans)
    assert (_pack(ctx)[1] == ref).all(), "second run"
    dev = [torch.from_numpy(s).cuda() for s in scans]
    torch.cuda.synchronize()
    descs = ctx.make_descs([d.data_ptr() for d in dev], [len(s) for s in scans], 16, 0.02, -0.015)
    _dense(ctx, scans, flags=capi.FX_IN_DEVICE, descs=descs)
    assert (_pack(ctx)[1] == ref).all(), "FX_IN_DEVICE"
    ctx.set_graph_batch(8)
    for _ in range(3):  # capture, then replays
        ctx.process_raw(descs, len(scans), capi.FX_IN_DEVICE)
    assert (_pack(ctx)[1] == ref).all(), "graph replay"
    host = ctx.process_host(scans, roll=0.02, pitch=-0.015, descriptors="csr")
    ref_host = [tuple(util.bits(x) if x.dtype == np.float32 else x for x in d["desc_csr"]) for d in host]
    ctx.close()
    # four contexts, a thread each, batches in flight together
    n_ctx, res, errs = 4, {}, []

    def run(i):
        try:
            c = capi.Context(p, lim)
            c.set_batches_in_flight(n_ctx)
            for _ in range(3):
                c.process_host(scans, roll=0.02, pitch=-0.015, debug=False, descriptors="csr")
            got = c.process_host(scans, roll=0.02, pitch=-0.015, debug=False, descriptors="csr")
            res[i] = ([tuple(util.bits(x) if x.dtype == np.float32 else x for x in d["desc_csr"]) for d in got], _pack(c)[1])
            c.close()
        except Exception as e:  # (reported below)
            errs.append(e)
    th = [threading.Thread(target=run, args=(i,)) for i in range(n_ctx)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    for i in range(n_ctx):
        h, raw = res[i]
        assert (raw == ref).all(), f"context {i}"
        assert all(all((a == b).all() for a, b in zip(x, y)) for x, y in zip(h, ref_host)), f"context {i} host"


def test_full_rows_hook_gives_the_same_block(fx_hooks):
    p, lim, scans = _config("vlp16", 8)
    blocks = []
    for full in (0, 1):
        fx_hooks(FX_CSR_FULL_ROWS=full)
        ctx = capi.Context(p, lim)
        v, dense = _dense(ctx, scans)
        blk, raw, guard = _pack(ctx)
        assert guard
        _check_block(blk, dense, f"FX_CSR_FULL_ROWS={full}")
        blocks.append(raw)
        ctx.close()
    assert (blocks[0] == blocks[1]).all()
    # and the NaN / dense-tier rows (the whole-row path in the product too) next to a group row, on hand-built scenes
    # (tests/desc_rows_util.py) whose outcome does not depend on the order the rows draw their pool entries in: dense rows that
    # all fit the pool, one of them NaN for want of a neighbour; then, with the smallest pool (4096 entries), dense rows that EACH
    # exceed it — every one of them fails whichever comes first
    for name, lim, exhausted in (("csr_fit", {}, False), ("csr_exhaust", dict(max_dense_points=4096), True)):
        p, scenes, cases = rows.built(name)
        (s, ora), = scenes
        n_dense = sum(sup > rows.LIST_CAP for _, sup, _ in cases)
        assert n_dense >= 2 and any(n == 0 and sup > rows.LIST_CAP for n, sup, _ in cases)
        blocks = []
        for full in (0, 1):
            fx_hooks(FX_CSR_FULL_ROWS=full)
            ctx = capi.Context(p, capi.limits(1, 1 << len(s).bit_length(), **lim))
            v, dense = _dense(ctx, [s], 0.0, 0.0)
            flags = int(capi._np(v.h_flags, (1,), np.uint32)[0])
            nan_rows = np.isnan(dense[:, :capi.FX_DESC_BINS]).all(axis=1)
            if exhausted:
                assert all(sup > 4096 for _, sup, _ in cases if sup > rows.LIST_CAP)
                assert flags == capi.FX_FLAG_NBR_OVERFLOW and int(nan_rows.sum()) == n_dense
            else:
                assert flags == 0 and int(nan_rows.sum()) == 1
                util.assert_bit_equal(dense, ora["descriptors"], f"{name} against the oracle")
            blocks.append(_pack(ctx)[1])
            R = ctx.limits.max_total_keypoints
            _check_block(capi.csr_parse(blocks[-1], R, R * capi.FX_DESC_FLOATS), dense, f"{name}, FX_CSR_FULL_ROWS={full}")
            ctx.close()
        assert (blocks[0] == blocks[1]).all(), name


def test_python_sparse_csr_tensor_matches_the_dense_rows_on_the_gpu(fxlib):
    import torch
    p, lim, scans = _config("vlp16", 8)
    ctx = capi.Context(p, lim)
    v, dense = _dense(ctx, scans)
    d_rows = torch.from_numpy(dense).cuda()
    t, hdr = ctx.descriptors_csr()
    assert t.layout == torch.sparse_csr and t.shape == (len(dense), capi.FX_DESC_FLOATS)
    assert t.crow_indices().dtype == torch.int32 and t.values().device.type == "cuda"
    assert hdr["rows"] == hdr["rows_stored"] == len(dense) and hdr["nnz_stored"] == hdr["nnz_needed"] == t.values().numel()
    assert torch.equal(t.to_dense().view(torch.int32), d_rows.view(torch.int32))
    # a caller's buffer, too small: the leading rows only, and the header says so
    n = int(fxlib.fx_descriptor_csr_bytes(lim.max_total_keypoints, 64))
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    t2, hdr2 = ctx.descriptors_csr(buf=buf, capacity=64)
    assert hdr2["rows_stored"] < hdr2["rows"] == len(dense) and hdr2["nnz_needed"] == hdr["nnz_needed"]
    k = hdr2["rows_stored"]
    assert torch.equal(t2.to_dense()[:k].view(torch.int32), d_rows[:k].view(torch.int32)) and not t2.to_dense()[k:].any()
    ctx.close()


def _read_csr_records(path):
    raw = open(path, "rb").read()
    pos, out = 0, {}
    while pos < len(raw):
        sensor, seq, flags, K = struct.unpack_from("<4I", raw, pos)
        pos += 16
        kp = np.frombuffer(raw, np.float32, K * 4, pos).reshape(K, 4)
        pos += K * 16
        rows, nnz = struct.unpack_from("<2I", raw, pos)
        pos += 8
        rp = np.frombuffer(raw, np.uint32, rows + 1, pos)
        pos += 4 * (rows + 1)
        col = np.frombuffer(raw, np.uint32, nnz, pos)
        pos += 4 * nnz
        val = np.frombuffer(raw, np.float32, nnz, pos)
        pos += 4 * nnz
        out[(sensor, seq)] = (flags, kp, rp, col, val)
    return out


def test_batcher_cli_csr_records_match_the_oracle(fxlib, oracle, tmp_path):
    exe = build.build_batcher()
    out = tmp_path / "csr.bin"
    r = subprocess.run([exe, "--sensors", "2", "--burst", "6", "--max-batch", "4", "--csr", "--out", str(out)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout.strip())
    got = _read_csr_records(out)
    assert len(got) == 12
    p = capi.params("launch")
    total_k = 0
    for (s, q), (flags, kp, rp, col, val) in sorted(got.items()):
        ora = oracle.run(p, util.vlp16_scan(1000 + 1000 * s + q), roll=0.02, pitch=-0.015)
        assert flags == 0
        util.assert_bit_equal(kp, ora["keypoints"], f"sensor {s} scan {q} keypoints")
        assert len(rp) == len(kp) + 1
        _check_structure(rp, col, val)
        desc, o = capi.dense_from_csr(rp, col, val), ora["descriptors"]
        assert desc.shape == o.shape and (np.isnan(desc) == np.isnan(o)).all()
        assert np.abs(np.where(np.isnan(o), 0, desc) - np.where(np.isnan(o), 0, o)).max(initial=0.0) <= util.DESC_TOL
        total_k += len(kp)
    assert total_k > 0
