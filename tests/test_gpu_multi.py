"""C++ multi-GPU driver (csrc/fx_multi.hpp) on the devices that are there: RCCL communicators come up, every rank runs
its block of the batch, ncclAllGather assembles the keypoint table, and the table equals the producing ranks' results.
The GPU box has one device, so this is the nranks = 1 run SURVEY.md 8e asks the RCCL path to be testable with."""
import re
import subprocess

import pytest

from feature_extraction_amd import build

pytestmark = pytest.mark.gpu


def test_fx_multi_cli_runs_the_rccl_gather():
    exe = build.build_multi()
    r = subprocess.run([exe, "--batch", "64", "--steps", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "RCCL communicators up" in r.stdout and "gathered table == per-rank results" in r.stdout, r.stdout


@pytest.mark.parametrize("ranks,batch,inflight", [(8, 61, 3), (2, 64, 2), (3, 2, 1)])
def test_many_ranks_on_one_device_through_the_host_gather(ranks, batch, inflight):
    """fx::MultiGpu has never run on more than one device.  Its self-test mode puts G worker threads — tickets,
    the error barrier before the collective, slots in flight, uneven blocks (61 scans over 8 ranks; 2 scans over 3: a rank
    with none) — on the ONE device of this box, the collective replaced by a gather through host memory (RCCL refuses a
    communicator with the same device twice).  The gathered table must equal every producing rank's results, every rank
    must hold the same table, a batch that one rank cannot run must fail on all of them, and the next one be right."""
    exe = build.build_multi()
    r = subprocess.run([exe, "--selftest", str(ranks), "--batch", str(batch), "--steps", "6", "--inflight", str(inflight), "--bad-scan", str(batch - 1)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{ranks} rank(s)" in r.stdout and "SELF-TEST" in r.stdout and "gathered table == per-rank results" in r.stdout, r.stdout
    assert "failed on every rank as it must" in r.stdout and "the batch after the failed one equals the reference table" in r.stdout, r.stdout


def _block_check(out):
    m = re.search(r"block check: (\d+) of (\d+) keypoints held, (\d+) scans cut, (\d+) scans flagged", out)
    assert m, out
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("pool", ["raised", "default"])
def test_gathered_table_of_keypoint_heavy_scans(fxlib, oracle, pool):
    """Scans of 256 poles (some 150 keypoints each, beyond the default pool's 64 a scan) over 3 ranks, 7 scans (uneven).
    The block defaults to the rank contexts' pool: raised, the table holds every keypoint and no scan is flagged; default,
    each rank's block holds exactly its pool's leading rows, and the CLI checks every scan's count, flags (the rank's plus
    FX_FLAG_KP_OVERFLOW where the block cut it) and keypoints against the rank's results."""
    from feature_extraction_amd import capi, sharding
    from tests import util
    G, B, per_rank = 3, 7, 3
    p = capi.params("launch")
    Ks = [int(oracle.run(p, util.vlp16_scan(1000 + b, n_poles=256), roll=0.02, pitch=-0.015)["n_keypoints"]) for b in range(B)]
    M = per_rank * 256 if pool == "raised" else per_rank * 64
    exe = build.build_multi()
    args = ["--selftest", str(G), "--batch", str(B), "--steps", "2", "--inflight", "1", "--poles", "256"]
    if pool == "raised":
        args += ["--pool-keypoints", str(M)]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"compact keypoint blocks of {M} keypoints" in r.stdout, r.stdout
    assert "gathered table == per-rank results" in r.stdout, r.stdout
    held, total, cut, flagged = _block_check(r.stdout)
    assert total == sum(Ks)
    want_held = want_cut = 0
    for rank in range(G):
        lo, hi = sharding.shard_range(B, G, rank)
        off = 0
        for b in range(lo, hi):
            h = max(0, min(off + Ks[b], M) - min(off, M))
            want_held += h
            want_cut += h < Ks[b]
            off += Ks[b]
    assert (held, cut, flagged) == (want_held, want_cut, want_cut), r.stdout
    if pool == "raised":
        assert held == total and cut == 0 and flagged == 0
    else:
        assert cut > 0 and held < total
