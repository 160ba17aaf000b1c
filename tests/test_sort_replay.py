"""The kernels' cluster-order replay (csrc/fx_sort_replay.h, host build through the C-ABI test
hooks) against the oracle's literal std::sort(rbegin, rend, bySize) call."""
import ctypes as C

import numpy as np
import pytest

from feature_extraction_amd import capi


def _replay(lib, sizes, ranked):
    s = np.ascontiguousarray(sizes, dtype=np.uint32)
    out = np.zeros(len(s), np.uint32)
    fn = {False: lib.fx_test_sort_replay, True: lib.fx_test_sort_replay_ranked, "lists": lib.fx_test_sort_replay_lists}[ranked]
    fn(s.ctypes.data_as(capi._U32P), len(s), out.ctypes.data_as(capi._U32P))
    return out


@pytest.mark.parametrize("ranked", [False, True, "lists"])
def test_random_sequences(fxtestlib, oracle, ranked):
    rng = np.random.default_rng(11)
    for trial in range(1500):
        n = int(rng.integers(0, 300)) if trial % 12 else int(rng.integers(1000, 4000))
        hi = int(rng.choice([1, 2, 3, 5, 16, 50, 1000]))
        s = rng.integers(1, hi + 1, n)
        assert np.array_equal(_replay(fxtestlib, s, ranked), oracle.sort_by_size_desc(s)), (trial, n, hi)


@pytest.mark.parametrize("ranked", [False, True, "lists"])
def test_structured_sequences(fxtestlib, oracle, ranked):
    for n in (0, 1, 2, 16, 17, 33, 100, 1000, 5000):
        idx = np.arange(n)
        for s in (idx % 60000 + 1, idx[::-1] % 60000 + 1, np.ones(n), np.minimum(idx, idx[::-1]) + 1,
                  (idx * 7919) % 13 + 1):
            assert np.array_equal(_replay(fxtestlib, s, ranked), oracle.sort_by_size_desc(s)), n


@pytest.mark.parametrize("ranked", [False, True, "lists"])
def test_heap_sort_fallback_is_replayed(fxtestlib, oracle, ranked):
    # McIlroy's adversary built against the very std::sort call drives introsort to its depth limit
    for n in (64, 500, 5000, 30000):
        s = oracle.antiqsort(n)
        assert len(np.unique(s)) == n
        assert np.array_equal(_replay(fxtestlib, s, ranked), oracle.sort_by_size_desc(s)), n


@pytest.mark.gpu
def test_wavefront_replay_on_the_device(fxtestlib, oracle):
    """The partition phase as the ring / merge kernels run it (one wavefront, ballots) on random,
    tie-heavy, structured and adversarial sequences of up to 192 clusters."""
    rng = np.random.default_rng(5)
    for n in (17, 18, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 160, 191, 192):
        seqs = []
        for hi in (1, 2, 3, 5, 16, 50, 1000):
            seqs += [rng.integers(1, hi + 1, n) for _ in range(12)]
        idx = np.arange(n)
        seqs += [idx + 1, idx[::-1] + 1, np.ones(n), np.minimum(idx, idx[::-1]) + 1, (idx * 7919) % 13 + 1, oracle.antiqsort(n)]
        s = np.ascontiguousarray(np.stack(seqs), dtype=np.uint32)
        out = np.zeros_like(s)
        capi.check(fxtestlib.fx_test_sort_replay_device(0, s.ctypes.data_as(capi._U32P), len(s), n, out.ctypes.data_as(capi._U32P)))
        for q in range(len(s)):
            assert np.array_equal(out[q], oracle.sort_by_size_desc(s[q])), (n, q)


# ---------------------------------------------------------------- cc_order itself (fx_test_cc_order_device)
CC_N = (16, 17, 64, 65, 128, 129, 192, 193, 255, 256, 257, 300, 1000)  # both sides of every arm of cc_order's dispatch
CC_MIN, CC_MAX = 2, 2000  # the gated launches' size gates: accepted sizes are the family's + 1, junk is 0, 1, 2001 or 65535
_cc_cases = {}


def _cc_families(oracle, n, rng):
    seqs = []
    for hi in (1, 2, 3, 5, 16, 50, 1000):
        seqs += [rng.integers(1, hi + 1, n) for _ in range(4)]
    idx = np.arange(n)
    seqs += [idx + 1, idx[::-1] + 1, np.minimum(idx, idx[::-1]) + 1, (idx * 7919) % 13 + 1, np.ones(n), oracle.antiqsort(n)]
    # the adversary's sizes all differ — any correct sort gives its one order —; halved they tie in pairs, the depth budget is
    # still spent from n = 37 on, and the heap sort's order of the ties differs from further partitions' (tests/test_sort_scenes.py)
    seqs.append((oracle.antiqsort(n).astype(np.int64) + 1) // 2)
    return [np.asarray(s, np.uint32) for s in seqs]


def _cc_case(oracle, n, gated):
    """(sizes [3 q][len], ccap [3 q], accepted indices per sequence, expected ordinals per sequence): every family of n accepted
    entries — among n // 3 + 1 rejected ones at random places when gated —, each three times: ccap = n_c - 1, n_c, n_c + 1.
    Shared by the (NT, GS) cases: the oracle sorts every sequence once."""
    key = (n, gated)
    if key not in _cc_cases:
        rng = np.random.default_rng(1000 * n + gated)
        rows, acc, want = [], [], []
        for s in _cc_families(oracle, n, rng):
            if gated:
                total = n + n // 3 + 1
                at = np.sort(rng.choice(total, n, replace=False))
                row = rng.choice(np.array([0, 1, CC_MAX + 1, 65535], np.uint32), total)
                row[at] = s + 1  # (one larger throughout: the same order)
            else:
                at, row = np.arange(n), s
            rows.append(row)
            acc.append(at)
            want.append(oracle.sort_by_size_desc(s))
        sizes = np.ascontiguousarray(np.repeat(np.stack(rows), 3, axis=0), dtype=np.uint32)
        ccap = np.ascontiguousarray(np.tile(np.array([n - 1, n, n + 1], np.uint32), len(rows)))
        _cc_cases[key] = (sizes, ccap, acc, want)
    return _cc_cases[key]


@pytest.mark.gpu
@pytest.mark.parametrize("gs", [0, 1], ids=["lds", "gs"])
@pytest.mark.parametrize("nt", [64, 256, 1024])
def test_cc_order_on_the_device(fxtestlib, oracle, nt, gs):
    """cc_order — the routine the ring and merge bodies call, not a restatement — against the oracle's std::sort: every arm of
    its dispatch (no sort up to 16, sort_partition_wave<1 .. 4> up to 256, one lane beyond), with its arrays in LDS and (gs) in
    HBM scratch as k_slow places them, by a single wavefront (k_rings_runs), 256 threads (k_slow, k_merge_small) and 1024
    (k_rings_large, k_merge_big).  Gated launches reject a quarter of the entries by size: the ordinals are ranks among the
    accepted in index order, croot their indices.  One entry short of room (ccap = n_c - 1) the count is still reported and
    nothing is ordered; the guard words behind the three arrays are never written."""
    U = capi._U32P
    for n in CC_N:
        for gated in (False, True):
            sizes, ccap, acc, want = _cc_case(oracle, n, gated)
            n_seq, width = sizes.shape
            perm, root = np.zeros_like(sizes), np.zeros_like(sizes)
            n_c, bad = np.zeros(n_seq, np.uint32), np.ones(n_seq, np.uint32)
            lo, hi = (CC_MIN, CC_MAX) if gated else (1, 65535)
            capi.check(fxtestlib.fx_test_cc_order_device(0, sizes.ctypes.data_as(U), n_seq, width, lo, hi, ccap.ctypes.data_as(U), nt, gs,
                                                         perm.ctypes.data_as(U), root.ctypes.data_as(U), n_c.ctypes.data_as(U), bad.ctypes.data_as(U)))
            assert (n_c == n).all(), (n, gated, n_c.tolist())
            assert not bad.any(), (n, gated, "guard words written", np.flatnonzero(bad).tolist())
            for q in range(n_seq):
                tag = (n, gated, q // 3, int(ccap[q]))
                if ccap[q] < n:  # does not fit: counted, not ordered
                    assert (perm[q] == 0xffffffff).all() and (root[q] == 0xffffffff).all(), tag
                    continue
                assert np.array_equal(perm[q, :n], want[q // 3]), tag
                assert np.array_equal(root[q, :n], acc[q // 3]), tag
                assert (perm[q, n:] == 0xffffffff).all() and (root[q, n:] == 0xffffffff).all(), tag
