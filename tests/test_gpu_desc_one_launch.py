"""Every descriptor tier of a batch runs in ONE launch (csrc/fx_kernels.hip: k_desc).  That rests on two things, pinned here bit
for bit against the oracle:

  * the support gather classifies every row where its support count becomes final (classify_rows: the tail of the gather
    when one workgroup has the scan to itself, k_rng_ord otherwise), so every tier's work list is complete before the launch;
  * a row is cleared exactly once a batch, by the workgroup or wavefront that then computes it, before its first store to it.

The scans are hand-built in the manner of tests/desc_rows_util.py — every row's neighbour count and support count is set exactly,
by points the detector never sees —, with EIGHT poles a scan: two on each horizontal axis, 1.2 m apart."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import desc_rows_util as rows
from tests import util

pytestmark = pytest.mark.gpu

N_POINTS = 16 * 1800
SLOTS = [(axis, side) for axis in rows.AXES for side in (-0.6, 0.6)]
# support sets of exactly 0, 1, FX_GROUP_CAP, + 1, FX_WAVE_CAP, + 1, dense_min, + 1 points: (neighbours, support points)
EDGE_CASES = [(0, 0), (1, 1), (30, 64), (30, 65), (100, 192), (100, 193), (500, 1024), (500, 1025)]
CLASSES = ("group", "wave", "list", "dense", "nan")
CLASS_CASE = {"group": (20, 40), "wave": (100, 150), "list": (300, 600), "dense": (1100, 1500), "nan": (0, 30)}
# (a directory of its own: tests/golden/*.npz are whole scans with their oracle results, which many tests iterate over)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "desc_one_launch", "pool_exhaustion.npz")


def scene8(oracle, p, cases, rng, n_points=N_POINTS):
    """One scan of len(cases) <= 8 poles, padded to n_points with points far outside everything, and what each row must
    count: (scan, [(keypoint xyz, nbr, sup)]).  desc_rows_util.scene with two poles an axis ("mixed" layout only)."""
    poles, clouds, want = [], [], []
    for (axis, side), (nbr, sup) in zip(SLOTS, cases):
        a = np.array(axis)
        pl = rows.pole(p, axis, side=side)
        s = np.zeros((len(pl), 4), np.float32)
        s[:, :3] = pl
        kps = oracle.run(p, s)["keypoints"]
        assert len(kps) == 1
        kp = kps[0, :3].astype(np.float64)
        poles.append(pl)

        def around(n, r_lo, r_hi):  # n points r_lo..r_hi from the keypoint, at least half of that beyond it along the axis
            c, th = rng.uniform(0.5, 1.0, n), rng.uniform(0.0, 2 * np.pi, n)
            s = np.sqrt(1.0 - c * c)
            d = np.stack([c * a[0] - s * np.cos(th) * a[1], c * a[1] + s * np.cos(th) * a[0], s * np.sin(th)], axis=1)
            return (kp + d * rng.uniform(r_lo, r_hi, (n, 1))).astype(np.float32)

        both = np.concatenate([around(nbr, 0.2 * rows.R, 0.9 * rows.R), around(sup - nbr, 1.05 * rows.R, 1.15 * rows.R)])
        clouds.append(both[rng.permutation(len(both))])
        want.append((kp, nbr, sup))
    xyz = np.concatenate(clouds + poles)
    pad = n_points - len(xyz)
    assert pad >= 0
    far = np.stack([30.0 + 0.01 * np.arange(pad), np.full(pad, 30.0), np.zeros(pad)], axis=1).astype(np.float32)
    xyz = np.concatenate([xyz[:len(xyz) // 2], far, xyz[len(xyz) // 2:]])  # (the padding in the middle of the scan)
    scan = np.zeros((len(xyz), 4), np.float32)
    scan[:, :3] = xyz
    return scan, want


def _oracle():
    from oracle import oracle_py
    oracle_py.load()
    return oracle_py


@functools.lru_cache(maxsize=None)
def edge_scene():
    """(params, scan, oracle result) of the tier-edge scan, built once a process; nobody writes into it."""
    ora_lib, p = _oracle(), rows.params()
    scan, want = scene8(ora_lib, p, EDGE_CASES, np.random.default_rng(46))
    assert scan.shape == (N_POINTS, 4)
    ora = ora_lib.run(p, scan)
    rows.check_counts(ora, scan, want, "tier edges")
    assert sorted(rows.support_counts(scan, ora)[1]) == sorted(s for _, s in EDGE_CASES)  # the device's wider radius holds the same sets
    return p, scan, ora


def class_of(nbr, sup, list_cap=rows.LIST_CAP):
    return "nan" if nbr == 0 else rows.tier_of(sup, list_cap)


@functools.lru_cache(maxsize=None)
def class_batches():
    """(params, A, B): two batches of four 8-pole scans, [(scan, oracle result)], in which the pole of scan i at slot j is of
    class a in A and of class b in B, (a, b) running over every ordered pair of CLASSES (25 of the 32 poles, the rest repeat)."""
    ora_lib, p = _oracle(), rows.params()
    pairs = [(a, b) for a in CLASSES for b in CLASSES]
    pairs += pairs[6:13]
    assert len(pairs) == 32
    out = []
    for which in (0, 1):
        rng = np.random.default_rng(460 + which)
        batch = []
        for i in range(4):
            cases = [CLASS_CASE[pr[which]] for pr in pairs[8 * i:8 * i + 8]]
            scan, want = scene8(ora_lib, p, cases, rng, n_points=8192)
            ora = ora_lib.run(p, scan)
            rows.check_counts(ora, scan, want, f"batch {'AB'[which]} scan {i}")
            batch.append((scan, ora))
        out.append(batch)
    return p, out[0], out[1]


def _counters(ctx):
    """The last batch's work-list counters: rows handed to the list, wave and dense tiers (fx_debug_counters)."""
    cnt = (C.c_uint32 * 16)()
    ctx.lib.fx_debug_counters.argtypes = [C.c_void_p, C.c_void_p]
    capi.check(ctx.lib.fx_debug_counters(ctx.handle, cnt))
    return {"list": int(cnt[4]), "wave": int(cnt[8]), "dense": int(cnt[6])}


def _check(ctx, p, scenes, tag, list_cap=rows.LIST_CAP):
    got = ctx.process_host([s for s, _ in scenes])
    for b, (scan, ora) in enumerate(scenes):
        rows.compare(got[b], ora, f"{tag}, scan {b}", scan=scan, radius=float(p.descriptor_radius), list_cap=list_cap)
    return got


def _expected(scenes, list_cap):
    tiers = [rows.tier_of(n, list_cap) for scan, ora in scenes for n in rows.support_counts(scan, ora)[1]]
    return {t: tiers.count(t) for t in ("group", "wave", "list", "dense")}


def _check_tiers(ctx, scenes, list_cap, tag):
    """Every tier received the rows meant for it — and at least one: a scene that puts no row in a tier has not tested it."""
    want = _expected(scenes, list_cap)
    assert all(want[t] > 0 for t in want), f"{tag}: the scene leaves a tier without rows: {want}"
    got = _counters(ctx)
    got["group"] = sum(want.values()) - sum(got.values())
    assert got == want, f"{tag}: rows per tier {got}, wanted {want}"


@pytest.mark.parametrize("list_cap", [rows.LIST_CAP, 256])
def test_tier_edges(fxlib, list_cap):
    """0, 1, 64 | 65, 192 | 193, 1024 | 1025 support points: the last row of a tier and the first of the next, each in its
    tier's list and each the oracle's row.  With max_neighbors = 256 the rows of 1024 and 1025 points overflow their lists
    (the entries beyond 256 sit in the scan's overflow region) and are dense rows for that."""
    p, scan, ora = edge_scene()
    ctx = capi.Context(p, capi.limits(1, N_POINTS, max_neighbors=list_cap))
    _check(ctx, p, [(scan, ora)], f"tier edges, max_neighbors={list_cap}", list_cap)
    _check_tiers(ctx, [(scan, ora)], list_cap, f"max_neighbors={list_cap}")
    assert _expected([(scan, ora)], list_cap) == ({"group": 3, "wave": 2, "list": 2, "dense": 1} if list_cap == rows.LIST_CAP else
                                                  {"group": 3, "wave": 2, "list": 1, "dense": 2})
    ctx.close()


def _pool(ctx, n_rows):
    """The context's whole descriptor pool, read back through the library's own unpack kernel (16-byte records, bit for bit)."""
    import torch
    v = ctx.process_raw(ctx.make_descs([0], [0]), 0, 0)  # (an empty batch: the view's device pointers)
    n_f4 = (n_rows * capi.FX_DESC_FLOATS + 3) // 4  # (the pool ends in four spare floats)
    out = torch.empty((n_f4, 4), dtype=torch.float32, device="cuda")
    lay = capi.FxPc2Layout(16, 0, 4, 8, 12, 0)
    capi.check(ctx.lib.fx_unpack_pointcloud2(ctx.handle, C.c_void_p(v.d_descriptors), n_f4, C.byref(lay), C.c_void_p(out.data_ptr())))
    ctx.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(-1)[:n_rows * capi.FX_DESC_FLOATS].reshape(n_rows, capi.FX_DESC_FLOATS)


@pytest.mark.parametrize("dense_slow", [0, 1])
def test_class_changes_between_batches(fx_hooks, dense_slow):
    """A, B, A through one context: at some global row index a row of every class is followed by a row of every class (group,
    wave, list, dense, no neighbour).  Every batch's rows are the oracle's, and every word of the pool outside the batch's rows'
    non-zero bins is zero — what a clear that ran twice, never ran or ran after the write leaves behind.  With the dense rows
    cleared and computed by the tier's own kernels (k_dense_finish: FX_DENSE_SLOW=0) and by the stand-in workgroups of k_desc's
    launch (dense_slow_loop: 1)."""
    fx_hooks(FX_DENSE_SLOW=dense_slow)
    p, A, B = class_batches()

    def classes(batch):
        out = []
        for scan, ora in batch:
            out += [class_of(int(n), s) for n, s in zip(ora["kp_neighbors"], rows.support_counts(scan, ora)[1])]
        return out
    ca, cb = classes(A), classes(B)
    assert len(ca) == len(cb) == 32
    assert set(zip(ca, cb)) == {(a, b) for a in CLASSES for b in CLASSES}, "an ordered pair of classes is missing"
    assert set(zip(cb, ca)) == {(a, b) for a in CLASSES for b in CLASSES}
    n_pool = 48  # (rows beyond the batch's 32 are never touched)
    ctx = capi.Context(p, capi.limits(4, 8192, max_total_keypoints=n_pool))
    for n, batch in enumerate((A, B, A)):
        got = _check(ctx, p, batch, f"batch {'ABA'[n]} ({n})")
        _check_tiers(ctx, batch, rows.LIST_CAP, f"batch {n}")
        want = np.concatenate([ora["descriptors"] for _, ora in batch])
        pool = _pool(ctx, n_pool)
        assert len(want) == 32
        util.assert_bit_equal(pool[:32], want, f"batch {n}: the pool's rows")
        util.assert_bit_equal(pool[:32], np.concatenate([g["descriptors"] for g in got]), f"batch {n}: the pool against the host copy")
        stray = (util.bits(pool[:32]) != 0) & (want == 0)
        assert not stray.any(), f"batch {n}: {int(stray.sum())} words outside the rows' non-zero bins are not zero, first at {np.argwhere(stray)[:4].tolist()}"
        assert not util.bits(pool[32:]).any(), f"batch {n}: rows beyond the batch were written"
    ctx.close()


# where the classification runs, which workgroups take the dense rows, and the grids of the one launch:
# name: (scans a batch, environment hooks of the test build, limits beyond the defaults, batches in flight)
PLACES = {
    "streaming-16-slices": (1, {}, {}, 1),                      # k_gather, sixteen workgroups a scan; k_rng_ord classifies
    "streaming-4-slices": (16, {}, {}, 1),                      # k_gather, four workgroups a scan; k_rng_ord
    "wide-solo": (64, {}, {}, 1),                               # k_gather_wide, the gather's own tail
    "counted-4": (16, dict(FX_GATHER_COUNTED=4), {}, 1),        # k_gather_count + k_gather_scatter; k_rng_ord
    "passes-sliced": (1, {}, dict(max_keypoints=2304, max_candidates=4096, max_total_keypoints=64), 1),   # k_gather_passes; k_rng_ord
    "passes-solo": (64, {}, dict(max_keypoints=2304, max_candidates=4096, max_total_keypoints=1024), 1),  # k_gather_passes, its own tail
    "dense-kernels": (1, dict(FX_DENSE_SLOW=0), {}, 1),         # k_dense_sort / _density / _finish (which clears its rows)
    "dense-stand-in": (1, dict(FX_DENSE_SLOW=1), {}, 1),        # dense_slow_loop in k_desc's launch
    "in-flight-1": (16, {}, {}, 1), "in-flight-3": (16, {}, {}, 3), "in-flight-4": (16, {}, {}, 4),  # the group workgroups' grid
    "desc-grid-1": (16, dict(FX_DESC_GRID=1), {}, 1), "desc-grid-7": (16, dict(FX_DESC_GRID=7), {}, 1),
}


@pytest.mark.parametrize("place", sorted(PLACES))
def test_every_place_the_classification_runs(fx_hooks, place):
    """The tier-edge scan through every gather mode, both homes of the dense rows, and the grids the hints choose among: the
    oracle's rows, every time (and so identical to each other), every tier with the rows meant for it.  Twice through the
    context: the second batch clears what the first one left."""
    batch, env, lim, in_flight = PLACES[place]
    fx_hooks(**env)
    p, scan, ora = edge_scene()
    ctx = capi.Context(p, capi.limits(batch, N_POINTS, **lim))
    ctx.set_batches_in_flight(in_flight)
    scenes = [(scan, ora)] * batch
    for rep in range(2):
        _check(ctx, p, scenes, f"{place}, batch {rep}")
        _check_tiers(ctx, scenes, rows.LIST_CAP, f"{place}, batch {rep}")
    ctx.close()


@functools.lru_cache(maxsize=None)
def exhaustion_scene():
    """Two dense rows (2500 and 2000 support points) next to a group and a wave row; a sorted pool of 4096 entries (the
    smallest a context takes) holds whichever of the two comes first and not the other."""
    ora_lib, p = _oracle(), rows.params()
    scan, want = scene8(ora_lib, p, [(20, 40), (1100, 2500), (100, 150), (900, 2000)], np.random.default_rng(461), n_points=8192)
    ora = ora_lib.run(p, scan)
    rows.check_counts(ora, scan, want, "pool exhaustion")
    return p, scan, ora


def run_exhaustion():
    p, scan, ora = exhaustion_scene()
    ctx = capi.Context(p, capi.limits(1, 8192, max_dense_points=4096))
    got = ctx.process_host([scan])[0]
    ctx.close()
    return got, ora


@pytest.mark.parametrize("dense_slow", [0, 1])
def test_pool_exhaustion_matches_the_recorded_verdict(fx_hooks, dense_slow):
    """max_dense_points too small for the second of two dense rows: the scan's flags, the neighbour counts and every row —
    the NaN row among them — are what the library produced before the tiers shared a launch (tests/golden/, recorded from
    this repository's own library at that commit), and every row but the NaN one is the oracle's."""
    fx_hooks(FX_DENSE_SLOW=dense_slow)
    got, ora = run_exhaustion()
    gold = np.load(GOLDEN)
    assert got["flags"] == int(gold["flags"]) and got["flags"] & capi.FX_FLAG_NBR_OVERFLOW
    assert np.array_equal(got["kp_neighbors"], gold["kp_neighbors"])
    util.assert_bit_equal(got["descriptors"], gold["descriptors"], "rows against the recorded ones")
    failed = [k for k in range(got["n_keypoints"]) if got["kp_neighbors"][k] == 0xffffffff]
    assert len(failed) == 1 and np.isnan(got["descriptors"][failed[0], :1980]).all() and not got["descriptors"][failed[0], 1980:].any()
    sup = rows.support_counts(exhaustion_scene()[1], ora)[1]
    assert failed[0] == max(k for k, n in enumerate(sup) if n > rows.LIST_CAP)  # the second of the two dense rows, in row order
    keep = [k for k in range(got["n_keypoints"]) if k != failed[0]]
    util.assert_bit_equal(got["descriptors"][keep], ora["descriptors"][keep], "the rows that fit")
