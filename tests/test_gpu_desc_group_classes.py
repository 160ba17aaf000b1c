"""The group tier of the descriptor stage takes its rows by SIZE CLASS (csrc/fx_kernels.hip: group_class, classify_rows,
desc_group_body<LANES>): rows of up to 16 / 32 / 64 support points run sixteen / eight / four to a wavefront, 4 / 8 / 16 lanes
and four support slots a lane each, from a work list per class that the support gather fills.  Every row is the oracle's, bit
for bit, whichever class computes it, whichever class wrote the row index last time, wherever the classification runs and
whatever the grid.  The scans are hand-built (tests/desc_rows_util.py): a row's neighbour count and support count are set exactly,
by points the detector never sees."""
import ctypes as C
import functools

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import desc_rows_util as rows
from tests import util
from tests.test_gpu_desc_one_launch import scene8

pytestmark = pytest.mark.gpu

CLASS_CAPS = (16, 32, 64)  # group_class_cap(0 .. 2): support points a row of the class holds at most (4 / 8 / 16 lanes, four slots each)
SUPPORT = (0, 1, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64)
# neighbour counts either side of a multiple of the class's lane count: the outer trips of the density loop
LANE_EDGES = {16: (4, 5, 12, 13), 32: (8, 9), 64: (16, 17, 48, 49)}


def class_of(n_support):
    """The row's size class; None: not a group row."""
    return next((c for c, cap in enumerate(CLASS_CAPS) if n_support <= cap), None)


def edge_cases(layout):
    out = []
    for sup in SUPPORT:
        marks = {0, 1, sup} | set(LANE_EDGES[CLASS_CAPS[class_of(sup)]])
        for nbr in sorted(n for n in marks if n <= sup):
            if layout == "origin" and nbr == 0:
                continue  # (the neighbour that is the keypoint)
            out.append((nbr, sup, layout))
    return out


def _oracle():
    from oracle import oracle_py
    oracle_py.load()
    return oracle_py


@functools.lru_cache(maxsize=None)
def built(cases, seed):
    """(params, ((scan, oracle result), ...)) of a tuple of cases, four a scan: built once a process; nobody writes into it."""
    p, scenes = rows.scenes(_oracle(), list(cases), seed)
    return p, tuple(scenes)


def _class_counts(ctx):
    """The last batch's group rows by size class (fx_debug_group_classes)."""
    cnt = (C.c_uint32 * 3)()
    ctx.lib.fx_debug_group_classes.argtypes = [C.c_void_p, C.c_void_p]
    capi.check(ctx.lib.fx_debug_group_classes(ctx.handle, cnt))
    return [int(c) for c in cnt]


def _expected_classes(scenes, failed_dense=0):
    """Rows per class by the device's support radius; dense rows without room in the pools ride in the widest class's list."""
    want = [0, 0, 0]
    for scan, ora in scenes:
        for n in rows.support_counts(scan, ora)[1]:
            if class_of(n) is not None:
                want[class_of(n)] += 1
    want[2] += failed_dense
    return want


def _check(ctx, scenes, tag, classes=True):
    got = ctx.process_host([s for s, _ in scenes])
    for b, (scan, ora) in enumerate(scenes):
        rows.compare(got[b], ora, f"{tag}, scan {b}", scan=scan)
    if classes:
        assert _class_counts(ctx) == _expected_classes(scenes), f"{tag}: group rows per size class"
    return got


@pytest.mark.parametrize("layout", ["mixed", "last", "origin"])
def test_class_edges(fxlib, layout):
    """Support counts at and beside 16 | 17, 32 | 33 and 64, down to 0 and 1; for each, no neighbour, one, all of them, and the
    counts either side of a multiple of the class's lane count."""
    cases = edge_cases(layout)
    assert {s for _, s, _ in cases} == set(SUPPORT) - ({0} if layout == "origin" else set())
    assert {(8, 17), (9, 32), (4, 15), (13, 16), (16, 33), (49, 64), (17, 63)} <= {(n, s) for n, s, _ in cases}
    p, scenes = built(tuple(cases), 70 + len(layout))
    ctx = capi.Context(p, capi.limits(len(scenes), 1024))
    for rep in range(2):  # (the second batch un-writes what the first recorded)
        _check(ctx, scenes, f"class edges, {layout}, batch {rep}")
    ctx.close()


NARROW = [(3, 5, "mixed"), (10, 16, "last"), (0, 7, "mixed"), (16, 16, "mixed")]
MIDDLE = [(8, 17, "mixed"), (20, 30, "mixed"), (32, 32, "last"), (1, 25, "origin")]
WIDE = [(40, 64, "mixed"), (17, 33, "mixed"), (50, 50, "last"), (0, 40, "mixed"), (33, 60, "mixed"), (48, 63, "origin")]
WAVES = [(30, 100, "mixed"), (64, 150, "mixed"), (100, 192, "last"), (0, 70, "mixed")]
PARTIAL = {
    "one-row-in-a-class": ([(10, 20, "mixed")], [0, 1, 0]),
    "seventeen-narrow-rows": ((NARROW * 5)[:17], [17, 0, 0]),  # a second trip with one group of sixteen live
    "narrow-rows-only": (NARROW + NARROW[::-1], [8, 0, 0]),
    "wide-rows-only": (WIDE, [0, 0, 6]),
    "no-group-row": (WAVES, [0, 0, 0]),
    "nine-middle-rows": ((MIDDLE * 3)[:9], [0, 9, 0]),         # a second trip with one group of eight live
}


@pytest.mark.parametrize("name", sorted(PARTIAL))
def test_partial_and_empty_wavefronts(fxlib, name):
    """Items (one trip's worth of rows: 16 / 8 / 4 list entries) that are not full, classes without a row, a batch without a group
    row: groups without a row stay idle, and nothing is read past the end of a list."""
    cases, want = PARTIAL[name]
    p, scenes = built(tuple(cases), 80 + len(name))
    assert _expected_classes(scenes) == want
    ctx = capi.Context(p, capi.limits(len(scenes), 1024))
    for rep in range(2):
        _check(ctx, scenes, f"{name}, batch {rep}")
    ctx.close()


# every class of the group tier, the wave and the list tier and a NaN row in each scan: (neighbours, support points) of eight poles
ALL_IN_ONE = [(3, 10), (10, 16), (20, 30), (40, 64), (100, 150), (200, 300), (5, 40), (0, 12)]


@functools.lru_cache(maxsize=None)
def all_in_one_batch():
    ora_lib, p = _oracle(), rows.params()
    out = []
    for i in range(6):
        cases = ALL_IN_ONE[i:] + ALL_IN_ONE[:i]
        scan, want = scene8(ora_lib, p, cases, np.random.default_rng(900 + i), n_points=1024)
        ora = ora_lib.run(p, scan)
        rows.check_counts(ora, scan, want, f"all in one, scan {i}")
        out.append((scan, ora))
    return p, tuple(out)


def test_every_class_and_tier_in_each_scan_of_a_batch(fxlib):
    """Six scans, each with rows of the three classes and of the wave and list tiers: every class's list gets its positions from
    several wavefronts of classify_rows, in whatever order they arrive."""
    p, scenes = all_in_one_batch()
    assert _expected_classes(scenes) == [18, 6, 12]
    ctx = capi.Context(p, capi.limits(len(scenes), 1024))
    for rep in range(2):
        _check(ctx, scenes, f"all in one, batch {rep}")
    ctx.close()


# what a row index is in turn (pole j of batch n: HISTORY[(n + j) % 9]): a 33-64 row that records more than 16 bins, a <= 16 row
# (the narrow group un-writes the long record), a wave row (left dirty), a <= 16 row (the whole row zeroed), a row without
# neighbours (NaN, left dirty), a <= 32 row, a 33-64 row that records more than 32 bins, and a <= 32 row right behind it (the
# group of eight lanes un-writes the record's slots behind its own 32), a <= 16 row behind that one (a record of 17-32 bins)
HISTORY = [(56, 64, "mixed"), (9, 14, "mixed"), (80, 120, "mixed"), (12, 16, "last"), (0, 10, "mixed"), (24, 31, "mixed"),
           (54, 62, "mixed"), (20, 28, "mixed"), (6, 12, "mixed")]


def test_rows_reused_across_classes(fxlib):
    """One context, twelve batches over the same four row indices.  A bin left behind by a class that un-wrote too little of
    another class's record shows as a non-zero word the oracle does not have."""
    ctx, n_bins, seen = None, None, set()
    for n in range(12):
        cases = tuple(HISTORY[(n + j) % len(HISTORY)] for j in range(4))
        p, scenes = built(cases, 300 + n)
        (scan, ora), = scenes
        if ctx is None:
            ctx = capi.Context(p, capi.limits(1, 1024))
        _check(ctx, scenes, f"history, batch {n}")
        # (what the row indices went through: the bins recorded last time and this batch's size class, group rows only)
        sup = rows.support_counts(scan, ora)[1]
        if n_bins is not None:
            seen |= {(min(b - 1, 63) // 16, class_of(s)) for b, s, was in zip(n_bins, sup, was_group) if was and b > 0 and class_of(s) is not None}
        n_bins = [int(x) for x in (ora["descriptors"][:, :capi.FX_DESC_BINS] != 0).sum(axis=1)]
        was_group = [class_of(s) is not None and nb > 0 for s, nb in zip(sup, ora["kp_neighbors"])]
    ctx.close()
    # records of 17-32, 33-48 (or more) bins un-written by the narrowest class, and of more than 32 by the middle one
    assert {(1, 0), (2, 0), (2, 1)} <= {(min(q, 2), c) for q, c in seen}, sorted(seen)


def test_pool_exhaustion_beside_narrow_rows(fxlib):
    """Dense rows that each exceed a 4096-entry pool (the outcome does not depend on who draws first) beside narrow rows: the
    dense rows come back NaN and flagged — they ride in the widest class's list —, the other rows are the oracle's, and the
    next batch through the same rows is clean."""
    p, (exhaust,), cases = rows.built("csr_exhaust")
    _, narrow = built(tuple(NARROW), 400)
    _, after = built(tuple(MIDDLE + NARROW), 401)
    n_dense = sum(sup > rows.LIST_CAP for _, sup, _ in cases)
    assert n_dense == 2 and all(sup > 4096 for _, sup, _ in cases if sup > rows.LIST_CAP)
    batch = [exhaust, narrow[0]]
    ctx = capi.Context(p, capi.limits(2, 1 << len(exhaust[0]).bit_length(), max_dense_points=4096))
    got = ctx.process_host([s for s, _ in batch])
    assert got[0]["flags"] == capi.FX_FLAG_NBR_OVERFLOW and got[1]["flags"] == 0
    sup = rows.support_counts(*exhaust)[1]
    failed = [k for k, n in enumerate(sup) if n > rows.LIST_CAP]
    keep = [k for k in range(len(sup)) if k not in failed]
    assert len(failed) == n_dense and (got[0]["kp_neighbors"][failed] == 0xffffffff).all()
    assert np.isnan(got[0]["descriptors"][failed][:, :capi.FX_DESC_BINS]).all() and not got[0]["descriptors"][failed][:, capi.FX_DESC_BINS:].any()
    util.assert_bit_equal(got[0]["descriptors"][keep], exhaust[1]["descriptors"][keep], "the rows beside the failed ones")
    assert np.array_equal(got[0]["kp_neighbors"][keep], exhaust[1]["kp_neighbors"][keep])
    rows.compare(got[1], narrow[0][1], "the narrow scan of the exhausted batch", scan=narrow[0][0])
    assert _class_counts(ctx) == _expected_classes(batch, failed_dense=n_dense)
    _check(ctx, after, "the batch after the exhausted one")
    ctx.close()


# where the classification runs and the grid of the group workgroups: (scans a batch, environment hooks of the test build)
PLACES = {
    "one-workgroup-a-scan": (64, {}),                        # the gather's own tail classifies
    "sliced": (3, {}),                                       # several workgroups a scan: k_rng_ord classifies
    "counted-5": (3, dict(FX_GATHER_COUNTED=5)),             # k_gather_count + k_gather_scatter; k_rng_ord
    "desc-grid-1": (12, dict(FX_DESC_GRID=1)),               # one group workgroup takes every item of every class
    "desc-grid-400": (12, dict(FX_DESC_GRID=400)),           # more wavefronts than items
}
PLACE_CASES = tuple(NARROW + MIDDLE + WIDE + WAVES + [(5, 16, "origin"), (8, 32, "mixed")] + NARROW[:2] + WIDE[:2] + MIDDLE[:2])


@pytest.mark.parametrize("place", sorted(PLACES))
def test_every_classifier_and_any_grid(fx_hooks, place):
    """The same scenes through every home of the classification and through grids smaller and larger than the items: the
    oracle's rows every time, and so the same bytes."""
    batch, env = PLACES[place]
    fx_hooks(**env)
    p, scenes = built(PLACE_CASES, 500)
    scenes = [scenes[i % len(scenes)] for i in range(batch)]
    ctx = capi.Context(p, capi.limits(batch, 1024))
    for rep in range(2):
        _check(ctx, scenes, f"{place}, batch {rep}")
    ctx.close()
