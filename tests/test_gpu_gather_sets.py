"""What the support gather WRITES, compared directly with a brute-force numpy reference (tests/gather_util.py): every row's list
and overflow entries as a multiset of point indices with bit-equal coordinates, the true counts, the overflow count, the rows'
classes and work lists, the 3DSC x-axis ordinals (row_xa) and the streaming pass's near-sector bits — read back through
fx_test_gather_state (the test build).  Until now all of this was seen only through the descriptor rows k_desc makes of it: a lost
support point arrived as "descriptor max |diff| 3e-4, row 17".  Here it arrives as "wide, run 0: scan 0, keypoint 2 (row 2): 1
support points are missing from the list, first point 65536 (d2 = ...)".  Every comparison is exact.

Every case runs through the kinds of gather that can reach it (KINDS), each context runs its batch twice, and every scan is also
held against the oracle end to end, bit for bit (desc_rows_util.compare), so the direct test and the end-to-end one stand side by
side.  The scenes — what sits at which scan index and why — are checked on the CPU by tests/test_gather_scenes.py.

Left out: the 64-tile refill of the near-sector words for sixteen counted slices or sixteen staged workgroups a scan (it needs
more than a million points a scan)."""
import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import desc_rows_util as du
from tests import gather_util as gu
from tests import util

pytestmark = pytest.mark.gpu

# kind: (environment hooks of the test build, scans the batch is padded to with empty ones, limits)
# (FX_GATHER_COUNTED=1 pins "no counted slices": a handful of scans of 65 536 points and more would otherwise take them, and the
#  staged workgroups — what every small batch of VLP-16-sized scans runs — would never see the long scans.)
KINDS = {
    "one256": (dict(FX_GATHER_ONE=256), 0, {}),         # k_gather, one workgroup a scan: direct hits, its own tail (from 1024 scans a batch)
    "wide": (dict(FX_GATHER_ONE=1024), 0, {}),          # k_gather_wide (from 64 scans a batch)
    "staged16": (dict(FX_GATHER_COUNTED=1), 0, {}),     # k_gather, 16 workgroups a scan: staged hits, k_rng_ord is the tail
    "staged4": (dict(FX_GATHER_COUNTED=1), 16, {}),     # k_gather, 4 workgroups a scan (batches of 16 to 63)
    "counted3": (dict(FX_GATHER_COUNTED=3), 0, {}),     # k_gather_count + k_gather_scatter
    "counted16": (dict(FX_GATHER_COUNTED=16), 0, {}),
    "passes": (dict(FX_GATHER_COUNTED=1), 0, dict(max_keypoints=2049)),  # k_gather_passes with scans that fit one pass (16 workgroups a scan)
}
EMPTY = np.zeros((0, 4), np.float32)


def check_constants(st, p, lim):
    want = gu.constants(float(p.descriptor_radius))
    for name, w in zip(("r2_support", "r2_search", "box_margin"), want):
        assert st[name] == w, f"{name}: the library reports {st[name]!r}, the reference computes {w!r}"
    assert st["list_cap"] == min(lim.max_neighbors, 4096) and st["dense_min"] == gu.DENSE_MIN
    # whole tiles of the widest gather workgroup: its wavefronts fetch their sector words for every tile that starts below n
    assert st["near_words"] * 128 >= (lim.max_points + 4095) // 4096 * 4096, (st["near_words"], lim.max_points)


def run_batches(fx_hooks, kind, batches, max_points, compare=du.compare, dense_cap=None, **lim_over):
    """One context of the kind; every batch (a list of scene names) twice; state and oracle checked after each (compare None: the
    scene exhausts the dense tier's pools on purpose — see gather_util.check_state's dense_cap —, its scans must be flagged)."""
    env, pad_to, lim_kind = KINDS[kind]
    fx_hooks(**env)
    p = gu.built(batches[0][0])["p"]
    width = max(max(len(b) for b in batches), pad_to)
    over = {**lim_kind, **lim_over}
    over.update({k: max(v, lim_kind[k]) for k, v in lim_over.items() if k in lim_kind})  # (max_keypoints: the larger of the kind's and the case's)
    lim = capi.limits(width, max_points, **over)
    ctx = capi.Context(p, lim)
    try:
        for names in batches:
            scenes = [gu.built(n) for n in names]
            scans = [s["scan"] for s in scenes] + [EMPTY] * (pad_to - len(scenes))
            refs = [s["ref"] for s in scenes] + [None] * (pad_to - len(scenes))
            for rep in range(2):
                tag = f"{kind}, batch {'+'.join(names)}, run {rep}"
                got = ctx.process_host(scans)
                st = ctx.gather_state()
                check_constants(st, p, ctx.limits)
                gu.check_state(st, got, refs, tag, dense_cap=dense_cap)
                for b, s in enumerate(scenes):
                    if compare is None:
                        assert got[b]["flags"] == capi.FX_FLAG_NBR_OVERFLOW, f"{tag}: scan {b} flags {got[b]['flags']:#x}"
                    else:
                        compare(got[b], s["ora"], f"{tag}: scan {b} against the oracle", s["scan"], list_cap=st["list_cap"])
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_sector_addressing_at_every_edge(fx_hooks, kind):
    """(a) 263 000 points of filler, four poles, and support points at the scan indices either side of 4, 64, 128, 256, 1024, 2048,
    4096, 65 536, 131 072, 196 608 and 262 144, at 0 and at n - 1 — each alone in its sector (edges) or its whole sector
    (edges_quad) —, beside scans of 4 k + 1 and 4 k + 3 points whose last point is a support point.  Under 0.1 % of the sectors are near: a
    near-sector word fetched for the wrong tile, wavefront or slice loads other points, and the sets show which."""
    run_batches(fx_hooks, kind, [["edges", "edges_quad", "short1", "short3"]], 263168)


@pytest.mark.parametrize("kind", list(KINDS))
def test_gates_at_equality(fx_hooks, kind):
    """(b) Points whose d2 is the float below r2_support, equal to it and above it: only the first is a support point.  A keypoint
    whose only candidate sits exactly at r2_search has no neighbour and draws no x-axis — the ordinals of the keypoints behind it
    show that in row_xa —; its twin one float closer has one."""
    eq, below = gu.built("gate_search_eq")["ref"], gu.built("gate_search_below")["ref"]
    assert not eq.has_nbr[0] and eq.has_nbr[1:].all() and below.has_nbr.all()
    run_batches(fx_hooks, kind, [["gate_support", "gate_search_eq", "gate_search_below"]], 3000)


@pytest.mark.parametrize("kind", list(KINDS))
def test_widened_box_and_thin_grids(fx_hooks, kind):
    """(c) Points one float outside, on and one float inside each of the six faces of the widened box (the near bits are exact on both
    sides), support points beyond the filter's faces out to the support radius; (d) one keypoint alone, and two keypoints of equal
    x: keypoint grids of one cell and of one column."""
    run_batches(fx_hooks, kind, [["faces", "one_keypoint", "equal_x"]], 3000)


@pytest.mark.parametrize("kind", list(KINDS))
def test_spread_keypoints_widen_the_cells(fx_hooks, kind):
    """(d) Forty poles over the whole 75 m x 60 m box: the cells widen to 2.1 m x 1.7 m (31 x 31 of them), every keypoint has a ring of
    24 support points at 0.95 support radii, and some rings cross cell borders in each of the four directions.  (The rings lie inside
    the filter box, where the detector sees them: against the oracle the suite's usual bound, util.compare_scan.)"""
    run_batches(fx_hooks, kind, [["spread"]], 4096, compare=lambda got, ora, tag, scan, list_cap: util.compare_scan(got, ora, tag=tag))


@pytest.mark.parametrize("kind", list(KINDS))
def test_burst_of_hits_across_a_tile_and_the_list_cap(fx_hooks, kind):
    """(e) 1024 consecutive scan points from index 512 on, all in one keypoint's support set, max_neighbors = 256: the staged kinds
    fill their 384-entry stage within a tile (512 hits in each of two tiles) and hand over to direct appends beside later flushes,
    the list crosses list_cap inside the burst, a queue is drained in the middle of a load, and 768 entries land in the overflow
    region in every kind."""
    assert gu.built("burst")["ref"].counts().tolist() == [1024]
    run_batches(fx_hooks, kind, [["burst"]], 6000, max_neighbors=256)


@pytest.mark.parametrize("kind", list(KINDS))
def test_what_a_context_remembers(fx_hooks, kind):
    """(f) A long scan with every sector near, then in the same slot a short sparse one (the stale sector words behind it must not be
    read), then a scan without keypoints, then one with keypoints."""
    run_batches(fx_hooks, kind, [["all_near"], ["short3"], ["no_keypoints"], ["short1"]], 20000)


def _bound(got, ora, tag, scan, list_cap):
    util.compare_scan(got, ora, tag=tag)


@pytest.mark.parametrize("kind", list(KINDS))
def test_crowded_cells_and_points_of_several_sets(fx_hooks, kind):
    """(d) 965 keypoints 0.95 m apart under a support radius of 3 m: up to 25 keypoints share a cell (a cell's list holds its eight
    neighbours' too) and every point of the scan belongs to more than two support sets — a candidate loop that dropped the second
    keypoint of a cell, or a drain, flush or scatter that appended a point to one row only, shows here in every kind.  (Points of
    tests/test_gpu_gather_passes.py's scene within 30 degrees of the x axis: below the LDS tables' 2048 keypoints.)"""
    run_batches(fx_hooks, kind, [["crowded"]], 4096, compare=_bound, max_ring_points=2400, max_ring_candidates=1024, max_candidates=4096,
                max_keypoints=2048, max_total_keypoints=2048, max_kpc_points=16384)


@pytest.mark.parametrize("kind", list(KINDS))
def test_burst_shared_by_overlapping_spheres(fx_hooks, kind):
    """(e) at R = 0.5 m: desc_rows_util's three keypoints 42 cm apart, 5100 consecutive scan points every one of which is a hit, 4100
    of them in two support sets and 1287 in all three, max_neighbors = 256: all three lists cross list_cap inside the burst, and
    more than 9000 entries of three rows interleave in the scan's overflow region."""
    run_batches(fx_hooks, kind, [["shared"]], 8192, max_neighbors=256,
                compare=lambda got, ora, tag, scan, list_cap: du.compare(got, ora, tag, scan, radius=du.R_SHARED, list_cap=list_cap))


@pytest.mark.parametrize("kind", list(KINDS))
def test_keypoints_at_a_corner_and_at_a_z_face(fx_hooks, kind):
    """(c) A narrow pole whose keypoint lies 2 mm inside the x and the y face of the filter box at once, support points beyond both;
    and — one detection channel — a single ring's cluster whose keypoint lies 1.2 mm under z_max, support points above it."""
    run_batches(fx_hooks, kind, [["corner"]], 3000)
    run_batches(fx_hooks, kind, [["zface"]], 3000)


@pytest.mark.parametrize("kind", list(KINDS))
def test_dense_row_without_room_in_the_pools(fx_hooks, kind):
    """Row tables, the last clause: dense WITHOUT room.  The three dense rows of the shared scene (3180, 4104, 3180 support points)
    against a sorted pool of 8192 entries: the first two fit, the third is FX_ROW_DENSE_FAIL — listed with the widest group class,
    FX_NONE in its slot of dense_rows, the scan flagged —, and its list and overflow entries are the support set all the same."""
    run_batches(fx_hooks, kind, [["shared"]], 8192, compare=None, dense_cap=8192, max_dense_points=8192)


# (g) beyond the LDS tables: always k_gather_passes; the batch decides its workgroups a scan
PASSES = {"passes16": 1, "passes4": 16, "passes1": 64}


@pytest.mark.parametrize("kind", list(PASSES))
@pytest.mark.parametrize("scene", ["many", "many_thin"])
def test_passes_across_the_table_limit(fx_hooks, kind, scene):
    """(g) tests/test_gpu_gather_passes.py's scenes of more than 2048 keypoints in 28 800 points, brute force in numpy: the sets of every
    pass, and the x-axis ordinals across the passes through row_xa directly (many_thin: hundreds of keypoints without a neighbour)."""
    s = gu.built(scene)
    width = PASSES[kind]
    lim = capi.limits(width, 28800, max_ring_points=2400, max_ring_candidates=1024, max_candidates=4096, max_keypoints=4096,
                      max_total_keypoints=8192, max_kpc_points=16384)
    ctx = capi.Context(s["p"], lim)
    try:
        scans, refs = [s["scan"]] + [EMPTY] * (width - 1), [s["ref"]] + [None] * (width - 1)
        for rep in range(2):
            got = ctx.process_host(scans)
            st = ctx.gather_state()
            check_constants(st, s["p"], ctx.limits)
            gu.check_state(st, got, refs, f"{kind}, {scene}, run {rep}")
            util.compare_scan(got[0], s["ora"], tag=f"{kind}, {scene}, run {rep}: against the oracle")
    finally:
        ctx.close()
