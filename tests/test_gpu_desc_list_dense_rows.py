"""The list tier (desc_body through desc_wg_loop, 193..1024 support points), the dense tier (k_dense_sort, k_dense_density,
k_dense_finish), its stand-in dense_slow_loop and the overflowed-list route, bit for bit against the oracle at the counts where
their code changes shape.  The numerics contract of these tiers is the ORDER of one sequential fp32 sum per bin — (bin, d2,
index) ascending — so a wrong in-bin rank, a key dropped at a chunk edge or a density off by one at a window edge is a changed
bit on rows like these and often less than compare_scan's 1e-5 on a random scan.

The rows are hand-built (tests/desc_rows_util.py): every row's neighbour count and support count is set exactly; that the scenes
are what they claim, and that their sums do depend on their order, is checked on the CPU by tests/test_desc_rows_scenes.py.
Every comparison is desc_rows_util.compare: compare_scan, every descriptor word, no inexact value; a failure names scan, row,
tier, bin and both bit patterns."""
import ctypes as C

import pytest

from feature_extraction_amd import capi
from tests import desc_rows_util as rows

pytestmark = pytest.mark.gpu


def _limits(scans, **over):
    """Sized to the scene: max_points the next power of two above the longest scan, default pools unless the case says otherwise."""
    return capi.limits(len(scans), 1 << max(len(s) for s in scans).bit_length(), **over)


def _dense_rows(ctx):
    """Rows the last batch handed to the dense tier (fx_debug_tier_hints()[4])."""
    h = (C.c_uint32 * 8)()
    ctx.lib.fx_debug_tier_hints.argtypes = [C.c_void_p, C.c_void_p]
    capi.check(ctx.lib.fx_debug_tier_hints(ctx.handle, h))
    return int(h[4])


def _tiers(scenes, list_cap=rows.LIST_CAP):
    return [rows.tier_of(n, list_cap) for scan, ora in scenes for n in rows.support_counts(scan, ora)[1]]


def _run(p, scenes, tag, list_cap=rows.LIST_CAP, ctx=None, **lim):
    """One batch of the scenes through a context (a fresh one unless given), every scan against its oracle result."""
    scans = [s for s, _ in scenes]
    own = ctx is None
    if own:
        ctx = capi.Context(p, _limits(scans, **lim))
    got = ctx.process_host(scans)
    for b, (scan, ora) in enumerate(scenes):
        rows.compare(got[b], ora, f"{tag}, scan {b}", scan=scan, radius=float(p.descriptor_radius), list_cap=list_cap)
    n_dense = _dense_rows(ctx)
    if own:
        ctx.close()
    return n_dense


def test_list_tier_rows(fxlib):
    """0 (NaN), 1 (the keypoint itself / one binned) neighbours; the `parts` edges of the density pass (32 / 33, 64 / 65,
    128 / 129 neighbours: 8, 4, 2, 1 lanes a count); the 256-wide trips of the compaction (255, 256, 257); 193 / 193 and
    1024 / 1024 (every support point a neighbour, the tier's first and last count); neighbours behind the shell; a few bins
    with hundreds of terms; duplicate points."""
    p, scenes, cases = rows.built("list")
    tiers = _tiers(scenes)
    assert len(tiers) == len(cases) == 19 and set(tiers) == {"list"}
    assert _run(p, scenes, "list tier") == 0


@pytest.mark.parametrize("slow", [0, 1])
def test_dense_tier_rows(fx_hooks, slow):
    """1025 support points (0 — NaN —, 1 — the keypoint —, 1024 and 1025 neighbours), 1023 / 1024 / 1025 neighbours in 2047 /
    2048 / 2049 support points (k_dense_density's work items of 1024 queries and windows of 2048 targets), a row in each of the
    tier's four size classes, a few bins with hundreds of terms, duplicate points: by the tier's kernels (FX_DENSE_SLOW=0) and by
    dense_slow_loop (=1)."""
    fx_hooks(FX_DENSE_SLOW=slow)
    p, scenes, cases = rows.built("dense")
    tiers = _tiers(scenes)
    assert len(tiers) == len(cases) == 13 and set(tiers) == {"dense"}
    assert _run(p, scenes, f"dense tier, FX_DENSE_SLOW={slow}") == 13


def test_dense_rows_in_the_product_library(fxlib):
    """No hook: the library chooses.  A context whose last batch had no dense row computes the dense rows of the next one by
    dense_slow_loop and those of the batches after it by the tier's kernels (a fresh context, knowing nothing, starts with the
    kernels): one batch without dense rows, then the same dense batch three times, every result the oracle's."""
    p, dense, _ = rows.built("dense")
    _, lst, _ = rows.built("list")
    batch = dense[:2]
    ctx = capi.Context(p, _limits([s for s, _ in batch + lst[:2]]))
    assert _run(p, lst[:2], "product library, list rows first", ctx=ctx) == 0
    for rep in range(3):
        assert _run(p, batch, f"product library, dense batch {rep}", ctx=ctx) == 8
    ctx.close()


def test_dense_finish_key_sort_beyond_a_small_lds_limit(fx_hooks):
    """k_dense_finish sorts up to dense_lds_keys binned neighbours in LDS and larger rows by a bitonic network in the key pool,
    padded to a power of two: with the limit at 300, rows that bin 299, 300, 301, 512, 513 and 1025 neighbours."""
    fx_hooks(FX_DENSE_LDS_KEYS=300, FX_DENSE_SLOW=0)
    p, scenes, cases = rows.built("keys")
    assert [n for n, _, _ in cases] == [299, 300, 301, 512, 513, 1025] and set(_tiers(scenes)) == {"dense"}
    assert _run(p, scenes, "FX_DENSE_LDS_KEYS=300") == 6


@pytest.fixture(scope="module")
def big_rows():
    return rows.built("big0")[0], rows.built("big0")[1] + rows.built("big1")[1]


def test_dense_finish_key_sort_at_the_real_lds_limit(fxlib, big_rows):
    """... and at the real limit, no hook: 14 336 binned neighbours (the last row sorted in LDS) and 14 337 (the first sorted in
    the key pool) in 14 400 support points, a batch of the two scans."""
    p, scenes = big_rows
    assert [int(ora["kp_neighbors"][0]) for _, ora in scenes] == [14336, 14337]
    assert _run(p, scenes, "14336 / 14337 keys") == 2


@pytest.mark.parametrize("slow", [0, 1])
@pytest.mark.parametrize("L", [32, 256])
def test_overflowed_lists(fx_hooks, L, slow):
    """max_neighbors = L: rows of L - 1 and L support points stay in their own tier; L + 1 and 4 L overflow their lists — the
    entries beyond L sit in the scan's overflow region — and go to the dense tier."""
    fx_hooks(FX_DENSE_SLOW=slow)
    p, scenes, cases = rows.built(f"overflow{L}")
    assert [s for _, s, _ in cases] == [L - 1, L, L + 1, 4 * L]
    own = "group" if L <= rows.GROUP_CAP else "list"
    assert sorted(_tiers(scenes, L)) == sorted([own, own, "dense", "dense"])
    assert _run(p, scenes, f"max_neighbors={L}, FX_DENSE_SLOW={slow}", list_cap=L, max_neighbors=L) == 2


def test_shared_densities(fxlib):
    """The dense tier computes a point's local density once a scan, by the row that claims it first, and every row that has the
    point as a neighbour reads it: three rows at R = 0.5 m whose neighbour sets overlap (tests/test_desc_rows_scenes.py: more
    than 1024 support points each, at least 200 points shared).  Alone; as scan 1 behind another dense scene; and in a context that
    has just processed another scene of the same number of points at other coordinates — a density kept from scan to scan or from
    batch to batch would be read for the wrong point."""
    p, scan, ora = rows.built_shared(0)
    _, other, ora_other = rows.built_shared(1)
    assert _run(p, [(scan, ora)], "shared densities, alone") == 3
    assert _run(p, [(other, ora_other), (scan, ora)], "shared densities, scan 1 of a batch") == 6
    ctx = capi.Context(p, _limits([scan]))
    assert _run(p, [(other, ora_other)], "shared densities, the other scene first", ctx=ctx) == 3
    assert _run(p, [(scan, ora)], "shared densities, after another scene of the same size", ctx=ctx) == 3
    assert _run(p, [(other, ora_other)], "shared densities, and back", ctx=ctx) == 3
    ctx.close()


def test_every_tier_in_one_batch(fxlib):
    """Four scans whose rows mix group, wave, list, dense and NaN rows, five batches in rotating order (and of different sizes)
    through one context: a row index sees another tier every time."""
    p, scenes, cases = rows.built("all")
    assert len(scenes) == 4
    assert all(len(set(_tiers([scene]))) >= 3 for scene in scenes)  # (three or four tiers in every scan)
    assert set(_tiers(scenes)) == {"group", "wave", "list", "dense"} and sum(n == 0 for n, _, _ in cases) == 3
    ctx = capi.Context(p, _limits([s for s, _ in scenes]))
    for rep in range(5):
        order = [(rep + b) % 4 for b in range(4)][: 4 - rep % 2]
        _run(p, [scenes[i] for i in order], f"batch {rep} (scenes {order})", ctx=ctx)
    ctx.close()
