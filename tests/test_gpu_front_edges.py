"""The front path on the device at fp32's edges (the scenes and their hand-stated tables: tests/front_edges_util.py; that they
sit where they claim: tests/test_front_edges_scenes.py): the filter's faces, the cluster radius, the size and diameter gates,
the +-1000 box, the fp64 centroid sums, the merge radius with its hashed grid, and the ring windows of a non-dyadic step —
through every body that restates those decisions: k_front fused, streamed (sliced pass + k_front_cd) and as two launches,
k_front_redo, k_slow, the separate kernels with both run tiers and the workgroup tier, the sliced prep, the merge tiers, and the
product library as it chooses for itself.  One context per (parameters, variant), one batch of all its scenes; every result is
held to the oracle (util.compare_scan) AND to the scene's table, and every variant is checked to have run (the tier hints,
the work-list counters, fx_debug_front)."""
import ctypes as C

import pytest

from feature_extraction_amd import capi
from tests import front_edges_util as fe
from tests import util

pytestmark = pytest.mark.gpu


_ORACLE = {}


def _oracle_of(oracle, sc):
    """The oracle's result of a scene, computed once a process and never written to."""
    key = (sc["name"], sc["group"])
    if key not in _ORACLE:
        _ORACLE[key] = oracle.run(fe.params(sc["group"]), sc["scan"], roll=sc["roll"], pitch=sc["pitch"])
    return _ORACLE[key]


def _state(ctx):
    """(tier hints [8], work-list counters [16], 1 if the last batch took the front kernel) of the context's last batch."""
    h, cnt = (C.c_uint32 * 8)(), (C.c_uint32 * 16)()
    ctx.lib.fx_debug_tier_hints.argtypes = [C.c_void_p, C.c_void_p]
    ctx.lib.fx_debug_counters.argtypes = [C.c_void_p, C.c_void_p]
    ctx.lib.fx_debug_front.argtypes = [C.c_void_p]
    ctx.lib.fx_debug_front.restype = C.c_int
    capi.check(ctx.lib.fx_debug_tier_hints(ctx.handle, h))
    capi.check(ctx.lib.fx_debug_counters(ctx.handle, cnt))
    return [int(v) for v in h], [int(v) for v in cnt], int(ctx.lib.fx_debug_front(ctx.handle))


def _batch(oracle, ctx, scenes, tag):
    got = ctx.process_host([s["scan"] for s in scenes], roll=[s["roll"] for s in scenes], pitch=[s["pitch"] for s in scenes])
    state = _state(ctx)
    for g, sc in zip(got, scenes):
        util.compare_scan(g, _oracle_of(oracle, sc), tag=f"{tag}: {sc['name']}")
        fe.check_expect(g, sc, tag=f"{tag}: ")
    return state


def _run(oracle, group, scenes, tag, **lim):
    ctx = capi.Context(fe.params(group), capi.limits(len(scenes), 2048, **lim))
    try:
        return _batch(oracle, ctx, scenes, f"{tag}, {group}")
    finally:
        ctx.close()


FRONT_GROUPS = [g for g in fe.PARAMS if fe.PARAMS[g].get("n_rings", 16) <= 32 and g != "r32"]  # (r32: the tier scenes' parameters)
VARIANTS = {"fused": dict(FX_FRONT_STREAM=0), "streamed": dict(FX_FRONT_STREAM=1), "two launches": dict(FX_FRONT_SPLIT=1),
            "two launches, lean": dict(FX_FRONT_SPLIT=2), "k_front_redo": dict(FX_FRONT_FORCE=1), "k_slow": dict(FX_FRONT_FORCE=2)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_scene_through_the_front_kernel(fx_hooks, oracle, variant):
    """k_front in its three shapes — hints (0, 0): nothing handed on —, and every scan forced on to k_front_redo (hints (B, 0))
    and from there to k_slow (hints (B, B))."""
    fx_hooks(**VARIANTS[variant])
    groups = fe.by_group()
    for group in FRONT_GROUPS:
        scenes = groups[group]
        hints, _, front = _run(oracle, group, scenes, variant)
        want = {"k_front_redo": (len(scenes), 0), "k_slow": (len(scenes), len(scenes))}.get(variant, (0, 0))
        assert front == 1 and (hints[6], hints[7]) == want, f"{variant}, {group}: front {front}, hints {hints}, {len(scenes)} scans"


def test_every_scene_through_the_separate_kernels(fx_hooks, oracle):
    """FX_FRONT=0: k_prep, k_bucket, k_rings_runs (first run tier; nothing handed on) and k_merge_small; the 64-ring scenes of the
    non-dyadic step too (k_bucket_many)."""
    fx_hooks(FX_FRONT=0)
    for group, scenes in fe.by_group().items():
        hints, cnt, front = _run(oracle, group, scenes, "separate")
        assert front == 0 and (cnt[0], cnt[5]) == (0, 0) and hints[2:4] == [0, 0] and hints[6:8] == [0, 0], f"separate, {group}: {front} {cnt} {hints}"


@pytest.mark.parametrize("slices", [2, 16])
def test_the_faces_through_the_sliced_prep(fx_hooks, oracle, slices):
    fx_hooks(FX_FRONT=0, FX_PREP_SLICES=slices)
    groups = fe.by_group()
    for group in ("faces", "zeros", "open"):
        _, _, front = _run(oracle, group, groups[group], f"{slices} slices")
        assert front == 0


@pytest.mark.parametrize("kind", ["second", "workgroup16", "workgroup32"])
def test_the_radius_scenes_in_the_later_ring_tiers(fx_hooks, oracle, kind):
    """A filler of single-return runs on the scenes' ring pushes it past the first run tier's 128 runs: into the second run
    tier (32 rings, up to 256 runs: k_rings_runs2) and into the workgroup tier (k_rings_large)."""
    fx_hooks(FX_FRONT=0)
    scenes = fe.tier_scenes(kind)
    _, cnt, front = _run(oracle, fe.TIERS[kind][0], scenes, kind, **fe.WIDE_LIMITS)
    B = len(scenes)
    want = {"second": (B, 0), "workgroup16": (0, B), "workgroup32": (B, B)}[kind]
    assert front == 0 and (cnt[0], cnt[5]) == want, f"{kind}: counters {cnt[:8]}, {B} scans"


@pytest.mark.parametrize("tier", ["big", "huge", "slow"])
def test_the_merge_scenes_in_the_later_merge_tiers(fx_hooks, oracle, tier):
    """A filler of 520 single-return candidates takes a scan past k_merge_small (512 candidates) into k_merge_big; the hooks
    lower that tier's capacity to hand the scan on to k_merge_huge, and that one's to hand it on to k_slow."""
    fx_hooks(**{"big": dict(FX_FRONT=0), "huge": dict(FX_FRONT=0, FX_MERGE_BIG_CAP=64),
                "slow": dict(FX_FRONT=0, FX_MERGE_BIG_CAP=64, FX_MERGE_HUGE_CAP=128)}[tier])
    scenes = fe.tier_scenes("merge")
    hints, _, front = _run(oracle, "tol01", scenes, f"merge {tier}", **fe.WIDE_LIMITS)
    B = len(scenes)
    want = {"big": (B, 0, 0), "huge": (B, B, 0), "slow": (B, B, B)}[tier]
    assert front == 0 and (hints[2], hints[3], hints[7]) == want, f"merge {tier}: hints {hints}, {B} scans"


def test_the_product_library_in_batches_of_nine_and_of_fewer(fxlib, oracle):
    """No hooks: what the product chooses — the fused kernel for nine scans and more, the sliced pass for up to eight."""
    for group, scenes in fe.by_group().items():
        ctx = capi.Context(fe.params(group), capi.limits(max(len(scenes), 9), 2048))
        try:
            many = (scenes * 9)[:max(len(scenes), 9)]
            for part, tag in ((many, "product"), (scenes[:8][::-1], "product, up to eight")):
                hints, _, front = _batch(oracle, ctx, part, f"{tag}, {group}")
                assert (hints[6], hints[7]) == (0, 0) and front == (1 if group in FRONT_GROUPS else 0), f"{tag}, {group}: {front} {hints}"
        finally:
            ctx.close()
