"""Prescribed size sequences (tests/sort_scenes_util.py; that the scenes can fail: tests/test_sort_scenes.py) through every body
that holds an instance of the cluster-order replay.  One context per (parameters, variant), one batch of all its scenes; every
result is held to the scene's own table — sizes and centroid bits in the order the oracle's bare std::sort gives — AND to
oracle.run (util.compare_scan, descriptors included), and every variant is checked to have run (tier hints, counters,
fx_debug_front).

body                                          variant                                       cluster / group counts it sees
k_front's own dispatch and ring ranking       FX_FRONT_STREAM=0 / 1, FX_FRONT_SPLIT=1 / 2    16 .. 192 a ring (wavefront forms), 193, 249,
                                                                                            256, 283, 300 (one lane); adjoining rings
cc_order in merge_body inside k_front         the same                                      17 .. 257 groups, up to 512 candidates
cc_order<64> in k_rings_runs                  FX_FRONT=0, 16 rings                          up to 128 a ring
cc_order<64> in k_rings_runs2                 FX_FRONT=0, 32 rings                          129 .. 256 a ring: sort_partition_wave<3>, <4>
cc_order in ring_body, LDS: k_rings_large     FX_FRONT=0 (beyond the run tiers)             129 .. 1000 (16 rings), 257 .. 1000 (32)
cc_order in ring_body, LDS: k_front_redo      FX_FRONT_FORCE=1                              every ring scene
cc_order in ring_body, GS: k_slow             FX_FRONT_FORCE=2                              every ring scene
cc_order in merge_body: k_merge_small         FX_FRONT=0                                    17 .. 257 groups, up to 512 candidates
                        k_merge_big           FX_FRONT=0                                    17 .. 600 groups, 567 .. 2550 candidates
                        k_merge_huge          FX_FRONT=0, FX_MERGE_BIG_CAP=64               the same
                        k_slow (GS)           + FX_MERGE_HUGE_CAP=128, and FX_FRONT_FORCE=2  the same
                        k_front_redo          FX_FRONT_FORCE=1                              every merge scene
the product library, no hook                  batches of nine and more, and of up to eight   every scene

The largest adversary (a sequence that spends introsort's depth budget, with ties: sort_scenes_util.adversary) per body:
k_front's ring dispatch 283 clusters (its wavefront forms: 175); merge_body inside k_front and k_merge_small 40 groups — 420
candidates; no adversary of 65 groups or more fits their 512 candidates, the forms beyond <1> see one only under the hook test
of tests/test_sort_replay.py —; k_rings_runs 65 (128 segments hold no larger one), k_rings_runs2 249, ring_body in k_front_redo 249 (its LDS image does not
hold the returns of the 283-cluster one), in k_rings_large and k_slow 283 clusters; k_merge_big, k_merge_huge, k_slow and
k_front_redo's merge 283 groups."""
import ctypes as C

import pytest

from feature_extraction_amd import capi
from tests import sort_scenes_util as ss
from tests import util

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle_of(oracle, sc):
    key = (sc["name"], sc["group"])
    if key not in _ORACLE:
        _ORACLE[key] = oracle.run(ss.params(sc["group"]), sc["scan"])
    return _ORACLE[key]


def _state(ctx):
    h, cnt = (C.c_uint32 * 8)(), (C.c_uint32 * 16)()
    ctx.lib.fx_debug_tier_hints.argtypes = [C.c_void_p, C.c_void_p]
    ctx.lib.fx_debug_counters.argtypes = [C.c_void_p, C.c_void_p]
    ctx.lib.fx_debug_front.argtypes = [C.c_void_p]
    ctx.lib.fx_debug_front.restype = C.c_int
    capi.check(ctx.lib.fx_debug_tier_hints(ctx.handle, h))
    capi.check(ctx.lib.fx_debug_counters(ctx.handle, cnt))
    return [int(v) for v in h], [int(v) for v in cnt], int(ctx.lib.fx_debug_front(ctx.handle))


def _batch(oracle, ctx, scenes, tag):
    got = ctx.process_host([s["scan"] for s in scenes])
    state = _state(ctx)
    print(f"{tag}: {len(scenes)} scans, hints {state[0]}, counters {state[1][:8]}, front {state[2]}")
    for g, sc in zip(got, scenes):
        ss.check(g, sc, tag=f"{tag}: ")
        util.compare_scan(g, _oracle_of(oracle, sc), tag=f"{tag}: {sc['name']}")
    return state


def _run(oracle, group, scenes, tag):
    ctx = capi.Context(ss.params(group), ss.limits(len(scenes)))
    try:
        return _batch(oracle, ctx, scenes, f"{tag}, {group}")
    finally:
        ctx.close()


def _run_tier_holds(sizes, S, RN):
    """A ring of single-run clusters in a run tier of S segments and RN runs (ring_runs_body): a run of m returns is
    ceil(m / seg_len) segments, seg_len = max(8, ceil(n / (3 S / 4))) for the ring's n returns."""
    n = int(sizes.sum())
    seg_len = max(8, -(-n // (S * 3 // 4)))
    return len(sizes) <= RN and sum(-(-int(m) // seg_len) for m in sizes) <= S


def _rings_handed_on(scenes):
    """(rings the first run tier — 128 segments, 128 runs — does not hold, those of them that the second — 384, 256 — does not)."""
    rings = [s for sc in scenes for s in sc["rings"].values()]
    first = [s for s in rings if not _run_tier_holds(s, 128, 128)]
    return len(first), sum(1 for s in first if not _run_tier_holds(s, 384, 256))


def _ring(scenes, name, count):
    return next(s for s in next(sc for sc in scenes if sc["name"] == name)["rings"].values() if len(s) == count)


FRONT_VARIANTS = {"fused": dict(FX_FRONT_STREAM=0), "streamed": dict(FX_FRONT_STREAM=1), "two launches": dict(FX_FRONT_SPLIT=1),
                  "two launches, lean": dict(FX_FRONT_SPLIT=2)}


@pytest.mark.parametrize("variant", list(FRONT_VARIANTS))
def test_the_front_kernels_own_dispatch_and_its_merge(fx_hooks, oracle, variant):
    """k_front in its shapes: a ring per wavefront (sort_partition_wave<1 .. 3> up to 192 clusters, one lane beyond), the
    ranking ring by ring in ranges that border one another (prefix_owner), and cc_order in its merge.  Nothing is handed on.
    Largest adversary: 283 clusters a ring (one lane), 175 (a wavefront), 40 groups in the merge (420 of its 512 candidates)."""
    fx_hooks(**FRONT_VARIANTS[variant])
    for group, scenes in (("ring16", [s for s in ss.ring_scenes("ring16") if s["front"]]), ("ring32", [s for s in ss.ring_scenes("ring32") if s["front"]]),
                          ("merge", [s for s in ss.merge_scenes() if s["small"]])):
        hints, _, front = _run(oracle, group, scenes, variant)
        assert front == 1 and (hints[6], hints[7]) == (0, 0), f"{variant}, {group}: front {front}, hints {hints}"


# ring scenes whose every ring fits k_front_redo's LDS image (the rings of 1000 clusters, of 283 and of the 100- and 175-cluster
# adversaries — 1500 returns and more — do not: they go on to k_slow)
REDO_LDS = ("rings 16 17 64 65 128 129", "rings 17 192 193", "rings 256 40 equal", "rings 100 300", "rings anti 65 249", "rings 16 .. 193")


@pytest.mark.parametrize("force", [1, 2])
def test_the_kernels_behind_the_front_kernel(fx_hooks, oracle, force):
    """FX_FRONT_FORCE=1: every scan through k_front_redo — cc_order<512> in ring_body (LDS) and in merge_body; a ring that its LDS
    image does not hold goes on to k_slow: the scenes of REDO_LDS stay (rings of 193, 249 and 256 clusters: sort_partition_wave<4>,
    of 300: one lane; largest adversary 249) —; 2: every ring and merge through k_slow, cc_order<256, GS> on HBM scratch
    (largest adversary: 283 clusters a ring, 283 groups a merge, as in k_front_redo's merge)."""
    fx_hooks(FX_FRONT_FORCE=force)
    rings = ss.ring_scenes("ring16")
    stay = [s for s in rings if s["name"] in REDO_LDS]
    assert len(stay) == len(REDO_LDS)
    for group, scenes, slow in (("ring16", stay, 0), ("ring16", [s for s in rings if s["name"] not in REDO_LDS], None), ("merge", ss.merge_scenes(), None)):
        B = len(scenes)
        hints, _, front = _run(oracle, group, scenes, f"forced {force}")
        want = B if force == 2 else slow
        assert front == 1 and hints[6] == B and (want is None or hints[7] == want), f"forced {force}, {group}: front {front}, hints {hints}, {B} scans"


@pytest.mark.parametrize("group", ["ring16", "ring32"])
def test_the_separate_ring_kernels(fx_hooks, oracle, group):
    """FX_FRONT=0.  16 rings: k_rings_runs (cc_order<64>, up to 128 runs and 128 segments: sort_partition_wave<1>, <2>; largest
    adversary 65), the rings beyond it in k_rings_large (cc_order<1024>, LDS: 100 .. 1000 clusters; largest adversary 283).
    32 rings: what the first run tier hands on and 256 runs and 384 segments hold in k_rings_runs2 (cc_order<64>:
    sort_partition_wave<2>, <3>, <4>; adversaries 100, 175, 249), the rest (257 .. 1000 clusters; adversary 283) as above."""
    fx_hooks(FX_FRONT=0)
    scenes = ss.ring_scenes(group)
    _, cnt, front = _run(oracle, group, scenes, "separate")
    first, second = _rings_handed_on(scenes)
    assert first >= 11 and second >= 4 and first - second >= 7
    # what the docstring claims each run tier sees, by the statement of what it holds
    assert _run_tier_holds(_ring(scenes, "rings anti 65 249", 65), 128, 128) and _run_tier_holds(_ring(scenes, "rings 16 17 64 65 128 129", 128), 128, 128)
    assert not _run_tier_holds(_ring(scenes, "rings anti 40 100", 100), 128, 128)
    for name, count in (("rings anti 175", 175), ("rings anti 65 249", 249), ("rings 17 192 193", 193), ("rings 256 40 equal", 256)):
        assert not _run_tier_holds(_ring(scenes, name, count), 128, 128) and _run_tier_holds(_ring(scenes, name, count), 384, 256), name
    want = (first, second) if group == "ring32" else (0, first)
    assert front == 0 and (cnt[0], cnt[5]) == want, f"separate, {group}: counters {cnt[:8]}, expected {want}"


@pytest.mark.parametrize("tier", ["small and big", "huge", "slow"])
def test_the_separate_merge_kernels(fx_hooks, oracle, tier):
    """FX_FRONT=0: up to 512 candidates in k_merge_small (cc_order<256>), more in k_merge_big (cc_order<1024>); the hooks lower
    that tier's capacity to hand its scans on to k_merge_huge, and that one's to hand them on to k_slow (GS).  Largest adversary:
    40 groups in k_merge_small (420 candidates), 283 in the others."""
    fx_hooks(**{"small and big": dict(FX_FRONT=0), "huge": dict(FX_FRONT=0, FX_MERGE_BIG_CAP=64),
                "slow": dict(FX_FRONT=0, FX_MERGE_BIG_CAP=64, FX_MERGE_HUGE_CAP=128)}[tier])
    scenes = ss.merge_scenes()
    hints, _, front = _run(oracle, "merge", scenes, f"merge {tier}")
    big = sum(1 for s in scenes if not s["small"])
    assert big >= 12 and len(scenes) - big >= 9
    want = {"small and big": (big, 0, 0), "huge": (big, big, 0), "slow": (big, big, big)}[tier]
    assert front == 0 and (hints[2], hints[3], hints[7]) == want, f"merge {tier}: hints {hints}, expected {want}"


def test_the_product_library_in_batches_of_nine_and_of_fewer(fxlib, oracle):
    """No hooks: what the product chooses for itself — and whatever that is, the tables hold."""
    for group, scenes in (("ring16", ss.ring_scenes("ring16")), ("merge", ss.merge_scenes())):
        assert len(scenes) >= 9
        ctx = capi.Context(ss.params(group), ss.limits(len(scenes)))
        try:
            for part, tag in ((scenes, "product"), (scenes[:8][::-1], "product, up to eight")):
                _batch(oracle, ctx, part, f"{tag}, {group}")
        finally:
            ctx.close()
