"""The descriptor's decisions at the floats where they flip, in every tier: the neighbour gate, the skip rule, the radial shells,
the elevation and azimuth bins (sc3d_bin<true>'s near-edge hand-over to the exact angles, the 360 - phi mirror, atan2(0, 0)
straight above and below the keypoint) and the density gate with the prefilters in front of it (the list tier's 12^3 grid, the
dense tier's cells).  The probes and their stated tables are tests/desc_edges_util.py's; that every probe reaches its
float and that the oracle's rows are the numpy statement's is checked on the CPU by tests/test_desc_edges_scenes.py.

Every pack runs at the smallest support counts that reach each body: 12 / 16 (4 lanes a row), 17 / 32 (8), 33 / 64 (16), 65 / 192
(one wavefront), 193 / 300 (the list tier and its grid), 40 support points under max_neighbors = 32 (the overflowed-list route:
the dense kernels and dense_slow_loop), 1025 (a true dense row) and, for the dense grid's pairs alone, 20 000 (pairs in two target
windows of k_dense_density).  The radial and density families run once more at R = 0.5 m ("xr").  Twice a context.  Device row == numpy statement == oracle, every word; a failure
names family, pack, tier and the expected and found value of the bins that differ, with the probes stated there."""
import numpy as np
import pytest

from feature_extraction_amd import build, capi
from tests import desc_edges_util as eu
from tests import desc_rows_util as rows

pytestmark = pytest.mark.gpu
KINDS = ("x", "ztop", "zbot", "f", "z0", "xr")
SUPPORT = (12, 16, 17, 32, 33, 64, 65, 192, 193, 300)
# (R = 0.5 m, "xr": the pole's own twelve points are support points, a pack of twelve makes 24: its rows start at 32)
CASES = [(kind, support) for kind in KINDS for support in SUPPORT if not (kind == "xr" and support < 32)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(kind, support, tag, reps=2, list_cap=rows.LIST_CAP, skip_epsilon=False, compare=True, state=False, **lim):
    """The kind's scenes at `support` support points a row as one batch, `reps` times through one context.  Returns (rows per
    group class, dense rows, the last batch's results — or, with `state` (the test build), what the support gather left)."""
    p, scenes = eu.scenes(kind, support)
    scans = [s for s, _, _ in scenes]
    ctx = capi.Context(p, capi.limits(len(scans), max(1024, 1 << max(len(s) for s in scans).bit_length()), **lim))
    try:
        for rep in range(reps):
            got = ctx.process_host(scans)
            for b, (scan, ora, where) in enumerate(scenes):
                if not compare:
                    continue
                for pole, what, pr, first in where:
                    st = eu.statement(scan[:, :3], pole.kp, pole.xa, pole.radius, skip_epsilon)
                    eu.check_row(pole, what, pr, first, scan, st, tag, skip_epsilon)
                    k = pole.ordinal
                    here = (f"{tag}, batch {rep}, scan {b}, family {eu.FAMILIES[what]} (pack {what}), {support} support points, "
                            f"{rows.tier_of(support, list_cap)} tier")
                    assert (_bits(got[b]["keypoints"][k, :3]) == _bits(pole.kp)).all(), here
                    assert int(got[b]["kp_neighbors"][k]) == st["n_nbr"], f"{here}: kp_neighbors {got[b]['kp_neighbors'][k]}, stated {st['n_nbr']}"
                    dev = got[b]["descriptors"][k]
                    if (_bits(dev[:1980]) != _bits(st["desc"])).any():
                        raise AssertionError(eu.explain(pole, what, pr, first, scan, dev, st["desc"], here))
                    assert not dev[1980:].any(), here
                if not skip_epsilon:
                    rows.compare(got[b], ora, f"{tag}, batch {rep}, scan {b}", scan=scan, radius=eu.KINDS[kind][1], list_cap=list_cap)
        return eu.group_class_counts(ctx), eu.dense_row_count(ctx), ctx.gather_state() if state else got
    finally:
        ctx.close()


def _n_rows(kind):
    return sum(len(row) for row in eu.packs(kind)[1])


@pytest.mark.parametrize("kind,support", CASES)
def test_every_family_in_the_group_wave_and_list_tiers(fxlib, kind, support):
    classes, dense, _ = _run(kind, support, f"{kind} scenes")
    want = [0, 0, 0]
    if eu.size_class(support) is not None:
        want[eu.size_class(support)] = _n_rows(kind)
    assert classes == want and dense == 0, f"{kind}, {support} support points: group rows per class {classes}, dense rows {dense}"


@pytest.mark.parametrize("kind", ["x", "xr"])
@pytest.mark.parametrize("support", [64, 65, 192, 193])
def test_the_tier_that_ran_and_the_constants_it_used(fx_hooks, kind, support):
    """The product library reports group classes and dense rows; which of the wave and the list tier took a row only the test
    build's gather state tells (its work lists): 64 | 65 and 192 | 193 support points.  The same state reports the library's
    r2_support and r2_search: they are the values tests/desc_edges_util.py restates (what the CPU proof about the margins rests
    on), at R = 0.05 and at R = 0.5 m."""
    fx_hooks()
    classes, dense, st = _run(kind, support, f"{kind} scenes, test build", reps=1, state=True)
    n = _n_rows(kind)
    want = (sum(classes), st["n_wave"], st["n_list"], dense)
    assert want == ((n, 0, 0, 0) if support <= 64 else (0, n, 0, 0) if support <= 192 else (0, 0, n, 0)), f"(group, wave, list, dense) rows {want}"
    radius = eu.KINDS[kind][1]
    rs = (radius + radius / 5.0) * 1.0001 + 1e-4
    assert _bits(st["r2_support"]) == _bits(np.float32(rs * rs)) and _bits(st["r2_search"]) == _bits(eu.gates(radius)[0])


@pytest.mark.parametrize("slow", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_every_family_on_the_overflowed_list_route(fx_hooks, kind, slow):
    """max_neighbors = 32 and 40 support points a row: every row overflows its list and goes to the dense tier — its three
    kernels (FX_DENSE_SLOW=0) and dense_slow_loop on scratch (=1)."""
    fx_hooks(FX_DENSE_SLOW=slow)
    _, dense, _ = _run(kind, 40, f"{kind} scenes, max_neighbors=32, FX_DENSE_SLOW={slow}", list_cap=32, max_neighbors=32)
    assert dense == _n_rows(kind)


@pytest.mark.parametrize("slow", [0, 1])
@pytest.mark.parametrize("kind", ["x", "ztop", "xr"])
def test_families_a_b_c_g_in_a_true_dense_row(fx_hooks, kind, slow):
    """1025 support points a row: radial, elevation, gate and density packs ("x", and "xr" at R = 0.5 m where dense_grid's cell
    width comes from the density radius: among them the pairs two cells apart in x and y and one layer apart in z, the x pair
    along x to within 0.7 degrees at the float below the gate and on it) and the azimuth packs ("ztop").  A row of 1025 has one
    target window: no pair spans two."""
    fx_hooks(FX_DENSE_SLOW=slow)
    _, dense, _ = _run(kind, 1025, f"{kind} scenes, dense rows, FX_DENSE_SLOW={slow}", reps=2)
    assert dense == _n_rows(kind)


@pytest.mark.parametrize("slow", [0, 1])
def test_density_pairs_in_two_target_windows(fx_hooks, slow):
    """One row of 20 000 support points with the dense grid's pairs: k_dense_density passes its work item's targets through LDS in
    five windows of 2048, and the two z pairs (mutual d2 below the gate: counted; on it: not) have the query's own cell wholly
    in one window and its partner's wholly in the next (tests/test_desc_edges_scenes.py restates the concatenation and asserts
    it): a count made of two windows' parts."""
    fx_hooks(FX_DENSE_SLOW=slow)
    _, dense, _ = _run("xw", eu.WINDOW_SUPPORT, f"the dense pairs in {eu.WINDOW_SUPPORT} support points, FX_DENSE_SLOW={slow}", reps=2)
    assert dense == 1


@pytest.mark.parametrize("support", [16, 64, 192, 300])
@pytest.mark.parametrize("kind", ["f", "z0"])
def test_skip_rule_under_the_epsilon_build(fxlib, kind, support):
    """Family F through -DFX_SKIP_EPSILON: exactly the probes with d2 in [FLT_MIN, FLT_EPSILON) move from binned to skipped
    (tests/test_desc_edges_scenes.py states which), and the row is the statement's under that reading."""
    eu.with_library(build.build_skip_epsilon(), lambda: _run(kind, support, f"{kind} scenes, FLT_EPSILON reading", skip_epsilon=True))


def test_the_gate_probe_in_the_stored_list(fx_hooks):
    """Family E through the support gather's own state (the test build): the probes with d2 below, on and above r2_search are all
    support points of their row; the one below the gate — the last point of the scan — is the last entry of the stored list;
    kp_neighbors counts the two probes below the gate and nothing else.
    The ORDER of a stored list is no contract of the gather (tests/test_gpu_gather_sets.py compares sets): the last entry being
    the scan's last point rests on this scan of some 150 points lying in one wavefront's stride, whose hits are appended in
    lane order.  A gather that stores another order is not wrong; this assertion then has to name the new position."""
    fx_hooks()
    p, scenes = eu.scenes("x", 16)
    b, (scan, ora, where) = next((b, sc) for b, sc in enumerate(scenes) if any(w == "E" for _, w, _, _ in sc[2]))
    pole, what, pr, first = next(x for x in where if x[1] == "E")
    at = {q["name"]: eu.probe_index("x", pr, first, i) for i, q in enumerate(pr)}
    assert at["E1below"] == len(scan) - 1
    ctx = capi.Context(p, capi.limits(len(scenes), 1024))
    try:
        got = ctx.process_host([s for s, _, _ in scenes])
        st = ctx.gather_state()
    finally:
        ctx.close()
    row = int(np.flatnonzero((st["row_map"][:, 0] == b) & (st["row_map"][:, 1] == pole.ordinal))[0])
    cnt = int(st["s_cnt"][row])
    idx = st["s_pts"][row, :cnt, 3].copy().view(np.uint32).astype(np.int64)
    assert cnt == 16 and set(at.values()) <= set(idx.tolist()), f"stored list {idx.tolist()}, the gate probes {at}"
    assert int(idx[-1]) == at["E1below"], f"the last stored entry is point {int(idx[-1])}, the probe below the gate is {at['E1below']}"
    assert int(got[b]["kp_neighbors"][pole.ordinal]) == 2


@pytest.mark.parametrize("kind", ["x", "ztop"])
def test_literal_trig_build_on_the_edges(fxlib, kind, capsys):
    """Families B and C through -DFX_TRIG_LITERAL_F32 (the device's atan2f / acosf, no exact re-evaluation): how many rows and
    words that build moves on these probes is printed, not asserted — it is the device libm's property."""
    _, _, ref = _run(kind, 16, "product", reps=1)
    _, _, lit = eu.with_library(build.build_trig_literal(), lambda: _run(kind, 16, "literal trig", reps=1, compare=False))
    words = sum(int((_bits(a["descriptors"]) != _bits(b["descriptors"])).sum()) for a, b in zip(ref, lit))
    moved = sum(int((_bits(a["descriptors"]) != _bits(b["descriptors"])).any(axis=1).sum()) for a, b in zip(ref, lit))
    with capsys.disabled():
        print(f"\nliteral fp32 trig on the {kind} edge scenes: {words} words in {moved} rows differ from the product's")
