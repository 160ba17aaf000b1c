"""CPU checks of the front path's edge scenes (tests/front_edges_util.py): what makes tests/test_gpu_front_edges.py able to fail.
Every gate scene sits on the floats it claims, by the plain statements; the oracle gives every scene's hand-stated table and the
pinned centroid bits; the twins of a family really differ; the filter's limits lie on the side where float and double disagree;
the fillers push their scenes into the intended tier and leave the scene's own clusters alone."""
import collections
import functools

import numpy as np

from tests import front_edges_util as fe
from tests import util


@functools.lru_cache(maxsize=None)
def _oracle_of(name):
    from oracle import oracle_py
    sc = _by_name()[name]
    return oracle_py.run(fe.params(sc["group"]), sc["scan"], roll=sc["roll"], pitch=sc["pitch"])


@functools.lru_cache(maxsize=None)
def _by_name():
    scenes = fe.all_scenes() + [s for kind in fe.TIERS for s in fe.tier_scenes(kind)]
    have = {s["name"] for s in scenes}
    for s in list(scenes):  # (the scenes under another group's parameters that ride with a filler)
        if "base" in s and s["base"]["name"] not in have:
            scenes.append(s["base"])
            have.add(s["base"]["name"])
    names = [s["name"] for s in scenes]
    assert len(set(names)) == len(names)
    return {s["name"]: s for s in scenes}


def _outcome(name):
    o = _oracle_of(name)
    return (o["cand_size"].tolist(), o["kp_size"].tolist(), util.bits(o["candidates"]).tolist(), util.bits(o["keypoints"]).tolist())


def test_gates_reach_their_three_floats(oracle):
    n = 0
    for sc in fe.all_scenes():
        for claim, got, want in fe.reached(sc):
            assert util.bits(got) == util.bits(want), f"{sc['name']}: {claim} is {got!r}, the scene claims {want!r}"
            n += 1
    assert n > 250
    # every family probes its gates at all three floats; only the diagonal boxes of family D straddle instead
    kinds = collections.defaultdict(set)
    for sc in fe.all_scenes():
        assert not sc["straddle"] or sc["name"].startswith("D diagonal"), f"{sc['name']} falls back to the straddle"
        if sc.get("twin") and sc["twin"][1] in fe.KINDS:
            kinds[(sc["twin"][0], sc["group"])].add(sc["twin"][1])
    assert len(kinds) >= 3 * 13 + 2 + 4 * 7
    for key, have in kinds.items():
        assert have == set(fe.KINDS), f"{key}: only {sorted(have)} reached"
    tol_b = {sc["name"] for sc in fe.family_b()}
    for tol in (1.0, 0.65, 0.1):
        for place in fe.PLACES:
            for d in fe.DIRS:
                for order in ("consecutive", "split"):
                    for kind in fe.KINDS:
                        assert f"B {tol} {place} {d} {order} {kind}" in tol_b
    assert fe.r2_of(1.0) == 1.0 and fe.r2_of(0.1) != np.float32(0.01) and fe.r2_of(0.2) == np.float32(0.040000003)


def test_the_oracle_gives_every_table_and_the_pinned_bits(oracle):
    ruled = 0
    for name, sc in _by_name().items():
        fe.check_expect(_oracle_of(name), sc, tag="oracle: ")
        ruled += bool(sc["expect"].get("oracle_rules"))
    # the pinned centroids: 0x1.000000p-4 with the tiny terms last, 0x1.000002p-4 with them first, in candidates and keypoints
    for q, x in fe.QUAD_X_BITS.items():
        for runs in (1, 2, 3):
            assert int(util.bits(_oracle_of(f"E {q} {runs} runs")["candidates"])[0, 0]) == x
        o = _oracle_of(f"E {q} merged")
        assert int(util.bits(o["keypoints"])[0, 0]) == x and o["kp_size"].tolist() == [4]
        assert util.bits(o["keypoints"])[0, 3] == util.bits(o["candidates"])[0, 3]  # the lowest candidate's elevation
    assert float.fromhex("0x1.000000p-4") == np.uint32(0x3d800000).view(np.float32) and float.fromhex("0x1.000002p-4") == np.uint32(0x3d800001).view(np.float32)
    # the elevation statement is the oracle's, bit for bit, on every point the scenes use
    for sc in fe.all_scenes():
        if sc["roll"] == 0.0:
            for p in sc["scan"]:
                if np.isfinite(p[:3]).all():
                    a, b = fe.elevation(*p[:3]), np.float32(oracle.load().fxo_elevation_deg(*[float(v) for v in p[:3]]))
                    assert util.bits(a) == util.bits(b) or (a == 0 and b == 0), f"{sc['name']}: elevation of {p[:3]}: {a!r} vs {b!r}"


def test_the_twins_of_every_family_differ(oracle):
    twins = collections.defaultdict(dict)
    for sc in _by_name().values():
        if sc.get("twin") and "base" not in sc:
            twins[(sc["twin"][0], sc["group"])][sc["twin"][1]] = sc["name"]
    assert len(twins) > 70
    for key, t in twins.items():
        if "below" in t and "at" in t:
            assert _outcome(t["below"]) != _outcome(t["at"]), f"{key}: below the gate and at it give one outcome"
            assert _outcome(t["at"])[:2] == _outcome(t["above"])[:2], f"{key}: at the gate and above it differ"
        else:
            assert len({repr(_outcome(n)) for n in t.values()}) > 1, f"{key}: all of {sorted(t)} give one outcome"
    for q in ("E 1 runs", "E 2 runs", "E 3 runs", "E merged"):
        t = twins[(q, "launch")]
        assert _outcome(t["tiny first"]) != _outcome(t["tiny last"])
    for key, t in twins.items():
        if key[0].startswith("D box"):
            assert _outcome(t["1000.25"])[0] == [2] and _outcome(t["1001"])[0] == [] and _outcome(t["1000"])[0] == [2]
        if key[0].startswith("F chain"):  # secondary_max
            assert _outcome(t["16"])[1] == [16] and _outcome(t["17"])[1] == []
        if key[0].startswith("F ") and "below" in t:  # number_detection_channels = 2: a group of ndc against two of ndc - 1
            assert _outcome(t["below"])[1] == [2] and _outcome(t["at"])[1] == []
    t = twins[("D dyadic", "dyadic")]
    assert _outcome(t["exact"])[0] == [] and _outcome(t["below x"])[0] == [2] and _outcome(t["below y"])[0] == [2] and _outcome(t["above x"])[0] == []
    # per-run partial sums would give the tiny-first value for both orders (the statement, on the split scenes' runs)
    xs = np.array(fe.QUADS["tiny last"])
    for cut in ((1,), (1, 2)):
        parts = np.split(xs, cut)
        assert fe.bits4([fe.seq_sum([fe.seq_sum(p) for p in parts]) / 4.0])[0] == fe.QUAD_X_BITS["tiny first"]


def test_the_limits_of_the_faces_lie_where_float_and_double_disagree(oracle):
    sides = fe.side_of_the_limits()
    assert len(sides) == 6
    for lim, as_float, double_drops in sides:
        assert as_float != lim and double_drops, f"limit {lim}: its float {as_float!r} is not outside it"
    for name in ("A faces forwards", "A faces backwards", "A faces rotated forwards", "A faces rotated backwards"):
        sc = _by_name()[name]
        lim = fe._face_limits("faces")
        M = sc.get("rotation")
        on_face = 0
        for kind, i, axis, v in sc["reach"]:
            lo, hi = lim[axis]
            if v in (fe.narrow(lo), fe.narrow(hi)):  # ON the face: float keeps it, double would drop it
                on_face += 1
                assert fe.face_keeps(v, lo, hi) and (float(v) < lo or float(v) > hi)
                assert i in sc["expect"]["kept"]
        assert on_face == 6
        assert len(sc["scan"]) == 27 and int(np.isnan(sc["scan"]).any(axis=1).sum()) == 3 and int(np.isinf(sc["scan"]).any(axis=1).sum()) == 6
        assert sc["expect"]["kept"] == sorted(sc["expect"]["kept"])
        o = _oracle_of(name)
        rot = sc["scan"][:, :3] if M is None else np.stack([fe.rotate_row(M, 3 * k, *sc["scan"][:, :3].T) for k in range(3)], axis=1)
        util.assert_bit_equal(o["filtered"][:, :3], rot[sc["expect"]["kept"]], f"{name}: the filtered cloud in input order")
    assert fe.narrow(1e39) == np.inf and fe.narrow(-1e39) == -np.inf


def test_ring_windows_of_the_non_dyadic_step(oracle):
    kinds = fe.g_borders()
    assert sum(len(v) for v in kinds.values()) == fe.G_RINGS - 1
    scenes = {s["name"].split()[1]: s for s in fe.family_g()}
    assert set(scenes) == {k for k, v in kinds.items() if v} and scenes
    for kind, sc in scenes.items():
        e0, e1 = sc["window_ends"]
        want = {"meet": [1, 1, 2, 1, 1], "overlap": [1, 1, 2, 2, 1, 1], "gap": [1, 1, 1, 1, 1, 1]}[kind]
        assert sc["held"] == want, f"{kind}: the elevations around the border are held by {sc['held']} windows"
        assert (e0 == e1) == (kind == "meet")


def test_the_fillers_reach_their_tiers_and_leave_the_scenes_alone(oracle):
    for kind, (group, _, (lo, hi), more_than) in fe.TIERS.items():
        scenes = fe.tier_scenes(kind)
        assert len(scenes) >= 10
        window = (0.5, 1.5) if group == "r32" else (0.0, 2.0)
        for sc in scenes:
            base, n0 = sc["base"], len(sc["base"]["scan"])
            o, o0 = _oracle_of(sc["name"]), _oracle_of(base["name"])
            fe.check_expect(o, sc, tag=f"{kind}: ")
            if kind != "merge":
                runs = fe.ring_runs(sc, *window)
                assert lo <= runs <= hi, f"{sc['name']}: {runs} runs on the scene's ring, the tier is for {lo} .. {hi}"
                assert int((o["cand_size"] == 1).sum()) >= lo - 3  # single-return clusters, a candidate each
            assert len(o["candidates"]) > more_than, f"{sc['name']}: {len(o['candidates'])} candidates"
            # the filler stays clear of the scene: of its tolerance, its merge radius and its merge cells' neighbourhood
            d = np.hypot(sc["scan"][n0:, None, 0] - sc["scan"][None, :n0, 0], sc["scan"][n0:, None, 1] - sc["scan"][None, :n0, 1])
            assert d.min() > 3 * fe.MERGE_W, f"{sc['name']}: a filler return {d.min():.3f} m from the scene"
            # and the scene's own clusters and keypoints are those of the scene alone
            rows = {tuple(r) for r in util.bits(o["candidates"]).tolist()}
            assert all(tuple(r) in rows for r in util.bits(o0["candidates"]).tolist()), f"{sc['name']}: the scene's candidates changed"
            util.assert_bit_equal(o["keypoints"], o0["keypoints"], f"{sc['name']}: keypoints")
            util.assert_bit_equal(o["kp_size"], o0["kp_size"], f"{sc['name']}: keypoint sizes")
    # the straddled borders of the merge grid: the two candidates lie in different cells of the axis named, with x_min / y_min = 0 / -50
    seen = set()
    for sc in fe.family_f():
        if sc.get("border"):
            a, b = sc["scan"][0], sc["scan"][1]
            dx, dy = fe.cell(b[0], 0.0) - fe.cell(a[0], 0.0), fe.cell(b[1], -50.0) - fe.cell(a[1], -50.0)
            assert (dx, dy) == {"x": (1, 0), "y": (0, 1), "xy": (1, 1)}[sc["border"]], f"{sc['name']}: cell steps {(dx, dy)}"
            seen.add(sc["border"])
    assert seen == {"x", "y", "xy"}
    # measured from -4e6 some pair below the gate would be TWO cells apart (what the group "tol01_4e6" can catch); from 0 none is
    apart = {org: max(abs(fe.cell(sc["scan"][1][k], org) - fe.cell(sc["scan"][0][k], org)) for sc in fe.family_f()
                      if sc.get("twin", ("", ""))[1] == "below" for k in (0, 1)) for org in (-4.0e6, 0.0)}
    assert apart == {-4.0e6: 2, 0.0: 1}, apart
    with np.errstate(over="ignore", invalid="ignore"):  # and under x_min = -1e30 / -inf every coordinate is in one cell
        assert {fe.cell(v, -1e30) for v in (0.0, 10.0, 99.0)} == {fe.cell(0.0, -1e30)}
