"""What makes the cases of tests/test_gpu_gather_sets.py able to fail, checked without a GPU: every probe sits at the scan index
it claims and belongs to the keypoint it claims, the gates' three floats are reached, every scene gives the intended keypoints
in the oracle, the reference (tests/gather_util.py) agrees with the oracle where both speak — neighbour counts — and contains
the float64 brute-force support sets, and the sparse scans ARE sparse, so that their near-sector bits stay informative."""
import os

import numpy as np
import pytest

from tests import desc_rows_util as du
from tests import gather_util as gu
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"edges": 4, "edges_quad": 4, "short1": 4, "short3": 4, "burst": 1, "all_near": 4, "no_keypoints": 0, "one_keypoint": 1,
          "equal_x": 2, "gate_support": 4, "gate_search_eq": 4, "gate_search_below": 4, "faces": 4, "spread": 40, "crowded": 965,
          "shared": 3, "corner": 1, "zface": 1}


@pytest.mark.parametrize("name", list(SCENES) + ["many", "many_thin"])
def test_reference_agrees_with_the_oracle_and_with_float64(oracle, name):
    s = gu.built(name)
    ora, ref = s["ora"], s["ref"]
    if name in SCENES:
        assert ora["n_keypoints"] == SCENES[name]
    else:
        assert ora["n_keypoints"] > 2300
    assert len(ref.kp) == ora["n_keypoints"]
    if not len(ref.kp):
        return
    util.assert_bit_equal(ref.n_nbr.astype(np.uint32), ora["kp_neighbors"].astype(np.uint32), f"{name}: neighbours, reference against oracle")
    radius = float(s["p"].descriptor_radius)
    r_oracle = radius + radius / 5
    assert r_oracle * r_oracle < float(ref.r2_support)
    rot = ref.rot.astype(np.float64)
    fin = np.isfinite(rot).all(axis=1)
    for k in range(0, len(ref.kp), max(1, len(ref.kp) // 64)):  # (every keypoint of the small scenes, a sample of the large ones)
        d2 = ((rot - ref.kp[k].astype(np.float64)) ** 2).sum(axis=1)
        inside = np.flatnonzero(fin & (d2 < r_oracle * r_oracle))
        lost = np.setdiff1d(inside, ref.sets[k])
        assert len(lost) == 0, f"{name}: keypoint {k}: point {lost[:1]} is within the oracle's radius and not in the reference's set"


@pytest.mark.parametrize("name", ["edges", "edges_quad", "short1", "short3", "burst"])
def test_probes_sit_where_they_claim(oracle, name):
    s = gu.built(name)
    ref, probes, owner = s["ref"], s["probes"], s["owner"]
    # keypoint of pole j: the one nearest D * axis
    kp_of = [int(np.argmin(np.abs(ref.kp[:, :2] - gu.D * np.array(a)).sum(axis=1))) for a in du.AXES]
    for k, want in enumerate(ref.sets):
        mine = sorted(i for i in probes if kp_of[owner[i]] == k)
        assert want.tolist() == mine, f"{name}: keypoint {k}'s support set is {want.tolist()[:8]} .., its probes are {mine[:8]} .."
    if name == "edges":
        want = {0, gu.N_LONG - 1} | {e - 1 for e in gu.EDGES} | set(gu.EDGES)
        assert set(probes) == want and len(s["scan"]) == gu.N_LONG == 263000
        sectors = [i // 4 for i in probes]
        assert sorted(sectors) == sorted(list(set(sectors)) + [0])  # each alone in its sector, but for points 0 and 3 (the scan's first, and the one before edge 4)
    if name == "edges_quad":
        assert all({4 * (i // 4) + j for j in range(4)} <= set(probes) for i in gu.edge_probes())
    if name in ("short1", "short3"):
        n = len(s["scan"])
        assert n % 4 == (1 if name == "short1" else 3) and n - 1 in probes and ref.near[-1] and len(ref.near) == (n + 3) // 4
    if name == "burst":
        assert probes == list(range(512, 1536)) and ref.counts().tolist() == [1024]
    # near: exactly the sectors of the probes and of the poles' points
    poles_at = 400 if name.startswith("short") else gu.POLES_AT
    n_poles = len(ref.kp)
    near = {i // 4 for i in probes} | {i // 4 for i in range(poles_at, poles_at + 12 * n_poles)}
    assert set(np.flatnonzero(ref.near).tolist()) == near


@pytest.mark.parametrize("name", ["edges", "edges_quad"])
def test_sparse_scans_are_sparse(oracle, name):
    """A condition, not a measurement: at most 1 % of the sectors of the long scans are near, so a refill that fetched the wrong
    sector words would load other points."""
    near = gu.built(name)["ref"].near
    assert len(near) == 65750 and 0 < near.sum() <= 0.01 * len(near), near.sum()


def test_near_share_of_the_dense_fixture(oracle):
    """For the record: the share of near sectors of the 128 x 2048 golden fixture, the only scan of the suite
    long enough to reach the 64-tile refill before these tests.  Printed, not asserted beyond being a share."""
    name = "dense_128x2048_R2m_launch_seed10.npz"
    p, _, pts, roll, pitch = util.golden_case(np.load(os.path.join(ROOT, "tests", "golden", name)), name)
    ref = gu.Reference(p, pts, np.zeros((0, 4), np.float32), roll, pitch)
    share = float(ref.near.mean())
    print(f"\n{name}: {int(ref.near.sum())} of {len(ref.near)} sectors are near ({100 * share:.1f} %)")
    assert 0.0 < share <= 1.0


def test_gates_reach_their_three_floats(oracle):
    s = gu.built("gate_support")
    ref, at = s["ref"], s["gate_at"]
    r2 = ref.r2_support
    assert [ref.d2(0, i) for i in at] == [np.nextafter(r2, np.float32(0)), r2, np.nextafter(r2, np.float32(1))]
    assert [i in ref.sets[0] for i in at] == [True, False, False]
    eq, below = gu.built("gate_search_eq")["ref"], gu.built("gate_search_below")["ref"]
    assert eq.d2(0, 2001) == eq.r2_search == np.float32(0.05 * 0.05) and below.d2(0, 2001) == np.nextafter(eq.r2_search, np.float32(0))
    assert eq.sets[0].tolist() == [2001] == below.sets[0].tolist()  # the keypoint's only candidate, a support point in both
    assert eq.has_nbr.tolist() == [False, True, True, True] and below.has_nbr.tolist() == [True] * 4
    # ... so the x-axis ordinals of the three keypoints behind it differ between the twins
    assert (np.cumsum(eq.has_nbr) - eq.has_nbr).tolist() == [0, 0, 1, 2] and (np.cumsum(below.has_nbr) - below.has_nbr).tolist() == [0, 1, 2, 3]
    assert gu.built("gate_search_eq")["ora"]["kp_neighbors"].tolist()[0] == 0 and gu.built("gate_search_below")["ora"]["kp_neighbors"].tolist()[0] == 1


def test_faces_scene_has_both_sides_of_every_face(oracle):
    s = gu.built("faces")
    ref, expect = s["ref"], s["expect_near"]
    assert len(expect) == 18 and sum(expect.values()) == 12
    for sector, is_near in expect.items():
        assert bool(ref.near[sector]) == is_near, sector
    # support points beyond the filter's faces, within 1.5 % of the support radius
    rs = gu.support_radius()
    for k in range(4):
        d = np.sqrt(gu.dist2(ref.kp[k], ref.rot[ref.sets[k]]).astype(np.float64))
        assert (d > 0.98 * rs).sum() >= 4 and d.max() < rs


def test_context_memory_scenes(oracle):
    long, short = gu.built("all_near"), gu.built("short3")
    assert long["ref"].near.all() and len(long["scan"]) > 4 * len(short["scan"])
    assert short["ref"].near.mean() < 0.02
    assert gu.built("no_keypoints")["ora"]["n_keypoints"] == 0 and not gu.built("no_keypoints")["ref"].near.any()


def test_thin_and_spread_grids(oracle):
    steps, (ncx, ncy, _, _) = gu.cell_steps(gu.built("one_keypoint")["ref"])
    assert ncx <= 3 and ncy <= 3
    steps, (ncx, ncy, _, _) = gu.cell_steps(gu.built("equal_x")["ref"])
    assert ncx <= 3 and ncy > 16  # one keypoint column (and its margins)
    ref = gu.built("spread")["ref"]
    steps, (ncx, ncy, wx, wy) = gu.cell_steps(ref)
    assert ncx >= 31 and ncy >= 31 and wx > 30 * float(ref.box_margin) and wy > 25 * float(ref.box_margin)  # widened to the grid's limit
    assert {(1, 0), (-1, 0), (0, 1), (0, -1)} <= steps, steps  # rings cross cell borders in all four directions
    assert (ref.counts() >= 24).all()
    assert any(not a and b for a, b in zip(ref.has_nbr[:-1], ref.has_nbr[1:]))  # a keypoint without a neighbour in front of one with


def test_row_classes_follow_the_thresholds():
    want = {0: (0, 0), 16: (0, 0), 17: (0, 1), 32: (0, 1), 33: (0, 2), 64: (0, 2), 65: (1, -1), 192: (1, -1), 193: (2, -1), 1024: (2, -1), 1025: (3, -1)}
    for n, c in want.items():
        assert gu.row_class(n, 4096) == c, n
    assert gu.row_class(256, 256) == (2, -1) and gu.row_class(257, 256) == (3, -1) and gu.row_class(40, 32) == (3, -1)


def _in_sets(ref):
    """How many support sets each point of the scan is in."""
    times = np.zeros(ref.n, np.int64)
    for idx in ref.sets:
        times[idx] += 1
    return times


def test_crowded_and_shared_scenes_crowd_and_share(oracle):
    """Several keypoints in one cell and points in several support sets, below the LDS tables' limit: what the other scenes of the
    one-pass kinds do not have (at most one keypoint a cell, no shared point)."""
    for name in ("edges", "burst", "equal_x", "spread", "faces"):
        ref = gu.built(name)["ref"]
        gu.cell_steps(ref)
        assert ref.max_kp_in_cell == 1 and _in_sets(ref).max() == 1, name
    ref = gu.built("crowded")["ref"]
    gu.cell_steps(ref)
    times = _in_sets(ref)
    assert len(ref.kp) < 2048 and ref.max_kp_in_cell >= 16 and (times >= 3).sum() >= 2000, (ref.max_kp_in_cell, (times >= 3).sum())
    ref = gu.built("shared")["ref"]
    times = _in_sets(ref)
    assert (ref.counts() > 4 * 256).all() and (times >= 2).sum() >= 4000 and (times == 3).sum() >= 600
    hits = np.flatnonzero(times)
    assert hits[0] == 0 and len(hits) >= 5100 and (np.diff(hits[:5100]) == 1).all()  # one burst: consecutive scan points, every one a hit
    # the pools of tests/test_gpu_gather_sets.py::test_dense_row_without_room_in_the_pools: two rows fit 8192 entries, the third does not
    c = ref.counts()
    assert all(gu.row_class(int(n), 1024)[0] == gu.ROW_DENSE for n in c) and c[0] + c[1] <= 8192 < c[0] + c[1] + c[2]


def test_keypoints_at_the_faces(oracle):
    s = gu.built("corner")
    kp, p = s["ref"].kp[0], s["p"]
    assert 0 < p.x_max - kp[0] <= 0.00201 and 0 < p.y_max - kp[1] <= 0.00201
    pts = s["ref"].rot[s["ref"].sets[0]]
    assert ((pts[:, 0] > p.x_max) & (pts[:, 1] > p.y_max)).sum() >= 10  # support points beyond both faces
    s = gu.built("zface")
    kp, p = s["ref"].kp[0], s["p"]
    assert 0 < p.z_max - kp[2] <= 0.002 and p.number_detection_channels == 1
    assert (s["ref"].rot[s["ref"].sets[0]][:, 2] > p.z_max).sum() >= 40
