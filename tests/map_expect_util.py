"""Helpers of the forgetting tests (tests/test_map_expect_reference.py, tests/test_gpu_map_expect.py): the cases of
fx_map_expect and fx_map_retire.  A case is map_observe_util's dict (frags / n_scans_map: a landmark of 2 observations at every
fragment, id = its place in frags; off / rows; loc; ids; edit; opts: what capi.map_expect_reference and Map.expect take) with
"retire": the options of the fx_map_retire that follows, and "repeat": how often the expect is accumulated before it."""
import math

import numpy as np

from feature_extraction_amd import capi
from tests import map_localize_util as lu
from tests import map_merge_util as mm
from tests import map_observe_util as ou

F32 = lu.F32
CHUNK = 512  # csrc/fx_map_expect.hip FXE_CHUNK: the rows of a scan staged in LDS at a time
WG = 256     # ... FXE_WG: landmarks in range taken a round
RESULT = capi.MAP_EXPECT_RESULT_FIELDS
WIDE = dict(x_min=-1000.0, x_max=1000.0, y_min=-1000.0, y_max=1000.0)  # a box that holds every test world


def case(frags, rows_by_scan, ids, loc=None, n_scans_map=3, edit=None, retire=None, repeat=1, **opts):
    c = ou.case(frags, rows_by_scan, ids, loc=loc, n_scans_map=n_scans_map, edit=edit, **opts)
    c["retire"], c["repeat"] = dict(retire or {}), repeat
    return c


state_of = ou.state_of
loc_records = ou.loc_records


def reference(st, c, expected=None, seen=None, **over):
    """capi.map_expect_reference on a case; over: n_scans, q_max_rows, stored and options in the place of the case's."""
    kw = dict(c["opts"], **over)
    n_scans, stored = kw.pop("n_scans", len(c["off"]) - 1), kw.pop("stored", len(c["rows"]))
    return capi.map_expect_reference(st, c["off"], c["rows"][:stored], c["loc"], c["ids"], n_scans, expected=expected, seen=seen, **kw)


def accumulated(st, c):
    """The counters of c["repeat"] FX_EXPECT_ADD calls from zero, and the result of one of them."""
    cap = int(st["max_landmarks"])
    e, s = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    res = None
    for _ in range(c["repeat"]):
        res, e, s = reference(st, c, expected=e, seen=s, mode=capi.FX_EXPECT_ADD)
    return res, e, s


def assert_counts(got, ref, what=""):
    """(result dict, expected, seen) of the device against the reference's: every word equal."""
    assert got[0] == ref[0], f"{what}: result {got[0]}, reference {ref[0]}"
    for name, a, b in (("expected_of_landmark", got[1], ref[1]), ("seen_of_landmark", got[2], ref[2])):
        a, b = np.asarray(a).astype(np.int64) & 0xffffffff, np.asarray(b).astype(np.int64) & 0xffffffff
        bad = np.flatnonzero(a != b) if a.shape == b.shape else [0]
        assert a.shape == b.shape and not len(bad), f"{what}: {name} differs at {bad[:8].tolist()}: got {a[bad[:8]]}, reference {b[bad[:8]]}"


def pose_records(poses, flags=capi.FX_LOC_VALID):
    """fx_localization records of poses [(yaw, tx, ty)]: c and s are the doubles math.cos / math.sin return."""
    return loc_records(len(poses), flags=flags, c=[math.cos(p[0]) for p in poses], s=[math.sin(p[0]) for p in poses], tx=[p[1] for p in poses],
                       ty=[p[2] for p in poses])


def local(pose, x, y):
    """A map point in the sensor frame of pose (yaw, tx, ty), as a float32 keypoint would hold it."""
    c, s = math.cos(pose[0]), math.sin(pose[0])
    dx, dy = x - pose[1], y - pose[2]
    return F32(c * dx + s * dy), F32(c * dy - s * dx)


# ---- hand-built cases: tests/test_map_expect_reference.py works the first ones out by hand
def hand4():
    """Landmarks 0 (10, 0), 1 (20, 5), 2 (30, 0), 3 (-10, 0).  Scan 0 under the identity sees landmark 0; scan 1, turned by a quarter
    (c = 0, s = 1), sees it again at (0, -10), outside the box."""
    frags = [(0, 10.0, 0.0), (0, 20.0, 5.0), (0, 30.0, 0.0), (0, -10.0, 0.0)]
    loc = loc_records(2, c=(1.0, 0.0), s=(0.0, 1.0))
    return case(frags, [[(10.0, 0.0, 1.0)], [(0.0, -10.0, 1.0)]], [0, 0], loc=loc, retire=dict(min_expected=2, seen_num=1, seen_den=2))


def shadow_gates():
    """One landmark at (16, 0) and one keypoint of no landmark a scan, at each gate's edge (shadow_width 0.5: |crs| <= 8):
    0: k2 == l2, not nearer; 1: along == 0, not in front; 2: crs^2 == w2 l2, shadowed; 3: the next float32 beyond, not shadowed;
    4: the next float32 below l2 on the ray, shadowed; 5: a keypoint whose z is not finite casts no shadow."""
    up = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
    below = float(np.nextafter(np.float32(16.0), np.float32(0.0)))
    rows = [[(16.0, 0.0, 1.0)], [(0.0, 0.25, 1.0)], [(8.0, 0.5, 1.0)], [(8.0, up, 1.0)], [(below, 0.0, 1.0)], [(8.0, 0.0, np.nan)]]
    return case([(0, 16.0, 0.0), (0, 500.0, 0.0)], rows, [-1] * 6, retire=dict(min_expected=4, seen_num=1, seen_den=8))


def edges():
    """One landmark at (10, 0), min_range 2, max_range 8, the identity turned nowhere and moved: 0: d2 == lo2; 1: d2 == hi2; 2: dx
    the next double beyond 8 (8 + 2^-49: the sensor is moved by that much, not by its own next double, which dx would round away);
    3: dx the next double below 2; 4: lx == x_min (d2 = 10); 5: lx the next double below x_min."""
    tx = (8.0, 2.0, 2.0 - 2.0 ** -49, float(np.nextafter(8.0, 9.0)), 9.0, float(np.nextafter(9.0, 10.0)))
    ty = (0.0, 0.0, 0.0, 0.0, -3.0, -3.0)
    return case([(0, 10.0, 0.0)], [[]] * 6, [], loc=loc_records(6, tx=tx, ty=ty), min_range=2.0, max_range=8.0)


def seen_outside():
    """Landmark 0 (100, 0) is named by a row but out of range: neither seen nor expected.  Landmark 1 (0, 20) is named and in range but
    outside the box (lx = 0 < 1): seen, hence expected."""
    return case([(0, 100.0, 0.0), (0, 0.0, 20.0)], [[(100.0, 0.0, 1.0), (0.0, 20.0, 1.0)]], [0, 1])


def _merged(st):
    return mm.merge_to_fixpoint(st)[0]


def twins():
    """map_observe_util.merged_twins after its merge (alias [-1, -1, 0], landmark 0 at 0.0625): rows named 0 and 2 in one scan name one
    landmark, once a scan."""
    c = ou.merged_twins()
    return dict(c, edit=_merged, opts=dict(min_range=0.0), retire={}, repeat=1)


def _nan_z(k):
    def edit(st):
        st["landmarks"][k]["z"] = float("nan")
        return st
    return edit


def stale():
    """Landmark 1's z is not finite: the row that names it is stale, and it is nobody's expectation.  Ids beyond N, -1 and garbage
    propose nothing."""
    frags = [(0, 10.0, 0.0), (0, 20.0, 0.0), (0, 10.0, 8.0)]
    rows = [[(10.0, 0.0, 1.0), (20.0, 0.0, 1.0), (10.0, 8.0, 1.0), (5.0, 5.0, 1.0), (5.0, -5.0, 1.0), (6.0, -5.0, 1.0)]]
    return case(frags, rows, [0, 1, 3, -1, ou.I32_MIN, ou.I32_MAX], edit=_nan_z(1))


def filters(require_flags=capi.FX_LOC_VALID):
    """map_observe_util.filters: seven scans, two of them VALID with a finite pose; rows with NaN and inf coordinates."""
    c = ou.filters(require_flags)
    return dict(c, opts=dict(c["opts"], min_range=0.0, **WIDE), retire={}, repeat=1)


def carried():
    """Three landmarks nobody sees; the third (the fragment that begins in scan 1: ids follow first_scan) is in the map's last scan,
    so a carry row holds it: the counters condemn all three, two are retired, one is protected."""
    frags = [(0, 10.0, 0.0), (1, 20.0, 5.0), (0, 30.0, 7.0)]
    return case(frags, [[], [(5.0, 5.0, 1.0)]], [-1], retire=dict(min_expected=2, seen_num=1, seen_den=8), **WIDE)


# ---- the flicker world with two poles cut down
def cut_world():
    """map_merge_util.flicker (40 poles, 24 scans, 25 % dropout) as the mapping run, and the same scans as the localised run with
    two poles cut down: their rows are not finite any more.  The poles are the first two that the map's last scan does not hold
    (a landmark the carry holds cannot be retired).  Returns (w, pieces, the localised rows, the mask of the rows that left)."""
    w, pieces, poles = mm.flicker()
    last = set(int(k) for k in w["pole"][int(w["off"][-2]):int(w["off"][-1])])
    gone = [k for k in range(len(poles)) if k not in last][:2]
    assert len(gone) == 2
    left = np.isin(w["pole"], gone)
    rows = w["rows"].copy()
    rows[left, :3] = np.nan
    return w, pieces, rows, left


def doomed_landmarks(st, w, left, priors):
    """The live landmarks that stand on the poles that left: those the rows of these poles are matched to when they are still there."""
    full = capi.map_localize_reference(st, w["off"], w["rows"], priors, len(w["off"]) - 1, segment=capi.FX_LOC_ANY_SEGMENT)["map_id_of_row"]
    return sorted(set(int(i) for i in mm.resolve(full, st["alias"])[left] if i >= 0))


CHAIN = dict(expect=dict(WIDE, min_range=0.0), retire=dict(min_expected=4, seen_num=1, seen_den=8), merge=dict(max_gap_scans=24))


# ---- generated fields: a lattice of landmarks, scans at random poses inside it
def field(n_landmarks, rows_by_scan, seed, poses=None, pitch=3.0, far=None, retire=None, repeat=1, **opts):
    """n_landmarks on a square lattice; scan b at a seeded pose inside it (or poses[b]) with rows_by_scan[b] rows: about half of them
    at landmarks within 40 m of the sensor and named so (a few named wrongly, a few through ids that propose nothing), the rest
    clutter of no landmark; every 37th row not finite.  far: (landmark, x) moves that landmark's record to x (an edit)."""
    rng = np.random.default_rng(seed)
    frags = lu.lattice(n_landmarks, pitch=pitch)
    side = pitch * math.ceil(math.sqrt(n_landmarks))
    xy = np.array([(f[1], f[2]) for f in frags])
    by_scan, ids, used = [], [], []
    for b, n in enumerate(rows_by_scan):
        pose = poses[b] if poses is not None and b < len(poses) else (float(rng.uniform(-math.pi, math.pi)), float(rng.uniform(0, side)), float(rng.uniform(0, side)))
        used.append(pose)
        near = np.flatnonzero(np.hypot(xy[:, 0] - pose[1], xy[:, 1] - pose[2]) <= 40.0)
        scan = []
        for i in range(n):
            r = len(ids)
            if len(near) and rng.random() < 0.5:
                g = int(near[rng.integers(len(near))])
                lx, ly = local(pose, xy[g, 0] + rng.uniform(-0.05, 0.05), xy[g, 1] + rng.uniform(-0.05, 0.05))
                ids.append(g if r % 11 else (int(rng.integers(n_landmarks)) if r % 22 else n_landmarks + r))
            else:
                lx, ly = F32(rng.uniform(-50, 50)), F32(rng.uniform(-50, 50))
                ids.append(-1 if r % 5 else ou.I32_MAX - r)
            scan.append((lx, ly, F32(rng.uniform(0.5, 2.0))) if (r + 1) % 37 else (lx, np.nan, 1.0))
        by_scan.append(scan)
    edit = None
    if far is not None:
        def edit(st, k=far[0], x=far[1]):
            st["landmarks"][k]["x"], st["acc"][k][0] = float(x), 2.0 * float(x)
            return st
    return case(frags, by_scan, ids, loc=pose_records(used), edit=edit, retire=retire, repeat=repeat, **opts)


HUGE = 2.0 ** 41  # a sensor there with max_range 0.5 lies in a cell beyond 2^41: it searches the far bucket alone
BORDER = 4.0 * (1.0 + 1.0 / 256.0)  # the cell edge of max_range 4

RETIRE = dict(min_expected=3, seen_num=1, seen_den=4)
CPU_CASES = dict(
    hand4=hand4, shadow_gates=shadow_gates, edges=edges, seen_outside=seen_outside, twins=twins, stale=stale, filters=filters,
    filters_any=lambda: filters(require_flags=0), carried=carried,
    three=lambda: field(3, [0, 1, 5], 11, retire=dict(min_expected=1, seen_num=1, seen_den=1), **WIDE),
    n255=lambda: field(255, [63, 64, 65], 12, retire=RETIRE, repeat=2),
    n256=lambda: field(256, [64, 0, 257], 13, retire=RETIRE, repeat=2, shadow_width=0.0),
    n257=lambda: field(257, [1, 65, 63], 14, retire=RETIRE, repeat=2, **WIDE),
    n1100=lambda: field(1100, [CHUNK - 1, CHUNK, CHUNK + 1, 0, 64], 15, retire=dict(min_expected=4, seen_num=1, seen_den=8), repeat=2, min_range=0.0, **WIDE),
    none_in_range=lambda: field(64, [8, 8], 16, poses=[(0.3, 1.5, 1.5), (1.0, 4.5, 7.5)], min_range=0.0, max_range=1.0, **WIDE),
    one_in_range=lambda: field(64, [8, 8], 17, poses=[(0.3, 3.25, 3.0), (1.0, 6.0, 8.5)], min_range=0.0, max_range=1.0, **WIDE),
    border=lambda: field(300, [16, 16, 16], 18, poses=[(0.0, 2 * BORDER, 3 * BORDER), (2.0, 5 * BORDER, BORDER), (-1.0, BORDER, 7 * BORDER)],
                         min_range=0.0, max_range=4.0, **WIDE),
    far=lambda: field(16, [4, 4], 19, poses=[(0.0, HUGE - 0.25, 0.0), (0.0, 1.0, 1.0)], far=(0, HUGE), min_range=0.0, max_range=0.5, **WIDE),
)
