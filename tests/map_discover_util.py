"""Helpers of the map discovery tests (tests/test_map_discover_reference.py, tests/test_gpu_map_discover.py): hand-built map states
(a state goes to the device through the snapshot: Map.import_state(capi.map_snapshot_pack(state))), hand-built scans, localisation
records and row-to-landmark tables, seeded worlds, and the comparison of a device result with capi.map_discover_reference bit for
bit.  A case is a dict: st (the map's state), off / rows (the scans), loc (LOC_DTYPE), ids (the table), opts (what the reference
and Map.discover take)."""
import math

import numpy as np

from feature_extraction_amd import capi
from tests import map_localize_util as lu
from tests import map_observe_util as ou

F32 = lu.F32
VALID = capi.FX_LOC_VALID
FIELDS = capi.MAP_DISCOVER_RESULT_FIELDS
SEEDS = (11, 12, 27, 34, 39)  # every one meets census() (tests/test_map_discover_reference.py checks it)
loc_records = ou.loc_records


# ---- map states by hand
def landmark(x, y, z=1.0, n_obs=2, segment=0, first_scan=0, last_scan=1, flags=0):
    """(record, sums) of a landmark of n_obs identical observations at (x, y, z): float32-exact values give exact sums."""
    x, y, z = float(x), float(y), float(z)
    rec = dict(x=x, y=y, z=z, rms_xy=np.float32(0.0), n_obs=int(n_obs), first_scan=int(first_scan), last_scan=int(last_scan), segment=int(segment), flags=int(flags))
    return rec, [x * n_obs, y * n_obs, z * n_obs, x, y, 0.0, 0.0, 0.0]


def state(lms, cap=None, carry=8, scans=4, segments=1, n_needed=None, alias=None, flags=0):
    """A map state holding the landmarks `lms` ((x, y) pairs or landmark() results), as a mapping run of `scans` scans in `segments`
    segments would have left it."""
    lms = [l if isinstance(l[0], dict) else landmark(*l) for l in lms]
    st = capi.map_state(len(lms) if cap is None else cap, carry)
    st["landmarks"], st["acc"] = [dict(r) for r, _ in lms], [list(a) for _, a in lms]
    st["header"].update(n_landmarks=len(lms), n_needed=len(lms) if n_needed is None else n_needed, n_obs=sum(r["n_obs"] for r, _ in lms),
                        scans=scans, batches=1, segments=segments, flags=flags)
    if alias is not None:
        st["alias"] = list(alias)
    return st


def case(st, rows_by_scan, ids=None, loc=None, **opts):
    off, rows = lu.scans(rows_by_scan)
    loc = loc_records(len(rows_by_scan)) if loc is None else loc
    ids = np.full(len(rows), -1, np.int32) if ids is None else np.array(ids, np.int64).astype(np.int32)
    return dict(st=st, off=off, rows=rows, loc=loc, ids=ids, opts=opts)


def reference(c, st=None, **over):
    """capi.map_discover_reference on a case; st: another state; over: n_scans, q_max_rows, stored (the rows the block stores),
    dry_run and options in the place of the case's."""
    kw = dict(c["opts"], **over)
    n_scans, stored = kw.pop("n_scans", len(c["off"]) - 1), kw.pop("stored", len(c["rows"]))
    return capi.map_discover_reference(c["st"] if st is None else st, c["off"], c["rows"][:stored], c["loc"], c["ids"], n_scans, **kw)


def assert_identities(res, what=""):
    assert res["unmatched"] == res["known"] + res["free_rows"], f"{what}: {res}"
    assert res["free_rows"] == res["orphans"] + res["duplicates"] + res["weak"] + res["added"] + res["lost"], f"{what}: {res}"


def assert_outputs(got, ref, what=""):
    """(result dict, new_id_of_row) of the device against the reference's: every word equal."""
    assert got[0] == ref[0], f"{what}: result {got[0]}, reference {ref[0]}"
    if got[1] is not None:
        a, b = np.asarray(got[1]).astype(np.int64), np.asarray(ref[1]).astype(np.int64)
        bad = np.flatnonzero(a != b) if a.shape == b.shape else [0]
        assert a.shape == b.shape and not len(bad), f"{what}: new_id_of_row differs at {bad[:8].tolist()}: got {a[bad[:8]]}, reference {b[bad[:8]]}"


def values(res):
    return tuple(res[k] for k in FIELDS)


# ---- the cases
def hand():
    """tests/test_map_discover_reference.py works this one out by hand.  Two landmarks of segment 0 at (0, 0) and (10, 0); three scans:
    the identity, a shift by (1, 0), a quarter turn about the origin.  World points: an inlier row at landmark 0 (id 0); an unmatched
    row 0.5 m east of landmark 1; a new pole near (5, 5), seen at (5, 5), (5.125, 5) and (5, 5.25); a pole at (-5, 5) seen in two
    scans only."""
    st = state([(0.0, 0.0), (10.0, 0.0)], cap=8, scans=7)
    scan0 = [(0.0, 0.0, 1.0), (10.5, 0.0, 1.0), (5.0, 5.0, 1.0), (-5.0, 5.0, 2.0)]
    scan1 = [(4.125, 5.0, 2.0), (-6.0, 5.0, 2.0)]  # under tx = 1
    scan2 = [(5.25, -5.0, 3.0)]                    # under a quarter turn: (x, y) -> (-y, x)
    loc = loc_records(3, c=(1.0, 1.0, 0.0), s=(0.0, 0.0, 1.0), tx=(0.0, 1.0, 0.0))
    return case(st, [scan0, scan1, scan2], [0, -1, -1, -1, -1, -1, -1], loc=loc)


def chain():
    """Three free rows 0.25 m apart in one line, join_dist 0.375 (all float32-exact): leader, attached, orphan; in three scans each so
    that the leader is confirmed."""
    st = state([(100.0, 100.0)], cap=8)
    by_scan = [[(0.0, 0.0, 1.0), (0.25, 0.0, 1.0), (0.5, 0.0, 1.0)] for _ in range(3)]
    return case(st, by_scan, known_dist=1.0, join_dist=0.375)


def join_edge():
    """A leader at the origin and a row at distance exactly jd = 0.5 (attaches), one at the next double above 0.5 (through tx: does
    not, and leads); min_obs 1."""
    up = float(np.nextafter(0.5, 1.0))
    st = state([(100.0, 100.0)], cap=8)
    return case(st, [[(0.0, 0.0, 1.0)]] * 3, loc=loc_records(3, tx=(0.0, 0.5, -up)), known_dist=1.0, join_dist=0.5, min_obs=1)


def known_edge():
    """A landmark at the origin, kd = 1: a row at exactly 1.0 is known, one at the next double above is free."""
    up = float(np.nextafter(1.0, 2.0))
    st = state([(0.0, 0.0)], cap=8)
    return case(st, [[(0.0, 0.0, 1.0)]] * 2, loc=loc_records(2, tx=(1.0, -up)), known_dist=1.0, join_dist=0.25, min_obs=1)


def two_in_a_scan():
    """Scan 0 sets the leader; scan 1 has three rows on it: 0.125 east, 0.0625 north (the lowest d2: kept), 0.125 west; scan 2 has two
    rows at equal d2 bits (0.125 east and west): the lower row is kept."""
    st = state([(100.0, 100.0)], cap=8)
    by_scan = [[(0.0, 0.0, 1.0)], [(0.125, 0.0, 1.0), (0.0, 0.0625, 2.0), (-0.125, 0.0, 3.0)], [(0.125, 0.0, 4.0), (-0.125, 0.0, 5.0)]]
    return case(st, by_scan)


def two_poles(n_scans=3, cap=8, n_needed=None, lms=1):
    """Two new poles seen in every one of n_scans scans, the pole of the HIGHER first row first in the later scans: ids follow the
    leader rows.  A map of `lms` landmarks far away."""
    st = state([(100.0 + 5.0 * k, 100.0) for k in range(lms)], cap=cap, n_needed=n_needed)
    by_scan = [[(20.0, 0.0, 1.0), (0.0, 20.0, 1.0)]] + [[(0.0, 20.0, 1.0), (20.0, 0.0, 1.0)] for _ in range(n_scans - 1)]
    return case(st, by_scan)


def segments_and_aliases():
    """Landmark 0 of segment 0 at (0, 0); landmark 1 of segment 1 at (10, 0); landmark 2 of segment 1 at (20, 0), absorbed by landmark 3
    at (20.5, 0).  Rows at (0.25, 0), (10.25, 0), (19.5, 0) and (20.25, 0), in three scans, segment 1: the first is not explained by a
    landmark of another segment, the third is 0.5 from the absorbed record and 1.0 from its root with kd = 0.75: free; the last is
    known through the root."""
    lms = [landmark(0.0, 0.0), landmark(10.0, 0.0, segment=1), landmark(20.0, 0.0, segment=1), landmark(20.5, 0.0, segment=1)]
    st = state(lms, cap=8, segments=2, alias=[-1, -1, 3, -1])
    rows = [(0.25, 0.0, 1.0), (10.25, 0.0, 1.0), (19.5, 0.0, 1.0), (20.25, 0.0, 1.0)]
    return case(st, [rows] * 3, known_dist=0.75, join_dist=0.25)


def filters(require_flags=VALID):
    """Seven scans of three rows on three new poles; the records as map_observe_util.filters has them: VALID, NO_SCAN, BAD_PRIOR,
    NO_HYPOTHESIS, VALID on a NaN pose, VALID on an infinite pose, VALID | TRUNCATED; rows with NaN and inf coordinates in the first
    and the last scan; a VALID pose so far out that the world point overflows; ids at and beyond N and INT32_MAX are matched rows."""
    st = state([(100.0, 100.0)], cap=8)
    by_scan = [[(0.0, 0.0, 1.0), (5.0, 0.0, 1.0), (0.0, 5.0, 1.0)] for _ in range(8)]
    by_scan[0][1] = (np.nan, 0.0, 1.0)
    by_scan[6][0] = (0.0, 0.0, np.inf)
    by_scan[6][2] = (0.0, -np.inf, 1.0)
    loc = loc_records(8)
    loc["flags"] = (VALID, capi.FX_LOC_NO_SCAN, capi.FX_LOC_BAD_PRIOR, capi.FX_LOC_NO_HYPOTHESIS, VALID, VALID, VALID | capi.FX_LOC_TRUNCATED, VALID)
    loc["pose"]["ty"][4], loc["pose"]["c"][5], loc["pose"]["tx"][7] = np.nan, np.inf, 1.7e308
    loc["pose"]["c"][7] = 1e308  # (the rows at 5 overflow; the row at the origin is a finite point at 1.7e308: every d2 from it is inf)
    ids = np.full(24, -1, np.int64)
    ids[[3, 9, 19]] = (1, 7, ou.I32_MAX)
    return case(st, by_scan, ids, loc=loc, require_flags=require_flags, min_obs=1)


def free_rows(n, pitch=2.0, n_scans=1, **opts):
    """n free rows `pitch` apart on a lattice in each of n_scans scans (min_obs 1 unless given): n leaders."""
    pts = [(x, y, 1.0) for _, x, y in lu.lattice(n, pitch=pitch)]
    return case(state([(-100.0, -100.0)], cap=n + 4), [pts] * n_scans, **dict(dict(min_obs=1), **opts))


def one_cell(n=70):
    """n free rows of one scan within 0.07 m of each other, join_dist 0.30: one grid cell (3.1 .. 3.15 over the cell edge 0.3012 is
    10.29 .. 10.46), one leader, n - 1 duplicates; two more scans confirm it."""
    rng = np.random.default_rng(70)
    crowd = [(F32(3.1 + rng.uniform(0, 0.05)), F32(3.1 + rng.uniform(0, 0.05)), 1.0) for _ in range(n)]
    return case(state([(-100.0, -100.0)], cap=8), [crowd, crowd[:1], crowd[1:3]])


def far_case():
    """A pole at 2^40 m (beyond 2^39 cells of 0.3 m: the far bucket; doubles there are 2^-12 apart) next to a near one.  A scan has
    one pose, so the far pole has scans of its own: scans 0 .. 2 see the near pole, scans 3 .. 5, under tx = 2^40, the far one."""
    far = float(2 ** 40)
    by_scan = [[(1.0, 1.0, 1.0)]] * 3 + [[(0.0, 0.125, 1.0)], [(0.0625, 0.125, 1.0)], [(0.0, 0.25, 1.0)]]
    return case(state([(-100.0, -100.0)], cap=8), by_scan, loc=loc_records(6, tx=(0.0, 0.0, 0.0, far, far, far)))


def long_list(n_scans=65):
    """One new pole seen in n_scans scans (a list longer than a wavefront), jittered by multiples of 2^-10."""
    rng = np.random.default_rng(65)
    by_scan = [[(3.0 + int(rng.integers(-32, 33)) / 1024.0, 4.0 + int(rng.integers(-32, 33)) / 1024.0, 1.0)] for _ in range(n_scans)]
    return case(state([(-100.0, -100.0)], cap=8), by_scan)


def world(seed):
    """A seeded localisation run: 5 - 40 scans at random poses over a map of up to 40 landmarks (a jittered 5 m lattice) and up to 6
    new poles between them.  A landmark is detected in a scan with probability 0.7 and its row matched with 0.8 (the others are
    unmatched rows a landmark explains); a new pole is detected with 0.8, the last new pole in scans 0 and 1 only (weak); every
    scan has one near-twin row 5 - 10 cm from one of its new-pole rows (a duplicate); the rows of a scan are shuffled; scan 0 ends in
    a chain of three rows 0.2 m apart at a place of its own (leader, attached, orphan); 3 cm of jitter everywhere else."""
    rng = np.random.default_rng(seed)
    S, L, P = int(rng.integers(5, 41)), int(rng.integers(8, 41)), int(rng.integers(2, 7))
    side = int(math.ceil(math.sqrt(L))) + 1
    lm_xy = [(F32(5.0 * (k % side) + rng.uniform(-0.5, 0.5)), F32(5.0 * (k // side) + rng.uniform(-0.5, 0.5))) for k in range(L)]
    cells = rng.permutation(side * side)[:P + 1]
    new_xy = [(5.0 * (int(k) % side) + 2.5, 5.0 * (int(k) // side) + 2.5) for k in cells]
    lms = [landmark(x, y, n_obs=int(rng.integers(1, 6))) for x, y in lm_xy]
    st = state(lms, cap=L + 8, scans=int(rng.integers(1, 50)))
    yaw, tx, ty = rng.uniform(-math.pi, math.pi, S), rng.uniform(0.0, 5.0 * side, S), rng.uniform(0.0, 5.0 * side, S)
    loc = loc_records(S, c=np.cos(yaw), s=np.sin(yaw), tx=tx, ty=ty, tz=0.5)
    by_scan, ids = [], []

    def local(b, wx, wy):
        c, s = math.cos(yaw[b]), math.sin(yaw[b])
        dx, dy = wx - tx[b], wy - ty[b]
        return (F32(c * dx + s * dy), F32(c * dy - s * dx), F32(rng.uniform(0.5, 1.5)))
    for b in range(S):
        rows = []
        for k, (x, y) in enumerate(lm_xy):
            if rng.random() < 0.7:
                rows.append((local(b, x + rng.normal(0, 0.03), y + rng.normal(0, 0.03)), k if rng.random() < 0.8 else -1))
        seen = []
        for k, (x, y) in enumerate(new_xy[:P]):
            if (b < 2) if k == P - 1 else (rng.random() < 0.8):
                p = (x + rng.normal(0, 0.03), y + rng.normal(0, 0.03))
                seen.append(p)
                rows.append((local(b, *p), -1))
        if seen:
            p = seen[int(rng.integers(len(seen)))]
            a = rng.uniform(0, 2 * math.pi)
            rows.append((local(b, p[0] + 0.075 * math.cos(a), p[1] + 0.075 * math.sin(a)), -1))
        rows = [rows[i] for i in rng.permutation(len(rows))]
        if b == 0:
            x, y = new_xy[P]
            rows += [(local(0, x + 0.2 * i, y), -1) for i in range(3)]
        by_scan.append([r for r, _ in rows])
        ids += [i for _, i in rows]
    return case(st, by_scan, ids, loc=loc)


def census(res):
    """What a seeded case must show: none of them is vacuous."""
    return all(res[k] >= 1 for k in ("created", "known", "orphans", "duplicates", "weak"))


CASES = dict(hand=hand, chain=chain, join_edge=join_edge, known_edge=known_edge, two_in_a_scan=two_in_a_scan, two_poles=two_poles,
             min_obs_short=lambda: two_poles(n_scans=2), one_short_of_full=lambda: two_poles(cap=2), overflowed=lambda: two_poles(cap=1, n_needed=3),
             segments_and_aliases=segments_and_aliases, filters=filters, filters_any=lambda: filters(require_flags=0), one_cell=one_cell,
             far=far_case, long_list=long_list)
