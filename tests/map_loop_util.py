"""Helpers of the loop closure tests (tests/test_map_loop_reference.py, tests/test_gpu_map_loop.py): a world whose trajectory
comes back to its start with drift in its registration records, hand-built maps with chosen scan numbers, and the comparison of a
device result with capi.map_loop_reference bit for bit.

The loop world.  track_util.world cannot serve: its circle has radius 25 m under a reach of 35 m, so the poles about the centre
are seen from everywhere, and it covers three quarters of a lap.  Here 250 poles lie in a field of 200 m, the trajectory is a
circle of radius 60 m about its centre run for 1.2 laps in 80 scans, the reach is 35 m and the noise 1 cm.  Every fx_registration
record carries a yaw bias and an along-track bias, so the chained poses drift and the poles of the first fifth of a lap are held
twice, the closure error apart.  The run is cut every 16 scans into batches that overlap by one scan.

SEED and BIAS: the first seed (from 0) and the first bias of the issue's table for which capi.map_loop_reference alone meets
tests/test_map_loop_reference.py's conditions, searched on the CPU.  Measured with seed 0, bias 3e-4 rad and 3 mm a link,
min_loop_scans 50, recent_scans 16: see MEASURED below (the test prints the same figures)."""
import math

import numpy as np

from feature_extraction_amd import capi
from tests import map_join_util as ju
from tests import map_merge_util as mm
from tests import map_util as mu
from tests import track_util as tu

WORLD = dict(seed=0, yaw_bias=3e-4, along_bias=3e-3, n_poles=250, n_scans=80, field=200.0, radius=60.0, laps=1.2, reach=35.0, sigma=0.01,
             step=16, cap=1024, carry=128)
OPTS = dict(min_loop_scans=50, recent_scans=16)  # of the 80 scans: targets ended by scan 29, queries began at scan 63 or later
# 206 landmarks, 39 queries, 39 correspondences, 39 inliers, rms 0.0099 m, s0 24, s1 63, 139 landmarks moved; T: yaw -0.01964 rad,
# t (-1.177, 0.010) m; the worst inlier pair afterwards 0.0237 m; the merge then joins 39 of the 39 pairs, and none without the closure
MEASURED = dict(d_before=1.8594, d_after=0.0237)
F32 = ju.F32


def loop_world(seed=None, yaw_bias=None, along_bias=None, step=None):
    """(w, pieces): a dict like track_util.world's for the layout above, its reg records biased, and its batches (cut every `step`
    scans, default WORLD's)."""
    f = WORLD
    seed = f["seed"] if seed is None else seed
    yaw_bias, along_bias = f["yaw_bias"] if yaw_bias is None else yaw_bias, f["along_bias"] if along_bias is None else along_bias
    rng = np.random.default_rng(seed)
    n_poles, n_scans, field, reach = f["n_poles"], f["n_scans"], f["field"], f["reach"]
    poles = np.concatenate([rng.uniform(0, field, (n_poles, 2)), rng.uniform(0, 2, (n_poles, 1))], axis=1)
    ang = np.linspace(0.0, f["laps"] * 2.0 * math.pi, n_scans)
    absolute = [(a + math.pi / 2, field / 2 + f["radius"] * math.cos(a), field / 2 + f["radius"] * math.sin(a), 0.0) for a in ang]
    y0, x0, y0_, z0 = absolute[0]
    c0, s0 = math.cos(y0), math.sin(y0)
    truth = [(y - y0, c0 * (x - x0) + s0 * (y_ - y0_), -s0 * (x - x0) + c0 * (y_ - y0_), z - z0) for y, x, y_, z in absolute]
    off, rows, pole = [0], [], []
    for yaw, x, y, z in absolute:
        d = poles[:, :2] - (x, y)
        seen = np.flatnonzero(np.hypot(d[:, 0], d[:, 1]) <= reach)
        seen = seen[rng.permutation(len(seen))]
        c, s = math.cos(yaw), math.sin(yaw)
        loc = np.zeros((len(seen), 4), np.float32)
        loc[:, 0], loc[:, 1], loc[:, 2] = c * d[seen, 0] + s * d[seen, 1], -s * d[seen, 0] + c * d[seen, 1], poles[seen, 2] - z
        loc[:, :3] += (f["sigma"] * rng.standard_normal((len(seen), 3))).astype(np.float32)
        loc[:, 3] = rng.uniform(-0.3, 0.3, len(seen))
        rows.append(loc), pole.append(seen), off.append(off[-1] + len(seen))
    rows, pole = np.concatenate(rows), np.concatenate(pole)
    m, inlier = tu.match_rows(off), np.zeros(off[-1], np.int32)
    for b in range(1, n_scans):
        before = {int(k): off[b - 1] + i for i, k in enumerate(pole[off[b - 1]:off[b]])}
        for r in range(off[b], off[b + 1]):
            t = before.get(int(pole[r]))
            if t is not None:
                m["train_row"][r], m["flags"][r], m["dist2"][r], inlier[r] = t, tu.ACC, 1.0, 1
    # the heading is along the track: the sensor's x is the along-track direction
    motions = [(yaw + yaw_bias, tx + along_bias, ty, tz) for yaw, tx, ty, tz in tu.relative(truth)]
    w = dict(off=np.array(off, np.uint32), rows=rows, pole=pole, m=m, inlier=inlier, reg=tu.reg_records(motions), truth=truth, n_scans=n_scans)
    return w, mu.split(w, mu.every(n_scans, f["step"] if step is None else step))


def run(w, pieces):
    """The reference's map of the run and the pole of every landmark."""
    st, _, ids = mu.run_reference(pieces, WORLD["cap"], WORLD["carry"])
    return st, ju.poles_of(w, pieces, ids, len(st["landmarks"]))


def eligible(st, min_obs=2):
    lms = st["landmarks"]
    a = list(st.get("alias", [])) + [-1] * (len(lms) - len(st.get("alias", [])))
    return [i for i, r in enumerate(lms) if a[i] == -1 and r["n_obs"] >= min_obs and all(math.isfinite(r[k]) for k in ("x", "y", "z"))]


def spread(st, pole):
    """The largest xy distance between two eligible landmarks of one pole."""
    by = {}
    for i in eligible(st):
        by.setdefault(int(pole[i]), []).append(i)
    worst = 0.0
    for ids in by.values():
        for a in ids:
            for b in ids:
                worst = max(worst, math.hypot(st["landmarks"][a]["x"] - st["landmarks"][b]["x"], st["landmarks"][a]["y"] - st["landmarks"][b]["y"]))
    return worst


def roots(st):
    a = list(st.get("alias", [])) + [-1] * (len(st["landmarks"]) - len(st.get("alias", [])))
    return [i if a[i] < 0 else a[i] for i in range(len(a))]


def timed(frags, scans, seed=7):
    """A hand-built state: one landmark of two identical observations for every (x, y) of frags, in one segment, then its
    first_scan, last_scan = scans[k] and header.scans = the highest last_scan + 1 set by hand (the loop reads nothing else of the
    time).  Returns the state."""
    st, _ = mm.reference_of(mm.fragments([(0, F32(x), F32(y)) for x, y in frags], 3, seed=seed), cap=len(frags) + 3, carry=8)
    st = dict(st, header=dict(st["header"]), landmarks=[dict(r) for r in st["landmarks"]])
    for r, (a, b) in zip(st["landmarks"], scans):
        r["first_scan"], r["last_scan"] = int(a), int(b)
    st["header"]["scans"] = max(int(b) for _, b in scans) + 1
    return st


def old_and_recent(n_old, n_recent, n_between=0, shift=(0.5, -0.25), pitch=4.0, jitter=0.01, last=400, seed=5):
    """n_old landmarks on a lattice that ended at scans 0 .. 9, n_recent twins of the first of them moved by `shift` (+ jitter *
    (k % 7) in x) that began at scans last - 9 .. last, and n_between landmarks in between (scans 100 .. 300), their ids
    interleaved while the kinds last.  Default options: min_loop_scans 256, recent_scans 32."""
    side = int(math.ceil(math.sqrt(max(n_old, 1))))
    old = [((pitch * (k % side), pitch * (k // side)), (k % 5, k % 5 + k % 6 + 4)) for k in range(n_old)]
    rec = [((old[k % n_old][0][0] + shift[0] + jitter * (k % 7), old[k % n_old][0][1] + shift[1]), (last - 9 + k % 7, last - k % 3)) for k in range(n_recent)]
    mid = [((pitch * (k % side) + 1.5, pitch * (k // side) + 1.5), (100 + k % 150, 150 + k % 150)) for k in range(n_between)]
    frags, scans = [], []
    for k in range(max(n_old, n_recent, n_between)):
        for arr in (old, rec, mid):
            if k < len(arr):
                frags.append(arr[k][0]), scans.append(arr[k][1])
    return timed(frags, scans, seed=seed)


def assert_result(got, ref, what=""):
    """A device result record against the reference's: integers equal, doubles and rms as bit patterns."""
    for f in capi.LOOP_DTYPE.names:
        a, b = np.atleast_1d(got[f]), np.atleast_1d(ref[f])
        a, b = (a, b) if a.dtype.kind == "u" else (ju.bits(a), ju.bits(b))
        assert (a == b).all(), f"{what}: result.{f}: got {got[f]!r}, reference {ref[f]!r}"


def transform_of(res):
    return tuple(float(res[k]) for k in ("c", "s", "tx", "ty", "tz"))
