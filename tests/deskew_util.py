"""Helpers of the de-skew tests (tests/test_deskew_reference.py, tests/test_gpu_deskew.py): a world of poles seen from a sensor that
moves DURING each sweep, the blocks and records the call takes, the exact constant-twist correction in closed form, a least-squares
pose fit, and the comparison with capi.deskew_reference (integers equal, floats bit for bit).

The world.  The sensor moves on a straight line or an arc at constant speed v (m/s) and yaw rate w (rad/s); a sweep takes TSW = 0.1 s,
starts behind the sensor (start_turn 0.5), turns clockwise seen from above (direction -1) and the scan is stamped at its end
(ref_fraction 1): fx_deskew_options's defaults.  Scan b (b = 1 .. n) is stamped at b TSW and holds the poles inside the reference's
pass-through box (x in [0, 75], y in [-30, 30]) under the pose at the stamp; each pole is seen from the pose at the moment its own
azimuth is swept, (b - 1 + phi) TSW, where phi is the sweep fraction of the row itself: a fixed point, iterated."""
import math

import numpy as np

from feature_extraction_amd import capi
from tests import track_util as tu

TSW = 0.1
BOX = (0.0, 75.0, -30.0, 30.0)
RUNS = ((15.0, 0.0), (15.0, 0.3), (8.0, 0.6), (30.0, 0.0))  # (v, w): two straight runs and two arcs
SEED = 1
# The interpolated transform against the exact constant-twist correction on the two arcs of RUNS, seed SEED: the largest distance
# measured on capi.deskew_reference is ARC_MEASURED (m); the bound is twice that.  (The interpolation moves the origin on the chord
# and turns by a normalised lerp, the twist on the arc: a few millimetres over a tenth of a second.)
ARC_MEASURED = 0.00602  # (5.63 mm at 15 m/s and 0.3 rad/s, 6.02 mm at 8 m/s and 0.6 rad/s)
ARC_BOUND = 2 * ARC_MEASURED
# LINKS with the motions capi.register_reference finds on the skewed scans themselves, 2 cm of noise, RUNS and SEED: the largest
# distance between a corrected scan's fitted pose and the true pose is POSE_MEASURED (m); the bound is twice that.
POSE_MEASURED = 0.01877  # (0.0150, 0.0188, 0.0183 and 0.0179 m in the order of RUNS)
POSE_BOUND = 2 * POSE_MEASURED


def pose_at(t, v, w):
    """(yaw, x, y) of the sensor at time t: constant body twist (v, w) from the identity at t = 0."""
    th = w * t
    if abs(w) < 1e-12:
        return th, v * t, 0.0
    return th, v / w * math.sin(th), v / w * (1.0 - math.cos(th))


def to_local(pose, p):
    yaw, x, y = pose
    c, s = math.cos(yaw), math.sin(yaw)
    dx, dy = p[0] - x, p[1] - y
    return c * dx + s * dy, -s * dx + c * dy


def to_world(pose, q):
    yaw, x, y = pose
    c, s = math.cos(yaw), math.sin(yaw)
    return c * q[0] - s * q[1] + x, s * q[0] + c * q[1] + y


def world(v, w, n_scans=9, seed=SEED, sigma=0.0, skew=True, n_poles=160):
    """-> dict: off, rows [N, 4] float32 (x, y, z, elevation), pole [N], phi [N] (the sweep fraction each row was seen at), poles,
    poses (the true pose at each scan's stamp), v, w, n_scans, and m / inlier: the fx_match records and inlier words of
    pairs_consecutive(off) built from the truth (a row whose pole is in the scan before is matched to that row)."""
    rng = np.random.default_rng(seed)
    poles = np.column_stack([rng.uniform(-10, 130, n_poles), rng.uniform(-60, 60, n_poles), rng.uniform(0, 2, n_poles)])
    off, rows, pole, phis, poses = [0], [], [], [], []
    for b in range(1, n_scans + 1):
        end = pose_at(b * TSW, v, w)
        poses.append(end)
        for k, p in enumerate(poles):
            l = to_local(end, p)
            if not (BOX[0] <= l[0] <= BOX[1] and BOX[2] <= l[1] <= BOX[3]):
                continue
            phi = 1.0
            if skew:
                phi, settled = 0.5, False
                for _ in range(60):
                    l = to_local(pose_at((b - 1 + phi) * TSW, v, w), p)
                    new = capi.deskew_share(l[0], l[1])[0]
                    settled = abs(new - phi) < 1e-14
                    phi = new
                    if settled:
                        break
                assert settled, f"pole {k} of scan {b}: the sweep fraction does not settle (a pole at the seam)"
                l = to_local(pose_at((b - 1 + phi) * TSW, v, w), p)
            n = sigma * rng.standard_normal(2) if sigma else (0.0, 0.0)
            rows.append((l[0] + n[0], l[1] + n[1], p[2], rng.uniform(-0.3, 0.3)))
            pole.append(k), phis.append(phi)
        off.append(len(rows))
    rows, pole = np.array(rows, np.float32).reshape(-1, 4), np.array(pole, np.int64)
    m, inlier = tu.match_rows(off), np.zeros(off[-1], np.int32)
    for b in range(1, n_scans):
        before = {int(k): off[b - 1] + i for i, k in enumerate(pole[off[b - 1]:off[b]])}
        for r in range(off[b], off[b + 1]):
            t = before.get(int(pole[r]))
            if t is not None:
                m["train_row"][r], m["flags"][r], m["dist2"][r], inlier[r] = t, tu.ACC, 1.0, 1
    return dict(off=np.array(off, np.uint32), rows=rows, pole=pole, phi=np.array(phis), poles=poles, poses=poses, v=v, w=w, n_scans=n_scans,
                m=m, inlier=inlier)


def motion_record(yaw, tx, ty, tz=0.0, flags=capi.FX_REG_VALID):
    r = np.zeros(1, capi.REG_DTYPE)
    r[0] = (math.cos(yaw), math.sin(yaw), tx, ty, tz, 0.0, 10, 10, flags, 0, 1)
    return r


def per_scan_motions(wd):
    """The exact motion of every scan over one period (FX_DESKEW_PER_SCAN): the frame at the stamp in the frame a period before;
    under a constant twist that is pose_at(TSW) for every scan."""
    return np.concatenate([motion_record(*pose_at(TSW, wd["v"], wd["w"])) for _ in range(wd["n_scans"])])


def link_motions(wd):
    """The exact link records "scan p + 1 -> scan p" (FX_DESKEW_LINKS) between the true poses at the stamps."""
    return np.concatenate([motion_record(*pose_at(TSW, wd["v"], wd["w"])) for _ in range(wd["n_scans"] - 1)])


def exact_rows(wd, rows=None):
    """The exact constant-twist correction of the world's rows in closed form: a row seen at sweep fraction phi is
    (phi - 1) TSW away from the stamp, and the frame then in the frame at the stamp is pose_at of that (negative) time.  The sweep
    fraction is taken from the row itself, as the call must."""
    rows = wd["rows"] if rows is None else rows
    out = np.zeros((len(rows), 2))
    for i, (x, y) in enumerate(rows[:, :2].astype(np.float64)):
        a = capi.deskew_share(x, y)[1]
        out[i] = to_world(pose_at(a * TSW, wd["v"], wd["w"]), (x, y))
    return out


def under_true_pose(wd, xy):
    """Distance of every row (xy: [N, 2], in its scan's frame) from its pole under the scan's true pose at the stamp."""
    off = [int(x) for x in wd["off"]]
    d = np.zeros(len(xy))
    for b in range(wd["n_scans"]):
        for r in range(off[b], off[b + 1]):
            wx, wy = to_world(wd["poses"][b], xy[r])
            d[r] = math.hypot(wx - wd["poles"][wd["pole"][r], 0], wy - wd["poles"][wd["pole"][r], 1])
    return d


def fit(q, t):
    """The least-squares rigid motion (c, s, tx, ty) that takes the points q [n, 2] onto t [n, 2]."""
    qc, tc = q.mean(0), t.mean(0)
    u, v = q - qc, t - tc
    sd, sc = (u * v).sum(), (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]).sum()
    n = math.hypot(sd, sc)
    c, s = sd / n, sc / n
    return c, s, tc[0] - (c * qc[0] - s * qc[1]), tc[1] - (s * qc[0] + c * qc[1])


def pose_fits(wd, xy):
    """Every scan's rows fitted to their poles: (the largest distance of a fitted pose's origin from the true pose's, the smallest
    share of a scan's rows within 0.30 m of the fit)."""
    off = [int(x) for x in wd["off"]]
    worst, share = 0.0, 1.0
    for b in range(wd["n_scans"]):
        q = np.asarray(xy[off[b]:off[b + 1]], np.float64)
        t = wd["poles"][wd["pole"][off[b]:off[b + 1]], :2]
        c, s, tx, ty = fit(q, t)
        d = np.hypot(c * q[:, 0] - s * q[:, 1] + tx - t[:, 0], s * q[:, 0] + c * q[:, 1] + ty - t[:, 1])
        worst = max(worst, math.hypot(tx - wd["poses"][b][1], ty - wd["poses"][b][2]))
        share = min(share, float((d <= 0.30).mean()))
    return worst, share


def block(wd, max_scans=None, max_total=None, rows=None):
    """(the world's keypoint block as tu.block builds it, max_scans, max_total)"""
    max_scans = wd["n_scans"] + 2 if max_scans is None else max_scans
    max_total = len(wd["rows"]) + 9 if max_total is None else max_total
    return tu.block(wd["off"], wd["rows"] if rows is None else rows, max_scans, max_total), max_scans, max_total


def block_rows(blk, max_scans, max_total, n):
    """The first n rows of a block's keypoint area, [n, 4] float32."""
    k0 = capi.keypoint_block_layout(max_scans, max_total).k0
    return np.ascontiguousarray(blk).view(np.uint8).reshape(-1)[16 * k0:16 * (k0 + n)].view(np.float32).reshape(n, 4).copy()


def register(wd, rows):
    """capi.register_reference over pairs_consecutive of the world with `rows` in the place of its rows."""
    return capi.register_reference(rows, rows, wd["m"], capi.pairs_consecutive(wd["off"]))


def special_rows(rng):
    """[30, 4] float32 rows at the edges of the turn and of the correction: on the axes and the diagonals, at +-0, denormal, at 1e30,
    with a NaN or an infinite coordinate (copied), with a NaN elevation (corrected, the word kept); three ordinary rows at the end."""
    nan, inf, den = float("nan"), float("inf"), 1e-45
    xy = [(10, 0), (-10, 0), (0, 10), (0, -10), (7, 7), (-7, 7), (-7, -7), (7, -7),
          (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (-0.0, 5), (5, -0.0), (-5, -0.0),
          (den, 3), (3, den), (den, den), (den, -2 * den), (1e30, 1), (1, -1e30), (1e30, 1e30), (-1e30, den)]
    rows = np.zeros((30, 4), np.float32)
    rows[:, :2] = rng.uniform(-40, 40, (30, 2))
    rows[:, 2], rows[:, 3] = rng.uniform(-1, 2, 30), rng.uniform(-0.3, 0.3, 30)
    rows[:len(xy), :2] = xy
    rows[23, 0], rows[24, 1], rows[25, 2], rows[26, 3] = nan, inf, -inf, nan
    return rows


def hand_case(rng, counts=(7, 0, 30, 5, 6), max_scans=None, max_total=None):
    """Scans of counts[b] random rows, special_rows in the scan of 30: (block, max_scans, max_total, off, rows)."""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    N = int(off[-1])
    rows = np.zeros((N, 4), np.float32)
    rows[:, :2], rows[:, 2], rows[:, 3] = rng.uniform(-40, 40, (N, 2)), rng.uniform(-1, 2, N), rng.uniform(-0.3, 0.3, N)
    b = list(counts).index(30)
    rows[int(off[b]):int(off[b + 1])] = special_rows(rng)
    max_scans = len(counts) + 2 if max_scans is None else max_scans
    max_total = N + 9 if max_total is None else max_total
    return tu.block(off, rows, max_scans, max_total), max_scans, max_total, off, rows


def random_motions(rng, n, flags=capi.FX_REG_VALID):
    """n plausible motion records: up to 0.1 rad and 3 m a period."""
    return np.concatenate([motion_record(rng.uniform(-0.1, 0.1), rng.uniform(-3, 3), rng.uniform(-0.5, 0.5), rng.uniform(-0.1, 0.1), flags)
                           for _ in range(n)])


def link_cases(rng, n=5):
    """Motion records and options at every branch of "The motion of scan b", for a block of n >= 4 scans:
    [(what, motions, n_scans, opts, the flags the n_scans records must carry)]."""
    MV, NX, NM = capi.FX_DESKEW_MOVED, capi.FX_DESKEW_NEXT_LINK, capi.FX_DESKEW_NO_MOTION
    V, T = capi.FX_REG_VALID, capi.FX_REG_TRUNCATED
    base = random_motions(rng, n)
    cases = [("every link good", base.copy(), n, {}, [MV | NX] + [MV] * (n - 1))]
    m = base.copy()
    m["flags"][1] = 0
    cases.append(("previous bad, next good", m, n, {}, [MV | NX, MV, MV | NX] + [MV] * (n - 3)))
    m = base.copy()
    m["flags"][1] = m["flags"][2] = 0
    cases.append(("both bad", m, n, {}, [MV | NX, MV, NM, MV | NX] + [MV] * (n - 4)))
    m = base.copy()
    m["flags"][0] = m["flags"][n - 2] = 0
    cases.append(("the first and the last link bad", m, n, {}, [NM, MV | NX] + [MV] * (n - 3) + [NM]))
    for what, field, value in (("c == 0", "c", 0.0), ("c < 0", "c", -0.5), ("c NaN", "c", np.nan), ("s inf", "s", np.inf), ("tx NaN", "tx", np.nan),
                               ("ty -inf", "ty", -np.inf), ("tz NaN", "tz", np.nan)):
        m = base.copy()
        m[field][1] = value
        cases.append((f"link 1 with {what}", m, n, {}, [MV | NX, MV, MV | NX] + [MV] * (n - 3)))
    m = base.copy()
    m["flags"][:n - 1] = [V | T, V, T, 0][:n - 1] + [V | T] * (n - 5)  # (record n - 1 is no link: nobody reads it)
    cases.append(("require_flags VALID | TRUNCATED", m, n, dict(require_flags=V | T), [MV | NX, MV, NM, NM] + [MV | NX if n > 5 else NM] + [MV] * (n - 5)))
    cases.append(("require_flags 0", m, n, dict(require_flags=0), [MV | NX] + [MV] * (n - 1)))
    cases.append(("S = 1 without records", None, 1, {}, [NM]))
    p = random_motions(rng, n)
    p["flags"][2], p["c"][3] = 0, -1.0
    cases.append(("per scan", p, n, dict(source=capi.FX_DESKEW_PER_SCAN), [MV, MV, NM, NM] + [MV] * (n - 4)))
    return cases


def assert_equal(got_block, got_rec, ref_block, ref_rec, what=""):
    """The device's block and records against capi.deskew_reference's: every byte of the block, every field of every record
    (max_shift bit for bit)."""
    g, r = np.ascontiguousarray(got_block).view(np.uint8).reshape(-1), np.ascontiguousarray(ref_block).view(np.uint8).reshape(-1)
    assert g.shape == r.shape, f"{what}: block of {g.shape} bytes, reference {r.shape}"
    bad = np.flatnonzero((g != r).reshape(-1, 16).any(axis=1))
    assert not len(bad), f"{what}: block rows {bad[:8].tolist()} differ: got {g.view(np.float32).reshape(-1, 4)[bad[:4]]}, reference {r.view(np.float32).reshape(-1, 4)[bad[:4]]}"
    assert got_rec.shape == ref_rec.shape, f"{what}: {got_rec.shape} records, reference {ref_rec.shape}"
    for f in capi.DESKEW_DTYPE.names:
        bad = np.flatnonzero(tu.bits(got_rec[f]) != tu.bits(ref_rec[f]))
        assert not len(bad), f"{what}: {f} differs at {bad[:8].tolist()}: got {got_rec[bad[:4]]}, reference {ref_rec[bad[:4]]}"
