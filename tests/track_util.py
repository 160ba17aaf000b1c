"""Helpers of the tracking tests (tests/test_track_reference.py, tests/test_gpu_track.py): a synthetic world of poles seen from a
known trajectory, hand-built blocks of scans with chosen links, random link structures, and the field-by-field comparison with
capi.track_reference.  The fx_match records, inlier words and fx_registration records are built from the truth, the way
register_util.records builds match records."""
import math
import os

import numpy as np

from feature_extraction_amd import capi
from tests import register_util as ru

ACC = capi.FX_MATCH_ACCEPTED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def match_rows(off):
    """The fx_match records a match over pairs_consecutive(off) leaves before any row found a partner: pair = scan - 1 for the rows
    of scans >= 1, no pair for scan 0's, train_row -1."""
    off = [int(x) for x in off]
    m = ru.records(off[-1], -1, np.inf, flags=0, pair=capi.FX_MATCH_NO_PAIR)
    for b in range(1, len(off) - 1):
        m["pair"][off[b]:off[b + 1]] = b - 1
    return m


def reg_records(motions, flags=capi.FX_REG_VALID):
    """fx_registration records of the motions [(yaw, tx, ty, tz)]: what a register that found them exactly would leave."""
    r = np.zeros(len(motions), capi.REG_DTYPE)
    for p, (yaw, tx, ty, tz) in enumerate(motions):
        r[p] = (math.cos(yaw), math.sin(yaw), tx, ty, tz, 0.0, 10, 10, flags, 0, 1)
    return r


def relative(poses):
    """The motions scan p + 1 -> scan p, (yaw, tx, ty, tz), between the absolute poses [(yaw, x, y, z)] (scan -> world)."""
    out = []
    for (ya, xa, ya_, za), (yb, xb, yb_, zb) in zip(poses[:-1], poses[1:]):
        c, s = math.cos(ya), math.sin(ya)
        dx, dy = xb - xa, yb_ - ya_
        out.append((yb - ya, c * dx + s * dy, -s * dx + c * dy, zb - za))
    return out


def world(rng, n_poles, n_scans, field=100.0, reach=35.0, dropout=0.0, sigma=0.0):
    """n_poles poles uniform in a field x field square (z in [0, 2]) seen from a trajectory of n_scans poses on a circle of radius
    field / 4 about the centre, heading along it, the first pose taken as the common frame.  A scan holds, in shuffled row order,
    the poles within `reach` of the sensor that did not drop out, in the sensor's frame, rounded to float32 (plus Gaussian noise
    sigma).  A row whose pole is also in the scan before is matched to that row and is an inlier.
    Returns a dict: off, rows [N, 4] float32, pole [N] the pole of each row, m, inlier, reg, truth (the poses relative to the
    first: [(yaw, x, y, z)]), n_scans."""
    poles = np.concatenate([rng.uniform(0, field, (n_poles, 2)), rng.uniform(0, 2, (n_poles, 1))], axis=1)
    R0 = field / 4
    ang = np.linspace(0.0, 1.5 * math.pi, n_scans) if n_scans > 1 else np.zeros(1)
    absolute = [(a + math.pi / 2, field / 2 + R0 * math.cos(a), field / 2 + R0 * math.sin(a), 0.01 * b) for b, a in enumerate(ang)]
    y0, x0, y0_, z0 = absolute[0]
    c0, s0 = math.cos(y0), math.sin(y0)
    truth = [(y - y0, c0 * (x - x0) + s0 * (y_ - y0_), -s0 * (x - x0) + c0 * (y_ - y0_), z - z0) for y, x, y_, z in absolute]
    off, rows, pole = [0], [], []
    for yaw, x, y, z in absolute:
        d = poles[:, :2] - (x, y)
        seen = np.flatnonzero((np.hypot(d[:, 0], d[:, 1]) <= reach) & (rng.random(n_poles) >= dropout))
        seen = seen[rng.permutation(len(seen))]
        c, s = math.cos(yaw), math.sin(yaw)
        loc = np.zeros((len(seen), 4), np.float32)
        loc[:, 0], loc[:, 1], loc[:, 2] = c * d[seen, 0] + s * d[seen, 1], -s * d[seen, 0] + c * d[seen, 1], poles[seen, 2] - z
        if sigma:
            loc[:, :3] += (sigma * rng.standard_normal((len(seen), 3))).astype(np.float32)
        loc[:, 3] = rng.uniform(-0.3, 0.3, len(seen))  # (elevation: not a coordinate)
        rows.append(loc), pole.append(seen), off.append(off[-1] + len(seen))
    rows, pole = np.concatenate(rows), np.concatenate(pole)
    m, inlier = match_rows(off), np.zeros(off[-1], np.int32)
    for b in range(1, n_scans):
        before = {int(k): off[b - 1] + i for i, k in enumerate(pole[off[b - 1]:off[b]])}
        for r in range(off[b], off[b + 1]):
            t = before.get(int(pole[r]))
            if t is not None:
                m["train_row"][r], m["flags"][r], m["dist2"][r], inlier[r] = t, ACC, 1.0, 1
    return dict(off=np.array(off, np.uint32), rows=rows, pole=pole, m=m, inlier=inlier, reg=reg_records(relative(truth)), truth=truth,
                n_scans=n_scans)


def pole_runs(w, good=None):
    """The sets of rows a tracker must find in world w: per pole, its rows over each maximal run of consecutive scans that see it
    (split at links that are not good)."""
    off, runs = [int(x) for x in w["off"]], []
    last = {}  # pole -> (scan of its latest row, the run)
    for b in range(w["n_scans"]):
        for r in range(off[b], off[b + 1]):
            k = int(w["pole"][r])
            if k in last and last[k][0] == b - 1 and (good is None or good[b - 1]):
                last[k][1].append(r)
                last[k] = (b, last[k][1])
            else:
                runs.append([r])
                last[k] = (b, runs[-1])
    return runs


class Hand:
    """A block of scans built row by row: chains of chosen length, rows with chosen parents."""

    def __init__(self, n_scans):
        self.count = [0] * n_scans
        self.links = []  # ((scan, i) child, (scan, i) parent)

    def new(self, b):
        self.count[b] += 1
        return (b, self.count[b] - 1)

    def chain(self, first_scan, length):
        """A chain of `length` rows from first_scan on, a row a scan; returns them."""
        rows = [self.new(first_scan + d) for d in range(length)]
        self.links += list(zip(rows[1:], rows[:-1]))
        return rows

    def child(self, parent):
        r = self.new(parent[0] + 1)
        self.links.append((r, parent))
        return r

    def finish(self, rng, motions=None):
        """-> dict like world()'s (without pole / truth) and `at`, the row index of a (scan, i)."""
        n = len(self.count)
        off = np.concatenate([[0], np.cumsum(self.count)]).astype(np.uint32)
        rows = np.zeros((int(off[-1]), 4), np.float32)
        rows[:, :2], rows[:, 2], rows[:, 3] = rng.uniform(-40, 40, (len(rows), 2)), rng.uniform(-1, 2, len(rows)), rng.uniform(-0.3, 0.3, len(rows))
        at = lambda bi: int(off[bi[0]]) + bi[1]
        m, inlier = match_rows(off), np.zeros(len(rows), np.int32)
        for c, p in self.links:
            m["train_row"][at(c)], m["flags"][at(c)], m["dist2"][at(c)], inlier[at(c)] = at(p), ACC, 1.0, 1
        if motions is None:
            motions = [(rng.uniform(-0.1, 0.1), rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-0.1, 0.1)) for _ in range(n - 1)]
        return dict(off=off, rows=rows, m=m, inlier=inlier, reg=reg_records(motions), n_scans=n, at=at)


def random_case(rng, counts, p_link=0.7, p_bad=0.0):
    """Scans of counts[b] random rows; every row of a scan >= 1 proposes, with probability p_link, a random row of the scan before
    (several may pick the same: conflicts); every link is bad (not VALID) with probability p_bad."""
    n = len(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    N = int(off[-1])
    rows = np.zeros((N, 4), np.float32)
    rows[:, :2], rows[:, 2], rows[:, 3] = rng.uniform(-40, 40, (N, 2)), rng.uniform(-1, 2, N), rng.uniform(-0.3, 0.3, N)
    m, inlier = match_rows(off), np.zeros(N, np.int32)
    for b in range(1, n):
        lo, hi, plo, phi = int(off[b]), int(off[b + 1]), int(off[b - 1]), int(off[b])
        if hi > lo and phi > plo:
            pick = rng.random(hi - lo) < p_link
            m["train_row"][lo:hi] = np.where(pick, rng.integers(plo, phi, hi - lo), -1)
            m["flags"][lo:hi] = np.where(pick, ACC, 0)
            inlier[lo:hi] = pick
    reg = reg_records([(rng.uniform(-0.1, 0.1), rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-0.1, 0.1)) for _ in range(n - 1)])
    if n > 1:
        reg["flags"][rng.random(n - 1) < p_bad] = 0
    return dict(off=off, rows=rows, m=m, inlier=inlier, reg=reg, n_scans=n)


def reference(w, n_scans=None, q_max_rows=None, stored=None, **kw):
    """capi.track_reference on a case dict; q_max_rows cuts (or pads with no-pair records) the per-row inputs, stored cuts the
    keypoint rows, as a block that stores fewer would."""
    m, inl = padded(w, q_max_rows)
    rows = w["rows"] if stored is None else w["rows"][:stored]
    return capi.track_reference(w["off"], rows, m, inl, w["reg"], w["n_scans"] if n_scans is None else n_scans, **kw)


def padded(w, q_max_rows=None):
    """(match records, inlier words) of the case cut or padded to q_max_rows."""
    n = len(w["m"]) if q_max_rows is None else int(q_max_rows)
    m = ru.records(n, -1, np.inf, flags=0, pair=capi.FX_MATCH_NO_PAIR)
    inl = np.zeros(n, np.int32)
    k = min(n, len(w["m"]))
    m[:k], inl[:k] = w["m"][:k], w["inlier"][:k]
    return m, inl


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def assert_equal(got, ref, what="", max_landmarks=None):
    """track_records' dict `got` against track_reference's `ref`: integers equal, doubles and rms_xy bit for bit."""
    assert got["header"] == ref["header"], f"{what}: header {got['header']} != {ref['header']}"
    for k in ("landmark_of_row", "obs_row"):
        bad = np.flatnonzero(got[k] != ref[k])
        assert got[k].shape == ref[k].shape and not len(bad), f"{what}: {k} differs at {bad[:8].tolist()}: got {got[k][bad[:8]]}, reference {ref[k][bad[:8]]}"
    want = ref["landmarks"] if max_landmarks is None else ref["landmarks"][:max_landmarks]
    for name, g, w_ in (("poses", got["poses"], ref["poses"]), ("landmarks", got["landmarks"], want)):
        assert g.shape == w_.shape, f"{what}: {name} {g.shape} != {w_.shape}"
        for f in g.dtype.names:
            a, b = (g[f], w_[f]) if g[f].dtype.kind == "u" else (bits(g[f]), bits(w_[f]))
            bad = np.flatnonzero(a != b)
            assert not len(bad), f"{what}: {name}.{f} differs at {bad[:8].tolist()}: got {g[bad[:4]]}, reference {w_[bad[:4]]}"


def block(off, rows, max_scans, max_total, stored=None):
    """The keypoint block fx_pack_keypoint_block would write for scans at kp_offset `off` holding `rows` ([n, 4] float32), laid out
    for (max_scans, max_total), as a uint8 array.  stored: the block's "keypoints stored" word (default all); the rows from there
    on are filled with a byte pattern nobody may read."""
    off = [int(x) for x in off]
    n, scans = len(rows), len(off) - 1
    stored = n if stored is None else int(stored)
    assert scans <= max_scans and n <= max_total and stored <= n
    k0, n_rows = capi.keypoint_block_layout(max_scans, max_total)
    blk = np.zeros((n_rows, 4), np.float32)
    u = blk.view(np.uint32).reshape(-1)
    u[:4] = (scans, stored, 0, max_total)
    u[4:4 + scans + 1] = off
    u[4 + scans + 1:capi.keypoint_block_layout(max_scans, max_total).f0] = off[-1]  # entries beyond the batch repeat the total
    blk[k0:k0 + n] = rows
    blk[k0 + stored:].view(np.uint8)[:] = 0xA5
    return blk.view(np.uint8).reshape(-1)


EDGE_OFF = (0, 2, 2, 5)  # three scans, the one in the middle empty


def edge_blocks(rows):
    """The smallest block at the edges that block() cannot build, for every call that reads a block as a query (fx_track_landmarks,
    fx_map_localize, fx_map_relocalize, fx_map_observe, fx_map_expect: one device definition, csrc/fx_scan_query.h, serves them all).
    rows: [5, 4] float32, the rows of three scans at EDGE_OFF.  Yields dicts: what, blk (the block's bytes), max_scans, max_total (its
    layout), and off, rows: what the call's numpy reference is given (the rows cut to min(stored, max_total))."""
    rows = np.ascontiguousarray(rows, np.float32)
    assert rows.shape == (5, 4)
    blk = block(EDGE_OFF, rows, 3, 5)
    blk.view(np.uint32)[0] = 4
    yield dict(what="a header of 4 scans in a block of max_scans 3", blk=blk, max_scans=3, max_total=5, off=list(EDGE_OFF), rows=rows)
    blk = block(EDGE_OFF, rows[:4], 3, 4)
    blk.view(np.uint32)[1] = 5
    yield dict(what="max_total 4 below the 5 rows stored", blk=blk, max_scans=3, max_total=4, off=list(EDGE_OFF), rows=rows[:4])
    yield dict(what="kp_offset 0 3 2 5", blk=block((0, 3, 2, 5), rows, 3, 5), max_scans=3, max_total=5, off=[0, 3, 2, 5], rows=rows)


# ---- the whole chain on rotated copies of a golden scan (tests/test_track_reference.py on the CPU, tests/test_gpu_track.py (f))
def yaw_err(a, b):
    return abs((a - b + math.pi) % (2 * math.pi) - math.pi)


def rotated_copies(n=5, step_deg=3.0):
    """Golden VLP-16 scan seed 1000 and n - 1 copies, each step_deg further about z than the last (fp64, rounded to fp32)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "vlp16_launch_seed1000.npz"))
    A = np.concatenate([g["points_xyz"], np.zeros((len(g["points_xyz"]), 1), np.float32)], axis=1)
    x, y = A[:, 0].astype(np.float64), A[:, 1].astype(np.float64)
    out = []
    for k in range(n):
        th = math.radians(step_deg * k)
        B = A.copy()
        B[:, 0], B[:, 1] = (math.cos(th) * x - math.sin(th) * y).astype(np.float32), (math.sin(th) * x + math.cos(th) * y).astype(np.float32)
        out.append(B)
    return out


def chain_checks(tr, reg, n_kp0, step_deg=3.0, n=5):
    """The bounds the rotated-copies chain is held to: every link FX_REG_VALID, the last pose within 5 x 0.30 m (error at 50 m plus
    translation), at least a third of scan 0's keypoints landmarks of n observations.  Returns (pose error, such landmarks, worst
    rms_xy)."""
    assert len(reg) == n - 1 and all(f & capi.FX_REG_VALID for f in reg["flags"]), reg["flags"]
    P = tr["poses"][n - 1]
    # scan k is scan 0 turned by k steps: its pose in scan 0's frame is the opposite rotation and no translation
    err = yaw_err(math.atan2(P["s"], P["c"]), -math.radians(step_deg * (n - 1))) * 50.0 + math.hypot(P["tx"], P["ty"])
    full = int((tr["landmarks"]["n_obs"] == n).sum())
    worst_rms = float(tr["landmarks"]["rms_xy"].max()) if len(tr["landmarks"]) else 0.0
    assert err <= 5 * 0.30 and 3 * full >= n_kp0, (err, full, n_kp0)
    return err, full, worst_rms
