"""Helpers of the map localisation tests (tests/test_map_localize_reference.py, tests/test_gpu_map_localize.py): the clean world
of the issue with disturbed priors, hand-built maps (map_merge_util.fragments through track -> map) with hand-built scans to
localise, and the comparison of a device result with capi.map_localize_reference bit for bit."""
import math

import numpy as np

from feature_extraction_amd import capi
from tests import map_merge_util as mm
from tests import map_util as mu
from tests import track_util as tu

WORLD = dict(n_poles=40, n_scans=24, step=5, cap=128, carry=64)
F32 = lambda v: float(np.float32(v))


def clean_world(seed, sigma):
    """track_util.world: 40 poles, 24 scans, no dropout, cut every 5 scans.  Returns (w, pieces)."""
    w = tu.world(np.random.default_rng(seed), WORLD["n_poles"], WORLD["n_scans"], sigma=sigma)
    return w, mu.split(w, mu.every(WORLD["n_scans"], WORLD["step"]))


def poses_of(truth, seed=None, yaw_deg=1.0, shift=0.5):
    """POSE_DTYPE records of the truth [(yaw, x, y, z)]; with a seed each turned by +-yaw_deg and shifted by +-shift in x and in y,
    the three signs from a seeded draw per scan."""
    P = np.zeros(len(truth), capi.POSE_DTYPE)
    sign = np.ones((len(truth), 3)) * 0.0 if seed is None else np.random.default_rng(seed).choice([-1.0, 1.0], (len(truth), 3))
    for b, (yaw, x, y, z) in enumerate(truth):
        a = yaw + sign[b, 0] * math.radians(yaw_deg)
        P[b] = (math.cos(a), math.sin(a), x + sign[b, 1] * shift, y + sign[b, 2] * shift, z, 0, 0)
    return P


def pose_errors(poses, truth):
    """(worst xy distance, worst |z|, worst yaw difference) of POSE_DTYPE records from the truth."""
    dxy = max(math.hypot(p["tx"] - x, p["ty"] - y) for p, (_, x, y, _z) in zip(poses, truth))
    dz = max(abs(p["tz"] - z) for p, (_, _x, _y, z) in zip(poses, truth))
    dyaw = max(tu.yaw_err(math.atan2(p["s"], p["c"]), yaw) for p, (yaw, _x, _y, _z) in zip(poses, truth))
    return dxy, dz, dyaw


def scans(rows_by_scan):
    """(kp_offset, rows [n, 4] float32) of scans given as lists of (x, y, z)."""
    off = np.concatenate([[0], np.cumsum([len(s) for s in rows_by_scan])]).astype(np.uint32)
    rows = np.zeros((int(off[-1]), 4), np.float32)
    flat = [p for s in rows_by_scan for p in s]
    if flat:
        rows[:, :3] = np.array(flat, np.float32)
    return off, rows


def identity(n, **fields):
    P = np.zeros(n, capi.POSE_DTYPE)
    P["c"] = 1.0
    for k, v in fields.items():
        P[k] = v
    return P


def lattice(n, pitch=4.0, side=None):
    """n landmark positions (first_scan 0) on a square lattice: float32-exact, `pitch` apart."""
    side = side or int(math.ceil(math.sqrt(n)))
    return [(0, F32(pitch * (k % side)), F32(pitch * (k // side))) for k in range(n)]


def rows_at(frags, which, dx=0.0, dy=0.0, z=1.0, grow=0.0):
    """Keypoint rows at the positions of fragments `which`, moved by (dx, dy) (+ grow * ordinal in x: the d2 of the association then
    ascends with the row)."""
    return [(F32(frags[k][1] + dx + grow * n), F32(frags[k][2] + dy), z) for n, k in enumerate(which)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def assert_equal(got, ref, what=""):
    """A device result {"rec", "map_id_of_row", "nearest_of_row"} against the reference's: integers equal, doubles and rms as bit
    patterns, both row arrays whole."""
    for k in ("nearest_of_row", "map_id_of_row"):
        if got.get(k) is None:
            continue
        bad = np.flatnonzero(got[k] != ref[k])
        assert got[k].shape == ref[k].shape and not len(bad), f"{what}: {k} differs at {bad[:8].tolist()}: got {got[k][bad[:8]]}, reference {ref[k][bad[:8]]}"
    g, r = got["rec"], ref["rec"]
    assert g.shape == r.shape, f"{what}: {g.shape} != {r.shape}"
    cols = [(f, g[f], r[f]) for f in capi.LOC_DTYPE.names if f != "pose"] + [("pose." + f, g["pose"][f], r["pose"][f]) for f in capi.POSE_DTYPE.names]
    for name, a, b in cols:
        a, b = (a, b) if a.dtype.kind == "u" else (bits(a), bits(b))
        bad = np.flatnonzero(a != b)
        assert not len(bad), f"{what}: {name} differs at scans {bad[:8].tolist()}: got {g[bad[:2]]}, reference {r[bad[:2]]}"


def assert_prior_kept(rec, priors, what=""):
    """Not VALID => the pose is the prior's bytes."""
    for b in range(len(rec)):
        if not rec["flags"][b] & capi.FX_LOC_VALID:
            assert rec["pose"][b].tobytes() == priors[b].tobytes(), f"{what}: scan {b} is not VALID and its pose is not the prior"


# ---- ties between samples of the consensus (k_loc_consensus deals its samples as k_register does, in fp64)
TIE_H = 128
TIE_SAMPLES = [(0, 1), (63, 64), (0, 255), (0, 256), (255, 256), (5, 8127), (4095, 4096)]
TIE_FRAGS = [(0, 0.0, 0.0), (0, 200.0, 0.0), (0, 210.0, 0.0), (0, 211.5, 0.0), (0, 200.0, 20.0), (0, 210.0, 20.0)]
TIE_OPTS = dict(hyp_corr=TIE_H, min_inliers=2)


def tie_scans():
    """A scan per (i, j) of TIE_SAMPLES: 128 rows, all in the pool, whose only live samples are i and j with 2 agreeing each.
    The row of pool rank r lies 1 + r / 256 m from its landmark, so d2 ranks it r, and rows run against the ranks.  Junk rows
    all sit west of landmark 0: two of them share the landmark (lt2 = 0: the baseline gate), and with a carrier, 200 m east and
    moved north or south, the row side is about a metre longer than the landmark side (the length gate).  Carriers are moved
    along y by their own distance: two moved the same way differ by a small rotation and agree with their own sample only;
    moved opposite ways they are 3 m apart in length (landmarks 1 and 4) or, 11.5 m apart in x, just inside the gate (1 and 3:
    the samples that share a member); landmarks 2 and 3 are 1.5 m apart: no sample.  Returns (rows by scan, [(hyp_a, hyp_b)] as
    rows of the scan)."""
    from tests import register_util as ru
    scans_, want = [], []
    for i, j in TIE_SAMPLES:
        (ai, bi), (aj, bj) = ru.ranks_of(TIE_H, i), ru.ranks_of(TIE_H, j)
        shared = set((ai, bi)) & set((aj, bj))
        if shared:
            s, = shared
            x, = set((ai, bi)) - shared
            y, = set((aj, bj)) - shared
            car = {s: (1, 1.0), x: (2, 1.0), y: (3, -1.0)}
        else:
            car = {ai: (1, 1.0), bi: (2, 1.0), aj: (4, -1.0), bj: (5, -1.0)}
        rows = []
        for r in range(TIE_H):
            d = 1.0 + r / 256.0
            if r in car:
                k, sign = car[r]
                rows.append((TIE_FRAGS[k][1], F32(TIE_FRAGS[k][2] + sign * d), 1.0))
            else:
                rows.append((F32(-d), 0.0, 1.0))
        scans_.append(rows[::-1])
        want.append((TIE_H - 1 - ai, TIE_H - 1 - bi))
    return scans_, want
