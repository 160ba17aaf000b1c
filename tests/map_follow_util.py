"""Helpers of the map follow tests (tests/test_map_follow_reference.py, tests/test_gpu_map_follow.py): the clean world of the
localise tests driven a second time with biased odometry, its variants with unusable links and empty scans, the dead-reckoned
priors the follow replaces, and the comparison of a device result with capi.map_follow_reference bit for bit."""
import math

import numpy as np

from feature_extraction_amd import capi
from tests import map_localize_util as lu
from tests import map_util as mu
from tests import track_util as tu

SIGMA = 0.01
SEEDS = (0, 1, 2, 5)
INLIER_DIST = 0.30
START, LINK, COASTED, HELD, LOST = (capi.FX_FOLLOW_START, capi.FX_FOLLOW_LINK, capi.FX_FOLLOW_COASTED, capi.FX_FOLLOW_HELD,
                                    capi.FX_FOLLOW_LOST)
NONE = capi.FX_FOLLOW_NO_MOTION


def spaced_seeds(below=6):
    """The seeds < below whose 40 poles are all more than 2 inlier_dist apart (test_map_localize_reference._world_seed's rule)."""
    out = []
    for seed in range(below):
        p = np.random.default_rng(seed).uniform(0, 100.0, (lu.WORLD["n_poles"], 2))  # (world()'s first draw)
        d = np.hypot(p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1]) + 1e9 * np.eye(len(p))
        if d.min() > 2 * INLIER_DIST:
            out.append(seed)
    return tuple(out)


def biased_links(w, scale=1.04, turn_deg=0.6):
    """The links of a second drive over w's trajectory with an odometry bias: every link `scale` long and turned turn_deg to the left."""
    return tu.reg_records([(yaw + math.radians(turn_deg), scale * tx, scale * ty, scale * tz) for yaw, tx, ty, tz in tu.relative(w["truth"])])


def world(seed):
    """(w, the map's state built from the clean run, the biased links, the start pose [1]) of the issue's world."""
    w, pieces = lu.clean_world(seed, SIGMA)
    st, _, _ = mu.run_reference(pieces, lu.WORLD["cap"], lu.WORLD["carry"])
    return w, st, biased_links(w), lu.poses_of(w["truth"][:1])


def dead_reckoned(start, links, n_scans):
    """The priors the library could produce before: the track's fold of the links from one start pose."""
    P = np.zeros(n_scans, capi.POSE_DTYPE)
    P[0] = start
    pc, ps, ptx, pty, ptz = (float(start[f]) for f in ("c", "s", "tx", "ty", "tz"))
    for b in range(1, n_scans):
        rc, rs, rtx, rty, rtz = (float(links[f][b - 1]) for f in ("c", "s", "tx", "ty", "tz"))
        pc, ps, ptx, pty, ptz = pc * rc - ps * rs, ps * rc + pc * rs, (pc * rtx - ps * rty) + ptx, (ps * rtx + pc * rty) + pty, ptz + rtz
        P[b] = (pc, ps, ptx, pty, ptz, 0, 0)
    return P


def without_rows(w, empty):
    """(kp_offset, rows) of w with the scans `empty` holding no rows."""
    off = [int(x) for x in w["off"]]
    keep = [w["rows"][off[b]:off[b + 1]] if b not in empty else w["rows"][:0] for b in range(w["n_scans"])]
    return np.concatenate([[0], np.cumsum([len(k) for k in keep])]).astype(np.uint32), np.concatenate(keep)


def separate_chains(st, off, rows, links, starts, n_scans, L, **opts):
    """The chains of chain_scans = L as one capi.map_follow_reference call each over the chain's own block."""
    off = [int(x) for x in off]
    outs = []
    for j, f in enumerate(range(0, n_scans, L)):
        e = min(f + L, n_scans)
        o = np.array(off[f:e + 1], np.uint32) - np.uint32(off[f])
        outs.append(capi.map_follow_reference(st, o, rows[off[f]:off[e]], links[f:e - 1], starts[j:j + 1], e - f, **opts))
    return outs


def assert_equal(got, ref, what=""):
    """{"rec", "follow", "poses", "map_id_of_row", "nearest_of_row"} of the device against the reference's: every byte."""
    lu.assert_equal(got, ref, what)
    for k, dt in (("follow", capi.FOLLOW_DTYPE), ("poses", capi.POSE_DTYPE)):
        if got.get(k) is None:
            continue
        g, r = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert g.shape == r.shape, f"{what}: {k} {g.shape} != {r.shape}"
        bad = [b for b in range(len(g)) if g[b].tobytes() != r[b].tobytes()]
        assert not bad, f"{what}: {k} differs at scans {bad[:8]}: got {g[bad[:2]]}, reference {r[bad[:2]]}"
