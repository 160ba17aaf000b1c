"""Helpers of the segment join tests (tests/test_map_join_reference.py, tests/test_gpu_map_join.py): the clean world with one
link made bad (two segments a held pose apart), hand-built maps of several segments, and the comparison of a device result with
capi.map_join_reference bit for bit."""
import math

import numpy as np

from feature_extraction_amd import capi
from tests import map_merge_util as mm
from tests import map_util as mu
from tests import track_util as tu

# the world of the issue: 40 poles, 24 scans, sigma 0.01, cut every 5 scans; the link scan BAD + 1 -> scan BAD is made unusable.
# The trajectory is a circle about the field's centre, so the held pose leaves the second segment turned about that centre by one
# step (0.205 rad): under the identity prior only the poles within search_dist / 0.205 = 9.8 m of the centre find their twin.  SEED
# is the first seed whose world has enough of them for the consensus (searched on the CPU; BAD lies inside a batch).
WORLD = dict(seed=10, bad=12, n_poles=40, n_scans=24, sigma=0.01, step=5, cap=256, carry=64)
F32 = lambda v: float(np.float32(v))


def world(seed=None, bad=None):
    """(w, pieces of the broken run, pieces of the unbroken run): track_util.world cut every 5 scans, once with the registration
    record of link `bad` cleared of FX_REG_VALID and once as it is."""
    f = WORLD
    seed, bad = f["seed"] if seed is None else seed, f["bad"] if bad is None else bad
    w = tu.world(np.random.default_rng(seed), f["n_poles"], f["n_scans"], sigma=f["sigma"])
    edges = mu.every(f["n_scans"], f["step"])
    whole = mu.split(w, edges)
    broken = dict(w, reg=w["reg"].copy())
    broken["reg"]["flags"][bad] &= ~np.uint32(capi.FX_REG_VALID)
    return w, mu.split(broken, edges), whole


def poles_of(w, pieces, ids, n):
    """pole of each of the n landmarks of a run from its pieces' map_id_of_row (every row of a landmark is of one pole)."""
    out = np.full(n, -1, np.int64)
    for p, row_ids in zip(pieces, ids):
        k = len(p["rows"])
        has = row_ids[:k] >= 0
        pole = w["pole"][p["row0"]:p["row0"] + k][has]
        old = out[row_ids[:k][has]]
        assert ((old == -1) | (old == pole)).all()
        out[row_ids[:k][has]] = pole
    return out


def live(state):
    """ids of the live landmarks of a state."""
    a = list(state.get("alias", [])) + [-1] * (len(state["landmarks"]) - len(state.get("alias", [])))
    return [i for i in range(len(state["landmarks"])) if a[i] == -1]


def set_segments(state, segs, segments=None):
    """A copy of the state with the landmarks' segments as given and header.segments (default: the highest + 1)."""
    st = dict(state, header=dict(state["header"]), landmarks=[dict(r) for r in state["landmarks"]])
    for r, s in zip(st["landmarks"], segs):
        r["segment"] = int(s)
    st["header"]["segments"] = int(max(segs) + 1 if segments is None else segments)
    return st


def two_segments(n_src, n_dst, shift=(0.5, -0.25), pitch=4.0, interleave=True, seed=5, jitter=0.0):
    """A hand-built state of n_dst landmarks on a lattice (segment 0) and n_src twins of the first of them moved by `shift`
    (segment 1) (+ jitter * (k % 7) in x: the association distances then differ), two observations each, ids of the two segments
    interleaved while both last.  Returns the state."""
    side = int(math.ceil(math.sqrt(max(n_dst, 1))))
    dst = [(0, F32(pitch * (k % side)), F32(pitch * (k // side))) for k in range(n_dst)]
    src = [(0, F32(dst[k % n_dst][1] + shift[0] + jitter * (k % 7)), F32(dst[k % n_dst][2] + shift[1])) for k in range(n_src)]
    frags, segs = [], []
    for k in range(max(n_src, n_dst)):
        for arr, sg in ((dst, 0), (src, 1)) if interleave else ():
            if k < len(arr):
                frags.append(arr[k]), segs.append(sg)
    if not interleave:
        frags, segs = dst + src, [0] * n_dst + [1] * n_src
    st, _ = mm.reference_of(mm.fragments(frags, 3, seed=seed), cap=len(frags) + 3, carry=8)
    return set_segments(st, segs)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def assert_result(got, ref, what=""):
    """A device result record against the reference's: integers equal, doubles and rms as bit patterns."""
    for f in capi.JOIN_DTYPE.names:
        a, b = np.atleast_1d(got[f]), np.atleast_1d(ref[f])
        a, b = (a, b) if a.dtype.kind == "u" else (bits(a), bits(b))
        assert (a == b).all(), f"{what}: result.{f}: got {got[f]!r}, reference {ref[f]!r}"
