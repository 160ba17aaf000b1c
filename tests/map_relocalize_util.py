"""Helpers of the map relocalisation tests (tests/test_map_relocalize_reference.py, tests/test_gpu_map_relocalize.py): hand-built
maps (map_merge_util.fragments through track -> map) with hand-built scans, the lattice cases of the issue, and the comparison of
a device result with capi.map_relocalize_reference bit for bit."""
import numpy as np

from feature_extraction_amd import capi
from tests import map_localize_util as lu
from tests import map_merge_util as mm

F32 = lu.F32
VALID, TRUNC, NOHYP, AMBIG, NOSCAN = (capi.FX_RELOC_VALID, capi.FX_RELOC_TRUNCATED, capi.FX_RELOC_NO_HYPOTHESIS, capi.FX_RELOC_AMBIGUOUS,
                                      capi.FX_RELOC_NO_SCAN)
# the off-lattice pole of the lattice case: 1.5 and 2.25 m from the lattice's lines, so no translation by the pitch and no quarter
# turn brings it within inlier_dist of a lattice point
LATTICE = dict(n=36, pitch=4.0, patch=[7, 8, 9, 13, 14, 15, 19, 20, 21], extra=(5.5, 6.25))


def state_of(frags, n_scans_map=3, bad=(), cap=None):
    """The map_reference state of one batch holding a two-observation landmark for every (first_scan, x, y) of frags."""
    st, _ = mm.reference_of(mm.fragments(frags, n_scans_map, bad), cap=cap or max(len(frags), 8), carry=8)
    return st


def lattice_case(extra):
    """(frags, rows of one scan): a 6 x 6 lattice 4 m apart and a scan of its inner 3 x 3 patch, seen from a pose 10 m east and 3 m
    north of the map's origin; with `extra` an off-lattice pole is in the map and in the scan."""
    L = LATTICE
    frags = lu.lattice(L["n"], L["pitch"])
    which = list(L["patch"])
    if extra:
        frags = frags + [(0, F32(L["extra"][0]), F32(L["extra"][1]))]
        which.append(L["n"])
    return frags, lu.rows_at(frags, which, -10.0, -3.0)


def random_field(n, seed, side=None):
    """n landmark positions (first_scan 0) uniform in a square of 1 pole per 250 m^2, float32 values."""
    rng = np.random.default_rng(seed)
    side = side or (250.0 * n) ** 0.5
    return [(0, F32(x), F32(y)) for x, y in rng.uniform(0.0, side, (n, 2))]


def view_of(frags, which, yaw, tx, ty, z=1.0):
    """Keypoint rows: the positions of fragments `which` seen from the pose (yaw, tx, ty) (float32 rounding of the inverse)."""
    c, s = np.cos(yaw), np.sin(yaw)
    out = []
    for k in which:
        dx, dy = frags[k][1] - tx, frags[k][2] - ty
        out.append((F32(c * dx + s * dy), F32(-s * dx + c * dy), z))
    return out


def assert_equal(got, ref, what=""):
    """A device result {"rec", "map_id_of_row"} against the reference's: integers equal, doubles as bit patterns, the row array
    whole."""
    bad = np.flatnonzero(got["map_id_of_row"] != ref["map_id_of_row"])
    assert got["map_id_of_row"].shape == ref["map_id_of_row"].shape and not len(bad), \
        f"{what}: map_id_of_row differs at {bad[:8].tolist()}: got {got['map_id_of_row'][bad[:8]]}, reference {ref['map_id_of_row'][bad[:8]]}"
    g, r = got["rec"], ref["rec"]
    assert g.shape == r.shape, f"{what}: {g.shape} != {r.shape}"
    cols = [(f, g[f], r[f]) for f in capi.RELOC_DTYPE.names if f != "pose"] + [("pose." + f, g["pose"][f], r["pose"][f]) for f in capi.POSE_DTYPE.names]
    for name, a, b in cols:
        a, b = (a, b) if a.dtype.kind == "u" else (lu.bits(a), lu.bits(b))
        bad = np.flatnonzero(a != b)
        assert not len(bad), f"{what}: {name} differs at scans {bad[:8].tolist()}: got {g[bad[:2]]}, reference {r[bad[:2]]}"


# ---- hand-built cases with known answers: the CPU test holds the reference to `expect`, the GPU test the device to the reference
def _ulps(v):
    """(v, the float32 below, the float32 above)"""
    v = np.float32(v)
    return float(v), float(np.nextafter(v, np.float32(-np.inf))), float(np.nextafter(v, np.float32(np.inf)))


EDGE = dict(inlier_dist=0.25, pair_tol=0.25, min_inliers=3)


def edge_cases():
    """name -> (frags, rows by scan, options, expect: field -> values by scan).  Float-exact coordinates (3-4-5 triangles, powers of
    two), inlier_dist = pair_tol = 0.25; every value sits exactly at a gate, one float32 below it and one above it."""
    out = {}
    far = [(0, 100.0, 100.0), (0, 140.0, 100.0), (0, 100.0, 130.0)]  # a map no seed of these scans can be laid on but once
    # a seed 5 m long (3-4-5) at min_baseline = 5 and at max_baseline = 5: mb mb <= d2 <= xb xb
    at, lo, hi = _ulps(3.0)
    two = [[(0.0, 0.0, 1.0), (x, 4.0, 1.0)] for x in (at, lo, hi)]
    out["min_baseline"] = (far, two, dict(EDGE, min_baseline=5.0, max_baseline=60.0), dict(n_seeds=[1, 0, 1]))
    out["max_baseline"] = (far, two, dict(EDGE, min_baseline=2.0, max_baseline=5.0), dict(n_seeds=[1, 1, 0]))
    # landmark pairs 5.25 m long (each on its own line y = 100 k, far from the others) under a seed of 5 m: |5 - 5.25| > 0.25 ?
    frags = [(0, x, 100.0 * k) for k, h in enumerate(_ulps(5.25)) for x in (0.0, h)]
    out["pair_tol"] = (frags, [[(0.0, 0.0, 1.0), (3.0, 4.0, 1.0)]], dict(EDGE, min_baseline=2.0, max_baseline=5.0),
                       dict(n_hyp=[4], hyp=[[(0, 0, 1), (0, 1, 0), (0, 2, 3), (0, 3, 2)]]))
    # the seed lies on landmarks 0 and 1 exactly (the identity: c = 1, s = tx = ty = 0), the third keypoint 0.25 m from landmark 2
    frags = [(0, 0.0, 0.0), (0, 3.0, 4.0), (0, 8.0, 0.0)]
    rows = [[(0.0, 0.0, 1.0), (3.0, 4.0, 1.0), (8.0, y, 1.0)] for y in _ulps(0.25)]
    out["inlier_dist"] = (frags, rows, dict(EDGE, min_baseline=2.0, max_baseline=5.0), dict(score=[3, 3, 2], lm_a=[0] * 3, lm_b=[1] * 3))
    # a second copy of the pattern moved along x by 2 inlier_dist = 0.5: its hypothesis puts a* (and b*) 0.5 m (- 2^-26, + 2^-25) from
    # where the winner does and scores 3 like it; every other hypothesis scores 2
    for name, x, runner in zip(("rival_at", "rival_below", "rival_above"), _ulps(0.5), (2, 2, 3)):
        frags = [(0, 0.0, 0.0), (0, 4.0, 0.0), (0, 2.0, 3.0), (0, x, 0.0), (0, 4.5, 0.0), (0, 2.5, 3.0)]
        out[name] = (frags, [[(0.0, 0.0, 1.0), (4.0, 0.0, 1.0), (2.0, 3.0, 1.0)]], dict(EDGE, min_baseline=3.75, max_baseline=4.0),
                     dict(score=[3], runner_up=[runner], lm_a=[0], lm_b=[1], flags=[AMBIG if runner == 3 else VALID]))
    return out


def check_expect(ref, expect, what=""):
    for f, want in expect.items():
        if f == "hyp":
            got = [sorted(zip(h["s"].tolist(), h["g"].tolist(), h["h"].tolist())) for h in ref["hyp"]]
            assert got == [sorted(w) for w in want], f"{what}: hypotheses {got}, expected {want}"
        else:
            assert ref["rec"][f].tolist() == want, f"{what}: {f} {ref['rec'][f].tolist()}, expected {want}"


def count_cases():
    """name -> (frags, rows by scan, options, expect): counts at their edges."""
    out = {}
    rng = np.random.default_rng(91)
    # 64 and 65 finite rows with rows that are not finite in between (the scan sees 65 poles of a field of 80 from inside it)
    frags = random_field(80, 92)
    pick = rng.permutation(80)[:65].tolist()
    rows = view_of(frags, pick, 0.3, 60.0, 70.0)
    bad = [(np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf)]

    def laced(rs):
        o = []
        for k, r in enumerate(rs):
            o.append(r)
            if k % 7 == 3:
                o.append(bad[(k // 7) % 3])
        return [bad[0]] + o
    out["rows_64_65"] = (frags, [laced(rows[:64]), laced(rows), laced(rows[:63])], dict(max_baseline=200.0),
                         dict(n_kp=[64, 64, 63], flags=[VALID, VALID | TRUNC, VALID], score=[64, 64, 63]))
    # 6 keypoints are 15 candidate pairs: max_seeds 16, 15 and 14
    frags = random_field(30, 93)
    rows = view_of(frags, [3, 8, 11, 17, 20, 29], -1.1, 40.0, 35.0)
    for ms, n in ((16, 15), (15, 15), (14, 14)):
        out[f"seeds_{ms}"] = (frags, [rows], dict(max_baseline=200.0, max_seeds=ms), dict(n_kp=[6], n_seeds=[n], flags=[VALID], score=[6]))
    # landmark counts at the workgroups' edges (the grid's kernels and the hypothesis kernel take 256 a workgroup)
    for n in (255, 256, 257):
        frags = random_field(n, 94 + n)
        rows = view_of(frags, [0, n - 1, n - 2, 100, 101, 200, 254], 2.0, 120.0, 130.0)
        out[f"landmarks_{n}"] = (frags, [rows, rows[::-1]], dict(max_baseline=300.0, max_seeds=8), dict(flags=[VALID, VALID], score=[7, 7]))
    return out
