"""The wavefront and group tiers of the descriptor stage the support set of a row with its neighbours (d2 < R^2) in front and
the shell out to the support radius behind them, and bin only the front (csrc/fx_kernels.hip: desc_wave_body, k_desc_group).
Hand-built scans pin the edges of that split against the oracle, bit for bit: every row's neighbour count and support count is
set exactly, by points the detector never sees.

A scene is up to four poles, one on each horizontal axis at D metres: three rings of four points each, which the detector
turns into one keypoint per pole.  The x / y windows of the filter end 2 mm behind the poles, so everything placed further out
is part of the descriptor's search surface (the unfiltered cloud) and of nothing else.  With R = 5 cm the pole's own points (10 cm
and more from the keypoint) are outside the support radius 1.2 R: a row's support set is exactly the points placed here, `nbr`
of them inside R and `sup - nbr` in the shell between 1.05 R and 1.15 R."""
import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import util

pytestmark = pytest.mark.gpu

R = 0.05
D = 5.0
GROUP_CAP, WAVE_CAP = 64, 192  # FX_GROUP_CAP, FX_WAVE_CAP: rows of up to 64 support points are group rows, up to 192 wave rows
AXES = [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)]

# (neighbours, support points, how they are laid out)
#   "mixed": neighbours scattered among the shell points in scan order; "last": every neighbour behind every shell point (the
#   neighbours sit in the last chunk of the stored list); "origin": one of the neighbours IS the keypoint (d2 = 0: counted, never binned)
GROUP_CASES = [(0, 0, "mixed"), (0, 20, "mixed"), (1, 30, "mixed"), (15, 40, "mixed"), (16, 48, "mixed"), (17, 64, "mixed"),
               (63, 64, "mixed"), (64, 64, "mixed"), (5, 40, "last"), (10, 30, "origin"), (1, 1, "origin")]
WAVE_CASES = [(0, 100, "mixed"), (1, 130, "mixed"), (15, 150, "mixed"), (16, 192, "mixed"), (17, 70, "mixed"), (63, 130, "mixed"),
              (64, 192, "mixed"), (65, 192, "mixed"), (WAVE_CAP, WAVE_CAP, "mixed"), (60, 130, "mixed"), (128, 129, "mixed"),
              (20, 190, "last"), (3, 192, "last"), (40, 100, "origin")]


def _params():
    return capi.params("launch", cloud_leveling=0, x_min=-(D + 0.002), x_max=D + 0.002, y_min=-(D + 0.002), y_max=D + 0.002,
                       z_min=-1.0, z_max=1.0, cluster_tolerance=0.25, cluster_min_count=3, cluster_max_count=50,
                       cluster_radius_threshold=0.4, number_detection_channels=3, descriptor_radius=R)


def _pole(p, axis, z_extra=None):
    """Rings 7, 8, 9 (elevations -1, 1, 3 degrees on a VLP-16), four points each, 20 cm apart across the axis."""
    a = np.array(axis)
    t = np.array([-a[1], a[0]])
    pts = []
    for ring in (7, 8, 9):
        el = np.deg2rad(p.el0_deg + ring * p.el_step_deg)
        for s in (-0.3, -0.1, 0.1, 0.3):
            xy = D * a + s * t
            pts.append([xy[0], xy[1], np.hypot(*xy) * np.tan(el)])
        if ring == 8 and z_extra is not None:  # a fifth point of the middle ring, on the axis: see _origin_z
            pts.append([D * a[0], D * a[1], z_extra])
    return np.array(pts, np.float32)


def _origin_z(oracle, p, axis):
    """The height at which a point on the pole's axis is the pole's keypoint to the bit.  The point is part of the middle ring's
    cluster, so it moves the keypoint it wants to sit on: by a fifteenth of its own move, which settles in a few rounds."""
    z = None
    for _ in range(20):
        s = np.zeros((13 if z is not None else 12, 4), np.float32)
        s[:, :3] = _pole(p, axis, z)
        kp = oracle.run(p, s)["keypoints"]
        assert len(kp) == 1
        if z is not None and np.float32(z) == kp[0, 2]:
            assert kp[0, 0] == np.float32(D * axis[0]) and kp[0, 1] == np.float32(D * axis[1])
            return float(z)
        z = kp[0, 2]
    raise AssertionError("the keypoint did not settle on the point")


def _scene(oracle, p, cases, rng):
    """One scan of len(cases) <= 4 poles and what each row must count: (scan, [(keypoint xyz, nbr, sup)])."""
    poles, first, last, want = [], [], [], []
    for axis, (nbr, sup, how) in zip(AXES, cases):
        a = np.array(axis)
        z_extra = _origin_z(oracle, p, axis) if how == "origin" else None
        pole = _pole(p, axis, z_extra)
        s = np.zeros((len(pole), 4), np.float32)
        s[:, :3] = pole
        kp = oracle.run(p, s)["keypoints"][0, :3].astype(np.float64)
        poles.append(pole)

        def around(n, r_lo, r_hi):  # n points r_lo..r_hi from the keypoint, at least half of that beyond it along the axis
            c, th = rng.uniform(0.5, 1.0, n), rng.uniform(0.0, 2 * np.pi, n)
            s = np.sqrt(1.0 - c * c)
            d = np.stack([c * a[0] - s * np.cos(th) * a[1], c * a[1] + s * np.cos(th) * a[0], s * np.sin(th)], axis=1)  # unit vectors
            return (kp + d * rng.uniform(r_lo, r_hi, (n, 1))).astype(np.float32)

        n_in = nbr - (1 if how == "origin" else 0)
        inner, shell = around(n_in, 0.2 * R, 0.9 * R), around(sup - nbr, 1.05 * R, 1.15 * R)
        if how == "last":
            first.append(shell)
            last.append(inner)
        else:
            both = np.concatenate([inner, shell])
            first.append(both[rng.permutation(len(both))])
        want.append((kp, nbr, sup))
    xyz = np.concatenate(first + poles + last)
    scan = np.zeros((len(xyz), 4), np.float32)
    scan[:, :3] = xyz
    return scan, want


def _check_counts(ora, scan, want, tag):
    """The oracle's own rows have the neighbour and support counts the case names (the tier a row takes follows from the latter)."""
    assert ora["n_keypoints"] == len(want), tag
    cloud = scan[:, :3]
    r_sup = np.float32((R + R / 5) * (1 + 1e-4))
    for kp, nbr, sup in want:
        k = int(np.argmin(np.abs(ora["keypoints"][:, :3] - kp).sum(axis=1)))
        d = cloud - ora["keypoints"][k, :3]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert int(ora["kp_neighbors"][k]) == nbr, f"{tag}: keypoint {k} has {ora['kp_neighbors'][k]} neighbours, wanted {nbr}"
        assert int((d2 < np.float32(R) * np.float32(R)).sum()) == nbr, tag
        assert int((d2 < r_sup * r_sup).sum()) == sup, f"{tag}: keypoint {k} has {(d2 < r_sup * r_sup).sum()} support points, wanted {sup}"
        if nbr == 0:
            assert np.isnan(ora["descriptors"][k, :1980]).all(), tag


def _compare(got, ora, tag):
    st = util.compare_scan(got, ora, tag=tag)
    util.assert_bit_equal(got["descriptors"], ora["descriptors"], f"{tag} descriptors")
    assert st["n_inexact"] == 0


def _scenes(oracle, cases, seed):
    p = _params()
    rng = np.random.default_rng(seed)
    out = []
    for i in range(0, len(cases), 4):
        scan, want = _scene(oracle, p, cases[i:i + 4], rng)
        ora = oracle.run(p, scan)
        _check_counts(ora, scan, want, f"cases {cases[i:i + 4]}")
        out.append((scan, ora))
    return p, out


@pytest.mark.parametrize("tier", ["group", "wave"])
def test_neighbour_counts_at_the_chunk_edges(fxlib, oracle, tier):
    cases = GROUP_CASES if tier == "group" else WAVE_CASES
    assert all(sup <= GROUP_CAP if tier == "group" else GROUP_CAP < sup <= WAVE_CAP for _, sup, _ in cases)
    p, scenes = _scenes(oracle, cases, 7)
    ctx = capi.Context(p, capi.limits(len(scenes), 1024))
    got = ctx.process_host([s for s, _ in scenes])
    for b, (_, ora) in enumerate(scenes):
        _compare(got[b], ora, f"{tier} tier, scan {b}")
    ctx.close()


def test_rows_reused_by_batches_of_other_shapes(fxlib, oracle):
    """A context's rows keep the bins the group tier wrote last time and un-write exactly those: three different batches through the
    same rows, every row changing its neighbour count, its support count and (most of them) its tier from batch to batch."""
    mixed = [c for pair in zip(GROUP_CASES, WAVE_CASES) for c in pair]
    batches = [mixed[0:8], mixed[8:16], list(reversed(mixed[0:8])), mixed[16:22] + mixed[0:2], mixed[0:8]]
    p = _params()
    ctx = capi.Context(p, capi.limits(2, 1024))
    for n, cases in enumerate(batches):
        _, scenes = _scenes(oracle, cases, 100 + n)
        got = ctx.process_host([s for s, _ in scenes])
        for b, (_, ora) in enumerate(scenes):
            _compare(got[b], ora, f"batch {n}, scan {b}")
    ctx.close()
