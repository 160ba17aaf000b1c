"""Hand-built descriptor rows (tests/test_gpu_desc_neighbour_compaction.py, tests/test_gpu_desc_list_dense_rows.py, the CPU
checks of their scenes in tests/test_desc_rows_scenes.py): scans in which every row's neighbour count and support count is set
exactly, by points the detector never sees, and the bit-for-bit comparison of the product's rows with the oracle's.

A scene is up to four poles, one on each horizontal axis at D metres: three rings of four points each, which the detector
turns into one keypoint per pole.  The x / y windows of the filter end 2 mm behind the poles, so everything placed further out
is part of the descriptor's search surface (the unfiltered cloud) and of nothing else.  With R = 5 cm the pole's own points (10 cm
and more from the keypoint) are outside the support radius 1.2 R: a row's support set is exactly the points placed here, `nbr`
of them inside R and `sup - nbr` in the shell between 1.05 R and 1.15 R.

A case is (neighbours, support points, layout):
  "mixed"    neighbours scattered among the shell points in scan order;
  "last"     every neighbour behind every shell point (the neighbours sit in the last chunk of the stored list);
  "origin"   one of the neighbours IS the keypoint (d2 = 0: counted, never binned);
  "one_bin"  every neighbour in a cone of 7 degrees about the axis and the three radial shells 0.64 R .. 0.97 R — half a dozen
             bins with hundreds of terms each —, drawn from clumps between half a millimetre and half a centimetre wide, so that
             the local densities (points within R / 5 = 1 cm) and with them the weights differ by an order of magnitude;
  "dup"      a third of the neighbours are exact copies of other neighbours: equal bin, equal d2, only the point index tells
             the keys apart."""
import functools

import numpy as np

from feature_extraction_amd import capi
from tests import sc3d_independent as ind
from tests import util

R = 0.05
D = 5.0
GROUP_CAP, WAVE_CAP = 64, 192  # FX_GROUP_CAP, FX_WAVE_CAP: rows of up to 64 support points are group rows, up to 192 wave rows
LIST_CAP = 1024                # kDenseMin, and the default max_neighbors: rows of up to 1024 support points are list rows, beyond that dense
AXES = [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)]


def params(radius=R):
    return capi.params("launch", cloud_leveling=0, x_min=-(D + 0.002), x_max=D + 0.002, y_min=-(D + 0.002), y_max=D + 0.002,
                       z_min=-1.0, z_max=1.0, cluster_tolerance=0.25, cluster_min_count=3, cluster_max_count=50,
                       cluster_radius_threshold=0.4, number_detection_channels=3, descriptor_radius=radius)


def pole(p, axis, z_extra=None, side=0.0, spread=(-0.3, -0.1, 0.1, 0.3)):
    """Rings 7, 8, 9 (elevations -1, 1, 3 degrees on a VLP-16), four points each, 20 cm apart across the axis (`side`: the whole
    pole moved that far across the axis)."""
    a = np.array(axis)
    t = np.array([-a[1], a[0]])
    pts = []
    for ring in (7, 8, 9):
        el = np.deg2rad(p.el0_deg + ring * p.el_step_deg)
        for s in spread:
            xy = D * a + (side + s) * t
            pts.append([xy[0], xy[1], np.hypot(*xy) * np.tan(el)])
        if ring == 8 and z_extra is not None:  # a fifth point of the middle ring, on the axis: see origin_z
            pts.append([D * a[0], D * a[1], z_extra])
    return np.array(pts, np.float32)


def origin_z(oracle, p, axis):
    """The height at which a point on the pole's axis is the pole's keypoint to the bit.  The point is part of the middle ring's
    cluster, so it moves the keypoint it wants to sit on: by a fifteenth of its own move, which settles in a few rounds."""
    z = None
    for _ in range(20):
        s = np.zeros((13 if z is not None else 12, 4), np.float32)
        s[:, :3] = pole(p, axis, z)
        kp = oracle.run(p, s)["keypoints"]
        assert len(kp) == 1
        if z is not None and np.float32(z) == kp[0, 2]:
            assert kp[0, 0] == np.float32(D * axis[0]) and kp[0, 1] == np.float32(D * axis[1])
            return float(z)
        z = kp[0, 2]
    raise AssertionError("the keypoint did not settle on the point")


def _clumps(rng, kp, a, n):
    """n points of the "one_bin" layout around keypoint kp on axis a (float64)."""
    up, t = np.array([0.0, 0.0, 1.0]), np.array([-a[1], a[0], 0.0])
    a3 = np.array([a[0], a[1], 0.0])
    half = np.deg2rad(7.0)
    out = []
    n_clumps = 9
    share = rng.dirichlet(np.full(n_clumps, 0.6))  # a few clumps hold most of the points
    width = np.geomspace(0.0005, 0.005, n_clumps)[rng.permutation(n_clumps)]
    centre_r, centre_u, centre_v = rng.uniform(0.68 * R, 0.93 * R, n_clumps), rng.uniform(-0.6, 0.6, n_clumps), rng.uniform(-0.6, 0.6, n_clumps)
    while len(out) < n:
        c = rng.choice(n_clumps, p=share)
        ctr = centre_r[c] * (a3 + np.tan(half) * (centre_u[c] * t + centre_v[c] * up))
        v = ctr + rng.normal(0.0, width[c], 3)
        r = np.linalg.norm(v)
        if 0.64 * R < r < 0.97 * R and np.arccos(np.clip(v @ a3 / r, -1.0, 1.0)) < half:
            out.append(kp + v)
    return np.array(out).astype(np.float32)


def scene(oracle, p, cases, rng):
    """One scan of len(cases) <= 4 poles and what each row must count: (scan, [(keypoint xyz, nbr, sup)])."""
    poles, first, last, want = [], [], [], []
    for axis, (nbr, sup, how) in zip(AXES, cases):
        a = np.array(axis)
        z_extra = origin_z(oracle, p, axis) if how == "origin" else None
        pl = pole(p, axis, z_extra)
        s = np.zeros((len(pl), 4), np.float32)
        s[:, :3] = pl
        kp = oracle.run(p, s)["keypoints"][0, :3].astype(np.float64)
        poles.append(pl)

        def around(n, r_lo, r_hi):  # n points r_lo..r_hi from the keypoint, at least half of that beyond it along the axis
            c, th = rng.uniform(0.5, 1.0, n), rng.uniform(0.0, 2 * np.pi, n)
            s = np.sqrt(1.0 - c * c)
            d = np.stack([c * a[0] - s * np.cos(th) * a[1], c * a[1] + s * np.cos(th) * a[0], s * np.sin(th)], axis=1)  # unit vectors
            return (kp + d * rng.uniform(r_lo, r_hi, (n, 1))).astype(np.float32)

        n_in = nbr - (1 if how == "origin" else 0)
        if how == "one_bin":
            inner = _clumps(rng, kp, a, n_in)
        elif how == "dup":
            n_own = n_in - n_in // 3
            inner = around(n_own, 0.2 * R, 0.9 * R)
            inner = np.concatenate([inner, inner[rng.integers(0, n_own, n_in - n_own)]])  # (some points three and four times)
        else:
            inner = around(n_in, 0.2 * R, 0.9 * R)
        shell = around(sup - nbr, 1.05 * R, 1.15 * R)
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


def sqdist(cloud, q):
    d = cloud - q
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def support_radii(radius=R):
    """(the oracle's support radius, the device's wider one: FxDevParams::r2_support), as float32."""
    return np.float32((radius + radius / 5) * (1 + 1e-4)), np.float32((radius + radius / 5.0) * 1.0001 + 1e-4)


def check_counts(ora, scan, want, tag):
    """The oracle's own rows have the neighbour and support counts the case names (the tier a row takes follows from the latter)."""
    assert ora["n_keypoints"] == len(want), tag
    cloud = scan[:, :3]
    r_sup = support_radii()[0]
    for kp, nbr, sup in want:
        k = int(np.argmin(np.abs(ora["keypoints"][:, :3] - kp).sum(axis=1)))
        d2 = sqdist(cloud, ora["keypoints"][k, :3])
        assert int(ora["kp_neighbors"][k]) == nbr, f"{tag}: keypoint {k} has {ora['kp_neighbors'][k]} neighbours, wanted {nbr}"
        assert int((d2 < np.float32(R) * np.float32(R)).sum()) == nbr, tag
        assert int((d2 < r_sup * r_sup).sum()) == sup, f"{tag}: keypoint {k} has {(d2 < r_sup * r_sup).sum()} support points, wanted {sup}"
        if nbr == 0:
            assert np.isnan(ora["descriptors"][k, :1980]).all(), tag


def support_counts(scan, ora, radius=R):
    """Per row of the oracle: (support points by the oracle's radius, by the device's wider one)."""
    lo, hi = support_radii(radius)
    d2 = [sqdist(scan[:, :3], kp[:3]) for kp in ora["keypoints"]]
    return [int((d < lo * lo).sum()) for d in d2], [int((d < hi * hi).sum()) for d in d2]


def tier_of(n_support, list_cap=LIST_CAP):
    if n_support > min(list_cap, LIST_CAP):
        return "dense"
    return "group" if n_support <= GROUP_CAP else "wave" if n_support <= WAVE_CAP else "list"


def first_mismatch(got, ora, tag, scan=None, radius=R, list_cap=LIST_CAP):
    """Where the product's descriptor rows leave the oracle's: scan tag, row, tier, bin and both bit patterns."""
    g, o = np.asarray(got["descriptors"]), np.asarray(ora["descriptors"])
    if g.shape != o.shape:
        return f"{tag}: descriptor rows {g.shape} against the oracle's {o.shape}"
    bad = (util.bits(g) != util.bits(o)) & ~((g == 0) & (o == 0))
    if not bad.any():
        return f"{tag}: every descriptor word equals the oracle's"
    sup = support_counts(scan, ora, radius)[1] if scan is not None else None
    lines = [f"{tag}: {int(bad.sum())} descriptor words in {int(bad.any(axis=1).sum())} rows differ from the oracle"]
    for row, b in np.argwhere(bad)[:8]:
        where = f"{sup[row]} support points, {tier_of(sup[row], list_cap)} tier" if sup else "tier unknown"
        lines.append(f"  row {row} ({int(ora['kp_neighbors'][row])} neighbours, {where}) bin {b}: device {g[row, b]!r} "
                     f"{util.bits(g)[row, b]:#010x}, oracle {o[row, b]!r} {util.bits(o)[row, b]:#010x}")
    return "\n".join(lines)


def compare(got, ora, tag, scan=None, radius=R, list_cap=LIST_CAP):
    try:
        st = util.compare_scan(got, ora, tag=tag)
        util.assert_bit_equal(got["descriptors"], ora["descriptors"], f"{tag} descriptors")
        assert st["n_inexact"] == 0
    except AssertionError as e:
        raise AssertionError(f"{e}\n{first_mismatch(got, ora, tag, scan, radius, list_cap)}") from None


def scenes(oracle, cases, seed):
    p = params()
    rng = np.random.default_rng(seed)
    out = []
    for i in range(0, len(cases), 4):
        scan, want = scene(oracle, p, cases[i:i + 4], rng)
        ora = oracle.run(p, scan)
        check_counts(ora, scan, want, f"cases {cases[i:i + 4]}")
        out.append((scan, ora))
    return p, out


def order_sensitive(p, scan, ora, k):
    """How many bins of row k change bits when their terms are added in the reverse of the contract's order ((d2, index)
    ascending within a bin): bins and weights recomputed here as tests/sc3d_independent.py states 3DSC (fp64 angles and radii,
    float32 set membership), the weights and the sums in numpy float32.  Also returns the largest number of terms of a bin.
    A row for which this is 0 cannot tell a reordered sum from the right one."""
    radius = float(p.descriptor_radius)
    cloud = np.ascontiguousarray(scan[:, :3], np.float32)
    kps = ora["keypoints"][:, :3]
    o = kps[k]
    d2 = ind.f32_sqdist(cloud, o)
    nb = np.where((d2 < np.float32(radius * radius)) & ~(d2 < np.finfo(np.float32).tiny))[0]
    if len(nb) == 0:
        return 0, 0
    # the reference direction of row k: draws 3 n, 3 n + 1 of mt19937(12345), n = rows before k that have a neighbour
    rng = ind.MT19937(12345)
    for _ in range(3 * int((ora["kp_neighbors"][:k] > 0).sum())):
        rng.u32()
    ax = [np.float32(rng.u32() / 4294967296.0) for _ in range(2)]
    a0 = np.arctan2(np.float64(ax[1]), np.float64(ax[0]))
    radii, vol = ind.bin_volumes(radius)
    lut = (1.0 / np.cbrt(vol)).astype(np.float32)  # [K, J]
    v = cloud[nb].astype(np.float64) - o.astype(np.float64)
    r = np.sqrt(d2[nb].astype(np.float64))
    theta = np.degrees(np.arccos(np.clip(v[:, 2] / np.linalg.norm(v, axis=1), -1.0, 1.0)))
    phi = np.where((v[:, 0] == 0) & (v[:, 1] == 0), 0.0, np.degrees(np.arctan2(v[:, 1], v[:, 0]) - a0) % 360.0)
    j = np.searchsorted(radii[1:], r, side="left")
    kk = np.searchsorted(np.arange(1, ind.K_BINS + 1) * (180.0 / ind.K_BINS), theta, side="left")
    ll = np.searchsorted(np.arange(1, ind.L_BINS + 1) * (360.0 / ind.L_BINS), phi, side="left")
    j, kk, ll = np.where(j >= ind.J_BINS, 0, j), np.where(kk >= ind.K_BINS, 0, kk), np.where(ll >= ind.L_BINS, 0, ll)
    sup = cloud[d2 < np.float32((radius * 1.2 + 1e-3) ** 2)]
    r2_density = np.float32((radius / 5.0) ** 2)
    rho = np.zeros(len(nb), np.int64)
    for c0 in range(0, len(nb), 256):  # (chunks of a [256, support] table)
        q = cloud[nb[c0:c0 + 256]]
        dd = sup[None, :, :] - q[:, None, :]
        rho[c0:c0 + 256] = ((dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2] < r2_density).sum(axis=1)
    w = (np.float32(1.0) / rho.astype(np.float32)) * lut[kk, j]
    b = (ll * ind.K_BINS + kk) * ind.J_BINS + j
    order = np.lexsort((nb, d2[nb], b))  # (bin, d2, index) ascending
    b, w = b[order], w[order].astype(np.float32)
    starts = np.flatnonzero(np.r_[True, b[1:] != b[:-1]])
    ends = np.r_[starts[1:], len(b)]
    changed = 0
    for s0, s1 in zip(starts, ends):
        if s1 - s0 >= 3:  # (two terms: fp32 addition commutes)
            fwd, rev = np.add.accumulate(w[s0:s1])[-1], np.add.accumulate(w[s0:s1][::-1])[-1]
            changed += int(fwd.view(np.uint32) != rev.view(np.uint32))
    return changed, int((ends - starts).max())


# ---- the scenes of tests/test_gpu_desc_list_dense_rows.py (checked on the CPU by tests/test_desc_rows_scenes.py)
# Four cases a scan.  A case with few neighbours shares its scan with one of hundreds: every scan with a row of 64 neighbours or
# more then has a row whose sums depend on their order (order_sensitive), so a reordered sum cannot hide in any of them.
LIST_CASES = [(0, 193, "mixed"), (1, 200, "origin"), (1, 193, "mixed"), (32, 300, "mixed"),
              (33, 300, "mixed"), (64, 400, "mixed"), (65, 400, "mixed"), (512, 1024, "mixed"),
              (128, 500, "mixed"), (129, 500, "mixed"), (193, 193, "mixed"), (1023, 1024, "mixed"),
              (255, 256, "mixed"), (256, 257, "mixed"), (257, 600, "mixed"), (300, 700, "last"),
              (400, 800, "one_bin"), (200, 500, "dup"), (1024, 1024, "mixed")]
DENSE_CASES = [(0, 1025, "mixed"), (1, 1025, "origin"), (1024, 1025, "mixed"), (1025, 1025, "mixed"),
               (1023, 2047, "mixed"), (1024, 2048, "mixed"), (1025, 2049, "mixed"), (2048, 2049, "mixed"),
               (2049, 4096, "mixed"), (3000, 4097, "mixed"), (5000, 8193, "mixed"), (1500, 3000, "one_bin"),
               (1200, 2500, "dup")]
# k_dense_finish with FX_DENSE_LDS_KEYS=300: binned neighbours at the limit, and at the power-of-two paddings of the sort in the key pool
KEYS_CASES = [(299, 1100, "mixed"), (300, 1100, "mixed"), (301, 1100, "mixed"), (512, 1100, "mixed"),
              (513, 1100, "mixed"), (1025, 1100, "mixed")]
# ... and at the real limit (FX_DFIN_K = 14336 keys in LDS), a scan each
BIG_CASES = [[(14336, 14400, "mixed")], [(14337, 14400, "mixed")]]
# every tier and a NaN row in each of four scans
ALL_TIER_CASES = [(20, 40, "mixed"), (100, 150, "mixed"), (300, 600, "mixed"), (1100, 1500, "mixed"),
                  (0, 30, "mixed"), (0, 1030, "mixed"), (150, 192, "last"), (700, 1024, "dup"),
                  (64, 64, "mixed"), (1300, 2100, "one_bin"), (10, 100, "origin"), (1025, 1025, "mixed"),
                  (400, 600, "mixed"), (0, 250, "mixed"), (63, 65, "mixed"), (5, 5, "mixed")]


def overflow_cases(L):
    """Rows of L - 1, L, L + 1 and 4 L support points for max_neighbors = L: the first two stay in their own tier, the others are
    dense rows whose entries beyond L sit in the scan's overflow region."""
    return [(L // 2, L - 1, "mixed"), (L // 2 + 1, L, "mixed"), (L // 2 + 1, L + 1, "mixed"), (min(3 * L, 60 + 3 * (L - 32)), 4 * L, "mixed")]


# dense rows that fit a 4096-entry pool, one of them NaN; and dense rows that EACH exceed it (tests/test_gpu_desc_csr.py)
CSR_FIT_CASES = [(700, 1300, "mixed"), (0, 1100, "mixed"), (40, 60, "mixed"), (900, 1500, "dup")]
CSR_EXHAUST_CASES = [(2000, 4200, "mixed"), (0, 4100, "mixed"), (30, 50, "mixed"), (100, 300, "mixed")]


# name: (cases, seed of the builder)
NAMED = {"list": (LIST_CASES, 38), "dense": (DENSE_CASES, 12), "keys": (KEYS_CASES, 13), "big0": (BIG_CASES[0], 14),
         "big1": (BIG_CASES[1], 15), "all": (ALL_TIER_CASES, 16), "overflow32": (overflow_cases(32), 17),
         "overflow256": (overflow_cases(256), 18), "csr_fit": (CSR_FIT_CASES, 19), "csr_exhaust": (CSR_EXHAUST_CASES, 20)}


@functools.lru_cache(maxsize=None)
def built(name):
    """(params, [(scan, oracle result)], cases) of a named case list, built once a process; nobody writes into it."""
    from oracle import oracle_py
    oracle_py.load()
    cases, seed = NAMED[name]
    return scenes(oracle_py, cases, seed) + (cases,)

# ---- shared densities: three keypoints 42 cm apart at R = 0.5 m, their support sets overlapping
R_SHARED = 0.5


def shared_scene(oracle, seed, n_own=1500, n_common=600):
    """(params, scan, oracle result): three narrow poles side by side at x = D (42 cm from pole to pole), and behind the window's
    edge a cloud for each — n_own points within 0.45 m of its keypoint — and n_common points within 6 cm of the middle
    one's, which all three spheres of 0.5 m hold."""
    p = params(R_SHARED)
    rng = np.random.default_rng(seed)
    sides = (-0.42, 0.0, 0.42)
    poles = [pole(p, AXES[0], side=s, spread=(-0.06, -0.02, 0.02, 0.06)) for s in sides]
    kps = []
    for pl in poles:
        s = np.zeros((len(pl), 4), np.float32)
        s[:, :3] = pl
        kp = oracle.run(p, s)["keypoints"]
        assert len(kp) == 1
        kps.append(kp[0, :3].astype(np.float64))

    def beyond(kp, n, r_hi):  # n points in the half ball of r_hi behind the window's edge (x > D + 2 mm)
        out = np.zeros((0, 3))
        while len(out) < n:
            v = rng.uniform(-r_hi, r_hi, (4 * n, 3))
            v = v[(np.linalg.norm(v, axis=1) < r_hi) & (kp[0] + v[:, 0] > D + 0.01)]
            out = np.concatenate([out, kp + v])
        return out[:n]

    extra = n_own // 50  # (spares for the points dropped next)
    cloud = np.concatenate([beyond(kp, n_own + extra, 0.45) for kp in kps] + [beyond(kps[1], n_common, 0.06)])
    cloud = cloud[rng.permutation(len(cloud))].astype(np.float32)
    # no point between the oracle's support radius and the device's wider one (nor within a millimetre of them): both count the same sets
    lo, hi = support_radii(R_SHARED)
    for kp in kps:
        d = np.sqrt(sqdist(cloud, kp.astype(np.float32)))
        cloud = cloud[(d < lo - 1e-3) | (d > hi + 1e-3)]
    assert len(cloud) >= 3 * n_own + n_common
    xyz = np.concatenate([cloud[:3 * n_own + n_common]] + poles)
    scan = np.zeros((len(xyz), 4), np.float32)
    scan[:, :3] = xyz
    return p, scan, oracle.run(p, scan)


@functools.lru_cache(maxsize=None)
def built_shared(which):
    """0: the scene of the shared-densities test; 1: another with the same number of points at other coordinates."""
    from oracle import oracle_py
    oracle_py.load()
    return shared_scene(oracle_py, 21 + which)
