"""The descriptor's decisions pinned at the floats where they flip (tests/test_gpu_desc_edges.py; the CPU checks of the scenes:
tests/test_desc_edges_scenes.py).

Two halves.

A numpy restatement of one 3DSC row in the contract's operation order, float32 throughout, independent of oracle/ (`quantities`,
`bins`, `statement`):
  distance   d2 = ((dx dx) + dy dy) + dz dz;  r = sqrt(d2)
  azimuth    pcl::geometry::project with the normal +z, Eigen's guarded normalize (z > 0), cross and dot as c0 + (c1 + c2),
             (float)atan2((double)|cross|, (double)dot) * 57.29578f, mirrored to 360 - phi when cross . n < 0
  elevation  (float)acos((double)clamp(n . normalized(neighbour - origin))) * 57.29578f
  bins       the first edge >= the value, else bin 0
  density    brute force over the whole surface, d2 < r2_density
  weight     (1.0f / (float)rho) * lut; per bin one sequential float32 sum in (d2, index) order
The x-axis comes from tests/sc3d_independent.MT19937, the edge tables and the lut from oracle_py.sc3d_tables (pinned by
tests/test_oracle_known_answers.py): what is restated here are the decisions, not powf.

Scenes of probes on tests/desc_rows_util.py's poles.  A probe is a point the detector never sees, placed by a seeded search so
that one float32 of the statement (r, theta, phi, d2, a mutual d2) is the float below, on or above the value at which a decision
flips.  Every probe carries a stated expectation: the (j, k, l) bin it must land in, "out" (not a neighbour) or "skip", and its
local density rho — derived when the scene is built, from the construction (the edge's side, a mid-bin direction in float64, a float64 count of the points
within R / 5), never from the statement under test.

Scene kinds (where the probes can live):
  "x"     desc_rows_util's three-ring poles; the probes lie beyond the filter's face 2 mm behind the pole
  "ztop"  ring 9's four points as the keypoint (one detection channel) under a z_max a millimetre above them: the probes lie
          above the face, at every azimuth and straight above the keypoint
  "zbot"  ring 7's four points over a z_min a millimetre below them: straight below the keypoint
  "f"     an "x" pole with a fifth point that IS the keypoint (desc_rows_util.origin_z) and the x face 0.05 mm behind it: probes a
          tenth of a millimetre from the keypoint
  "z0"    ring 8 at elevation 0 (el0_deg moved): the keypoint's z is 0 exactly and the z window ends at it, so a probe 2^-63 above
          it has d2 = FLT_MIN exactly
  "xr"    the "x" poles at R = 0.5 m (desc_rows_util.R_SHARED): the radial and density families once more, the pole's own points
          inside every support set
Packs hold at most 12 probes, so that a pack plus filler fits the narrowest size class of the group tier; `scenes(kind, support)`
pads every row with shell filler (1.05 R .. 1.15 R, more than R / 5 from every probe) to exactly `support` support points."""
import functools

import numpy as np

from tests import desc_rows_util as du
from tests import sc3d_independent as ind

F32 = np.float32
F64 = np.float64
R, D = du.R, du.D
FLT_MIN, FLT_EPSILON = np.finfo(F32).tiny, np.finfo(F32).eps
DEG = F32(57.29578)
J, K, L = ind.J_BINS, ind.K_BINS, ind.L_BINS
N_TRIES = 200000  # candidates of one search (the number of tries a failed azimuth search is recorded with)


def below(v):
    return np.nextafter(F32(v), F32(-np.inf))


def above(v):
    return np.nextafter(F32(v), F32(np.inf))


def gates(radius=R):
    """(r2_search, r2_density): doubles, narrowed once."""
    radius = float(radius)
    rd = radius / 5.0
    return F32(radius * radius), F32(rd * rd)


@functools.lru_cache(maxsize=None)
def tables(radius=R):
    from oracle import oracle_py
    return oracle_py.sc3d_tables(float(radius))  # radii[16], theta[12], phi[13], lut[1980]


@functools.lru_cache(maxsize=None)
def xaxis(ordinal):
    """The 3DSC x-axis of the ordinal-th keypoint that has a neighbour: draws 3 n and 3 n + 1 of mt19937(12345) as floats, the
    third component -(0 a0 + 0 a1) / 1 = -0, Eigen's normalize.  float32 [2]."""
    rng = ind.MT19937(12345)
    for _ in range(3 * ordinal):
        rng.u32()
    a0, a1 = (F32(rng.u32() / 4294967296.0) for _ in range(2))
    az = F32(-0.0)
    z = a0 * a0 + (a1 * a1 + az * az)
    s = np.sqrt(z)
    return np.array([a0 / s, a1 / s], F32)


def _normalize(v0, v1, v2):
    zz = v0 * v0 + (v1 * v1 + v2 * v2)
    pos = zz > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(zz)
        return np.where(pos, v0 / s, v0), np.where(pos, v1 / s, v1), np.where(pos, v2 / s, v2)


def quantities(kp, xa, pts):
    """Every float32 a 3DSC row computes of the points pts [n, 3] about keypoint kp with x-axis xa, before the bins."""
    kp = np.asarray(kp, F32)
    pts = np.asarray(pts, F32).reshape(-1, 3)
    bx, by, bz = pts[:, 0], pts[:, 1], pts[:, 2]
    nx, ny, nz = F32(0), F32(0), F32(1)
    ax, ay, az = F32(xa[0]), F32(xa[1]), F32(-0.0)
    pox, poy, poz = bx - kp[0], by - kp[1], bz - kp[2]
    d2 = (pox * pox + poy * poy) + poz * poz
    r = np.sqrt(d2)
    lam = nx * pox + (ny * poy + nz * poz)
    q0, q1, q2 = (bx - lam * nx) - kp[0], (by - lam * ny) - kp[1], (bz - lam * nz) - kp[2]
    residue = q2
    p0, p1, p2 = _normalize(q0, q1, q2)
    c0 = ay * p2 - az * p1
    c1 = az * p0 - ax * p2
    c2 = ax * p1 - ay * p0
    cn = np.sqrt(c0 * c0 + (c1 * c1 + c2 * c2))
    xd = ax * p0 + (ay * p1 + az * p2)
    pe = np.arctan2(cn.astype(F64), xd.astype(F64)).astype(F32) * DEG
    cdn = c0 * nx + (c1 * ny + c2 * nz)
    phi = np.where(cdn < 0, F32(360.0) - pe, pe)
    n0, n1, n2 = _normalize(pox, poy, poz)
    th = nx * n0 + (ny * n1 + nz * n2)
    tc = np.minimum(F32(1.0), np.maximum(F32(-1.0), th))
    theta = theta_of_tc(tc)
    out = dict(d2=d2, r=r, phi=phi, theta=theta, tc=tc, cn=cn, xd=xd, cdn=cdn, residue=residue, pe=pe)
    assert all(v.dtype == F32 for v in out.values())
    return out


def theta_of_tc(tc):
    return np.arccos(np.asarray(tc, F32).astype(F64)).astype(F32) * DEG


def first_edge(edges, v, n):
    """PCL's scan: the first of edges[1 .. n] that is >= v names bin (its index - 1); none (or NaN): bin 0."""
    b = np.searchsorted(edges[1:n + 1], v, side="left")
    return np.where((b >= n) | ~(v == v), 0, b)


def bins(radius, q):
    radii, theta, phi, _ = tables(radius)
    return first_edge(radii, q["r"], J), first_edge(theta, q["theta"], K), first_edge(phi, q["phi"], L)


def sqdist(cloud, p):
    d = cloud - np.asarray(p, F32)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def statement(cloud, kp, xa, radius=R, skip_epsilon=False):
    """One row.  cloud [N, 3] float32: the whole surface.  Returns desc [1980] float32 (NaN without a neighbour), n_nbr (what
    kp_neighbors holds), and per point of the cloud: j, k, l, rho (-1 where the point is no binned neighbour) and `state`:
    0 not a neighbour, 1 skipped, 2 binned."""
    cloud = np.ascontiguousarray(cloud, F32)
    r2_search, r2_density = gates(radius)
    lut = tables(radius)[3]
    q = quantities(kp, xa, cloud)
    d2 = q["d2"]
    nb = d2 < r2_search
    use = nb & ~(np.abs(d2 - F32(0)) < (FLT_EPSILON if skip_epsilon else FLT_MIN))
    n = len(cloud)
    state = np.where(use, 2, np.where(nb, 1, 0))
    jj, kk, ll = (np.where(use, b, -1) for b in bins(radius, q))
    rho = np.full(n, -1, np.int64)
    desc = np.zeros(J * K * L, F32)
    if not nb.any():
        desc[:] = np.nan
        return dict(desc=desc, n_nbr=0, j=jj, k=kk, l=ll, rho=rho, state=state, q=q)
    idx = np.flatnonzero(use)
    for i in idx:
        rho[i] = int((sqdist(cloud, cloud[i]) < r2_density).sum())
    for i in idx[np.lexsort((idx, d2[idx]))]:  # (d2, index) ascending: the sorted radius search
        b = (ll[i] * K + kk[i]) * J + jj[i]
        w = (F32(1.0) / F32(rho[i])) * lut[b]
        desc[b] = desc[b] + w
    assert desc.dtype == F32
    return dict(desc=desc, n_nbr=int(nb.sum()), j=jj, k=kk, l=ll, rho=rho, state=state, q=q)


# ---------------------------------------------------------------- where probes can live
class Pole:
    """One pole of a scene: its points, its keypoint (float32 [3], the oracle's, from the pole alone), the row's x-axis, and the
    half space beyond the filter's face: a point v from the keypoint is unseen by the detector iff v . out > margin."""

    def __init__(self, kind, axis, pts, kp, ordinal, out, margin, radius):
        self.kind, self.axis, self.pts, self.kp, self.ordinal = kind, axis, pts, np.asarray(kp, F32), ordinal
        self.xa = xaxis(ordinal)
        self.out, self.margin, self.radius = np.asarray(out, F64), float(margin), float(radius)
        self.kp64 = self.kp.astype(F64)
        self.slack = 2e-5 if kind == "f" else 3e-4
        self.coarse = int(np.argmax(np.abs(self.kp)))  # the coordinate of 5 m: its floats are 0.5 um apart, the others' nanometres
        self.a0 = np.degrees(np.arctan2(F64(self.xa[1]), F64(self.xa[0])))
        self.rng = np.random.default_rng(1000 + 17 * ordinal + 101 * len(kind) + int(7 * axis[0] + 3 * axis[1]))

    def direction(self, theta_deg, phi_deg):
        """Unit vector (float64) at elevation theta from +z and azimuth phi from the row's x-axis."""
        t, a = np.radians(theta_deg), np.radians(phi_deg + self.a0)
        return np.array([np.sin(t) * np.cos(a), np.sin(t) * np.sin(a), np.cos(t)])

    def mid(self, k, l):
        return self.direction((k + 0.5) * 180.0 / K, (l + 0.5) * 360.0 / L)

    def free(self, v):
        return float(np.dot(v, self.out)) > self.margin + self.slack

    def free_bins(self, r, n, ks=range(K)):
        """n mid-bin directions (k, l) at which a point r from the keypoint is unseen, the most outward first."""
        cand = sorted(((float(np.dot(self.mid(k, l), self.out)), k, l) for k in ks for l in range(L)), reverse=True)
        # (a search steers a float32 through the two fine coordinates: both need a share of the direction)
        fine = [a for a in range(3) if a != self.coarse]
        got = [(k, l) for c, k, l in cand if self.free(r * self.mid(k, l)) and min(abs(self.mid(k, l)[a]) for a in fine) > 0.15]
        assert len(got) >= n, f"only {len(got)} free mid-bin directions at r = {r} ({self.kind})"
        return got[:n]

    def near(self, base, spread, n=N_TRIES):
        """n float32 candidates within `spread` of the float64 point `base`, all unseen by the detector."""
        c = (np.asarray(base, F64) + self.rng.uniform(-spread, spread, (n, 3))).astype(F32)
        return c[(c.astype(F64) - self.kp64) @ self.out > self.margin]

    def sweep(self, base, axis, n):
        """2 n + 1 candidates: the float32 point `base` with coordinate `axis` stepped float by float."""
        b = np.asarray(base, F64).astype(F32)
        c = np.tile(b, (2 * n + 1, 1))
        v = b[axis]
        assert v != 0
        c[:, axis] = (np.array([v], F32).view(np.int32)[0] + np.arange(-n, n + 1, dtype=np.int32)).view(F32)
        return c

    def q(self, pts):
        return quantities(self.kp, self.xa, pts)


R_WIDE = du.R_SHARED
# kind: (where the probes live, descriptor radius)
KINDS = {"x": ("x", R), "ztop": ("ztop", R), "zbot": ("zbot", R), "f": ("f", R), "z0": ("z0", R), "xr": ("x", R_WIDE), "xw": ("x", R)}


def kind_params(kind, radius=R):
    p = du.params(radius)
    if kind == "z0":  # ring 8 at elevation 0: its points, and so the keypoint, have z = 0 exactly; the z window ends AT them
        p.el0_deg = -8 * p.el_step_deg
        p.number_detection_channels = 1
        p.z_max = 0.0
    if kind == "ztop":
        p.number_detection_channels = 1
        p.z_max = float(du.pole(p, du.AXES[0])[8:12, 2].max()) + 0.001
    elif kind == "zbot":
        p.number_detection_channels = 1
        p.z_min = float(du.pole(p, du.AXES[0])[0:4, 2].min()) - 0.001
    elif kind == "f":
        p.x_max = D + 5e-5
    return p


def mid_shell(radius, j):
    radii = tables(radius)[0].astype(F64)
    return float(np.sqrt(radii[j] * radii[j + 1]))


def j_of(radius, r):
    """The shell of a radius that is on no edge (float64)."""
    radii = tables(radius)[0].astype(F64)
    assert np.abs(radii - r).min() > 1e-5 * radius
    return max(int(np.searchsorted(radii[1:J + 1], r)), 0) if r <= radii[J] else None


def k_of(theta):
    e = np.arange(1, K + 1) * (180.0 / K)
    assert np.abs(e[:-1] - theta).min() > 0.05
    return min(int(np.searchsorted(e, theta)), K - 1)


def l_of(phi):
    phi = phi % 360.0
    assert min(phi % 30.0, 30.0 - phi % 30.0) > 0.05, phi
    return int(phi // 30.0)


def probe(name, family, xyz, expect, claim=None, pair=None, expect_eps=None):
    """expect: ("bin", j, k, l) | ("out",) | ("skip",).  claim: {quantity: the float32 the probe was built to reach}.
    pair: (name of the gate partner, "below" | "on" | "above"): the mutual d2 against r2_density.
    expect_eps: the expectation under the FLT_EPSILON reading of the skip rule, where it differs."""
    return dict(name=name, family=family, xyz=np.asarray(xyz, F32).copy(), expect=tuple(expect), claim=dict(claim or {}), pair=pair,
                expect_eps=tuple(expect_eps) if expect_eps else tuple(expect))


def _pick(cands, values, target, what):
    hit = np.flatnonzero(values == target)
    assert len(hit), f"no candidate of {len(cands)} reaches {what} = {target!r}"
    return cands[hit[0]]


# ---------------------------------------------------------------- family A: radial shells
def radial_facts(radius):
    """What the radial table and the neighbour gate say about each other, on floats alone: (which of the floats below / on / above
    radii[15] as r have a d2 < r2_search that maps to them, and whether any d2 < r2_search has sqrt(d2) > radii[15])."""
    radii = tables(radius)[0]
    r2 = gates(radius)[0]
    d2 = F32(r2)
    worst = F32(0)
    for _ in range(64):  # the 64 floats below the gate: sqrt is monotonic, the largest r is the first one's
        d2 = below(d2)
        worst = max(worst, np.sqrt(d2))
    return dict(edge15=radii[15], r_max=np.sqrt(below(r2)), fallback_reachable=bool(worst > radii[15]),
                on_gate_r=np.sqrt(F32(r2)))


def pack_radial(pole, edges, shell0=False):
    """For each edge e of radii[1 .. 15]: three probes with sqrtf(d2) the float below, equal to and above radii[e], in a direction
    of their own.  Edge 15 is stated against the neighbour gate."""
    radius = pole.radius
    radii = tables(radius)[0]
    r2 = gates(radius)[0]
    out = []
    dirs = pole.free_bins(float(radii[min(edges)]), len(edges) + 1, ks=range(2, 9))
    for (k, l), e in zip(dirs, edges):
        u = pole.mid(k, l)
        cands = pole.near(pole.kp64 + u * float(radii[e]), 3e-6)
        q = pole.q(cands)
        for side, target in (("below", below(radii[e])), ("on", radii[e]), ("above", above(radii[e]))):
            ok = np.flatnonzero(q["r"] == target)
            assert len(ok), f"radial edge {e}: no candidate with r {side} the edge"
            i = ok[0]
            if e < 15:
                exp = ("bin", e - 1 if side != "above" else e, k, l)
            else:  # a neighbour only if d2 < r2_search; at most radii[15] then (radial_facts): shell 14
                exp = ("bin", 14, k, l) if q["d2"][i] < r2 else ("out",)
            out.append(probe(f"A{e}{side}", "A", cands[i], exp, {"r": target}))
    if shell0:
        k, l = dirs[len(edges)]
        r0 = 0.9 * float(radii[0])
        if pole.free(r0 * pole.mid(k, l)):
            out.append(probe("A0inner", "A", pole.kp64 + r0 * pole.mid(k, l), ("bin", 0, k, l), {}))
    return out


# ---------------------------------------------------------------- family B: elevation
def theta_reachable(edge, width=64):
    """The elevations the floats tc within `width` of cos(edge) give, either side of theta's edge: (the largest below the edge,
    the edge itself if some tc gives it else None, the smallest above it), and the same three for the float radians alone
    (rad * 57.29578f either side of the edge: whether ANY radian gives the edge)."""
    edge = F32(edge)
    c = F32(np.cos(np.radians(F64(edge))))
    tcs = [c]
    for _ in range(width):
        tcs.append(below(tcs[-1]))
    lo = c
    for _ in range(width):
        lo = above(lo)
        tcs.append(lo)
    th = theta_of_tc(np.array(tcs, F32))
    rad0 = F32(np.radians(F64(edge)))
    rads = [rad0]
    for _ in range(16):
        rads.append(below(rads[-1]))
    hi = rad0
    for _ in range(16):
        hi = above(hi)
        rads.append(hi)
    deg = np.array(rads, F32) * DEG

    def three(v):
        return (v[v < edge].max(), edge if (v == edge).any() else None, v[v > edge].min())
    return three(th), three(deg)


def pack_theta(pole, edges):
    """For each edge e of theta[1 .. 10]: the nearest reachable elevation below the edge, the edge itself where a tc gives it,
    and the nearest above it."""
    theta = tables(pole.radius)[1]
    out = []
    for n, e in enumerate(edges):
        jj = 13 - n % 4
        r = mid_shell(pole.radius, jj)
        ls = [l for l in range(L) if pole.free(r * pole.direction(float(theta[e]), (l + 0.5) * 30.0))]
        assert ls, f"no free azimuth for elevation edge {e}"
        l = max(ls, key=lambda l: float(np.dot(pole.direction(float(theta[e]), (l + 0.5) * 30.0), pole.out)))
        cands = pole.near(pole.kp64 + r * pole.direction(float(theta[e]), (l + 0.5) * 30.0), 1e-6)
        q = pole.q(cands)
        (lo, on, hi), _ = theta_reachable(theta[e])
        for side, target in (("below", lo), ("on", on), ("above", hi)):
            if target is None:
                continue
            p = _pick(cands, q["theta"], target, f"theta at edge {e} ({side})")
            out.append(probe(f"B{e}{side}", "B", p, ("bin", jj, e - 1 if side != "above" else e, l), {"theta": target}))
    return out


# ---------------------------------------------------------------- family C: azimuth
def pack_phi(pole, edges):
    """For each multiple m of 30 degrees (m = 12: the 0 / 360 seam), relative to the row's x-axis: the candidate with the largest
    phi not above the edge, one ON the edge when the search finds one, and the one with the smallest phi above it.  At the seam:
    the largest phi <= 360 (360.0 itself when 360 - pe rounds to it: bin 11), and the smallest phi on the other side (0 itself when
    the cross product vanishes: bin 0).  Returns (probes, {edge: whether equality was found, tries})."""
    out, found = [], {}
    for n, m in enumerate(edges):
        jj = 14 - n % 4
        r = mid_shell(pole.radius, jj)
        edge = F32(30.0 * m)
        cands = pole.near(pole.kp64 + r * pole.direction(45.0, 30.0 * m), 1e-6)
        q = pole.q(cands)
        phi = q["phi"]
        k = k_of(45.0)
        if m < 12:
            lo = phi[phi <= edge].max()
            hi = phi[phi > edge].min()
            sides = [("below", phi[phi < edge].max(), m - 1), ("above", hi, m)]
            if lo == edge:
                sides.insert(1, ("on", edge, m - 1))
            found[m] = (bool(lo == edge), len(cands))
        else:
            far = phi > 180.0
            sides = [("below", phi[far].max(), 11), ("above", phi[~far].min(), 0)]
            if sides[0][1] == F32(360.0):
                sides[0] = ("on", F32(360.0), 11)
                sides.insert(0, ("below", phi[far & (phi < F32(360.0))].max(), 11))
            found[m] = (bool((phi == F32(360.0)).any()), len(cands))
            found[0] = (bool((phi == F32(0.0)).any()), len(cands))
        for side, target, l in sides:
            out.append(probe(f"C{m}{side}", "C", _pick(cands, phi, target, f"phi at {30 * m}"), ("bin", jj, k, l), {"phi": target}))
    return out, found


# ---------------------------------------------------------------- family D: the pole
def pack_pole(pole):
    """Straight above ("ztop") or below ("zbot") the keypoint: x and y the keypoint's to the bit; one float off in x, in y and in
    both (the normalised projection is an axis vector, or the diagonal).  residue_search looks for a height at which the literal
    projection (bz - lambda) - kp.z leaves a residue."""
    up = 1.0 if pole.kind == "ztop" else -1.0
    kp = pole.kp
    radius = pole.radius
    k_end = 0 if up > 0 else K - 1  # theta = 0: bin 0; theta = 180 = theta[11]: bin 10, not the fall-back
    out = []
    # atan2(0, 0) = 0, cross . n = 0: phi = 0, bin 0
    for n, jj in enumerate((9, 13)):
        z = F32(kp[2] + F32(up * mid_shell(radius, jj)))
        out.append(probe(f"D_axis{n}", "D", [kp[0], kp[1], z], ("bin", jj, k_end, 0), {"tc": F32(up), "phi": F32(0)}))
    # one float off: the projection is (+-ulp, 0, 0), (0, +-ulp, 0) or both, normalised to an axis vector or the diagonal
    jj = 11
    z = F32(kp[2] + F32(up * mid_shell(radius, jj)))
    for name, sx, sy in (("x+", 1, 0), ("x-", -1, 0), ("y+", 0, 1), ("y-", 0, -1), ("xy", 1, 1)):
        # (a coordinate that is exactly 0 steps by 2^-30: the float next to 0 is subnormal and its square underflows)
        x = (np.nextafter(kp[0], F32(sx * np.inf)) if kp[0] != 0 else F32(sx * 2.0 ** -30)) if sx else kp[0]
        y = (np.nextafter(kp[1], F32(sy * np.inf)) if kp[1] != 0 else F32(sy * 2.0 ** -30)) if sy else kp[1]
        az = np.degrees(np.arctan2(F64(y) - F64(kp[1]), F64(x) - F64(kp[0])))
        out.append(probe(f"D_{name}", "D", [x, y, z], ("bin", jj, k_end, l_of(az - pole.a0)), {}))
    # tc the float next to +-1, and the farthest offset found that still gives +-1 (at some heights float32 steps over the
    # neighbour of 1: the shells are tried in turn)
    h = 0 if pole.coarse == 1 else 1  # the fine horizontal coordinate
    one = F32(up)
    nxt = np.nextafter(one, F32(0))
    l = l_of((90.0 if h == 1 else 0.0) - pole.a0)
    for jj in (12, 10, 13, 9, 8, 14):
        n = 20000
        c = np.zeros((n, 3), F32)
        c[:, 1 - h], c[:, 2] = kp[1 - h], F32(kp[2] + F32(up * mid_shell(radius, jj)))
        c[:, h] = (F64(kp[h]) + np.linspace(1e-7, 1e-4, n)).astype(F32)
        q = pole.q(c)
        hit, same = np.flatnonzero(q["tc"] == nxt), np.flatnonzero(q["tc"] == one)
        if len(hit) and len(same):
            out.append(probe("D_tc_next", "D", c[hit[0]], ("bin", jj, k_end, l), {"tc": nxt}))
            out.append(probe("D_tc_one_off_axis", "D", c[same[-1]], ("bin", jj, k_end, l), {"tc": one}))
            break
    else:
        raise AssertionError("no height at which an offset reaches the float next to +-1")
    return out


def pack_skip_min(pole):
    """The keypoint's z is 0 exactly ("z0"): dz = 2^-63 gives d2 = FLT_MIN exactly (not below it: binned — shell 0, theta = 0,
    phi = 0) and the float below 2^-63 a subnormal d2 (skipped, whether the subtraction and the square keep subnormals or flush
    them); both skipped under the FLT_EPSILON reading.  And one ordinary probe straight above."""
    assert pole.kp[2] == 0 and pole.kind == "z0"
    dz = F32(2.0 ** -63)
    assert dz * dz == FLT_MIN and below(dz) * below(dz) < FLT_MIN
    kp = pole.kp
    return [probe("F_min", "F", [kp[0], kp[1], dz], ("bin", 0, 0, 0), {"d2": FLT_MIN}, expect_eps=("skip",)),
            probe("F_subnormal", "F", [kp[0], kp[1], below(dz)], ("skip",), {"d2": below(dz) * below(dz)}),
            probe("F_above", "F", [kp[0], kp[1], F32(mid_shell(pole.radius, 10))], ("bin", 10, 0, 0), {"tc": F32(1)})]


def residue_search(pole, n=N_TRIES):
    """How many of n heights straight above / below the keypoint leave a non-zero residue (bz - lambda) - kp.z."""
    up = 1.0 if pole.kind == "ztop" else -1.0
    c = np.zeros((n, 3), F32)
    c[:, 0], c[:, 1] = pole.kp[0], pole.kp[1]
    c[:, 2] = (F64(pole.kp[2]) + up * np.linspace(pole.margin + 1e-4, 0.99 * pole.radius, n)).astype(F32)
    return int((pole.q(c)["residue"] != 0).sum()), n


# ---------------------------------------------------------------- family E: the neighbour gate
def pack_gate(pole):
    """d2 the float below, equal to and above r2_search, in two directions."""
    r2 = gates(pole.radius)[0]
    out = []
    for n, (k, l) in enumerate(pole.free_bins(pole.radius, 2, ks=range(3, 8))):
        cands = pole.near(pole.kp64 + pole.radius * pole.mid(k, l), 3e-6)
        d2 = pole.q(cands)["d2"]
        # (the probe below the gate last: the last point of the scan, and so the last entry of the stored list)
        for side, target in (("on", r2), ("above", above(r2)), ("below", below(r2))):
            exp = ("bin", 14, k, l) if side == "below" else ("out",)
            out.append(probe(f"E{n}{side}", "E", _pick(cands, d2, target, "d2 at the neighbour gate"), exp, {"d2": target}))
    return out


# ---------------------------------------------------------------- family F: the skip rule
def pack_skip(pole):
    """The keypoint itself (the pole's fifth point, d2 = 0: skipped), two points a fifth of a millimetre away (d2 in [FLT_MIN,
    FLT_EPSILON): binned by this build, skipped under the FLT_EPSILON reading), and d2 the float below, equal to and above
    FLT_EPSILON (the first skipped under that reading, the others binned under both)."""
    out = [probe("F_origin", "F", pole.kp, ("skip",), {"d2": F32(0)})]
    dirs = pole.free_bins(2e-4, 3, ks=range(4, 7))
    for n, (k, l) in enumerate(dirs[:2]):
        p = (pole.kp64 + (2.2e-4 + 0.6e-4 * n) * pole.mid(k, l)).astype(F32)
        out.append(probe(f"F_tenth{n}", "F", p, ("bin", 0, k, l), {}, expect_eps=("skip",)))
    k, l = dirs[2]
    fine = [a for a in range(3) if a != pole.coarse and abs(pole.kp[a]) < 1e-3]
    assert fine, "no coordinate of the keypoint is near zero: d2 cannot be steered float by float at FLT_EPSILON"
    cands = pole.sweep(pole.kp64 + np.sqrt(float(FLT_EPSILON)) * pole.mid(k, l), fine[0], 40000)
    d2 = pole.q(cands)["d2"]
    for side, target in (("below", below(FLT_EPSILON)), ("on", FLT_EPSILON), ("above", above(FLT_EPSILON))):
        out.append(probe(f"F_eps{side}", "F", _pick(cands, d2, target, "d2 at FLT_EPSILON"), ("bin", 0, k, l), {"d2": target},
                         expect_eps=("skip",) if side == "below" else None))
    return out


# ---------------------------------------------------------------- family G: the density gate
def list_grid_cell(kp, pt, radius=R):
    """desc_body's 12^3 grid: the (x, y, z) cell of a support point, float32 as the kernel computes it."""
    G = 12
    rs = (float(radius) + float(radius) / 5.0) * 1.0001 + 1e-4
    r_sup = np.sqrt(F32(rs * rs))
    cell_w = max(np.sqrt(gates(radius)[1]) * F32(1.001), F32(2.0) * r_sup / F32(G - 1) * F32(1.0001))
    inv = F32(1.0) / cell_w
    kp, pt = np.asarray(kp, F32), np.asarray(pt, F32)
    return tuple(int(min(max(int(np.floor((pt[a] - (kp[a] - r_sup)) * inv)), 0), G - 1)) for a in range(3))


def dense_grid_cell(kp, pt, radius=R):
    """dense_grid's 25 x 25 x 7 grid: the (x, y, z) cell of a support point."""
    DG, DGZ = 25, 7
    rs = (float(radius) + float(radius) / 5.0) * 1.0001 + 1e-4
    r_sup, r_d = np.sqrt(F32(rs * rs)), np.sqrt(gates(radius)[1])
    cw = max(F32(0.5) * r_d * F32(1.001), F32(2.0) * r_sup / F32(DG - 1) * F32(1.0001))
    ch = max(r_d * F32(1.001), F32(2.0) * r_sup / F32(DGZ - 1) * F32(1.0001))
    kp, pt = np.asarray(kp, F32), np.asarray(pt, F32)
    inv = (F32(1.0) / cw, F32(1.0) / cw, F32(1.0) / ch)
    return tuple(int(min(max(int(np.floor((pt[a] - (kp[a] - r_sup)) * inv[a])), 0), (DG, DG, DGZ)[a] - 1)) for a in range(3))


def grid_widths(radius=R):
    """(list grid's cell width, dense grid's cell width, dense grid's layer height, the device's support radius), float64."""
    rs = (float(radius) + float(radius) / 5.0) * 1.0001 + 1e-4
    rd = float(radius) / 5.0
    return max(rd * 1.001, 2 * rs / 11 * 1.0001), max(0.5 * rd * 1.001, 2 * rs / 24 * 1.0001), max(rd * 1.001, 2 * rs / 6 * 1.0001), rs


def _pair(pole, name, n_pos, u, side, n_is_nbr=True, p_is_nbr=True, n_expect=None):
    """Two probes: N at n_pos (float64, rounded) and its partner a density radius from it along u, their mutual d2 the float
    below, on or above r2_density.  Both are far from every edge of the tables: their bins are stated from float64."""
    r2d = gates(pole.radius)[1]
    n_pt = np.asarray(n_pos, F64).astype(F32)
    # (tilted a little off the named separation: the mutual d2 is steered through the fine coordinates)
    u = np.asarray(u, F64) / np.linalg.norm(u) + np.array([0.17, 0.13, 0.19])
    u = u / np.linalg.norm(u)
    cands = pole.near(n_pt.astype(F64) + u * (pole.radius / 5.0), 3e-6)
    d2 = sqdist(cands, n_pt)
    target = {"below": below(r2d), "on": r2d, "above": above(r2d)}[side]
    p_pt = _pick(cands, d2, target, f"mutual d2 {side} the density gate ({name})")

    def expect(pt, is_nbr):
        v = pt.astype(F64) - pole.kp64
        rr = np.linalg.norm(v)
        if not is_nbr:
            assert rr > pole.radius * 1.0001
            return ("out",)
        th = np.degrees(np.arccos(v[2] / rr))
        az = np.degrees(np.arctan2(v[1], v[0]))
        return ("bin", j_of(pole.radius, rr), k_of(th), l_of(az - pole.a0))
    return [probe(f"{name}{side}_n", "G", n_pt, n_expect or expect(n_pt, n_is_nbr), {"mutual_d2": target}, pair=(f"{name}{side}_p", side)),
            probe(f"{name}{side}_p", "G", p_pt, expect(p_pt, p_is_nbr), {"mutual_d2": target}, pair=(f"{name}{side}_n", side))]


def _pair_along_coarse(pole, name, n_pos, side):
    """A pair separated along the keypoint's coarse coordinate (x on an "x" pole; its floats are 0.48 um apart, so d2 cannot be
    steered through it): the partner's coarse offset is the largest float step with dx^2 <= the target, and the remainder
    (under 1e-8 R / 0.05 m^2: an offset of at most 0.6 degrees) is made up along a fine coordinate, float by float."""
    a = pole.coarse
    fine = [i for i in range(3) if i != a and i != 2][0]
    r2d = gates(pole.radius)[1]
    target = {"below": below(r2d), "on": r2d, "above": above(r2d)}[side]
    n_pt = np.asarray(n_pos, F64).astype(F32)
    px = F32(F64(n_pt[a]) + np.sqrt(F64(target)))
    while True:
        dx = F32(px - n_pt[a])
        rem = F64(target) - F64(dx) * F64(dx)
        if rem > (2e-5 * pole.radius / R) ** 2:
            break
        px = below(px)
    base = n_pt.astype(F64)
    base[a] = F64(px)
    base[fine] += np.sqrt(rem)
    cands = pole.sweep(base, fine, 300000)
    d2 = sqdist(cands, n_pt)
    p_pt = _pick(cands, d2, target, f"mutual d2 {side} the density gate along the coarse axis ({name})")
    off = np.degrees(np.arctan2(abs(F64(p_pt[fine]) - F64(n_pt[fine])), abs(F64(p_pt[a]) - F64(n_pt[a]))))
    assert off < 0.7 and p_pt[2] == n_pt[2], off

    def expect(pt):
        v = pt.astype(F64) - pole.kp64
        rr = np.linalg.norm(v)
        return ("bin", j_of(pole.radius, rr), k_of(np.degrees(np.arccos(v[2] / rr))), l_of(np.degrees(np.arctan2(v[1], v[0])) - pole.a0))
    return [probe(f"{name}{side}_n", "G", n_pt, expect(n_pt), {"mutual_d2": target}, pair=(f"{name}{side}_p", side)),
            probe(f"{name}{side}_p", "G", p_pt, expect(p_pt), {"mutual_d2": target}, pair=(f"{name}{side}_n", side))]


def pack_density(pole, axes_names):
    """Pairs of neighbours along the named separations, three twins each."""
    seps = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1), "diag": (1, 1, 1)}
    dirs = pole.free_bins(0.6 * pole.radius, 3 * len(axes_names), ks=range(2, 9))
    out = []
    for a, name in enumerate(axes_names):
        for s, side in enumerate(("below", "on", "above")):
            k, l = dirs[3 * a + s]
            v = mid_shell(pole.radius, 11 + (a + s) % 2) * pole.mid(k, l)
            out += _pair(pole, f"G{name}", pole.kp64 + v, np.array(seps[name], F64), side)
    return out


def pack_density_shell(pole):
    """The partner is a shell point (between R and the support radius): three twins; and the far limit: a neighbour with d2 the
    float below r2_search and a partner collinear beyond it, the float below (and on) the density gate from it — inside the
    device's support set and counted (not counted on the gate)."""
    out = []
    dirs = pole.free_bins(pole.radius, 5, ks=range(3, 8))
    for (k, l), side in zip(dirs[:3], ("below", "on", "above")):
        u = pole.mid(k, l)
        out += _pair(pole, "Gshell", pole.kp64 + 0.93 * pole.radius * u, u, side, p_is_nbr=False)
    r2 = gates(pole.radius)[0]
    for (k, l), side in zip(dirs[3:5], ("below", "on")):
        u = pole.mid(k, l)
        cands = pole.near(pole.kp64 + pole.radius * u, 3e-6)
        n_pt = _pick(cands, pole.q(cands)["d2"], below(r2), "d2 below the neighbour gate")
        pr = _pair(pole, "Gfar", n_pt.astype(F64), u, side, p_is_nbr=False, n_expect=("bin", 14, k, l))
        pr[0]["claim"]["d2"] = below(r2)
        out += pr
    return out


def pack_list_grid(pole):
    """Pairs the float below the density gate apart (each counts the other) whose cells in desc_body's 12^3 grid differ by one in
    x, in y, in z and in all three; a pair inside the first cell of a row (index 0, where the clamp ends) and one inside the
    last cell a support point can reach (index 10; cell 11 begins 1.0001 support diameters out)."""
    cw, _, _, rs = grid_widths(pole.radius)
    g0 = pole.kp64 - rs
    o = int(np.argmax(np.abs(pole.out)))          # the outward axis (x on the "x" poles)
    sgn = 1.0 if pole.out[o] > 0 else -1.0
    others = [a for a in range(3) if a != o]
    h = pole.radius / 10.0

    def border(axis, want):  # the cell border of `axis` nearest to kp + want
        m = np.rint((pole.kp64[axis] + want - g0[axis]) / cw)
        return g0[axis] + m * cw

    def unit(axis, s=1.0):
        u = np.zeros(3)
        u[axis] = s
        return u
    out = []
    # along the outward axis
    base = pole.kp64.copy()
    sc = pole.radius / R  # (the offsets below are written for R = 5 cm)
    base[o] = border(o, sgn * 0.022 * sc) - h
    base[others[0]] += 0.002 * sc
    out += _pair(pole, "Gcell_o", base, unit(o), "below")
    # across the two other axes
    for n, a in enumerate(others):
        base = pole.kp64.copy()
        base[o] += sgn * 0.012 * sc
        base[a] = border(a, (-0.022 if n == 0 else 0.022) * sc) - h
        base[others[1 - n]] -= 0.003 * sc
        out += _pair(pole, f"Gcell_{'xyz'[a]}", base, unit(a), "below")
    # all three at once
    corner = np.array([border(a, sc * (sgn * 0.03 if a == o else (0.012 if a == others[0] else -0.014))) for a in range(3)])
    out += _pair(pole, "Gcell_all", corner - h / np.sqrt(3.0) * np.ones(3), np.ones(3), "below")
    # the first cell and the last reachable one of the first other axis
    a = others[0]
    for name, s in (("first", -1.0), ("last", 1.0)):
        base = pole.kp64.copy()
        base[o] += sgn * 0.005 * sc
        base[a] += s * 0.0493 * sc
        base[others[1]] += (0.001 if s < 0 else -0.001) * sc
        out += _pair(pole, f"Gcell_{name}", base, unit(a, s), "below", p_is_nbr=False)
    return out


def pack_dense_grid(pole):
    """Pairs whose cells in dense_grid differ by exactly two in x, two in y and one layer in z: the float below the gate (counted)
    and on it (not counted)."""
    _, cw, ch, rs = grid_widths(pole.radius)
    g0 = pole.kp64 - rs
    o = int(np.argmax(np.abs(pole.out)))
    sgn = 1.0 if pole.out[o] > 0 else -1.0
    others = [a for a in range(3) if a != o]
    out = []
    # (outward offset, offsets along the two other axes) of the six pairs: more than 2.5 density radii from one another
    spots = [(0.010, -0.022, -0.015), (0.010, 0.018, -0.015), (0.010, -0.022, 0.018), (0.010, 0.018, 0.018), (0.034, -0.016, 0.0), (0.034, 0.016, 0.0)]
    for a in range(3):
        w = ch if a == 2 else cw
        for t, side in enumerate(("below", "on")):
            s = [v * pole.radius / R for v in spots[2 * a + t]]
            base = pole.kp64.copy()
            base[o] += sgn * s[0]
            base[others[0]] += s[1]
            base[others[1]] += s[2]
            # N 0.3 cells under a border of axis a: the partner a density radius (1.996 cells, half a layer) further is two
            # cells (one layer) on
            m = np.floor((base[a] - g0[a]) / w)
            base[a] = g0[a] + (m + 1) * w - 0.3 * cw
            u = np.zeros(3)
            u[a] = 1.0
            if a == pole.coarse:  # along the coarse axis to within 0.6 degrees: the end of a row's chord in k_dense_density
                out += _pair_along_coarse(pole, f"Gdense_{'xyz'[a]}", base, side)
            else:
                out += _pair(pole, f"Gdense_{'xyz'[a]}", base, u, side)
    return out


# ---------------------------------------------------------------- scenes
# kind: the packs of each scan, a pole (and so a row, and an x-axis ordinal) each
PACKS = {
    "x": [[("A", (1, 5, 9, 13)), ("A", (2, 6, 10, 14)), ("A", (3, 7, 11, 15)), ("A", (4, 8, 12))],
          [("B", (1, 4, 7, 10)), ("B", (2, 5, 8)), ("B", (3, 6, 9)), ("E", None)],
          [("G", ("x", "y")), ("G", ("z", "diag")), ("Gshell", None), ("Gcell", None)],
          [("Gdense", None)]],
    "ztop": [[("C", (1, 2, 3, 4)), ("C", (2, 5, 8, 11)), ("D", None)],
             [("C", (5, 6, 7, 8)), ("C", (3, 6, 9, 12))],
             [("C", (9, 10, 11, 12)), ("C", (1, 4, 7, 10))]],
    "zbot": [[("D", None)]],
    "f": [[("F", None)]],
    "z0": [[("Fmin", None)]],
    # one pole with the dense grid's pairs alone: the row of tests/test_gpu_desc_edges.py's target-window case
    "xw": [[("Gdense", None)]],
    # R = 0.5 m: the pole's own points (10 .. 32 cm from the keypoint) are part of every support set
    "xr": [[("A", (1, 5, 9, 13)), ("A", (2, 6, 10, 14)), ("A", (3, 7, 11, 15)), ("A", (4, 8, 12))],
           [("G", ("x", "y")), ("G", ("z", "diag")), ("Gshell", None), ("Gcell", None)],
           [("Gdense", None)]],
}
FAMILIES = {"A": "A", "B": "B", "C": "C", "D": "D", "E": "E", "F": "F", "Fmin": "F", "G": "G", "Gshell": "G", "Gcell": "G", "Gdense": "G"}


def _build_pack(pole, what, arg):
    if what == "A":
        return pack_radial(pole, arg, shell0=len(arg) < 4)
    if what == "B":
        return pack_theta(pole, arg)
    if what == "C":
        pr, found = pack_phi(pole, arg)
        pole.phi_found = found
        return pr
    if what == "D":
        return pack_pole(pole)
    if what == "E":
        return pack_gate(pole)
    if what == "F":
        return pack_skip(pole)
    if what == "Fmin":
        return pack_skip_min(pole)
    if what == "G":
        return pack_density(pole, arg)
    if what == "Gshell":
        return pack_density_shell(pole)
    if what == "Gcell":
        return pack_list_grid(pole)
    if what == "Gdense":
        return pack_dense_grid(pole)
    raise KeyError(what)


def _oracle():
    from oracle import oracle_py
    oracle_py.load()
    return oracle_py


def _scan_of(xyz):
    s = np.zeros((len(xyz), 4), F32)
    s[:, :3] = xyz
    return s


@functools.lru_cache(maxsize=None)
def packs(name):
    """(params, [scan: [(Pole, what, [probe])]]) of a kind: the poles, their keypoints and ordinals from the oracle on the poles
    alone (the probes are unseen: the final scenes assert that nothing moved), and every pack's probes.  Built once a process."""
    ora = _oracle()
    kind, radius = KINDS[name]
    p = kind_params(kind, radius)
    out = []
    for spec in PACKS[name]:
        pts = []
        for i, _ in enumerate(spec):
            axis = du.AXES[i]
            if kind == "f":
                pl = du.pole(p, axis, du.origin_z(ora, p, axis))
            else:
                pl = du.pole(p, axis)
                pl = pl[8:12] if kind == "ztop" else pl[0:4] if kind == "zbot" else pl[4:8] if kind == "z0" else pl
            pts.append(pl)
        kps = ora.run(p, _scan_of(np.concatenate(pts)))["keypoints"][:, :3]
        assert len(kps) == len(spec), f"{kind}: {len(kps)} keypoints from {len(spec)} poles"
        row = []
        for i, (what, arg) in enumerate(spec):
            own = [o for o, kp in enumerate(kps) if np.abs(pts[i][:, :2].astype(F64).mean(axis=0) - kp[:2]).max() < 0.05]
            assert len(own) == 1
            kp = kps[own[0]]
            a = np.array([du.AXES[i][0], du.AXES[i][1], 0.0])
            if kind == "x":
                face, margin = a, 0.002
            elif kind == "f":
                face, margin = a, 5e-5
            elif kind in ("ztop", "z0"):
                face, margin = np.array([0.0, 0.0, 1.0]), float(p.z_max) - float(kp[2])
            else:
                face, margin = np.array([0.0, 0.0, -1.0]), float(kp[2]) - float(p.z_min)
            margin += 2e-5 if kind == "f" else 0.0 if kind == "z0" else 2e-4
            pole = Pole(kind, du.AXES[i], pts[i], kp, own[0], face, margin, radius)
            pr = _build_pack(pole, what, arg)
            assert len(pr) <= 12, f"{kind} {what}: a pack of {len(pr)} probes"
            assert len({q["name"] for q in pr}) == len(pr)
            row.append((pole, what, pr))
        out.append(row)
    return p, out


def _filler(pole, probes, n, rng):
    """n shell points (1.05 R .. 1.15 R from the keypoint, unseen by the detector), more than R / 5 + 0.5 mm from every probe."""
    radius = pole.radius
    t1 = np.cross(pole.out, [0.3, 0.5, 0.8])
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(pole.out, t1)
    px = np.array([q["xyz"] for q in probes], F64).reshape(-1, 3)
    out = np.zeros((0, 3), F32)
    while len(out) < n:
        m = 4 * (n - len(out)) + 16
        c, th = rng.uniform(0.3, 1.0, m), rng.uniform(0.0, 2 * np.pi, m)
        s = np.sqrt(1.0 - c * c)
        d = c[:, None] * pole.out + (s * np.cos(th))[:, None] * t1 + (s * np.sin(th))[:, None] * t2
        pts = (pole.kp64 + d * rng.uniform(1.05 * radius, 1.15 * radius, (m, 1))).astype(F32)
        keep = (pts.astype(F64) - pole.kp64) @ pole.out > pole.margin + 1e-3
        if len(px):
            keep &= np.linalg.norm(pts[:, None, :].astype(F64) - px[None], axis=2).min(axis=1) > radius / 5.0 + 5e-4
        out = np.concatenate([out, pts[keep]])
    return out[:n]


def support_count(pole, cloud):
    lo, hi = du.support_radii(pole.radius)
    d2 = sqdist(np.asarray(cloud, F32).reshape(-1, 3), pole.kp)
    n_lo, n_hi = int((d2 < lo * lo).sum()), int((d2 < hi * hi).sum())
    return n_lo, n_hi


@functools.lru_cache(maxsize=None)
def scenes(name, support):
    """(params, [(scan, oracle result, [(Pole, what, probes, first index of the probes in the scan)])]): every row of the kind
    padded to exactly `support` support points (by the oracle's radius and the device's alike).  Nobody writes into it."""
    ora = _oracle()
    kind = KINDS[name][0]
    p, rows = packs(name)
    out = []
    for si, row in enumerate(rows):
        fill, tail, where = [], [], []
        for pole, what, pr in row:
            own = np.array([q["xyz"] for q in pr], F32)
            if kind == "f":  # the origin probe IS the pole's fifth point: it is already in the scan
                own = own[1:]
            have = support_count(pole, np.concatenate([own, pole.pts]))
            assert have[0] == have[1] and have[0] <= support, f"{kind} {what}: {have} support points before the filler, wanted {support}"
            rng = np.random.default_rng(5000 + 131 * si + 7 * pole.ordinal + support)
            fill.append(_filler(pole, pr, support - have[0], rng))
            tail.append(own)
        xyz = [f for f in fill] + [pole.pts for pole, _, _ in row]
        at = sum(len(a) for a in xyz)
        for (pole, what, pr), own in zip(row, tail):
            where.append((pole, what, pr, at))
            at += len(own)
        scan = _scan_of(np.concatenate(xyz + tail))
        res = ora.run(p, scan)
        assert res["n_keypoints"] == len(row)
        for pole, what, pr, _ in where:
            assert (res["keypoints"][pole.ordinal, :3].view(np.uint32) == pole.kp.view(np.uint32)).all(), f"{kind}: the probes moved a keypoint"
            assert support_count(pole, scan[:, :3]) == (support, support), f"{kind} {what}: {support_count(pole, scan[:, :3])} support points"
        out.append((scan, res, where))
    return p, out


def probe_index(kind, pr, first, i):
    """Index in the scan of probe i of a pack whose probes start at `first` (the "f" kind's origin is a point of the pole)."""
    return first + i - (1 if kind == "f" else 0)


def rho_expected(pole, scan, probes, names):
    """The local density of every probe, stated from float64 distances between the scan's float32 points: the points within R / 5,
    itself included; the gate partner counts iff the pair was built below the gate.  No other point may be within a micrometre of
    the gate (its side could not be stated from float64)."""
    cloud = scan[:, :3].astype(F64)
    rd = pole.radius / 5.0
    out = []
    for q in probes:
        d = np.linalg.norm(cloud - q["xyz"].astype(F64), axis=1)
        gate = np.abs(d - rd) < 1e-6
        n = int((d < rd).sum())
        if q["pair"] is not None:
            partner = names[q["pair"][0]]
            pd = np.linalg.norm(partner.astype(F64) - q["xyz"].astype(F64))
            assert abs(pd - rd) < 1e-6 and int(gate.sum()) == 1, q["name"]
            n = n - int(pd < rd) + (1 if q["pair"][1] == "below" else 0)
        else:
            assert not gate.any(), f"{q['name']}: a point within a micrometre of its density gate"
        out.append(n)
    return out


def check_row(pole, what, probes, first, scan, st, tag, skip_epsilon=False):
    """The statement's row `st` against the pack's table: every probe's state, bin and density.  Raises naming family, probe, the
    expected and the found value."""
    names = {q["name"]: q["xyz"] for q in probes}
    rho = rho_expected(pole, scan, probes, names)
    for i, q in enumerate(probes):
        at = probe_index(pole.kind, probes, first, i)
        if pole.kind == "f" and i == 0:
            at = int(np.flatnonzero((scan[:, :3].view(np.uint32) == q["xyz"].view(np.uint32)).all(axis=1))[0])
        assert (scan[at, :3].view(np.uint32) == q["xyz"].view(np.uint32)).all(), f"{tag}: probe {q['name']} is not at {at}"
        exp = q["expect_eps"] if skip_epsilon else q["expect"]
        state = int(st["state"][at])
        got = ("out",) if state == 0 else ("skip",) if state == 1 else ("bin", int(st["j"][at]), int(st["k"][at]), int(st["l"][at]))
        assert got == exp, f"{tag}: family {q['family']}, probe {q['name']}: expected {exp}, found {got}"
        if exp[0] == "bin":
            assert int(st["rho"][at]) == rho[i], f"{tag}: family {q['family']}, probe {q['name']}: expected rho {rho[i]}, found {int(st['rho'][at])}"


def explain(pole, what, probes, first, scan, got_row, want_row, tag):
    """Which probes' bins differ between two rows (a device row and the statement's): family, probe, bin, both values."""
    bad = np.flatnonzero((np.asarray(got_row[:J * K * L]).view(np.uint32) != np.asarray(want_row[:J * K * L]).view(np.uint32))
                         & ~((got_row[:J * K * L] == 0) & (want_row[:J * K * L] == 0)))
    lines = [f"{tag}: {len(bad)} words differ (pack {what}, {pole.kind} pole, ordinal {pole.ordinal})"]
    for b in bad[:12]:
        l, k, j = b // (K * J), b // J % K, b % J
        who = [q["name"] for q in probes if q["expect"] == ("bin", j, k, l)]
        lines.append(f"  bin (j {j}, k {k}, l {l}): found {got_row[b]!r}, expected {want_row[b]!r}; probes stated there: {who or 'none'}")
    return "\n".join(lines)


# ---------------------------------------------------------------- what a context reports, and other builds of the library
def group_class_counts(ctx):
    """The last batch's group rows by size class (fx_debug_group_classes)."""
    import ctypes as C
    from feature_extraction_amd import capi
    cnt = (C.c_uint32 * 3)()
    ctx.lib.fx_debug_group_classes.argtypes = [C.c_void_p, C.c_void_p]
    capi.check(ctx.lib.fx_debug_group_classes(ctx.handle, cnt))
    return [int(c) for c in cnt]


def dense_row_count(ctx):
    """Rows the last batch handed to the dense tier (fx_debug_tier_hints()[4])."""
    import ctypes as C
    from feature_extraction_amd import capi
    h = (C.c_uint32 * 8)()
    ctx.lib.fx_debug_tier_hints.argtypes = [C.c_void_p, C.c_void_p]
    capi.check(ctx.lib.fx_debug_tier_hints(ctx.handle, h))
    return int(h[4])


def with_library(path, fn):
    """fn() with `path` as the library capi loads (a measurement build), the process's own restored afterwards."""
    from feature_extraction_amd import capi
    saved = capi.LIB_PATH, capi._lib
    capi.LIB_PATH, capi._lib = path, None
    try:
        return fn()
    finally:
        capi.LIB_PATH, capi._lib = saved


def size_class(n_support):
    """The group tier's size class of a row (16 / 32 / 64 support points); None: not a group row."""
    return next((c for c, cap in enumerate((16, 32, 64)) if n_support <= cap), None)


# ---------------------------------------------------------------- k_dense_density's target windows, restated
DENSE_WINDOW = 2048  # FX_DDENS_C: targets a window
WINDOW_SUPPORT = 20000  # support points of the "xw" row: its z pairs then lie in two windows (tests/test_desc_edges_scenes.py)


def dense_concatenation(pole, cloud):
    """Where k_dense_density finds every support point of a dense row, restated from the kernels' text for a row whose binned
    neighbours are all its own queries (no other row claims them: the poles are metres apart) and fill one work item (at most
    1024 query slots).  k_dense_sort stores the support set cell by cell, cell-major (cz 25 + cy) 25 + cx, and lists the queries
    cell by cell, each cell's padded to fours: a quad is up to four queries of ONE cell.  The item's box is the union of its
    quads' reach: two cells either side in y, one layer either side in z, and in x the cells of (x - hmax, x + hmax).  The rows
    (cz, cy) of the box, each cut to the box's x cells, are laid end to end (z-major) and pass through LDS in windows of 2048.
    Returns (t_tot, {point index: (window of its cell's first target, window of its cell's last target)}) — the order
    inside a cell is the sort's own, so a cell wholly inside one window is what can be stated."""
    DG, DGZ = 25, 7
    radius = pole.radius
    cloud = np.ascontiguousarray(cloud, F32)
    rs = (radius + radius / 5.0) * 1.0001 + 1e-4
    r2_support = F32(rs * rs)
    r2_search, r2d = gates(radius)
    r_sup, r_d = np.sqrt(r2_support), np.sqrt(r2d)
    cw = max(F32(0.5) * r_d * F32(1.001), F32(2.0) * r_sup / F32(DG - 1) * F32(1.0001))
    ch = max(r_d * F32(1.001), F32(2.0) * r_sup / F32(DGZ - 1) * F32(1.0001))
    inv_cw, inv_ch = F32(1.0) / cw, F32(1.0) / ch
    g0 = pole.kp - r_sup

    def cxy(v, a):
        return np.clip(np.floor((np.asarray(v, F32) - g0[a]) * inv_cw), 0, DG - 1).astype(np.int64)

    def cz(v):
        return np.clip(np.floor((np.asarray(v, F32) - g0[2]) * inv_ch), 0, DGZ - 1).astype(np.int64)
    d2 = sqdist(cloud, pole.kp)
    sup = np.flatnonzero(d2 < r2_support)
    use = np.flatnonzero((d2 < r2_search) & ~(np.abs(d2) < FLT_MIN))
    cell = {i: (int(cxy(cloud[i, 0], 0)), int(cxy(cloud[i, 1], 1)), int(cz(cloud[i, 2]))) for i in sup}
    counts = np.zeros((DGZ, DG, DG), np.int64)  # [cz, cy, cx]
    for i in sup:
        x, y, z = cell[i]
        counts[z, y, x] += 1
    # the quads: the queries of a cell, four at a time
    by_cell = {}
    for i in use:
        by_cell.setdefault(cell[i], []).append(i)
    assert sum((len(v) + 3) // 4 * 4 for v in by_cell.values()) <= 1024, "more than one work item"
    cw_k, ch_k = F32(1.0) / inv_cw, F32(1.0) / inv_ch
    eps_w = F32(1e-3) * cw_k
    rr = r_d * F32(1.0001)
    hmax = rr * F32(1.0001) + eps_w
    assert ch_k > 0
    box = dict(y0=DG, y1=-1, z0=DGZ, z1=-1, x0=DG, x1=-1)
    for members in by_cell.values():  # (the box of a cell's quads: within the cell; the union over its quads is the cell's queries')
        pts = cloud[members]
        y0, y1 = int(cxy(pts[:, 1].min(), 1)), int(cxy(pts[:, 1].max(), 1))
        z0, z1 = int(cz(pts[:, 2].min())), int(cz(pts[:, 2].max()))
        box["y0"], box["y1"] = min(box["y0"], max(y0 - 2, 0)), max(box["y1"], min(y1 + 2, DG - 1))
        box["z0"], box["z1"] = min(box["z0"], max(z0 - 1, 0)), max(box["z1"], min(z1 + 1, DGZ - 1))
        box["x0"] = min(box["x0"], int(cxy(pts[:, 0].min() - hmax, 0)))
        box["x1"] = max(box["x1"], int(cxy(pts[:, 0].max() + hmax, 0)))
    start, pos = {}, 0
    for z in range(box["z0"], box["z1"] + 1):
        for y in range(box["y0"], box["y1"] + 1):
            for x in range(box["x0"], box["x1"] + 1):
                start[(x, y, z)] = pos
                pos += int(counts[z, y, x])
    t_tot = pos
    where = {}
    for i in sup:
        c = cell[i]
        if c in start:
            where[int(i)] = (start[c] // DENSE_WINDOW, (start[c] + int(counts[c[2], c[1], c[0]]) - 1) // DENSE_WINDOW)
    return t_tot, where
