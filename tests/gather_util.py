"""The support gather pinned directly (tests/test_gpu_gather_sets.py; the CPU checks of its scenes: tests/test_gather_scenes.py).

Two halves.

A plain numpy reference of what k_gather and its instances leave on the device (Context.gather_state reads it back in the test
build): every keypoint's support set, the has-a-neighbour flags and with them the 3DSC x-axis ordinals, the rows' classes and
work lists, and the streaming pass's near-sector bits.  Everything is float32 in the kernels' operation order, so every
comparison is exact: no tolerance anywhere in this file.
  rotation     ((R0 x + R1 y) + R2 z) + 0, R from fx_rotation_from_roll_pitch
  surface      a point is part of the search surface iff its three rotated coordinates are finite
  distance     d2 = ((dx dx) + dy dy) + dz dz, dx = kp.x - p.x (dist2 in csrc/fx_kernels.hip)
  support set  {i : d2 < r2_support}, strict; a keypoint has a neighbour iff some d2 < r2_search
  near bits    sector s (points 4 s .. 4 s + 3) is near iff one of its points below n lies inside the filter box widened by
               box_margin: float32(limit -+ margin), then >= / <=; NaN fails
The reference is brute force: it knows nothing of cells, tiles, sectors, queues, stages or slices.

Scene builders on tests/desc_rows_util.py's poles and parameters (cloud_leveling = 0, the filter's x / y windows 2 mm behind the
poles, R = 5 cm): what they add is control over WHERE in the scan a support point sits.  Filler points lie 300 m and more
behind the sensor, far outside the widened box: their sectors must stay clear."""
import ctypes as C
import functools

import numpy as np

from feature_extraction_amd import capi
from tests import desc_rows_util as du
from tests import util

R = du.R
D = du.D
ROW_GROUP, ROW_WAVE, ROW_LIST, ROW_DENSE, ROW_DENSE_FAIL = 0, 1, 2, 3, 4  # FX_ROW_* (csrc/fx_device.h)
FX_NONE = 0xffffffff
GROUP_CAP, WAVE_CAP, DENSE_MIN = 64, 192, 1024          # FX_GROUP_CAP, FX_WAVE_CAP, kDenseMin
F32 = np.float32


# ---------------------------------------------------------------- constants
def constants(radius=R):
    """(r2_support, r2_search, box_margin) as fx_create computes them (csrc/fx_api.cpp): doubles, narrowed once."""
    radius = float(radius)
    rs = (radius + radius / 5.0) * 1.0001 + 1e-4
    return F32(rs * rs), F32(radius * radius), F32(rs * 1.001 + 1e-3)


def support_radius(radius=R):
    return (float(radius) + float(radius) / 5.0) * 1.0001 + 1e-4


def rotation(roll, pitch):
    out = np.zeros(9, F32)
    capi.load().fx_rotation_from_roll_pitch(float(roll), float(pitch), out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


@functools.lru_cache(maxsize=None)
def xaxis_table(n):
    """Entries 0 .. n - 1 of fx_sc3d_xaxis' table, [n, 2] float32."""
    lib = capi.load()
    out = np.zeros((n, 2), F32)
    for k in range(n):
        lib.fx_sc3d_xaxis(k, out[k].ctypes.data_as(C.POINTER(C.c_float)))
    return out


def rotate(scan, rot9):
    x, y, z = (np.ascontiguousarray(scan[:, i], F32) for i in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((rot9[3 * i] * x + rot9[3 * i + 1] * y) + rot9[3 * i + 2] * z) + F32(0) for i in range(3)], axis=1)


def dist2(kp, pts):
    """d2 of every row of pts [n, 3] from keypoint kp [3], float32, the kernel's order."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = kp[0] - pts[:, 0], kp[1] - pts[:, 1], kp[2] - pts[:, 2]
        return (dx * dx + dy * dy) + dz * dz


def near_sectors(p, rot, box_margin):
    """bool per sector of four points: some point of it (below n) lies inside the filter box widened by box_margin."""
    m = F32(box_margin)
    lo = [F32(p.x_min) - m, F32(p.y_min) - m, F32(p.z_min) - m]
    hi = [F32(p.x_max) + m, F32(p.y_max) + m, F32(p.z_max) + m]
    with np.errstate(invalid="ignore"):
        near = np.ones(len(rot), bool)
        for a in range(3):
            near &= (rot[:, a] >= lo[a]) & (rot[:, a] <= hi[a])
    pad = (-len(near)) % 4
    return np.concatenate([near, np.zeros(pad, bool)]).reshape(-1, 4).any(axis=1)


class Reference:
    """Brute force over one scan and its keypoints [K, >= 3] (float32, the rotated frame the detector emits them in)."""

    def __init__(self, p, scan, keypoints, roll=0.0, pitch=0.0, radius=None):
        radius = float(p.descriptor_radius) if radius is None else radius
        self.r2_support, self.r2_search, self.box_margin = constants(radius)
        self.n = len(scan)
        self.rot = rotate(scan, rotation(roll, pitch))
        self.kp = np.ascontiguousarray(np.asarray(keypoints, F32)[:, :3])
        surface = np.isfinite(self.rot).all(axis=1)
        self.sets, self.has_nbr, self.n_nbr = [], np.zeros(len(self.kp), bool), np.zeros(len(self.kp), np.int64)
        # (a coarse float64 cut first — 1.5 support radii, far beyond any rounding — keeps the exact float32 test small)
        cut = 2.25 * float(self.r2_support)
        rot64 = np.where(surface[:, None], self.rot, np.inf).astype(np.float64)
        for k, kp in enumerate(self.kp):
            with np.errstate(invalid="ignore"):
                cand = np.flatnonzero(((rot64 - kp.astype(np.float64)) ** 2).sum(axis=1) < cut)
            d2 = dist2(kp, self.rot[cand])
            self.sets.append(cand[d2 < self.r2_support].astype(np.int64))
            self.n_nbr[k] = int((d2 < self.r2_search).sum())  # (what 3DSC's radius search returns; the kernels only need "any")
            self.has_nbr[k] = self.n_nbr[k] > 0
        self.near = near_sectors(p, self.rot, self.box_margin)

    def d2(self, k, i):
        return dist2(self.kp[k], self.rot[i:i + 1])[0]

    def counts(self):
        return np.array([len(s) for s in self.sets], np.int64)


def row_class(n_support, list_cap):
    """FX_ROW_* of a row of n_support support points (classify_rows; pools with room), and its group size class (or -1)."""
    if n_support > min(list_cap, DENSE_MIN):
        return ROW_DENSE, -1
    if n_support <= GROUP_CAP:
        return ROW_GROUP, 0 if n_support <= 16 else 1 if n_support <= 32 else 2
    return (ROW_WAVE if n_support <= WAVE_CAP else ROW_LIST), -1


# ---------------------------------------------------------------- the comparison
def check_state(st, got, refs, tag, check_near=True, dense_cap=None):
    """st: Context.gather_state() after a batch; got: what process_host returned for it; refs: a Reference a scan (None: a scan
    that must have no keypoints).  dense_cap: the dense tier's pool of sorted entries (FxDevParams::dense_cap = max(4096,
    limits.max_dense_points)) when the scene is meant to exhaust it — the dense rows then draw their regions in row order (one
    scan of up to 64 keypoints: one wavefront classifies them, a row a lane), a row that does not fit is FX_ROW_DENSE_FAIL, rides in
    the widest group class's list and leaves FX_NONE in its slot of dense_rows.  Raises AssertionError naming the kind (tag), the scan, the keypoint, the point index and its d2."""
    B = len(refs)
    assert st["batch"] == B, f"{tag}: the state is of a batch of {st['batch']} scans, not {B}"
    list_cap, ovf_cap = st["list_cap"], st["ovf_cap"]
    row0, pool = 0, 0
    want_class, want_gcls = [], []
    for b, ref in enumerate(refs):
        K = got[b]["n_keypoints"]
        where = f"{tag}: scan {b}"
        if ref is None:
            assert K == 0, f"{where}: {K} keypoints in a scan that has none"
        else:
            assert K == len(ref.kp), f"{where}: {K} keypoints, the reference was built for {len(ref.kp)}"
            assert (util.bits(got[b]["keypoints"][:, :3]) == util.bits(ref.kp)).all(), f"{where}: the keypoints are not the reference's"
        if check_near:
            n = ref.n if ref is not None else int(got[b].get("n_points", 0))
            want = ref.near if ref is not None else np.zeros(0, bool)
            bits = np.unpackbits(st["near_bits"][b].view(np.uint8), bitorder="little")[:len(want)].astype(bool)
            # (every sector, the last, partial one included: the streaming pass loads a lane past the scan's end from the
            #  clamped address of the last record and sets its x to NaN, which fails the box — prep_stream's load_tile)
            bad = np.flatnonzero(bits != want)
            assert len(bad) == 0, (f"{where}: {len(bad)} near-sector bits differ, first sector {bad[0]} (points {4 * bad[0]} .. "
                                   f"{4 * bad[0] + 3} of {n}): device {int(bits[bad[0]])}, reference {int(want[bad[0]])}")
        if K == 0:
            continue
        assert row0 + K <= st["rows"], f"{where}: rows {row0} .. {row0 + K} of {st['rows']}"
        rows = np.arange(row0, row0 + K)
        assert (st["row_map"][rows, 0] == b).all() and (st["row_map"][rows, 1] == np.arange(K)).all(), f"{where}: row_map {st['row_map'][rows].tolist()[:4]} .."
        assert (util.bits(st["row_kp"][rows, :3]) == util.bits(ref.kp)).all(), f"{where}: row_kp is not the scan's keypoints"
        n_ovf = min(int(st["ovf_cnt"][b]), ovf_cap)
        ovf_kp, ovf_pts = st["ovf_kp"][b, :n_ovf], st["ovf_pts"][b, :n_ovf]
        over = 0
        for k in range(K):
            row, want = row0 + k, ref.sets[k]
            cnt = int(st["s_cnt"][row])
            ent = np.concatenate([st["s_pts"][row, :min(cnt, list_cap)], ovf_pts[ovf_kp == k]])
            idx = ent[:, 3].copy().view(np.uint32).astype(np.int64)
            here = f"{where}, keypoint {k} (row {row})"

            def name(i):
                if not 0 <= i < ref.n:
                    return f"point {i} (not a point of the scan: n = {ref.n})"
                return f"point {i} (d2 = {ref.d2(k, i)!r}; r2_support = {ref.r2_support!r})"
            missing, extra = np.setdiff1d(want, idx), np.setdiff1d(idx, want)
            uniq, times = np.unique(idx, return_counts=True)
            assert len(missing) == 0, f"{here}: {len(missing)} support points are missing from the list, first {name(int(missing[0]))}"
            assert len(extra) == 0, f"{here}: {len(extra)} entries are no support points, first {name(int(extra[0]))}"
            assert (times == 1).all(), f"{here}: {name(int(uniq[times > 1][0]))} is stored {int(times.max())} times"
            assert cnt == len(want), f"{here}: s_cnt {cnt}, the support set has {len(want)} points"
            bad = np.flatnonzero((util.bits(ent[:, :3]) != util.bits(ref.rot[idx])).any(axis=1))
            assert len(bad) == 0, (f"{here}: the stored coordinates of point {int(idx[bad[0]])} are {ent[bad[0], :3].tolist()}, "
                                   f"rotated it is {ref.rot[idx[bad[0]]].tolist()}")
            over += max(0, cnt - list_cap)
            cls, gcls = row_class(len(want), list_cap)
            if cls == ROW_DENSE and dense_cap is not None:
                fits = pool <= dense_cap and len(want) <= dense_cap - pool
                pool += len(want)  # (a row without room has drawn its entries all the same)
                if not fits:
                    cls, gcls = ROW_DENSE_FAIL, 2
            want_class.append(cls), want_gcls.append(gcls)
            assert int(st["row_class"][row]) == cls, f"{here}: row_class {int(st['row_class'][row])}, {len(want)} support points make it {cls}"
        assert over <= ovf_cap, f"{where}: the scene overflows the overflow region ({over} > {ovf_cap})"
        assert int(st["ovf_cnt"][b]) == over, f"{where}: ovf_cnt {int(st['ovf_cnt'][b])}, the lists overflow by {over}"
        # a keypoint without a neighbour draws no x-axis: keypoint k takes entry (earlier keypoints of the scan that have one)
        ordinal = np.cumsum(ref.has_nbr) - ref.has_nbr
        want_xa = xaxis_table(int(ordinal.max()) + 1)[ordinal]
        bad = np.flatnonzero((util.bits(st["row_xa"][rows]) != util.bits(want_xa)).any(axis=1))
        assert len(bad) == 0, (f"{where}, keypoint {bad[0]} (row {row0 + bad[0]}): row_xa {st['row_xa'][row0 + bad[0]].tolist()} is not x-axis "
                               f"{int(ordinal[bad[0]])} {want_xa[bad[0]].tolist()} ({int(ref.has_nbr[:bad[0]].sum())} of the {bad[0]} keypoints before it have a neighbour)")
        row0 += K
    assert st["rows"] == row0, f"{tag}: {st['rows']} rows, the scans have {row0} keypoints"
    want_class, want_gcls = np.array(want_class, np.int64), np.array(want_gcls, np.int64)
    lists = [("list_desc", st["list_desc"], st["n_list"], want_class == ROW_LIST), ("wave_desc", st["wave_desc"], st["n_wave"], want_class == ROW_WAVE),
             ("dense_rows", st["dense_rows"], st["n_dense"], want_class == ROW_DENSE)]
    in_group = (want_class == ROW_GROUP) | (want_class == ROW_DENSE_FAIL)
    lists += [(f"group_desc[{c}]", st["group_desc"][c], st["n_group"][c], in_group & (want_gcls == c)) for c in range(3)]
    n_fail = int((want_class == ROW_DENSE_FAIL).sum())
    for name_, lst, counter, mask in lists:
        want_rows = np.flatnonzero(mask)
        if name_ == "dense_rows":  # (a slot each, the rows without room too)
            want_rows = np.concatenate([want_rows, np.full(n_fail, FX_NONE, np.int64)])
        assert counter == len(want_rows), f"{tag}: the counter of {name_} is {counter}, {len(want_rows)} rows are of its class"
        assert sorted(lst.tolist()) == want_rows.tolist(), f"{tag}: {name_} holds rows {sorted(lst.tolist())[:8]} .., its class is rows {want_rows.tolist()[:8]} .."


# ---------------------------------------------------------------- scene builders
def filler(n, seed=0):
    """n points 300 m and more behind the sensor, all different: outside the widened box by hundreds of metres."""
    i = np.arange(n)
    out = np.zeros((n, 4), F32)
    out[:, 0] = -300.0 - (i % 997) * 0.25
    out[:, 1] = ((i * 31 + seed) % 1013) * 0.05 - 25.0
    out[:, 2] = ((i * 17) % 101) * 0.01 - 0.5
    return out


def pole_keypoint(oracle, p, axis, **kw):
    pl = du.pole(p, axis, **kw)
    s = np.zeros((len(pl), 4), F32)
    s[:, :3] = pl
    kp = oracle.run(p, s)["keypoints"]
    assert len(kp) == 1
    return pl, kp[0, :3].astype(np.float64)


def around(rng, kp, axis, n, r_lo, r_hi):
    """n points r_lo .. r_hi from kp, at least half of that beyond it along the axis (behind the filter's window: the detector
    never sees them) — desc_rows_util.scene's rule."""
    a = np.array(axis)
    c, th = rng.uniform(0.5, 1.0, n), rng.uniform(0.0, 2 * np.pi, n)
    s = np.sqrt(1.0 - c * c)
    d = np.stack([c * a[0] - s * np.cos(th) * a[1], c * a[1] + s * np.cos(th) * a[0], s * np.sin(th)], axis=1)
    return (kp + d * rng.uniform(r_lo, r_hi, (n, 1))).astype(F32)


def support_points(rng, kp, axis, n):
    """n support points of the keypoint, two in three inside R (neighbours), the rest in the shell 1.05 R .. 1.15 R — never
    between the oracle's support radius and the device's wider one."""
    n_in = (2 * n + 2) // 3
    pts = np.concatenate([around(rng, kp, axis, n_in, 0.2 * R, 0.9 * R), around(rng, kp, axis, n - n_in, 1.05 * R, 1.15 * R)])
    return pts[rng.permutation(n)]


POLES_AT = 3000  # scan index of the first pole point in the placed scenes (48 points: no probe edge is near)


def placed_scan(oracle, p, n, probe_idx, seed, n_poles=4, poles_at=POLES_AT):
    """A scan of n points: filler, n_poles poles (their points from index poles_at on) and one support point at every index of
    probe_idx, dealt to the poles in turn.  Returns (scan, {index: pole})."""
    rng = np.random.default_rng(seed)
    scan = filler(n, seed)
    probe_idx = sorted(int(i) for i in probe_idx)
    assert len(set(probe_idx)) == len(probe_idx) and 0 <= probe_idx[0] and probe_idx[-1] < n
    owner = {}
    for j, axis in enumerate(du.AXES[:n_poles]):
        pl, kp = pole_keypoint(oracle, p, axis)
        at = poles_at + 12 * j
        assert not set(range(at, at + 12)) & set(probe_idx) and at + 12 <= n
        scan[at:at + 12, :3] = pl
        mine = probe_idx[j::n_poles]
        scan[mine, :3] = support_points(rng, kp, axis, len(mine))
        owner.update({i: j for i in mine})
    return scan, owner


EDGES = (4, 64, 128, 256, 1024, 2048, 4096, 65536, 131072, 196608, 262144)
N_LONG = 263000


def edge_probes(n=N_LONG, quad=False):
    """The scan indices either side of every edge — of a quad, a load, a sector word, a wavefront, the gather's tiles (1024 and
    4096 points), the streaming pass's tile (2048), and the 64-tile refill of the near-sector words: 65 536 points for a
    256-thread workgroup alone on its scan, 196 608 for three counted slices, 262 144 for the wide workgroup and for four staged
    workgroups' chunks (131 072 is where the wide workgroup's lane 32 starts) — and 0 and n - 1.  quad: the whole sector of each.
    (The refills of sixteen slices or sixteen staged workgroups need more than a million points: left out.)"""
    idx = {0, n - 1}
    for e in EDGES:
        idx |= {e - 1, e}
    if quad:
        idx = {4 * (i // 4) + j for i in idx for j in range(4) if 4 * (i // 4) + j < n}
    return sorted(idx)


def _scene(oracle, p, scan, extra=None):
    ora = oracle.run(p, scan)
    d = {"p": p, "scan": scan, "ora": ora, "ref": Reference(p, scan, ora["keypoints"])}
    d.update(extra or {})
    return d


@functools.lru_cache(maxsize=None)
def built(name):
    """A named scene, built once a process; nobody writes into it.  {"p", "scan", "ora", "ref", ...}"""
    from oracle import oracle_py
    oracle_py.load()
    p = du.params()
    if name in ("edges", "edges_quad"):
        probes = edge_probes(quad=name == "edges_quad")
        scan, owner = placed_scan(oracle_py, p, N_LONG, probes, seed=41)
        return _scene(oracle_py, p, scan, {"probes": probes, "owner": owner})
    if name in ("short1", "short3"):  # n = 4 k + 1, 4 k + 3: the last point, alone in a partial sector, is a probe
        n = 4 * 300 + 1 if name == "short1" else 4 * 1000 + 3
        probes = [0, 5, 9, n - 1]
        scan, owner = placed_scan(oracle_py, p, n, probes, seed=42, poles_at=400)
        return _scene(oracle_py, p, scan, {"probes": probes, "owner": owner})
    if name == "burst":  # 1024 consecutive points from index 512 on, all in the +x pole's support set
        n, first, m = 6000, 512, 1024
        scan, owner = placed_scan(oracle_py, p, n, range(first, first + m), seed=43, n_poles=1)
        return _scene(oracle_py, p, scan, {"probes": list(range(first, first + m)), "owner": owner})
    if name == "all_near":  # every sector near: a sheet between the filter box and the widened box, out of every pole's reach
        n = 20000
        rng = np.random.default_rng(44)
        scan = np.zeros((n, 4), F32)
        scan[:, 0] = D + 0.03
        scan[:, 1] = rng.uniform(0.5, 4.5, n) * rng.choice([-1.0, 1.0], n)
        scan[:, 2] = rng.uniform(-0.9, 0.9, n)
        for j, axis in enumerate(du.AXES):
            scan[POLES_AT + 12 * j:POLES_AT + 12 * j + 12, :3] = du.pole(p, axis)
            scan[POLES_AT + 12 * j:POLES_AT + 12 * j + 12, 3] = 0
        rng2 = np.random.default_rng(45)
        for j, axis in enumerate(du.AXES):
            _, kp = pole_keypoint(oracle_py, p, axis)
            at = 9000 + 100 * j
            scan[at:at + 20, :3] = support_points(rng2, kp, axis, 20)
        return _scene(oracle_py, p, scan)
    if name == "no_keypoints":
        return _scene(oracle_py, p, filler(5000, 7))
    if name == "one_keypoint":
        scan, owner = placed_scan(oracle_py, p, 3000, [0, 1, 1023, 1024, 2999] + list(range(2000, 2030)), seed=46, n_poles=1, poles_at=500)
        return _scene(oracle_py, p, scan)
    if name == "equal_x":  # two keypoints of equal x (the +y and -y poles): a keypoint grid of one column
        rng = np.random.default_rng(47)
        scan = filler(3000, 47)
        for j, axis in enumerate(du.AXES[2:]):
            pl, kp = pole_keypoint(oracle_py, p, axis)
            scan[500 + 12 * j:512 + 12 * j, :3] = pl
            scan[1000 + 40 * j:1040 + 40 * j, :3] = support_points(rng, kp, axis, 40)
        return _scene(oracle_py, p, scan)
    if name == "gate_support":  # three points at the support radius: d2 the float below r2_support, equal to it, above it
        scan, owner = placed_scan(oracle_py, p, 3000, list(range(1000, 1040)), seed=48, poles_at=500)
        _, kp = pole_keypoint(oracle_py, p, du.AXES[0])
        gates = gate_points(kp.astype(F32), du.AXES[0], constants()[0])
        at = [2001, 2006, 2011]  # (each alone in its sector)
        scan[at, :3] = gates
        return _scene(oracle_py, p, scan, {"gate_at": at})
    if name in ("gate_search_eq", "gate_search_below"):  # keypoint 0's ONLY candidate: d2 equal to r2_search / the float below
        scan, owner = placed_scan(oracle_py, p, 3000, list(range(1000, 1040)), seed=49, poles_at=500)
        mine = [i for i, j in owner.items() if j == 0]
        scan[mine] = filler(len(mine), 3)
        _, kp = pole_keypoint(oracle_py, p, du.AXES[0])
        scan[2001, :3] = gate_points(kp.astype(F32), du.AXES[0], constants()[1])[1 if name == "gate_search_eq" else 0]
        return _scene(oracle_py, p, scan, {"gate_at": [2001]})
    if name == "faces":  # points one float outside, on, and one float inside every face of the widened box
        rng = np.random.default_rng(50)
        scan, owner = placed_scan(oracle_py, p, 3000, list(range(1000, 1040)), seed=50, poles_at=500)
        for j, axis in enumerate(du.AXES):  # support points beyond the filter's faces, out to just inside the support radius
            _, kp = pole_keypoint(oracle_py, p, axis)
            scan[1100 + 4 * j:1104 + 4 * j, :3] = around(rng, kp, axis, 4, 0.985 * support_radius(), 0.995 * support_radius())
        m = constants()[2]
        lim = [(F32(p.x_min) - m, F32(p.x_max) + m), (F32(p.y_min) - m, F32(p.y_max) + m), (F32(p.z_min) - m, F32(p.z_max) + m)]
        at, expect = 2001, {}
        for a in range(3):
            for side in range(2):
                b = lim[a][side]
                away = F32(-np.inf) if side == 0 else F32(np.inf)
                for v, is_near in ((np.nextafter(b, away), False), (b, True), (np.nextafter(b, -away), True)):
                    pt = np.array([2.0, 2.0, 0.5], F32)
                    pt[a] = v
                    scan[at, :3] = pt
                    expect[at // 4] = is_near
                    at += 4
        return _scene(oracle_py, p, scan, {"expect_near": expect})
    if name in ("many", "many_thin"):  # tests/test_gpu_gather_passes.py's scenes: more than 2048 keypoints in 28 800 points
        from tests.test_gpu_gather_passes import many_small_clusters
        if name == "many":
            return _scene(oracle_py, capi.params("launch", number_detection_channels=1, cluster_tolerance=0.65), many_small_clusters())
        return _scene(oracle_py, capi.params("launch", number_detection_channels=1, cluster_tolerance=0.65, descriptor_radius=0.05),
                      many_small_clusters(two_returns_from=-40.0))
    if name == "crowded":  # many keypoints a cell, thousands of points in several support sets, below the LDS tables' 2048 keypoints
        from tests.test_gpu_gather_passes import many_small_clusters
        s = many_small_clusters()
        s = s[np.abs(np.degrees(np.arctan2(s[:, 1], s[:, 0]))) < 30.0]
        return _scene(oracle_py, capi.params("launch", number_detection_channels=1, cluster_tolerance=0.65), s)
    if name == "shared":  # desc_rows_util's three overlapping spheres at R = 0.5 m: 5100 consecutive points, every one a hit
        p2, scan, ora = du.built_shared(0)
        return {"p": p2, "scan": scan, "ora": ora, "ref": Reference(p2, scan, ora["keypoints"])}
    if name == "corner":  # a narrow pole 0.5 mm inside the x and the y face at once
        rng = np.random.default_rng(52)
        spread = (-0.0015, -0.0005, 0.0005, 0.0015)
        pl, kp = pole_keypoint(oracle_py, p, du.AXES[0], side=D, spread=spread)
        scan = filler(3000, 52)
        scan[500:512, :3] = pl
        d = np.array([1.0, 1.0]) / np.sqrt(2.0)  # (beyond both faces)
        scan[1000:1040, :3] = support_points(rng, kp, d, 40)
        scan[1100:1104, :3] = around(rng, kp, d, 4, 0.985 * support_radius(), 0.995 * support_radius())
        return _scene(oracle_py, p, scan)
    if name == "zface":  # one ring's cluster as a keypoint (one detection channel) under a z window that ends 1 mm above it
        rng = np.random.default_rng(53)
        pl = du.pole(p, du.AXES[0])[8:12]  # ring 9's four points
        pz = capi.params("launch", cloud_leveling=0, x_min=-(D + 0.002), x_max=D + 0.002, y_min=-(D + 0.002), y_max=D + 0.002,
                         z_min=-1.0, z_max=float(pl[:, 2].max()) + 0.001, cluster_tolerance=0.25, cluster_min_count=3, cluster_max_count=50,
                         cluster_radius_threshold=0.4, number_detection_channels=1, descriptor_radius=R)
        s4 = np.zeros((4, 4), F32)
        s4[:, :3] = pl
        kp = oracle_py.run(pz, s4)["keypoints"]
        assert len(kp) == 1
        kp = kp[0, :3].astype(np.float64)
        c, th = rng.uniform(0.5, 1.0, 44), rng.uniform(0.0, 2 * np.pi, 44)  # above the face: at least half of the distance upwards
        sn = np.sqrt(1.0 - c * c)
        rr = np.concatenate([rng.uniform(0.2 * R, 0.9 * R, 30), rng.uniform(1.05 * R, 1.15 * R, 10), rng.uniform(0.985, 0.995, 4) * support_radius()])
        scan = filler(3000, 53)
        scan[500:504, :3] = pl
        scan[1000:1044, :3] = (kp + np.stack([sn * np.cos(th), sn * np.sin(th), c], axis=1) * rr[:, None]).astype(F32)
        return _scene(oracle_py, pz, scan)
    if name == "spread":
        return spread_scene(oracle_py, 57)  # (the seed: rings cross cell borders in all four directions, tests/test_gather_scenes.py)
    raise KeyError(name)


def gate_points(kp, axis, r2):
    """Three points whose reference d2 from kp (float32 [3]) is the float just below r2, r2 itself, and the float just above:
    beyond kp along the axis by a little less than sqrt(r2), and z stepped float by float until d2 lands on each target."""
    a = np.array(axis)
    horiz = np.array([kp[0], kp[1]], F32) + (a * np.sqrt(float(r2) - 1e-6)).astype(F32)
    z0 = F32(kp[2] + F32(0.0004))
    z = (np.array([z0], F32).view(np.uint32)[0] + np.arange(400000, dtype=np.uint32)).view(F32)
    pts = np.zeros((len(z), 3), F32)
    pts[:, 0], pts[:, 1], pts[:, 2] = horiz[0], horiz[1], z
    d2 = dist2(kp, pts)
    out = []
    for target in (np.nextafter(F32(r2), F32(0)), F32(r2), np.nextafter(F32(r2), F32(1))):
        hit = np.flatnonzero(d2 == target)
        assert len(hit), f"no z reaches d2 = {target!r}"
        out.append(pts[hit[0]])
    return np.array(out, F32)


def spread_params():
    return capi.params("launch", cloud_leveling=0, x_min=0.5, x_max=75.0, y_min=-30.0, y_max=30.0, z_min=-1.6, z_max=4.5,
                       cluster_tolerance=0.25, cluster_min_count=3, cluster_max_count=50, cluster_radius_threshold=0.4,
                       number_detection_channels=3, descriptor_radius=R)


def spread_scene(oracle, seed, nx=8, ny=5):
    """nx * ny poles on a jittered lattice over the whole 75 m x 60 m box — the gather's cells widen to the grid's limit, 31 x 31
    cells of 2.1 m x 1.7 m (the width is the span / 31 and a little) —, each keypoint with a ring of 24 points at 0.95 support radii in all horizontal directions: wherever the cell
    borders fall, some rings cross them.  (The ring lies inside the filter box: the detector sees it, as part of the pole.)"""
    p = spread_params()
    rng = np.random.default_rng(seed)
    parts = []
    for ix in range(nx):
        for iy in range(ny):
            c = np.array([6.0 + ix * 9.2, -24.0 + iy * 12.0]) + rng.uniform(-2.0, 2.0, 2)
            a = c / np.hypot(*c)
            t = np.array([-a[1], a[0]])
            pl = []
            for ring in (7, 8, 9):
                el = np.deg2rad(p.el0_deg + ring * p.el_step_deg)
                for s in (-0.3, -0.1, 0.1, 0.3):
                    xy = c + s * t
                    pl.append([xy[0], xy[1], np.hypot(*xy) * np.tan(el)])
            pl = np.array(pl, F32)
            s4 = np.zeros((len(pl), 4), F32)
            s4[:, :3] = pl
            kp = oracle.run(p, s4)["keypoints"]
            assert len(kp) == 1
            th = np.arange(24) * (2 * np.pi / 24) + rng.uniform(0, 1)
            ring_pts = kp[0, :3].astype(np.float64) + 0.95 * support_radius() * np.stack([np.cos(th), np.sin(th), np.zeros(24)], axis=1)
            parts += [pl, ring_pts.astype(F32)]
            if (ix + iy) % 2 == 0:  # every other keypoint has neighbours (six points at 0.6 R): the x-axis ordinals skip the rest
                th = np.arange(6) * (2 * np.pi / 6) + rng.uniform(0, 1)
                parts.append((kp[0, :3].astype(np.float64) + 0.6 * R * np.stack([np.cos(th), np.sin(th), np.zeros(6)], axis=1)).astype(F32))
    xyz = np.concatenate(parts)
    scan = filler(len(xyz) + 600, seed)
    scan[300:300 + len(xyz), :3] = xyz
    return _scene(oracle, p, scan)


def cell_steps(ref):
    """How the support points of a scene lie in k_gather's keypoint grid (gather_tables' arithmetic, float32): the set of
    (cell_x(point) - cell_x(keypoint), cell_y(point) - cell_y(keypoint)) over all support points, and (ncx, ncy, wx, wy).
    Only the CPU check of the scenes uses this (that the rings do cross cell borders); the reference knows nothing of cells."""
    m, G = ref.box_margin, 32
    kp = ref.kp
    bx0, bx1, by0, by1 = kp[:, 0].min() - m, kp[:, 0].max() + m, kp[:, 1].min() - m, kp[:, 1].max() + m
    wx = max(m, (bx1 - bx0) / F32(G - 1) * F32(1.0001) + F32(1e-6))
    wy = max(m, (by1 - by0) / F32(G - 1) * F32(1.0001) + F32(1e-6))
    iwx, iwy = F32(1.0) / wx, F32(1.0) / wy
    ncx, ncy = min(int((bx1 - bx0) * iwx) + 1, G), min(int((by1 - by0) * iwy) + 1, G)

    def cx(x):
        return np.clip(np.floor((x - bx0) * iwx).astype(int), 0, ncx - 1)

    def cy(y):
        return np.clip(np.floor((y - by0) * iwy).astype(int), 0, ncy - 1)
    steps = set()
    per_cell = np.bincount(cy(kp[:, 1]) * ncx + cx(kp[:, 0]))
    ref.max_kp_in_cell = int(per_cell.max())  # (keypoints whose OWN cell it is; a cell's list also holds its eight neighbours')
    for k, idx in enumerate(ref.sets):
        pts = ref.rot[idx]
        steps |= set(zip((cx(pts[:, 0]) - cx(kp[k:k + 1, 0])).tolist(), (cy(pts[:, 1]) - cy(kp[k:k + 1, 1])).tolist()))
    return steps, (ncx, ncy, float(wx), float(wy))
