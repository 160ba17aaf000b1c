"""Scenes that put PRESCRIBED size sequences into real rings and real merges (tests/test_gpu_sort_scenes.py; that they can
fail: tests/test_sort_scenes.py).

Keypoint ordinals depend on how libstdc++'s unstable std::sort(rbegin, rend, bySize) leaves clusters of equal size
(csrc/fx_sort_replay.h).  Every ring and merge body holds an instance of the replay; the whole-pipeline scenes elsewhere reach
them with all-equal sizes only.  Here a ring's clusters — and a scan's merge groups — have, in discovery order, exactly the
sizes of a tie-heavy or adversarial sequence, and the scene states its own table: the clusters (groups) in the order
oracle.sort_by_size_desc gives — the oracle's literal std::sort call on the bare sizes, independent of oracle.run — by size
and by the centroid's bits, so a tie resolved wrongly shows although the sizes agree.

Geometry.  Everything lies on arcs of constant horizontal radius ("shells", 1 m apart, azimuth -60 .. 60 degrees) of a ring's
cone; shells of ring r start at 10 + 0.25 (r % 4) m, so no two rings closer than four apart share a shell.
  ring_of_sizes   a cluster's returns are 1 mm apart along the shell and consecutive in the scan (one run), clusters 0.45 m
                  apart; cluster_tolerance 0.1: every cluster is its own, passes the diameter gate (0.4 m) by far, and no two
                  candidates are within the merge radius (0.2 m) — no keypoints.
  merge_of_sizes  one-return candidates (cluster_tolerance 0.02) 0.05 m apart in a chain per group, groups 0.5 m apart;
                  number_detection_channels 1: every group is a keypoint.  The candidates of a ring are single returns — all
                  of one size —, so the ring's own order is sort_by_size_desc(ones): the returns are dealt to the scan so that
                  the candidate order comes out group by group, chain by chain.

The partition phase is also stated once here in plain Python (replay), with the depth limit as a parameter: with libstdc++'s
2 floor(log2 n) it equals the oracle on every sequence used; without it, it differs on every adversary — the heap fallback is
reached and matters."""
import functools

import numpy as np

from feature_extraction_amd import capi
from tests import front_edges_util as fe
from tests.test_gpu_ring_run_tier import ring_points

F32 = np.float32
AZ_LIM = np.radians(60.0)

PARAMS = {
    "ring16": dict(cluster_tolerance=0.1, z_min=-20.0, z_max=20.0),
    "ring32": dict(cluster_tolerance=0.1, z_min=-20.0, z_max=20.0, n_rings=32, el0_deg=-15.0, el_step_deg=1.0, secondary_max=32),
    "merge": dict(cluster_tolerance=0.02, z_min=-20.0, z_max=20.0, number_detection_channels=1, secondary_max=1000),
}
LIMITS = dict(max_ring_points=4096, max_ring_candidates=4096, max_candidates=4096, max_keypoints=1024, max_kpc_points=8192)
MAX_POINTS = 8192


def params(group):
    return capi.params("launch", **PARAMS[group])


def limits(batch, **over):
    return capi.limits(batch, MAX_POINTS, **dict(LIMITS, max_total_keypoints=batch * LIMITS["max_keypoints"], **over))


def _ring16(group, ring):
    """The ring as tests/test_gpu_ring_run_tier.ring_points counts it (elevation -15 + 2 ring): the 32-ring groups' step is 1."""
    return ring / 2.0 if PARAMS[group].get("n_rings", 16) == 32 else ring


# ---------------------------------------------------------------- the sort, stated once
def _sift(v, first, hole, length, value):
    """libstdc++'s __adjust_heap: the hole walks down to a leaf along the larger child (the right one on a tie), then the value
    climbs back up past strictly smaller parents."""
    top = hole
    child = hole
    while child < (length - 1) // 2:
        child = 2 * (child + 1)
        if v[first + child][0] < v[first + child - 1][0]:
            child -= 1
        v[first + hole] = v[first + child]
        hole = child
    if length % 2 == 0 and child == (length - 2) // 2:
        child = 2 * (child + 1)
        v[first + hole] = v[first + child - 1]
        hole = child - 1
    while hole > top and v[first + (hole - 1) // 2][0] < value[0]:
        v[first + hole] = v[first + (hole - 1) // 2]
        hole = (hole - 1) // 2
    v[first + hole] = value


def _heap_sort(v, first, last):
    length = last - first
    for parent in range((length - 2) // 2, -1, -1):
        _sift(v, first, parent, length, v[first + parent])
    while last - first > 1:
        last -= 1
        value = v[last]
        v[last] = v[first]
        _sift(v, first, 0, last - first, value)


def _partition(v, first, last):
    """Median of v[first + 1], v[mid], v[last - 1] to v[first]; then the two walking pointers."""
    a, b, c = first + 1, first + (last - first) // 2, last - 1
    ka, kb, kc = v[a][0], v[b][0], v[c][0]
    if ka < kb:
        m = b if kb < kc else (c if ka < kc else a)
    else:
        m = a if ka < kc else (c if kb < kc else b)
    v[first], v[m] = v[m], v[first]
    pivot = v[first][0]
    lo, hi = first + 1, last
    while True:
        while v[lo][0] < pivot:
            lo += 1
        hi -= 1
        while pivot < v[hi][0]:
            hi -= 1
        if not lo < hi:
            return lo
        v[lo], v[hi] = v[hi], v[lo]
        lo += 1


def replay(sizes, depth_limit=True):
    """std::sort(rbegin, rend, bySize) as libstdc++ runs it: ordinals in the order the clusters come out.  An ascending
    introsort of the reversed sequence: partitions down to ranges of 16, heap sort for a range whose depth budget
    (2 floor(log2 n)) is spent — never, with depth_limit=False —, then insertion sort, which is a stable sort of what is left.
    Returns (ordinals, ranges that were heap sorted)."""
    n = len(sizes)
    v = [(int(s), i) for i, s in enumerate(sizes)][::-1]
    heaps = 0
    pending = [(0, n, 2 * (n.bit_length() - 1) if n else 0)]
    while pending:
        first, last, depth = pending.pop()
        while last - first > 16:
            if depth_limit and depth == 0:
                _heap_sort(v, first, last)
                heaps += 1
                break
            depth -= 1
            cut = _partition(v, first, last)
            pending.append((cut, last, depth))
            last = cut
    v.sort(key=lambda rec: rec[0])  # (stable)
    return np.array([i for _, i in v[::-1]], np.uint32), heaps


def sort_order(sizes):
    from oracle import oracle_py
    return oracle_py.sort_by_size_desc(np.asarray(sizes, np.uint32))


def stable_desc(sizes):
    return np.argsort(-np.asarray(sizes, np.int64), kind="stable").astype(np.uint32)


def stable_desc_reversed_ties(sizes):
    """Descending, equal sizes in REVERSE discovery order (a stable ascending sort read backwards)."""
    return np.argsort(np.asarray(sizes, np.int64), kind="stable")[::-1].astype(np.uint32)


# ---------------------------------------------------------------- sequences
# McIlroy's adversary against the very std::sort call (oracle.antiqsort) drives introsort to its depth limit, but its sizes are
# all different: ANY correct sort gives the one descending order, and the heap fallback could be left out unnoticed.  Dividing
# the sizes (rounding up) makes ties and keeps the adversary's shape: for these (n, divisor) — the cheapest in points of every
# range of cc_order's dispatch, found by search with replay() below — the budget is still spent, and the order the heap sort
# leaves its ties in differs from the one further partitions would (tests/test_sort_scenes.py asserts both).  Below n = 37 no
# divisor does: introsort stops partitioning at 16 entries, before eight levels are spent.
ADVERSARY_DIV = {40: 2, 65: 2, 100: 2, 175: 7, 249: 32, 283: 29}


def adversary(n, div=None):
    from oracle import oracle_py
    div = div or ADVERSARY_DIV.get(n, 2)
    return ((oracle_py.antiqsort(n).astype(np.int64) + div - 1) // div).astype(np.uint32)


def seq(kind, n, seed=0):
    """The size sequences of tests/test_sort_replay.py: "r<hi>" random in 1 .. hi ("u<lo>-<hi>": in lo .. hi), "mod13", "pipe" (organ pipe, capped at 50),
    "asc" / "desc" (capped at 50: long plateaus), "ones", "anti" (adversary(n))."""
    idx = np.arange(n)
    if kind.startswith("r"):
        return np.random.default_rng(1000 * n + seed).integers(1, int(kind[1:]) + 1, n).astype(np.uint32)
    if kind.startswith("u"):  # "u<lo>-<hi>": random in lo .. hi
        lo, hi = (int(v) for v in kind[1:].split("-"))
        return np.random.default_rng(1000 * n + seed).integers(lo, hi + 1, n).astype(np.uint32)
    if kind == "anti":
        return adversary(n)
    return {"mod13": (idx * 7919) % 13 + 1, "pipe": np.minimum(np.minimum(idx, idx[::-1]) + 1, 50), "asc": np.minimum(idx + 1, 50),
            "desc": np.minimum(idx[::-1] + 1, 50), "ones": np.ones(n)}[kind].astype(np.uint32)


# ---------------------------------------------------------------- geometry
class _Arc:
    """Hands out stretches of arc on a ring's shells, in order: shell after shell, each from -60 to 60 degrees."""

    def __init__(self, ring, gap):
        self.h, self.az, self.gap = 10.0 + 0.25 * (ring % 4), -AZ_LIM, gap

    def take(self, length):
        if self.az + length / self.h > AZ_LIM:
            self.h, self.az = self.h + 1.0, -AZ_LIM
        assert self.h <= 55.0, "out of shells inside the filter box"
        at = (self.h, self.az)
        self.az += (length + self.gap) / self.h
        return at


def _arc_points(group, ring, h, az0, count, spacing):
    el = np.radians(-15.0 + 2.0 * _ring16(group, ring))
    az = az0 + spacing / h * np.arange(count)
    return ring_points(_ring16(group, ring), np.degrees(az), np.full(count, h / np.cos(el)))


def ring_of_sizes(ring, sizes, group="ring16"):
    """(points [sum(sizes), 4], [members of cluster k]) of one ring whose clusters, in discovery order — ascending first index
    in ring order —, have exactly the sizes given."""
    arc = _Arc(ring, 0.45)
    clusters = []
    for m in sizes:
        h, az = arc.take(0.001 * (int(m) - 1))
        clusters.append(_arc_points(group, ring, h, az, int(m), 0.001))
    return np.concatenate(clusters), clusters


def merge_of_sizes(sizes, rings=(8,), group="merge"):
    """(points, [members of group g in candidate order]): one-return candidates that the secondary merge groups into keypoints
    of exactly those sizes in discovery order (ascending first candidate; candidates are listed ring by ring).  The groups are
    dealt to the rings in consecutive blocks of about equal candidate counts; the rings must be three or more apart."""
    sizes = [int(m) for m in sizes]
    assert all(b - a >= 3 for a, b in zip(rings, rings[1:]))
    share = -(-sum(sizes) // len(rings))
    blocks, cur = [[]], 0
    for m in sizes:
        if cur + m > share and blocks[-1] and len(blocks) < len(rings):
            blocks.append([])
            cur = 0
        blocks[-1].append(m)
        cur += m
    parts, groups = [], []
    for ring, block in zip(rings, blocks):
        arc = _Arc(ring, 0.5)
        chains = [_arc_points(group, ring, *arc.take(0.05 * (m - 1)), m, 0.05) for m in block]
        want = np.concatenate(chains)  # the ring's candidates in the order wanted
        order = sort_order(np.ones(len(want)))  # candidate s is the ring's return number order[s]
        pts = np.empty_like(want)
        pts[order] = want
        parts.append(pts)
        groups += chains
    return np.concatenate(parts), groups


def candidate_of(members):
    return fe.centroid(np.ascontiguousarray(members[:, :3]))


def keypoint_of(members):
    """A merge group of one-return candidates: the sequential double mean of the candidates in order, the first one's elevation."""
    a = np.ascontiguousarray(members[:, :3])
    n = float(len(a))
    return np.array([F32(fe.seq_sum(a[:, k]) / n) for k in range(3)] + [fe.elevation(*a[0])], F32)


# ---------------------------------------------------------------- scenes
def ring_scene(name, group, rings):
    """rings: {ring: sizes}.  The table: ring by ring (ascending), each ring's clusters in the order sort_by_size_desc gives."""
    parts, cand_size, cand_bits = [], [], {}
    for ring in sorted(rings, reverse=True):  # (the scan lists the rings backwards: the ring split has to sort them out)
        parts.append(ring_of_sizes(ring, rings[ring], group)[0])
    for ring in sorted(rings):
        sizes = np.asarray(rings[ring], np.uint32)
        clusters = ring_of_sizes(ring, sizes, group)[1]
        for k in sort_order(sizes):
            cand_bits[len(cand_size)] = fe.bits4(candidate_of(clusters[k]))
            cand_size.append(int(sizes[k]))
    return fe.scene(name, group, np.concatenate(parts)[:, :3], dict(cand_size=cand_size, kp_size=[], cand_bits=cand_bits),
                    rings={r: np.asarray(s, np.uint32) for r, s in rings.items()}, kind="ring")


def merge_scene(name, sizes, rings=(8,), group="merge"):
    sizes = np.asarray(sizes, np.uint32)
    pts, groups = merge_of_sizes(sizes, rings, group)
    order = sort_order(sizes)
    cands = np.concatenate(groups)
    cand_bits = {i: fe.bits4(candidate_of(cands[i:i + 1])) for i in range(len(cands))}
    kp_bits = {s: fe.bits4(keypoint_of(groups[g])) for s, g in enumerate(order)}
    return fe.scene(name, group, pts[:, :3], dict(cand_size=[1] * len(cands), kp_size=[int(sizes[g]) for g in order], cand_bits=cand_bits, kp_bits=kp_bits),
                    sizes=sizes, kind="merge")


def sequences_of(sc):
    """The prescribed sequences of a scene: a ring scene's per ring, a merge scene's one."""
    return list(sc["rings"].values()) if sc["kind"] == "ring" else [sc["sizes"]]


BORDER_COUNTS = (16, 17, 64, 65, 128, 129, 192, 193)
BORDER_KINDS = ("r3", "r2", "mod13", "r5", "r3", "r2", "r3", "r2")  # tie-heavy, another family at every border


@functools.lru_cache(maxsize=None)
def ring_scenes(group="ring16"):
    """front: the scenes k_front's tables hold (512 runs and clusters a scan, 3328 points); the rest needs the kernels behind it.
    adversary: the scenes whose sequence spends the depth budget."""
    step = 2 if group == "ring32" else 1  # (the same cones under both ring geometries)
    R = lambda r: r * step
    b = dict(zip(BORDER_COUNTS, BORDER_KINDS))
    out = [
        ring_scene("rings 16 17 64 65 128 129", group, {R(4 + i): seq(b[n], n) for i, n in enumerate(BORDER_COUNTS[:6])}),
        ring_scene("rings 17 192 193", group, {R(6): seq("r50", 17), R(7): seq(b[192], 192), R(8): seq(b[193], 193)}),
        ring_scene("rings 256 40 equal", group, {R(8): seq("r3", 256), R(9): seq("ones", 40)}),
        ring_scene("rings 100 300", group, {R(7): seq("mod13", 100), R(8): seq("r5", 300)}),
        ring_scene("rings anti 40 100", group, {R(8): seq("anti", 40), R(9): seq("anti", 100)}),
        ring_scene("rings anti 175", group, {R(8): seq("anti", 175), R(9): seq("r3", 33)}),
        ring_scene("rings anti 65 249", group, {R(8): seq("anti", 249), R(9): seq("anti", 65)}),
        ring_scene("rings anti 283", group, {R(8): seq("anti", 283)}),
        ring_scene("rings 16 .. 193", group, {R(3 + i): seq(k, n, seed=1) for i, (n, k) in enumerate(zip(BORDER_COUNTS, BORDER_KINDS))}),
        ring_scene("rings 257 1000", group, {R(7): seq("r2", 257), R(8): seq("r3", 1000)}),
    ]
    for sc in out:
        counts = [len(s) for s in sc["rings"].values()]
        sc["front"] = sum(counts) <= 512 and len(sc["scan"]) <= 3328
        sc["adversary"] = "anti" in sc["name"]
    return out


@functools.lru_cache(maxsize=None)
def merge_scenes():
    """small: up to 512 candidates (k_front's merge and k_merge_small hold that many)."""
    out = [
        merge_scene("merge 17", seq("r50", 17)),
        merge_scene("merge 64", seq("r5", 64)),
        merge_scene("merge 65", seq("mod13", 65)),
        merge_scene("merge 192", seq("r3", 192)),
        merge_scene("merge 193", seq("r2", 193)),
        merge_scene("merge 256", seq("r2", 256, seed=1)),
        merge_scene("merge 257", seq("r2", 257)),
        merge_scene("merge 40 equal", np.full(40, 3)),
        merge_scene("merge anti 40", seq("anti", 40)),
        # the same counts with more than 512 candidates: past k_merge_small, into the tiers behind it
        merge_scene("merge 17 big", seq("u30-50", 17), rings=(5, 8)),
        merge_scene("merge 64 big", seq("u5-14", 64), rings=(5, 8)),
        merge_scene("merge 65 big", seq("u5-14", 65), rings=(5, 8)),
        merge_scene("merge 192 big", seq("u2-4", 192), rings=(5, 8)),
        merge_scene("merge 193 big", seq("u2-4", 193), rings=(5, 8)),
        merge_scene("merge 256 big", seq("u2-3", 256), rings=(5, 8)),
        merge_scene("merge 257 big", seq("u2-3", 257), rings=(5, 8)),
        merge_scene("merge 600", seq("r3", 600), rings=(2, 5, 8, 11)),
        merge_scene("merge anti 100", seq("anti", 100), rings=(2, 5, 8, 11)),
        merge_scene("merge anti 175", seq("anti", 175), rings=(2, 5, 8, 11)),
        merge_scene("merge anti 249", seq("anti", 249), rings=(5, 8)),
        merge_scene("merge anti 283", seq("anti", 283), rings=(5, 8)),
    ]
    for sc in out:
        sc["small"] = len(sc["scan"]) <= 512
        sc["adversary"] = "anti" in sc["name"]
    return out


def check(got, sc, tag=""):
    fe.check_expect(got, sc, tag=tag)
