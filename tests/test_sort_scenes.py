"""CPU checks of the prescribed-size scenes (tests/sort_scenes_util.py): what makes tests/test_gpu_sort_scenes.py able to fail.
The oracle finds, ring by ring and merge by merge, exactly the prescribed sizes in discovery order and loses nothing to a gate;
the table every scene states for itself is the oracle's output; outside the all-equal scenes the order differs from a stable
descending sort and from its mirror image, so a stable sort in the replay's place would fail; the plain-Python statement of the
sort equals the oracle's std::sort with the depth limit and differs without it on every adversary."""
import functools

import numpy as np

from tests import sort_scenes_util as ss


def _scenes():
    return ss.ring_scenes("ring16") + ss.ring_scenes("ring32") + ss.merge_scenes()


@functools.lru_cache(maxsize=None)
def _oracle_of(key):
    from oracle import oracle_py
    sc = {(s["name"], s["group"]): s for s in _scenes()}[key]
    return oracle_py.run(ss.params(sc["group"]), sc["scan"], want_labels=True)


def test_the_oracle_finds_the_prescribed_sizes_in_discovery_order(oracle):
    for sc in _scenes():
        o = _oracle_of((sc["name"], sc["group"]))
        tag = f"{sc['name']} ({sc['group']})"
        assert len(o["filtered"]) == len(sc["scan"]), tag
        if sc["kind"] == "ring":
            for ring in range(ss.params(sc["group"]).n_rings):
                lab = o["ring_labels"][ring]
                roots, counts = np.unique(lab[lab >= 0], return_counts=True)  # (ascending smallest member: discovery order)
                want = sc["rings"].get(ring, np.zeros(0, np.uint32))
                assert counts.tolist() == want.tolist(), f"{tag}: ring {ring} has clusters of {counts.tolist()[:12]} .., prescribed {want.tolist()[:12]} .."
            assert len(o["candidates"]) == sum(len(s) for s in sc["rings"].values()), f"{tag}: a cluster is lost to a gate"
            assert o["n_keypoints"] == 0, f"{tag}: candidates of different clusters merge"
        else:
            assert len(o["candidates"]) == int(sc["sizes"].sum()) and (o["cand_size"] == 1).all(), tag
            ck = o["cand_keypoint"]
            assert (ck >= 0).all(), f"{tag}: a group is lost to a gate"
            first = [int(np.flatnonzero(ck == k)[0]) for k in range(o["n_keypoints"])]
            found = [int((ck == k).sum()) for k in np.argsort(first)]
            assert found == sc["sizes"].tolist(), f"{tag}: groups of {found[:12]} .., prescribed {sc['sizes'].tolist()[:12]} .."
            for k in range(o["n_keypoints"]):  # a group's candidates are consecutive: the chain, in chain order
                at = np.flatnonzero(ck == k)
                assert at[-1] - at[0] + 1 == len(at), tag


def test_every_stated_table_is_the_oracles_output(oracle):
    n_bits = 0
    for sc in _scenes():
        o = _oracle_of((sc["name"], sc["group"]))
        ss.check(o, sc, tag="oracle: ")
        ex = sc["expect"]
        assert len(ex["cand_bits"]) == len(o["candidates"]) and len(ex.get("kp_bits", {})) == o["n_keypoints"]
        n_bits += len(ex["cand_bits"]) + len(ex.get("kp_bits", {}))
    assert n_bits > 10000


def test_a_stable_sort_in_the_replays_place_would_fail(oracle):
    """Every sequence but the all-equal ones and those of at most 16 entries (which std::sort only insertion-sorts: stable) comes
    out in an order that is neither the stable descending one nor its mirror image."""
    n = 0
    for sc in _scenes():
        for s in ss.sequences_of(sc):
            order = ss.sort_order(s)
            if len(s) <= 16:
                assert np.array_equal(order, ss.stable_desc(s))
                continue
            assert not np.array_equal(order, ss.stable_desc(s)), f"{sc['name']}: the stable order"
            assert not np.array_equal(order, ss.stable_desc_reversed_ties(s)), f"{sc['name']}: the mirrored stable order"
            n += 1
    assert n >= 40
    assert np.array_equal(ss.stable_desc([2, 1, 2, 1]), [0, 2, 1, 3]) and np.array_equal(ss.stable_desc_reversed_ties([2, 1, 2, 1]), [2, 0, 3, 1])


def test_the_plain_statement_of_the_sort(oracle):
    """replay() with libstdc++'s depth limit is the oracle's std::sort on every sequence the scenes and the hook test use; without
    the limit it differs on every adversary: the heap fallback is reached and decides the order."""
    seqs = [s for sc in _scenes() for s in ss.sequences_of(sc)]
    for n in (16, 17, 64, 65, 128, 129, 192, 193, 255, 256, 257, 300, 1000):
        seqs += [ss.seq(k, n) for k in ("r1", "r2", "r3", "r5", "r16", "r50", "r1000", "asc", "desc", "pipe", "mod13", "ones", "anti")]
    for s in seqs:
        got, _ = ss.replay(s)
        assert np.array_equal(got, ss.sort_order(s)), (len(s), s[:8])
    adversaries = [ss.adversary(n) for n in ss.ADVERSARY_DIV]
    adversaries += [ss.adversary(n, 2) for n in (64, 65, 128, 129, 192, 193, 255, 256, 257, 300, 1000)]  # (the hook test's)
    marked = [sc for sc in _scenes() if sc["adversary"]]
    assert len(marked) >= 13
    for sc in marked:  # every scene that claims an adversary holds one of them
        assert any(np.array_equal(s, a) for s in ss.sequences_of(sc) for a in adversaries), sc["name"]
    for s in adversaries:
        with_limit, heaps = ss.replay(s)
        without, none = ss.replay(s, depth_limit=False)
        assert heaps > 0 and none == 0, len(s)
        assert not np.array_equal(with_limit, without), f"antiqsort({len(s)}): the depth limit changes nothing"


def test_the_scenes_fit_what_they_are_meant_for():
    for sc in ss.ring_scenes("ring16"):
        runs = sum(len(s) for s in sc["rings"].values())
        assert sc["front"] == (runs <= 512 and len(sc["scan"]) <= 3328), sc["name"]
        assert max(int(s.max()) for s in sc["rings"].values()) <= 50 or sc["adversary"], sc["name"]
    assert [sc["name"] for sc in ss.ring_scenes("ring16") if not sc["front"]] == ["rings 16 .. 193", "rings 257 1000"]
    for sc in ss.merge_scenes():
        assert sc["small"] == (len(sc["scan"]) <= 512) and (int(sc["sizes"].max()) <= 50 or sc["adversary"]), sc["name"]
