"""The hand-built scenes of tests/test_gpu_desc_list_dense_rows.py (and of test_gpu_desc_csr.py's dense rows), checked on the
CPU: what makes the GPU comparison ABLE to fail.  A scene whose rows had other counts than the case names would test another
tier than the one named; a scene with a point between the oracle's support radius and the device's wider one would give the
device another support count (and tier) than the oracle's; a row whose bins hold one or two terms each cannot tell a reordered
fp32 sum from the right one."""
import numpy as np
import pytest

from tests import desc_rows_util as rows


def _no_point_between_the_radii(scan, ora, radius, tag):
    lo, hi = rows.support_counts(scan, ora, radius)
    assert lo == hi, f"{tag}: support counts {lo} by the oracle's radius, {hi} by the device's"


@pytest.mark.parametrize("name", sorted(rows.NAMED))
def test_scene_counts_and_order_sensitivity(oracle, name):
    p, scenes, cases = rows.built(name)  # (built() asserts the oracle's neighbour and support counts: check_counts)
    assert len(scenes) == (len(cases) + 3) // 4
    for b, (scan, ora) in enumerate(scenes):
        mine = cases[4 * b:4 * b + 4]
        tag = f"{name} scan {b} {mine}"
        assert sorted(int(n) for n in ora["kp_neighbors"]) == sorted(n for n, _, _ in mine), tag
        lo, _ = rows.support_counts(scan, ora)
        assert sorted(lo) == sorted(s for _, s, _ in mine), tag
        _no_point_between_the_radii(scan, ora, rows.R, tag)
        sens = [rows.order_sensitive(p, scan, ora, k) for k in range(ora["n_keypoints"])]
        print(f"{tag}: (bins that change under a reversed sum, most terms of a bin) per row "
              f"{[(int(ora['kp_neighbors'][k]), s) for k, s in enumerate(sens)]}")
        if max(n for n, _, _ in mine) >= 64:
            assert max(s for s, _ in sens) >= 8, tag
        for n, sup, how in mine:
            if how == "one_bin":
                k = int(np.flatnonzero(ora["kp_neighbors"] == n)[0])
                assert sens[k][1] >= 64, f"{tag}: the one_bin row's fullest bin has {sens[k][1]} terms"
            if how == "dup":  # (really duplicates: fewer distinct points than neighbours)
                k = int(np.flatnonzero(ora["kp_neighbors"] == n)[0])
                d2 = rows.sqdist(scan[:, :3], ora["keypoints"][k, :3])
                inside = scan[d2 < np.float32(rows.R) * np.float32(rows.R), :3]
                assert len(np.unique(inside, axis=0)) <= n - n // 4, tag


def test_shared_density_scenes(oracle):
    """Three rows of more than 1024 support points, at least 200 points neighbours of two of them; the second scene has the same
    number of points at other coordinates."""
    p, scan, ora = rows.built_shared(0)
    _, other, ora_other = rows.built_shared(1)
    assert len(other) == len(scan) and not np.array_equal(other, scan)
    for s, o, tag in ((scan, ora, "shared"), (other, ora_other, "other")):
        assert o["n_keypoints"] == 3, tag
        lo, hi = rows.support_counts(s, o, rows.R_SHARED)
        assert min(lo) > rows.LIST_CAP and lo == hi, f"{tag}: support counts {lo} / {hi}"
        r2 = np.float32(rows.R_SHARED * rows.R_SHARED)
        member = np.stack([rows.sqdist(s[:, :3], kp[:3]) < r2 for kp in o["keypoints"]])
        assert [int(m.sum()) for m in member] == [int(n) for n in o["kp_neighbors"]], tag
        assert int((member.sum(axis=0) >= 2).sum()) >= 200, tag
        assert max(rows.order_sensitive(p, s, o, k)[0] for k in range(3)) >= 8, tag
