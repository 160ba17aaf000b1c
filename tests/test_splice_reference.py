"""capi.splice_reference — the definition of fx_splice_blocks (include/fx.h) in numpy, fed the sources' BLOCKS — against an
independent construction: the selected scans' keypoint rows and dense descriptor rows laid behind each other by hand and written
as the two packs write a batch (tests/splice_util.py: capi.keypoint_block_from_rows, capi.csr_from_dense, capi.csr_layout).  Whole
blocks, byte for byte; what the call leaves undefined holds the fill byte on both sides."""
import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import splice_util as su
from tests import util


def _check(what, a, b, parts, dst_kp, dst_csr):
    kp, csr = capi.splice_reference(a, b, dst_kp, dst_csr)
    want_kp, want_csr = su.expected(parts, dst_kp, dst_csr)
    su.assert_blocks(kp, None if csr is None else su.csr_image(csr, *dst_csr), want_kp, want_csr, what)
    return kp, csr


def test_hand_built_cases():
    cases = su.cases(np.random.default_rng(71))
    assert len(cases) > 30
    for c in cases:
        _check(*c)
    by = {c[0]: _check(*c) for c in cases}
    # the cases are what their names say
    kp, csr = by["all of both"]
    blk = capi.keypoint_block_parse(kp, 6, 12)
    assert blk["kp_offset"].tolist() == [0, 2, 2, 5, 6, 10] and blk["flags"].tolist() == [8, 16, 0, 32, 8] and blk["flags_or"] == 56
    assert csr["header"].tolist() == [10, 26, 26, 10]
    assert by["the sentinel on an empty block"][1]["header"].tolist() == [5, 12, 12, 5] and by["two empty blocks"][1]["header"].tolist() == [0, 0, 0, 0]
    assert by["dst_max_total 9 of 10"][0].view(np.uint32)[:4].tolist() == [5, 9, 56 | su.KP_OVERFLOW, 9]
    assert by["dst_max_scans 3 below 5"][0].view(np.uint32)[:4].tolist() == [3, 5, 24 | su.KP_OVERFLOW, 12]
    assert by["capacity 25 of 26 (14 in a)"][1]["header"].tolist() == [10, 23, 26, 9]
    assert by["capacity 13 of 26 (14 in a)"][1]["header"].tolist() == [10, 10, 26, 4]
    assert by["capacity 14 of 26 (14 in a)"][1]["header"].tolist() == [10, 14, 26, 5]
    assert by["dst_max_rows 4 of 10 (5 in a)"][1]["header"].tolist() == [10, 10, 26, 4]
    assert by["a's CSR cut by its own capacity"][1]["header"].tolist() == [10, 10, 10 + 12, 4]
    assert by["b's CSR cut by its own capacity"][1]["header"].tolist() == [3 + 5, 11 + 9, 11 + 9, 3 + 4]
    assert by["both CSRs cut, a missing row in each selection"][1]["header"].tolist() == [3 + 4, 7, 7 + 8, 2]


@pytest.mark.parametrize("rows", [255, 256, 257])
def test_many_rows_and_many_scans(rows):
    """One scan of `rows` rows behind a scan of 3, and `rows` scans of 0 .. 2 rows: the sizes at the device code's tile edges."""
    rng = np.random.default_rng(72 + rows)
    A, B = su.Source(rng, (2, 3)), su.Source(rng, (1, rows))
    parts = [(A, 1, 2), (B, 0, 2)]
    _check(f"{rows} rows", A.src(su.LAST, 1), B.src(0, su.ALL), parts, *su.room(parts))
    C = su.Source(rng, rng.integers(0, 3, rows))
    parts = [(A, 1, 2), (C, 0, rows)]
    for s in (rows + 1, rows, 5, 4, 3, 1):
        _check(f"{rows} scans into {s}", A.src(su.LAST, 1), C.src(0, su.ALL), parts, (s, su.room(parts)[0][1]), su.room(parts)[1])


def test_kp_offset_for_the_pairs():
    off_a, off_b = [0, 2, 2, 5], [0, 1, 5]
    assert capi.splice_kp_offset(off_a, off_b).tolist() == [0, 3, 4, 8]
    assert capi.splice_kp_offset(off_a, off_b, a=(0, su.ALL), b=(1, 1)).tolist() == [0, 2, 2, 5, 9]
    assert capi.splice_kp_offset([0], off_b).tolist() == [0, 1, 5]
    assert capi.pairs_consecutive(capi.splice_kp_offset(off_a, off_b)) == [(3, 1, 0, 3), (4, 4, 3, 1)]


def test_the_premise_scans_are_not_empty(oracle):
    """tests/test_gpu_splice.py compares a splice of processed scans with one batch of them: the three scans it uses have keypoints
    and descriptor rows with non-zero words, so that comparison is not one of empty blocks."""
    p = capi.params("launch")
    for seed in su.PREMISE_SEEDS:
        r = oracle.run(p, util.vlp16_scan(seed), roll=0.02, pitch=-0.015)
        assert r["n_keypoints"] >= 2 and len(r["descriptors"]) == r["n_keypoints"], seed
        assert ((np.ascontiguousarray(r["descriptors"], dtype=np.float32).view(np.uint32) != 0).sum(axis=1) > 0).any(), seed
