"""Descriptor rows as compressed rows (CSR, include/fx.h fx_descriptor_csr_bytes): the C-ABI declares and exports the entry
points, the block's size follows the documented layout, and the numpy statement of the storage rule (capi.csr_from_dense /
dense_from_csr, the GPU tests' reference) gives every fixture's rows back bit for bit.  No GPU needed."""
import ctypes as C
import glob
import os
import re

import numpy as np

from feature_extraction_amd import capi
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSR_API = ("fx_descriptor_csr_bytes", "fx_pack_descriptors_csr", "fx_get_descriptors_csr", "fx_set_descriptor_csr_capacity")


def test_csr_entry_points_declared_exported_and_listed(fxlib):
    src = open(os.path.join(ROOT, "include", "fx.h")).read()
    for name in CSR_API:
        assert re.search(rf"\b{name}\s*\(", src), name
        assert hasattr(fxlib, name), name
        assert name in capi.EXPORTS, name
    assert re.search(r"#define FX_OUT_DESC_CSR 0x10u", src) and capi.FX_OUT_DESC_CSR == 0x10
    assert "fx_descriptor_csr_view" in src
    assert C.sizeof(capi.FxDescriptorCsrView) == 8 + 6 * 8


def test_csr_bytes_follow_the_layout(fxlib):
    for max_rows in (0, 1, 2, 3, 4, 5, 7, 64, 1000, 65536):
        for cap in (0, 1, 3, 4, 5, 128, 4097, 65536 * 128):
            rp, col, val, end = capi.csr_layout(max_rows, cap)
            assert (rp, col % 16, val % 16, end % 16) == (16, 0, 0, 0)
            assert col - rp >= 4 * (max_rows + 1) > col - rp - 16
            assert val - col >= 4 * cap > val - col - 16 and end - val == val - col
            assert fxlib.fx_descriptor_csr_bytes(max_rows, cap) == end, (max_rows, cap)


def _roundtrip(rows, what):
    rp, col, val = capi.csr_from_dense(rows)
    bits = util.bits(rows)
    assert rp[0] == 0 and (np.diff(rp.astype(np.int64)) >= 0).all()
    assert rp[-1] == len(col) == len(val) == int((bits != 0).sum()), what
    for r in range(len(rows)):
        c = col[rp[r]:rp[r + 1]].astype(np.int64)
        assert (np.diff(c) > 0).all() and (c < capi.FX_DESC_FLOATS).all()
    assert (util.bits(val) != 0).all()
    back = capi.dense_from_csr(rp, col, val)
    assert back.shape == rows.shape and (util.bits(back) == bits).all(), what


def test_golden_descriptors_roundtrip_bit_for_bit():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    assert len(files) >= 5
    for f in files:
        d = np.load(f)["descriptors"]
        _roundtrip(d, os.path.basename(f))
        nnz = (util.bits(d) != 0).sum(axis=1)
        assert nnz.max() < capi.FX_DESC_FLOATS and (d[:, capi.FX_DESC_BINS:] == 0).all()


def test_synthetic_rows_with_nan_negative_zero_and_rf_roundtrip():
    rows = np.zeros((5, capi.FX_DESC_FLOATS), np.float32)
    rows[0, [0, 7, 1979]] = [1.5, -0.0, np.nan]
    rows[0, capi.FX_DESC_BINS + 3] = 2.0           # a non-zero rf word
    rows[1, :capi.FX_DESC_BINS] = np.nan             # an overflow row: every bin NaN
    rows[3, capi.FX_DESC_BINS:] = -0.0                # rf words that are -0.0 only
    rows[4] = np.arange(capi.FX_DESC_FLOATS, dtype=np.float32) + 1.0  # a full row
    rows[4, 100] = np.float32(np.uint32(0x7fc01234).view(np.float32))  # a NaN with a payload
    _roundtrip(rows, "synthetic")
    rp, col, val = capi.csr_from_dense(rows)
    assert list(np.diff(rp.astype(np.int64))) == [4, capi.FX_DESC_BINS, 0, capi.FX_DESC_RF, capi.FX_DESC_FLOATS]
    assert list(col[:4]) == [0, 7, 1979, capi.FX_DESC_BINS + 3]


def test_dense_from_csr_of_a_slice_and_of_a_parsed_block():
    rows = np.zeros((3, capi.FX_DESC_FLOATS), np.float32)
    rows[0, 5], rows[1, 6], rows[1, 1985], rows[2, 0] = 1.0, 2.0, 3.0, -0.0
    rp, col, val = capi.csr_from_dense(rows)
    # the last two rows alone, indexed from row_ptr[1]
    assert (util.bits(capi.dense_from_csr(rp[1:], col, val)) == util.bits(rows[1:])).all()
    # the same rows written as a block of max_rows 4, capacity 6, and read back
    rp_o, col_o, val_o, end = capi.csr_layout(4, 6)
    blk = np.zeros(end, np.uint8)
    blk[:16].view(np.uint32)[:] = [3, len(col), len(col), 3]
    blk[rp_o:rp_o + 20].view(np.uint32)[:] = list(rp) + [rp[-1]]
    blk[col_o:col_o + 4 * len(col)].view(np.uint32)[:] = col
    blk[val_o:val_o + 4 * len(col)].view(np.float32)[:] = val
    got = capi.csr_parse(blk, 4, 6)
    assert (got["rows"], got["nnz_stored"], got["rows_stored"]) == (3, 4, 3)
    assert (util.bits(capi.dense_from_csr(got["row_ptr"], got["col"], got["val"])) == util.bits(rows)).all()


def test_full_rows_hook_only_in_the_test_build(fxlib, fxtestlib):
    from feature_extraction_amd import build
    assert b"FX_CSR_FULL_ROWS" not in open(build.LIB, "rb").read()
    assert b"FX_CSR_FULL_ROWS" in open(build.build_test_hooks(), "rb").read()
    assert b"k_csr_write" in open(build.LIB, "rb").read()
