"""Helpers of the descriptor-matching tests (tests/test_match_reference.py, tests/test_gpu_match.py): random sparse rows, CSR
blocks built on the host, and the comparison of fx_match records with capi.match_reference under the rules of include/fx.h's
error bound eps = 2^-23 d2 + 2^-40 (|q|^2 + |t|^2)."""
import numpy as np

from feature_extraction_amd import capi

BINS, SECTOR = capi.FX_DESC_BINS, capi.FX_MATCH_SECTOR


def shift_rows(rows, s):
    """Row i rotated by s[i] azimuth sectors: out[i][c] = rows[i][(c + 165 s[i]) mod 1980] (the rf words stay), so that
    d2(out[i], rows[i], s[i]) = 0."""
    rows = np.asarray(rows, np.float32)
    out = rows.copy()
    for i, si in enumerate(np.broadcast_to(s, (len(rows),))):
        out[i, :BINS] = np.roll(rows[i, :BINS], -SECTOR * int(si))
    return out


def random_rows(rng, n, nnz=(30, 80), lo=0.05, hi=25.0):
    """n dense [1989] float32 rows of nnz[0]..nnz[1] non-zero bins with values in [lo, hi]."""
    rows = np.zeros((n, capi.FX_DESC_FLOATS), np.float32)
    for i in range(n):
        k = int(rng.integers(nnz[0], nnz[1] + 1))
        rows[i, rng.choice(BINS, k, replace=False)] = rng.uniform(lo, hi, k).astype(np.float32)
    return rows


def make_block(rows, max_rows=None, capacity=None, rows_stored=None):
    """The CSR block fx_pack_descriptors_csr would write for these dense rows, as a uint8 array; rows_stored < len(rows) cuts it
    the way a capacity cut does (the rows beyond stay empty, row_ptr repeats nnz_stored).  Returns (block, max_rows, capacity)."""
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, capi.FX_DESC_FLOATS)
    rp, col, val = capi.csr_from_dense(rows)
    n = len(rows)
    stored = n if rows_stored is None else rows_stored
    max_rows = n if max_rows is None else max_rows
    nnz = int(rp[stored])
    capacity = max(nnz, 1) if capacity is None else capacity
    assert stored <= n <= max_rows and nnz <= capacity
    o_rp, o_col, o_val, end = capi.csr_layout(max_rows, capacity)
    b = np.zeros(end, np.uint8)
    b[:16].view(np.uint32)[:] = (n, nnz, int(rp[-1]), stored)
    r = b[o_rp:o_rp + 4 * (max_rows + 1)].view(np.uint32)
    r[:stored + 1] = rp[:stored + 1]
    r[stored + 1:] = nnz
    b[o_col:o_col + 4 * nnz].view(np.uint32)[:] = col[:nnz]
    b[o_val:o_val + 4 * nnz].view(np.uint32)[:] = val[:nnz].view(np.uint32)
    return b, max_rows, capacity


def unambiguous_self_matches(rows, s):
    """Match shift_rows(rows, s) against rows with the reference.  Returns (unambiguous [n] bool, ref): a row is unambiguous
    when the reference's runner-up over (row, shift) exceeds its best by more than 4 eps."""
    ref = capi.match_reference(shift_rows(rows, s), rows, [(0, len(rows), 0, len(rows))])
    d2 = ref["d2"][0]
    ok = np.zeros(len(rows), bool)
    for i in range(len(rows)):
        flat = np.sort(d2[i][~np.isnan(d2[i])])
        if len(flat) >= 2:
            eps = capi.match_epsilon(flat[0], ref["nq2"][i], np.nanmax(ref["nt2"]))
            ok[i] = flat[1] - flat[0] > 4 * eps
    return ok, ref


def compare(got, ref, shifts=12, max_dist2=np.inf, max_ratio=1.0, mutual=False, require_all=False, what=""):
    """fx_match records `got` (MATCH_DTYPE) against match_reference's `ref`:
    - the reported dist2 is within eps of the reference d2 of the reported (train_row, shift), and that d2 within 2 eps of the
      reference minimum;
    - train_row, shift, second_row and the flags are equal wherever the reference gap exceeds 4 eps (a flag is also ambiguous
      when a threshold lies within 2 eps of the tested value);
    - rows without a match (no pair, clipped, NaN, nothing to match) carry the sentinels exactly.
    require_all: no row may be ambiguous.  Returns the number of rows compared field by field."""
    want = ref["rec"]
    assert got.shape == want.shape, what
    assert (got["reserved"] == 0).all() and (got["pair"] == want["pair"]).all(), what
    none = want["train_row"] < 0
    for f in capi.MATCH_DTYPE.names:
        assert (got[f][none].view(np.uint32) == want[f][none].view(np.uint32)).all(), f"{what}: sentinel field {f}"
    ratio2 = float(np.float32(max_ratio) * np.float32(max_ratio))
    exact = 0
    for p, (q0, q1, t0, t1) in enumerate(ref["ranges"]):
        d2 = ref["d2"][p]
        if not d2.size:
            continue
        per_t = np.where(np.isnan(d2), np.inf, d2).min(axis=2)  # [q, t] best over the shifts
        nt2 = ref["nt2"][t0:t1]
        nt2_max = np.nanmax(nt2) if np.isfinite(nt2).any() else 0.0
        nq2 = ref["nq2"][q0:q1]
        nq2_max = np.nanmax(nq2) if np.isfinite(nq2).any() else 0.0
        col_gap_ok = np.zeros(t1 - t0, bool)  # mutual: the train row's two best query rows are more than 4 eps apart
        if mutual:
            for j in range(t1 - t0):
                c = np.sort(per_t[:, j])
                c = c[np.isfinite(c)]
                col_gap_ok[j] = len(c) < 2 or c[1] - c[0] > 4 * capi.match_epsilon(c[1], nq2_max, nt2[j])
        for i in range(q1 - q0):
            g, w = got[q0 + i], want[q0 + i]
            tag = f"{what} pair {p} query row {q0 + i}: got {g}, reference {w}"
            if w["train_row"] < 0:
                continue
            nq2 = ref["nq2"][q0 + i]
            j = int(g["train_row"]) - t0
            assert 0 <= j < t1 - t0 and g["shift"] < shifts and not np.isnan(d2[i, j, 0]), tag
            D, dmin = d2[i, j, int(g["shift"])], np.nanmin(d2[i])
            eps = capi.match_epsilon(D, nq2, nt2[j])
            assert abs(float(g["dist2"]) - D) <= eps, f"{tag}: dist2 off by {abs(float(g['dist2']) - D)} > eps {eps}"
            assert D - dmin <= 2 * eps, tag
            big = capi.match_epsilon(max(D, dmin), nq2, nt2_max)  # (the bound used for gaps: the largest it can be here)
            flat = np.sort(d2[i][~np.isnan(d2[i])])
            rows_sorted = np.sort(per_t[i])
            shift_clear = len(flat) < 2 or flat[1] - flat[0] > 4 * big
            row_clear = not np.isfinite(rows_sorted[1:2]).any() or rows_sorted[1] - rows_sorted[0] > 4 * big
            second_clear = row_clear
            if np.isfinite(rows_sorted[1:2]).any():
                big2 = capi.match_epsilon(rows_sorted[1], nq2, nt2_max)
                second_clear = row_clear and (not np.isfinite(rows_sorted[2:3]).any() or rows_sorted[2] - rows_sorted[1] > 4 * big2)
                # the second-best is a real other row, and its distance is that row's
                j2 = int(g["second_row"]) - t0
                assert 0 <= j2 < t1 - t0 and j2 != j, tag
                assert abs(float(g["dist2_second"]) - per_t[i, j2]) <= capi.match_epsilon(per_t[i, j2], nq2, nt2[j2]), tag
                if row_clear:
                    assert per_t[i, j2] - rows_sorted[1] <= 2 * big2, tag
            else:
                assert g["second_row"] == -1 and np.isposinf(g["dist2_second"]), tag
            if require_all:
                assert shift_clear and row_clear and second_clear, f"{tag}: ambiguous in the reference"
            if row_clear:
                assert g["train_row"] == w["train_row"], tag
            if row_clear and shift_clear:
                assert g["shift"] == w["shift"], tag
            if second_clear:
                assert g["second_row"] == w["second_row"], tag
            flags_clear = row_clear and second_clear
            if np.isfinite(max_dist2):
                flags_clear = flags_clear and abs(D - max_dist2) > 2 * big
            if max_ratio < 1 and np.isfinite(rows_sorted[1:2]).any():
                flags_clear = flags_clear and abs(D - ratio2 * rows_sorted[1]) > 2 * (big + ratio2 * big2)
            if flags_clear:
                assert (g["flags"] & capi.FX_MATCH_ACCEPTED) == (w["flags"] & capi.FX_MATCH_ACCEPTED), tag
            if mutual and row_clear and col_gap_ok[j]:
                assert (g["flags"] & capi.FX_MATCH_MUTUAL) == (w["flags"] & capi.FX_MATCH_MUTUAL), tag
            if not mutual:
                assert not g["flags"] & capi.FX_MATCH_MUTUAL, tag
            exact += bool(row_clear and shift_clear and second_clear)
    return exact
