"""Descriptor matching across azimuth shifts, the part that needs no GPU: the C-ABI's new names and struct sizes, and
capi.match_reference — the numpy statement of include/fx.h's rule — against a brute-force triple loop and on the golden
fixtures' rows rotated by random sector counts."""
import ctypes as C
import glob
import math
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import match_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fx_match_pair", "fx_match_options", "fx_match", "fx_match_options_default", "fx_match_descriptors_csr")


def test_names_declared_exported_and_listed(fxlib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fx.h")).read(), flags=re.S)
    for n in NAMES[:3]:
        assert re.search(r"typedef struct %s\s*\{[^}]*\}\s*%s;" % (n, n), src), n
    for n in NAMES[3:]:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(fxlib, n), n
        assert n in capi.EXPORTS, n
    assert "#define FX_VERSION_MINOR 7" in src and fxlib.fx_version() == 7


def test_struct_sizes_and_default_options(fxlib):
    assert C.sizeof(capi.FxMatchPair) == 16 and C.sizeof(capi.FxMatchOptions) == 16 and C.sizeof(capi.FxMatch) == 32
    assert capi.MATCH_DTYPE.itemsize == 32
    assert [f[0] for f in capi.FxMatch._fields_] == list(capi.MATCH_DTYPE.names)
    o = capi.FxMatchOptions(5, 1.0, 0.5, 9)
    fxlib.fx_match_options_default(C.byref(o))
    assert (o.azimuth_shifts, o.max_dist2, o.max_ratio, o.mutual) == (12, math.inf, 1.0, 0)


def test_pairs_consecutive():
    assert capi.pairs_consecutive([0, 3, 3, 10, 12]) == [(3, 0, 0, 3), (3, 7, 3, 0), (10, 2, 3, 7)]
    assert capi.pairs_consecutive([0, 5]) == [] and capi.pairs_consecutive([0]) == []


def _brute_d2(q, t, shifts):
    """d2[i][j][s] by the definition, one term at a time in Python floats (float64)."""
    out = np.zeros((len(q), len(t), shifts))
    ql, tl = [[float(x) for x in r[:mu.BINS]] for r in q], [[float(x) for x in r[:mu.BINS]] for r in t]
    for i, qi in enumerate(ql):
        for j, tj in enumerate(tl):
            for s in range(shifts):
                k = mu.SECTOR * s
                rot = tj[k:] + tj[:k]  # rot[c] = t[(c + 165 s) mod 1980]
                out[i, j, s] = math.fsum((a - b) * (a - b) for a, b in zip(qi, rot) if a != 0.0 or b != 0.0)
    return out


def _brute_records(d2, pairs, n_q, shifts, max_dist2, max_ratio, mutual):
    """The records by plain loops over d2[q][t][s] (global row indices); fp32 values compared, ties to the lowest row, then shift."""
    rec = []
    f32 = d2.astype(np.float32)
    r2 = np.float32(max_ratio) * np.float32(max_ratio)
    for i in range(n_q):
        rec.append(dict(train_row=-1, shift=0, dist2=np.float32(np.inf), second_row=-1, dist2_second=np.float32(np.inf), flags=0,
                        pair=capi.FX_MATCH_NO_PAIR))
    for p, (q0, qn, t0, tn) in enumerate(pairs):
        for i in range(q0, q0 + qn):
            r = rec[i]
            r["pair"] = p
            per_row = []
            for j in range(t0, t0 + tn):
                best = (np.float32(np.inf), 0)
                for s in range(shifts):
                    if s == 0 or f32[i, j, s] < best[0]:
                        best = (f32[i, j, s], s)
                per_row.append((best[0], j, best[1]))
            per_row.sort(key=lambda x: (x[0], x[1]))
            if per_row:
                r["dist2"], r["train_row"], r["shift"] = per_row[0]
                if len(per_row) > 1:
                    r["dist2_second"], r["second_row"] = per_row[1][0], per_row[1][1]
                ok = r["dist2"] <= np.float32(max_dist2) and (max_ratio >= 1 or r["dist2"] <= r2 * r["dist2_second"])
                r["flags"] = capi.FX_MATCH_ACCEPTED if ok else 0
        if mutual:
            for j in range(t0, t0 + tn):
                c = sorted((min(f32[i, j, :shifts]), i) for i in range(q0, q0 + qn))
                if c and rec[c[0][1]]["train_row"] == j:
                    rec[c[0][1]]["flags"] |= capi.FX_MATCH_MUTUAL
    return rec


@pytest.mark.parametrize("opts", [dict(), dict(shifts=1), dict(max_dist2=9000.0), dict(max_ratio=0.8), dict(mutual=True)],
                         ids=["default", "shifts1", "max_dist2", "max_ratio", "mutual"])
def test_reference_against_brute_force(opts):
    rng = np.random.default_rng(7)
    t = mu.random_rows(rng, 11, nnz=(20, 50))
    q = mu.shift_rows(t[rng.integers(0, 11, 9)], rng.integers(0, 12, 9))
    nz = q != 0
    q[nz] += rng.normal(0, 2.0, int(nz.sum())).astype(np.float32)  # (coarse noise: some rows fail the thresholds)
    q[:, 1980:] = rng.normal(0, 1, (9, 9)).astype(np.float32)  # rf words: ignored
    pairs = [(0, 4, 0, 6), (4, 5, 3, 8)]
    shifts = opts.get("shifts", 12)
    d2 = _brute_d2(q, t, shifts)
    ref = capi.match_reference(q, t, pairs, **opts)
    for p, (q0, qn, t0, tn) in enumerate(pairs):
        assert ref["ranges"][p] == (q0, q0 + qn, t0, t0 + tn)
        np.testing.assert_allclose(ref["d2"][p], d2[q0:q0 + qn, t0:t0 + tn], rtol=1e-13, atol=0)
    want = _brute_records(d2, pairs, len(q), shifts, opts.get("max_dist2", np.inf), opts.get("max_ratio", 1.0), opts.get("mutual", False))
    flags = set()
    for i, w in enumerate(want):
        for f, v in w.items():
            assert ref["rec"][f][i] == v, (i, f, ref["rec"][i], w)
        flags.add(int(w["flags"]))
    if opts.get("max_dist2") or opts.get("max_ratio"):
        assert {0, capi.FX_MATCH_ACCEPTED} <= flags, "the threshold must split the rows"
    if opts.get("mutual"):
        assert any(f & capi.FX_MATCH_MUTUAL for f in flags) and any(not f & capi.FX_MATCH_MUTUAL for f in flags)


def test_reference_special_rows_and_clipping():
    rng = np.random.default_rng(3)
    t = mu.random_rows(rng, 6)
    q = t.copy()
    q[1, :mu.BINS] = np.nan  # an FX_FLAG_NBR_OVERFLOW row as a query
    t[2, 5] = np.nan  # and one as a train row: skipped
    q[3] = 0  # an all-zero descriptor matches like any other
    ref = capi.match_reference(q, t, [(0, 5, 0, 100), (5, 10, 4, 0)])
    r = ref["rec"]
    assert ref["ranges"] == [(0, 5, 0, 6), (5, 6, 4, 4)]
    assert r["train_row"][0] == 0 and r["dist2"][0] == 0 and r["shift"][0] == 0
    assert r["train_row"][1] == -1 and np.isposinf(r["dist2"][1]) and r["pair"][1] == 0 and r["flags"][1] == 0
    assert r["train_row"][2] != 2 and r["second_row"][2] != 2  # (its own copy holds a NaN)
    assert r["dist2"][3] == pytest.approx(ref["nt2"][r["train_row"][3]], rel=1e-6) and r["train_row"][4] == 4  # |0 - t|^2
    assert r["pair"][5] == 1 and r["train_row"][5] == -1 and r["second_row"][5] == -1
    with pytest.raises(ValueError):
        capi.match_reference(q, t, [(0, 3, 0, 6), (2, 2, 0, 6)])


def test_golden_rows_find_themselves_at_the_expected_shift():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    assert len(files) >= 5
    rng = np.random.default_rng(2024)
    for f in files:
        rows = np.load(f)["descriptors"]
        assert not np.isnan(rows).any()
        s = rng.integers(0, 12, len(rows))
        ok, ref = mu.unambiguous_self_matches(rows, s)
        r = ref["rec"]
        print(f"{os.path.basename(f)}: {int(ok.sum())} unambiguous rows of {len(rows)}")
        assert 2 * ok.sum() >= len(rows), f"{f}: the test would go vacuous"
        idx = np.flatnonzero(ok)
        assert (r["train_row"][idx] == idx).all() and (r["shift"][idx] == s[idx]).all(), f
        eps = capi.match_epsilon(0.0, ref["nq2"][idx], ref["nt2"][idx])
        assert (r["dist2"][idx] <= eps).all(), f
        assert (r["flags"][idx] == capi.FX_MATCH_ACCEPTED).all()
