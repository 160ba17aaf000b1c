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


# ---- the row families at fp32's edges (tests/match_util.py): the exact d2, the conditions on the inputs, the non-finite rule
# and the tie rules, all on the CPU.  tests/test_gpu_match_numerics.py runs the same families on the GPU.
Q = 2.0 ** -149  # the smallest fp32 subnormal


def test_round_f32_and_exact_d2_by_hand():
    F = mu.Fraction
    for x, want in [(F(9, 2) * F(Q), 4 * Q), (F(11, 2) * F(Q), 6 * Q), (F(Q) / 2, 0.0), (F(Q) / 2 + F(Q) / 2 ** 60, Q), (F(0), 0.0),
                    (F(2) ** -126 - F(Q) / 2, 2.0 ** -126), (F(1) + F(2) ** -24, 1.0), (F(1) + 3 * F(2) ** -24, 1 + 2.0 ** -22),
                    (F(mu.F32_OVERFLOW), np.inf), (F(mu.F32_OVERFLOW) - 1, mu.FLT_MAX), (F(2) ** 200, np.inf)]:
        got = mu.round_f32(x)
        assert got.dtype == np.float32 and got.view(np.uint32) == np.float32(want).view(np.uint32), (x, got, want)
    z = np.zeros(capi.FX_DESC_FLOATS, np.float32)
    a = z.copy()
    a[500] = 1.5 * 2.0 ** -74
    x, f = mu.exact_d2(a, z, 7)
    assert x == F(9, 2) * F(Q) and f == np.float32(4 * Q)
    a[500] = mu.W64
    x, f = mu.exact_d2(z, a, 3)
    assert x == F(2) ** 128 * (1 - F(2) ** -24) ** 2 and f == np.float32(2.0 ** 128 * (1 - 2.0 ** -23)) and f < mu.FLT_MAX
    a[500] = 2.0 ** 64
    assert np.isposinf(mu.exact_d2(a, z, 0)[1]) and mu.exact_d2(a, a, 0) == (0, np.float32(0))
    b = z.copy()
    b[(500 + 165 * 5) % 1980] = -2.0 ** 64  # meets a[500] under shift 5: (2^64 + 2^64)^2
    assert mu.exact_d2(a, b, 5)[0] == F(2) ** 130 and mu.exact_d2(a, b, 4)[0] == F(2) ** 129
    # ordinary rows: the brute-force float64 sum agrees to its own precision
    rng = np.random.default_rng(5)
    t = mu.random_rows(rng, 3)
    q = mu.shift_rows(t, [4, 0, 11]) * np.float32(1.01)
    d2 = _brute_d2(q, t, 12)
    for i, j, s in [(0, 0, 4), (1, 2, 0), (2, 2, 11), (2, 1, 6)]:
        assert float(mu.exact_d2(q[i], t[j], s)[0]) == pytest.approx(d2[i, j, s], rel=1e-14)


FINITE_FAMILIES = ["overflow", "cancellation", "underflow", "signs", "thresholds"]


@pytest.mark.parametrize("name", FINITE_FAMILIES)
def test_family_reference_is_exact_and_unambiguous(name):
    """(i) no query row is ambiguous under compare's rules (gap above 4 eps, or a tie between values known bit for bit);
    (ii) the reference's d2 of the best and the second-best row is within eps / 8 of exact_d2, and its fp32 record values are the
    exact values correctly rounded."""
    q, t, pairs, _, _ = mu.family(name)
    ref = mu.family_reference(name)
    r = ref["rec"]
    assert len(q) <= 64 and len(t) <= 130 and np.isfinite(q).all() and np.isfinite(t).all()
    assert mu.compare(r, ref, require_all=True, what=name) == int((r["train_row"] >= 0).sum()) == sum(p[1] for p in pairs) >= 48
    worst = 0.0
    for p, (q0, q1, t0, t1) in enumerate(ref["ranges"]):
        for i in range(q0, q1):
            for row, f in ((r["train_row"][i], r["dist2"][i]), (r["second_row"][i], r["dist2_second"][i])):
                d = ref["d2"][p][i - q0, row - t0]
                s = int(r["shift"][i]) if row == r["train_row"][i] else int(np.argmin(d))
                x, x32 = mu.exact_d2(q[i], t[row], s)
                eps = capi.match_epsilon(float(x), ref["nq2"][i], ref["nt2"][row])
                assert abs(mu.Fraction(d[s]) - x) <= mu.Fraction(eps) / 8, (name, i, row, s, d[s], float(x), eps)
                assert f.view(np.uint32) == x32.view(np.uint32), (name, i, row, s, f, x32)
                worst = max(worst, float(abs(mu.Fraction(d[s]) - x)) / eps)
    print(f"{name}: the reference's worst |d2 - exact| / eps = {worst:.3g}")
    # compare counts a side without a non-zero bin as one candidate over the shifts: the reference's fp32 values must then be
    # equal at every shift, although it sums the terms in rolled order
    for p, (q0, q1, t0, t1) in enumerate(ref["ranges"]):
        f = ref["d2"][p].astype(np.float32).view(np.uint32)
        flat = f[ref["nq2"][q0:q1] == 0].reshape(-1, f.shape[2]), f[:, ref["nt2"][t0:t1] == 0].reshape(-1, f.shape[2])
        for x in flat:
            assert (x == x[:, :1]).all(), name


def test_family_overflow_ties_and_flags():
    q, t, pairs, info, _ = mu.family("overflow")
    r = mu.family_reference("overflow")["rec"]
    acc = capi.FX_MATCH_ACCEPTED
    inf, copies = info["all_inf"], info["copies"]
    assert len(set(q[:8].max(axis=1)) | set(q[:8].min(axis=1))) == 9  # eight different words (and zero)
    assert (r["train_row"][:2] == 0).all() and (r["dist2"][:2] == np.float32(2.0 ** 128 * (1 - 2.0 ** -23))).all()
    assert (r["second_row"][:8] == 1).all() and (r["train_row"][2:8] == 0).all()
    assert (r["train_row"][8:40] == 3).all() and (r["second_row"][8:40] == 4).all() and not r["shift"][inf].any()
    assert (r["train_row"][56:] == 90).all() and (r["second_row"][56:] == 91).all()  # +inf against ordinary rows too
    assert (r["train_row"][copies] == info["src"]).all() and (r["shift"][copies] == info["s"]).all() and len(set(info["src"])) == 16
    assert np.isposinf(r["dist2"][inf]).all() and np.isposinf(r["dist2_second"][inf]).all() and np.isposinf(r["dist2_second"][:2]).all()
    assert np.isfinite(r["dist2"][copies]).all() and np.isfinite(r["dist2_second"][copies]).all() and (r["flags"] == acc).all()
    finite_max = mu.family_reference("overflow", max_dist2=3e38)["rec"]["flags"]
    assert np.flatnonzero(finite_max).tolist() == copies  # (the d2 of rows 0 and 1 is above 3e38)
    half = mu.family_reference("overflow", max_ratio=0.5)["rec"]["flags"]
    assert (half == acc).all()  # 0.25 * inf = inf: a finite dist2 and +inf both pass
    assert not mu.family_reference("overflow", max_ratio=0.0)["rec"]["flags"].any()  # 0 * inf is NaN
    m = mu.family_reference("overflow", mutual=True)["rec"]["flags"] & capi.FX_MATCH_MUTUAL
    assert np.flatnonzero(m).tolist() == [0, 8] + copies  # equal distances: the lowest query row is the train row's minimiser


def _kinds(d):
    """The kinds of fp32 distances in d: 0 zero, 1 subnormal, 2 normal, 3 +inf."""
    return {0 if x == 0 else 3 if np.isposinf(x) else 1 if x < 2.0 ** -126 else 2 for x in d}


@pytest.mark.parametrize("name,pair,kinds", [("overflow", 2, {2, 3}), ("underflow", 0, {0, 1, 2}), ("cancellation", 0, {0, 2})])
def test_family_records_make_registration_depend_on_the_pool_order(name, pair, kinds):
    """mu.ranking_keypoints on the reference's records: the pair is valid with the expected hypothesis and inliers at every
    hyp_corr, and a record from behind the pool that is ranked ahead of it — a +inf, a subnormal or a normal distance taken
    for 0 — changes the result.  (A record that wrongly falls behind the pool does not show here; a -0.0, which would, is
    refused by compare on its sign bit.)"""
    q, t, pairs, _, _ = mu.family(name)
    rec = mu.family_reference(name, mutual=True)["rec"]
    q0, qn = pairs[pair][:2]
    d = rec["dist2"][q0:q0 + qn]
    assert _kinds(d) == kinds
    finite = int(np.isfinite(d).sum())
    seen = set()
    for H in range(2, finite - 1):
        q_kp, t_kp, exp = mu.ranking_keypoints(rec, pairs, H, len(t))
        r = capi.register_reference(q_kp, t_kp, rec, pairs, hyp_corr=H)["rec"][pair]
        assert r["n_corr"] == qn > H and r["flags"] == capi.FX_REG_VALID and (r["hyp_a"], r["hyp_b"], r["n_inliers"]) == exp[pair], (H, r, exp)
        order = q0 + np.lexsort((np.arange(qn), d.view(np.uint32)))
        for kind in (1, 2, 3):  # the last record of that kind behind the pool, ranked as if it were 0
            behind = [i for i in order[H:] if _kinds([rec["dist2"][i]]) == {kind}]
            if behind and rec["dist2"][order[H - 2]] > 0:  # (among zeros the query row decides: a new 0 need not rank ahead)
                bad = rec.copy()
                bad["dist2"][behind[-1]] = 0.0
                rb = capi.register_reference(q_kp, t_kp, bad, pairs, hyp_corr=H)["rec"][pair]
                assert (rb["hyp_a"], rb["hyp_b"], rb["n_inliers"]) != exp[pair], (H, kind, behind[-1])
                seen.add(kind)
    assert seen == kinds - {0}


def test_family_thresholds_cover_every_combination():
    r = mu.family_reference("thresholds")["rec"]
    kind = lambda x: 0 if x == 0 else 2 if np.isposinf(x) else 1
    seen = {(kind(a), kind(b)) for a, b in zip(r["dist2"], r["dist2_second"])}
    assert seen == {(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)}
    for opts in mu.THRESHOLDS:
        f = mu.family_reference("thresholds", **opts)["rec"]["flags"]
        print(opts, int((f & capi.FX_MATCH_ACCEPTED != 0).sum()), "accepted of", len(f))
    assert (mu.family_reference("thresholds", max_dist2=0.0)["rec"]["flags"] == np.where(r["dist2"] == 0, 1, 0)).all()
    assert (mu.family_reference("thresholds", max_ratio=0.0)["rec"]["flags"] == np.where((r["dist2"] == 0) & np.isfinite(r["dist2_second"]), 1, 0)).all()
    for ratio in (1.0, 1.5, np.inf):
        assert mu.family_reference("thresholds", max_ratio=ratio)["rec"]["flags"].all()
    assert (mu.family_reference("thresholds", max_ratio=-0.5)["rec"]["flags"] == mu.family_reference("thresholds", max_ratio=0.5)["rec"]["flags"]).all()


def test_family_nonfinite_rows_never_match_and_equal_nan_rows():
    q, t, pairs, info, _ = mu.family("nonfinite")
    qn, tn, _, _, _ = mu.family("nonfinite", nan=True)
    assert np.isinf(q).sum() == 5 and np.isinf(t).sum() == 6 and (np.isinf(q) == np.isnan(qn)).all() and (np.isinf(t) == np.isnan(tn)).all()
    for opts in (dict(), dict(mutual=True)):
        ref, ref_nan = mu.family_reference("nonfinite", **opts), capi.match_reference(qn, tn, pairs, **opts)
        r = ref["rec"]
        assert r.tobytes() == ref_nan["rec"].tobytes()
        bad = info["q_bad"]
        assert (r["train_row"][bad] == -1).all() and np.isposinf(r["dist2"][bad]).all() and not r["flags"][bad].any() and (r["pair"][bad] == 0).all()
        assert (r["second_row"][bad] == -1).all() and np.isposinf(r["dist2_second"][bad]).all()
        assert not np.isin(r["train_row"], info["t_bad"]).any() and not np.isin(r["second_row"], info["t_bad"]).any()
        assert np.isnan(ref["d2"][0][bad]).all() and np.isnan(ref["d2"][0][:, info["t_bad"]]).all()
        assert np.isfinite(ref["d2"][0][np.ix_(np.setdiff1d(np.arange(64), bad), np.setdiff1d(np.arange(130), info["t_bad"]))]).all()
        n = mu.compare(r, ref, require_all=True, what="nonfinite", **opts)
        assert n == 64 - len(bad)


def test_compare_refuses_a_vacuous_pass():
    """A reference whose eps is not finite (rows of an infinity under the old NaN-only rule) must not let any dist2 through,
    a negative zero is a negative distance, and a pinned +inf is not met by FLT_MAX."""
    q, t, pairs, _, _ = mu.family("overflow")
    ref = mu.family_reference("overflow")
    bad = ref["rec"].copy()
    bad["dist2"][5] = mu.FLT_MAX
    with pytest.raises(AssertionError, match="pinned"):
        mu.compare(bad, ref, what="FLT_MAX for inf")
    ref_t = mu.family_reference("thresholds")
    neg = ref_t["rec"].copy()
    neg["dist2"][0] = -0.0
    with pytest.raises(AssertionError, match="negative"):
        mu.compare(neg, ref_t, what="-0.0")
    fake = dict(ref_t, nq2=ref_t["nq2"].copy())
    fake["nq2"][3] = np.inf  # eps = inf for row 3
    off = ref_t["rec"].copy()
    mu.compare(off, fake, what="equal bits")
    off["dist2"][3] = 0.0
    with pytest.raises(AssertionError, match="pinned"):
        mu.compare(off, fake, what="eps = inf")
