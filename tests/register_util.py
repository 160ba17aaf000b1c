"""Helpers of the registration tests (tests/test_register_reference.py, tests/test_gpu_register.py): synthetic correspondences
with a known motion, hand-built fx_match records, and the field-by-field comparison with capi.register_reference."""
import math

import numpy as np

from feature_extraction_amd import capi


def scene(rng, n, yaw, t, sigma=0.03, n_outliers=0, half=50.0):
    """n query keypoints uniform in a (2 half)^2 field (z in [-1, 2]) and their train keypoints Rz(yaw) q + t with Gaussian noise
    sigma on every coordinate; n_outliers of them, picked at random, get a train keypoint anywhere in the field instead.
    Returns ([n, 4] float32 query rows, [n, 4] float32 train rows, [n] bool: a true correspondence)."""
    q = np.zeros((n, 4), np.float32)
    q[:, :2] = rng.uniform(-half, half, (n, 2))
    q[:, 2] = rng.uniform(-1, 2, n)
    q[:, 3] = rng.uniform(-0.3, 0.3, n)  # (elevation: not a coordinate)
    x, y, z = (q[:, k].astype(np.float64) for k in range(3))
    c, s = math.cos(yaw), math.sin(yaw)
    tr = np.stack([c * x - s * y + t[0], s * x + c * y + t[1], z + t[2]], axis=1) + sigma * rng.standard_normal((n, 3))
    true = np.ones(n, bool)
    if n_outliers:
        out = rng.choice(n, n_outliers, replace=False)
        true[out] = False
        tr[out, :2] = rng.uniform(-half, half, (n_outliers, 2))
    tt = np.zeros((n, 4), np.float32)
    tt[:, :3] = tr
    return q, tt, true


def records(n_rows, train_rows, d2=None, flags=capi.FX_MATCH_ACCEPTED, pair=0):
    """fx_match records as the match would leave them: row i matched to train_rows[i] at distance d2[i] (default: rising with i)."""
    m = np.zeros(n_rows, capi.MATCH_DTYPE)
    m["train_row"] = train_rows
    m["dist2"] = np.arange(n_rows, dtype=np.float32) + 1 if d2 is None else d2
    m["second_row"], m["dist2_second"] = -1, np.inf
    m["flags"], m["pair"] = flags, pair
    return m


def run_reference(q, t, train_rows=None, d2=None, **opts):
    """register_reference on one pair: query row i matched to train row train_rows[i] (default i)."""
    n = len(q)
    m = records(n, np.arange(n) if train_rows is None else train_rows, d2)
    return capi.register_reference(q, t, m, [(0, n, 0, len(t))], **opts)


def apply(r, p):
    return np.array([r["c"] * p[0] - r["s"] * p[1] + r["tx"], r["s"] * p[0] + r["c"] * p[1] + r["ty"]])


def apply_truth(yaw, t, p):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([c * p[0] - s * p[1] + t[0], s * p[0] + c * p[1] + t[1]])


def multi_pair_case(rng, sizes, outlier_share=0.3, sigma=0.03, gap=0):
    """One pair per entry of sizes: that many query rows, as many train rows in shuffled order, a motion of its own.  `gap` rows
    in no pair follow every pair's query rows.  Returns (query rows, train rows, fx_match records, pairs)."""
    qs, ts, ms, pairs = [], [], [], []
    q0 = t0 = 0
    for p, n in enumerate(sizes):
        q, t, _ = scene(rng, n, rng.uniform(-0.6, 0.6), rng.uniform(-4, 4, 3), sigma, int(outlier_share * n))
        perm = rng.permutation(n)
        t_sh = np.zeros_like(t)
        t_sh[perm] = t  # train row perm[i] is query row i's partner
        m = records(n, t0 + perm, rng.uniform(0.5, 200, n).astype(np.float32), pair=p)
        qs.append(q), ts.append(t_sh), ms.append(m)
        pairs.append((q0, n, t0, n))
        q0, t0 = q0 + n, t0 + n
        if gap:
            qs.append(np.zeros((gap, 4), np.float32))
            ms.append(records(gap, -1, np.inf, flags=0, pair=capi.FX_MATCH_NO_PAIR))
            q0 += gap
    return np.concatenate(qs), np.concatenate(ts), np.concatenate(ms), pairs


def assert_equal(got, inl, ref, what=""):
    """fx_registration records `got` (REG_DTYPE) and inlier words `inl` against register_reference's `ref`: integers and inlier
    words equal, the five doubles and rms bit for bit."""
    want = ref["rec"]
    assert got.shape == want.shape, what
    for f in ("n_corr", "n_inliers", "flags", "hyp_a", "hyp_b"):
        bad = np.flatnonzero(got[f] != want[f])
        assert not len(bad), f"{what}: {f} differs at pairs {bad[:8].tolist()}: got {got[bad[:4]]}, reference {want[bad[:4]]}"
    for f in ("c", "s", "tx", "ty", "tz", "rms"):
        u = np.uint64 if got[f].dtype.itemsize == 8 else np.uint32
        bad = np.flatnonzero(got[f].view(u) != want[f].view(u))
        assert not len(bad), f"{what}: {f} differs in its bits at pairs {bad[:8].tolist()}: got {got[bad[:4]]}, reference {want[bad[:4]]}"
    if inl is not None:
        bad = np.flatnonzero(np.asarray(inl).astype(np.uint32) != ref["inlier"])
        assert not len(bad), f"{what}: inlier words differ at rows {bad[:8].tolist()}"


# ---- the hypothesis stage restated for inspection, and the inputs of the numerics tests (tests/test_gpu_register_numerics.py)
TINY32 = np.float32(2.0 ** -126)  # the smallest normal float32


def _subnormal(x):
    return (x != 0) & (np.abs(x) < TINY32)


def sample_of(H, a, b):
    """The index of the sample (a, b), a < b, of pool ranks among the H (H - 1) / 2 lexicographic ones."""
    return a * (H - 1) - a * (a - 1) // 2 + (b - a - 1)


def ranks_of(H, idx):
    """The pool ranks (a, b) of sample idx: the inverse of sample_of."""
    a = 0
    while idx >= H - 1 - a:
        idx -= H - 1 - a
        a += 1
    return a, a + 1 + idx


def census(q, t, m, pairs, **opts):
    """What the hypothesis stage of fx_register_matches meets on these inputs, pair by pair: the stage restated in numpy float32
    on the correspondences register_reference gathers, with every gate counted where the definition applies it (a sample counts
    at the first gate that rejects it).  Returns a list of dicts, one a pair:
      n_corr, H, n_samples
      baseline_rejected, length_rejected, nrm_rejected   samples a gate rejected
      nan_passed       samples the length gate let through because |sqrt(lq2) - sqrt(lt2)| is NaN
      nrm_inf          samples that reached nrm with nrm = +inf
      nrm_zero_distinct  samples rejected by nrm > 0 whose two query keypoints differ and whose two train keypoints differ
      cs_nonfinite     samples that passed every gate with a non-finite c or s
      cs_zero          samples that passed every gate with nrm = +inf and c = s = 0
      subnormal        samples with a subnormal lq2 or lt2, or, past the first two gates, a subnormal dot, crs, dot dot, crs crs
                       or sum of the two
      subnormal_nrm    samples past the first two gates whose dot dot + crs crs, the operand of nrm's root, is subnormal (nrm
                       itself never is: the root of the smallest subnormal is 2^-74.5)
      counts           agreeing correspondences of every sample (0 for a rejected one)
      live             the samples with at least 2 agreeing;  max_count, top: the largest count and the samples that reach it
      winner           the lowest sample of top, or None;  fallback: the first fit agrees with fewer than 2 (None without a winner)
      on_edge          per correspondence, rx rx + ry ry == id2 exactly under the winner's transform (fp32)
      retest_on_edge   per correspondence, the fp64 residual of the re-test == the fp64 threshold exactly
      pool, pool_float the pool by (dist2 bits, row), and the one a float comparison of dist2 would give (NaN last, -0 = +0)
      rows             the query rows of the correspondences;  lq2, lt2, diff, nrm, c, s: the stage's values, a sample each"""
    o = dict(capi.REG_DEFAULTS)
    o.update(opts)
    f32 = np.float32
    ref = capi.register_reference(q, t, m, pairs, **opts)
    idist, mb = f32(o["inlier_dist"]), f32(o["min_baseline"])
    with np.errstate(all="ignore"):
        mb2, gate, id2 = mb * mb, f32(2) * idist, idist * idist
    id2d = float(idist) * float(idist)
    kq, kt = np.asarray(q, f32), np.asarray(t, f32)
    out = []
    for p, rows in enumerate(ref["corr"]):
        i = rows.astype(np.int64)
        tr = m["train_row"][i].astype(np.int64)
        n = len(i)
        P = np.concatenate([kq[i][:, :2], kt[tr][:, :2]], axis=1) if n else np.zeros((0, 4), f32)
        H = min(n, int(o["hyp_corr"]))
        d2 = m["dist2"][i]
        pool = np.lexsort((i, d2.view(np.uint32)))[:H]
        with np.errstate(all="ignore"):
            pool_float = np.lexsort((i, d2 + f32(0)))[:H]
        c = dict(n_corr=n, H=H, n_samples=H * (H - 1) // 2, rows=rows, pool=pool, pool_float=pool_float, winner=None, fallback=None,
                 on_edge=np.zeros(n, bool), retest_on_edge=np.zeros(n, bool))
        a, b = np.triu_indices(H, 1) if H >= 2 else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        A, B = P[pool[a]], P[pool[b]]
        with np.errstate(all="ignore"):
            dqx, dqy, dtx, dty = B[:, 0] - A[:, 0], B[:, 1] - A[:, 1], B[:, 2] - A[:, 2], B[:, 3] - A[:, 3]
            lq2, lt2 = dqx * dqx + dqy * dqy, dtx * dtx + dty * dty
            base = (lq2 >= mb2) & (lt2 >= mb2)
            diff = np.abs(np.sqrt(lq2) - np.sqrt(lt2))
            length = ~(diff > gate)
            dot, crs = dqx * dtx + dqy * dty, dqx * dty - dqy * dtx
            dd, kk = dot * dot, crs * crs
            nrm2 = dd + kk
            nrm = np.sqrt(nrm2)
            pos = nrm > 0
            cc, ss = dot / nrm, crs / nrm
            mqx, mqy, mtx, mty = (A[:, 0] + B[:, 0]) * f32(0.5), (A[:, 1] + B[:, 1]) * f32(0.5), (A[:, 2] + B[:, 2]) * f32(0.5), (A[:, 3] + B[:, 3]) * f32(0.5)
            tx, ty = mtx - (cc * mqx - ss * mqy), mty - (ss * mqx + cc * mqy)
            reach, keep = base & length, base & length & pos
            counts = np.zeros(len(a), np.int64)
            ks = np.flatnonzero(keep)
            for lo in range(0, len(ks), 512):
                k = ks[lo:lo + 512]
                rx = ((cc[k, None] * P[None, :, 0] - ss[k, None] * P[None, :, 1]) + tx[k, None]) - P[None, :, 2]
                ry = ((ss[k, None] * P[None, :, 0] + cc[k, None] * P[None, :, 1]) + ty[k, None]) - P[None, :, 3]
                counts[k] = (rx * rx + ry * ry <= id2).sum(axis=1)
            distinct = ((A[:, 0] != B[:, 0]) | (A[:, 1] != B[:, 1])) & ((A[:, 2] != B[:, 2]) | (A[:, 3] != B[:, 3]))
            c.update(baseline_rejected=int((~base).sum()), length_rejected=int((base & ~length).sum()), nrm_rejected=int((reach & ~pos).sum()),
                     nan_passed=int((base & np.isnan(diff)).sum()), nrm_inf=int((reach & np.isposinf(nrm)).sum()),
                     nrm_zero_distinct=int((reach & (nrm == 0) & distinct).sum()),
                     cs_nonfinite=int((keep & ~(np.isfinite(cc) & np.isfinite(ss))).sum()),
                     cs_zero=int((keep & np.isposinf(nrm) & (cc == 0) & (ss == 0)).sum()),
                     subnormal=int((_subnormal(lq2) | _subnormal(lt2) | (reach & (_subnormal(dot) | _subnormal(crs) | _subnormal(dd) | _subnormal(kk) | _subnormal(nrm2)))).sum()),
                     subnormal_nrm=int((reach & _subnormal(nrm2)).sum()), counts=counts, lq2=lq2, lt2=lt2, diff=diff, nrm=nrm, c=cc, s=ss)
            live = np.flatnonzero(counts >= 2)
            c["live"] = live
            c["max_count"] = int(counts[live].max()) if len(live) else 0
            c["top"] = np.flatnonzero((counts >= 2) & (counts == c["max_count"]))
            if len(live):
                w = int(c["top"][0])
                c["winner"] = w
                rx = ((cc[w] * P[:, 0] - ss[w] * P[:, 1]) + tx[w]) - P[:, 2]
                ry = ((ss[w] * P[:, 0] + cc[w] * P[:, 1]) + ty[w]) - P[:, 3]
                r2 = rx * rx + ry * ry
                c["on_edge"] = r2 == id2
                Pd = [tuple(float(x) for x in row) for row in P]
                fit = capi._register_fit(Pd, [int(x) for x in np.flatnonzero(r2 <= id2)], float(cc[w]), float(ss[w]))
                r2d = np.array([capi._register_r2(Pd, k, *fit) for k in range(n)])
                c["retest_on_edge"] = r2d == id2d
                c["fallback"] = bool((r2d <= id2d).sum() < 2)
        # the restatement and the reference agree on the winner, or one of them is wrong
        r = ref["rec"][p]
        if c["winner"] is None:
            assert r["flags"] & capi.FX_REG_NO_HYPOTHESIS, (p, r)
        else:
            wa, wb = ranks_of(H, c["winner"])
            assert (r["hyp_a"], r["hyp_b"]) == (rows[pool[wa]], rows[pool[wb]]), (p, r, wa, wb)
        out.append(c)
    return out


def assemble(cases):
    """Hand-built pairs -> (query rows, train rows, fx_match records, pairs).  A case is (q_xy, t_xy, dist2) with a correspondence
    per entry: query keypoint q_xy[k] (z = 0) matched to train keypoint t_xy[k] (z = 0.5) at dist2[k] (floats, or uint32 words)."""
    qs, ts, ms, pairs = [], [], [], []
    r0 = 0
    for p, (qxy, txy, d2) in enumerate(cases):
        n = len(qxy)
        q, t = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        if n:
            q[:, :2], t[:, :2], t[:, 2] = np.asarray(qxy, np.float32), np.asarray(txy, np.float32), 0.5
        d2 = np.asarray(d2)
        m = records(n, r0 + np.arange(n), d2.view(np.float32) if d2.dtype == np.uint32 else d2.astype(np.float32), pair=p)
        qs.append(q), ts.append(t), ms.append(m)
        pairs.append((r0, n, r0, n))
        r0 += n
    return np.concatenate(qs), np.concatenate(ts), np.concatenate(ms), pairs


def up(x, steps=1):
    """The float32 `steps` ulps above x (below for negative steps)."""
    x = np.float32(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, np.float32(np.inf if steps > 0 else -np.inf))
    return x


# -- family 1: every gate at equality next to a twin one float on the other side.  inlier_dist = 0.25, min_baseline = 2: mb2 = 4,
# the length gate 0.5, id2 = 0.0625; all coordinates are dyadic, so every intermediate of the kept twin is exact.
GATE_OPTS = dict(inlier_dist=0.25, min_baseline=2.0, min_inliers=2, hyp_corr=64)
BELOW2 = (float(up(2.0, -1)), 2.0 ** -11)  # (2 - 2^-23)^2 + 2^-22 = 4 - 2^-22 after rounding: the float below 4


def gate_cases():
    """(name, case, expected) of the gate pairs: expected = dict of record fields (hyp = (hyp_a, hyp_b) as rows of the pair, None:
    FX_REG_NO_HYPOTHESIS) written down by hand."""
    T = np.array([1.0, 1.0])
    at = lambda pts, off=(0, 0): [tuple(np.asarray(p, np.float64) + T + np.asarray(off)) for p in pts]
    out = []
    # the baseline gate on the query side: lq2 == 4 with lt = 2.25 (the transform splits 0.25: residuals 0.125), and lq2 the float below 4
    out.append(("baseline q ==", ([(0, 0), (2, 0)], [(1, 1), (3.25, 1)], [1, 2]), dict(hyp=(0, 1), n=2, c=1.0, s=0.0, tx=1.125, ty=1.0)))
    out.append(("baseline q below", ([(0, 0), BELOW2], [(1, 1), (3.25, 1)], [1, 2]), dict(hyp=None)))
    out.append(("baseline t ==", ([(0, 0), (2.25, 0)], [(1, 1), (3, 1)], [1, 2]), dict(hyp=(0, 1), n=2, c=1.0, s=0.0, tx=0.875, ty=1.0)))
    out.append(("baseline t below", ([(0, 0), (2.25, 0)], [(0, 0), BELOW2], [1, 2]), dict(hyp=None)))
    # the length gate: lengths 4 and 4.5 on an axis; the same pair sits at equality in the agreement test and in the re-test
    # (both residuals are exactly 0.25).  The twin's train length is the next float: the difference of the roots is 0.5 + 2^-21
    out.append(("length ==", ([(0, 0), (4, 0)], [(0, 0), (4.5, 0)], [1, 2]), dict(hyp=(0, 1), n=2, c=1.0, s=0.0, tx=0.25, ty=0.0, rms=0.25)))
    out.append(("length beyond", ([(0, 0), (4, 0)], [(0, 0), (float(up(4.5)), 0)], [1, 2]), dict(hyp=None)))
    # agreement: motion M1 = + (1, 1) carried by rows 2, 3 with row 4 exactly 0.25 off it (and within the baseline of both, so it
    # forms no sample of its own); motion M2 by rows 0, 1, whose sample is the lower one.  3 against 2: M1.  In the twin row 4 is
    # one float farther: 2 against 2, and the lower sample, M2's, wins
    q5 = [(0, 40), (17, 40), (0, 0), (3, 0), (1.5, 0)]
    t5 = [(-7, 70), (10, 70)] + at(q5[2:4]) + at(q5[4:], (0.25, 0))
    out.append(("agreement ==", (q5, t5, [1, 2, 3, 4, 5]), dict(hyp=(2, 3), n=3, c=1.0, s=0.0, inlier=[0, 0, 1, 1, 1])))
    t5b = list(t5)
    t5b[4] = (float(up(t5[4][0])), t5[4][1])
    out.append(("agreement beyond", (q5, t5b, [1, 2, 3, 4, 5]), dict(hyp=(0, 1), n=2, c=1.0, s=0.0, tx=-7.0, ty=30.0, inlier=[1, 1, 0, 0, 0])))
    # the re-test: hyp_corr = 2 in its own launch (RETEST_OPTS): the one sample is rows 0, 1, exact; rows 2 (0.125 off) and 3 agree,
    # the first fit moves by 0.125 / 4, and row 4, 0.28125 off the hypothesis, is exactly 0.25 off the first fit
    return out


RETEST_OPTS = dict(GATE_OPTS, hyp_corr=2)


def retest_cases():
    q = [(0, 0), (4, 0), (1, 0), (2, 0), (3, 0)]
    t = [(1, 1), (5, 1), (2.125, 1), (3, 1), (4.28125, 1)]
    tb = list(t)
    tb[4] = (float(up(t[4][0])), 1)
    return [("re-test ==", (q, t, [1, 2, 3, 4, 5]), dict(hyp=(0, 1), n=5, c=1.0, s=0.0, inlier=[1] * 5)),
            ("re-test beyond", (q, tb, [1, 2, 3, 4, 5]), dict(hyp=(0, 1), n=4, c=1.0, s=0.0, tx=1.03125, ty=1.0, inlier=[1, 1, 1, 1, 0]))]


# a min_baseline whose square rounds to 0: coincident keypoints pass the baseline gate, and nrm > 0 alone keeps them from 0 / 0
TINY_OPTS = dict(GATE_OPTS, min_baseline=1e-30)


def tiny_baseline_cases():
    # rows 0, 1: one query position, train keypoints 0.25 apart; rows 2, 3: query keypoints 0.25 apart, one train position;
    # rows 4, 5: both sides coincide; rows 6 .. 9 carry the motion + (1, 1)
    q = [(0, 0), (0, 0), (8, 0), (8.25, 0), (0, 8), (0, 8), (20, 0), (24, 0), (20, 4), (24, 4)]
    t = [(50, 50), (50.25, 50), (90, 50), (90, 50), (50, 90), (50, 90), (21, 1), (25, 1), (21, 5), (25, 5)]
    dup = ([(3, 3)] * 5, [(7, 7)] * 5, [1, 2, 3, 4, 5])
    return [("duplicates in the pool", (q, t, np.arange(10) + 1.0), dict(hyp=(6, 7), n=4, c=1.0, s=0.0, tx=1.0, ty=1.0, rms=0.0, inlier=[0] * 6 + [1] * 4)),
            ("every sample a duplicate", dup, dict(hyp=None))]


def check_expected(rec, inlier, pairs, cases, what=""):
    """The hand-written outcomes of gate_cases() and its kin against REG_DTYPE records and inlier words."""
    V, N = capi.FX_REG_VALID, capi.FX_REG_NO_HYPOTHESIS
    for (name, case, want), r, (q0, qn, _, _) in zip(cases, rec, pairs):
        tag = f"{what} {name}"
        assert r["n_corr"] == len(case[0]), tag
        if want["hyp"] is None:
            assert r["flags"] == N and r["n_inliers"] == 0 and r["hyp_a"] == r["hyp_b"] == capi.FX_REG_NO_ROW and np.isposinf(r["rms"]), (tag, r)
            assert not inlier[q0:q0 + qn].any(), tag
            continue
        assert (r["hyp_a"] - q0, r["hyp_b"] - q0) == want["hyp"] and r["n_inliers"] == want["n"] and r["flags"] == V, (tag, r)
        assert r["tz"] == 0.5, (tag, r)
        for f in ("c", "s", "tx", "ty", "rms"):
            if f in want:
                assert r[f] == want[f], (tag, f, r)
        if "inlier" in want:
            assert inlier[q0:q0 + qn].tolist() == want["inlier"], tag


# -- family 2: power-of-two scaling
SCALE_SIZES = [200, 54, 30, 7, 3, 150, 0, 129, 128, 2]
SCALE_SEED = 31
SCALE_OPTS = dict(inlier_dist=0.25, min_baseline=2.0, hyp_corr=32)
K_BAND = (-36, 24)          # the exact band of SCALE_SEED, established by test_register_reference.py from the reference alone
K_BAND_GPU = [-36, -30, -16, -1, 1, 16, 24]
K_ZONES = list(range(-48, -36)) + list(range(25, 33))
K_FAR = [-144, -133, -126, -100, -70, -60, 60, 100, 120]  # (-133: every coordinate of the case is subnormal; -70: lq2, lt2, dot, crs are)


def scale_base():
    return multi_pair_case(np.random.default_rng(SCALE_SEED), SCALE_SIZES, outlier_share=0.4, sigma=0.04)


def scaled(base, k, opts=SCALE_OPTS):
    """The case and the two distances of the options times 2^k (ldexp: exact unless the result leaves float32's normal range)."""
    q, t, m, pairs = base
    q2, t2 = q.copy(), t.copy()
    with np.errstate(all="ignore"):
        q2[:, :3], t2[:, :3] = np.ldexp(q[:, :3], k), np.ldexp(t[:, :3], k)
        o = dict(opts, inlier_dist=float(np.ldexp(np.float32(opts["inlier_dist"]), k)), min_baseline=float(np.ldexp(np.float32(opts["min_baseline"]), k)))
    return q2, t2, m, pairs, o


def assert_scaled(got, base, k, what=""):
    """REG_DTYPE records of the case times 2^k against those of the case itself: integers equal, c and s the same bits, the
    translation and rms scaled exactly."""
    for f in ("n_corr", "n_inliers", "flags", "hyp_a", "hyp_b"):
        assert (got[f] == base[f]).all(), (what, k, f, np.flatnonzero(got[f] != base[f]))
    for f in ("c", "s"):
        assert (got[f].view(np.uint64) == base[f].view(np.uint64)).all(), (what, k, f)
    for f in ("tx", "ty", "tz", "rms"):
        u = np.uint64 if got[f].dtype.itemsize == 8 else np.uint32
        assert (got[f].view(u) == np.ldexp(base[f], k).view(u)).all(), (what, k, f)


def extreme_case():
    """Coordinates at +-3e38: every difference of unlike signs overflows, lq2 is +inf, sqrt - sqrt is NaN and the length gate
    lets the sample through."""
    rng = np.random.default_rng(32)
    q, t, m, pairs = multi_pair_case(rng, [40, 9, 2, 64])
    for x in (q, t):
        x[:, :2] = np.where(rng.random((len(x), 2)) < 0.5, np.float32(3e38), np.float32(-3e38))
    return q, t, m, pairs


# -- family 3: ties and the ends of the sample range
TIE_H = 128
TIE_SAMPLES = [(0, 1), (63, 64), (0, 255), (0, 256), (255, 256), (5, 8127), (4095, 4096)]
LAST_H = [2, 3, 64, 127, 128]
TIE_OPTS = dict(inlier_dist=0.25, min_baseline=2.0, hyp_corr=TIE_H, min_inliers=2)


def _junk(k):
    """A correspondence whose train side is three times its query side, far from every carrier: a sample that holds one fails
    the length gate (two of them: lt = 3 lq, lq >= 16; with a carrier: lq is about 1400 and lt about 4200)."""
    return (1000.0 + 16.0 * k, 1000.0), (3000.0 + 48.0 * k, 3000.0)


def _by_rank(n, carriers):
    """n correspondences, carriers = {pool rank: (q, t)}, junk at every other rank; dist2 = rank + 1, and the query rows run
    against the ranks (row = n - 1 - rank).  Returns (case, row_of_rank)."""
    by_rank = [carriers.get(r) or _junk(r) for r in range(n)]
    qxy, txy = [c[0] for c in by_rank[::-1]], [c[1] for c in by_rank[::-1]]
    return (qxy, txy, [float(n - r) for r in range(n)]), (lambda r: n - 1 - r)


def tie_case(i, j, third, H=TIE_H):
    """Samples i < j of a pool of H alive with 2 agreeing each (third: j with 3, its third carrier outside the pool), every other
    sample gated out.  H + 1 correspondences: the last rank is outside the pool.  Returns (case, expected)."""
    (ai, bi), (aj, bj) = ranks_of(H, i), ranks_of(H, j)
    shared = set((ai, bi)) & set((aj, bj))
    car = {}
    if not shared:  # two translations, as test_tie_goes_to_the_lowest_sample_of_pool_ranks
        car[ai], car[bi] = ((0, 0), (5, 5)), ((10, 0), (15, 5))
        car[aj], car[bj] = ((0, 40), (-7, 70)), ((17, 40), (10, 70))
        extra = ((30, 40), (23, 70))
    else:  # one member S in both: + (5, 5) with X, and a quarter turn about S, then + (5, 5), with Y
        s, = shared
        x, = set((ai, bi)) - shared
        y, = set((aj, bj)) - shared
        car[s], car[x], car[y] = ((0, 0), (5, 5)), ((10, 0), (15, 5)), ((0, 17), (-12, 5))
        extra = ((0, -20), (25, 5))
    car[H] = extra if third else None
    case, row = _by_rank(H + 1, car)
    w = (aj, bj) if third else (ai, bi)
    return case, dict(hyp=(row(w[0]), row(w[1])), n=3 if third else 2, rms=0.0)


def last_sample_case(H):
    """H correspondences, all in the pool; the only live sample is the last one, (H - 2, H - 1)."""
    case, row = _by_rank(H, {H - 2: ((0, 0), (5, 5)), H - 1: ((10, 0), (15, 5))})
    return case, dict(hyp=(row(H - 2), row(H - 1)), n=2, c=1.0, s=0.0, tx=5.0, ty=5.0, rms=0.0)


def tie_cases():
    out = [(f"tie {i} {j}", *tie_case(i, j, False)) for i, j in TIE_SAMPLES]
    out += [(f"three on {j} against two on {i}", *tie_case(i, j, True)) for i, j in TIE_SAMPLES]
    return out + [(f"last sample of {H}", *last_sample_case(H)) for H in LAST_H]


# -- family 4: the pool is ranked by dist2's BITS
W_POS = [0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x3f800000, 0x7f800000, 0x7f800001, 0x7fa00000, 0x7fc00000, 0x7fc00123, 0x7fffffff]
W_NEG = [0x80000000, 0x80000001, 0x807fffff, 0x80800000, 0xbf800000, 0xc2c80000, 0xff800000, 0xff800001, 0xffc00000, 0xffc00123, 0xffffffff]
BITS_H = [2, 7, 64]
RUN_WORD = {2: 0x00000001, 7: 0x7fc00123, 64: 0xbf800000}  # a subnormal, a quiet NaN with a payload, -1.0


def bits_opts(H):
    return dict(inlier_dist=0.25, min_baseline=2.0, hyp_corr=H, min_inliers=2)


def _scramble(n, seed):
    return np.random.default_rng(seed).permutation(n)


def bits_all_carriers(H):
    """Every correspondence carries + (1, 1) exactly and any two are 4 m or more apart: every sample has all agreeing, and the
    winner is the sample of pool ranks (0, 1) — the rows of the two lowest (bits, row).  The words are all of W_POS and W_NEG and
    + 0 and - 0 twice more; floats would rank - inf and the negative numbers first."""
    words = np.array(W_POS + W_NEG + [0x00000000, 0x80000000, 0x00000000, 0x80000000] + [0x40000000 + (k << 12) for k in range(H)], np.uint32)
    n = len(words)
    words = words[_scramble(n, 100 + H)]
    qxy = [(4.0 * (k % 16), 4.0 * (k // 16)) for k in range(n)]
    txy = [(x + 1, y + 1) for x, y in qxy]
    order = np.lexsort((np.arange(n), words))
    return (qxy, txy, words), dict(hyp=(int(order[0]), int(order[1])), n=n)


def bits_cut_case(H):
    """The cut at H falls inside a run of three equal words (RUN_WORD[H]) whose lowest row is a carrier; the pool's only other
    carrier has the lowest word of all, every other member of the pool is junk, and two more carriers have words that are last
    as bits and first, or nowhere, as floats (- inf, a negative NaN).  The one live sample is (0, H - 1)."""
    run = RUN_WORD[H]
    every = sorted(set(W_POS + W_NEG + [0x40000000 + (k << 12) for k in range(64)] + [0x80000002 + k for k in range(8)]))
    below = [w for w in every if w < run]
    above = [w for w in every if w > run and w not in (0xff800000, 0xffc00123)]
    inside = below[:1] + below[len(below) - (H - 2):] if H > 2 else below[:1]  # the lowest word, then the H - 2 just below the run
    assert len(inside) == H - 1 and len(set(inside)) == H - 1
    words = inside + [run] * 3 + above[:6] + [0xff800000, 0xffc00123]
    n = len(words)
    carrier = [False] * n
    for k in (0, H - 1, n - 2, n - 1):
        carrier[k] = True
    # rows: scrambled, but the run's carrier gets the lowest row of the three
    perm = list(_scramble(n, 200 + H))
    run_rows = sorted(perm[H - 1:H + 2])
    perm[H - 1:H + 2] = run_rows
    qxy, txy, d2 = [None] * n, [None] * n, np.zeros(n, np.uint32)
    spots = iter([((0, 0), (1, 1)), ((8, 0), (9, 1)), ((0, 8), (1, 9)), ((8, 8), (9, 9))])
    for k in range(n):
        qxy[perm[k]], txy[perm[k]] = next(spots) if carrier[k] else _junk(k)
        d2[perm[k]] = words[k]
    return (qxy, txy, d2), dict(hyp=(int(perm[0]), int(perm[H - 1])), n=4, c=1.0, s=0.0, tx=1.0, ty=1.0, rms=0.0)


def bits_cases(H):
    return [(f"bits, all carriers, H {H}", *bits_all_carriers(H)), (f"bits, the cut inside a run, H {H}", *bits_cut_case(H))]


# -- family 5: the refit's fallback.  Two correspondences whose lengths differ by the length gate: the hypothesis leaves both
# residuals at about inlier_dist, the first fit is the same transform in fp64, and rounding decides the re-test
FALLBACK_OPTS = dict(inlier_dist=0.25, min_baseline=2.0, hyp_corr=2, min_inliers=2)


def edge_pair(seed):
    """A two-correspondence pair at the length gate's edge, from a seed."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-20, 20, 2)
    L, th, ph = rng.uniform(3, 30), rng.uniform(0, 2 * math.pi), rng.uniform(0, 2 * math.pi)
    b = a + L * np.array([math.cos(th), math.sin(th)])
    ta = rng.uniform(-20, 20, 2)
    tb = ta + (L + 0.5) * np.array([math.cos(ph), math.sin(ph)])
    return ([tuple(a), tuple(b)], [tuple(ta), tuple(tb)], [1, 2])


FALLBACK_SEEDS = [15, 107, 132]  # the first three of seeds 0 .. 499 whose census shows the fallback (9 of the 500 do)
STAY_SEEDS = [0, 1, 2, 3]        # neighbours that do not: gated out, or the re-test keeps both


def fallback_cases():
    return [(f"edge pair {s}", edge_pair(s)) for s in FALLBACK_SEEDS + STAY_SEEDS]


def total(cen, key):
    return sum(c[key] for c in cen)
