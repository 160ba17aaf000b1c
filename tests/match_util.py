"""Helpers of the descriptor-matching tests (tests/test_match_reference.py, tests/test_gpu_match.py,
tests/test_gpu_match_numerics.py): random sparse rows, the row families at fp32's edges, an exact d2, CSR blocks built on the
host, and the comparison of fx_match records with capi.match_reference under the rules of include/fx.h's error bound
eps = 2^-23 d2 + 2^-40 (|q|^2 + |t|^2) + 2^-150."""
from fractions import Fraction

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


F32_OVERFLOW = 2.0 ** 128 - 2.0 ** 103  # the least value that rounds to +inf in fp32: FLT_MAX plus half an ulp
FLT_MAX = float(np.finfo(np.float32).max)
W64 = np.float32(2.0 ** 64 * (1 - 2.0 ** -24))  # the largest fp32 word whose square is below FLT_MAX
_ONE = 1 << 149  # every finite fp32 value is an integer multiple of 2^-149


def round_f32(x):
    """A non-negative Fraction rounded once to fp32: to nearest, ties to even, subnormals kept, +inf from F32_OVERFLOW on."""
    x = Fraction(x)
    assert x >= 0
    if x == 0:
        return np.float32(0)
    e = x.numerator.bit_length() - x.denominator.bit_length()  # 2^(e-1) < x < 2^(e+1)
    if x < Fraction(2) ** e:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    r = round(x / quantum) * quantum  # (round() of a Fraction: ties to even)
    return np.float32(np.inf) if r >= 2 ** 128 else np.float32(float(r))


def exact_d2(q_row, t_row, s):
    """d2(q, t, s) of include/fx.h by its definition, one term at a time in integer arithmetic on the fp32 words (each an
    integer multiple of 2^-149): (the exact value as a Fraction, its correct rounding to fp32).  Finite rows only."""
    q = np.asarray(q_row, np.float32)[:BINS]
    t = np.roll(np.asarray(t_row, np.float32)[:BINS], -SECTOR * int(s))
    assert np.isfinite(q).all() and np.isfinite(t).all()
    acc = 0
    for c in np.flatnonzero((q != 0) | (t != 0)):
        (a, da), (b, db) = float(q[c]).as_integer_ratio(), float(t[c]).as_integer_ratio()
        d = a * (_ONE // da) - b * (_ONE // db)
        acc += d * d
    x = Fraction(acc, _ONE * _ONE)
    return x, round_f32(x)


# ---- row families at fp32's edges (tests/test_match_reference.py checks each one's conditions, tests/test_gpu_match_numerics.py
# runs them on the GPU).  Every builder returns (query rows, train rows, pairs, info).
def _copies(rng, t, src, s):
    return shift_rows(t[src], s)


def family_nonfinite(nan=False):
    """Ordinary rows, some of which store +Inf / -Inf (nan=True: NaN in the same places): in a bin of a query row, of a train
    row in each of the three train tiles, in both rows at a bin that meets under shift 2, and in an rf word.  info: the
    non-finite query rows and train rows, and the queries copied from a non-finite train row."""
    rng = np.random.default_rng(31)
    t = random_rows(rng, 130)
    src, s = rng.integers(0, 130, 64), rng.integers(0, 12, 64)
    src[[10, 11, 12, 13, 20]] = [5, 70, 129, 100, 40]
    s[20] = 2
    q = shift_rows(t[src], s)
    nz = q != 0
    q[nz] *= (1 + 0.01 * rng.standard_normal(int(nz.sum()))).astype(np.float32)
    pinf, ninf = (np.nan, np.nan) if nan else (np.inf, -np.inf)
    q[3, 77], q[9, 1979], q[30, 1983] = pinf, ninf, pinf
    t[5, 0], t[70, 1000], t[129, 500], t[100, 1985] = pinf, ninf, pinf, ninf
    c = 300
    t[40, c], q[20, (c - SECTOR * 2) % BINS] = pinf, pinf  # q[20][c'] meets t[40][c' + 165 * 2]: inf - inf
    t[41, c], q[21, c] = pinf, ninf
    return q, t, [(0, 64, 0, 130)], dict(q_bad=[3, 9, 20, 21, 30], t_bad=[5, 40, 41, 70, 100, 129], orphans=[10, 11, 12, 13])


def _one_word(n, bins, words):
    rows = np.zeros((n, capi.FX_DESC_FLOATS), np.float32)
    rows[np.arange(n), bins] = words
    return rows


def family_overflow():
    """Finite rows whose d2 reaches FLT_MAX.  Train rows 0..2: all zero, the word 2^64, the word 2^65; rows 3..89: one word of
    2^65 .. FLT_MAX (either sign), some with ordinary words beside it; rows 90..129: ordinary.  The huge words of the train rows
    sit at bins = 0..99 mod 165 and those of the query rows at 100..164 mod 165, so they never meet under a shift.  Pair 0 (query
    rows 0..7 against train rows 0..2): the words +-W64, whose d2 against the zero row is the largest finite one, then +-2^64,
    the next word above, 2^100 and +-FLT_MAX, whose d2 is +inf against every row.  Pair 1 (query rows 8..39 against train rows
    3..89, two tiles): every d2 is +inf.  Pair 2 (query rows 40..63 against train rows 90..129): rows 40..55 are noisy rotated
    copies of distinct train rows, rows 56..63 hold one word of 2^65 or more (+inf beyond doubt), so that finite and +inf records share one pair."""
    rng = np.random.default_rng(32)
    big = np.array([2.0 ** 65, -2.0 ** 65, 2.0 ** 90, FLT_MAX, -FLT_MAX, 2.0 ** 127], np.float32)
    t = random_rows(rng, 130, nnz=(0, 40))
    t[:3] = 0
    t[1, 165 * 3 + 7], t[2, 165 * 5 + 99] = 2.0 ** 64, 2.0 ** 65
    tb = 165 * rng.integers(0, 12, 87) + rng.integers(0, 100, 87)
    t[np.arange(3, 90), tb] = big[np.arange(87) % len(big)]
    t[90:] = random_rows(rng, 40)
    q = random_rows(rng, 64, nnz=(0, 40))
    q[:8], q[56:] = 0, 0
    qb = 165 * rng.integers(0, 12, 64) + rng.integers(100, 165, 64)
    q[np.arange(8), qb[:8]] = np.array([W64, -W64, 2.0 ** 64, -2.0 ** 64, 2.0 ** 100, FLT_MAX, -FLT_MAX, 2.0 ** 64 + 2.0 ** 41], np.float32)
    q[np.arange(8, 32), qb[8:32]] = big[np.arange(24) % len(big)]  # (rows 32..39 stay ordinary; row 39 is all zero)
    q[39] = 0
    src, s = 90 + rng.permutation(40)[:16], rng.integers(0, 12, 16)
    q[40:56] = shift_rows(t[src], s)
    nz = q[40:56] != 0
    q[40:56][nz] *= (1 + 0.01 * rng.standard_normal(int(nz.sum()))).astype(np.float32)
    q[np.arange(56, 64), qb[56:]] = np.array([2.0 ** 65, -2.0 ** 65, 2.0 ** 66, 2.0 ** 90, 2.0 ** 100, -2.0 ** 127, FLT_MAX, -FLT_MAX], np.float32)
    copies = list(range(40, 56))
    return q, t, [(0, 8, 0, 3), (8, 32, 3, 87), (40, 24, 90, 40)], dict(
        finite=[0, 1], copies=copies, src=src, s=s, all_inf=[i for i in range(2, 64) if i not in copies])


def family_cancellation():
    """Train rows of 1980 non-zero words in [2^8, 2^20); query row i is train row src[i] rotated by s[i] sectors with `moved[i]`
    of its words one ulp off.  Rows 0..7 are unmoved copies, the first four at shift 0."""
    rng = np.random.default_rng(33)
    t = np.zeros((130, capi.FX_DESC_FLOATS), np.float32)
    t[:, :BINS] = (2.0 ** rng.uniform(8, 20, (130, BINS))).astype(np.float32)
    src, s = rng.permutation(130)[:64], rng.integers(1, 12, 64)
    s[:4] = 0
    moved = np.array([0] * 8 + [1, 3, 40] * 18 + [1, 3])
    q = shift_rows(t[src], s)
    for i in range(64):
        c = rng.choice(BINS, moved[i], replace=False)
        q[i, c] = np.nextafter(q[i, c], np.where(rng.random(moved[i]) < 0.5, np.float32(0), np.float32(np.inf)).astype(np.float32))
    return q, t, [(0, 64, 0, 130)], dict(src=src, s=s, moved=moved)


def _tiny_rows(rng, n, scale_lo, scale_hi, mmax):
    """Rows of 3..8 words +-m 2^-k, m odd below mmax, k in [scale_lo, scale_hi]: few enough bits that every sum the matcher
    forms is exact in fp64."""
    rows = np.zeros((n, capi.FX_DESC_FLOATS), np.float32)
    for i in range(n):
        k = int(rng.integers(3, 9))
        m = (2 * rng.integers(0, mmax // 2, k) + 1) * rng.choice([-1, 1], k)
        rows[i, rng.choice(BINS, k, replace=False)] = (m * 2.0 ** -rng.integers(scale_lo, scale_hi + 1, k).astype(np.float64)).astype(np.float32)
    return rows


def family_underflow():
    """d2 in and below fp32's subnormal range.  Pair 0: rows of tiny normal words (+-m 2^-k, k = 60..70), query rows copies of
    train rows 0..99 with one word changed (rows 0..5: unchanged).  Pair 1: rows of subnormal words (+-m 2^-149): every d2 is
    below 2^-150 and rounds to +0.  Pair 2: the hand case, the single word 1.5 * 2^-74 against the zero row 128 (d2 = 4.5 *
    2^-149, a tie that rounds to the even 4 * 2^-149) and the word 2^-60 of row 129."""
    rng = np.random.default_rng(34)
    t = np.zeros((130, capi.FX_DESC_FLOATS), np.float32)
    t[:100] = _tiny_rows(rng, 100, 60, 70, 16)
    t[100:128] = _tiny_rows(rng, 28, 149, 149, 1024)
    t[129, 10] = 2.0 ** -60
    src, s = rng.permutation(100)[:48], rng.integers(0, 12, 48)
    q = np.zeros((64, capi.FX_DESC_FLOATS), np.float32)
    q[:48] = shift_rows(t[src], s)
    for i in range(6, 48):
        c = rng.choice(np.flatnonzero(q[i, :BINS]))
        q[i, c] += np.float32(2.0) * np.float32(2.0 ** -int(rng.integers(60, 71)))
    q[48:60] = _tiny_rows(rng, 12, 149, 149, 1024)
    q[60, 500] = 1.5 * 2.0 ** -74
    q[61, 500] = -1.5 * 2.0 ** -74
    return q, t, [(0, 48, 0, 100), (48, 12, 100, 28), (60, 2, 128, 2)], dict(src=src, s=s, hand=[60, 61])


def family_signs():
    """Words of both signs: noisy rotated copies of mixed-sign train rows, the exact negatives q = -t of train rows 0..3 (d2 = 4
    |t|^2 against their own row; the negation stores -0.0 in all their empty bins), and five -0.0 words stored in otherwise empty
    bins of every third row of both sides."""
    rng = np.random.default_rng(35)
    t = random_rows(rng, 130)
    t[t != 0] *= rng.choice(np.array([-1, 1], np.float32), int((t != 0).sum()))
    t[120:] = -np.abs(t[120:])  # all-negative rows
    src, s = rng.integers(0, 130, 64), rng.integers(0, 12, 64)
    q = shift_rows(t[src], s)
    nz = q != 0
    q[nz] *= (1 + 0.01 * rng.standard_normal(int(nz.sum()))).astype(np.float32)
    q[:4] = -t[:4]
    for rows in (q, t):
        for i in range(0, len(rows), 3):
            c = rng.choice(np.flatnonzero(rows[i, :BINS] == 0), 5, replace=False)
            rows[i, c] = -0.0
    return q, t, [(0, 64, 0, 130)], dict(src=src, s=s, negated=[0, 1, 2, 3])


def family_thresholds():
    """Records whose (dist2, dist2_second) are (0, 0), (0, finite), (finite, finite), (0, +inf), (finite, +inf) and (+inf, +inf):
    pair 0 has ordinary train rows 0..39 with row 1 a copy of row 0; pair 1 has the ordinary row 40 followed by rows 41..49 that
    hold FLT_MAX; pair 2 only such rows.  Zero distances are identical rows at shift 0."""
    rng = np.random.default_rng(36)
    t = random_rows(rng, 60)
    t[1] = t[0]
    t[np.arange(41, 60), 165 * rng.integers(0, 12, 19) + rng.integers(0, 100, 19)] = FLT_MAX
    src = rng.integers(2, 40, 30)
    q = np.zeros((48, capi.FX_DESC_FLOATS), np.float32)
    q[:30] = shift_rows(t[src], rng.integers(0, 12, 30))
    nz = q != 0
    q[nz] *= (1 + 0.04 * rng.standard_normal(int(nz.sum()))).astype(np.float32)
    q[24:30] = random_rows(rng, 6)               # rows without a partner: max_ratio splits them from the copies
    q[0], q[1], q[2] = t[0], t[5], t[9]          # (0, 0), (0, finite), (0, finite)
    q[30], q[31:36] = t[40], random_rows(rng, 5)  # (0, +inf), (finite, +inf)
    q[36:48] = random_rows(rng, 12)               # (+inf, +inf)
    return q, t, [(0, 30, 0, 40), (30, 6, 40, 10), (36, 12, 50, 10)], dict()


# the threshold options of the thresholds family: the CPU tests check what they cover, the GPU test runs them
THRESHOLDS = [dict(max_ratio=0.0), dict(max_ratio=-0.5), dict(max_ratio=0.5), dict(max_ratio=1.0), dict(max_ratio=1.5), dict(max_ratio=np.inf),
              dict(max_dist2=0.0), dict(max_dist2=np.inf), dict(max_dist2=0.0, max_ratio=0.0, mutual=True), dict(max_dist2=40.0, max_ratio=0.7, mutual=True)]


def ranking_keypoints(rec, pairs, hyp_corr, n_t):
    """Keypoint rows under which fx_register_matches' result for `pairs` of the match records `rec` shows which correspondences
    rank among the first hyp_corr by (dist2 bits, query row).  The train keypoints lie on a 3.5 m grid.  In every pair with more
    than hyp_corr + 1 finite-distance records, the records of rank hyp_corr - 2, hyp_corr - 1 and every finite one behind them
    follow one rigid motion; every other record's query keypoint lies somewhere far off.  The pool then holds exactly one sample
    of that motion, its last two members: the pair is valid with hyp_a, hyp_b those two rows and every follower an inlier, and a
    record ranked wrongly ahead of them pushes the sample out of the pool.  Returns (q_kp, t_kp, expected), expected[p] =
    (hyp_a, hyp_b, n_inliers), or None where the pair is too small for this hyp_corr or two followers share a train row."""
    rng = np.random.default_rng(37)
    j = np.arange(n_t)
    t_kp = np.zeros((n_t, 4), np.float32)
    t_kp[:, 0], t_kp[:, 1], t_kp[:, 2] = 3.5 * (j % 12) - 20, 3.5 * (j // 12) - 20, rng.uniform(-1, 3, n_t)
    q_kp = rng.uniform(-400, 400, (len(rec), 4)).astype(np.float32)
    c, s, tr = np.cos(0.2), np.sin(0.2), np.array([1.5, -0.7, 0.1])
    expected = []
    for q0, qn, _, _ in pairs:
        rows = q0 + np.flatnonzero(rec["train_row"][q0:q0 + qn] >= 0)
        order = rows[np.lexsort((rows, rec["dist2"][rows].view(np.uint32)))]
        finite = int(np.isfinite(rec["dist2"][rows]).sum())
        m = order[hyp_corr - 2:finite]  # (finite distances rank ahead of +inf)
        if not 2 <= hyp_corr < finite - 1 or len(set(rec["train_row"][m])) < len(m):  # (one train row twice: no baseline)
            expected.append(None)
            continue
        p = t_kp[rec["train_row"][m], :3].astype(np.float64) - tr  # the train keypoint moved back: q = R^T (t - tr)
        q_kp[m, 0], q_kp[m, 1], q_kp[m, 2] = c * p[:, 0] + s * p[:, 1], -s * p[:, 0] + c * p[:, 1], p[:, 2]
        expected.append((int(m[0]), int(m[1]), len(m)))
    return q_kp, t_kp, expected


FAMILIES = {"nonfinite": family_nonfinite, "overflow": family_overflow, "cancellation": family_cancellation,
            "underflow": family_underflow, "signs": family_signs, "thresholds": family_thresholds}
_CACHE = {}


def family(name, **kw):
    """(q, t, pairs, info, reference) of a family, built once and shared: read-only."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        q, t, pairs, info = FAMILIES[name](**kw)
        q.setflags(write=False), t.setflags(write=False)
        _CACHE[key] = (q, t, pairs, info, {})
    return _CACHE[key]


def family_reference(name, **opts):
    """capi.match_reference of a family under these options, computed once."""
    q, t, pairs, _, refs = family(name)
    key = tuple(sorted(opts.items()))
    if key not in refs:
        refs[key] = capi.match_reference(q, t, pairs, **opts)
    return refs[key]


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


def _pinned(d2, nq2, nt2):
    """Where the fp32 value of a reference d2 [q, t, s] is known exactly: every value within the fp64 stage's error (the bound
    without its rounding term) rounds to the same fp32 — distances so small that they round to +0, so large that they round to
    +inf — and, by the header's own clause, the exact 0 of identical rows at shift 0.  NaN entries are not pinned."""
    e = 2.0 ** -23 * d2 + 2.0 ** -40 * (nq2[:, None, None] + nt2[None, :, None])
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = np.maximum(d2 - e, 0.0).astype(np.float32), (d2 + e).astype(np.float32)
        pin = (lo.view(np.uint32) == hi.view(np.uint32)) & ~np.isnan(d2)
    if d2.shape[2]:
        pin[:, :, 0] |= d2[:, :, 0] == 0
    return pin


def _within(got, D, eps):
    """|got - D| <= eps, where a D that the bound lets reach fp32's overflow threshold may be reported as +inf."""
    return abs(float(got) - D) <= eps or (np.isposinf(got) and D + eps >= F32_OVERFLOW)


def _candidates_within(values, eps, live):
    """The live entries of `values` that their bounds `eps` cannot tell from the least live one: the gap is at most twice the sum
    of the two bounds (4 eps for rows of equal norm).  Infinite values are apart from everything, themselves included."""
    masked = np.where(live, values, np.inf)
    k = np.unravel_index(np.argmin(masked), masked.shape)
    with np.errstate(invalid="ignore"):
        return live & (values - masked[k] <= 2 * (eps + eps[k]))


def compare(got, ref, shifts=12, max_dist2=np.inf, max_ratio=1.0, mutual=False, require_all=False, what=""):
    """fx_match records `got` (MATCH_DTYPE) against match_reference's `ref`:
    - the reported dist2 is within eps of the reference d2 of the reported (train_row, shift), and that d2 within 2 eps of the
      reference minimum; where the reference's fp32 value is pinned (_pinned) or eps is not finite, dist2 equals it bit for
      bit; no dist2 or dist2_second has its sign bit set;
    - train_row, shift, second_row and the flags are equal wherever the reference gap exceeds twice the sum of the two
      candidates' eps (4 eps for rows of equal norm), or every candidate inside that gap has a pinned fp32 value, so that the
      header's tie order decides (a flag is also ambiguous when a threshold lies within 2 eps of a tested value that is not
      pinned);
    - rows without a match (no pair, clipped, non-finite, nothing to match) carry the sentinels exactly.
    require_all: no row may be ambiguous.  Returns the number of rows compared field by field."""
    want = ref["rec"]
    assert got.shape == want.shape, what
    assert (got["reserved"] == 0).all() and (got["pair"] == want["pair"]).all(), what
    assert not ((got["dist2"].view(np.uint32) | got["dist2_second"].view(np.uint32)) >> 31).any(), f"{what}: a negative distance"
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
        nt2_max = nt2[np.isfinite(nt2)].max() if np.isfinite(nt2).any() else 0.0  # (a non-finite row's norm is NaN or inf)
        nq2 = ref["nq2"][q0:q1]
        nq2_max = nq2[np.isfinite(nq2)].max() if np.isfinite(nq2).any() else 0.0
        pin = _pinned(d2, np.where(np.isfinite(nq2), nq2, 0.0), np.where(np.isfinite(nt2), nt2, 0.0))
        pin_t = pin.all(axis=2) | (pin[:, :, 0] & (d2[:, :, 0] == 0))  # the row's (dist2, shift) over the shifts is known
        f32_t = per_t.astype(np.float32)
        col_gap_ok = np.zeros(t1 - t0, bool)  # mutual: the train row's best query row is more than 4 eps ahead, or decided by pins
        if mutual:
            for j in range(t1 - t0):
                k = np.flatnonzero(np.isfinite(per_t[:, j]))
                c = per_t[k, j]
                if len(c) >= 2:
                    near = c - c.min() <= 4 * capi.match_epsilon(np.sort(c)[1], nq2_max, nt2[j])
                    col_gap_ok[j] = near.sum() == 1 or pin_t[k, j][near].all()
                else:
                    col_gap_ok[j] = True
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
            if pin[i, j, int(g["shift"])] or not np.isfinite(eps):
                assert g["dist2"].view(np.uint32) == np.float32(D).view(np.uint32), f"{tag}: dist2 is not the pinned {np.float32(D)}"
            else:
                assert _within(g["dist2"], D, eps), f"{tag}: dist2 off by {abs(float(g['dist2']) - D)} > eps {eps}"
            assert D - dmin <= 2 * eps, tag
            big = capi.match_epsilon(max(D, dmin), nq2, nt2_max)  # (the bound used for thresholds: the largest it can be here)
            live = ~np.isnan(d2[i])
            near = _candidates_within(d2[i], capi.match_epsilon(d2[i], nq2, nt2[:, None]), live)
            # A side without a non-zero bin has the same d2 at every shift: one candidate, at shift 0.  This relies on the
            # reference's fp32 values of such a row being equal at every shift, although it sums them in rolled order;
            # tests/test_match_reference.py asserts that for every family.
            near[(nt2 == 0) | (nq2 == 0), 1:] = False
            shift_clear = near.sum() <= 1 or bool(pin[i][near].all())
            rows_sorted = np.sort(per_t[i])
            E_t = capi.match_epsilon(per_t[i], nq2, nt2)
            near_t = np.flatnonzero(_candidates_within(per_t[i], E_t, live[:, 0]))
            row_clear = len(near_t) <= 1 or bool(pin_t[i, near_t].all())
            second_clear = row_clear
            if np.isfinite(rows_sorted[1:2]).any():
                big2 = capi.match_epsilon(rows_sorted[1], nq2, nt2_max)
                others = live[:, 0] & (np.arange(t1 - t0) != int(w["train_row"]) - t0)
                near_2 = np.flatnonzero(_candidates_within(per_t[i], E_t, others))
                second_clear = row_clear and (len(near_2) <= 1 or bool(pin_t[i, near_2].all()))
                # the second-best is a real other row, and its distance is that row's
                j2 = int(g["second_row"]) - t0
                assert 0 <= j2 < t1 - t0 and j2 != j, tag
                if pin_t[i, j2]:
                    assert g["dist2_second"].view(np.uint32) == f32_t[i, j2].view(np.uint32), tag
                else:
                    assert _within(g["dist2_second"], per_t[i, j2], capi.match_epsilon(per_t[i, j2], nq2, nt2[j2])), tag
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
            known = bool(pin_t[i, j])  # the tested values are known bit for bit: the thresholds decide as in the reference
            if np.isfinite(max_dist2) and not known:
                flags_clear = flags_clear and abs(D - max_dist2) > 2 * big
            if max_ratio < 1 and np.isfinite(rows_sorted[1:2]).any() and not (known and pin_t[i, int(g["second_row"]) - t0]):
                flags_clear = flags_clear and abs(D - ratio2 * rows_sorted[1]) > 2 * (big + ratio2 * big2)
            if flags_clear:
                assert (g["flags"] & capi.FX_MATCH_ACCEPTED) == (w["flags"] & capi.FX_MATCH_ACCEPTED), tag
            if mutual and row_clear and col_gap_ok[j]:
                assert (g["flags"] & capi.FX_MATCH_MUTUAL) == (w["flags"] & capi.FX_MATCH_MUTUAL), tag
            if not mutual:
                assert not g["flags"] & capi.FX_MATCH_MUTUAL, tag
            exact += bool(row_clear and shift_clear and second_clear)
    return exact
