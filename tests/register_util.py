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
