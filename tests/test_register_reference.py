"""Scan-to-scan rigid motion from descriptor matches, the part that needs no GPU: the C-ABI's new names and struct sizes, and
capi.register_reference — the numpy statement of include/fx.h's definition — on synthetic correspondences with known motion,
on every gate and sentinel, and at the end of the whole chain oracle -> match_reference -> register_reference."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import register_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACC, MUT = capi.FX_MATCH_ACCEPTED, capi.FX_MATCH_MUTUAL
VALID, TRUNC, NOHYP = capi.FX_REG_VALID, capi.FX_REG_TRUNCATED, capi.FX_REG_NO_HYPOTHESIS


def test_names_declared_exported_and_listed(fxlib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fx.h")).read(), flags=re.S)
    for n in ("fx_register_options", "fx_registration"):
        assert re.search(r"typedef struct %s\s*\{[^}]*\}\s*%s;" % (n, n), src), n
    for n in ("fx_register_options_default", "fx_register_matches"):
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(fxlib, n), n
        assert n in capi.EXPORTS, n
    assert "#define FX_VERSION_MINOR 7" in src and fxlib.fx_version() == 7  # added symbols only


def test_struct_sizes_and_default_options(fxlib):
    assert C.sizeof(capi.FxRegisterOptions) == 20 and C.sizeof(capi.FxRegistration) == 64 and capi.REG_DTYPE.itemsize == 64
    assert [f[0] for f in capi.FxRegistration._fields_] == list(capi.REG_DTYPE.names)
    assert [getattr(capi.FxRegistration, n).offset for n in capi.REG_DTYPE.names] == [capi.REG_DTYPE.fields[n][1] for n in capi.REG_DTYPE.names]
    o = capi.FxRegisterOptions(9.0, 9.0, 9, 9, 9)
    fxlib.fx_register_options_default(C.byref(o))
    got = (o.inlier_dist, o.min_baseline, o.hyp_corr, o.min_inliers, o.require_flags)
    assert got == (np.float32(0.30), 2.0, 64, 3, ACC)
    assert capi.REG_DEFAULTS == dict(inlier_dist=0.30, min_baseline=2.0, hyp_corr=64, min_inliers=3, require_flags=ACC)


def test_keypoint_block_parse_reads_what_the_pack_rule_writes():
    from feature_extraction_amd import sharding
    rng = np.random.default_rng(3)
    kps = [rng.standard_normal((n, 4)).astype(np.float32) for n in (5, 0, 7)]
    blk = sharding.pack_block(kps, [0, 1, 8], 6, 40)
    got = capi.keypoint_block_parse(blk, 6, 40)
    assert (got["scans"], got["keypoints"], got["flags_or"], got["max_total"]) == (3, 12, 9, 40)
    assert got["kp_offset"].tolist() == [0, 5, 5, 12] and got["flags"].tolist() == [0, 1, 8]
    assert (got["rows"].view(np.uint32) == np.concatenate(kps).view(np.uint32)).all()
    one, s, t = capi.keypoint_block_from_rows(kps[2], 1, 9)
    hdr, scans = sharding.unpack_block(one.view(np.float32).reshape(-1, 4), 1)
    assert hdr == dict(scans=1, keypoints=7, flags_or=0, max_total=9) and (scans[0][2] == kps[2]).all()


# ---- recovery of a known motion
def test_recovery_of_known_motion_under_noise_and_outliers():
    """60 scenes of 20..60 correspondences in a 100 m x 100 m field, sigma = 3 cm on every train coordinate, up to 60 % gross
    outliers.  The bound is the model's own: a consensus whose transform misplaces a point of the scene's far edge (its corners)
    by more than inlier_dist is a wrong consensus.  tz is the mean of at least 4 z differences whose only error is the train
    noise, sigma 3 cm: held to the same bound, 20 sigma of that mean."""
    rng = np.random.default_rng(20240)
    worst = 0.0
    corners = np.array([[50, 50], [50, -50], [-50, 50], [-50, -50]], np.float64)
    for scene in range(60):
        n, share = int(rng.integers(20, 61)), rng.uniform(0.0, 0.6)
        n_out = min(int(share * n), n - 4)
        yaw, t = rng.uniform(-0.5, 0.5), rng.uniform(-3, 3, 3)
        q, tr, true = ru.scene(rng, n, yaw, t, sigma=0.03, n_outliers=n_out)
        assert true.sum() >= 4
        ref = ru.run_reference(q, tr)
        r = ref["rec"][0]
        assert r["flags"] == VALID and r["n_corr"] == n, (scene, r)
        err = max(np.hypot(*(ru.apply(r, p) - ru.apply_truth(yaw, t, p))[:2]) for p in corners)
        worst = max(worst, err)
        assert err <= 0.30, (scene, err, r)
        assert abs(r["tz"] - t[2]) <= 0.30, (scene, r["tz"], t[2])
        assert r["n_inliers"] >= true.sum() - 1 and r["rms"] <= 0.30
        assert (ref["inlier"][true] == 1).sum() >= true.sum() - 1
        assert abs(math.hypot(r["c"], r["s"]) - 1) < 1e-15
        assert abs(capi.register_yaw(ref["rec"])[0] - yaw) <= 0.30 / 50
    print(f"worst far-edge error {worst * 100:.2f} cm")


# ---- gates and sentinels
def _sentinel(r, n_corr, extra=0):
    assert (r["c"], r["s"], r["tx"], r["ty"], r["tz"]) == (1.0, 0.0, 0.0, 0.0, 0.0) and np.isposinf(r["rms"]), r
    assert (r["n_corr"], r["n_inliers"], r["flags"], r["hyp_a"], r["hyp_b"]) == (n_corr, 0, NOHYP | extra, 0xffffffff, 0xffffffff), r


def test_zero_and_one_correspondence():
    rng = np.random.default_rng(1)
    q, t, _ = ru.scene(rng, 6, 0.1, (1, 2, 0))
    m = ru.records(6, np.arange(6))
    m["train_row"][:] = -1
    ref = capi.register_reference(q, t, m, [(0, 6, 0, 6)])
    _sentinel(ref["rec"][0], 0)
    m["train_row"][3] = 3
    ref = capi.register_reference(q, t, m, [(0, 6, 0, 6)])
    _sentinel(ref["rec"][0], 1)
    assert not ref["inlier"].any()
    # no pairs, empty sides, ranges beyond the records
    assert len(capi.register_reference(q, t, m, [])["rec"]) == 0
    ref = capi.register_reference(q, t, ru.records(6, np.arange(6)), [(0, 0, 0, 6), (2, 3, 0, 0), (6, 9, 0, 6), (0xfffffff0, 0x40, 0, 6)])
    _sentinel(ref["rec"][0], 0)
    _sentinel(ref["rec"][3], 0)
    _sentinel(ref["rec"][2], 0)
    _sentinel(ref["rec"][1], 0)  # (the records say pair 0)


def test_all_samples_below_min_baseline():
    rng = np.random.default_rng(2)
    q, t, _ = ru.scene(rng, 12, 0.2, (0.5, -1, 0.1), half=0.6)  # every point within 1.7 m of every other
    ref = ru.run_reference(q, t)
    _sentinel(ref["rec"][0], 12)
    ref = ru.run_reference(q, t, min_baseline=0.2)
    assert ref["rec"][0]["flags"] == VALID and ref["rec"][0]["n_inliers"] == 12


def test_two_queries_on_one_train_row():
    rng = np.random.default_rng(4)
    q, t, _ = ru.scene(rng, 10, -0.3, (2, 0, 0))
    rows = np.arange(10)
    rows[7] = 2  # query 7 claims train row 2 as well: it is an outlier like any other, both are used
    ref = ru.run_reference(q, t, train_rows=rows)
    r = ref["rec"][0]
    assert r["n_corr"] == 10 and r["n_inliers"] == 9 and r["flags"] == VALID
    assert ref["inlier"].tolist() == [1] * 7 + [0] + [1] * 2


def test_non_finite_coordinates_and_rows_beyond_the_stored_count_are_dropped():
    rng = np.random.default_rng(5)
    q, t, _ = ru.scene(rng, 14, 0.05, (0, 1, 0))
    q2, t2 = q.copy(), t.copy()
    q2[3, 1], t2[5, 2], q2[8, 2] = np.nan, np.inf, -np.inf
    ref = ru.run_reference(q2, t2)
    assert ref["corr"][0].tolist() == [0, 1, 2, 4, 6, 7, 9, 10, 11, 12, 13] and ref["rec"][0]["n_corr"] == 11
    assert ref["inlier"][[3, 5, 8]].tolist() == [0, 0, 0] and ref["rec"][0]["n_inliers"] == 11
    q3 = q.copy()
    q3[:, 3] = np.nan  # (the elevation word is not a coordinate)
    assert ru.run_reference(q3, t)["rec"][0]["n_corr"] == 14
    # the query block stores 12 rows, the train block 10: query rows 12.. and the matches into train rows 10.. are dropped
    rows = np.arange(14)
    rows[1] = 13
    ref = capi.register_reference(q[:12], t[:10], ru.records(14, rows), [(0, 14, 0, 14)])
    assert ref["corr"][0].tolist() == [0, 2, 3, 4, 5, 6, 7, 8, 9]


def test_require_flags_filtering():
    rng = np.random.default_rng(6)
    q, t, _ = ru.scene(rng, 10, 0.1, (0, 0, 0))
    m = ru.records(10, np.arange(10))  # ACCEPTED only
    _sentinel(capi.register_reference(q, t, m, [(0, 10, 0, 10)], require_flags=ACC | MUT)["rec"][0], 0)
    m["flags"][[0, 4, 5, 9]] |= MUT
    ref = capi.register_reference(q, t, m, [(0, 10, 0, 10)], require_flags=ACC | MUT)
    assert ref["corr"][0].tolist() == [0, 4, 5, 9] and ref["rec"][0]["n_inliers"] == 4
    m["flags"][4] = MUT  # not accepted
    assert capi.register_reference(q, t, m, [(0, 10, 0, 10)], require_flags=ACC | MUT)["corr"][0].tolist() == [0, 5, 9]
    assert capi.register_reference(q, t, m, [(0, 10, 0, 10)], require_flags=0)["rec"][0]["n_corr"] == 10
    m["pair"][2] = 1  # a record of another pair
    assert capi.register_reference(q, t, m, [(0, 10, 0, 10)], require_flags=0)["corr"][0].tolist() == [0, 1, 3, 4, 5, 6, 7, 8, 9]


def test_min_inliers_not_met_gives_the_transform_without_valid():
    rng = np.random.default_rng(7)
    q, t, true = ru.scene(rng, 9, 0.25, (1, -2, 0.5), n_outliers=6, sigma=0.0)
    ref = ru.run_reference(q, t, min_inliers=4)
    r = ref["rec"][0]
    assert r["flags"] == 0 and r["n_inliers"] == 3 and (ref["inlier"] == true).all()
    assert abs(math.atan2(r["s"], r["c"]) - 0.25) < 1e-5 and abs(r["tx"] - 1) < 1e-3 and abs(r["ty"] + 2) < 1e-3 and abs(r["tz"] - 0.5) < 1e-5
    assert ru.run_reference(q, t, min_inliers=3)["rec"][0]["flags"] == VALID
    for bad in (dict(hyp_corr=1), dict(hyp_corr=129), dict(min_inliers=1), dict(inlier_dist=0.0), dict(inlier_dist=np.inf),
                dict(min_baseline=-1.0), dict(min_baseline=np.nan)):
        with pytest.raises(ValueError):
            ru.run_reference(q, t, **bad)
    with pytest.raises(ValueError, match="overlap"):
        capi.register_reference(q, t, ru.records(9, np.arange(9)), [(0, 5, 0, 9), (4, 2, 0, 9)])


def test_truncation_uses_the_first_1024_in_query_row_order():
    rng = np.random.default_rng(8)
    q, t, _ = ru.scene(rng, 1100, 0.1, (1, 1, 0), sigma=0.02, n_outliers=300)
    d2 = rng.uniform(1, 100, 1100).astype(np.float32)
    full = ru.run_reference(q, t, d2=d2)
    head = ru.run_reference(q[:1024], t, d2=d2[:1024])
    a, b = full["rec"][0], head["rec"][0]
    assert a["flags"] == VALID | TRUNC and b["flags"] == VALID and a["n_corr"] == b["n_corr"] == 1024
    for f in capi.REG_DTYPE.names:
        if f != "flags":
            assert a[f].tobytes() == b[f].tobytes(), f
    assert (full["inlier"][:1024] == head["inlier"]).all() and not full["inlier"][1024:].any()
    assert not ru.run_reference(q[:1024], t[:1024])["rec"][0]["flags"] & TRUNC  # exactly 1024 is not truncated


def test_tie_goes_to_the_lowest_sample_of_pool_ranks():
    # two motions, each carried by exactly two correspondences 10 m apart; every mixed sample fails the length gate
    q = np.array([[0, 0, 0], [10, 0, 0], [0, 40, 0], [17, 40, 0]], np.float32)
    t = q.copy()
    t[:2, :2] += (5, 5)
    t[2:, :2] += (-7, 30)
    for d2, want in (([3, 4, 1, 2], (2, 3, 1.0, 0.0, -7.0, 30.0)), ([1, 2, 3, 4], (0, 1, 1.0, 0.0, 5.0, 5.0)), ([2, 1, 9, 9], (1, 0, 1.0, 0.0, 5.0, 5.0)),
                     ([5, 5, 5, 5], (0, 1, 1.0, 0.0, 5.0, 5.0))):  # (equal dist2: the query row decides the rank)
        ref = ru.run_reference(q, t, d2=np.array(d2, np.float32), min_inliers=2)
        r = ref["rec"][0]
        assert (r["hyp_a"], r["hyp_b"], r["c"], r["s"], r["tx"], r["ty"]) == want, (d2, r)
        assert r["n_inliers"] == 2 and r["flags"] == VALID and r["rms"] == 0
    # hyp_corr = 2: only the two best correspondences form a sample
    ref = ru.run_reference(q, t, d2=np.array([1, 9, 2, 9], np.float32), hyp_corr=2, min_inliers=2)
    _sentinel(ref["rec"][0], 4)  # (rows 0 and 2: a mixed sample)


def test_pairs_are_independent_and_may_come_in_any_order():
    rng = np.random.default_rng(9)
    q, t, m, pairs = ru.multi_pair_case(rng, [30, 0, 1, 54, 17, 2, 25])
    ref = capi.register_reference(q, t, m, pairs)
    assert (ref["rec"]["flags"] & VALID).sum() >= 4
    perm = [3, 0, 6, 5, 1, 4, 2]
    m2 = m.copy()
    inv = np.argsort(perm)
    has = m2["pair"] != capi.FX_MATCH_NO_PAIR
    m2["pair"][has] = inv[m2["pair"][has]]
    ref2 = capi.register_reference(q, t, m2, [pairs[k] for k in perm])
    assert ref2["rec"].tobytes() == ref["rec"][perm].tobytes() and (ref2["inlier"] == ref["inlier"]).all()
    # other pairs' records changed: pair 3's result stays
    m3 = m.copy()
    q0, qn = pairs[3][:2]
    other = np.ones(len(m), bool)
    other[q0:q0 + qn] = False
    m3["train_row"][other] = rng.integers(-1, len(t), int(other.sum()))
    m3["dist2"][other] = 0
    ref3 = capi.register_reference(q, t, m3, pairs)
    assert ref3["rec"][3].tobytes() == ref["rec"][3].tobytes() and (ref3["inlier"][q0:q0 + qn] == ref["inlier"][q0:q0 + qn]).all()


def test_identity_is_exact():
    rng = np.random.default_rng(10)
    q, _, _ = ru.scene(rng, 40, 0.0, (0, 0, 0))
    r = ru.run_reference(q, q.copy())["rec"][0]
    assert (r["c"], r["s"], r["tx"], r["ty"], r["tz"], r["rms"]) == (1.0, 0.0, 0.0, 0.0, 0.0, 0.0) and r["n_inliers"] == 40


# ---- the whole chain on the CPU
@pytest.mark.parametrize("deg", [3.0, -5.0])
def test_whole_chain_recovers_a_rotation_about_z(fxlib, oracle, deg):
    """A golden VLP-16 scan and the same scan rotated about z (fp64, rounded to fp32) through the oracle (no levelling: the two
    clouds then differ by exactly that rotation), match_reference, register_reference.  The query is the rotated scan, so the
    motion that takes it back onto the train scan is the opposite rotation and no translation."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "vlp16_launch_seed1000.npz"))
    A = np.concatenate([g["points_xyz"], np.zeros((len(g["points_xyz"]), 1), np.float32)], axis=1)
    th = math.radians(deg)
    B = A.copy()
    x, y = A[:, 0].astype(np.float64), A[:, 1].astype(np.float64)
    B[:, 0], B[:, 1] = (math.cos(th) * x - math.sin(th) * y).astype(np.float32), (math.sin(th) * x + math.cos(th) * y).astype(np.float32)
    p = capi.params("launch")
    oa, ob = oracle.run(p, A), oracle.run(p, B)
    assert oa["n_keypoints"] > 20 and ob["n_keypoints"] > 20
    pairs = [(0, ob["n_keypoints"], 0, oa["n_keypoints"])]
    m = capi.match_reference(ob["descriptors"], oa["descriptors"], pairs, mutual=True)["rec"]
    ref = capi.register_reference(ob["keypoints"], oa["keypoints"], m, pairs)
    r = ref["rec"][0]
    yaw = float(capi.register_yaw(ref["rec"])[0])
    err = abs(yaw + th) * 50.0 + math.hypot(r["tx"], r["ty"])
    print(f"{deg} deg: {r['n_corr']} correspondences, {r['n_inliers']} inliers, yaw {math.degrees(yaw):.4f} deg, t ({r['tx']:.4f}, {r['ty']:.4f}, {r['tz']:.4f}), "
          f"rms {r['rms']:.4f}, error at 50 m + translation {err:.4f} m")
    assert r["flags"] & VALID and err <= 0.30 and 2 * r["n_inliers"] >= r["n_corr"]


# ---- the gates at equality, ties, fp32's edges: the inputs of tests/test_gpu_register_numerics.py held to known answers here
def _family(cases, opts):
    q, t, m, pairs = ru.assemble([c[1] for c in cases])
    return (q, t, m, pairs), capi.register_reference(q, t, m, pairs, **opts), ru.census(q, t, m, pairs, **opts)


def test_gates_at_equality_keep_and_one_float_beyond_skips():
    cases = ru.gate_cases()
    _, ref, cen = _family(cases, ru.GATE_OPTS)
    ru.check_expected(ref["rec"], ref["inlier"], _[3], cases, "gates")
    c = {name: x for (name, _c, _w), x in zip(cases, cen)}
    four = np.float32(4.0)
    # each pair reaches the clause it is named for, on the side it is named for
    assert c["baseline q =="]["lq2"][0] == four and c["baseline q =="]["baseline_rejected"] == 0
    assert c["baseline q below"]["lq2"][0] == ru.up(4.0, -1) and c["baseline q below"]["lt2"][0] > four and c["baseline q below"]["baseline_rejected"] == 1
    assert c["baseline t =="]["lt2"][0] == four and c["baseline t =="]["baseline_rejected"] == 0
    assert c["baseline t below"]["lt2"][0] == ru.up(4.0, -1) and c["baseline t below"]["lq2"][0] > four and c["baseline t below"]["baseline_rejected"] == 1
    assert c["length =="]["diff"][0] == np.float32(0.5) and c["length =="]["length_rejected"] == 0
    assert c["length =="]["on_edge"].all() and c["length =="]["retest_on_edge"].all(), "both residuals are exactly inlier_dist, fp32 and fp64"
    assert c["length beyond"]["diff"][0] == np.float32(0.5 + 2.0 ** -21) and (c["length beyond"]["baseline_rejected"], c["length beyond"]["length_rejected"]) == (0, 1)
    a, b = c["agreement =="], c["agreement beyond"]
    assert a["on_edge"].tolist() == [False] * 4 + [True] and a["counts"][a["live"]].tolist() == [2, 3] and a["winner"] == ru.sample_of(5, 2, 3)
    assert not b["on_edge"].any() and b["counts"][b["live"]].tolist() == [2, 2] and b["live"].tolist() == a["live"].tolist() and b["winner"] == 0
    print("gates:", {n: (x["baseline_rejected"], x["length_rejected"], x["nrm_rejected"], x["max_count"]) for n, x in c.items()})


def test_the_retest_at_equality_and_one_float_beyond():
    cases = ru.retest_cases()
    inp, ref, cen = _family(cases, ru.RETEST_OPTS)
    ru.check_expected(ref["rec"], ref["inlier"], inp[3], cases, "re-test")
    assert cen[0]["retest_on_edge"].tolist() == [False] * 4 + [True] and not cen[0]["on_edge"].any() and cen[0]["max_count"] == 4
    assert not cen[1]["retest_on_edge"].any() and cen[1]["max_count"] == 4
    assert ref["rec"]["tx"][1] == 1.03125 and ref["rec"]["tx"][0] != 1.03125, "the second fit runs over five in the kept twin"


def test_a_min_baseline_whose_square_is_zero_leaves_only_nrm_positive():
    assert np.float32(1e-30) > 0 and np.float32(1e-30) * np.float32(1e-30) == 0
    cases = ru.tiny_baseline_cases()
    inp, ref, cen = _family(cases, ru.TINY_OPTS)
    ru.check_expected(ref["rec"], ref["inlier"], inp[3], cases, "tiny min_baseline")
    assert cen[0]["baseline_rejected"] == 0 and cen[0]["nrm_rejected"] == 3, "duplicate query rows, duplicate train rows, both"
    assert (cen[1]["baseline_rejected"], cen[1]["length_rejected"], cen[1]["nrm_rejected"]) == (0, 0, 10) == (0, 0, cen[1]["n_samples"])
    # with the default min_baseline the same pairs stop at the baseline gate
    q, t, m, pairs = inp
    assert ru.census(q, t, m, pairs, **ru.GATE_OPTS)[1]["baseline_rejected"] == 10


@pytest.fixture(scope="module")
def scale_base():
    base = ru.scale_base()
    return base, capi.register_reference(*base, **ru.SCALE_OPTS)["rec"]


def _scaled_reference(base, k):
    q, t, m, pairs, o = ru.scaled(base, k)
    return capi.register_reference(q, t, m, pairs, **o)["rec"], ru.census(q, t, m, pairs, **o)


def test_power_of_two_scaling_is_exact_inside_the_band(scale_base):
    """The band of the committed seed, by the reference alone: every k of K_BAND leaves the integers and the bits of c and s
    alone and scales tx, ty, tz and rms exactly."""
    base, r0 = scale_base
    assert ((r0["flags"] & VALID) != 0).sum() >= 7 and (r0["flags"] & NOHYP).any()
    lo, hi = ru.K_BAND
    assert lo <= -30 and hi >= 20 and set(ru.K_BAND_GPU) <= set(range(lo, hi + 1))
    for k in range(lo, hi + 1):
        ru.assert_scaled(_scaled_reference(base, k)[0], r0, k, "reference")


def test_the_transition_zones_and_far_out_reach_fp32s_edges(scale_base):
    base, r0 = scale_base
    seen = {z: dict(subnormal_nrm=0, nrm_zero_distinct=0, nrm_inf=0, cs_zero=0, mixed=0) for z in ("low", "high")}
    for k in ru.K_ZONES:
        rec, cen = _scaled_reference(base, k)
        z = seen["low" if k < 0 else "high"]
        for key in ("subnormal_nrm", "nrm_zero_distinct", "nrm_inf", "cs_zero"):
            z[key] += ru.total(cen, key)
        valid = (rec["flags"] & VALID) != 0
        z["mixed"] += int(valid.any() and (valid != ((r0["flags"] & VALID) != 0)).any())
    print("zones:", seen)
    assert seen["low"]["subnormal_nrm"] > 0 and seen["low"]["nrm_zero_distinct"] > 0 and seen["low"]["mixed"] > 0
    assert seen["high"]["nrm_inf"] > 0 and seen["high"]["cs_zero"] > 0 and seen["high"]["mixed"] > 0
    far = dict(nan_passed=0, cs_nonfinite=0, subnormal=0)
    for k in ru.K_FAR:
        rec, cen = _scaled_reference(base, k)
        assert (rec["flags"] == NOHYP).all(), k
        for key in far:
            far[key] += ru.total(cen, key)
    q, t, m, pairs, _ = ru.scaled(base, -133)
    assert (np.abs(q[:, :3]) < ru.TINY32).all() and (np.abs(t[:, :3]) < ru.TINY32).all() and (q[:, :2] != 0).any(), "subnormal coordinates"
    q, t, m, pairs = ru.extreme_case()
    ext = ru.census(q, t, m, pairs, **ru.SCALE_OPTS)
    assert (capi.register_reference(q, t, m, pairs, **ru.SCALE_OPTS)["rec"]["flags"] == NOHYP).all()
    print("far out:", far, "at +-3e38: nan_passed", ru.total(ext, "nan_passed"))
    assert far["nan_passed"] > 0 and far["cs_nonfinite"] > 0 and far["subnormal"] > 0 and ru.total(ext, "nan_passed") > 0


def test_ties_and_the_ends_of_the_sample_range():
    cases = ru.tie_cases()
    inp, ref, cen = _family(cases, ru.TIE_OPTS)
    ru.check_expected(ref["rec"], ref["inlier"], inp[3], cases, "ties")
    n = len(ru.TIE_SAMPLES)
    for (i, j), c in zip(ru.TIE_SAMPLES, cen[:n]):
        assert c["H"] == 128 and c["live"].tolist() == [i, j] and c["counts"][[i, j]].tolist() == [2, 2] and c["winner"] == i, (i, j)
    for (i, j), c in zip(ru.TIE_SAMPLES, cen[n:2 * n]):
        assert c["live"].tolist() == [i, j] and c["counts"][[i, j]].tolist() == [2, 3] and c["winner"] == j, (i, j)
    for H, c in zip(ru.LAST_H, cen[2 * n:]):
        assert c["H"] == H and c["live"].tolist() == [H * (H - 1) // 2 - 1] and c["max_count"] == 2, H
    assert all(ru.ranks_of(H, ru.sample_of(H, a, b)) == (a, b) for H in (2, 3, 128) for a in range(H) for b in range(a + 1, H))


@pytest.mark.parametrize("H", ru.BITS_H)
def test_the_pool_is_ranked_by_the_bits_of_dist2(H):
    cases = ru.bits_cases(H)
    inp, ref, cen = _family(cases, ru.bits_opts(H))
    ru.check_expected(ref["rec"], ref["inlier"], inp[3], cases, f"bits {H}")
    for (name, case, want), c in zip(cases, cen):
        assert c["n_corr"] > c["H"] == H and set(c["pool"]) != set(c["pool_float"]) and c["pool"][0] != c["pool_float"][0], name
    words = np.asarray(cases[1][1][2])
    cut = cen[1]
    run = np.flatnonzero(words == ru.RUN_WORD[H])
    assert len(run) == 3 and cut["pool"][H - 1] == run.min() and not set(run[1:]) & set(cut["pool"]), "the cut falls inside the run: its lowest row is in"
    assert cut["live"].tolist() == [ru.sample_of(H, 0, H - 1)] and cut["max_count"] == 4


def test_the_refit_falls_back_to_the_first_set():
    cases = ru.fallback_cases()
    q, t, m, pairs = ru.assemble([c[1] for c in cases])
    ref, cen = capi.register_reference(q, t, m, pairs, **ru.FALLBACK_OPTS), ru.census(q, t, m, pairs, **ru.FALLBACK_OPTS)
    k = len(ru.FALLBACK_SEEDS)
    assert [c["fallback"] for c in cen[:k]] == [True] * k and not any(c["fallback"] for c in cen[k:])
    rec = ref["rec"][:k]
    assert (rec["flags"] == VALID).all() and (rec["n_inliers"] == 2).all() and ref["inlier"][:2 * k].all()
    assert (np.abs(rec["rms"] - 0.25) < 1e-6).all(), "both residuals sit at inlier_dist"
