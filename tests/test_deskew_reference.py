"""capi.deskew_reference, the numpy / Python-float definition fx_deskew_keypoint_block is held to (tests/test_gpu_deskew.py), on
its own: the turn against numpy's arctangent, the clauses at their edges, and what the correction is for — a sensor that moves
during its sweep (tests/deskew_util.py), straight and on arcs, with exact motions and with the motions fx_register_matches's
reference finds on the skewed scans themselves."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import deskew_util as du
from tests import track_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_SCAN = capi.FX_DESKEW_PER_SCAN
K = capi.DESKEW_TURN_K
G1 = K[0] + (K[1] + (K[2] + (K[3] + (K[4] + K[5]))))  # the polynomial at a = 1 in the clause's order (the products by 1 are exact)


def _run(wd, motions, rows=None, **opts):
    """deskew_reference on a world's block -> (the first N rows of the keypoint area, the records, the block)."""
    blk, S, K = du.block(wd, rows=rows)
    dst, rec = capi.deskew_reference(blk, S, K, motions, wd["n_scans"], **opts)
    return du.block_rows(dst, S, K, len(wd["rows"])), rec, (blk, dst)


@pytest.fixture(scope="module")
def worlds():
    return {(v, w): du.world(v, w) for v, w in du.RUNS}


@pytest.fixture(scope="module")
def noisy():
    """Per run: the world with 2 cm of noise, the first register on its skewed rows, the de-skew by those links."""
    out = {}
    for v, w in du.RUNS:
        wd = du.world(v, w, sigma=0.02)
        r1 = du.register(wd, wd["rows"])
        rows, rec, _ = _run(wd, r1["rec"])
        out[(v, w)] = (wd, r1, rows, rec)
    return out


def test_constants_and_structs_are_the_headers(fxlib):
    src = open(os.path.join(ROOT, "include", "fx.h")).read()
    m = re.search(r"#define FX_DESKEW_TURN_K \{([^}]*)\}", src)
    assert m and tuple(float(x) for x in m.group(1).split(",")) == capi.DESKEW_TURN_K
    assert C.sizeof(capi.FxDeskewOptions) == 40 and C.sizeof(capi.FxDeskewScan) == 16 == capi.DESKEW_DTYPE.itemsize
    o = capi.FxDeskewOptions()
    fxlib.fx_deskew_options_default(C.byref(o))
    assert {k: getattr(o, k) for k in capi.DESKEW_DEFAULTS} == capi.DESKEW_DEFAULTS and o.reserved == 0
    for name in ("FX_DESKEW_LINKS", "FX_DESKEW_PER_SCAN", "FX_DESKEW_MOVED", "FX_DESKEW_NEXT_LINK", "FX_DESKEW_NO_MOTION", "FX_DESKEW_NO_SCAN"):
        assert int(re.search(rf"#define {name}\s+(0x[0-9a-f]+|\d+)u", src).group(1), 0) == getattr(capi, name), name


def test_turn_against_arctan2_in_all_octants():
    """At most 5e-7 of a turn from numpy.arctan2 on a dense grid of float32 directions of several lengths, and monotone along the
    circle (the octant seams included: the step there goes upwards)."""
    n = 200_000
    th = -math.pi + 2 * math.pi * (np.arange(n) + 0.5) / n
    for radius in (1.0, 37.5, 1e-3, 1e30):
        x, y = (radius * np.cos(th)).astype(np.float32).astype(np.float64), (radius * np.sin(th)).astype(np.float32).astype(np.float64)
        got = np.array([capi.deskew_turn(float(a), float(b)) for a, b in zip(x, y)])
        want = np.arctan2(y, x) / (2 * math.pi)
        err = np.abs(got - want)
        print(f"radius {radius}: largest error {err.max():.3g} of a turn")
        assert err.max() <= 5e-7, (radius, err.max())
        assert (np.diff(got) >= 0).all(), (radius, np.flatnonzero(np.diff(got) < 0)[:4])
        assert -0.5 < got.min() and got.max() <= 0.5


def test_turn_exact_values():
    t, den = capi.deskew_turn, float(np.float32(1e-45))
    assert abs(G1 - 0.12499974) < 1e-8
    g_half = 0.5 * (K[0] + 0.25 * (K[1] + 0.25 * (K[2] + 0.25 * (K[3] + 0.25 * (K[4] + 0.25 * K[5])))))  # a = 0.5
    for (x, y), want in (((1.0, 0.0), 0.0), ((0.0, 1.0), 0.25), ((-1.0, 0.0), 0.5), ((0.0, -1.0), -0.25),
                         ((1.0, 1.0), G1), ((-1.0, 1.0), 0.5 - G1), ((-1.0, -1.0), -(0.5 - G1)), ((1.0, -1.0), -G1),
                         ((0.0, 0.0), 0.0), ((-0.0, 0.0), 0.0), ((0.0, -0.0), 0.0), ((-0.0, -0.0), 0.0),
                         ((-0.0, 5.0), 0.25), ((5.0, -0.0), 0.0), ((-5.0, -0.0), 0.5), ((-0.0, -5.0), -0.25),
                         ((den, den), G1), ((den, -2 * den), -(0.25 - g_half)), ((1e30, 1e30), G1), ((-1e30, 1e30), 0.5 - G1),
                         ((1e30, den), (den / 1e30) * K[0]), ((-1e30, den), 0.5 - (den / 1e30) * K[0]), ((den, 1e30), 0.25 - (den / 1e30) * K[0])):
        got = t(x, y)
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), ((x, y), got, want)
    # the sweep fraction: clockwise from behind the sensor by default; u - floor(u) that rounds to 1 is 0
    assert capi.deskew_share(-10.0, 0.0) == (0.0, -1.0) and capi.deskew_share(10.0, 0.0) == (0.5, -0.5) and capi.deskew_share(0.0, 10.0)[0] == 0.25
    assert capi.deskew_share(0.0, 10.0, direction=1)[0] == 0.75 and capi.deskew_share(10.0, 0.0, start_turn=0.0, ref_fraction=0.0) == (0.0, 0.0)
    assert capi.deskew_share(10.0, 0.0, start_turn=1e-20, direction=1, ref_fraction=0.25, sweep_fraction=0.5) == (0.0, -0.125)


def test_identity_motions_give_the_block_back(worlds):
    wd = worlds[(15.0, 0.3)]
    ident = np.concatenate([du.motion_record(0.0, 0.0, 0.0) for _ in range(wd["n_scans"])])
    for src, m in ((PER_SCAN, ident), (capi.FX_DESKEW_LINKS, ident[:-1])):
        rows, rec, (blk, dst) = _run(wd, m, source=src)
        assert (blk == dst).all() and (rec["flags"] & capi.FX_DESKEW_MOVED).all() and (rec["max_shift"] == 0).all()
        assert rec["rows_moved"].tolist() == np.diff(wd["off"].astype(np.int64)).tolist()


def test_rows_at_the_reference_fraction_keep_their_bytes():
    """Every row of the block on the ray phi = 0.5 (ahead) or phi = 0 (behind) with ref_fraction the same: MOVED scans, nothing moved."""
    rng = np.random.default_rng(5)
    for sign, ref in ((1.0, 0.5), (-1.0, 0.0)):
        rows = np.zeros((6, 4), np.float32)
        rows[:, 0], rows[:, 2:] = sign * np.arange(1, 7), rng.uniform(-1, 1, (6, 2))
        blk = tu.block((0, 2, 6), rows, 3, 8)
        m = du.random_motions(rng, 2)
        dst, rec = capi.deskew_reference(blk, 3, 8, m, 2, source=PER_SCAN, ref_fraction=ref)
        assert (dst == blk).all() and rec["flags"].tolist() == [1, 1] and rec["rows_moved"].tolist() == [0, 0] and (rec["max_shift"] == 0).all()
        dst, rec = capi.deskew_reference(blk, 3, 8, m, 2, source=PER_SCAN, ref_fraction=0.25)  # (and elsewhere they do move)
        assert rec["rows_moved"].tolist() == [2, 4] and (du.block_rows(dst, 3, 8, 6)[:, 3] == rows[:, 3]).all()


def test_a_whole_period_is_the_motion_or_its_inverse_bit_for_bit():
    """w == 1: a row behind the sensor (phi = 0) stamped at the sweep's end moves by M's inverse, stamped at the start (ref 0, seen
    at phi = ... never 1) — and under direction +1 from start_turn 1e-20 the row ahead does; no interpolation touches it."""
    rng = np.random.default_rng(6)
    m = du.random_motions(rng, 1)
    c, s, tx, ty, tz = (float(m[f][0]) for f in ("c", "s", "tx", "ty", "tz"))
    rows = np.array([[-10, 0, 1, 0.1], [10, 0, 1, 0.1]], np.float32)
    blk = tu.block((0, 2), rows, 1, 2)
    dst, rec = capi.deskew_reference(blk, 1, 2, m, 1, source=PER_SCAN)
    gx, gy = -(c * tx + s * ty), (s * tx - c * ty)
    want = np.array([(c * -10.0 - -s * 0.0) + gx, (-s * -10.0 + c * 0.0) + gy, 1.0 + -tz], np.float64).astype(np.float32)
    got = du.block_rows(dst, 1, 2, 2)
    assert (tu.bits(got[0, :3]) == tu.bits(want)).all() and rec["rows_moved"][0] == 2
    shift = np.float32(math.sqrt((float(want[0]) + 10.0) ** 2 + float(want[1]) ** 2))
    assert rec["max_shift"][0] >= shift
    dst, rec = capi.deskew_reference(blk, 1, 2, m, 1, source=PER_SCAN, start_turn=1e-20, direction=1, ref_fraction=1.0)
    got = du.block_rows(dst, 1, 2, 2)  # (the row ahead: phi 0, a = -1)
    want = np.array([(c * 10.0 - -s * 0.0) + gx, (-s * 10.0 + c * 0.0) + gy, 1.0 + -tz], np.float64).astype(np.float32)
    assert (tu.bits(got[1, :3]) == tu.bits(want)).all()


@pytest.mark.parametrize("v", [15.0, 30.0])
def test_straight_runs_with_exact_motions(worlds, v):
    """Every corrected row within 3e-5 m of its pole under the true pose: four float32 half-ulps of 128 m over two coordinates,
    2.2e-5 m, plus the polynomial's sub-micrometre error.  Uncorrected they lie more than 0.3 m off."""
    wd = worlds[(v, 0.0)]
    assert np.abs(wd["rows"][:, :2]).max() < 128 and 42 <= np.diff(wd["off"].astype(np.int64)).min()
    rows, rec, _ = _run(wd, du.per_scan_motions(wd), source=PER_SCAN)
    raw, cor = du.under_true_pose(wd, wd["rows"][:, :2].astype(np.float64)), du.under_true_pose(wd, rows[:, :2].astype(np.float64))
    print(f"{v} m/s: uncorrected {raw.min():.3g} .. {raw.max():.3g} m, corrected at most {cor.max():.3g} m")
    assert raw.min() > 0.3 and cor.max() <= 3e-5, (raw.min(), cor.max())
    assert (rec["flags"] == capi.FX_DESKEW_MOVED).all() and (rec["motion"] == np.arange(wd["n_scans"])).all()
    assert abs(float(rec["max_shift"].max()) - raw.max()) < 1e-3
    # the links between the stamps are the same records: LINKS gives the same rows
    rows_l, rec_l, _ = _run(wd, du.link_motions(wd))
    assert (tu.bits(rows_l) == tu.bits(rows)).all() and rec_l["flags"].tolist() == [3] + [1] * (wd["n_scans"] - 1)


@pytest.mark.parametrize("run", [(15.0, 0.3), (8.0, 0.6)])
def test_arcs_against_the_exact_constant_twist(worlds, run):
    wd = worlds[run]
    rows, _, _ = _run(wd, du.per_scan_motions(wd), source=PER_SCAN)
    ex = du.exact_rows(wd)
    d = np.hypot(rows[:, 0] - ex[:, 0], rows[:, 1] - ex[:, 1])
    raw = du.under_true_pose(wd, wd["rows"][:, :2].astype(np.float64))
    print(f"{run}: at most {d.max():.4g} m from the exact correction (rows moved by up to {raw.max():.3g} m)")
    assert du.ARC_BOUND < 0.02 and d.max() <= du.ARC_BOUND and raw.max() > 1.0, (d.max(), raw.max())
    assert du.under_true_pose(wd, ex).max() < 1e-5  # (the closed form itself puts every row on its pole)


@pytest.mark.parametrize("run", du.RUNS)
def test_links_estimated_from_the_skewed_scans(noisy, run):
    """Register on the skewed scans (2 cm of noise), de-skew by its links, fit every corrected scan to the poles."""
    wd, r1, rows, rec = noisy[run]
    assert (r1["rec"]["flags"] & capi.FX_REG_VALID).all() and rec["flags"].tolist() == [3] + [1] * (wd["n_scans"] - 1)
    err_raw, share_raw = du.pose_fits(wd, wd["rows"][:, :2])
    err, share = du.pose_fits(wd, rows[:, :2])
    print(f"{run}: pose error {err_raw:.3g} -> {err:.3g} m, rows within 0.30 m of the fit {share_raw:.3g} -> {share:.3g}")
    assert err <= du.POSE_BOUND and share == 1.0, (err, share)
    if run == (15.0, 0.0):
        assert err_raw > 0.5, err_raw


@pytest.mark.parametrize("run", du.RUNS)
def test_a_second_register_is_not_worse(run):
    """Without noise a link's rms on the skewed scans is what the two scans' skews differ by; on the corrected block it may not be
    larger on any link.  (With 2 cm of noise the rms is the noise's, 0.04 m, and moves by a millimetre either way.)"""
    wd = du.world(*run)
    r1 = du.register(wd, wd["rows"])
    rows, _, _ = _run(wd, r1["rec"])
    r2 = du.register(wd, rows)
    print(f"{run}: rms {r1['rec']['rms'].max():.3g} -> {r2['rec']['rms'].max():.3g} m")
    assert (r2["rec"]["flags"] & capi.FX_REG_VALID).all() and (r2["rec"]["rms"] <= r1["rec"]["rms"]).all(), (r1["rec"]["rms"], r2["rec"]["rms"])
    assert (r2["rec"]["n_inliers"] >= r1["rec"]["n_inliers"]).all()


def test_link_choice():
    rng = np.random.default_rng(7)
    blk, S, K, off, rows = du.hand_case(rng)
    for what, m, n_scans, opts, flags in du.link_cases(rng):
        dst, rec = capi.deskew_reference(blk, S, K, m, n_scans, **opts)
        assert rec["flags"].tolist() == flags, (what, rec["flags"].tolist(), flags)
        got = du.block_rows(dst, S, K, len(rows))
        for b in range(n_scans):
            lo, hi = int(off[b]), int(off[b + 1])
            moved = bool(rec["flags"][b] & capi.FX_DESKEW_MOVED)
            assert (rec["motion"][b] != capi.FX_DESKEW_NO_RECORD) == moved and bool(rec["rows_moved"][b]) == (moved and hi > lo), (what, b)
            if not moved:
                assert (tu.bits(got[lo:hi]) == tu.bits(rows[lo:hi])).all() and rec["max_shift"][b] == 0, (what, b)
        assert (tu.bits(got[int(off[n_scans]):]) == tu.bits(rows[int(off[n_scans]):])).all(), what  # (scans >= S: copied)
        k0 = capi.keypoint_block_layout(S, K).k0
        assert (dst[:16 * k0] == blk[:16 * k0]).all() and (dst[16 * (k0 + len(rows)):] == blk[16 * (k0 + len(rows)):]).all(), what


def test_special_rows_and_edge_blocks():
    """NaN / inf rows are copied and not counted, a NaN elevation rides along, -0.0 is not below 0; tu.edge_blocks' headers."""
    rng = np.random.default_rng(8)
    blk, S, K, off, rows = du.hand_case(rng)
    m = du.random_motions(rng, 5)
    dst, rec = capi.deskew_reference(blk, S, K, m, 5, source=PER_SCAN)
    got = du.block_rows(dst, S, K, len(rows))
    lo = int(off[2])
    assert rec["rows_moved"].tolist() == [7, 0, 27, 5, 6] and rec["flags"].tolist() == [1] * 5  # (an empty scan still gets its record)
    assert (tu.bits(got[lo + 23:lo + 26]) == tu.bits(rows[lo + 23:lo + 26])).all()
    assert (tu.bits(got[:, 3]) == tu.bits(rows[:, 3])).all() and np.isfinite(got[lo + 26, :3]).all() and np.isfinite(got[lo + 19:lo + 23, :3]).all()
    sp = du.special_rows(rng)
    for k in range(0, 30, 5):
        for e in tu.edge_blocks(sp[k:k + 5]):
            for n_scans in (1, 2, 3):
                dst, rec = capi.deskew_reference(e["blk"], e["max_scans"], e["max_total"], du.random_motions(rng, 3), n_scans, source=PER_SCAN)
                assert len(rec) == n_scans and len(dst) == len(e["blk"]) and int(rec["rows_moved"].sum()) <= len(e["rows"]), e["what"]


def test_n_scans_above_and_below_the_blocks(worlds):
    wd = worlds[(8.0, 0.6)]
    blk, S, K = du.block(wd)  # (max_scans = scans + 2)
    m = du.random_motions(np.random.default_rng(9), S)
    dst, rec = capi.deskew_reference(blk, S, K, m, S, source=PER_SCAN)
    assert rec["flags"].tolist() == [1] * 9 + [8, 8] and (rec["motion"][9:] == capi.FX_DESKEW_NO_RECORD).all() and not rec["rows_moved"][9:].any()
    dst4, rec4 = capi.deskew_reference(blk, S, K, m, 4)
    assert rec4["flags"].tolist() == [3, 1, 1, 1]
    o4 = int(wd["off"][4])
    assert (du.block_rows(dst4, S, K, len(wd["rows"]))[o4:] == wd["rows"][o4:]).all() and (du.block_rows(dst4, S, K, o4)[:, :2] != wd["rows"][:o4, :2]).any()
    m["flags"][3] = 0
    assert capi.deskew_reference(blk, S, K, m, 4)[1]["flags"].tolist() == [3, 1, 1, 1]  # (S = 4 has the links 0 .. 2: record 3 is not read)
    m["flags"][2] = 0
    assert capi.deskew_reference(blk, S, K, m, 4)[1]["flags"].tolist() == [3, 1, 1, 4]  # (no link S - 1 stands in for the last scan)


def test_arguments_outside_the_call_raise():
    blk = tu.block((0, 1), np.ones((1, 4), np.float32), 2, 2)
    m = du.random_motions(np.random.default_rng(10), 2)
    for n_scans, opts in ((0, {}), (3, {}), (1, dict(start_turn=np.inf)), (1, dict(ref_fraction=-0.1)), (1, dict(ref_fraction=1.5)),
                          (1, dict(sweep_fraction=0.0)), (1, dict(sweep_fraction=1.1)), (1, dict(direction=0)), (1, dict(direction=2)), (1, dict(source=2))):
        with pytest.raises(ValueError):
            capi.deskew_reference(blk, 2, 2, m, n_scans, **opts)
    with pytest.raises(TypeError):
        capi.deskew_reference(blk, 2, 2, m, 1, speed=3)
