"""fx_map_follow, the part that needs no GPU: the C-ABI's new names, and capi.map_follow_reference — the chain of include/fx.h's
definition in Python floats around capi.map_localize_reference — held to what the call exists for: a second drive with biased
odometry stays in the map scan after scan where its dead-reckoned priors lose it, over unusable links and over empty scans."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_follow_util as fu
from tests import map_localize_util as lu
from tests import map_merge_util as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALID, NOHYP, BADP, NOSCAN = capi.FX_LOC_VALID, capi.FX_LOC_NO_HYPOTHESIS, capi.FX_LOC_BAD_PRIOR, capi.FX_LOC_NO_SCAN
START, LINK, COASTED, HELD, LOST, NONE = fu.START, fu.LINK, fu.COASTED, fu.HELD, fu.LOST, fu.NONE
# (a)'s bounds: 3 x the worst error of the reference over the worlds of seeds 0, 1, 2 and 5 (sigma = 0.01 m, links 4 % long and
# turned 0.6 degrees), which is 0.00846 m in xy (seed 1) and 3.69e-4 rad (seed 0); 0.0254 m is below inlier_dist / 2 = 0.15 m
XY_BOUND, YAW_BOUND = 3 * 0.00846, 3 * 3.69e-4
N = lu.WORLD["n_scans"]


def test_names_declared_exported_and_listed(fxlib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fx.h")).read(), flags=re.S)
    for n in ("fx_follow_options", "fx_follow_scan"):
        assert re.search(r"typedef struct %s\s*\{[^}]*\}\s*%s;" % (n, n), src), n
    for n in ("fx_follow_options_default", "fx_map_follow"):
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(fxlib, n) and n in capi.EXPORTS, n
    assert "#define FX_VERSION_MINOR 7" in src and fxlib.fx_version() == 7  # added symbols only
    for name, val in (("START", 1), ("LINK", 2), ("COASTED", 4), ("HELD", 8), ("LOST", 16), ("NO_MOTION", 0xffffffff)):
        m = re.search(r"#define FX_FOLLOW_%s\s+(\w+)u" % name, src)
        assert m and int(m.group(1), 0) == val == getattr(capi, "FX_FOLLOW_" + name), name
    assert C.sizeof(capi.FxFollowOptions) == 48 and C.sizeof(capi.FxFollowScan) == 64 == capi.FOLLOW_DTYPE.itemsize
    assert capi.FxFollowOptions.loc.offset == 0 and capi.FxFollowOptions.chain_scans.offset == C.sizeof(capi.FxLocalizeOptions)
    assert [capi.FOLLOW_DTYPE.fields[f][1] for f in ("prior", "flags", "motion", "streak", "reserved")] == [0, 48, 52, 56, 60]
    o = capi.FxFollowOptions()
    fxlib.fx_follow_options_default(C.byref(o))
    got = {k: getattr(o.loc, k) for k in capi.LOC_DEFAULTS}
    got.update(chain_scans=o.chain_scans, require_flags=o.require_flags, max_lost=o.max_lost)
    assert got == {k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in capi.FOLLOW_DEFAULTS.items()}
    assert o.reserved == 0 and o.loc.reserved == 0
    l = capi.FxLocalizeOptions()
    fxlib.fx_localize_options_default(C.byref(l))
    same = [k for k in capi.LOC_DEFAULTS if getattr(o.loc, k) != getattr(l, k)]
    assert same == ["segment"] and o.loc.segment == capi.FX_LOC_ANY_SEGMENT and o.require_flags == capi.FX_REG_VALID and o.max_lost == 5


def test_the_seeds_are_the_well_spaced_worlds_below_six():
    assert fu.spaced_seeds(6) == fu.SEEDS


@pytest.fixture(scope="module", params=fu.SEEDS)
def driven(request):
    w, st, links, start = fu.world(request.param)
    assert st["header"]["segments"] == 1 and st["header"]["n_landmarks"] >= 30
    return request.param, w, st, links, start, capi.map_follow_reference(st, w["off"], w["rows"], links, start, N)


def test_a_biased_odometry_is_followed_where_dead_reckoning_is_lost(driven):
    """Measured: xy 0.0073, 0.0085, 0.0082, 0.0073 m and yaw 3.7e-4, 2.6e-4, 2.2e-4, 2.4e-4 rad on seeds 0, 1, 2, 5; the
    dead-reckoned priors end 6.13 m off and leave 10, 8, 17 and 10 of 24 scans VALID."""
    seed, w, st, links, start, out = driven
    rec, fol = out["rec"], out["follow"]
    assert (rec["flags"] == VALID).all(), rec["flags"]
    assert fol["flags"].tolist() == [START] + [LINK] * (N - 1) and fol["motion"].tolist() == [NONE] + list(range(N - 1))
    assert (fol["streak"] == 0).all() and (fol["reserved"] == 0).all()
    assert fol["prior"][0].tobytes() == start[0].tobytes() and out["poses"].tobytes() == rec["pose"].tobytes()
    dxy, dz, dyaw = lu.pose_errors(out["poses"], w["truth"])
    dead = fu.dead_reckoned(start[0], links, N)
    one = capi.map_localize_reference(st, w["off"], w["rows"], dead, N, segment=capi.FX_LOC_ANY_SEGMENT)
    n_valid = int((one["rec"]["flags"] & VALID != 0).sum())
    print(f"(a) seed {seed}: xy {dxy:.3g} m, z {dz:.3g} m, yaw {dyaw:.3g} rad; dead reckoning ends {lu.pose_errors(dead[-1:], w['truth'][-1:])[0]:.3g} m off, "
          f"{n_valid} of {N} VALID")
    assert n_valid < N
    assert XY_BOUND < fu.INLIER_DIST / 2
    assert dxy <= XY_BOUND and dyaw <= YAW_BOUND
    # a scan's prior is the pose before composed with its link: the follow of the scan alone from that pose
    b = 7
    r0, r1, r2 = (int(w["off"][k]) for k in (b - 1, b, b + 1))
    two = capi.map_follow_reference(st, np.array([0, r1 - r0, r2 - r0], np.uint32), w["rows"][r0:r2], links[b - 1:b], fol["prior"][b - 1:b], 2)
    assert two["follow"]["prior"][1].tobytes() == fol["prior"][b].tobytes() and two["rec"]["pose"][1].tobytes() == rec["pose"][b].tobytes()


def test_b_two_unusable_links_are_coasted_over(driven):
    seed, w, st, links, start, whole = driven
    bad = links.copy()
    bad["flags"][[9, 10]] = 0
    out = capi.map_follow_reference(st, w["off"], w["rows"], bad, start, N)
    fol = out["follow"]
    assert fol["flags"].tolist() == [START] + [LINK] * 9 + [COASTED] * 2 + [LINK] * 12
    assert fol["motion"][[10, 11]].tolist() == [8, 8] and fol["motion"][12] == 11
    assert (out["rec"]["flags"] == VALID).all()
    dxy, _, dyaw = lu.pose_errors(out["poses"], w["truth"])
    assert dxy <= XY_BOUND and dyaw <= YAW_BOUND
    assert out["rec"][:10].tobytes() == whole["rec"][:10].tobytes(), "the scans in front of the bad links are as without them"
    nan = links.copy()
    nan["tx"][9], nan["c"][10] = np.nan, np.inf  # (VALID records that are not finite are unusable as well)
    again = capi.map_follow_reference(st, w["off"], w["rows"], nan, start, N)
    assert again["follow"].tobytes() == fol.tobytes() and again["rec"].tobytes() == out["rec"].tobytes()
    trunc = capi.map_follow_reference(st, w["off"], w["rows"], links, start, N, require_flags=capi.FX_REG_VALID | capi.FX_REG_TRUNCATED)
    assert (trunc["follow"]["flags"] & np.uint32(0xffffffff ^ LOST)).tolist() == [START] + [HELD] * (N - 1), "no link carries FX_REG_TRUNCATED: nothing to coast on"


def test_c_empty_scans_keep_their_priors_and_the_chain_recovers(driven):
    seed, w, st, links, start, whole = driven
    off, rows = fu.without_rows(w, (5, 6, 7))
    out = capi.map_follow_reference(st, off, rows, links, start, N, max_lost=3)
    rec, fol = out["rec"], out["follow"]
    assert fol["streak"].tolist() == [0] * 5 + [1, 2, 3] + [0] * 16
    assert (rec["flags"][[5, 6, 7]] == NOHYP).all() and (np.delete(rec["flags"], [5, 6, 7]) == VALID).all()
    for b in (5, 6, 7):
        assert out["poses"][b].tobytes() == fol["prior"][b].tobytes(), "a scan without a fix stays at its prior"
    assert [b for b in range(N) if fol["flags"][b] & LOST] == [7] and fol["flags"][7] == LINK | LOST and fol["flags"][8] == LINK
    assert lu.pose_errors(fol["prior"][5:8], w["truth"][5:8])[0] < 1.0, "three links of biased odometry stay within search_dist"
    dxy, _, dyaw = lu.pose_errors(np.delete(out["poses"], [5, 6, 7]), [t for b, t in enumerate(w["truth"]) if b not in (5, 6, 7)])
    assert dxy <= XY_BOUND and dyaw <= YAW_BOUND
    default = capi.map_follow_reference(st, off, rows, links, start, N)
    assert not (default["follow"]["flags"] & LOST).any() and default["rec"].tobytes() == rec.tobytes()


def test_d_chain_edges(driven):
    seed, w, st, links, start, whole = driven
    L = 5
    starts = lu.poses_of([w["truth"][f] for f in range(0, N, L)])
    starts["segment"], starts["flags"] = np.arange(len(starts)) + 2, capi.FX_POSE_GAP
    wild = links.copy()
    wild["tx"][4], wild["ty"][4] = 500.0, -500.0  # (link 4 joins the last scan of chain 0 to the first of chain 1: never read)
    out = capi.map_follow_reference(st, w["off"], w["rows"], wild, starts, N, chain_scans=L)
    fol = out["follow"]
    assert [b for b in range(N) if fol["flags"][b] & START] == [0, 5, 10, 15, 20]
    assert fol["prior"][5].tobytes() == starts[1].tobytes() and out["rec"]["flags"][5] == VALID
    assert fol["prior"]["segment"].tolist() == [2 + b // L for b in range(N)] and fol["prior"]["flags"].tolist() == [capi.FX_POSE_GAP if b % L == 0 else 0 for b in range(N)]
    parts = fu.separate_chains(st, w["off"], w["rows"], wild, starts, N, L)
    assert [len(p["rec"]) for p in parts] == [5, 5, 5, 5, 4]
    off = [int(x) for x in w["off"]]
    for j, p in enumerate(parts):
        f, e = j * L, min(j * L + L, N)
        assert p["rec"]["pose"].tobytes() == out["rec"]["pose"][f:e].tobytes() and p["follow"]["prior"].tobytes() == fol["prior"][f:e].tobytes()
        assert (p["follow"]["flags"] == fol["flags"][f:e]).all() and (p["follow"]["streak"] == fol["streak"][f:e]).all()
        assert (p["map_id_of_row"] == out["map_id_of_row"][off[f]:off[e]]).all() and (p["nearest_of_row"] == out["nearest_of_row"][off[f]:off[e]]).all()
        for k in ("dc", "ds", "dtx", "dty", "dtz", "rms", "n_corr", "n_inliers", "flags"):
            assert p["rec"][k].tobytes() == out["rec"][k][f:e].tobytes(), k
    for big in (N, N + 1, 0xffffffff):
        one = capi.map_follow_reference(st, w["off"], w["rows"], links, start, N, chain_scans=big)
        assert all(one[k].tobytes() == whole[k].tobytes() for k in ("rec", "follow", "poses", "map_id_of_row", "nearest_of_row")), big


# ---- (e) special priors, on a hand-built map (map_merge_util.fragments: two identical observations each, z = 1)
LAT = lu.lattice(16)  # 4 x 4, 4 m apart
SCAN = lu.rows_at(LAT, [0, 1, 2, 5, 6, 9], 0.1)


def _lattice_state():
    st, ids = mm.reference_of(mm.fragments(LAT, 3))
    assert ids == list(range(len(LAT)))
    return st


def _still(n, **fields):
    """n links that move nothing."""
    r = np.zeros(n, capi.REG_DTYPE)
    r["c"], r["flags"] = 1.0, capi.FX_REG_VALID
    for k, v in fields.items():
        r[k] = v
    return r


def test_e_a_start_that_is_not_finite_is_held_through_the_chain():
    st = _lattice_state()
    off, rows = lu.scans([SCAN] * 4)
    start = lu.identity(1, segment=7, flags=capi.FX_POSE_GAP)
    start["ty"] = np.frombuffer(np.uint64(0xfff8dead0000beef).tobytes(), np.float64)[0]  # (a NaN with a payload and a sign)
    out = capi.map_follow_reference(st, off, rows, _still(3), start, 4)
    assert out["rec"]["flags"].tolist() == [BADP] * 4 and out["follow"]["flags"].tolist() == [START] + [HELD] * 3
    assert all(out["follow"]["prior"][b].tobytes() == start[0].tobytes() == out["poses"][b].tobytes() for b in range(4))
    assert out["follow"]["streak"].tolist() == [1, 2, 3, 4] and (out["follow"]["motion"] == NONE).all()
    assert (out["nearest_of_row"] == -1).all() and (out["map_id_of_row"] == -1).all()


def test_e_a_composition_that_overflows_is_held():
    st = _lattice_state()
    off, rows = lu.scans([SCAN] * 3)
    start = lu.identity(1, tx=1e308)
    links = _still(2)
    links["tx"][0] = 1e308
    out = capi.map_follow_reference(st, off, rows, links, start, 3)
    fol = out["follow"]
    assert fol["flags"].tolist() == [START, HELD, LINK] and fol["motion"].tolist() == [NONE, NONE, 1]
    assert fol["prior"][1].tobytes() == start[0].tobytes() and np.isfinite(fol["prior"]["tx"]).all()
    assert out["rec"]["flags"].tolist() == [NOHYP] * 3
    links["flags"][1] = 0  # link 0 is usable (its composition was not finite): the chain coasts on it, and is held again
    out = capi.map_follow_reference(st, off, rows, links, start, 3)
    assert out["follow"]["flags"].tolist() == [START, HELD, HELD] and out["follow"]["prior"][2].tobytes() == start[0].tobytes()


def test_e_an_unusable_first_link_is_held_and_later_ones_coast():
    st = _lattice_state()
    off, rows = lu.scans([SCAN] * 5)
    links = _still(5, tx=0.05)
    links["flags"][[0, 2, 3]] = 0  # (link 4 is usable and leads beyond the block's scans)
    out = capi.map_follow_reference(st, off, rows, links, lu.identity(1), 6, max_lost=1)
    fol = out["follow"]
    assert fol["flags"].tolist() == [START, HELD, LINK, COASTED, COASTED, HELD | LOST] and fol["motion"].tolist() == [NONE, NONE, 1, 1, 1, NONE]
    assert out["rec"]["flags"].tolist() == [VALID] * 5 + [NOSCAN] and fol["streak"].tolist() == [0] * 5 + [1]
    assert fol["prior"][1].tobytes() == out["poses"][0].tobytes() and fol["prior"][5].tobytes() == out["poses"][4].tobytes() == out["poses"][5].tobytes()
    assert abs(fol["prior"]["tx"][2] - (out["poses"]["tx"][1] + 0.05)) < 1e-12
    with pytest.raises(ValueError):
        capi.map_follow_reference(st, off, rows, links, lu.identity(1), 5, max_lost=0)
    with pytest.raises(ValueError):
        capi.map_follow_reference(st, off, rows, links, lu.identity(1), 5, require_flags=8)
    with pytest.raises(ValueError):
        capi.map_follow_reference(st, off, rows, None, lu.identity(1), 5)
    with pytest.raises(TypeError):
        capi.map_follow_reference(st, off, rows, links, lu.identity(1), 5, gate=1.0)
    single = capi.map_follow_reference(st, off, rows, None, lu.identity(5), 5, chain_scans=1)
    assert single["follow"]["flags"].tolist() == [START] * 5 and (single["rec"]["flags"] == VALID).all()
