"""fx_map_relocalize, the part that needs no GPU: the C-ABI's new names, and capi.map_relocalize_reference — the executable
statement of include/fx.h's definition — held to what the call exists for: scans given WITHOUT a pose come back at their pose in
the map's frame, a scan of a repeating pattern comes back AMBIGUOUS, and one pole off the pattern decides it."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from feature_extraction_amd import build, capi
from tests import map_localize_util as lu
from tests import map_relocalize_util as ru
from tests import map_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INLIER_DIST = 0.30


def test_names_declared_exported_and_listed(fxlib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fx.h")).read(), flags=re.S)
    for n in ("fx_relocalize_options", "fx_relocalization"):
        assert re.search(r"typedef struct %s\s*\{[^}]*\}\s*%s;" % (n, n), src), n
    for n in ("fx_relocalize_options_default", "fx_map_relocalize"):
        assert re.search(r"\b%s\s*\(" % n, src) and hasattr(fxlib, n) and n in capi.EXPORTS, n
    assert "#define FX_VERSION_MINOR 7" in src and fxlib.fx_version() == 7  # added symbols only
    for name, val in (("MAX_KP", 64), ("VALID", 1), ("TRUNCATED", 2), ("NO_HYPOTHESIS", 4), ("AMBIGUOUS", 8), ("NO_SCAN", 16)):
        m = re.search(r"#define FX_RELOC_%s\s+(\w+)u" % name, src)
        assert m and int(m.group(1), 0) == val == getattr(capi, "FX_RELOC_" + name), name
    assert C.sizeof(capi.FxRelocalizeOptions) == 40 and C.sizeof(capi.FxRelocalization) == 96 == capi.RELOC_DTYPE.itemsize
    assert "/* 96 B" in open(os.path.join(ROOT, "include", "fx.h")).read()
    assert [capi.RELOC_DTYPE.fields[f][1] for f in capi.RELOC_DTYPE.names] == [getattr(capi.FxRelocalization, f).offset for f in capi.RELOC_DTYPE.names]
    o = capi.FxRelocalizeOptions()
    fxlib.fx_relocalize_options_default(C.byref(o))
    got = {k: getattr(o, k) for k in capi.RELOC_DEFAULTS}
    assert got == {k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in capi.RELOC_DEFAULTS.items()} and o.reserved == 0
    assert capi.RELOC_DEFAULTS == dict(inlier_dist=0.30, pair_tol=0.30, min_baseline=2.0, max_baseline=60.0, max_seeds=16, min_inliers=4,
                                       min_margin=1, min_landmark_obs=2, segment=capi.FX_LOC_ANY_SEGMENT)
    assert "fx_map_relocalize.hip" in build.SOURCES


@pytest.fixture(scope="module")
def clean():
    w, pieces = lu.clean_world(0, 0.01)
    st, _, _ = mu.run_reference(pieces, lu.WORLD["cap"], lu.WORLD["carry"])
    return w, st, capi.map_relocalize_reference(st, w["off"], w["rows"], w["n_scans"])


def test_clean_world_every_scan_is_found_without_a_pose(clean):
    """40 poles at random positions, 24 scans, sigma 0.01 m.  Every scan is VALID; the pose of the one winning two-point
    hypothesis is within inlier_dist of the truth (each seed keypoint lands within pair_tol / 2 + noise of its pole, and the
    sensor is inside the scan's reach of 35 m of a seed at least 2 m long: what fx_map_localize then refines)."""
    w, st, ref = clean
    rec = ref["rec"]
    assert (rec["flags"] == ru.VALID).all(), rec["flags"]
    assert (rec["n_seeds"] == 16).all() and (rec["score"] >= 4).all() and (rec["n_hyp"] > 0).all()
    dxy, dz, dyaw = lu.pose_errors(rec["pose"], w["truth"])
    print(f"clean world: xy {dxy:.3g} m, z {dz:.3g} m, yaw {dyaw:.3g} rad; score {rec['score'].min()} .. {rec['score'].max()}, "
          f"runner_up up to {rec['runner_up'].max()}, n_hyp {rec['n_hyp'].min()} .. {rec['n_hyp'].max()}")
    assert dxy <= INLIER_DIST and dyaw <= math.radians(1.0)
    ids = ref["map_id_of_row"]
    assert ((ids >= 0).sum() == rec["score"].sum()) and (rec["pose"]["segment"] == 0).all()
    # the scored rows name their poles: one landmark stands for one pole
    pole_of = {}
    for r in np.flatnonzero(ids >= 0):
        assert pole_of.setdefault(int(ids[r]), int(w["pole"][r])) == int(w["pole"][r])


def test_lattice_is_ambiguous_and_one_pole_off_it_decides():
    frags, rows = ru.lattice_case(extra=False)
    off, kp = lu.scans([rows])
    rec = capi.map_relocalize_reference(ru.state_of(frags), off, kp, 1)["rec"][0]
    assert rec["flags"] == ru.AMBIG and rec["score"] == rec["runner_up"] == 9, rec
    frags, rows = ru.lattice_case(extra=True)
    off, kp = lu.scans([rows])
    ref = capi.map_relocalize_reference(ru.state_of(frags), off, kp, 1)
    rec = ref["rec"][0]
    assert rec["flags"] == ru.VALID and rec["score"] == 10 and rec["runner_up"] == 9, rec
    P = rec["pose"]
    assert abs(P["tx"] - 10.0) < 1e-5 and abs(P["ty"] - 3.0) < 1e-5 and abs(P["s"]) < 1e-6 and P["c"] > 0.999999 and P["tz"] == 0.0
    assert ref["map_id_of_row"].tolist() == ru.LATTICE["patch"] + [ru.LATTICE["n"]]


def test_scans_of_fewer_than_three_keypoints_have_no_hypothesis():
    """0 and 1 keypoints: no seed.  2 keypoints: one candidate pair at most; closer than min_baseline it is no seed, and of a length
    no landmark pair has (the lattice's lengths are 4, 5.66, 8, 8.94 ...: 6.5 m is 0.84 m from the nearest) every pair is gated out.
    Where the two DO match a landmark pair the definition's clause applies as written (a winner needs a score of 2): the scan has
    a winner of score 2, which min_inliers >= 3 keeps from ever being VALID."""
    frags = lu.lattice(16)
    full = lu.rows_at(frags, [0, 1, 2, 5, 6], 0.0)
    near, odd = [(0.0, 0.0, 1.0), (1.5, 0.0, 1.0)], [(0.0, 0.0, 1.0), (6.5, 0.0, 1.0)]
    off, kp = lu.scans([[], full[:1], near, odd, [(np.nan, 0.0, 1.0)] + odd, full[:2], full])
    ref = capi.map_relocalize_reference(ru.state_of(frags), off, kp, 8)
    rec = ref["rec"]
    assert rec["n_kp"].tolist() == [0, 1, 2, 2, 2, 2, 5, 0] and rec["n_seeds"].tolist() == [0, 0, 0, 1, 1, 1, 10, 0]
    assert rec["flags"].tolist() == [ru.NOHYP] * 5 + [0, ru.AMBIG, ru.NOSCAN], rec["flags"]
    assert rec["score"].tolist() == [0, 0, 0, 0, 0, 2, 5, 0] and rec["runner_up"][5] == 2 and (rec["n_hyp"][:5] == 0).all()
    for b in (0, 1, 2, 3, 4, 7):
        r = rec[b]
        assert (r["pose"]["c"], r["pose"]["s"], r["pose"]["tx"], r["pose"]["ty"], r["pose"]["tz"]) == (1.0, 0.0, 0.0, 0.0, 0.0)
        assert r["score"] == r["runner_up"] == r["n_hyp"] == 0 and r["seed_a"] == r["seed_b"] == r["lm_a"] == r["lm_b"] == capi.FX_RELOC_NONE
    assert (ref["map_id_of_row"] == -1).all()
    # no landmark at all: nothing to lay a seed on
    empty = capi.map_relocalize_reference(capi.map_state(8, 8), off, kp, 7)["rec"]
    assert (empty["flags"] == ru.NOHYP).all() and (empty["n_hyp"] == 0).all()


@pytest.mark.parametrize("name", sorted(ru.edge_cases()))
def test_gates_at_their_edges(name):
    frags, rows, opts, expect = ru.edge_cases()[name]
    off, kp = lu.scans(rows)
    ru.check_expect(capi.map_relocalize_reference(ru.state_of(frags), off, kp, len(rows), **opts), expect, name)


@pytest.mark.parametrize("name", ["rows_64_65", "seeds_16", "seeds_15", "seeds_14", "landmarks_256"])
def test_counts_at_their_edges(name):
    frags, rows, opts, expect = ru.count_cases()[name]
    off, kp = lu.scans(rows)
    ru.check_expect(capi.map_relocalize_reference(ru.state_of(frags), off, kp, len(rows), **opts), expect, name)
