"""What makes the scenes of tests/test_gpu_desc_edges.py able to fail, checked on the CPU (tests/desc_edges_util.py): every probe
reaches the float its table claims, by the numpy statement; the twins of a family land in different bins / counts; the oracle's
rows equal the statement's bit for bit, kp_neighbors included; the cell-border claims of family G hold; and the caps on equality
probes (which edges cannot be reached) are enumerated, not measured."""
import numpy as np
import pytest

from tests import desc_edges_util as eu

KINDS = ("x", "ztop", "zbot", "f", "z0", "xr")
SUPPORT = {"xr": 32}  # (R = 0.5 m: the pole's own twelve points are support points)
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _rows(kind, support, skip_epsilon=False):
    """(pole, what, probes, first, scan, oracle result, the statement's row) of every row of the kind's scenes."""
    p, scenes = eu.scenes(kind, support)
    for scan, ora, where in scenes:
        if skip_epsilon:
            from oracle import oracle_py
            ora = oracle_py.run(p, scan, policy=oracle_py.POLICY_SKIP_EPSILON)
        for pole, what, pr, first in where:
            yield pole, what, pr, first, scan, ora, eu.statement(scan[:, :3], pole.kp, pole.xa, pole.radius, skip_epsilon)


@pytest.mark.parametrize("kind", KINDS)
def test_probes_reach_their_floats_and_the_oracle_is_the_statement(oracle, kind):
    n = 0
    for pole, what, pr, first, scan, ora, st in _rows(kind, SUPPORT.get(kind, 16)):
        tag = f"{kind} pack {what} (ordinal {pole.ordinal})"
        eu.check_row(pole, what, pr, first, scan, st, tag)
        names = {q["name"]: q["xyz"] for q in pr}
        for i, q in enumerate(pr):
            at = eu.probe_index(kind, pr, first, i) if not (kind == "f" and i == 0) else None
            for what_q, v in q["claim"].items():
                if what_q == "mutual_d2":
                    got = eu.sqdist(names[q["pair"][0]][None], q["xyz"])[0]
                elif at is None:
                    got = eu.quantities(pole.kp, pole.xa, q["xyz"])[what_q][0]
                else:
                    got = st["q"][what_q][at]
                assert _bits(got) == _bits(v) or (got == v == 0), f"{tag}: probe {q['name']} claims {what_q} = {v!r}, the statement computes {got!r}"
            n += 1
        k = pole.ordinal
        assert int(ora["kp_neighbors"][k]) == st["n_nbr"], f"{tag}: kp_neighbors {ora['kp_neighbors'][k]}, the statement counts {st['n_nbr']}"
        bad = np.flatnonzero(_bits(ora["descriptors"][k, :1980]) != _bits(st["desc"]))
        assert len(bad) == 0, eu.explain(pole, what, pr, first, scan, ora["descriptors"][k], st["desc"], tag)
        assert not ora["descriptors"][k, 1980:].any()
    assert n >= 3


def test_twins_differ():
    """below / on / above are three different floats, and the decision differs between `on` and `above` (radial, elevation,
    azimuth) or between `below` and `on` (the gates)."""
    seen = set()
    for kind in KINDS:
        for row in eu.packs(kind)[1]:
            for pole, what, pr in row:
                by = {q["name"]: q for q in pr}
                for name, q in by.items():
                    if not name.endswith("on") and not name.endswith("on_n"):
                        continue
                    stem, tail = (name[:-2], "") if name.endswith("on") else (name[:-4], "_n")
                    lo, hi = by.get(stem + "below" + tail), by.get(stem + "above" + tail)
                    key = next(iter(q["claim"]))
                    if lo is not None:
                        assert lo["claim"][key] < q["claim"][key]
                    if hi is not None and stem != "C12":  # (the seam's other side starts again at 0)
                        assert q["claim"][key] < hi["claim"][key]
                    fam = q["family"]
                    if fam in "ABC" and hi is not None and not (fam == "A" and stem == "A15"):
                        assert q["expect"] != hi["expect"], name
                    if fam == "E":
                        assert lo is not None and hi is not None, name
                        assert lo["expect"][0] == "bin" and q["expect"] == hi["expect"] == ("out",)
                    if fam == "G" and lo is not None:
                        assert lo["pair"][1] == "below" and q["pair"][1] == "on"
                    seen.add(fam)
    assert {"A", "B", "C", "E", "G"} <= seen


@pytest.mark.parametrize("radius", [0.05, 0.1, 0.25, 0.3, 0.5, 1.0, 2.0])
def test_the_radial_fallback_is_unreachable(oracle, radius):
    """No float d2 < r2_search has sqrtf(d2) > radii[15]: `j == 15 -> 0` cannot be reached, at any radius the scenes could use."""
    f = eu.radial_facts(radius)
    assert not f["fallback_reachable"] and f["r_max"] <= f["edge15"], f


def test_all_fifteen_radial_edges_have_the_equality_probe(oracle):
    names = {q["name"] for row in eu.packs("x")[1] for _, what, pr in row if what == "A" for q in pr}
    assert {f"A{e}{s}" for e in range(1, 16) for s in ("below", "on", "above")} <= names and "A0inner" in names


def test_elevation_straddles_only_where_equality_is_out_of_reach(oracle):
    """An elevation edge without an `on` probe: no float tc within 64 of cos(edge) gives the edge.  Every edge has both sides, and
    they are the nearest values any tc gives."""
    theta = eu.tables()[1]
    by = {q["name"]: q for row in eu.packs("x")[1] for _, what, pr in row if what == "B" for q in pr}
    n_on = 0
    for e in range(1, 11):
        (lo, on, hi), (rlo, ron, rhi) = eu.theta_reachable(theta[e])
        assert by[f"B{e}below"]["claim"]["theta"] == lo < theta[e] < hi == by[f"B{e}above"]["claim"]["theta"]
        assert (f"B{e}on" in by) == (on is not None), f"edge {e}"
        if on is not None:
            assert ron is not None  # (some radian times 57.29578f is the edge)
            n_on += 1
        assert (on is not None) == (e >= 3), f"edge {e}"  # edges 1 and 2: tc steps theta over the edge; 3 .. 10: some tc gives it
        print(f"theta edge {e} ({theta[e]!r}): below {lo!r}, on {'yes' if on is not None else 'no'} "
              f"(a radian gives it: {'yes' if ron is not None else 'no'}), above {hi!r}")
    assert n_on >= 3


def test_azimuth_edges_have_both_sides_and_record_their_tries(oracle):
    found = {}
    for row in eu.packs("ztop")[1]:
        for pole, what, pr in row:
            if what != "C":
                continue
            names = {q["name"] for q in pr}
            for m, (hit, tries) in pole.phi_found.items():
                if m == 0:
                    continue
                assert {f"C{m}below", f"C{m}above"} <= names and (f"C{m}on" in names) == hit
                assert tries > 50000
                found.setdefault(pole.ordinal, {})[m] = hit
    assert set(found) == {0, 1} and all(set(v) == set(range(1, 13)) for v in found.values())  # every edge, on two x-axes
    print({o: sorted(m for m, h in v.items() if h) for o, v in found.items()})
    assert sum(h for v in found.values() for h in v.values()) >= 6


def test_pole_residue_search(oracle):
    """Straight above / below the keypoint the literal projection leaves no residue on these poles: bz - kp.z is exact when both
    lie within a factor of two of each other, so (bz - lambda) - kp.z is 0.  The count is recorded, not assumed."""
    for kind in ("ztop", "zbot"):
        pole = next(pole for row in eu.packs(kind)[1] for pole, what, _ in row if what == "D")
        n, tries = eu.residue_search(pole)
        print(f"{kind}: {n} of {tries} heights leave a residue")
        assert n == 0


@pytest.mark.parametrize("kind", ["x", "xr"])
def test_density_pairs_straddle_the_cells_they_claim(oracle, kind):
    by, pole_of = {}, {}
    for row in eu.packs(kind)[1]:
        for pole, what, pr in row:
            if what in ("Gcell", "Gdense"):
                for q in pr:
                    by[q["name"]], pole_of[q["name"]] = q, pole
    def delta(name, cell):
        pole = pole_of[name + "_n"]
        a, b = cell(pole.kp, by[name + "_n"]["xyz"], pole.radius), cell(pole.kp, by[name + "_p"]["xyz"], pole.radius)
        return pole, a, b, tuple(abs(x - y) for x, y in zip(a, b))
    pole, a, b, d = delta("Gcell_obelow", eu.list_grid_cell)
    o = int(np.argmax(np.abs(pole.out)))
    assert d[o] == 1, (a, b)
    for ax in "xyz":
        if f"Gcell_{ax}below_n" in by:
            assert delta(f"Gcell_{ax}below", eu.list_grid_cell)[3]["xyz".index(ax)] == 1
    assert delta("Gcell_allbelow", eu.list_grid_cell)[3] == (1, 1, 1)
    others = [i for i in range(3) if i != o]
    _, a, b, _ = delta("Gcell_firstbelow", eu.list_grid_cell)
    assert a[others[0]] == b[others[0]] == 0
    _, a, b, _ = delta("Gcell_lastbelow", eu.list_grid_cell)
    assert a[others[0]] == b[others[0]] == 10
    for side in ("below", "on"):
        assert delta(f"Gdense_x{side}", eu.dense_grid_cell)[3][0] == 2
        assert delta(f"Gdense_y{side}", eu.dense_grid_cell)[3][1] == 2
        assert delta(f"Gdense_z{side}", eu.dense_grid_cell)[3][2] == 1


def test_skip_rule_twins_move_under_the_epsilon_reading(oracle):
    """Exactly the probes with d2 in [FLT_MIN, FLT_EPSILON) change from binned to skipped; the oracle's switch agrees."""
    moved = []
    for pole, what, pr, first, scan, ora, st in _rows("f", 16, skip_epsilon=True):
        eu.check_row(pole, what, pr, first, scan, st, "f under the FLT_EPSILON reading", skip_epsilon=True)
        assert not (_bits(ora["descriptors"][pole.ordinal, :1980]) != _bits(st["desc"])).any()
        for q in pr:
            d2 = eu.quantities(pole.kp, pole.xa, q["xyz"])["d2"][0]
            assert (q["expect"] != q["expect_eps"]) == bool(eu.FLT_MIN <= d2 < eu.FLT_EPSILON), q["name"]
            moved += [q["name"]] if q["expect"] != q["expect_eps"] else []
    assert sorted(moved) == ["F_epsbelow", "F_tenth0", "F_tenth1"]


@pytest.mark.parametrize("kind", ["x", "xr"])
def test_the_pair_along_x_ends_the_chord(oracle, kind):
    """The dense pack's x pair lies along x to within 0.7 degrees at equal z: at the float below the gate the partner is the last
    point of the query's chord through its row of cells, on the gate the first point beyond it."""
    pole, pr = next((pole, pr) for row in eu.packs(kind)[1] for pole, what, pr in row if what == "Gdense")
    by = {q["name"]: q["xyz"].astype(np.float64) for q in pr}
    for side in ("below", "on"):
        d = by[f"Gdense_x{side}_p"] - by[f"Gdense_x{side}_n"]
        assert d[2] == 0 and abs(d[1]) < 0.0125 * abs(d[0]) and abs(abs(d[0]) - pole.radius / 5) < 1e-4 * pole.radius, (side, d)


def test_twin_pairs_have_different_densities(oracle):
    """The density the table states for the `below` member of a pair counts its partner, that of its `on` and `above` twins does
    not: the twins of family G differ in a count, not only in a label."""
    n = 0
    for kind in ("x", "xr"):
        support = SUPPORT.get(kind, 16)
        for scan, ora, where in eu.scenes(kind, support)[1]:
            for pole, what, pr, first in where:
                if eu.FAMILIES[what] != "G":
                    continue
                names = {q["name"]: q["xyz"] for q in pr}
                rho = dict(zip((q["name"] for q in pr), eu.rho_expected(pole, scan, pr, names)))
                alone = {nm: int((np.linalg.norm(scan[:, :3].astype(np.float64) - names[nm].astype(np.float64), axis=1) < pole.radius / 5 * 0.999).sum())
                         for nm in names}  # (the points clearly inside the density radius: without the gate partner)
                for nm, q in ((q["name"], q) for q in pr):
                    assert rho[nm] == alone[nm] + (1 if q["pair"][1] == "below" else 0), nm
                    n += q["pair"][1] == "below"
    assert n >= 20


@pytest.mark.parametrize("radius", [0.05, 0.1, 0.25, 0.3, 0.5, 1.0, 2.0])
def test_margins_that_no_probe_can_reach(oracle, radius):
    """Two margins of the device can change no result, so no wrong build of them can fail a scene; shown here instead.
    (1) r2_support's `+ 1e-4`: a density query of a neighbour N (|N| < R) counts P only if |P - N| < R / 5, so |P| < R + R / 5 in exact
    arithmetic; float32's d2 adds a relative 3e-7 at most (three roundings of 6e-8 on the squares' sum and one each on the
    differences).  The factor 1.0001 alone leaves a relative 1e-4 beyond R + R / 5, three hundred times that: with or without the
    `+ 1e-4` every countable P is a support point.
    (2) dense_grid's 1.001 / 1.0001 on `cw` and `ch`: two points closer than r_d are at most two cells apart in x and y iff
    r_d < 2 cw (one layer apart iff r_d < ch).  2 r_sup / 24 alone is 0.10001 R + 8e-6 > 0.1 R = r_d / 2 for every R (and
    2 r_sup / 6 > r_d), so without the margins r_d is at most 1.9998 cells; the cell index is floor((v - v0) * inv_cw) in float32
    with an error under 25 * 3 * 6e-8 = 5e-6 cells, far below the 3e-4 cells to spare."""
    rd = radius / 5.0
    rs_lean = (radius + rd) * 1.0001
    assert np.sqrt(np.float32(rs_lean * rs_lean)) > (radius + rd) * (1 + 3e-5)
    rs = rs_lean + 1e-4
    cw_lean, ch_lean = max(0.5 * rd, 2 * rs / 24), max(rd, 2 * rs / 6)
    assert rd / cw_lean < 2 - 1e-4 and rd / ch_lean < 1 - 1e-4
    # which branch of dense_grid's fmaxf gives cw: the support diameter's up to R = 0.1, the density radius's beyond (the "x"
    # and the "xr" scenes see one each); desc_body's 12^3 grid takes the diameter's at every R
    assert (2 * rs / 24 * 1.0001 > 0.5 * rd * 1.001) == (radius <= 0.1) and 2 * rs / 11 * 1.0001 > rd * 1.001


def test_skip_rule_at_flt_min(oracle):
    """dz = 2^-63 above a keypoint whose z is 0: d2 = FLT_MIN exactly, binned; the float below: a subnormal d2, skipped.  Under
    the FLT_EPSILON reading both are skipped."""
    for eps in (False, True):
        for pole, what, pr, first, scan, ora, st in _rows("z0", 16, skip_epsilon=eps):
            eu.check_row(pole, what, pr, first, scan, st, f"z0, epsilon reading {eps}", skip_epsilon=eps)
            assert not (_bits(ora["descriptors"][pole.ordinal, :1980]) != _bits(st["desc"])).any()
            at = {q["name"]: eu.probe_index("z0", pr, first, i) for i, q in enumerate(pr)}
            d2 = st["q"]["d2"]
            assert d2[at["F_min"]] == eu.FLT_MIN and 0 < d2[at["F_subnormal"]] < eu.FLT_MIN
            assert int(st["state"][at["F_min"]]) == (1 if eps else 2) and int(st["state"][at["F_subnormal"]]) == 1


def test_the_z_pairs_lie_in_two_target_windows(oracle):
    """The "xw" row (the dense grid's pairs in 20 000 support points), by the restated concatenation of k_dense_density's work
    item: more than two windows of 2048 targets, and for the z pair below the gate and the one on it the query's own cell lies
    wholly in one window and its partner's wholly in another.  The rows of 1025 support points have a single window."""
    (scan, ora, where), = eu.scenes("xw", eu.WINDOW_SUPPORT)[1]
    (pole, what, pr, first), = where
    st = eu.statement(scan[:, :3], pole.kp, pole.xa, pole.radius)
    eu.check_row(pole, what, pr, first, scan, st, "xw")
    assert not (_bits(ora["descriptors"][pole.ordinal, :1980]) != _bits(st["desc"])).any()
    t_tot, win = eu.dense_concatenation(pole, scan[:, :3])
    assert t_tot > 2 * eu.DENSE_WINDOW
    at = {q["name"]: eu.probe_index("x", pr, first, i) for i, q in enumerate(pr)}
    for side in ("below", "on"):
        n, p = win[at[f"Gdense_z{side}_n"]], win[at[f"Gdense_z{side}_p"]]
        assert n[0] == n[1] and p[0] == p[1] and n[0] != p[0], f"z pair {side}: windows {n} and {p}"
    for scan, ora, where in eu.scenes("x", 1025)[1]:
        for pole, what, pr, first in where:
            assert eu.dense_concatenation(pole, scan[:, :3])[0] <= eu.DENSE_WINDOW
