"""fx_map_observe on the GPU.  Every call of every case is compared with capi.map_observe_reference — an all-pairs statement of
include/fx.h's definition in numpy float64 that knows nothing of counts, cursors or a sort — bit for bit: the eight result words,
gained_of_landmark and observed_id_of_row whole, with guard words behind each, and the map's whole private state (header, records,
sums, alias, carry) through the snapshot: Map.export_state() against capi.map_snapshot_pack, byte for byte."""
import ctypes as C
import threading

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_compact_util as mc
from tests import map_localize_util as lu
from tests import map_merge_util as mm
from tests import map_observe_util as ou
from tests import track_util as tu
from tests.test_gpu_map import _run, _step
from tests.test_gpu_map_compact import _compact, _same_state
from tests.test_gpu_map_localize import _device
from tests.test_gpu_map_merge import _merge_to_fixpoint, _one_batch
from tests.test_gpu_track import FILL, GUARD

pytestmark = pytest.mark.gpu
ANY = capi.FX_LOC_ANY_SEGMENT
LOC_WORDS = capi.LOC_DTYPE.itemsize // 8


@pytest.fixture
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def _upload(ctx, c, n_scans, q, max_scans=None, max_total=None, stored=None, blk=None):
    """A case's block, records and table on the device: the records padded to n_scans with VALID identities, the table to q words
    with landmark 0 (a non-row's word must not matter).  blk: the block's bytes, laid out for max_scans and max_total, in the place
    of the one built from the case."""
    import torch
    dev = f"cuda:{ctx.device}"
    scans = len(c["off"]) - 1
    max_scans = max(scans, n_scans) + 2 if max_scans is None else max_scans
    max_total = len(c["rows"]) + 9 if max_total is None else max_total
    blk = tu.block(c["off"], c["rows"], max_scans, max_total, stored) if blk is None else blk
    loc = np.concatenate([c["loc"], ou.loc_records(max(0, n_scans - len(c["loc"])))])
    ids = np.concatenate([c["ids"], np.zeros(max(0, q - len(c["ids"])), np.int32)])
    return ((torch.from_numpy(blk).to(dev), max_scans, max_total), torch.from_numpy(loc.view(np.float64).reshape(-1, LOC_WORDS).copy()).to(dev),
            torch.from_numpy(ids).to(dev), loc, ids)


def _call(ctx, mp, kp, loc, ids, n_scans, q, optional=True, **opts):
    """Map.observe into guarded outputs.  Returns (result dict, gained, observed); without `optional` the two arrays are NULL (None)."""
    import torch
    dev = f"cuda:{ctx.device}"
    sizes = (8, mp.max_landmarks, q)
    raw = [torch.full((n + GUARD,), FILL, dtype=torch.int32, device=dev) for n in sizes]
    mp.observe(kp, loc, n_scans, ids, q_max_rows=q, out=raw[0][:8], gained=raw[1][:sizes[1]] if optional else False,
               observed=raw[2][:q] if optional else False, **opts)
    ctx.synchronize()
    for r, n, name in zip(raw, (8, sizes[1] if optional else 0, q if optional else 0), ("the result", "gained_of_landmark", "observed_id_of_row")):
        assert (r[n:] == FILL).all().item(), f"the guard behind {name}"
    return (capi.observe_records(raw[0][:8]), raw[1][:sizes[1]].cpu().numpy().astype(np.uint32) if optional else None,
            raw[2][:q].cpu().numpy() if optional else None)


def _observe(ctx, mp, st, c, what, n_scans=None, q_max_rows=None, stored=None, max_scans=None, max_total=None, dry_run=False, edge=None, **opts):
    """One fx_map_observe of a case against one map_observe_reference call, the map's state through the snapshot.  Returns (the
    reference's new state, (result, gained, observed)).  edge: one of tu.edge_blocks(c["rows"]) in the place of the case's block."""
    n_scans = len(c["off"]) - 1 if n_scans is None else n_scans
    q = len(c["rows"]) if q_max_rows is None else q_max_rows
    opts = dict(c["opts"], **opts)
    if edge:
        c, max_scans, max_total = dict(c, off=edge["off"], rows=edge["rows"]), edge["max_scans"], edge["max_total"]
    kp, loc_d, ids_d, loc, ids = _upload(ctx, c, n_scans, q, max_scans, max_total, stored, edge and edge["blk"])
    got = _call(ctx, mp, kp, loc_d, ids_d, n_scans, q, mode=capi.FX_OBS_DRY_RUN if dry_run else capi.FX_OBS_APPLY, **opts)
    off = c["off"][:min(len(c["off"]) - 1, kp[1]) + 1]
    new, *ref = capi.map_observe_reference(st, off, c["rows"][:len(c["rows"]) if stored is None else stored], loc, ids, n_scans, q_max_rows=q,
                                           dry_run=dry_run, **opts)
    ou.assert_outputs(got, ref, what)
    ou.assert_sums_to_proposed(got[0], what)
    _same_state(mp, new, what)
    return new, got


def _map_of(ctx, c, what, cap=None, carry=8):
    """The case's map on the device (track -> map, compared on the way); a state no run produces goes in through the import."""
    mp, st = _one_batch(ctx, mm.fragments(c["frags"], c["n_scans_map"]), what, cap=cap or len(c["frags"]), carry=carry)
    if c["edit"]:
        st = c["edit"](st)
        mp.import_state(capi.map_snapshot_pack(st))
    return mp, st


def _localized(ctx, mp, w, rows, priors, **opts):
    """fx_map_localize on the device; its outputs stay there.  Returns (kp, records, map_id_of_row): device tensors."""
    n = len(w["off"]) - 1
    kp, pri = _device(ctx, w["off"], rows, priors, n + 2, len(rows) + 9)
    recs, ids, _ = mp.localize(kp, pri, n, q_max_rows=len(rows), nearest=False, **opts)
    return kp, recs, ids


# ---- 1. the chain on the device
def test_01_localize_then_observe_with_no_host_read_between(ctx):
    w, pieces, rows = ou.renoised(0, 0.01, 4000)
    W = lu.WORLD
    S, q = W["n_scans"], len(rows)
    mp = ctx.map_create(W["cap"], W["carry"])
    st, _, _, _ = _run(ctx, pieces, "(1)", W["cap"], W["carry"], mp=mp)
    kp, recs, ids = _localized(ctx, mp, w, rows, lu.poses_of(w["truth"], seed=1000))
    got = _call(ctx, mp, kp, recs, ids, S, q)  # (reads the localise's outputs where they are)
    loc, table = capi.localize_records(recs), ids.cpu().numpy()
    assert (loc["flags"] == capi.FX_LOC_VALID).all()
    st1, *ref = capi.map_observe_reference(st, w["off"], rows, loc, table, S)
    ou.assert_outputs(got, ref, "(1)")
    _same_state(mp, st1, "(1)")
    res = got[0]
    assert res["scans_used"] == S and res["added"] == res["proposed"] == int((table >= 0).sum()) > 10 * S and res["landmarks_touched"] >= 30
    got2 = _call(ctx, mp, kp, recs, ids, S, q)  # the same table once more, on the changed map
    st2, *ref2 = capi.map_observe_reference(st1, w["off"], rows, loc, table, S)
    ou.assert_outputs(got2, ref2, "(1) a second observe")
    _same_state(mp, st2, "(1) a second observe")
    assert st2["header"]["n_obs"] == st["header"]["n_obs"] + res["added"] + got2[0]["added"]
    print("(1)", res, got2[0])
    mp.close()


# ---- 2. list lengths
def test_02_list_lengths_at_every_edge(ctx):
    c = ou.lists()
    mp, st = _map_of(ctx, c, "(2)")
    st, (res, gained, observed) = _observe(ctx, mp, st, c, "(2) lists")
    assert gained[:len(ou.COUNTS)].tolist() == ou.COUNTS and res["duplicates"] == 0 and res["added"] == sum(ou.COUNTS)
    assert [st["landmarks"][k]["n_obs"] for k in range(len(ou.COUNTS))] == [2 + n for n in ou.COUNTS]
    mp.close()


# ---- 3. landmark counts
def test_03_a_map_of_1100_all_observed_and_a_few_at_the_block_edges(ctx):
    BIG = lu.lattice(1100, pitch=3.0)
    rng = np.random.default_rng(93)
    every = [int(k) for k in rng.permutation(1100)]
    few = [0, 255, 256, 257, 1023, 1024, 1099]
    c = ou.case(BIG, [lu.rows_at(BIG, every, 0.05, -0.02), lu.rows_at(BIG, few, -0.03, 0.04)], every + few, loc=ou.loc_records(2, tx=(0.0, 0.015625)))
    mp, st = _map_of(ctx, c, "(3)", cap=1100)
    assert st["header"]["n_landmarks"] == 1100
    st, (res, gained, _) = _observe(ctx, mp, st, c, "(3) 1100")
    assert res["added"] == 1107 and res["landmarks_touched"] == 1100 and sorted(np.flatnonzero(gained == 2).tolist()) == few
    only = dict(c, off=np.array([0, 0, 7], np.uint32), rows=c["rows"][1100:], ids=c["ids"][1100:])
    st, (res, gained, _) = _observe(ctx, mp, st, only, "(3) seven of 1100")
    assert res["added"] == 7 and np.flatnonzero(gained).tolist() == few
    mp.close()


# ---- 4. duplicates and aliases
def test_04_duplicates_ties_and_ids_that_are_no_proposals(ctx):
    c = ou.duplicates()
    mp, st = _map_of(ctx, c, "(4) duplicates")
    st, (res, _, observed) = _observe(ctx, mp, st, c, "(4) duplicates")
    assert observed.tolist() == [-1, -1, 0, 1, 2, -1, -1, 5, 2, -1, 0, 1] and res["duplicates"] == 5
    mp.close()
    c = ou.garbage_ids()
    mp, st = _map_of(ctx, c, "(4) ids")
    st, (res, _, observed) = _observe(ctx, mp, st, c, "(4) ids")
    assert res["proposed"] == 1 and observed.tolist() == [-1] * 6 + [6, -1]
    mp.close()


def test_04_a_table_from_before_a_merge_and_from_before_a_compaction(ctx):
    w, pieces, _ = mm.flicker()
    f = mm.FLICKER
    mp = ctx.map_create(f["cap"], f["carry"])
    st, _, _, _ = _run(ctx, pieces, "(4)", f["cap"], f["carry"], mp=mp)
    kp, recs, ids = _localized(ctx, mp, w, w["rows"], lu.poses_of(w["truth"], seed=1072), segment=ANY)
    st, results = _merge_to_fixpoint(ctx, mp, st, "(4)", max_gap_scans=mc.GAP)
    assert sum(r["merged"] for r in results) > 0
    loc, table = capi.localize_records(recs), ids.cpu().numpy()
    c = dict(off=w["off"], rows=w["rows"], loc=loc, ids=table, opts={}, edit=None)
    alias = np.array(st["alias"])
    assert (alias[table[table >= 0]] >= 0).any(), "the table names absorbed landmarks"
    st, (res, gained, observed) = _observe(ctx, mp, st, c, "(4) after the merge")
    assert res["stale"] == 0 and (alias[observed[observed >= 0]] == -1).all() and not gained[:len(alias)][alias >= 0].any()
    mp.compact(remap=False, result=False)
    st, _, _ = capi.map_compact_reference(st)
    st, (res, gained, observed) = _observe(ctx, mp, st, c, "(4) after a compaction without remap")
    N = st["header"]["n_landmarks"]
    assert (table >= N).any() and (observed < N).all() and not gained[N:].any()
    mp.close()


def test_04_two_ids_of_one_root_are_deduplicated(ctx):
    c = ou.merged_twins()
    mp, st = _map_of(ctx, c, "(4) twins")
    st, _ = _merge_to_fixpoint(ctx, mp, st, "(4) twins")
    assert st["alias"] == [-1, -1, 0]
    st, (res, gained, observed) = _observe(ctx, mp, st, c, "(4) twins")
    assert observed.tolist() == [0, -1, 1, 0] and gained.tolist() == [2, 1, 0] and res["duplicates"] == 1
    mp.close()


def test_04_stale_records(ctx):
    c = ou.hand3()
    mp, st = _map_of(ctx, c, "(4) stale")
    st["landmarks"][1]["n_obs"] = 0  # (a record of no observation: its row, gated otherwise, is stale)
    mp.import_state(capi.map_snapshot_pack(st))
    st, (res, _, _) = _observe(ctx, mp, st, c, "(4) stale")
    assert tuple(res[k] for k in ou.RESULT) == (2, 5, 2, 1, 0, 2, 1)
    mp.close()


# ---- 5. the gate
def test_05_the_gate_at_its_edge_reads_the_record_the_call_starts_with(ctx):
    c = ou.gate_edge()
    mp, st = _map_of(ctx, c, "(5)")
    st, (res, gained, observed) = _observe(ctx, mp, st, c, "(5) d2 == gd gd")
    assert observed.tolist() == [0, -1, 0, -1, 0] and (res["added"], res["gated"]) == (3, 2) and gained.tolist() == [3, 0]
    st, (res, _, _) = _observe(ctx, mp, st, c, "(5) the default gate", gate_dist=0.30)
    assert (res["added"], res["gated"]) == (1, 4)
    mp.close()


# ---- 6. scan filters and sizes
def test_06_scan_filters_bad_rows_and_sizes(ctx):
    c = ou.filters()
    mp, st = _map_of(ctx, c, "(6)")
    st, (res, _, observed) = _observe(ctx, mp, st, c, "(6) VALID required")
    assert res["scans_used"] == 2 and observed.reshape(7, 3).tolist() == [[0, -1, 8]] + [[-1] * 3] * 5 + [[-1, 10, -1]]
    c = ou.filters(require_flags=0)
    st, (res, _, observed) = _observe(ctx, mp, st, c, "(6) require_flags 0")
    assert res["scans_used"] == 5 and (observed.reshape(7, 3)[4:6] == -1).all()
    st, (res, _, _) = _observe(ctx, mp, st, c, "(6) TRUNCATED required", require_flags=capi.FX_LOC_VALID | capi.FX_LOC_TRUNCATED)
    assert res["scans_used"] == 1
    n, rows = 7, len(c["rows"])
    st, _ = _observe(ctx, mp, st, c, "(6) scans beyond the block", n_scans=n + 2, max_scans=n + 2)
    st, _ = _observe(ctx, mp, st, c, "(6) max_scans scans", max_scans=n, max_total=rows)
    st, (res, _, _) = _observe(ctx, mp, st, c, "(6) fewer scans than the block", n_scans=3)
    assert res["scans_used"] == 3
    for q in (rows - 8, rows - 1, rows + 1, rows + 300):
        st, _ = _observe(ctx, mp, st, c, f"(6) q_max_rows {q}", q_max_rows=q)
    st, _ = _observe(ctx, mp, st, c, "(6) a block that stores fewer rows", stored=rows - 5)
    st, (res, _, _) = _observe(ctx, mp, st, c, "(6) no rows at all", q_max_rows=0)
    assert res == dict(zip(capi.MAP_OBSERVE_RESULT_FIELDS, (5, 0, 0, 0, 0, 0, 0, 0)))
    mp.close()
    # the edges only a hand-made block reaches, on a map of four landmarks: scans of 2, 0 and 3 rows, every row on its landmark
    frags = lu.lattice(4, pitch=7.0)
    four = ou.case(frags, [lu.rows_at(frags, [0, 1], 0.02), [], lu.rows_at(frags, [1, 2, 3], -0.03, 0.01)], [0, 1, 1, 2, 3])
    mp, st = _map_of(ctx, four, "(6) a map of four")
    for edge in tu.edge_blocks(four["rows"]):
        st, (res, _, observed) = _observe(ctx, mp, st, four, f"(6) {edge['what']}", edge=edge)
        assert res["scans_used"] == 3 and res["added"] == len(edge["rows"]) and observed.tolist() == [0, 1, 1, 2, 3][:res["added"]] + [-1] * (5 - res["added"])
    mp.close()
    empty = ctx.map_create(8, 8)
    _, (res, gained, observed) = _observe(ctx, empty, capi.map_state(8, 8), c, "(6) an empty map")
    assert res["proposed"] == 0 and res["scans_used"] == 5 and not gained.any() and (observed == -1).all()
    empty.close()


# ---- 7. the dry run
def test_07_a_dry_run_reports_everything_and_changes_no_byte(ctx):
    for make in (ou.duplicates, ou.lists):
        c = make()
        mp, st = _map_of(ctx, c, "(7)")
        twin, _ = _map_of(ctx, c, "(7) the twin")
        before = mp.export_state()
        assert twin.export_state() == before
        _, dry = _observe(ctx, mp, st, c, "(7) dry", dry_run=True)
        assert mp.export_state() == before and mp.landmarks().tobytes() == twin.landmarks().tobytes()
        _, wet = _observe(ctx, twin, st, c, "(7) applying")
        assert dry[0] == wet[0] and dry[1].tobytes() == wet[1].tobytes() and dry[2].tobytes() == wet[2].tobytes() and wet[0]["added"] > 0
        assert twin.export_state() != before
        mp.close(), twin.close()


# ---- 8. the observed map among the other calls
def test_08_export_import_merge_compact_and_update_on_an_observed_map(ctx):
    w, pieces, _ = mm.flicker()
    f = mm.FLICKER
    mp, other = ctx.map_create(f["cap"], f["carry"]), ctx.map_create(f["cap"] + 37, f["carry"] + 5)
    st, _, _, _ = _run(ctx, pieces[:4], "(8)", f["cap"], f["carry"], mp=mp)
    n = 12
    sub = dict(off=w["off"][:n + 1], rows=w["rows"][:int(w["off"][n])])
    kp, recs, ids = _localized(ctx, mp, sub, sub["rows"], lu.poses_of(w["truth"][:n], seed=1072), segment=ANY)
    c = dict(sub, loc=capi.localize_records(recs), ids=ids.cpu().numpy(), opts={}, edit=None)
    st, (res, _, _) = _observe(ctx, mp, st, c, "(8) observe")
    assert res["added"] > 50
    other.import_state(mp.export_state())
    st_other = dict(st, max_landmarks=other.max_landmarks, max_carry_rows=other.max_carry_rows)
    st, _ = _observe(ctx, mp, st, c, "(8) again")
    st_other, _ = _observe(ctx, other, st_other, c, "(8) again, on the imported map")
    assert mp.export_state() == other.export_state()
    st, results = _merge_to_fixpoint(ctx, mp, st, "(8) merge", max_gap_scans=mc.GAP)
    assert sum(r["merged"] for r in results) > 0
    _same_state(mp, st, "(8) merge")
    st, _, _ = _compact(ctx, mp, st, "(8) compact")
    st, _, _ = _step(ctx, mp, st, pieces[4], True, "(8) update")
    assert not st["header"]["flags"] & capi.FX_MAP_OVERLAP_MISMATCH and st["header"]["last_joined"] > 0
    _same_state(mp, st, "(8) update")
    assert any(r["flags"] & capi.FX_MAP_LM_OBSERVED and r["flags"] & capi.FX_MAP_LM_CONTINUED for r in st["landmarks"])
    mp.close(), other.close()


# ---- 9. refusals
def test_09_host_refusals_touch_no_output_byte(ctx, fxlib):
    import torch
    c = ou.duplicates()
    mp, st = _map_of(ctx, c, "(9)")
    other = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    theirs = other.map_create(8, 8)
    n, q = 2, len(c["rows"])
    (kb, S, T), loc, ids, _, _ = _upload(ctx, c, n, q, max_scans=4)
    dev = f"cuda:{ctx.device}"
    res, gained, obs = (torch.full((k,), FILL, dtype=torch.int32, device=dev) for k in (8 + 2, mp.max_landmarks + 2, q + 2))
    before = mp.export_state()
    O = capi.FxMapObserveOptions
    ok = dict(gate_dist=0.3, require_flags=capi.FX_LOC_VALID, mode=capi.FX_OBS_APPLY, reserved=0)
    opt = lambda **kw: C.byref(O(**dict(ok, **kw)))
    good = dict(c=ctx.handle, m=mp.handle, kp=kb.data_ptr(), S=S, T=T, loc=loc.data_ptr(), n=n, ids=ids.data_ptr(), q=q, opt=opt(), res=res.data_ptr(),
                gained=gained.data_ptr(), obs=obs.data_ptr())
    cases = [(dict(c=None), b"null"), (dict(m=None), b"null"), (dict(kp=None), b"null"), (dict(loc=None), b"null"), (dict(ids=None), b"null"),
             (dict(m=theirs.handle), b"another context"), (dict(c=other.handle), b"another context"), (dict(n=0), b"n_scans"), (dict(n=S + 1), b"n_scans")]
    cases += [(dict(opt=opt(gate_dist=v)), b"gate_dist") for v in (0.0, -1.0, float("nan"), float("inf"))]
    cases += [(dict(opt=opt(require_flags=0x20)), b"require_flags"), (dict(opt=opt(require_flags=0x80000001)), b"require_flags"),
              (dict(opt=opt(mode=2)), b"mode"), (dict(opt=opt(reserved=1)), b"reserved"),
              (dict(kp=kb.data_ptr() + 4), b"aligned"), (dict(loc=loc.data_ptr() + 4), b"aligned"), (dict(ids=ids.data_ptr() + 2), b"aligned"),
              (dict(res=res.data_ptr() + 2), b"aligned"), (dict(gained=gained.data_ptr() + 1), b"aligned"), (dict(obs=obs.data_ptr() + 2), b"aligned")]
    call = lambda a: fxlib.fx_map_observe(a["c"], a["m"], a["kp"], a["S"], a["T"], a["loc"], a["n"], a["ids"], a["q"], a["opt"], a["res"], a["gained"], a["obs"])
    for change, word in cases:
        assert call(dict(good, **change)) == 1 and word in fxlib.fx_last_error(), (change, word, fxlib.fx_last_error())
    ctx.synchronize()
    assert all((t == FILL).all().item() for t in (res, gained, obs)) and mp.export_state() == before
    # all three optional outputs NULL is legal, and so is a NULL table with q_max_rows == 0; opt == NULL: the defaults
    assert call(dict(good, ids=None, q=0, opt=None, res=None, gained=None, obs=None)) == capi.FX_OK
    ctx.synchronize()
    assert mp.export_state() == before, "no row, no change"
    assert call(dict(good, opt=None, res=None, gained=None, obs=None)) == capi.FX_OK
    ctx.synchronize()
    st1, ref, _, _ = ou.reference(st, c)
    _same_state(mp, st1, "(9) without outputs")
    assert call(dict(good, opt=None)) == capi.FX_OK
    ctx.synchronize()
    st2, *ref = ou.reference(st1, c)
    ou.assert_outputs((capi.observe_records(res[:8]), gained[:mp.max_landmarks].cpu().numpy(), obs[:q].cpu().numpy()), ref, "(9) defaults")
    _same_state(mp, st2, "(9) defaults")
    assert all((t[k:] == FILL).all().item() for t, k in ((res, 8), (gained, mp.max_landmarks), (obs, q)))
    theirs.close(), other.close(), mp.close()


# ---- 10. the same bytes from run to run, across contexts, with and without the optional arrays
def test_10_identical_bytes_across_runs_contexts_and_without_the_optional_arrays(ctx):
    c = ou.lists()
    w = mm.fragments(c["frags"], c["n_scans_map"])
    n, q = len(c["off"]) - 1, len(c["rows"])

    def once(cx, optional=True, repeat=1):
        outs = []
        for _ in range(repeat):
            mp, _ = _one_batch(cx, w, "(10)", cap=len(c["frags"]), carry=8)
            kp, loc, ids, _, _ = _upload(cx, c, n, q)
            res, gained, observed = _call(cx, mp, kp, loc, ids, n, q, optional)
            outs.append(repr(sorted(res.items())).encode() + mp.export_state() + (gained.tobytes() + observed.tobytes() if optional else b""))
            mp.close()
        assert len(set(outs)) == 1, "the same bytes twice"
        return outs[0]
    first = once(ctx, repeat=2)
    without = once(ctx, optional=False)
    assert first[:len(without)] == without, "without the optional arrays the map and the result are the same bytes"
    res, errs = {}, []

    def run(i):
        try:
            cx = capi.Context(capi.params("launch"), capi.limits(2, 1024))
            cx.set_batches_in_flight(4)
            res[i] = once(cx, repeat=3)
            cx.close()
        except Exception as e:  # (reported below)
            errs.append(e)
    ths = [threading.Thread(target=run, args=(i,)) for i in range(3)]
    [x.start() for x in ths]
    mine = once(ctx, repeat=3)  # (this context works while the others are busy on the device)
    [x.join() for x in ths]
    assert not errs, errs
    assert mine == first and all(res[i] == first for i in range(3))
