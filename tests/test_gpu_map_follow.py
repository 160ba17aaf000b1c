"""fx_map_follow on the GPU.  Every call of every case is compared with capi.map_follow_reference — the chain in Python floats
around capi.map_localize_reference, one scan at a time — bit for bit: every byte of the records, the follow records, the poses
and both row arrays.  The priors the device formed then go through ONE parallel fx_map_localize call, which must give the same
records and row arrays.  The guard words behind the five outputs must be untouched, and so must the map's snapshot."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import map_follow_util as fu
from tests import map_localize_util as lu
from tests import map_merge_util as mm
from tests import track_util as tu
from tests.test_gpu_map import _run
from tests.test_gpu_map_merge import _one_batch
from tests.test_gpu_track import FILL, GUARD
from tests.test_map_follow_reference import XY_BOUND, YAW_BOUND

pytestmark = pytest.mark.gpu
WORDS = tuple(dt.itemsize // 4 for dt in (capi.LOC_DTYPE, capi.FOLLOW_DTYPE, capi.POSE_DTYPE))
VALID = capi.FX_LOC_VALID
START, LINK, COASTED, HELD, LOST, NONE = fu.START, fu.LINK, fu.COASTED, fu.HELD, fu.LOST, fu.NONE
N = lu.WORLD["n_scans"]
F32 = lu.F32


def _context():
    return capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)


@pytest.fixture
def ctx(fxlib):
    c = _context()
    yield c
    c.close()


def _map_bytes(mp):
    """The map's snapshot: header, records, sums, alias and carry."""
    return mp.export_state()


def _up(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(f"cuda:{ctx.device}")


def _call(ctx, mp, kp, links, starts, n_scans, q, poses=True, nearest=True, **opts):
    """Map.follow into guarded outputs.  Returns ({"rec", "follow", "poses", "map_id_of_row", "nearest_of_row"}, the device tensor
    of the records)."""
    import torch
    dev = f"cuda:{ctx.device}"
    sizes = [n_scans * w for w in WORDS] + [q, q]
    raw = [torch.full((n + GUARD,), FILL, dtype=torch.int32, device=dev) for n in sizes]
    mp.follow(kp, links, starts, n_scans, q_max_rows=q, out=(raw[0][:sizes[0]], raw[1][:sizes[1]], raw[3][:q]),
              poses=raw[2][:sizes[2]] if poses else False, nearest=raw[4][:q] if nearest else False, **opts)
    ctx.synchronize()
    used = [sizes[0], sizes[1], sizes[2] if poses else 0, q, q if nearest else 0]
    for r, n, name in zip(raw, used, ("the records", "the follow records", "the poses", "map_id_of_row", "nearest_of_row")):
        assert (r[n:] == FILL).all().item(), f"the guard behind {name}"
    return {"rec": capi.localize_records(raw[0][:sizes[0]]), "follow": capi.follow_records(raw[1][:sizes[1]]),
            "poses": raw[2][:sizes[2]].cpu().numpy().view(np.uint8).reshape(-1).view(capi.POSE_DTYPE).copy() if poses else None,
            "map_id_of_row": raw[3][:q].cpu().numpy(), "nearest_of_row": raw[4][:q].cpu().numpy() if nearest else None}, raw[0]


def _follow(ctx, mp, st, off, rows, links, starts, what, n_scans=None, max_scans=None, max_total=None, q_max_rows=None, poses=True, nearest=True,
            starts_device=None, **opts):
    """One fx_map_follow against one map_follow_reference call, then the device against itself: the priors it formed through one
    fx_map_localize call.  The map must come out as it went in.  starts_device: a device address the call reads its start poses
    from in place of an upload of `starts` (which is then what the reference is given)."""
    import torch
    n_scans = len(off) - 1 if n_scans is None else n_scans
    max_scans = max(len(off) - 1, n_scans) + 2 if max_scans is None else max_scans
    max_total = len(rows) + 9 if max_total is None else max_total
    q = len(rows) if q_max_rows is None else q_max_rows
    kp = (torch.from_numpy(tu.block(off, rows, max_scans, max_total)).to(f"cuda:{ctx.device}"), max_scans, max_total)
    dl = _up(ctx, links) if links is not None and len(links) else None
    ds = _up(ctx, starts) if starts_device is None else starts_device
    before = _map_bytes(mp)
    got, recs = _call(ctx, mp, kp, dl, ds, n_scans, q, poses, nearest, **opts)
    ref = capi.map_follow_reference(st, off, rows, links, starts, n_scans, q_max_rows=q, **opts)
    fu.assert_equal(got, ref, what)
    # the device against itself
    loc = dict({k: capi.FOLLOW_DEFAULTS[k] for k in capi.LOC_DEFAULTS}, **{k: v for k, v in opts.items() if k in capi.LOC_DEFAULTS})
    pri = _up(ctx, got["follow"]["prior"])
    r2, ids2, near2 = mp.localize(kp, pri, n_scans, q_max_rows=q, **loc)
    ctx.synchronize()
    assert capi.localize_records(r2).tobytes() == got["rec"].tobytes(), f"{what}: one parallel localise under the follow's priors gives other records"
    assert (ids2.cpu().numpy() == got["map_id_of_row"]).all() and (nearest is False or (near2.cpu().numpy() == got["nearest_of_row"]).all()), what
    assert _map_bytes(mp) == before, f"{what}: the map is read, never written"
    return got, ref, recs


# ---- the worlds of the reference's tests through the device
@pytest.fixture(scope="module")
def driven(fxlib):
    c = _context()
    w, pieces = lu.clean_world(0, fu.SIGMA)
    W = lu.WORLD
    mp = c.map_create(W["cap"], W["carry"])
    st, _, _, _ = _run(c, pieces, "the map of seed 0", W["cap"], W["carry"], mp=mp)
    yield c, mp, st, w, fu.biased_links(w), lu.poses_of(w["truth"][:1])
    mp.close(), c.close()


def test_a_biased_odometry(driven):
    c, mp, st, w, links, start = driven
    got, _, _ = _follow(c, mp, st, w["off"], w["rows"], links, start, "(a)")
    assert (got["rec"]["flags"] == VALID).all() and got["follow"]["flags"].tolist() == [START] + [LINK] * (N - 1)
    dxy, _, dyaw = lu.pose_errors(got["poses"], w["truth"])
    assert dxy <= XY_BOUND and dyaw <= YAW_BOUND
    _follow(c, mp, st, w["off"], w["rows"], links, start, "(a) without the optional arrays", poses=False, nearest=False)


def test_b_unusable_links(driven):
    c, mp, st, w, links, start = driven
    bad = links.copy()
    bad["flags"][[9, 10]] = 0
    got, _, _ = _follow(c, mp, st, w["off"], w["rows"], bad, start, "(b)")
    assert got["follow"]["flags"][[10, 11]].tolist() == [COASTED] * 2 and got["follow"]["motion"][[10, 11]].tolist() == [8, 8]
    assert (got["rec"]["flags"] == VALID).all()
    bad["tx"][3], bad["s"][15] = np.inf, np.nan
    _follow(c, mp, st, w["off"], w["rows"], bad, start, "(b) links that are not finite")
    _follow(c, mp, st, w["off"], w["rows"], links, start, "(b) a flag no link carries", require_flags=capi.FX_REG_VALID | capi.FX_REG_TRUNCATED)


def test_c_empty_scans(driven):
    c, mp, st, w, links, start = driven
    off, rows = fu.without_rows(w, (5, 6, 7))
    got, _, _ = _follow(c, mp, st, off, rows, links, start, "(c)", max_lost=3)
    assert got["follow"]["streak"][4:9].tolist() == [0, 1, 2, 3, 0] and [b for b in range(N) if got["follow"]["flags"][b] & LOST] == [7]


def test_d_chain_edges(driven):
    c, mp, st, w, links, start = driven
    starts = lu.poses_of([w["truth"][f] for f in range(0, N, 5)])
    starts["segment"], starts["flags"] = np.arange(len(starts)) + 2, capi.FX_POSE_GAP
    wild = links.copy()
    wild["tx"][4], wild["ty"][4] = 500.0, -500.0
    got, _, _ = _follow(c, mp, st, w["off"], w["rows"], wild, starts, "(d) chains of 5", chain_scans=5)
    assert [b for b in range(N) if got["follow"]["flags"][b] & START] == [0, 5, 10, 15, 20] and (got["rec"]["flags"] == VALID).all()
    whole, _, _ = _follow(c, mp, st, w["off"], w["rows"], links, start, "(d) chain_scans 0")
    for big in (N, N + 7):
        one, _, _ = _follow(c, mp, st, w["off"], w["rows"], links, start, f"(d) chain_scans {big}", chain_scans=big)
        assert all(one[k].tobytes() == whole[k].tobytes() for k in one)
    _follow(c, mp, st, w["off"], w["rows"], links, lu.poses_of(w["truth"]), "(d) chains of 1", chain_scans=1)


def test_batch_to_batch_without_a_host_read(driven):
    """24 scans as batches of 9, 9 and 8 that overlap by one scan; a batch's start pose is the address of the pose in the last
    record of the batch before, on the device."""
    c, mp, st, w, links, start = driven
    off = [int(x) for x in w["off"]]
    whole, _, _ = _follow(c, mp, st, w["off"], w["rows"], links, start, "one chain")
    ref_start, dev_start, keep = start, None, []
    for a, b in ((0, 8), (8, 16), (16, 23)):
        o = np.array(off[a:b + 2], np.uint32) - np.uint32(off[a])
        got, ref, recs = _follow(c, mp, st, o, w["rows"][off[a]:off[b + 1]], links[a:b], ref_start, f"batch {a} .. {b}", starts_device=dev_start)
        keep.append(recs)  # (the next call reads it)
        ref_start = ref["rec"]["pose"][-1:].copy()
        dev_start = recs[(b - a) * WORDS[0]:]  # &out[last].pose
        assert (got["rec"]["flags"] == VALID).all()
    d = math.hypot(got["poses"]["tx"][-1] - whole["poses"]["tx"][-1], got["poses"]["ty"][-1] - whole["poses"]["ty"][-1])
    dyaw = tu.yaw_err(math.atan2(got["poses"]["s"][-1], got["poses"]["c"][-1]), math.atan2(whole["poses"]["s"][-1], whole["poses"]["c"][-1]))
    assert d <= XY_BOUND and dyaw <= YAW_BOUND, (d, dyaw)


def test_two_contexts_follow_two_maps_at_once(fxlib):
    errs, done = [], {}

    def run(seed):
        try:
            c = _context()
            c.set_batches_in_flight(4)
            w, pieces = lu.clean_world(seed, fu.SIGMA)
            W = lu.WORLD
            mp = c.map_create(W["cap"], W["carry"])
            st, _, _, _ = _run(c, pieces, f"the map of seed {seed}", W["cap"], W["carry"], mp=mp)
            starts = lu.poses_of([w["truth"][f] for f in range(0, N, 6)])
            outs = [_follow(c, mp, st, w["off"], w["rows"], fu.biased_links(w), starts, f"seed {seed}, run {k}", chain_scans=6)[0] for k in range(3)]
            assert all(o[k].tobytes() == outs[0][k].tobytes() for o in outs for k in o), "the same bytes from run to run"
            done[seed] = True
            mp.close(), c.close()
        except Exception as e:  # (reported below)
            errs.append(e)
    ths = [threading.Thread(target=run, args=(s,)) for s in (0, 1)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, errs
    assert done == {0: True, 1: True}


# ---- hand-built small shapes: maps of fragments (two identical observations each, z = 1), scans placed by hand
LAT = lu.lattice(16)  # 4 x 4, 4 m apart
SCAN = lu.rows_at(LAT, [0, 1, 2, 5, 6, 9], 0.1)
BIG = lu.lattice(1100, pitch=3.0)


def _still(n, **fields):
    r = np.zeros(n, capi.REG_DTYPE)
    r["c"], r["flags"] = 1.0, capi.FX_REG_VALID
    for k, v in fields.items():
        r[k] = v
    return r


@pytest.fixture(scope="module")
def lat_map(fxlib):
    c = _context()
    mp, st = _one_batch(c, mm.fragments(LAT, 3), "the map of 16")
    yield c, mp, st
    mp.close(), c.close()


def test_chains_of_one_and_two_scans_and_a_scan_beyond_the_block(lat_map):
    c, mp, st = lat_map
    off, rows = lu.scans([SCAN])
    got, _, _ = _follow(c, mp, st, off, rows, None, lu.identity(1, ty=0.2), "a chain of 1, links NULL")
    assert got["follow"]["flags"].tolist() == [START] and got["rec"]["flags"].tolist() == [VALID]
    off, rows = lu.scans([SCAN, lu.rows_at(LAT, [3, 7, 10, 11, 14], -0.1, 0.05)])
    got, _, _ = _follow(c, mp, st, off, rows, _still(1, tx=0.25, ty=-0.125), lu.identity(1, ty=0.2), "a chain of 2")
    assert got["follow"]["flags"].tolist() == [START, LINK] and got["rec"]["flags"].tolist() == [VALID, VALID]
    got, _, _ = _follow(c, mp, st, off, rows, _still(2, tx=0.25), lu.identity(1, ty=0.2), "n_scans one above the block's scans", n_scans=3, max_scans=3)
    assert got["follow"]["flags"].tolist() == [START, LINK, HELD] and got["rec"]["flags"][2] == capi.FX_LOC_NO_SCAN
    assert got["poses"][2].tobytes() == got["poses"][1].tobytes()
    _follow(c, mp, st, off, rows, _still(2, tx=0.25), lu.identity(3, ty=0.2), "the same in chains of 1", n_scans=3, max_scans=3, chain_scans=1)
    for q in (len(rows) - 3, len(rows) - 6, 0, len(rows) + 5):
        _follow(c, mp, st, off, rows, _still(1, tx=0.25), lu.identity(1, ty=0.2), f"q_max_rows {q}", q_max_rows=q, nearest=bool(q))


def test_special_priors(lat_map):
    c, mp, st = lat_map
    off, rows = lu.scans([SCAN] * 4)
    start = lu.identity(1, segment=7, flags=capi.FX_POSE_GAP)
    start["ty"] = np.frombuffer(np.uint64(0xfff8dead0000beef).tobytes(), np.float64)[0]
    got, _, _ = _follow(c, mp, st, off, rows, _still(3), start, "a start that is no number")
    assert got["rec"]["flags"].tolist() == [capi.FX_LOC_BAD_PRIOR] * 4 and all(p.tobytes() == start[0].tobytes() for p in got["follow"]["prior"])
    links = _still(3)
    links["tx"][0] = 1e308
    got, _, _ = _follow(c, mp, st, off, rows, links, lu.identity(1, tx=1e308), "a composition that overflows")
    assert got["follow"]["flags"].tolist()[:3] == [START, HELD, LINK]
    links = _still(3, tx=0.05)
    links["flags"][[0, 2]] = 0
    got, _, _ = _follow(c, mp, st, off, rows, links, lu.identity(1), "held, then coasting", max_lost=1)
    assert got["follow"]["flags"].tolist() == [START, HELD, LINK, COASTED] and got["follow"]["motion"].tolist() == [NONE, NONE, 1, 1]


def test_64_chains_of_3_scans_in_one_call(lat_map):
    c, mp, st = lat_map
    rng = np.random.default_rng(91)
    by_scan, motions = [], []
    for b in range(192):
        pick = rng.permutation(16)[:rng.integers(0, 9)]
        by_scan.append([(F32(LAT[k][1] + rng.uniform(-0.1, 0.1)), F32(LAT[k][2] + rng.uniform(-0.1, 0.1)), F32(rng.uniform(0, 2))) for k in pick])
        motions.append((rng.uniform(-0.01, 0.01), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(-0.05, 0.05)))
    links = tu.reg_records(motions[:191])
    links["flags"][rng.permutation(191)[:40]] = 0
    starts = lu.identity(64)
    starts["tx"], starts["ty"], starts["segment"] = rng.uniform(-0.3, 0.3, 64), rng.uniform(-0.3, 0.3, 64), np.arange(64)
    off, rows = lu.scans(by_scan)
    got, _, _ = _follow(c, mp, st, off, rows, links, starts, "64 chains of 3", chain_scans=3, max_lost=2, min_baseline=1.0)
    kinds = set((got["follow"]["flags"] & 0xf).tolist())
    assert kinds == {START, LINK, COASTED, HELD} and 40 < int((got["rec"]["flags"] & VALID != 0).sum()) < 192


def test_the_tie_scans_as_scan_1_of_a_chain(ctx):
    """lu.tie_scans behind an empty scan 0 and a link that moves nothing: the prior of scan 1 is the start pose's five doubles, and
    the lower of the two live samples wins in every position of the reduction."""
    rows, want = lu.tie_scans()
    mp, st = _one_batch(ctx, mm.fragments(lu.TIE_FRAGS, 3), "the tie map", carry=8)
    by_scan = [s for tie in rows for s in ([], tie)]
    off, flat = lu.scans(by_scan)
    n = len(by_scan)
    got, _, _ = _follow(ctx, mp, st, off, flat, _still(n - 1), lu.identity(len(rows)), "ties", chain_scans=2, **lu.TIE_OPTS)
    rec = got["rec"][1::2]
    assert (rec["n_corr"] == lu.TIE_H).all() and (rec["n_inliers"] == 2).all() and (rec["flags"] == VALID).all()
    assert [(int(a) - lu.TIE_H * b, int(c_) - lu.TIE_H * b) for b, (a, c_) in enumerate(zip(rec["hyp_a"], rec["hyp_b"]))] == want
    mp.close()


def test_long_scans_in_front_of_short_ones(fxlib):
    """A scan of 257 rows (two strides of the search), one of 1025 correspondences (FX_LOC_TRUNCATED) and one of 3 behind it: the
    short scan's record is clean, whatever the long ones left in LDS."""
    c = _context()
    mp, st = _one_batch(c, mm.fragments(BIG, 3), "the map of 1100", cap=1100, carry=8)
    rng = np.random.default_rng(92)
    at = lambda ks, dx: [(F32(BIG[k][1] + dx + rng.uniform(-0.02, 0.02)), F32(BIG[k][2] + rng.uniform(-0.02, 0.02)), F32(rng.uniform(0, 2))) for k in ks]
    by_scan = [at(rng.permutation(1100)[:257], 0.1), at(range(1025), -0.1), at([7, 400, 1000], 0.05), at(rng.permutation(1100)[:64], 0.0)]
    off, rows = lu.scans(by_scan)
    got, _, _ = _follow(c, mp, st, off, rows, _still(3, tx=0.03, ty=-0.02), lu.identity(1, tz=0.5), "long, then short", hyp_corr=4)
    rec = got["rec"]
    assert rec["n_corr"].tolist() == [257, 1024, 3, 64] and rec["flags"].tolist() == [VALID, VALID | capi.FX_LOC_TRUNCATED, VALID, VALID]
    assert rec["n_inliers"].tolist() == [257, 1024, 3, 64]
    mp.close(), c.close()


# ---- refusals
def test_host_refusals_touch_no_output_byte(lat_map, fxlib):
    import torch
    c, mp, st = lat_map
    other = _context()
    theirs = other.map_create(8, 8)
    off, rows = lu.scans([SCAN, SCAN])
    dev = f"cuda:{c.device}"
    kb, S, T = torch.from_numpy(tu.block(off, rows, 4, 16)).to(dev), 4, 16
    links, starts = _up(c, _still(1)), _up(c, lu.identity(2))
    outs = [torch.full((n,), FILL, dtype=torch.int32, device=dev) for n in (2 * WORDS[0] + 2, 2 * WORDS[1] + 2, 2 * WORDS[2] + 2, 14, 14)]
    before = _map_bytes(mp)
    ok = dict(search_dist=2.0, inlier_dist=0.3, min_baseline=2.0, hyp_corr=64, min_inliers=3, min_landmark_obs=2, segment=capi.FX_LOC_ANY_SEGMENT, reserved=0)

    def opt(chain_scans=0, require_flags=capi.FX_REG_VALID, max_lost=5, reserved=0, **loc):
        return C.byref(capi.FxFollowOptions(capi.FxLocalizeOptions(**dict(ok, **loc)), chain_scans, require_flags, max_lost, reserved))
    good = dict(c=c.handle, m=mp.handle, kp=kb.data_ptr(), S=S, T=T, links=links.data_ptr(), starts=starts.data_ptr(), n=2, q=12, opt=opt(),
                out=outs[0].data_ptr(), fol=outs[1].data_ptr(), poses=outs[2].data_ptr(), ids=outs[3].data_ptr(), near=outs[4].data_ptr())
    cases = [(dict(c=None), b"null"), (dict(m=None), b"null"), (dict(kp=None), b"null"), (dict(starts=None), b"null"), (dict(out=None), b"null"),
             (dict(fol=None), b"null"), (dict(ids=None), b"null"), (dict(links=None), b"null"), (dict(links=None, opt=opt(chain_scans=3)), b"null"),
             (dict(m=theirs.handle), b"another context"), (dict(c=other.handle), b"another context"), (dict(n=0), b"n_scans"), (dict(n=S + 1), b"n_scans")]
    cases += [(dict({k: good[k] + (2 if k in ("ids", "near") else 4)}), b"aligned") for k in ("kp", "links", "starts", "out", "fol", "poses", "ids", "near")]
    for f in ("search_dist", "inlier_dist", "min_baseline"):
        cases += [(dict(opt=opt(**{f: v})), f.encode()) for v in (0.0, -1.0, float("nan"), float("inf"))]
    cases += [(dict(opt=opt(hyp_corr=1)), b"hyp_corr"), (dict(opt=opt(hyp_corr=129)), b"hyp_corr"), (dict(opt=opt(min_inliers=1)), b"min_inliers"),
              (dict(opt=opt(min_landmark_obs=0)), b"min_landmark_obs"), (dict(opt=opt(max_lost=0)), b"max_lost"),
              (dict(opt=opt(require_flags=8)), b"require_flags"), (dict(opt=opt(require_flags=0x80000001)), b"require_flags"), (dict(opt=opt(reserved=1)), b"reserved")]
    loc_reserved = capi.FxFollowOptions(capi.FxLocalizeOptions(**dict(ok, reserved=1)), 0, capi.FX_REG_VALID, 5, 0)
    cases.append((dict(opt=C.byref(loc_reserved)), b"reserved"))

    def call(a):
        return fxlib.fx_map_follow(a["c"], a["m"], a["kp"], a["S"], a["T"], a["links"], a["starts"], a["n"], a["q"], a["opt"], a["out"], a["fol"], a["poses"],
                                   a["ids"], a["near"])
    for change, word in cases:
        assert call(dict(good, **change)) == 1 and word in fxlib.fx_last_error(), (change, word, fxlib.fx_last_error())
    c.synchronize()
    assert all((t == FILL).all().item() for t in outs) and _map_bytes(mp) == before
    # opt == NULL: the defaults; links may be NULL when every chain is one scan; poses and nearest_of_row may be NULL
    assert call(dict(good, links=None, opt=opt(chain_scans=1), poses=None, near=None)) == capi.FX_OK
    assert call(dict(good, opt=None)) == capi.FX_OK
    c.synchronize()
    ref = capi.map_follow_reference(st, off, rows, _still(1), lu.identity(2), 2)
    got = {"rec": capi.localize_records(outs[0][:2 * WORDS[0]]), "follow": capi.follow_records(outs[1][:2 * WORDS[1]]),
           "poses": outs[2][:2 * WORDS[2]].cpu().numpy().view(np.uint8).reshape(-1).view(capi.POSE_DTYPE).copy(),
           "map_id_of_row": outs[3][:12].cpu().numpy(), "nearest_of_row": outs[4][:12].cpu().numpy()}
    fu.assert_equal(got, ref, "the defaults")
    assert all((t[n:] == FILL).all().item() for t, n in zip(outs, (2 * WORDS[0], 2 * WORDS[1], 2 * WORDS[2], 12, 12)))
    theirs.close(), other.close()
