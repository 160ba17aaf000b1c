"""The landmark map's device calls in seeded random sequences (tests/map_walk_util.py): ONE context, the main map (1024 landmarks)
and the second map (192), the committed seeds' plans step by step through the per-call helpers of the other test_gpu_map_* modules.
After every step the call's outputs are the reference's bit for bit with their guards intact (the helpers), export_state() of BOTH
maps is capi.map_snapshot_pack of the reference states byte for byte, and fx_map_snapshot_check accepts the exported bytes.  There is
no tolerance anywhere.  The context is never recreated during a walk: every call starts on the scratch words the call before it
left, carved for another call, another capacity or another q_max_rows, and the alias and carry tables go through merge, append,
compact, join, close_loop and import in the orders tests/test_map_walk_reference.py counts.

What a stale word would show, read from the code (nothing broken was run).  Seed 16, step 20, fx_map_merge on the main map.  Step
16 was a merge of the same map that kept 14 links: prop[h] = g, pred[h] = g, succ[g] = h and keep[g] = (first_scan << 32) | h stay
in the scratch.  Nothing in between writes there: the update (17) has its own buffer, the join (18) nulls the merge's four arrays
and puts its own behind the grid's layout, the snapshot append (19) stages 12 KB of snapshot from the buffer's start, where the
main map's cand lies, while its keep begins 32 KB in and its prop 53 KB in; the buffer holds more than 128 KB since the
compaction of step 2 and the relocalize of step 8 and is not replaced before the localize of step 22.  Without the `if (A.prop)`
reset of k_mm_mark the 14 landmarks absorbed at step 16 no longer take part, so k_mm_search writes nothing for them, k_mm_link
still finds prop[h] = g with keep[g]'s low word h and keeps the 14 old links besides the 14 new ones: the result reads merged = 28
where the reference reads 14, and k_mm_fold adds the absorbed landmarks' sums to their roots a second time, which the snapshot
comparison shows as well.  Without k_mm_clear's reset of the state words the same step reports step 16's counts added to its own
(proposals, merged, live)."""
import threading

import pytest

from feature_extraction_amd import capi
from tests import map_walk_util as wu
from tests.map_append_util import _append
from tests.test_gpu_map import _step
from tests.test_gpu_map_compact import _compact, _same_state
from tests.test_gpu_map_find_loop import _find
from tests.test_gpu_map_join import _join
from tests.test_gpu_map_localize import _localize
from tests.test_gpu_map_loop import _close
from tests.test_gpu_map_merge import _merge
from tests.test_gpu_map_relocalize import REC_WORDS as RELOC_WORDS, _reloc

pytestmark = pytest.mark.gpu
MAIN, SECOND = wu.MAIN, wu.SECOND
POSE_WORDS = capi.POSE_DTYPE.itemsize // 4


class Device:
    """tests/map_walk_util.py's backend on the device: every method is one device call through its helper, which compares it with
    the reference and returns the reference's new state."""

    def __init__(self, ctx, lib):
        f = wu.WORLD
        self.ctx, self.lib = ctx, lib
        self.maps = [ctx.map_create(f["cap"], f["carry"]), ctx.map_create(f["cap2"], f["carry2"])]
        self.shrunk = [False, False]  # compacted, reset or imported into: the records past the ones stored are unspecified

    def release(self):
        for mp in self.maps:
            mp.close()

    def update(self, which, st, p, overlap, what):
        new, _, ids = _step(self.ctx, self.maps[which], st, p, overlap, what)
        return new, ids

    def merge(self, which, st, what, **kw):
        return _merge(self.ctx, self.maps[which], st, what, shrunk=self.shrunk[which], **kw)

    def compact(self, st, what, **kw):
        new, _, res = _compact(self.ctx, self.maps[MAIN], st, what, **kw)
        self.shrunk[MAIN] = True
        return new, res

    def append(self, dst_st, src_st, via, what):
        dst, src = self.maps
        if via == "device":
            return _append(self.ctx, dst, dst_st, src_st, what, src=src)
        data = src.export_state()
        if src_st["header"]["n_needed"] > src_st["header"]["n_landmarks"]:
            # fx_map_append_host runs fx_map_snapshot_check first: a source that overflowed is refused on the host, nothing is enqueued
            new, ref = capi.map_append_reference(dst_st, src_st)
            assert ref["flags"] & capi.FX_APPEND_OVERFLOWED and not ref["flags"] & capi.FX_APPEND_APPLIED
            with pytest.raises(capi.FxError):
                dst.append_state(data)
            self.ctx.synchronize()
            _same_state(dst, new, what)
            return new, ref
        return _append(self.ctx, dst, dst_st, src_st, what, data=data)

    def find(self, st, what, **opts):
        keep = {}
        ref = _find(self.ctx, self.maps[MAIN], st, what, keep=keep, **opts)
        return ref["rec"], keep["result"]

    def join(self, st, src, dst, what, prior, handle, **opts):
        host = dict(prior=prior) if handle is None else dict(prior_device=handle, prior_ref=prior)
        new, res, _ = _join(self.ctx, self.maps[MAIN], st, src, dst, what, **host, **opts)
        return new, res

    def close_loop(self, st, what, prior, handle, **opts):
        host = dict(prior=prior) if handle is None else dict(prior_device=handle, prior_ref=prior)
        new, res, _ = _close(self.ctx, self.maps[MAIN], st, what, **host, **opts)
        return new, res

    def localize(self, st, off, rows, priors, handle, q_max_rows, what):
        _, ref = _localize(self.ctx, self.maps[MAIN], st, off, rows, priors, what, q_max_rows=q_max_rows, priors_device=handle, **wu.LOCALIZE)
        return ref["rec"]

    def relocalize(self, st, off, rows, what):
        got, ref = _reloc(self.ctx, self.maps[MAIN], st, off, rows, what)
        n = len(off) - 1
        poses = got["raw"][:n * RELOC_WORDS].view(n, RELOC_WORDS)[:, :POSE_WORDS].contiguous()  # the fx_pose a record starts with
        return ref["rec"], poses

    def snapshot(self, which, st, what):
        mp = self.maps[which]
        blob = mp.export_state()
        assert blob == capi.map_snapshot_pack(st), f"{what}: the exported bytes"
        mp.reset()
        mp.import_state(blob)
        self.shrunk[which] = True
        return capi.map_snapshot_parse(blob, st["max_landmarks"], st["max_carry_rows"])

    def reset(self, which, what):
        self.maps[which].reset()
        self.shrunk[which] = True
        return wu.fresh(which)

    def check(self, states, what):
        for which, (mp, st) in enumerate(zip(self.maps, states)):
            _same_state(mp, st, f"{what}: map {which} afterwards")
            blob = mp.export_state()
            status = self.lib.fx_map_snapshot_check(blob, len(blob), mp.max_landmarks, mp.max_carry_rows)
            assert status == capi.FX_OK, f"{what}: map {which}: fx_map_snapshot_check refuses the export: {self.lib.fx_last_error().decode()}"

    def exported(self):
        return [mp.export_state() for mp in self.maps]


def _context():
    return capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)


def _walk(seed, lib, ctx=None):
    """The seed's walk on one context (made here unless given).  Returns (the two exported snapshots at the end, the log)."""
    own = ctx is None
    ctx = ctx or _context()
    be = Device(ctx, lib)
    try:
        st, log = wu.walk(seed, be)
        out = be.exported()
        if out != [capi.map_snapshot_pack(s) for s in st]:
            raise wu.WalkError(f"seed {seed}, after the last step: the exported snapshots are not the reference states'\n{wu.describe(log)}")
    finally:
        be.release()
        if own:
            ctx.close()
    return out, log


def _assert_same(seed, got, want, what):
    """(snapshots, log) of a walk against the same seed's walk alone; the message carries the seed, the first step that differs
    and the log."""
    if got[1] != want[1] or got[0] != want[0]:
        k = next((i for i, (a, b) in enumerate(zip(got[1], want[1])) if a != b), None)
        where = f"step {k}: {got[1][k]} against {want[1][k]}" if k is not None else f"the final snapshots differ (main {got[0][0] != want[0][0]}, second {got[0][1] != want[0][1]})"
        raise wu.WalkError(f"seed {seed}, {what}: {where}\nthe log (replay with plan({seed})):\n{wu.describe(got[1])}")


@pytest.fixture(scope="module")
def alone():
    """{seed: (the two final snapshots, the log)} of the walks test_walk ran, each alone on its own context."""
    return {}


@pytest.mark.parametrize("seed", wu.SEEDS)
def test_walk(fxlib, alone, seed):
    alone[seed] = _walk(seed, fxlib)
    out, log = alone[seed]
    assert len(log) == len(wu.plan(seed)), f"seed {seed}"


def test_walk_scratch_growth(fxlib, alone):
    """What this test holds on the device is one thing: wu.GROWTH_SEED's walk gives the plain walk's log and both final snapshots
    bit for bit when the scratch is replaced under it.  That the buffer is replaced is not observed here: the fxk_map_*_scratch
    sizes are not reachable from Python, so the steps are argued from the carve functions, and the model of them
    (map_walk_util.scratch_need, scratch_growths) is asserted on the CPU by tests/test_map_walk_reference.py.
    The context's first map call is a merge of a map of 8 landmarks, so the scratch is allocated at its minimum of 4096 bytes (the
    carve of 8 landmarks is under 1 KB).  DevScratch::reserve then replaces it by max(need, twice the old size, 4096) bytes after
    a stream synchronise, certainly at
      step 1   the main map's first localize, 67 KB (the grid: 56 B a landmark of 1024 and two tables of 1025 words; 12 B a row);
      step 2   the main map's compaction, 120 KB (it stages 112 B a landmark and keeps 8), to twice the 67 KB;
      step 22  a localize with q_max_rows 32768, 448 KB, which stands between the find_loop of step 21 and the join of step 24 that
               reads the find's result on the device: the result lies in the caller's tensor, and the join starts on a fresh
               buffer that nothing has initialised;
    the relocalize of step 8 and the find_loop of step 21 (132 KB and a few KB) need about what the buffer then holds and may or
    may not replace it.  The plain walk's buffer starts at the 67 KB of step 1 instead and grows at steps 2 and 22."""
    seed = wu.GROWTH_SEED
    ctx = _context()
    tiny = ctx.map_create(8, 8)
    tiny.merge(result=False)
    ctx.synchronize()
    try:
        got = _walk(seed, fxlib, ctx)
    finally:
        tiny.close()
        ctx.close()
    _assert_same(seed, got, alone[seed] if seed in alone else _walk(seed, fxlib), "on a scratch that starts at 4096 bytes")


def test_two_walks_at_once(fxlib, alone):
    """Two different seeds on two contexts in two threads: each gives the final snapshots and the log it gives alone."""
    seeds = wu.SEEDS[1], wu.SEEDS[3]
    want = {s: alone[s] if s in alone else _walk(s, fxlib) for s in seeds}
    res, errs = {}, []

    def run(seed):
        try:
            c = _context()
            c.set_batches_in_flight(2)
            try:
                res[seed] = _walk(seed, fxlib, c)
            finally:
                c.close()
        except Exception as e:  # (reported below)
            errs.append(e)
    ths = [threading.Thread(target=run, args=(s,)) for s in seeds]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errs, f"seeds {seeds} at once: {errs}"
    for s in seeds:
        _assert_same(s, res[s], want[s], f"beside seed {[x for x in seeds if x != s][0]} on another context")
