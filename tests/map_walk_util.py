"""Helpers of the map walk tests (tests/test_map_walk_reference.py, tests/test_gpu_map_walk.py): seeded, guided random sequences
of the landmark map's calls over two maps of different capacities, run step by step through a backend (the numpy references here,
the device helpers in tests/test_gpu_map_walk.py), and the census that proves a set of walks reaches the states that matter.
CPU only: no torch is imported here.

The world.  map_loop_util.loop_world as it is (250 poles in a field of 200 m, a circle of radius 60 m run for 1.2 laps in 80 scans,
reach 35 m, noise 1 cm, a yaw bias of 3e-4 rad and an along-track bias of 3 mm a link), cut every 8 scans into 10 pieces that
overlap by one scan.  The main map (max_landmarks 1024, max_carry_rows 128: a table of 1024 buckets) is fed this run, 206
landmarks in all.  The second map (192 and 64: a table of 256 buckets) is fed a second session of the same world: fresh noise
of 2 cm on the rows' x, y, z (seed 99), the same cut, from another start pose, in the style of map_append_util.CHAIN; its whole
run needs more than 192 landmarks, so it overflows in its last pieces and an append of it is then refused.

The schedule.  plan(seed) is a pure function of the seed: a list of (call, map, options).  It is guided by a small model of the
run (pieces fed to either map, segments, twins waiting for a merge, absorbed landmarks waiting for a compaction): a call is drawn
only where its precondition can hold, and with a weight that is high where it is likely to change something.  Half of the seeds
Two fifths of the seeds feed the main run first and nearly unbroken, so that its loop can close, and append afterwards; a
fifth feed the second map six pieces and append it until the main map has no room (FX_APPEND_NO_ROOM); of the others most carry a
scripted subsequence (GENERATIONS below) with read-only calls and calls on the second map strewn in.  The second map's merges
never merge anything (its run has no fragments): they are there for their carve of the scratch, drawn often in one seed of
seven and rarely elsewhere.  A grid call of the main map is favoured directly after a merge of the second map (the other
capacity's carve), a join or a close_loop directly after the find_loop whose transform is its prior, a localize directly after
a relocalize (its poses are the priors).  The options that name a segment are symbolic ("first", "prev") and resolved against the state when the
step runs.  SEEDS are the committed walks; tests/test_map_walk_reference.py states what they meet and measures them."""
import functools
import math

import numpy as np

from feature_extraction_amd import capi
from tests import map_append_util as au
from tests import map_find_loop_util as fu
from tests import map_localize_util as llu
from tests import map_loop_util as lu
from tests import map_util as mu
from tests import track_util as tu

WORLD = dict(step=8, cap=1024, carry=128, cap2=192, carry2=64, sigma2=0.02, seed2=99,
             init_pose2=(math.cos(0.7), math.sin(0.7), 40.0, -25.0, 0.5))
MAIN, SECOND = 0, 1
CHANGING = ("update", "merge", "compact", "append", "join", "close_loop", "snapshot")
READ_ONLY = ("find_loop", "localize", "relocalize")
CALLS = CHANGING + READ_ONLY + ("reset",)
TOP = 0xffffffff
N_PIECES = 10
WIDE_ROWS = 32768  # q_max_rows of a "wide" localize: 12 B a row behind the grid, more than twice any other call's scratch
GENERATIONS = ("merge", "append", "merge", "join", "update", "compact", "merge", "update")
LOCALIZE = dict(segment=capi.FX_LOC_ANY_SEGMENT)
FIND = dict(same=dict(lu.OPTS), cross=dict(segment=fu.LAST, target_segment=0, recent_scans=TOP))


@functools.lru_cache(maxsize=None)
def world():
    """(w, the main run's pieces, the second session's pieces)."""
    f = WORLD
    w, pieces = lu.loop_world(step=f["step"])
    w2 = dict(w, rows=w["rows"].copy())
    w2["rows"][:, :3] += (f["sigma2"] * np.random.default_rng(f["seed2"]).standard_normal((len(w2["rows"]), 3))).astype(np.float32)
    pieces2 = mu.split(w2, mu.every(w["n_scans"], f["step"]))
    assert len(pieces) == len(pieces2) == N_PIECES
    return w, pieces, pieces2


def fresh(which):
    f = WORLD
    return capi.map_state(f["cap"], f["carry"]) if which == MAIN else capi.map_state(f["cap2"], f["carry2"])


# ---- the schedule
def _pick(rng, weighted):
    names = [k for k, v in weighted if v > 0]
    p = np.array([v for _, v in weighted if v > 0], float)
    return names[int(rng.choice(len(names), p=p / p.sum()))]


def plan(seed):
    """The walk of `seed`: [(call, map, options)], 40 to 60 steps."""
    rng = np.random.default_rng([int(seed), 0x77616c6b])
    n = int(rng.integers(44, 57))
    m = dict(fed=0, fed2=0, segs=0, segs2=0, twins=0, absorbed=False, relocs=0, find=None, reloc=None, foreign=False, n=0)
    style = str(rng.choice(["early", "late", "crowd"], p=[0.4, 0.4, 0.2]))
    late = style == "late"  # the main run first, nearly unbroken (its loop can close), the appends afterwards
    crowd = style == "crowd"  # the second map fed to 6 pieces and appended until the main map has no room for it
    carve = rng.random() < 0.15  # merges of the second map, for their carve of the scratch (they never merge anything)
    script = []
    if not late and rng.random() < 0.7:
        script = [("update", dict(overlap=False)), ("join", dict(dst="first")), ("merge", dict(max_gap_scans=1 << 20)),
                  ("update", dict(overlap=False)), ("join", dict(dst="first")), ("append", None), ("merge", dict(max_gap_scans=1 << 20)),
                  ("find_loop", dict(kind="cross")), ("join", dict(dst="first", device=True)), ("update", None),
                  ("compact", dict(min_obs=1, min_age_scans=64)), ("merge", dict(max_gap_scans=1 << 20)), ("update", None)]
    steps = []

    def options(call, which):
        if call == "update":
            k = m["fed"] if which == MAIN else m["fed2"]
            return dict(piece=k, overlap=bool(k > 0 and rng.random() < (0.9 if late and which == MAIN else 0.75)))
        if call == "merge":
            return dict(max_gap_scans=int(rng.choice([16, 64, 1 << 20], p=[0.2, 0.3, 0.5])))
        if call == "compact":
            return dict(min_obs=int(rng.choice([1, 2, 3])), min_age_scans=int(rng.choice([0, 8, 64])))
        if call == "append":
            return dict(via=str(rng.choice(["device", "snapshot"])))
        if call == "join":
            return dict(dst=str(rng.choice(["first", "prev"])), device=bool(rng.random() < 0.5))
        if call == "close_loop":
            return dict(device=bool(rng.random() < 0.5))
        if call == "find_loop":
            same = m["fed"] >= 9 and (m["segs"] < 2 or rng.random() < 0.6)
            return dict(kind="same" if same else "cross")
        if call == "localize":
            if m["reloc"] is not None and rng.random() < 0.8:
                return dict(piece=m["reloc"][0], scan=m["reloc"][1], device=bool(rng.random() < 0.5), wide=False)
            return dict(piece=int(rng.integers(0, m["fed"])), scan=None, seed=int(rng.integers(1000, 2000)), device=False,
                        wide=bool(m["find"] is not None and rng.random() < 0.5))
        if call == "relocalize":
            return dict(piece=int(rng.integers(0, m["fed"])), scan=int(rng.integers(1, 8)))
        return {}

    def emit(call, which, o):
        steps.append((call, which, o))
        if which == SECOND:
            if call == "update":
                m["fed2"] += 1
                m["segs2"] += 0 if o["overlap"] else 1
            elif call == "reset":
                m["fed2"] = m["segs2"] = 0
            return
        if call in CHANGING:
            m["find"], m["reloc"] = None, None
        if call == "update":
            m["fed"] += 1
            m["n"] += 21
            m["segs"] += 0 if (o["overlap"] and not m["foreign"]) else 1
            m["foreign"] = False
        elif call == "join" and m["segs"] >= 2:
            m["segs"] -= 1
            m["twins"] += 1
        elif call == "close_loop" and m["fed"] >= 9:
            m["twins"] += 1
        elif call == "merge" and m["twins"]:
            m["twins"], m["absorbed"] = 0, True
        elif call == "compact":
            m["absorbed"] = False
        elif call == "append" and 0 < m["fed2"] < 7 and m["n"] + 27 * m["fed2"] <= WORLD["cap"]:
            m["segs"] += m["segs2"]
            m["foreign"] = True
            m["n"] += 27 * m["fed2"]
        elif call == "find_loop":
            m["find"] = o["kind"]
        elif call == "relocalize":
            m["relocs"] += 1
            m["reloc"] = (o["piece"], o["scan"])

    def aside():
        """A step that leaves the main map as it is: a read-only call or a call on the second map."""
        c = [("localize", 2.0 if m["fed"] else 0), ("relocalize", 0.7 if m["fed"] and m["relocs"] < 2 and m["n"] <= 450 else 0),
             ("update2", 2.0 if m["fed2"] < N_PIECES else 0), ("merge2", 0 if not m["fed2"] else 1.5 if carve else 0.1),
             ("find_loop", 0.5 if m["fed"] else 0)]
        k = _pick(rng, c)
        if k.endswith("2"):
            emit(k[:-1], SECOND, options(k[:-1], SECOND))
        else:
            emit(k, MAIN, options(k, MAIN))

    while len(steps) < n:
        left = n - len(steps)
        if script and (len(script) >= left or (m["fed"] >= 3 and m["fed2"] >= 2)) and m["fed"] >= 1:
            if m["fed2"] == 0 or (len(script) < left and rng.random() < 0.3):
                if m["fed2"] == 0:
                    emit("update", SECOND, options("update", SECOND))
                else:
                    aside()
                continue
            call, o = script.pop(0)
            base = options(call, MAIN)
            if call == "update" and m["fed"] >= N_PIECES:
                continue
            emit(call, MAIN, dict(base, **(o or {})))
            continue
        fed, fed2 = m["fed"], m["fed2"]
        looped = fed >= 9
        c = [("update", (6.0 if N_PIECES - fed >= left / 4 else 3.0) if fed < N_PIECES else 0),
             ("update2", (4.0 if fed2 < 6 else 0) if crowd else 2.5 if fed2 < N_PIECES else 0),
             ("merge2", 0 if not fed2 else 1.5 if carve else 0.08),
             ("reset2", 0.0 if not fed2 or crowd else 2.0 if fed2 >= 9 else 0.25),
             ("merge", 0 if not fed else 5.0 if m["twins"] else 0.25),
             ("compact", 0 if not fed else 3.5 if m["absorbed"] else 0.5),
             ("append", 0 if not (fed and fed2) or (late and fed < N_PIECES) else (4.0 if fed2 >= 5 else 0.3) if crowd else 1.6 if fed2 < 9 else 0.5),
             ("join", 3.5 if m["segs"] >= 2 else 0),
             ("close_loop", (3.0 if late else 0.8) if looped else 0.1 if fed >= 2 else 0),
             ("find_loop", 2.5 if looped or m["segs"] >= 2 else 0.3 if fed else 0),
             ("localize", 1.3 if fed else 0),
             ("relocalize", 0.6 if fed and m["relocs"] < 2 and m["n"] <= 450 else 0),
             ("snapshot", 1.0 if fed else 0.5)]
        if steps and steps[-1][:2] == ("merge", SECOND):  # the main map's grid calls on the other capacity's carve
            c = [(k, v * (6.0 if k in ("merge", "localize", "relocalize", "find_loop") else 1.0)) for k, v in c]
        if m["find"] is not None and steps[-1][:2] == ("find_loop", MAIN):  # its transform is the prior of the join or the closure
            c = [(k, v * (8.0 if k == ("join" if m["find"] == "cross" else "close_loop") else 1.0)) for k, v in c]
        if m["reloc"] is not None and steps[-1][0] == "relocalize":  # its poses are the next localize's priors
            c = [(k, v * (10.0 if k == "localize" else 1.0)) for k, v in c]
        k = _pick(rng, c)
        which = SECOND if k.endswith("2") else MAIN
        k = k[:-1] if which == SECOND else k
        emit(k, which, options(k, which))
    return steps


# ---- one step's result, boiled down to what the log and the census need
def effective(call, r):
    """Did the step change or find something?  r: the step's summary (the walk's log keeps it)."""
    if call == "update":
        return r["rows_with_id"] > 0 or r["added"] > 0
    if call == "merge":
        return r["merged"] > 0
    if call == "compact":
        return r["kept"] < r["before"]
    if call == "append":
        return bool(r["flags"] & capi.FX_APPEND_APPLIED)
    if call in ("join", "close_loop"):
        return bool(r["flags"] & 0x1) and r["moved"] > 0  # FX_JOIN_APPLIED == FX_LOOP_APPLIED == 0x1
    if call == "find_loop":
        return bool(r["flags"] & capi.FX_FIND_VALID)
    if call in ("localize", "relocalize"):
        return r["valid"] > 0
    if call in ("snapshot", "reset"):
        return r["n_landmarks"] > 0
    raise KeyError(call)


assert capi.FX_JOIN_APPLIED == capi.FX_LOOP_APPLIED == 0x1 and capi.FX_LOC_VALID == capi.FX_RELOC_VALID == 0x1


def _ints(rec, names):
    return {k: int(rec[k]) for k in names}


def describe(log):
    return "\n".join(f"  {e['step']:2d} {'main  ' if e['map'] == MAIN else 'second'} {e['call']:<10} {e['options']} -> {e['result']}"
                     f" {'effective' if e['effective'] else 'nothing'}" for e in log)


class WalkError(AssertionError):
    pass


# ---- the backends
class Reference:
    """The numpy references alone.  Every method returns what the device backend returns: the new state(s) and plain results."""

    def __init__(self, lib=None):
        self.lib = lib

    def update(self, which, st, p, overlap, what):
        tr = tu.reference(p, init_pose=st["header"]["last_pose"][:5])
        return capi.map_reference(st, p["off"], p["rows"], tr, overlap=overlap)

    def merge(self, which, st, what, **kw):
        return capi.map_merge_reference(st, **kw)

    def compact(self, st, what, **kw):
        new, _, res = capi.map_compact_reference(st, **kw)
        return new, res

    def append(self, dst_st, src_st, via, what):
        return capi.map_append_reference(dst_st, src_st)

    def find(self, st, what, **opts):
        return capi.map_find_loop_reference(st, **opts)["rec"], None

    def join(self, st, src, dst, what, prior, handle, **opts):
        new, res, _ = capi.map_join_reference(st, src, dst, prior=prior, **opts)
        return new, res

    def close_loop(self, st, what, prior, handle, **opts):
        new, res, _ = capi.map_loop_reference(st, prior=prior, **opts)
        return new, res

    def localize(self, st, off, rows, priors, handle, q_max_rows, what):
        return capi.map_localize_reference(st, off, rows, priors, len(off) - 1, q_max_rows=q_max_rows, **LOCALIZE)["rec"]

    def relocalize(self, st, off, rows, what):
        return capi.map_relocalize_reference(st, off, rows, len(off) - 1)["rec"], None

    def snapshot(self, which, st, what):
        back = capi.map_snapshot_parse(capi.map_snapshot_pack(st), st["max_landmarks"], st["max_carry_rows"])
        assert capi.map_snapshot_pack(back) == capi.map_snapshot_pack(st), f"{what}: parse then pack is not the identity"
        return back

    def reset(self, which, what):
        return fresh(which)

    def check(self, states, what):
        for which, st in enumerate(states):
            invariants(st, self.lib, f"{what}, map {which}")


def invariants(st, lib, what=""):
    """What include/fx.h states as always true of a map's private state: fx_map_snapshot_check accepts its snapshot for the map's
    capacities (the block's sizes, n_landmarks <= n_needed, every alias word in [-1, n) and resolved, every carry word in [-1, n), n
    <= max_landmarks and r <= max_carry_rows); the snapshot parses back to the same bytes; alias[i] >= 0 exactly for the records
    that carry FX_MAP_LM_ABSORBED (fx_map_merge's fold), and an absorbed landmark's root is live."""
    blob = capi.map_snapshot_pack(st)
    if lib is not None:
        status = lib.fx_map_snapshot_check(blob, len(blob), st["max_landmarks"], st["max_carry_rows"])
        assert status == capi.FX_OK, f"{what}: fx_map_snapshot_check refuses the state: {lib.fx_last_error().decode()}"
    back = capi.map_snapshot_parse(blob, st["max_landmarks"], st["max_carry_rows"])
    assert capi.map_snapshot_pack(back) == blob, f"{what}: parse then pack is not the identity"
    for i, (a, r) in enumerate(zip(back["alias"], back["landmarks"])):
        assert (a >= 0) == bool(r["flags"] & capi.FX_MAP_LM_ABSORBED), f"{what}: landmark {i}: alias {a}, flags {r['flags']:#x}"
        assert a < 0 or back["alias"][a] == -1, f"{what}: alias[{i}] = {a} is not live"
    return blob


# ---- the walk
def walk(seed, be, steps=None, check_read_only=True):
    """Runs plan(seed) (or `steps`) through the backend `be`, checking after every step.  Returns (the two final states, the log:
    per step a dict step, call, map, options, result, effective).  A failure is a WalkError whose message carries the seed, the
    step and the log so far: plan(seed)[:step + 1] replays it."""
    w, pieces, pieces2 = world()
    steps = plan(seed) if steps is None else steps
    st = [fresh(MAIN), fresh(SECOND)]
    fed = [0, 0]
    find = reloc = None  # the main map's last find / relocalize with no state-changing call since: (record, handle, options)
    log = []
    for k, (call, which, o) in enumerate(steps):
        what = f"seed {seed}, step {k}: {call} {o}"
        try:
            before = capi.map_snapshot_pack(st[which]) if call in READ_ONLY and check_read_only else None
            n0 = st[which]["header"]["n_landmarks"]
            if call == "update":
                p = (pieces, pieces2)[which][fed[which]]
                s = st[which]
                if which == SECOND and s["header"]["scans"] == 0:  # the second session starts from its own pose
                    s = au.with_header(s, last_pose=tuple(WORLD["init_pose2"]) + (0, 0))
                st[which], ids = be.update(which, s, p, o["overlap"], what)
                fed[which] += 1
                r = dict(rows_with_id=int((np.asarray(ids) >= 0).sum()), added=st[which]["header"]["n_landmarks"] - n0,
                         n=st[which]["header"]["n_landmarks"], segments=st[which]["header"]["segments"])
            elif call == "merge":
                st[which], res = be.merge(which, st[which], what, max_gap_scans=o["max_gap_scans"])
                r = _ints(res, ("proposals", "merged", "live"))
            elif call == "compact":
                st[MAIN], res = be.compact(st[MAIN], what, min_obs=o["min_obs"], min_age_scans=o["min_age_scans"])
                r = _ints(res, ("before", "kept", "dropped_absorbed", "dropped_live"))
            elif call == "append":
                st[MAIN], res = be.append(st[MAIN], st[SECOND], o["via"], what)
                r = _ints(res, ("id_base", "segment_base", "appended", "flags"))
            elif call == "find_loop":
                opts = FIND[o["kind"]]
                rec, handle = be.find(st[MAIN], what, **opts)
                find = (rec, handle, o)
                r = _ints(rec, ("flags", "score", "runner_up", "n_query", "n_targets"))
            elif call in ("join", "close_loop"):
                kind = "cross" if call == "join" else "same"
                prior = handle = None
                if find is not None and find[2]["kind"] == kind and int(find[0]["flags"]) & capi.FX_FIND_VALID:
                    prior, handle = fu.transform_of(find[0]), find[1] if o["device"] else None
                opts = dict(search_dist=0.6) if prior is not None else {}
                if call == "join":
                    SEG = st[MAIN]["header"]["segments"]
                    src = max(SEG - 1, 1)
                    dst = 0 if o["dst"] == "first" else max(src - 1, 0)
                    st[MAIN], res = be.join(st[MAIN], src, dst, what, prior, handle, **opts)
                else:
                    st[MAIN], res = be.close_loop(st[MAIN], what, prior, handle, **dict(lu.OPTS, **opts))
                r = dict(_ints(res, ("flags", "n_corr", "n_inliers", "moved")), prior="find" if prior is not None else "identity",
                         device=prior is not None and bool(o["device"]))
            elif call in ("localize", "relocalize"):
                p = pieces[o["piece"]]
                off = [int(x) for x in p["off"]]
                if o.get("scan") is not None:
                    s = o["scan"]
                    off_, rows, scan0 = np.array([0, off[s + 1] - off[s]], np.uint32), p["rows"][off[s]:off[s + 1]], p["scan0"] + s
                else:
                    off_, rows, scan0 = p["off"], p["rows"], p["scan0"]
                if call == "relocalize":
                    rec, handle = be.relocalize(st[MAIN], off_, rows, what)
                    reloc = (rec, handle, o)
                    r = dict(valid=int((rec["flags"] & capi.FX_RELOC_VALID).astype(bool).sum()), score=int(rec["score"][0]))
                else:
                    handle, handed = None, False
                    if o.get("scan") is not None and reloc is not None and (reloc[2]["piece"], reloc[2]["scan"]) == (o["piece"], o["scan"]):
                        priors, handle, handed = np.ascontiguousarray(reloc[0]["pose"]), reloc[1] if o["device"] else None, True
                    else:
                        priors = llu.poses_of(w["truth"][scan0:scan0 + len(off_) - 1], seed=o.get("seed", 1000 + k))
                    rec = be.localize(st[MAIN], off_, rows, priors, handle, WIDE_ROWS if o.get("wide") else len(rows), what)
                    r = dict(valid=int((rec["flags"] & capi.FX_LOC_VALID).astype(bool).sum()), scans=len(rec), prior="relocalize" if handed else "truth",
                             device=handed and bool(o["device"]))
            elif call == "snapshot":
                r = dict(n_landmarks=n0)
                st[which] = be.snapshot(which, st[which], what)
            elif call == "reset":
                r = dict(n_landmarks=n0)
                st[which] = be.reset(which, what)
                fed[which] = 0
            else:
                raise KeyError(call)
            if which == MAIN and call in CHANGING:
                find = reloc = None
            if before is not None:
                assert capi.map_snapshot_pack(st[which]) == before, "a read-only call changed the state"
            log.append(dict(step=k, call=call, map=which, options=o, result=r, effective=effective(call, r), n_main=st[MAIN]["header"]["n_landmarks"]))
            be.check(st, what)
        except WalkError:
            raise
        except Exception as e:
            raise WalkError(f"{what}: {e}\nthe log so far (replay with plan({seed})[:{k + 1}]):\n{describe(log)}") from e
    return st, log


# ---- the census
def census(logs):
    """logs: {seed: log}.  Returns a dict:
    counts       {call: [effective, ineffective]} over all walks and both maps
    second_merges the merges of the second map among them
    pairs        {(A, B): [times adjacent, times with both effective]}: state-changing calls that ran directly after one another on
                 the main map; read-only calls and calls on the second map in between do not break adjacency
    between      {(A, R, B)}: the adjacent pairs that had the read-only call R between them
    after_second {seed: the main map's calls that ran directly after a merge on the second map (the other capacity's carve)}
    generations  {seed: the walk holds GENERATIONS as a subsequence of its effective steps on the main map}
    largest      {seed: the most landmarks the main map held}"""
    counts = {c: [0, 0] for c in CALLS}
    second_merges = 0
    pairs, between, after_second, generations, largest = {}, set(), {}, {}, {}
    for seed, log in logs.items():
        prev, mids, want = None, [], 0
        after_second[seed], largest[seed] = set(), 0
        for i, e in enumerate(log):
            counts[e["call"]][0 if e["effective"] else 1] += 1
            if e["map"] == SECOND and e["call"] == "merge":
                second_merges += 1
            if e["map"] == SECOND:
                continue
            if i and log[i - 1]["map"] == SECOND and log[i - 1]["call"] == "merge":
                after_second[seed].add(e["call"])
            largest[seed] = max(largest[seed], e["n_main"])
            if e["effective"] and want < len(GENERATIONS) and e["call"] == GENERATIONS[want]:
                want += 1
            if e["call"] in READ_ONLY:
                mids.append(e["call"])
                continue
            if e["call"] not in CHANGING:
                continue
            if prev is not None:
                cell = pairs.setdefault((prev["call"], e["call"]), [0, 0])
                cell[0] += 1
                cell[1] += int(prev["effective"] and e["effective"])
                between.update((prev["call"], r, e["call"]) for r in mids)
            prev, mids = e, []
        generations[seed] = want == len(GENERATIONS)
    return dict(counts=counts, second_merges=second_merges, pairs=pairs, between=between, after_second=after_second, generations=generations, largest=largest)


# ---- the context's shared scratch: a model of csrc's carve functions, for the growth test
SEEDS = (16, 197, 97, 297, 257, 85, 26, 11, 212, 9, 175)  # the committed walks (tests/test_map_walk_reference.py states what they meet)
GROWTH_SEED = 16
SCRATCH_MIN = 4096
SCRATCH_SLACK = 2048  # above the leading terms below: the state words, the block sums, the result record, 16-byte rounding


def scratch_need(e):
    """(lower, upper) bounds of the bytes the step's call reserves of the context's one map scratch (c->merge_scratch), from the
    leading terms of the fxk_map_*_scratch functions: the merge's grid is 56 B a landmark of max_landmarks and 8 B a bucket (cand
    32, keep 8, bucket, prop, pred, succ 4 each; count and start); localize adds 12 B a row of q_max_rows behind it; join and
    close_loop 16 B a landmark and 4096 B of correspondences; relocalize and find_loop carve two grids, 3 KiB of keypoints, seeds
    and partials and a byte a landmark; compact stages 48 + 64 B a landmark and keeps 8 B a landmark: the true size lies within
    SCRATCH_SLACK above these.  fx_map_append_host stages the source's snapshot there, which the log does not size: between
    nothing and the snapshot of a full second map (160 B of headers, 116 B a landmark, 20 B a carry row).  fx_map_append needs
    its state words only, fx_map_update has a buffer of its own, reset, export and import use none."""
    cap, table = (WORLD["cap"], 1024) if e["map"] == MAIN else (WORLD["cap2"], 256)
    grid = 56 * cap + 8 * (table + 1)
    call, o = e["call"], e["options"]
    need = None
    if call == "merge":
        need = grid
    elif call == "compact":
        need = 120 * cap
    elif call == "localize":
        if not o.get("wide"):  # q_max_rows is the rows of the scans localised: at most a piece's, under 512
            return grid, grid + 12 * 512 + SCRATCH_SLACK
        need = grid + 12 * WIDE_ROWS
    elif call in ("join", "close_loop"):
        need = grid + 16 * cap + 4096
    elif call in ("find_loop", "relocalize"):
        need = 2 * grid + 3072 + cap
    elif call == "append":
        return (0, 256 + 116 * WORLD["cap2"] + 20 * WORLD["carry2"] + SCRATCH_SLACK) if o["via"] == "snapshot" else (0, SCRATCH_SLACK)
    return (0, 0) if need is None else (need, need + SCRATCH_SLACK)


def scratch_growths(log, first=SCRATCH_MIN):
    """The steps at which DevScratch::reserve certainly replaces the buffer (max(need, twice the old size, 4096) bytes) when the
    buffer holds `first` bytes before the walk: a step counts only if the lower bound of its need exceeds the largest size the
    buffer can have by then.  A step that may or may not grow it only widens what the buffer can be."""
    lo = hi = first
    out = []
    for e in log:
        need_lo, need_hi = scratch_need(e)
        if need_lo > hi:
            out.append(e["step"])
            lo, hi = max(need_lo, 2 * lo), max(need_hi, 2 * hi)
        elif need_hi > lo:  # it may grow: a buffer below the need is replaced by less than twice the need
            hi = max(hi, 2 * need_hi)
    return out


def growth_between_find_and_consumer(log, grown):
    """The (find_loop, growth, join or close_loop) step triples of a walk's log: the consumer takes the find's result from the device
    and the scratch grows at a step between the two."""
    out = []
    for e in log:
        if e["call"] in ("join", "close_loop") and e["result"]["prior"] == "find" and e["result"]["device"]:
            f = max(x["step"] for x in log if x["call"] == "find_loop" and x["step"] < e["step"])
            out += [(f, g, e["step"]) for g in grown if f < g < e["step"]]
    return out
