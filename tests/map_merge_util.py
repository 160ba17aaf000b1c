"""Helpers of the map merge tests (tests/test_map_merge_reference.py, tests/test_gpu_map_merge.py): the flicker world of the
issue, hand-built fragments with exact means, and the comparison of a device map (records, alias) with a capi.map_merge_reference
state."""
import numpy as np

from feature_extraction_amd import capi
from tests import map_util as mu
from tests import track_util as tu

FLICKER = dict(seed=72, n_poles=40, n_scans=24, dropout=0.25, sigma=0.01, step=5, cap=128, carry=64)
MAX_CALLS = 4  # calls of map_merge_reference the flicker world needs at most before one merges nothing (checked on the CPU)


def flicker():
    """The world of the issue (40 poles, 24 scans, 25 % dropout, seed 72) cut every 5 scans.  Returns (w, pieces, the poles' xy)."""
    f = FLICKER
    w = tu.world(np.random.default_rng(f["seed"]), f["n_poles"], f["n_scans"], dropout=f["dropout"], sigma=f["sigma"])
    poles = np.random.default_rng(f["seed"]).uniform(0, 100.0, (f["n_poles"], 2))  # (world()'s first draw)
    return w, mu.split(w, mu.every(f["n_scans"], f["step"])), poles


def long_runs(w):
    """pole -> the rows of its runs of at least two observations (what the tracker makes landmarks of), in row order."""
    out = {}
    for run in tu.pole_runs(w):
        if len(run) >= 2:
            out.setdefault(int(w["pole"][run[0]]), []).extend(run)
    return {k: sorted(v) for k, v in out.items()}


def merge_to_fixpoint(state, max_calls=MAX_CALLS, **kw):
    """map_merge_reference until a call merges nothing.  Returns (state, the results of all calls)."""
    results = []
    for _ in range(max_calls + 1):
        state, res = capi.map_merge_reference(state, **kw)
        results.append(res)
        if res["merged"] == 0:
            return state, results
    raise AssertionError(f"no fixpoint after {max_calls + 1} calls: {results}")


def resolve(ids, alias):
    """map_id_of_row words through the alias table."""
    ids = np.asarray(ids).astype(np.int64)
    a = np.asarray(alias, np.int64)
    out = ids.copy()
    has = ids >= 0
    via = a[ids[has]]
    out[has] = np.where(via >= 0, via, ids[has])
    return out


def fragments(frags, n_scans, bad=(), length=2, seed=7):
    """A track_util case of identity motions holding one chain of `length` identical observations for every (first_scan, x, y) of
    frags (float32 values: the means are exact), good links except those in `bad`.  Landmark ids follow (first_scan, order in
    frags).  Returns the case; w["chains"][k] are fragment k's (scan, i) rows."""
    h = tu.Hand(n_scans)
    chains = [h.chain(int(fs), length) for fs, _, _ in frags]
    w = h.finish(np.random.default_rng(seed), motions=[(0.0, 0.0, 0.0, 0.0)] * (n_scans - 1))
    for (_, x, y), ch in zip(frags, chains):
        for r in ch:
            w["rows"][w["at"](r), :3] = (x, y, 1.0)
    for b in bad:
        w["reg"]["flags"][b] = 0
    w["chains"] = chains
    return w


def ids_of(w, row_ids):
    """The map id of every fragment of a fragments() case from the update's map_id_of_row."""
    return [int(row_ids[w["at"](ch[0])]) for ch in w["chains"]]


def reference_of(w, cap=None, carry=None):
    """fragments() case -> (map_reference state after its one batch, the fragments' ids)."""
    n = len(w["rows"])
    st, _, ids = mu.run_reference([w], cap or max(n, 1), carry or max(n, 1))
    return st, ids_of(w, ids[0])


def state_bytes(st):
    r = capi.map_state_records(st)
    return repr(sorted(r["header"].items())).encode() + r["landmarks"].tobytes() + np.array(st.get("alias", []), np.int32).tobytes() + \
        np.array(st["carry"], np.int32).tobytes() + b"".join(np.array(a, np.float64).tobytes() for a in st["acc"])


def assert_alias(got, st, what=""):
    """A device alias table (all max_landmarks words) against the state's: equal where stored, -1 beyond."""
    ref = np.full(len(got), -1, np.int32)
    a = np.array(st.get("alias", []), np.int32)
    ref[:len(a)] = a
    bad = np.flatnonzero(got != ref)
    assert not len(bad), f"{what}: alias differs at {bad[:8].tolist()}: got {got[bad[:8]]}, reference {ref[bad[:8]]}"
