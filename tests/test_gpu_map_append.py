"""fx_map_append and fx_map_append_host on the GPU.  Every call is compared with capi.map_append_reference: the result word for
word and the target's whole private state through the snapshot, Map.export_state() against capi.map_snapshot_pack byte for byte
(records, sums, alias, carry, the carry scan, the header); the source's snapshot and the guard words about the result must be
untouched.  The maps hold a few hundred landmarks at most and the context never processes a batch."""
import struct

import pytest

from feature_extraction_amd import capi
from tests import map_append_util as au
from tests import map_find_loop_util as fu
from tests import map_merge_util as mm
from tests.map_append_util import _append
from tests.test_gpu_map import _step
from tests.test_gpu_map_compact import _compact, _same_state
from tests.test_gpu_map_find_loop import _find
from tests.test_gpu_map_join import _join
from tests.test_gpu_map_merge import _merge_to_fixpoint
from tests.test_gpu_track import FILL, GUARD

pytestmark = pytest.mark.gpu
A, CD, EMPTY, OVER, NOROOM, LONG, TOP = au.A, au.CD, au.EMPTY, au.OVER, au.NOROOM, au.LONG, au.TOP


@pytest.fixture
def ctx(fxlib):
    c = capi.Context(capi.params("launch"), capi.limits(2, 1024))  # (no batch is ever processed on it)
    yield c
    c.close()


def _map_of(ctx, st):
    mp = ctx.map_create(st["max_landmarks"], st["max_carry_rows"])
    mp.import_state(capi.map_snapshot_pack(st))
    return mp


def _pair(ctx, dst_st, src_st, what):
    """The two states as device maps, src appended to dst.  Returns (dst, src, the new state, the result)."""
    dst, src = _map_of(ctx, dst_st), _map_of(ctx, src_st)
    pointers = (dst.device_pointers(), dst.alias_device_pointer())
    st, res = _append(ctx, dst, dst_st, src_st, what, src=src)
    assert (dst.device_pointers(), dst.alias_device_pointer()) == pointers, f"{what}: the target's addresses are stable"
    return dst, src, st, res


# ---- (a) the reference's cases on the device
def test_a1_the_flicker_world_in_two_sessions_equals_the_one_run(ctx):
    f = mm.FLICKER
    _, pieces, _ = mm.flicker()
    for cut in au.cuts(pieces):
        a, b, one = au.two_sessions(pieces, cut, f["cap"], f["carry"])
        dst, src, st, res = _pair(ctx, a, b, f"(a1) cut {cut}")
        assert res["flags"] == A and dst.export_state() == capi.map_snapshot_pack(one), f"(a1) cut {cut}: the device's map is the one run's"
        dst.close(), src.close()


def test_a2_a_merged_source_and_a_merged_target(ctx):
    merged = au.merged_flicker()
    dst, src, st, res = _pair(ctx, au.hand(5, cap=128), merged, "(a2) merged source")
    assert res["flags"] == A and st["alias"][5:] == [a + 5 if a >= 0 else -1 for a in merged["alias"]]
    assert (dst.alias()[:5] == -1).all() and (dst.alias()[5 + len(merged["alias"]):] == -1).all()
    dst.close(), src.close()
    dst, src, st, res = _pair(ctx, merged, au.hand(7, salt=3), "(a2) merged target")
    assert res["flags"] == A and st["alias"][:len(merged["alias"])] == merged["alias"]
    dst.close(), src.close()


def test_a3_the_carry_fits_exactly_or_is_dropped(ctx):
    _, b, _ = au.flicker_sessions()
    r = b["header"]["carry_rows"]
    for carry, flags, rows in ((r, A, r), (r - 1, A | CD, 0)):
        dst, src, st, res = _pair(ctx, au.hand(3, cap=128, carry=carry), b, f"(a3) max_carry_rows {carry}")
        assert res["flags"] == flags and res["carry_rows"] == rows == dst.header()["carry_rows"]
        dst.close(), src.close()


# ---- (b) workgroup and vector edges: 256 landmarks a workgroup, 7 vectors a landmark; N + M == max_landmarks exactly
@pytest.mark.parametrize("n,m", [(0, 1), (1, 0), (255, 2), (256, 1), (257, 255), (1, 513)])
def test_b_workgroup_and_vector_edges(ctx, n, m):
    dst_st = au.hand(n, cap=n + m) if n else capi.map_state(n + m, 8)
    src_st = au.hand(m, salt=5)
    assert src_st["header"]["scans"] > 0
    dst, src, st, res = _pair(ctx, dst_st, src_st, f"(b) {n} + {m}")
    assert res["flags"] == A and res["id_base"] == n and res["appended"] == m and st["header"]["n_landmarks"] == n + m == dst.max_landmarks
    dst.close(), src.close()


# ---- (c) refusals on the device
def test_c_every_device_refusal_leaves_the_target_unchanged(ctx):
    dst_st, src_st = au.hand(4, cap=16), au.hand(3, salt=2)
    s = src_st["header"]
    cases = [(dst_st, capi.map_state(4, 4), EMPTY), (dst_st, au.with_caps(au.with_header(src_st, n_needed=5), cap=3), OVER),
             (au.with_caps(au.with_header(dst_st, n_needed=9), cap=4), au.hand(0), OVER), (au.with_caps(dst_st, cap=6), src_st, NOROOM),
             (au.with_caps(au.with_header(dst_st, n_needed=9, scans=TOP), cap=4), au.with_caps(au.with_header(src_st, n_needed=5), cap=3), OVER | NOROOM | LONG)]
    cases += [(au.with_header(dst_st, **{k: TOP - s[k] + 1}), src_st, LONG) for k in ("scans", "segments", "batches", "n_obs")]
    for k, (d, sr, flags) in enumerate(cases):
        dst, src = _map_of(ctx, d), _map_of(ctx, sr)
        before = dst.export_state()
        st, res = _append(ctx, dst, d, sr, f"(c) case {k}", src=src)
        assert res["flags"] == flags and res["appended"] == 0 and dst.export_state() == before, f"(c) case {k}"
        dst.close(), src.close()
    # the edges on the side that applies: N + M == max_landmarks, a count that sums to 2^32 - 1
    for d in (au.with_caps(dst_st, cap=7), au.with_header(dst_st, scans=TOP - s["scans"]), au.with_header(dst_st, n_obs=TOP - s["n_obs"])):
        dst, src, st, res = _pair(ctx, d, src_st, "(c) the edge that applies")
        assert res["flags"] == A
        dst.close(), src.close()


# ---- (d) the snapshot as the source
def test_d_append_state_is_append(ctx):
    merged = au.merged_flicker()
    dst_st = au.hand(5, cap=128, carry=64)
    dst, src, st, res = _pair(ctx, dst_st, merged, "(d) append")
    want = dst.export_state()
    data = src.export_state()
    assert data == capi.map_snapshot_pack(merged)
    other = _map_of(ctx, dst_st)
    before = other.export_state()
    # refused before anything is staged: a truncated block, a bad magic, more landmarks than the target holds
    small = _map_of(ctx, au.hand(2, cap=len(merged["landmarks"]) - 1))
    for mp, block, word in ((other, data[:-16], b"total bytes"), (other, struct.pack("<I", 0x12345678) + data[4:], b"magic"), (small, data, b"max_landmarks")):
        kept = mp.export_state()
        with pytest.raises(capi.FxError):
            mp.append_state(block)
        assert word in ctx.lib.fx_last_error(), ctx.lib.fx_last_error()
        ctx.synchronize()
        assert mp.export_state() == kept, word
    assert other.export_state() == before
    st2, res2 = _append(ctx, other, dst_st, merged, "(d) append_state", data=data)
    assert other.export_state() == want and res2 == res
    # a source whose carry scan is larger than the target's table: no bound on the carry rows in the check, dropped on the device
    _, b, _ = au.flicker_sessions()
    tight = _map_of(ctx, au.hand(3, cap=128, carry=2))
    _, res3 = _append(ctx, tight, au.hand(3, cap=128, carry=2), b, "(d) a carry that does not fit", data=capi.map_snapshot_pack(b))
    assert res3["flags"] == A | CD
    for mp in (dst, src, other, small, tight):
        mp.close()


# ---- (e) the live run is the source's
def test_e_the_sources_run_continues_on_the_target(ctx):
    f = mm.FLICKER
    _, pieces, _ = mm.flicker()
    a, b, _ = au.two_sessions(pieces[:4], 2, f["cap"], f["carry"])
    dst, src, st, res = _pair(ctx, a, b, "(e)")
    N = res["id_base"]
    src_next, _ = au.feed(b, pieces[4:5], flags=[True])
    st, _, ids = _step(ctx, dst, st, pieces[4], True, "(e) the next batch of the source's run, with overlap")
    assert not st["header"]["flags"] & capi.FX_MAP_OVERLAP_MISMATCH and st["header"]["last_joined"] == src_next["header"]["last_joined"] > 0
    k = len(pieces[4]["rows"])
    _, want = au.feed(b, pieces[4:5], flags=[True])
    got, want = ids[:k], want[0][:k]
    assert (want >= 0).any() and ((got >= 0) == (want >= 0)).all() and (got[got >= 0] == want[want >= 0] + N).all(), "the rows continue under ids + N"
    _same_state(dst, st, "(e) after the next update")
    dst.close(), src.close()


# ---- (f) the chain, and twice
def test_f_the_chain_on_the_device_and_equal_bytes_from_run_to_run(ctx):
    a, b = au.chain_sessions()
    ref = au.chain_reference(a, b)

    def once():
        dst, src, st, res = _pair(ctx, a, b, "(f) append")
        keep = {}
        find = _find(ctx, dst, st, "(f) find", keep=keep, segment=fu.LAST, target_segment=0, recent_scans=TOP)
        assert int(find["rec"]["flags"]) == capi.FX_FIND_VALID and int(find["rec"]["score"]) == 41
        st, join, _ = _join(ctx, dst, st, res["segment_base"], 0, "(f) join", prior_device=keep["result"], prior_ref=fu.transform_of(find["rec"]),
                            search_dist=0.6)
        assert int(join["flags"]) == 0x21 and int(join["n_inliers"]) == 41
        st, merges = _merge_to_fixpoint(ctx, dst, st, "(f) merge", max_gap_scans=1 << 20)
        st, remap, comp = _compact(ctx, dst, st, "(f) compact")
        assert comp["kept"] == 38
        out = dst.export_state()
        assert out == capi.map_snapshot_pack(ref["compacted"][0]), "(f) the final snapshot is the reference chain's"
        dst.close(), src.close()
        return out + keep["bytes"]
    assert once() == once()


# ---- (g) host refusals through the raw library
def test_g_host_refusals_launch_nothing(ctx, fxlib):
    import torch
    dst_st, src_st = au.hand(4, cap=16), au.hand(3, salt=2)
    dst, src = _map_of(ctx, dst_st), _map_of(ctx, src_st)
    other = capi.Context(capi.params("launch"), capi.limits(2, 1024))
    theirs = other.map_create(8, 8)
    out = torch.full((8 + GUARD,), FILL, dtype=torch.int32, device=f"cuda:{ctx.device}")
    res = out.data_ptr()
    data = capi.map_snapshot_pack(src_st)
    before = (dst.export_state(), src.export_state())
    for args, word in [((ctx.handle, dst.handle, theirs.handle, res), b"another context"), ((ctx.handle, theirs.handle, src.handle, res), b"another context"),
                       ((other.handle, dst.handle, src.handle, res), b"another context"), ((ctx.handle, dst.handle, dst.handle, res), b"same map"),
                       ((ctx.handle, dst.handle, src.handle, res + 2), b"aligned"), ((ctx.handle, dst.handle, None, res), b"null")]:
        assert fxlib.fx_map_append(*args) == capi.FX_ERR_INVALID_ARG and word in fxlib.fx_last_error(), (word, fxlib.fx_last_error())
    for args, word in [((ctx.handle, theirs.handle, data, len(data), res), b"another context"), ((ctx.handle, dst.handle, data, len(data), res + 1), b"aligned"),
                       ((ctx.handle, dst.handle, None, len(data), res), b"null")]:
        assert fxlib.fx_map_append_host(*args) == capi.FX_ERR_INVALID_ARG and word in fxlib.fx_last_error(), (word, fxlib.fx_last_error())
    ctx.synchronize()
    assert (out == FILL).all().item() and (dst.export_state(), src.export_state()) == before
    # result_device == NULL: nothing is reported
    assert fxlib.fx_map_append(ctx.handle, dst.handle, src.handle, None) == capi.FX_OK
    ctx.synchronize()
    st, _ = capi.map_append_reference(dst_st, src_st)
    assert (out == FILL).all().item()
    _same_state(dst, st, "(g) without a result")
    theirs.close(), other.close(), dst.close(), src.close()
