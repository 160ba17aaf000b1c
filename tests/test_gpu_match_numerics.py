"""fx_match_descriptors_csr at fp32's edges, on the GPU: the row families of tests/match_util.py (non-finite words, overflow,
cancellation, underflow, signs, thresholds at their edges), each held against capi.match_reference through match_util.compare
with require_all — tests/test_match_reference.py asserts on the CPU that no row of a family is ambiguous and that the reference
is within eps / 8 of the exact d2 — plus the exact assertions of each family, against match_util.exact_d2 where a value is
pinned.  Every case prints its worst |dist2 - exact| / eps."""
import numpy as np
import pytest

from feature_extraction_amd import capi
from tests import match_util as mu
from tests import test_gpu_match as gm
from tests import test_gpu_register as gr

pytestmark = pytest.mark.gpu
ACC, MUT = capi.FX_MATCH_ACCEPTED, capi.FX_MATCH_MUTUAL
ctx = gm.ctx


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _family(ctx, name, **opts):
    """The family matched on the GPU and compared with the shared reference: (got, ref, q, t, pairs, info)."""
    q, t, pairs, info, _ = mu.family(name)
    ref = mu.family_reference(name, **opts)
    got = gm._match(ctx, gm._device_block(mu.make_block(q)), gm._device_block(mu.make_block(t)), pairs, **opts)
    n = mu.compare(got, ref, require_all=True, what=f"{name} {opts}", **opts)
    assert n == int((ref["rec"]["train_row"] >= 0).sum())
    return got, ref, q, t, pairs, info


def _worst_against_exact(name, got, ref, q, t, rows=None):
    """max |dist2 - exact| / eps over the matched rows (all finite dist2), every one asserted <= 1, with exact from exact_d2."""
    worst = 0.0
    for i in (range(len(got)) if rows is None else rows):
        g = got[i]
        if g["train_row"] < 0 or not np.isfinite(g["dist2"]):
            continue
        x, _ = mu.exact_d2(q[i], t[g["train_row"]], g["shift"])
        eps = capi.match_epsilon(float(x), ref["nq2"][i], ref["nt2"][g["train_row"]])
        err = float(abs(mu.Fraction(float(g["dist2"])) - x))
        assert err <= eps, f"{name} row {i}: {g}, exact {float(x)}, off by {err} > eps {eps}"
        worst = max(worst, err / eps)
    print(f"{name}: worst |dist2 - exact| / eps = {worst:.3g}")
    return worst


def test_a_non_finite_words_never_match(ctx):
    q, t, pairs, info, _ = mu.family("nonfinite")
    qn, tn, _, _, _ = mu.family("nonfinite", nan=True)
    for opts in (dict(), dict(mutual=True)):
        got, ref, *_ = _family(ctx, "nonfinite", **opts)
        bad = info["q_bad"]
        assert (got["train_row"][bad] == -1).all() and (_bits(got["dist2"][bad]) == _bits(np.inf)).all() and not got["flags"][bad].any()
        assert (got["pair"][bad] == 0).all() and (got["second_row"][bad] == -1).all()
        assert not np.isin(got["train_row"], info["t_bad"]).any() and not np.isin(got["second_row"], info["t_bad"]).any()
        assert (got["train_row"] >= 0).sum() == 64 - len(bad)
        # differential: the same blocks with NaN where the infinities are
        nan = gm._match(ctx, gm._device_block(mu.make_block(qn)), gm._device_block(mu.make_block(tn)), pairs, **opts)
        assert got.tobytes() == nan.tobytes(), opts
        _worst_against_exact(f"(a) {opts}", got, ref, q, t)


def test_b_overflow_of_finite_rows(ctx):
    got, ref, q, t, pairs, info = _family(ctx, "overflow")
    for i in info["finite"]:  # +-W64 against the zero row: the largest finite d2, the exact value rounded once
        x, x32 = mu.exact_d2(q[i], t[0], 0)
        assert got["train_row"][i] == 0 and got["shift"][i] == 0 and _bits(got["dist2"][i]) == _bits(x32) and x32 < mu.FLT_MAX
    inf, copies = info["all_inf"], info["copies"]
    assert (_bits(got["dist2"][inf]) == _bits(np.inf)).all() and (_bits(got["dist2_second"][inf]) == _bits(np.inf)).all()
    assert (got["train_row"][:8] == 0).all() and (got["second_row"][:8] == 1).all()      # the lowest valid row, then the next
    assert (got["train_row"][8:40] == 3).all() and (got["second_row"][8:40] == 4).all() and not got["shift"][inf].any()
    assert (got["train_row"][56:] == 90).all() and (got["second_row"][56:] == 91).all()
    assert (got["train_row"][copies] == info["src"]).all() and (got["shift"][copies] == info["s"]).all()
    assert (got["flags"] == ACC).all()
    _worst_against_exact("(b)", got, ref, q, t)
    for opts in (dict(max_dist2=3e38), dict(max_ratio=0.5), dict(max_ratio=0.0), dict(mutual=True), dict(max_ratio=0.5, mutual=True)):
        g, rf, *_ = _family(ctx, "overflow", **opts)
        for f in ("train_row", "shift", "second_row", "flags", "pair"):
            assert (g[f] == rf["rec"][f]).all(), (opts, f)
        assert (_bits(g["dist2"]) == _bits(got["dist2"])).all()
        if "max_dist2" in opts:
            assert np.flatnonzero(g["flags"]).tolist() == copies, opts  # only the ordinary copies are below 3e38
        if opts.get("max_ratio") == 0.0:
            assert not g["flags"].any(), opts
        if "mutual" in opts:
            assert np.flatnonzero(g["flags"] & MUT).tolist() == [0, 8] + copies


def test_c_cancellation(ctx):
    got, ref, q, t, pairs, info = _family(ctx, "cancellation")
    src, s, moved = info["src"], info["s"], info["moved"]
    assert (got["train_row"] == src).all() and (got["shift"] == s).all() and (got["flags"] == ACC).all()
    assert (_bits(got["dist2"][:4]) == 0).all()  # the unmoved copy at shift 0: +0 bit for bit
    for i in range(4, 8):                        # the unmoved copy at another shift: within [0, eps]
        assert 0 <= got["dist2"][i] <= capi.match_epsilon(0.0, ref["nq2"][i], ref["nt2"][src[i]])
    _worst_against_exact("(c)", got, ref, q, t)
    print("(c) dist2 of the unmoved rotated copies:", got["dist2"][4:8], "of the moved ones, max:", got["dist2"][8:].max())


def test_d_underflow(ctx):
    got, ref, q, t, pairs, info = _family(ctx, "underflow")
    sub = 0
    for i in range(62):  # every sum the matcher forms on these rows is exact in fp64: one rounding, subnormals kept
        _, x32 = mu.exact_d2(q[i], t[got["train_row"][i]], got["shift"][i])
        assert _bits(got["dist2"][i]) == _bits(x32), (i, got[i], x32)
        sub += bool(0 < x32 < 2.0 ** -126)
    assert (got["train_row"][:6] == info["src"][:6]).all() and (got["shift"][:6] == info["s"][:6]).all() and (_bits(got["dist2"][:6]) == 0).all()
    assert (_bits(got["dist2"][48:60]) == 0).all() and (got["train_row"][48:60] == 100).all() and (got["second_row"][48:60] == 101).all()
    for i in info["hand"]:  # 1.5 * 2^-74 against zero: 4.5 * 2^-149, a tie that rounds to the even 4 * 2^-149
        assert got["train_row"][i] == 128 and _bits(got["dist2"][i]) == 4 and got["second_row"][i] == 129
    assert sub >= 10, "the family must produce subnormal results"
    print(f"(d) {sub} subnormal dist2 values kept by the device's fp64 -> fp32 conversion, none flushed")
    _worst_against_exact("(d)", got, ref, q, t)


def test_e_signs(ctx):
    got, ref, q, t, pairs, info = _family(ctx, "signs")
    for f in ("train_row", "shift", "second_row", "flags", "pair"):
        assert (got[f] == ref["rec"][f]).all(), f
    assert (got["train_row"][4:] == info["src"][4:]).all() and (got["shift"][4:] == info["s"][4:]).all()
    for i in info["negated"]:  # q = -t: 4 |t|^2 against its own row, so some other row is nearer
        assert got["train_row"][i] != i and float(mu.exact_d2(q[i], t[i], 0)[0]) == pytest.approx(4 * ref["nt2"][i], rel=1e-12)
    assert (_bits(q) == 0x80000000).sum() >= 100 and (_bits(t) == 0x80000000).sum() >= 200
    _worst_against_exact("(e)", got, ref, q, t)
    for opts in (dict(mutual=True), dict(shifts=1)):
        _family(ctx, "signs", **opts)


def _refused(ctx, q, t, pairs, **opts):
    """Context.match_descriptors must refuse these options on the host and write nothing: the output and the guard region
    behind it keep their fill pattern."""
    import torch
    n = int(q[1])
    raw = torch.full((n * 8 + gm.GUARD,), gr.FILL, dtype=torch.int32, device=f"cuda:{ctx.device}")
    torch.cuda.synchronize()
    with pytest.raises(capi.FxError, match="status 1"):
        ctx.match_descriptors(q, t, pairs, out=raw[:n * 8].view(n, 8), **opts)
    ctx.synchronize()
    assert (raw == gr.FILL).all().item(), opts


def test_f_thresholds_at_the_edges(ctx):
    seen = set()
    for opts in mu.THRESHOLDS:
        got, ref, *_ = _family(ctx, "thresholds", **opts)
        assert (got["flags"] == ref["rec"]["flags"]).all(), opts  # every row: zero and +inf distances are known bit for bit
        seen.add(tuple(got["flags"] & ACC))
    assert len(seen) >= 4
    for name, opts in (("overflow", dict(max_dist2=0.0)), ("overflow", dict(max_ratio=-0.5)), ("underflow", dict(max_dist2=0.0, mutual=True))):
        got, ref, *_ = _family(ctx, name, **opts)
        assert (got["flags"] == ref["rec"]["flags"]).all(), (name, opts)
    # a NaN threshold is refused on the host and nothing is written
    q, t, pairs, _, _ = mu.family("thresholds")
    qb, tb = gm._device_block(mu.make_block(q)), gm._device_block(mu.make_block(t))
    for opts in (dict(max_dist2=np.nan), dict(max_ratio=np.nan)):
        _refused(ctx, qb, tb, pairs, **opts)


def _kinds(d):
    """The kinds of fp32 distances in d: 0 zero, 1 subnormal, 2 normal, 3 +inf."""
    return {0 if x == 0 else 3 if np.isposinf(x) else 1 if x < 2.0 ** -126 else 2 for x in d}


@pytest.mark.parametrize("name,pair,kinds", [("overflow", 2, {2, 3}), ("cancellation", 0, {0, 2}), ("underflow", 0, {0, 1, 2})])
def test_g_registration_ranks_the_real_records(ctx, name, pair, kinds):
    """The matcher's own records through fx_register_matches, whose pool is ranked by the bits of dist2.  The records of `pair`
    mix the kinds of distance named (+0, subnormal, normal, +inf), the finite ones on distinct train rows, and hyp_corr stays
    below their number.  Under mu.ranking_keypoints the only sample of the true motion is the last two members of the pool, so
    a +inf or a subnormal ranked ahead of its place empties the pool of it: the pair must be valid with exactly the expected
    hyp_a, hyp_b and n_inliers at every hyp_corr (tests/test_match_reference.py shows on the CPU that a wrong rank changes
    them), and every record equals capi.register_reference bit for bit."""
    got, ref, q, t, pairs, _ = _family(ctx, name, mutual=True)
    q0, qn = pairs[pair][:2]
    d = got["dist2"][q0:q0 + qn]
    assert _kinds(d) == kinds and (got["train_row"][q0:q0 + qn] >= 0).all()
    finite = int(np.isfinite(d).sum())
    assert 4 < finite <= qn
    for H in range(2, finite - 1):
        q_kp, t_kp, exp = mu.ranking_keypoints(got, pairs, H, len(t))
        reg, _, _ = gr._run(ctx, q_kp, t_kp, got, pairs, f"(g) {name} hyp_corr {H}", hyp_corr=H)
        r = reg[pair]
        assert r["n_corr"] == qn > H and r["flags"] == gr.VALID and (r["hyp_a"], r["hyp_b"], r["n_inliers"]) == exp[pair], (H, r, exp)
    q_kp, t_kp, _ = mu.ranking_keypoints(got, pairs, 0, len(t))  # (nobody follows a motion: the records as they are)
    gr._run(ctx, q_kp, t_kp, got, pairs, f"(g) {name} no motion", hyp_corr=4, require_flags=0)
