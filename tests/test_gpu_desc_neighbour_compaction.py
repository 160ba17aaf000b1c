"""The wavefront and group tiers of the descriptor stage the support set of a row with its neighbours (d2 < R^2) in front and
the shell out to the support radius behind them, and bin only the front (csrc/fx_kernels.hip: desc_wave_body, k_desc_group).
Hand-built scans pin the edges of that split against the oracle, bit for bit: every row's neighbour count and support count is
set exactly, by points the detector never sees (the builders: tests/desc_rows_util.py)."""
import pytest

from feature_extraction_amd import capi
from tests.desc_rows_util import GROUP_CAP, WAVE_CAP
from tests.desc_rows_util import compare as _compare, params as _params, scenes as _scenes

pytestmark = pytest.mark.gpu

# (neighbours, support points, how they are laid out)
#   "mixed": neighbours scattered among the shell points in scan order; "last": every neighbour behind every shell point (the
#   neighbours sit in the last chunk of the stored list); "origin": one of the neighbours IS the keypoint (d2 = 0: counted, never binned)
GROUP_CASES = [(0, 0, "mixed"), (0, 20, "mixed"), (1, 30, "mixed"), (15, 40, "mixed"), (16, 48, "mixed"), (17, 64, "mixed"),
               (63, 64, "mixed"), (64, 64, "mixed"), (5, 40, "last"), (10, 30, "origin"), (1, 1, "origin")]
WAVE_CASES = [(0, 100, "mixed"), (1, 130, "mixed"), (15, 150, "mixed"), (16, 192, "mixed"), (17, 70, "mixed"), (63, 130, "mixed"),
              (64, 192, "mixed"), (65, 192, "mixed"), (WAVE_CAP, WAVE_CAP, "mixed"), (60, 130, "mixed"), (128, 129, "mixed"),
              (20, 190, "last"), (3, 192, "last"), (40, 100, "origin")]


@pytest.mark.parametrize("tier", ["group", "wave"])
def test_neighbour_counts_at_the_chunk_edges(fxlib, oracle, tier):
    cases = GROUP_CASES if tier == "group" else WAVE_CASES
    assert all(sup <= GROUP_CAP if tier == "group" else GROUP_CAP < sup <= WAVE_CAP for _, sup, _ in cases)
    p, scenes = _scenes(oracle, cases, 7)
    ctx = capi.Context(p, capi.limits(len(scenes), 1024))
    got = ctx.process_host([s for s, _ in scenes])
    for b, (_, ora) in enumerate(scenes):
        _compare(got[b], ora, f"{tier} tier, scan {b}")
    ctx.close()


def test_rows_reused_by_batches_of_other_shapes(fxlib, oracle):
    """A context's rows keep the bins the group tier wrote last time and un-write exactly those: three different batches through the
    same rows, every row changing its neighbour count, its support count and (most of them) its tier from batch to batch."""
    mixed = [c for pair in zip(GROUP_CASES, WAVE_CASES) for c in pair]
    batches = [mixed[0:8], mixed[8:16], list(reversed(mixed[0:8])), mixed[16:22] + mixed[0:2], mixed[0:8]]
    p = _params()
    ctx = capi.Context(p, capi.limits(2, 1024))
    for n, cases in enumerate(batches):
        _, scenes = _scenes(oracle, cases, 100 + n)
        got = ctx.process_host([s for s, _ in scenes])
        for b, (_, ora) in enumerate(scenes):
            _compare(got[b], ora, f"batch {n}, scan {b}")
    ctx.close()
