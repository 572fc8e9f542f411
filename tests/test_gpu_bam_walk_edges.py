"""The edge case of tests/test_bam_walk_edges.py through every caller of the shared CIGAR code (pbsim3_amd/csrc/bam_cigar.h) on the
device: bam_stats, bam_errors, bam_depth, bam_pileup, bam_consensus and bam_lift, each against its model, byte for byte, and the
sums that tie errors to the pileup taken from what the device returned.  The models run once (test_bam_walk_edges.models)."""
import numpy as np
import pytest

import bam_writer as B
import depth_model as DM
import lift_model as LM
import pbsim3_amd as P
import pileup_model as PM
import stats_model as SM
import test_gpu_bam_consensus as TK
import test_gpu_bam_errors as TE
import test_gpu_bam_pileup as TP
from test_bam_walk_edges import column_sums, edge_case, models, origin_maps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


@pytest.fixture(scope="module")
def bam():
    return B.W.bgzf(edge_case()[0])


def test_stats(ctx, bam):
    want = models()["stats"]
    counts, len_row, totals, hist_q, hist_identity, hist_qacc, report, text = ctx.bam_stats([bam], text=True)
    assert [counts[n] for n in SM.COUNT_NAMES] == want.counts
    assert [len_row[n] for n in SM.LEN_NAMES] == want.len_row
    assert [totals[n] for n in SM.TOTAL_NAMES] == want.totals
    assert (hist_q.tolist(), hist_identity.tolist(), hist_qacc.tolist()) == (want.hist_q, want.hist_identity, want.hist_qacc)
    assert text == want.text and report == want.report


def test_depth(ctx, bam):
    want = models()["depth"]
    text, counts, refs, hist, report, arrays = ctx.bam_depth(bam, arrays=True)
    assert [counts[n] for n in DM.COUNT_NAMES] == want.counts
    assert refs == want.refs and hist.tolist() == want.hist
    assert [a.tolist() for a in arrays] == want.arrays
    assert text == want.text and report == want.report


def test_errors_and_pileup_and_their_common_sums(ctx, bam):
    genome = edge_case()[1]
    want = models()["errors"]
    errors = ctx.bam_errors([bam], genome, text=True)
    TE.compare(errors, want)
    assert errors[2] == want.text
    piles = models()["pileup"]
    for fmt in PM.FORMATS:
        pile = ctx.bam_pileup([bam], genome, text=True, arrays=True, fmt=fmt)
        TP.compare(pile, piles[fmt])
        assert pile[2] == piles[fmt].text
        for mine, theirs in zip(pile[3], piles[fmt].cells):
            assert np.array_equal(mine.numpy(), theirs)
    ours, theirs = column_sums(errors[0]["totals"], pile[0]["cell_sums"], pile[0]["ins_unanchored"])
    assert ours == theirs


def test_consensus(ctx, bam):
    want = models()["consensus"]
    got = ctx.bam_consensus([bam], edge_case()[1])
    TK.compare(got, want)
    assert got[2] == want.text and got[3] == want.lengths


@pytest.mark.parametrize("name", ["identity", "cut"])
def test_lift(ctx, bam, name):
    want, res = models()["lift_" + name]
    got = ctx.lift_bam(bam, edge_case()[1], [origin_maps()[name]])
    assert got[0] == res and got[1] == LM.report(res)
    assert SM.inflate(got[2]) == want
