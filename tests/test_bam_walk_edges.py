"""One small BAM whose records sit on every edge of the CIGAR column walk the BAM stages share (pbsim3_amd/csrc/bam_cigar.h): the
rounds of 64 ops, the blocks of kErrSegOps ops, the segments of kErrSegCols columns, and a CIGAR given through the CG tag.  Here
the input goes through the models alone, and the sums that tie the stages to each other are asserted, so that the input is known
to be consistent before tests/test_gpu_bam_walk_edges.py gives it to the device."""
import functools
import random

import numpy as np

import bam_writer as B
import consensus_model as KM
import depth_model as DM
import errors_model as EM
import lift_model as LM
import pileup_model as PM
import stats_model as SM
from test_gpu_bam_errors import aligned
from test_gpu_bam_grid_caps import constant
from test_lift_model import header_text

SEG_OPS, SEG_COLS = constant("bam_errors.h", "kErrSegOps"), constant("bam_errors.h", "kErrSegCols")
L_REF = 900


def mixed(n, start=0):
    """n ops of one base each: M, = or X between I and D in turn; 3 reference bases per 4 ops"""
    return [(1, "M=X"[(k // 2) % 3]) if k % 2 == 0 else (1, "ID"[(k // 2) % 2]) for k in range(start, start + n)]


def edge_cigars():
    """name -> (pos, ops, through the CG placeholder)"""
    out = {"one_op": (40, [(700, "M")], False)}                                   # the long M the second origin map cuts twice
    for n in (63, 64, 65, SEG_OPS - 1, SEG_OPS, SEG_OPS + 1, 2 * SEG_OPS + 1):
        out["ops%d" % n] = (n % 50, mixed(n), False)
    c = SEG_COLS
    out["m_crosses"] = (3, [(10, "M"), (c - 16, "I"), (20, "M")], False)         # the second M lies on columns c - 6 .. c + 13
    out["i_first"] = (5, [(5, "M"), (c - 10, "I"), (5, "X"), (3, "I"), (5, "M")], False)    # the second I op begins at column c
    out["i_last"] = (7, [(5, "M"), (c - 12, "I"), (5, "M"), (2, "I"), (5, "M")], False)     # the second I op ends at column c - 1
    out["i_leads"] = (9, [(3, "I"), (20, "M"), (2, "I"), (4, "M")], False)                  # nothing of the reference in front
    out["d_crosses"] = (11, [(10, "M"), (c - 20, "I"), (6, "M"), (10, "D"), (10, "M")], False)   # the D lies on c - 4 .. c + 5
    big = [(1, "M") if k % 94 == 0 else (1, "I") for k in range(65700)]                     # 699 reference bases
    out["cg_big"] = (1, big, True)
    return out


@functools.lru_cache(maxsize=None)
def edge_case():
    """(stream, genome, refs): a genome of L_REF bases and the records of edge_cigars on it, with qualities and true NM tags"""
    rng = random.Random(2025)
    seq = bytes(rng.choice(b"ACGT") for _ in range(L_REF))
    recs = []
    for k, (name, (pos, ops, through_cg)) in enumerate(edge_cigars().items()):
        assert pos + sum(n for n, op in ops if op in "MDN=X") <= L_REF, name
        recs.append(aligned(name, ops, pos=pos, rng=random.Random(k), placeholder=through_cg, seqs={0: seq}, qual="none" if k % 5 == 4 else "random"))
    refs = [("edge", L_REF)]
    return B.stream(recs, refs=refs, text=header_text(refs)), [("edge", seq)], refs


def origin_maps():
    """the identity, and a map with original bases 150 and 151 deleted and two bases inserted in front of original base 400: both
    inside one_op's M, and the variant record keeps its length"""
    same = np.arange(L_REF, dtype=np.int32)
    cut = list(range(L_REF))
    del cut[150:152]
    at = cut.index(400)
    cut[at:at] = [-1 - 399] * 2
    cut = np.array(cut, dtype=np.int32)
    assert len(cut) == L_REF and LM.check_origin(cut, L_REF) is None and LM.check_origin(same, L_REF) is None
    return {"identity": same, "cut": cut}


@functools.lru_cache(maxsize=None)
def models():
    """every stage's model over the case, computed once for the tests of both files"""
    stream, genome, _ = edge_case()
    out = {"stats": SM.stats([stream]), "errors": EM.errors([stream], genome), "depth": DM.depth(stream),
           "pileup": dict(zip(PM.FORMATS, PM.pileup([stream], genome, fmt="both"))), "consensus": KM.consensus([stream], genome)}
    for name, origin in origin_maps().items():
        out["lift_" + name] = LM.lift_stream(stream, genome, [origin])
    return out


def column_sums(errors_totals, pile_cells, pile_unanchored):
    """the sums both stages must agree on, from {name: value} of errors' totals and pileup's cell sums: the M and D columns, the I ops"""
    e_md = errors_totals["cols"] - errors_totals["ins"]
    p_md = sum(pile_cells[n] for n in ("A", "C", "G", "T", "other", "del", "masked"))       # the depths, deletions and masked bases
    return (e_md, errors_totals["ins_events"]), (p_md, pile_cells["ins"] + pile_unanchored)


def test_the_case_has_its_edges():
    cig = edge_cigars()
    assert sorted(len(ops) for _, ops, _ in cig.values())[:4] == [1, 3, 4, 5]
    for n in (1, 63, 64, 65, SEG_OPS - 1, SEG_OPS, SEG_OPS + 1, 2 * SEG_OPS + 1):
        assert any(len(ops) == n for _, ops, _ in cig.values()), n
    assert len(cig["cg_big"][1]) > 65535 and cig["cg_big"][2]

    def columns(name):
        out = []
        for n, op in cig[name][1]:
            out += [op] * n if op in "MID=X" else []
        return out
    c = SEG_COLS
    assert columns("m_crosses")[c - 1] == columns("m_crosses")[c] == "M" and columns("m_crosses")[c - 7] == "I"
    assert columns("i_first")[c - 1] == "X" and columns("i_first")[c:c + 3] == ["I"] * 3
    assert columns("i_last")[c - 2:c] == ["I"] * 2 and columns("i_last")[c - 3] == columns("i_last")[c] == "M"
    assert columns("i_leads")[0] == "I"
    assert columns("d_crosses")[c - 4:c + 6] == ["D"] * 10 and columns("d_crosses")[c - 5] == columns("d_crosses")[c + 6] == "M"
    assert {op for _, ops, _ in cig.values() for _, op in ops} == set("MID=X")


def test_the_models_agree_across_the_stages():
    m = models()
    n = len(edge_cigars())
    stats, errors, depth, pile = m["stats"], m["errors"], m["depth"], m["pileup"]["sites"]
    assert dict(zip(SM.COUNT_NAMES, stats.counts))["scored"] == n
    assert dict(zip(EM.COUNT_NAMES, errors.counts))["scored"] == dict(zip(EM.COUNT_NAMES, errors.counts))["nm_agree"] == n
    assert dict(zip(DM.COUNT_NAMES, depth.counts))["counted"] == n
    assert dict(zip(PM.COUNT_NAMES, pile.counts))["scored"] == n and pile.ins_unanchored == 1
    assert m["consensus"].counts == pile.counts
    e_totals, p_cells = dict(zip(EM.TOTAL_NAMES, errors.totals)), dict(zip(PM.CELL_NAMES, pile.cell_sums))
    ours, theirs = column_sums(e_totals, p_cells, pile.ins_unanchored)
    assert ours == theirs
    cols = sum(sum(k for k, op in ops if op in "MID=X") for _, ops, _ in edge_cigars().values())
    assert e_totals["cols"] == cols == dict(zip(SM.TOTAL_NAMES, stats.totals))["cols"]
    for name in origin_maps():
        res = m["lift_" + name][1]
        assert res["lifted"] == res["records"] == n and res["cols_in"] == cols and res["long_cigar_in"] == 1
    same, cut = m["lift_identity"][1], m["lift_cut"][1]
    assert same["gap_del"] == same["bases_to_ins"] == same["dels_vanished"] == 0
    assert same["m"] == e_totals["cols"] - e_totals["ins"] - e_totals["del"]     # (I and D columns outside the M columns leave the core)
    assert cut["gap_del"] > 0 and cut["bases_to_ins"] > 0 and cut["moved"] > 0
