"""tests/pileup_model.py (the rule of `pbsim --pileup-bam`) held to values worked out by hand and to properties on seeded random
inputs, and the places where the feature shows without a GPU: the ABI's declarations with their ctypes mirror and the built
library's symbols, pbsim_pileup_report against the model, the option mirror with the command line's refusals, the checks in front
of any device work, and the HIP-free rule file under the sanitizers."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import bam_writer as B
import errors_model as E
import harness
import pbsim3_amd as P
import pileup_model as M
from pbsim3_amd import args as A

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def rec(name, pos, cigar, seq="", flag=0, ref=0, mapq=60, qual=None, tags=()):
    """qual None: no qualities (0xFF)"""
    ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    return B.record(name, flag, ref, pos, cigar=ops, seq=seq, qual=bytes([255] * len(seq)) if qual is None else qual, tags=tags, mapq=mapq)


# ---------------------------------------------------------------- the worked case of the rule
# g1, prepared: A C G T A C G T T T N A C G T (the T run has class 3, N class 1); g2: G G C A T T A C (G G and T T class 2).
# g1 0 .. 3   a1 ACGT, a2 ACTT: position 2 has G 1, T 1: a tie the genome's own class wins.
# g1 4, 5     a3 CC, a4 TC: position 4 (A) has C 1, T 1: a tie the first in the order wins: the call is C, a sub_site.
# g1 6 .. 8   a5 G, -T, +A, T and a6 GTT: position 7 has T 1, del 1, ins 1: the tie with del goes to the genome's T; 2 ins == depth:
#             no ins_site.  The insertion comes behind a D.
# g1 9 .. 11  a7 T, +C, = over the genome's N (other), A: position 9 has depth 1 and ins 1: 2 ins == depth + 1, an ins_site.
# g1 11 .. 14 a8 A R G T ends at l_ref; R is other: position 12 has depth 1, all five cells 0: the call is the genome's C.
# g2 0 .. 2   b1 2S1I3M: the insertion behind S is unanchored; its qualities 5 5 5 | 19 20 30.  b2 1I2M: unanchored too.
# g2 2 .. 5   b3 C, 2N, +T, T: the insertion behind N anchors at 4, which nothing covers: depth 0, low.  Position 3 is bare.
# g2 5 .. 7   b4 T +A P +A A C: two I ops at anchor 5; b5 T -A C; b6 -A C: position 5 has T 3, ins 2: 4 > 3, an ins_site;
#             position 6 has A 1, del 2: a del_site.
# u1 unaligned, s1 secondary, m1 runs past l_ref, z1 lies on a reference the genome lacks.
# discordant 4 of called 20: 200000 ppm, -10 log10(0.2) = 6.9897.
GENOME = [("g1", b"ACGTac\ngtTTNACGT\n"), ("g2", b"GGCATTAC\n")]
WORKED_REFS = [("g1", 15), ("g2", 8), ("zz", 50)]
WORKED = [rec("a1", 0, "4M", "ACGT", mapq=7),
          rec("a2", 0, "4M", "ACTT"),
          rec("a3", 4, "2M", "CC"),
          rec("a4", 4, "2M", "TC"),
          rec("a5", 6, "1M1D1I1M", "GAT"),
          rec("a6", 6, "3M", "GTT"),
          rec("a7", 9, "1M1I2M", "TC=A"),
          rec("a8", 11, "4M", "ARGT"),
          rec("u1", -1, "", "ACG", flag=4, ref=-1),
          rec("s1", 0, "3M", "TTT", flag=0x100),
          rec("m1", 13, "5M", "GTACG"),
          rec("z1", 0, "3M", "ACG", ref=2),
          rec("b1", 0, "2S1I3M", "TTAGGC", ref=1, qual=bytes([5, 5, 5, 19, 20, 30])),
          rec("b2", 1, "1I2M", "AGC", ref=1),
          rec("b3", 2, "1M2N1I1M", "CTT", ref=1),
          rec("b4", 5, "1M1I1P1I2M", "TAAAC", ref=1),
          rec("b5", 5, "1M1D1M", "TC", ref=1),
          rec("b6", 6, "1D1M", "C", ref=1)]
WORKED_COUNTS = [18, 1, 1, 0, 1, 15, 0, 1, 14]
WORKED_SITES = [23, 1, 2, 20, 18, 1, 1, 2, 4]
WORKED_CELLS = [
    [[2, 0, 0, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0, 0, 0], [0, 0, 0, 2, 0, 0, 0, 0], [0, 1, 0, 1, 0, 0, 0, 0],
     [0, 2, 0, 0, 0, 0, 0, 0], [0, 0, 2, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 1, 1, 0], [0, 0, 0, 2, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 1, 0],
     [0, 0, 0, 0, 1, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0, 0]],
    [[0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 2, 0, 0, 0, 0, 0], [0, 3, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 1, 0],
     [0, 0, 0, 3, 0, 0, 2, 0], [1, 0, 0, 0, 0, 2, 0, 0], [0, 3, 0, 0, 0, 0, 0, 0]]]
WORKED_SITES_TEXT = (b"g1\t5\tA\t2\t0\t1\t0\t1\t0\t0\t0\t0\tC\tsub\n"
                     b"g1\t10\tT\t1\t0\t0\t0\t1\t0\t0\t1\t0\tT\tmatch+ins\n"
                     b"g2\t6\tT\t3\t0\t0\t0\t3\t0\t0\t2\t0\tT\tmatch+ins\n"
                     b"g2\t7\tA\t3\t1\t0\t0\t0\t0\t2\t0\t0\t*\tdel\n")
WORKED_ALL_TEXT = (b"g1\t1\tA\t2\t2\t0\t0\t0\t0\t0\t0\t0\tA\tmatch\n"
                   b"g1\t2\tC\t2\t0\t2\t0\t0\t0\t0\t0\t0\tC\tmatch\n"
                   b"g1\t3\tG\t2\t0\t0\t1\t1\t0\t0\t0\t0\tG\tmatch\n"
                   b"g1\t4\tT\t2\t0\t0\t0\t2\t0\t0\t0\t0\tT\tmatch\n"
                   b"g1\t5\tA\t2\t0\t1\t0\t1\t0\t0\t0\t0\tC\tsub\n"
                   b"g1\t6\tC\t2\t0\t2\t0\t0\t0\t0\t0\t0\tC\tmatch\n"
                   b"g1\t7\tG\t2\t0\t0\t2\t0\t0\t0\t0\t0\tG\tmatch\n"
                   b"g1\t8\tT\t2\t0\t0\t0\t1\t0\t1\t1\t0\tT\tmatch\n"
                   b"g1\t9\tT\t2\t0\t0\t0\t2\t0\t0\t0\t0\tT\tmatch\n"
                   b"g1\t10\tT\t1\t0\t0\t0\t1\t0\t0\t1\t0\tT\tmatch+ins\n"
                   b"g1\t11\tN\t1\t0\t0\t0\t0\t1\t0\t0\t0\t.\tref_n\n"
                   b"g1\t12\tA\t2\t2\t0\t0\t0\t0\t0\t0\t0\tA\tmatch\n"
                   b"g1\t13\tC\t1\t0\t0\t0\t0\t1\t0\t0\t0\tC\tmatch\n"
                   b"g1\t14\tG\t1\t0\t0\t1\t0\t0\t0\t0\t0\tG\tmatch\n"
                   b"g1\t15\tT\t1\t0\t0\t0\t1\t0\t0\t0\t0\tT\tmatch\n"
                   b"g2\t1\tG\t1\t0\t0\t1\t0\t0\t0\t0\t0\tG\tmatch\n"
                   b"g2\t2\tG\t2\t0\t0\t2\t0\t0\t0\t0\t0\tG\tmatch\n"
                   b"g2\t3\tC\t3\t0\t3\t0\t0\t0\t0\t0\t0\tC\tmatch\n"
                   b"g2\t4\tA\t0\t0\t0\t0\t0\t0\t0\t0\t0\t.\tlow\n"
                   b"g2\t5\tT\t0\t0\t0\t0\t0\t0\t0\t1\t0\t.\tlow\n"
                   b"g2\t6\tT\t3\t0\t0\t0\t3\t0\t0\t2\t0\tT\tmatch+ins\n"
                   b"g2\t7\tA\t3\t1\t0\t0\t0\t0\t2\t0\t0\t*\tdel\n"
                   b"g2\t8\tC\t3\t0\t3\t0\t0\t0\t0\t0\t0\tC\tmatch\n")
WORKED_REPORT = (b"# records=18 skipped_flag=1 unaligned=1 skipped_mapq=0 skipped_ref=1 aligned=15 no_seq=0 misfit=1 scored=14\n"
                 b"S\t23\t1\t2\t20\t18\t1\t1\t2\t4\t200000\t6989\n"
                 b"C\t5\t11\t7\t12\t2\t3\t5\t0\t2\t3\n"
                 b"HP\t1\t14\t1\t1\t0\nHP\t2\t3\t0\t0\t1\nHP\t3\t3\t0\t0\t1\n")
# the options moved off their defaults, one at a time: what changes (dicts of the model's keyword arguments)
WORKED_OPTIONS = [dict(min_baseq=20), dict(min_baseq=21), dict(min_depth=2), dict(min_depth=3), dict(min_depth=0), dict(min_mapq=8),
                  dict(exclude_flags=0), dict(fmt="all"), dict(fmt="all", min_baseq=31, min_depth=2, exclude_flags=0x10, min_mapq=7)]


def sparse(values):
    return {k: v for k, v in enumerate(values) if v}


def worked(**kw):
    return M.pileup(B.stream(WORKED, WORKED_REFS), GENOME, **kw)


def test_the_worked_case():
    r = worked()
    assert r.counts == WORKED_COUNTS and r.sites == WORKED_SITES
    assert r.cell_sums == [5, 11, 7, 12, 2, 3, 5, 0] and r.ins_unanchored == 2 and r.max_depth == 3
    assert sparse(r.hp_called) == {1: 14, 2: 3, 3: 3} and sparse(r.hp_sub) == {1: 1} and sparse(r.hp_del) == {1: 1} and sparse(r.hp_ins) == {2: 1, 3: 1}
    assert [c.tolist() for c in r.cells] == WORKED_CELLS and all(c.dtype == np.uint32 for c in r.cells)
    assert r.text == WORKED_SITES_TEXT and r.report == WORKED_REPORT
    every = worked(fmt="all")
    assert every.text == WORKED_ALL_TEXT and every[:9] == r[:9] and every.report == r.report
    # qualities: b1's first aligned base has 19, the second 20.  At min_baseq 20 the first is masked, at 21 both; a1 .. b6 have none
    q20, q21 = worked(min_baseq=20), worked(min_baseq=21)
    assert q20.cells[1][0].tolist() == [0, 0, 0, 0, 0, 0, 0, 1] and q20.cells[1][1].tolist() == [0, 0, 2, 0, 0, 0, 0, 0]
    assert q21.cells[1][1].tolist() == [0, 0, 1, 0, 0, 0, 0, 1] and q21.cell_sums[7] == 2 and worked(min_baseq=255).cell_sums[7] == 3
    assert q20.sites == [23, 1, 3, 19, 17, 1, 1, 2, 4] and q20.cells[0].tolist() == WORKED_CELLS[0]
    assert q20.report.splitlines()[1] == b"S\t23\t1\t3\t19\t17\t1\t1\t2\t4\t210526\t6766"
    # depth: a site of depth 2 is called at min_depth 2 and low at 3
    assert worked(min_depth=2).sites == [23, 1, 7, 15, 13, 1, 1, 1, 3] and worked(min_depth=3).sites == [23, 1, 18, 4, 3, 0, 1, 1, 2]
    assert worked(min_depth=2).text == b"".join(WORKED_SITES_TEXT.splitlines(True)[k] for k in (0, 2, 3))
    # at min_depth 0 the two bare sites are called, as the genome's base; the one with an insertion and depth 0 is an ins_site
    zero = worked(min_depth=0, fmt="all")
    assert zero.sites == [23, 1, 0, 22, 20, 1, 1, 3, 5]
    assert b"g2\t4\tA\t0\t0\t0\t0\t0\t0\t0\t0\t0\tA\tmatch\n" in zero.text and b"g2\t5\tT\t0\t0\t0\t0\t0\t0\t0\t1\t0\tT\tmatch+ins\n" in zero.text
    # the record classes are the errors rule's
    assert worked(min_mapq=7).counts == WORKED_COUNTS and worked(min_mapq=8).counts == [18, 1, 1, 1, 1, 14, 0, 1, 13]
    assert worked(min_mapq=8).cells[0][:4].tolist() == [[1, 0, 0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0, 0]]
    assert worked(exclude_flags=0).counts == [18, 0, 1, 0, 1, 16, 0, 1, 15] and worked(exclude_flags=0).cells[0][0].tolist() == [2, 0, 0, 1, 0, 0, 0, 0]
    errs = E.errors(B.stream(WORKED, WORKED_REFS), GENOME)
    assert errs.counts[:9] == WORKED_COUNTS
    # two files give what one gives, in either order; a file's only reference goes by the name given for it
    two = M.pileup([B.stream(WORKED[9:], WORKED_REFS), B.stream(WORKED[:9], WORKED_REFS)], GENOME)
    assert two[:-3] == r[:-3] and [c.tolist() for c in two.cells] == WORKED_CELLS and two.text == r.text and two.report == r.report
    named = M.pileup(B.stream(WORKED[:8], [("ref", 15)]), GENOME, ref_names=["g1"], fmt="all")
    assert [c.tolist() for c in named.cells] == [WORKED_CELLS[0], [[0] * 8] * 8] and named.counts == [8, 0, 0, 0, 0, 8, 0, 0, 8]
    assert M.pileup(B.stream(WORKED[:8], [("ref", 15)]), GENOME).counts == [8, 0, 0, 0, 8, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="exactly one"):
        M.pileup(B.stream(WORKED, WORKED_REFS), GENOME, ref_names=["g1"])
    with pytest.raises(ValueError, match="l_ref 16, 15 bases"):
        M.pileup(B.stream(WORKED, [("g1", 16), ("g2", 8), ("zz", 50)]), GENOME)
    with pytest.raises(ValueError, match="two records named"):
        M.pileup(B.stream(WORKED, WORKED_REFS), GENOME + [("g1", b"AC")])


def test_ties_and_the_ins_threshold_cell_by_cell():
    """classify() on cells written down directly: every tie, and 2 ins against depth on both sides"""
    seq = np.frombuffer(b"ACGTNAAAAC", np.uint8)
    hp = np.ones(10, np.uint8)
    cells = np.array([[3, 3, 0, 0, 0, 3, 0, 0],      # A C del tie on A: the genome's
                      [3, 0, 3, 0, 0, 3, 0, 0],      # A G del tie on C: the first, A: sub
                      [0, 0, 1, 2, 0, 2, 0, 0],      # T del tie on G: T before del: sub
                      [0, 2, 0, 1, 0, 2, 9, 0],      # C del tie on T: C: sub, and 18 > 5
                      [9, 0, 0, 0, 0, 0, 9, 0],      # N: ref_n whatever lies there
                      [0, 0, 0, 0, 7, 1, 4, 0],      # del 1 on A, other 7: del; 2 * 4 == 8: no ins_site
                      [0, 0, 0, 0, 6, 1, 4, 0],      # 8 > 7: del+ins
                      [0, 0, 0, 0, 0, 0, 1, 5],      # depth 0 (masked is no part of it)
                      [2 ** 32 - 1, 0, 0, 0, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 0],   # depth 3 * (2^32 - 1): 64-bit
                      [0, 0, 0, 0, 0, 0, 0, 0]], np.int64)
    depth, call, cls, ins = M.classify(cells, seq, hp, 1)
    assert depth.tolist() == [9, 9, 5, 5, 9, 8, 7, 0, 3 * (2 ** 32 - 1), 0]
    assert call.tolist() == [0, 0, 3, 1, -1, 4, 4, -1, 0, -1]
    assert [M.CLASS_NAMES[k] for k in cls] == ["match", "sub", "sub", "sub", "ref_n", "del", "del", "low", "match", "low"]
    assert ins.tolist() == [False, False, False, True, False, False, True, False, False, False]


# ---------------------------------------------------------------- properties, on seeded random inputs
def small_case(seed, n=120, files=3):
    from test_gpu_bam_errors import aligned, noisy_ops, planted
    rng = random.Random(seed)
    seqs = {0: planted(rng, 3000), 1: planted(rng, 600) + b"NNnn" + planted(rng, 90).lower() + b"RYacgt"}
    genome = [("s0", seqs[0]), ("s1", seqs[1][:400] + b"\n" + seqs[1][400:])]
    refs = [("s0", len(seqs[0])), ("s1", len(seqs[1]))]
    recs = []
    for k in range(n):
        ref = k % 2
        ops = noisy_ops(rng, rng.choice([1, 2, 3, 5, 8, 30, 70]))
        if k % 9 == 0:
            ops = [(rng.randrange(1, 3), "I")] + ops                  # a leading insertion
        if k % 11 == 0:
            ops = [(2, "S"), (1, "I")] + ops
        span = sum(m for m, op in ops if op in "MDN=X")
        recs.append(aligned("q%d" % k, ops, pos=rng.randrange(max(1, len(seqs[ref]) - span)), ref=ref, rng=rng, seqs=seqs,
                            flag=[0, 16, 0x100, 0, 4, 0][k % 6], mapq=rng.randrange(60), qual="none" if k % 4 == 1 else "random",
                            placeholder=k % 13 == 5))
    return genome, refs, recs, rng


@pytest.mark.parametrize("seed", [3, 4])
def test_properties_on_random_inputs(seed):
    genome, refs, recs, rng = small_case(seed)
    whole = M.pileup(B.stream(recs, refs), genome, fmt="all")
    assert whole.counts[8] > 50 and whole.ins_unanchored > 5 and whole.sites[7] > 0 and whole.sites[5] > 0
    # permuting records and files changes nothing
    mixed = list(recs)
    rng.shuffle(mixed)
    cut = sorted(rng.sample(range(len(mixed)), 2))
    parts = [B.stream(mixed[:cut[0]], refs), B.stream(mixed[cut[0]:cut[1]], refs), B.stream(mixed[cut[1]:], refs)]
    again = M.pileup(parts[::-1], genome, fmt="all")
    assert again[:-3] == whole[:-3] and all((a == b).all() for a, b in zip(again.cells, whole.cells))
    assert again.text == whole.text and again.report == whole.report
    # the sums against the CIGARs of the scored records, and against the errors rule on the same input
    errs = E.errors(B.stream(recs, refs), genome)
    totals = dict(zip(E.TOTAL_NAMES, errs.totals))
    for min_baseq in (0, 30):
        r = M.pileup(B.stream(recs, refs), genome, min_baseq=min_baseq)
        assert sum(r.cell_sums[:5]) + r.cell_sums[7] == sum(errs.pair) == totals["cols"] - totals["ins"] - totals["del"]
        assert r.cell_sums[5] == totals["del"] and r.cell_sums[6] + r.ins_unanchored == totals["ins_events"]
        assert (r.cell_sums[7] == 0) == (min_baseq == 0) and r.counts == errs.counts[:9]
        assert r.sites[1] + r.sites[2] + r.sites[3] == r.sites[0] == sum(len(c) for c in r.cells)
        assert r.sites[3] == r.sites[4] + r.sites[5] + r.sites[6] == sum(r.hp_called) and r.sites[8] <= r.sites[5] + r.sites[6] + r.sites[7]
        assert r.text.count(b"\n") == r.sites[8]
    assert whole.text.count(b"\n") == whole.sites[0]


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_calls_and_the_library_has_them():
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        h = f.read()
    assert re.search(r"int pbsim_bam_pileup\(pbsim_ctx \*ctx, const pbsim_errors_ref \*refs, int n_refs, const pbsim_errors_file \*files, int n_files,\s*"
                     r"const pbsim_pileup_opts \*opts, const pbsim_pileup_sink \*sink, pbsim_pileup_result \*result\);", h)
    assert re.search(r"int64_t pbsim_pileup_report\(const pbsim_pileup_result \*result, char \*buf, int64_t cap\);", h)
    assert re.search(r"typedef struct pbsim_pileup_opts \{[^;]*int32_t exclude_flags, min_mapq, min_baseq;\s*int32_t format;[^;]*\s*int64_t min_depth;\s*"
                     r"int64_t piece_bytes;", h)
    assert "modulo 2^32" in h and len(re.findall(r"typedef struct pbsim_errors_ref \{", h)) == 1
    body = re.search(r"typedef struct pbsim_pileup_result \{(.*?)\} pbsim_pileup_result;", h, re.S).group(1)
    declared = []
    for names in re.findall(r"int64_t ([^;]+);", body):
        for item in names.split(","):
            name, dims = re.match(r"\s*(\w+)((?:\[\d+\])*)", item).groups()
            declared.append((name, int(dims[1:-1]) if dims else 1))
    mirrored = [(n, C.sizeof(t) // 8) for n, t in P.PileupResult._fields_]
    assert declared == mirrored and C.sizeof(P.PileupResult) == 8 * sum(n for _, n in declared)
    assert mirrored == [("counts", 9), ("sites", 9), ("cell_sums", 8), ("ins_unanchored", 1), ("max_depth", 1)] + [(n, 12) for n in M.HP_ARRAYS]
    bound = [name for name, _, _ in P.API]
    assert "pbsim_bam_pileup" in bound and "pbsim_pileup_report" in bound
    assert [n for n, _ in P.PileupOpts._fields_] == ["exclude_flags", "min_mapq", "min_baseq", "format", "min_depth", "piece_bytes"]
    assert C.sizeof(P.PileupOpts) == 32 and [n for n, _ in P.PileupSink._fields_] == ["user", "on_text", "on_cells"]
    assert (P.PILEUP_COUNTS, P.PILEUP_SITES, P.PILEUP_CELLS, P.PILEUP_HP) == (M.COUNT_NAMES, M.SITE_NAMES, M.CELL_NAMES, M.HP_ARRAYS)
    assert list(P.PILEUP_FORMATS) == list(M.FORMATS) and callable(getattr(P.Context, "bam_pileup")) and callable(P.pileup_report)
    lib = P.load()
    assert hasattr(lib, "pbsim_bam_pileup") and hasattr(lib, "pbsim_pileup_report")


def as_dict(r):
    return dict(counts=r[0], sites=r[1], cell_sums=r[2], ins_unanchored=r[3], max_depth=r[4], hp_called=r[5], hp_sub=r[6], hp_del=r[7], hp_ins=r[8])


def random_result(rng):
    pick = lambda: rng.choice([0, 0, 1, 10 ** 12, rng.randrange(2 ** 50)])
    sites = [pick() for _ in range(9)]
    sites[3] = sites[8] + pick()                    # called >= discordant, as a result has it: the ppm value stays inside 64 bits
    return [[rng.randrange(2 ** 31) for _ in range(9)], sites, [pick() for _ in range(8)], pick(), pick()] + [[pick() for _ in range(12)] for _ in range(4)]


ZERO = [[0] * 9, [0] * 9, [0] * 8, 0, 0, [0] * 12, [0] * 12, [0] * 12, [0] * 12]
ZERO_REPORT = (b"# records=0 skipped_flag=0 unaligned=0 skipped_mapq=0 skipped_ref=0 aligned=0 no_seq=0 misfit=0 scored=0\n"
               b"S" + b"\t0" * 10 + b"\t*\nC" + b"\t0" * 10 + b"\n")


def test_report_of_the_library_is_the_models_without_a_device():
    r = worked()
    assert P.pileup_report(as_dict(r)) == WORKED_REPORT
    by_name = as_dict(r)
    by_name.update(counts=dict(zip(M.COUNT_NAMES, r.counts)), sites=dict(zip(M.SITE_NAMES, r.sites)), cell_sums=dict(zip(M.CELL_NAMES, r.cell_sums)))
    assert P.pileup_report(by_name) == WORKED_REPORT
    assert M.report(*ZERO) == ZERO_REPORT == P.pileup_report(as_dict(ZERO))
    rng = random.Random(41)
    for _ in range(30):
        x = random_result(rng)
        assert P.pileup_report(as_dict(x)) == M.report(*x)
    # the quality: 1 of 10, 1 of 1, 999999 of 1000000, more discordant than called (the struct is not held to the rule)
    for d, c, want in ((1, 10, b"100000\t10000"), (1, 1, b"1000000\t0"), (999999, 10 ** 6, b"999999\t0"), (0, 5, b"0\t*"), (5, 0, b"0\t*"),
                       (20, 10, b"2000000\t-3011")):
        x = [list(v) if isinstance(v, list) else v for v in ZERO]
        x[1] = [0, 0, 0, c, 0, 0, 0, 0, d]
        assert M.report(*x).splitlines()[1].endswith(b"\t" + want) and P.pileup_report(as_dict(x)) == M.report(*x)
    assert P.load().pbsim_pileup_report(None, None, 0) == -1
    with pytest.raises(ValueError, match="sites has 8 values"):
        P.pileup_report(dict(as_dict(ZERO), sites=[0] * 8))


# ---------------------------------------------------------------- the option mirror and the command line
GOOD = ["--pileup-bam", "in.bam", "--pileup-genome", "g.fa"]
REFUSED = [
    (GOOD + ["--depth", "3"], "(--depth): --pileup-bam takes"),
    (GOOD + ["--errors-out", "x"], "(--errors-out): --pileup-bam takes"),
    (["--pileup-out", "o", "--pileup-bam"], "needs a value"),
    (["--pileup-bam", "in.bam"], "--pileup-bam needs --pileup-genome FASTA"),
    (GOOD + ["--pileup-min-mapq", "256"], "(pileup-min-mapq: 256): a whole number, 0 .. 255"),
    (GOOD + ["--pileup-min-baseq", "-1"], "(pileup-min-baseq: -1): a whole number, 0 .. 255"),
    (GOOD + ["--pileup-min-baseq", "256"], "(pileup-min-baseq: 256): a whole number, 0 .. 255"),
    (GOOD + ["--pileup-min-depth", "x"], "(pileup-min-depth: x): a whole number"),
    (GOOD + ["--pileup-min-depth", "-2"], "(pileup-min-depth: -2): a whole number"),
    (GOOD + ["--pileup-format", "vcf"], "(pileup-format: vcf): sites or all"),
    (GOOD + ["--pileup-ref-names", "a,b"], "(pileup-ref-names): 2 names for 1 --pileup-bam files"),
    (GOOD + ["--pileup-bam", "b.bam", "--pileup-ref-names", "a,"], "(pileup-ref-names): an empty name"),
    (GOOD + ["--devices", "0,1"], "--pileup-bam runs on one GPU"),
    (GOOD + ["--processes", "2"], "--pileup-bam runs on one GPU"),
]


def test_option_mirror_accepts_and_rejects():
    assert A.pileup_bam(GOOD) == dict(bams=["in.bam"], genome="g.fa", ref_names=None, out=None, fmt="sites", min_mapq=0, min_baseq=0, min_depth=1)
    got = A.pileup_bam(["--pileup-out", "o", "--pileup-bam", "a", "--pileup-min-mapq", "255", "--pileup-bam", "b", "--pileup-min-baseq", "20",
                        "--pileup-genome", "g", "--pileup-ref-names", "x,y", "--device", "1", "--pileup-format", "all", "--pileup-min-depth", "0"])
    assert got == dict(bams=["a", "b"], genome="g", ref_names=["x", "y"], out="o", fmt="all", min_mapq=255, min_baseq=20, min_depth=0)
    for argv, message in REFUSED + [(["--pileup-genome", "g"], "--pileup-bam FILE: name the BAM file")]:
        with pytest.raises(ValueError) as e:
            A.pileup_bam(argv)
        assert message in str(e.value), argv


def test_cli_refuses_from_the_command_line_alone(tmp_path):
    """the same refusals by the binary, with the mirror's words, before a device or a file is touched"""
    import pbsim3_amd.build as b
    b.build()
    for argv, message in REFUSED:
        r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and r.stdout == "" and message in r.stderr, (argv, r.stderr[-500:])
    r = subprocess.run([CLI] + GOOD + ["--pileup-out", "o.tsv"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "Cannot open file: in.bam" in r.stderr
    (tmp_path / "in.bam").write_bytes(B.bam(WORKED, WORKED_REFS))
    r = subprocess.run([CLI] + GOOD + ["--pileup-out", "o.tsv"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "--pileup-genome g.fa: Cannot open file: g.fa" in r.stderr
    assert os.listdir(tmp_path) == ["in.bam"]
    r = subprocess.run([CLI], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert "--pileup-bam FILE [--pileup-bam FILE ...] --pileup-genome FASTA" in r.stderr + r.stdout


# ---------------------------------------------------------------- the checks in front of any device work
def test_bad_arguments_fail_before_device_work():
    data = B.bam(WORKED, WORKED_REFS)
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), -1) as c:
        for kw, word in ((dict(min_mapq=256), "min_mapq must be 0 .. 255"), (dict(exclude_flags=65536), "exclude_flags must be 0 .. 65535"),
                         (dict(min_baseq=256), "min_baseq must be 0 .. 255"), (dict(min_baseq=-1), "min_baseq must be 0 .. 255"),
                         (dict(min_depth=-1), "min_depth must not be negative"), (dict(piece_bytes=-1), "piece_bytes must not be negative")):
            with pytest.raises(P.PbsimError, match="pbsim_bam_pileup: " + word):
                c.bam_pileup(data, GENOME, **kw)
        with pytest.raises(ValueError, match="fmt must be sites or all"):
            c.bam_pileup(data, GENOME, fmt="vcf")
        opts = P.PileupOpts(0x900, 0, 0, 2, 1, 0)
        refs = (P.ErrorsRef * 1)(P.ErrorsRef(b"g", C.cast(C.c_char_p(b"ACGT"), C.c_void_p), 4))
        arr = (P.ErrorsFile * 1)(P.ErrorsFile(C.cast(C.c_char_p(data), C.c_void_p), len(data), None))
        res = P.PileupResult()
        assert c.lib.pbsim_bam_pileup(c.h, refs, 1, arr, 1, C.byref(opts), None, C.byref(res)) == 0
        assert b"pbsim_bam_pileup: format must be 0 (sites) or 1 (all)" in c.lib.pbsim_last_error()
        with pytest.raises(P.PbsimError, match="pbsim_bam_pileup: bad argument"):
            c.bam_pileup([], GENOME)
        with pytest.raises(P.PbsimError, match="pbsim_bam_pileup: bad argument"):
            c.bam_pileup(data, [])
        with pytest.raises(P.PbsimError, match=r"pbsim_bam_pileup: the genome holds two records named \"g1\" \(records 0 and 2\)"):
            c.bam_pileup(data, GENOME + [("g1", b"AC")])
        with pytest.raises(ValueError, match="one entry per file"):
            c.bam_pileup(data, GENOME, ref_names=["a", "b"])
        # good arguments reach the device check: a tables-only context refuses as pbsim_inflate_buffer does, and stays usable
        for kw in (dict(), dict(text=True, arrays=True), dict(min_mapq=255, min_baseq=255, min_depth=0, fmt="all", ref_names=["g1", None])):
            with pytest.raises(P.PbsimError, match="no HIP device"):
                c.bam_pileup([data, data], GENOME, **kw)


# ---------------------------------------------------------------- the host's decisions under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("asan") / "bam_pileup_rule_driver")
    p = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(harness.ROOT, "tests", "asan", "bam_pileup_rule_driver.cpp"), os.path.join(csrc, "bam_pileup_rule.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if p.returncode != 0 and "sanitize" in p.stderr:
        pytest.skip("no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def drive(exe, *argv):
    p = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, timeout=60)
    assert p.returncode == 0, (argv, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout


def flat(x):
    return [v for part in x for v in (part if isinstance(part, list) else [part])]


def test_rule_code_under_asan(driver):
    assert drive(driver, "opts", "-") == b"opts 2304 0 0 0 1 8388608\n"
    assert drive(driver, "opts", 0, 255, 255, 1, 0, 7) == b"opts 0 255 255 1 0 7\n"
    for bad, word in (((65536, 0, 0, 0, 1, 0), b"exclude_flags"), ((-1, 0, 0, 0, 1, 0), b"exclude_flags"), ((4, 256, 0, 0, 1, 0), b"min_mapq"),
                      ((4, -1, 0, 0, 1, 0), b"min_mapq"), ((4, 0, 256, 0, 1, 0), b"min_baseq"), ((4, 0, -1, 0, 1, 0), b"min_baseq"),
                      ((4, 0, 0, 2, 1, 0), b"format"), ((4, 0, 0, -1, 1, 0), b"format"), ((4, 0, 0, 0, -1, 0), b"min_depth"),
                      ((4, 0, 0, 0, 1, -1), b"piece_bytes")):
        assert drive(driver, "opts", *bad).startswith(b"opts refused: " + word), bad
    assert drive(driver, "report", *flat(list(worked()[:9]))) == WORKED_REPORT
    assert drive(driver, "report", *flat(ZERO)) == ZERO_REPORT
    rng = random.Random(42)
    for _ in range(5):
        x = random_result(rng)
        assert drive(driver, "report", *flat(x)) == M.report(*x)
