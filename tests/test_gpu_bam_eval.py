"""`pbsim --eval-bam` (pbsim_truth_bam_eval; pbsim3_amd/csrc/bam_eval.hip, bam_eval.cpp): a mapper's BAM scored against truth BAMs on
the GPU.  Files built here with tests/bam_writer.py go through Context.eval_bam, and the counts, the MAPQ histogram, the verdict
bytes and the report text must be what tests/mapeval_model.py says, byte for byte; then the product's own truth files against
themselves and against a merged query, through the command line."""
import os
import random
import shutil
import subprocess

import pytest

import bam_spec_reader as R
import bam_writer as B
import harness
import mapeval_model as M
import pbsim3_amd as P
from cases import CASES

pytestmark = pytest.mark.gpu

TILE = 4096                     # bytes per workgroup of the record scan (bam_scan.h kBamTile)


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


def check(ctx, truths, query, ref_names=None, permille=100, container="bgzf", hash_bits=0, block=B.W.BGZIP_BLOCK, no_sink=False):
    """inflated streams -> through the product in `container`, against the model"""
    names = None if ref_names is None else [None if n is None else n.encode() for n in ref_names]
    want_counts, want_hist, want_verdicts = M.evaluate(truths, query, names, permille)
    containers = container if isinstance(container, (list, tuple)) else [container] * (len(truths) + 1)
    files = [B.contain(s, c, block) for s, c in zip(truths + [query], containers)]
    counts, hist, report, verdicts = ctx.eval_bam(files[:-1], files[-1], ref_names, overlap=permille / 1000, verdicts=True,
                                                  hash_bits=hash_bits)
    assert [counts[n] for n in M.COUNT_NAMES] == want_counts
    assert hist.shape == (256, 2) and hist.tolist() == want_hist
    assert verdicts.tobytes() == want_verdicts
    assert report == M.report(want_counts, want_hist)
    if no_sink:
        assert ctx.eval_bam(files[:-1], files[-1], ref_names, overlap=permille / 1000, hash_bits=hash_bits)[2] == report
    return dict(zip(M.COUNT_NAMES, want_counts)), want_verdicts


def cigar_over(rng, span, ops):
    """`ops` operations (ops >= 1) whose M / D / N / = / X lengths add up to `span` (span >= ops), insertions between them"""
    cuts = sorted(rng.sample(range(1, span), ops - 1)) if ops > 1 else []
    lens = [b - a for a, b in zip([0] + cuts, cuts + [span])]
    out = []
    for k, n in enumerate(lens):
        out.append((n, "MD=XN"[k % 5] if k % 7 else "M"))
    return out


def with_insertions(cigar, every=3):
    out = []
    for k, c in enumerate(cigar):
        out.append(c)
        if k % every == 0:
            out.append((1 + k % 4, "I"))
    return out


def truth_rec(name, ref, pos, cigar, flag=0, **kw):
    return B.record(name, flag, ref, pos, cigar=cigar, seq=kw.pop("seq", ""), qual=kw.pop("qual", b""), mapq=60, **kw)


def query_rec(rng, name, flag, ref, pos, span, **kw):
    """a mapped record as a mapper writes it: soft clips, bases, a MAPQ"""
    n = rng.randrange(1, 40)
    cigar = kw.pop("cigar", None) or [(3, "S")] + with_insertions(cigar_over(rng, span, min(span, rng.randrange(1, 9)))) + [(2, "S")]
    return B.record(name, flag, ref, pos, cigar=cigar, seq="ACGT"[n % 4] * n, qual=bytes([n]) * n, mapq=kw.pop("mapq", rng.choice([0, 1, 3, 20, 59, 60, 60, 255])),
                    tags=kw.pop("tags", (("NM", "C", n),)), **kw)


T_REFS = [("t0", 100_000), ("t1", 50_000), ("t2", 80_000)]
Q_REFS = [("t2", 80_000), ("extra", 9_000), ("t0", 100_000), ("t1", 50_000)]      # permuted, and one the truth does not have
Q_ID = {0: 2, 1: 3, 2: 0}


def make_mix(seed, n):
    """n truth records on three references and a query that holds every class of record (see the kinds below)"""
    rng = random.Random(seed)
    truth, front, later = [], [], []
    for k in range(n):
        ref = rng.randrange(3)
        span = rng.randrange(60, 3000)
        pos = rng.randrange(T_REFS[ref][1] - 2 * span)
        flag = 16 * rng.randrange(2)
        name = "S%d_%d" % (ref + 1, k)
        truth.append(truth_rec(name, ref, pos, with_insertions(cigar_over(rng, span, rng.randrange(1, 30))), flag))
        good = query_rec(rng, name, flag, Q_ID[ref], pos, span)
        kind = k % 11
        if kind == 0:
            front.append(good)
        elif kind == 1:                   # shifted by a third: inter / union = 1 / 2
            front.append(query_rec(rng, name, flag, Q_ID[ref], pos + span // 3, span))
        elif kind == 2:                   # shifted by 19 / 20: below a tenth
            front.append(query_rec(rng, name, flag, Q_ID[ref], pos + span * 19 // 20, span))
        elif kind == 3:
            front.append(query_rec(rng, name, flag ^ 16, Q_ID[ref], pos, span))
        elif kind == 4:                   # another reference of the truth, or one it does not have
            front.append(query_rec(rng, name, flag, [Q_ID[(ref + 1) % 3], 1][k // 11 % 2], min(pos, 5000), span))
        elif kind == 5:                   # unmapped by flag, by refID, and by flag with a mate's place filled in
            which = k // 11 % 3
            front.append(B.record(name, [4, 0, 4 | 1 | 8][which], [-1, -1, Q_ID[ref]][which], [-1, -1, pos][which], seq="ACG", qual=b"\x05" * 3,
                                  mapq=[0, 0, 60][which]))
        elif kind == 6:
            pass                          # left out
        elif kind == 7:                   # two primaries: the good one first in the file
            front.append(good)
            later.append(query_rec(rng, name, flag ^ 16, Q_ID[ref], pos, span))
        elif kind == 8:                   # ... and the good one last
            front.append(query_rec(rng, name, flag, 1, 100, span))
            later.append(good)
        elif kind == 9:                   # with a secondary without bases and a supplementary with hard clips and an SA tag
            front.append(good)
            sec = B.record(name, flag | 0x100, Q_ID[(ref + 1) % 3], 77, cigar=[(span, "M")], seq="", qual=b"", mapq=0)
            sup = query_rec(rng, name, (flag ^ 16) | 0x800, Q_ID[ref], pos + 10, span // 2, cigar=[(30, "H"), (span // 2, "M"), (40, "H")],
                            tags=(("SA", "Z", "t0,%d,+,30S%dM40S,60,3;" % (pos + 1, span // 2)),))
            (front if k % 2 else later).extend([sec, sup])
        else:                             # paired: the mate's fields are filled in
            front.append(query_rec(rng, name, flag | 1 | 0x40 | 0x20, Q_ID[ref], pos, span, next_ref_id=Q_ID[ref], next_pos=pos + 300, tlen=-450))
    for k in range(15):
        front.append(query_rec(rng, "nobody%d" % k, 0, rng.randrange(4), rng.randrange(5000), 500))
    front.append(B.record("nobody_sec", 0x100, 0, 5, cigar=[(10, "M")], seq="", qual=b""))
    rng.shuffle(front)
    rng.shuffle(later)
    text = b"@HD\tVN:1.6\tSO:unsorted\n@PG\tID:mapper\n"
    return B.stream(truth, T_REFS, b"@HD\tVN:1.6\tSO:unknown\n"), B.stream(front + later, Q_REFS, text)


@pytest.fixture(scope="module")
def mix():
    return make_mix(41, 330)


# ---------------------------------------------------------------- the rule
@pytest.mark.parametrize("permille", [100, 500, 1000, 1])
def test_synthetic_mix(ctx, mix, permille):
    truth, query = mix
    counts, verdicts = check(ctx, [truth], query, permille=permille, block=[B.W.BGZIP_BLOCK, 777, 4095, 65280][permille % 4],
                             no_sink=True)
    if permille == 100:
        # every class is there, and the counts add up as the rule says
        assert all(counts[n] > 0 for n in M.COUNT_NAMES)
        assert counts["primary"] + counts["secondary"] + counts["supplementary"] == counts["query_records"]
        assert counts["scored"] + counts["unmapped"] + counts["missing"] == counts["truth_records"] == 330
        assert counts["primary"] == counts["unknown"] + counts["duplicate"] + counts["scored"] + counts["unmapped"]
        assert set(verdicts) == {0, 1, 2, 3}
    if permille == 500:
        # the records shifted by a third of a span that three divides: exactly 1 / 2
        assert counts["correct"] > check(ctx, [truth], query, permille=501)[0]["correct"]


def test_the_truth_in_several_files_and_names_given(ctx):
    """three truth files: a one-reference file that calls its reference "ref" and is told the mapper's name, a two-reference
    file, and a file that repeats a reference name of the second; sorted and unsorted order give the same verdicts, record by
    record"""
    rng = random.Random(5)
    files = [[("ref", 90_000)], [("t1", 50_000), ("t2", 80_000)], [("t2", 80_000)]]
    q_refs = [("t2", 80_000), ("t0", 100_000), ("ref", 90_000), ("t1", 50_000)]
    q_id = {"ref": 1, "t1": 3, "t2": 0}              # file 0's "ref" is the mapper's t0; the mapper's own "ref" is someone else
    truths, query = [], []
    for f, refs in enumerate(files):
        recs = []
        for k in range(70):
            ref = rng.randrange(len(refs))
            span = rng.randrange(100, 2000)
            pos = rng.randrange(refs[ref][1] - span)
            name = "f%d_%d" % (f, k)
            recs.append(truth_rec(name, ref, pos, [(span, "M")], 16 * (k % 2)))
            to = [q_id[refs[ref][0]], 2][k % 9 == 0]          # every ninth: onto the mapper's "ref", which is no truth reference
            query.append(query_rec(rng, name, 16 * (k % 2), to, pos, span))
        truths.append(recs)
    rng.shuffle(query)
    names = ["t0", None, None]
    q = B.stream(query, q_refs)
    counts, v = check(ctx, [B.stream(r, refs) for r, refs in zip(truths, files)], q, names)
    assert counts["wrong"] == sum(1 for k in range(70) if k % 9 == 0) * 3 and counts["correct"] == 210 - counts["wrong"]
    order = [sorted(range(70), key=lambda k: (r[k]["ref_id"], r[k]["pos"])) for r in truths]
    _, v_sorted = check(ctx, [B.stream([r[k] for k in o], refs) for r, o, refs in zip(truths, order, files)], q, names)
    assert [v_sorted[70 * f + i] for f, o in enumerate(order) for i in range(70)] == [v[70 * f + k] for f, o in enumerate(order) for k in o]
    # without the name file 0's reads are all on a reference the query does not have under that name... but "ref" exists there
    assert check(ctx, [B.stream(r, refs) for r, refs in zip(truths, files)], q, None)[0]["correct"] < counts["correct"]


@pytest.mark.parametrize("hash_bits", [64, 8, 2, 1])
def test_collisions_change_nothing(ctx, mix, hash_bits):
    """with 8, 2 and 1 bits of the hash every lookup walks a run of other names: the name bytes decide"""
    truth, query = mix
    check(ctx, [truth], query, hash_bits=hash_bits)


# ---------------------------------------------------------------- shapes that break kernels
def test_names_of_1_and_254_bytes_and_long_common_prefixes(ctx):
    rng = random.Random(9)
    p = "p" * 200
    names = ["x", "y", "Y" * 254, "Z" * 253 + "a", "Z" * 253 + "b", p, p + "a", p + "b", p + "ab", p + "ba", p[:-1], "a" + p, "b" + p,
             "Z" * 253, "xy", "yx"]
    assert len(set(names)) == len(names) and max(len(n) for n in names) == 254
    truth = [truth_rec(n, 0, 1000 * k, [(500, "M")]) for k, n in enumerate(names)]
    query = [query_rec(rng, n, 0, 0, 1000 * k + (50_000 if k % 5 == 4 else 0), 500) for k, n in enumerate(names)]
    query += [query_rec(rng, n, 0, 0, 0, 500) for n in ["z", "Y" * 253, "Z" * 253 + "c", p + "c", p + "aa", p[:-2], "", "X" * 254]]     # unknown, all
    rng.shuffle(query)
    refs = [("chr", 200_000)]
    for hash_bits in (0, 1):
        counts, _ = check(ctx, [B.stream(truth, refs)], B.stream(query, refs), hash_bits=hash_bits)
        assert counts["unknown"] == 8 and counts["missing"] == 0 and counts["wrong"] == len(names) // 5


def test_records_across_every_tile_edge(ctx):
    """a leading record whose length takes 64 consecutive values shifts every later record by one byte at a time: with records of
    60 to 300 bytes over three tiles of the scan, every field of some record lies across a 4096-byte edge at some shift, and so
    does every part that the key kernel reads (name, CIGAR)"""
    rng = random.Random(13)
    refs = [("chr", 1_000_000)]
    body_t, body_q = [], []
    for k in range(75):
        span = rng.randrange(10, 900)
        pos = rng.randrange(900_000)
        name = "r%d" % k + "n" * rng.randrange(0, 60)
        body_t.append(truth_rec(name, 0, pos, with_insertions(cigar_over(rng, span, min(span, rng.randrange(1, 20)))), 16 * (k % 2)))
        body_q.append(query_rec(rng, name, 16 * (k % 2), 0, pos + (span if k % 6 == 0 else 0), span))
    rng.shuffle(body_q)
    for pad in range(64):
        lead = dict(tags=(("XP", "Z", "p" * pad),))
        truth = B.stream([truth_rec("pad", 0, 0, [(1, "M")], **lead)] + body_t, refs)
        query = B.stream([query_rec(rng, "pad", 0, 0, 0, 1, cigar=[(1, "M")], **lead)] + body_q, refs)
        assert len(truth) > 2 * TILE and len(query) > 2 * TILE
        check(ctx, [truth], query, container=["none", "bgzf"][pad % 2], block=1000 + pad)


def test_more_than_2048_records_in_each_stream(ctx):
    """more records than one tile of any scan or one workgroup of any kernel holds, in two truth files and the query"""
    rng = random.Random(17)
    refs = [("a", 3_000_000), ("b", 500_000)]
    truth, query = [], []
    for k in range(4700):
        ref = k % 2
        pos = rng.randrange(refs[ref][1] - 400)
        truth.append(truth_rec("m%d" % k, ref, pos, [(300, "M")], 16 * (k % 3 == 0)))
        if k % 50 != 7:
            query.append(query_rec(rng, "m%d" % k, 16 * (k % 3 == 0), ref, pos + (290 if k % 10 == 3 else 0), 300, mapq=k % 256, cigar=[(300, "M")],
                                   tags=()))
    rng.shuffle(query)
    counts, _ = check(ctx, [B.stream(truth[:2300], refs), B.stream(truth[2300:], refs)], B.stream(query, refs), container="none")
    assert counts["query_records"] > 2 * 2048 and counts["missing"] == 94 and counts["wrong"] == 470


def test_long_cigars_take_the_wave_path(ctx):
    """the key kernel sums a CIGAR of more than 64 operations with its whole wave: 65 535 operations (all a record can hold),
    two such records next to each other in one wave, 65 and 64 operations on either side of the switch; and the read whose 70 000
    operations went into the CG tag -- its placeholder's N carries the span -- against a mapper's record of 300 operations"""
    rng = random.Random(21)
    refs = [("chr", 3_000_000)]
    cg_ops = [(3, "M"), (1, "I")] * 35_000
    cg = truth_rec("cg", 0, 1000, [(4 * 35_000, "S"), (3 * 35_000, "N")], tags=(("CG", "BI", [n << 4 | "MIDNSHP=X".index(op) for n, op in cg_ops]),))
    most = truth_rec("most", 0, 200_000, with_insertions(cigar_over(rng, 300_000, 49_151), every=3)[:65_535], 16)
    assert len(most["cigar"]) == 65_535
    truth = [truth_rec("s0", 0, 5, [(10, "M")]), cg, truth_rec("s1", 0, 50, [(10, "M")]), most,
             truth_rec("w1", 0, 700_000, cigar_over(rng, 9000, 100)), truth_rec("w2", 0, 800_000, cigar_over(rng, 9000, 200), 16),
             truth_rec("l64", 0, 900_000, cigar_over(rng, 5000, 64)), truth_rec("l65", 0, 950_000, cigar_over(rng, 5000, 65)),
             truth_rec("s2", 0, 990_000, [(10, "M")])]
    spans = {r["name"]: M.interval(x)[1] - x["pos"] for r, x in zip(truth, M.parse(B.stream(truth, refs))[1])}
    assert spans["cg"] == 105_000 and spans["w1"] == 9000 and spans["l65"] == 5000
    query = [query_rec(rng, "cg", 0, 0, 1000, 0, cigar=[(7, "S")] + cigar_over(rng, 105_000, 298) + [(9, "S")]),
             query_rec(rng, "most", 16, 0, 200_000 + spans["most"] * 9 // 10 + 1, 0, cigar=cigar_over(rng, spans["most"], 65)),      # just wrong
             query_rec(rng, "w1", 0, 0, 700_000, 0, cigar=cigar_over(rng, 900, 70)),                  # a tenth exactly: correct
             query_rec(rng, "w2", 16, 0, 800_000, 0, cigar=cigar_over(rng, 899, 200)),                # one base less: wrong
             query_rec(rng, "l64", 0, 0, 900_000, 0, cigar=cigar_over(rng, 5000, 64)),
             query_rec(rng, "l65", 0, 0, 950_000, 0, cigar=cigar_over(rng, 5000, 66)),
             query_rec(rng, "s0", 0, 0, 5, 10), query_rec(rng, "s1", 0, 0, 50, 10), query_rec(rng, "s2", 0, 0, 990_000, 10)]
    assert len(query[0]["cigar"]) == 300
    counts, v = check(ctx, [B.stream(truth, refs)], B.stream(query, refs))
    assert v == bytes([3, 3, 3, 2, 3, 2, 3, 3, 3])
    check(ctx, [B.stream(truth[::-1], refs)], B.stream(query[::-1], refs), container="none")


def test_no_query_record_and_one_truth_record(ctx):
    rng = random.Random(2)
    refs = [("chr", 10_000)]
    one = B.stream([truth_rec("only", 0, 100, [(50, "M")])], refs)
    counts, v = check(ctx, [one], B.stream([], refs))
    assert counts["missing"] == 1 and counts["query_records"] == 0 and v == b"\0"
    check(ctx, [one], B.stream([], []))
    counts, v = check(ctx, [one], B.stream([query_rec(rng, "only", 0, 0, 100, 50, mapq=255)], refs))
    assert v == b"\3"
    counts, v = check(ctx, [B.stream([], refs), one, B.stream([], [])], B.stream([query_rec(rng, "only", 0, 0, 100, 50, mapq=0)], refs))
    assert v == b"\3" and counts["truth_records"] == 1
    counts, v = check(ctx, [B.stream([], refs)], B.stream([query_rec(rng, "only", 0, 0, 100, 50)], refs))
    assert v == b"" and counts["unknown"] == 1


@pytest.mark.parametrize("container", ["bgzf", "gzip", "none", ("gzip", "none", "bgzf"), ("stored", "bgzf", "gzip")])
def test_containers(ctx, container):
    truth, query = make_mix(3, 120)
    _, recs = M.parse(truth)
    refs_only = truth[:recs[0]["offset"]]
    half = recs[60]["offset"]
    check(ctx, [truth[:half], refs_only + truth[half:]], query, container=container, block=3000)


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(ctx, mix):
    rng = random.Random(6)
    refs = [("chr", 100_000)]
    two_refs = [("chr", 100_000), ("chr2", 5000)]
    recs = [truth_rec("n%d" % k, 0, 100 * k, [(80, "M")]) for k in range(300)]
    other = [truth_rec("o%d" % k, 0, 100 * k, [(80, "M")]) for k in range(40)]
    fresh = [truth_rec("z%d" % k, 0, 100 * k, [(80, "M")]) for k in range(10)]
    query = B.bam([query_rec(rng, "n%d" % k, 0, 0, 100 * k, 80) for k in range(0, 300, 7)], refs)
    good = dict(correct=43, missing=257)

    def usable():
        counts = ctx.eval_bam(B.bam(recs, refs), query)[0]
        assert {k: counts[k] for k in good} == good
        check(ctx, [mix[0]], mix[1])

    twice = recs[:200] + [truth_rec("n57", 0, 9, [(5, "M")], 16)] + recs[200:]
    with pytest.raises(P.PbsimError, match=r'"n57" occurs twice in the truth: record 57 of truth file 0 and record 200 of truth file 0'):
        ctx.eval_bam(B.bam(twice, refs), query)
    usable()
    with pytest.raises(P.PbsimError, match=r'"n57" occurs twice .* record 57 of truth file 0 and record 200 of truth file 0'):
        ctx.eval_bam(B.bam(twice, refs), query, hash_bits=1)              # not neighbours in the sorted order: the run is walked
    with pytest.raises(P.PbsimError, match=r'"n299" occurs twice in the truth: record 299 of truth file 1 and record 3 of truth file 2'):
        ctx.eval_bam([B.bam(other, refs), B.bam(recs, refs), B.bam(fresh[:3] + recs[299:] + fresh[3:], refs, container="none")], query)
    usable()
    with pytest.raises(P.PbsimError, match=r"truth file 1 has 2 references: a reference name can be given only to a truth file with exactly one"):
        ctx.eval_bam([B.bam(other, refs), B.bam(recs, two_refs)], query, ref_names=["chr", "chr"])
    usable()
    assert ctx.eval_bam([B.bam(other, refs), B.bam(recs, two_refs)], query, ref_names=["chrX", None])[0]["correct"] == 43
    # a query record that is none, a truth record that is not placed, a file that is no BAM
    broken = B.stream([query_rec(rng, "n0", 0, 0, 0, 80)], refs)
    with pytest.raises(P.PbsimError, match=r"the query: the record at inflated byte offset %d does not fit" % len(broken)):
        ctx.eval_bam(B.bam(recs, refs), B.contain(broken + b"\0" * 40 + b"\x07" * 30, "bgzf"))
    with pytest.raises(P.PbsimError, match=r"truth file 0: the record at inflated byte offset %d does not fit" % len(B.header(refs))):
        ctx.eval_bam(B.bam([B.record("unplaced", 4, -1, -1, seq="A", qual=b"\x09")] + recs, refs), query)
    with pytest.raises(P.PbsimError, match="truth file 1: neither BGZF, gzip nor an uncompressed BAM"):
        ctx.eval_bam([B.bam(recs, refs), b"@HD\tVN:1.6\n"], query)
    with pytest.raises(P.PbsimError, match="the query: not a BAM file"):
        ctx.eval_bam(B.bam(recs, refs), B.W.bgzf(b"SAM\1" + bytes(100)))
    usable()


# ---------------------------------------------------------------- the product's own files, through the command line
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def _run(cmd, workdir, ok=True):
    r = subprocess.run(cmd, capture_output=True, cwd=workdir, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr[-4000:]
    return r


def _simulate(case, workdir):
    import pbsim3_amd.build as b
    b.build()
    os.makedirs(workdir, exist_ok=True)
    _run([CLI] + harness.resolve(CASES[case]["args"]) + ["--prefix", os.path.join(workdir, "out"), "--truth-format", "bam"], workdir)
    return sorted(os.path.join(workdir, n) for n in os.listdir(workdir) if n.endswith(".aln.bam"))


def _inflate(path):
    with open(path, "rb") as f:
        return b"".join(R.blocks(f.read()))


def _all_correct(report, n):
    lines = report.split(b"\n")
    assert lines[0].startswith(b"# truth_records=%d query_records=%d primary=%d " % (n, n, n)) and b" correct=%d wrong=0 missing=0" % n in lines[0]
    assert lines[1:] == [b"Q\t60\t%d\t0\t%d\t0\t0\t1000000" % (n, n), b""]


def test_cli_a_trans_truth_file_against_itself(tmp_path):
    (aln,) = _simulate("trans_errhmm_sequel", str(tmp_path))
    stream = _inflate(aln)
    n = len(M.parse(stream)[1])
    assert n > 10
    r = _run([CLI, "--eval-bam", aln, "--truth-bam", aln], str(tmp_path))
    assert r.stdout == M.report(*M.evaluate([stream], stream)[:2])
    _all_correct(r.stdout, n)


def test_cli_wgs_truth_files_against_themselves_and_a_merged_query(tmp_path):
    """a genome of two records: each .aln.bam against itself, then one query that holds both files' records under the names the
    mapper would have seen, against the unsorted and against the sorted truth files"""
    alns = _simulate("wgs_errhmm-ont_quirk", str(tmp_path / "u"))
    assert len(alns) == 2
    parsed = []
    for aln in alns:
        with open(aln, "rb") as f:
            parsed.append(R.read_bam(f.read()))
        stream = _inflate(aln)
        r = _run([CLI, "--eval-bam", aln, "--truth-bam", aln], str(tmp_path))
        _all_correct(r.stdout, len(parsed[-1][2]))
        assert r.stdout == M.report(*M.evaluate([stream], stream)[:2])
    assert all([name for name, _ in refs] == ["ref"] for _, refs, _ in parsed)
    q_refs = [("chrA", parsed[0][1][0][1]), ("chrB", parsed[1][1][0][1])]
    merged = [B.record(a["read_name"], a["flag"], f, a["pos"], cigar=a["cigar"], seq=a["seq"], qual=a["qual"], tags=a["aux"], mapq=a["mapq"],
                       bin=a["bin"]) for f, (_, _, recs) in enumerate(parsed) for a in recs]
    random.Random(1).shuffle(merged)
    query = str(tmp_path / "mapped.bam")
    with open(query, "wb") as f:
        f.write(B.bam(merged, q_refs))
    q_stream = B.stream(merged, q_refs)
    os.makedirs(tmp_path / "s")
    srt = [shutil.copy(a, str(tmp_path / "s")) for a in alns]
    _run([CLI, "--sort-truth-bam"] + srt, str(tmp_path / "s"))
    assert _inflate(srt[0]) != _inflate(alns[0])
    for files in (alns, srt):
        truths = [_inflate(a) for a in files]
        want = M.report(*M.evaluate(truths, q_stream, [b"chrA", b"chrB"])[:2])
        r = _run([CLI, "--eval-bam", query, "--truth-bam", files[0], "--truth-bam", files[1], "--truth-ref-names", "chrA,chrB"], str(tmp_path))
        assert r.stdout == want
        _all_correct(r.stdout, len(merged))
    # the names the other way round: every read is on the wrong reference; and into a file
    out = str(tmp_path / "report.txt")
    r = _run([CLI, "--eval-bam", query, "--truth-bam", alns[0], "--truth-bam", alns[1], "--truth-ref-names", "chrB,chrA", "--eval-overlap", "0.5",
              "--eval-out", out], str(tmp_path))
    with open(out, "rb") as f:
        text = f.read()
    assert r.stdout == b"" and text == M.report(*M.evaluate([_inflate(a) for a in alns], q_stream, [b"chrB", b"chrA"], 500)[:2])
    assert b" correct=0 wrong=%d " % len(merged) in text
    # without names "ref" is no reference of the query; a name for a file that does not exist is refused by count
    r = _run([CLI, "--eval-bam", query, "--truth-bam", alns[0], "--truth-bam", alns[1]], str(tmp_path))
    assert b" correct=0 " in r.stdout
    r = _run([CLI, "--eval-bam", query, "--truth-bam", alns[0], "--truth-ref-names", "chrA,chrB"], str(tmp_path), ok=False)
    assert b"2 names for 1 --truth-bam files" in r.stderr
    # the same file twice: every name occurs twice; refused with the first such name, and the command line says which files those are
    first = M.parse(_inflate(alns[1]))[1][0]["name"]
    r = _run([CLI, "--eval-bam", query, "--truth-bam", alns[0], "--truth-bam", alns[1], "--truth-bam", alns[1]], str(tmp_path), ok=False)
    assert b'the read name "%s" occurs twice in the truth: record 0 of truth file 1 and record 0 of truth file 2' % first in r.stderr
    assert b"truth file 2 is " + alns[1].encode() in r.stderr and r.stdout == b""
