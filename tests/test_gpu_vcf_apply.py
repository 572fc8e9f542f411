"""`pbsim --apply-vcf` (pbsim_vcf_apply) on the device, held to tests/apply_model.py byte for byte: the result, the report, the FASTA,
the annotated text under both settings of `lines` and the origin maps, with every output asked for and not asked for; and round
trips against the stages that already exist: the mutate stage's VCF applied gives its FASTA, the call stage's VCF applied gives the
consensus stage's FASTA."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import apply_model as M
import bam_writer as B
import bgzf_writer as W
import harness
import pbsim3_amd as P
from test_apply_model import (GENOTYPES, HEAD, WORKED_FASTA, WORKED_GENOME, WORKED_ORIGINS, WORKED_REPORT, WORKED_TEXT, WORKED_VCF, WORKED_VERDICTS, vcf)
from test_call_model import lines_of
from test_gpu_bam_grid_caps import constant
from test_mutate_model import four_records, spelling_reads

pytestmark = pytest.mark.gpu

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")
THREADS, TILE = constant("bam_pileup_walk.h", "kThreads"), constant("bam_pileup.h", "kPileTile")
TEXT_TILE = constant("vcf_apply.h", "kApTile")


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


def numbers(result):
    out = []
    for k in M.FIELDS:
        out += [result[k][t] for t in P.APPLY_TYPES] if k == "types" else [result[k]]
    return out


def check(ctx, text, genome, modes=(0, 1), piece_bytes=0, **kw):
    """the text through the product, every output against the model under each setting of `lines`; then with no output asked for,
    with each one alone, and in small pieces; returns the model's result under the first setting"""
    first = None
    for lines in modes:
        want = M.apply(text, genome, lines=lines, **kw)
        got = ctx.apply_vcf(text, genome, lines=lines, origin=True, piece_bytes=piece_bytes, **kw)
        assert len(got) == 6
        assert numbers(got[0]) == M.flat(want)
        assert got[1] == want.report and got[2] == want.fasta and got[3] == want.per_record and got[4] == want.text
        assert len(got[5]) == len(want.origins) and all(np.array_equal(a, b) for a, b in zip(got[5], want.origins))
        first = first or want
    want = first
    lines = modes[0]
    bare = ctx.apply_vcf(text, genome, lines=("discordant", "all")[lines], fasta=False, text=False, **kw)
    assert len(bare) == 2 and numbers(bare[0]) == M.flat(want) and bare[1] == want.report
    only = ctx.apply_vcf(text, genome, lines=lines, fasta=False, text=False, origin=True, **kw)
    assert len(only) == 3 and numbers(only[0]) == M.flat(want) and all(np.array_equal(a, b) for a, b in zip(only[2], want.origins))
    only = ctx.apply_vcf(text, genome, lines=lines, fasta=False, **kw)
    assert len(only) == 3 and only[2] == want.text
    only = ctx.apply_vcf(text, genome, lines=lines, text=False, piece_bytes=piece_bytes or 61, **kw)
    assert len(only) == 4 and only[2] == want.fasta and only[3] == want.per_record and numbers(only[0]) == M.flat(want)
    return want


def verdicts(r):
    return [row["cls"] for row in r.rows]


def flip(base):
    return "C" if base in "Aa" else "A"


# ---------------------------------------------------------------- basics
def test_the_worked_case(ctx):
    r = check(ctx, WORKED_VCF, WORKED_GENOME)
    assert r.report == WORKED_REPORT and r.text == WORKED_TEXT and r.fasta == WORKED_FASTA[0] and [o.tolist() for o in r.origins] == WORKED_ORIGINS
    for h in (1, 2):
        r = check(ctx, WORKED_VCF, WORKED_GENOME, haplotype=h, piece_bytes=7)
        assert r.fasta == WORKED_FASTA[h] and verdicts(r) == WORKED_VERDICTS[h]
    assert check(ctx, WORKED_VCF, WORKED_GENOME, haplotype=2, sample=1, line_width=5).ref_allele == 17
    got = ctx.apply_vcf(WORKED_VCF, WORKED_GENOME, haplotype=2, sample="NA1")
    assert got[2] == WORKED_FASTA[2]


def test_every_class_and_both_line_ends(ctx):
    genome = [("c1", b"ACGTNACGTACGT"), ("c2", b"acgtt")]
    rows = [b"c1\t2\t.\tC", b"\t2\t.\tC\tT", b"c1\t2\t.\t\tT", b"c1\t2\t.\tC\t", b"c1\t0\t.\tC\tT", b"c1\t2147483648\t.\tC\tT", b"c1\t2x\t.\tC\tT",
            b"c1\t\t.\tC\tT", b"c1\t+2\t.\tC\tT", b"c1\t99999999999999999999999\t.\tC\tT", b"c3\t2\t.\tC\tT", b"c\t2\t.\tC\tT", b"c11\t2\t.\tC\tT",
            b"C1\t2\t.\tC\tT", b"c1\t2\t.\tC\tT,G", b"c1\t2\t.\tC\t<DEL>", b"c1\t2\t.\tC\t*", b"c1\t2\t.\tC\t.", b"c1\t2\t.\tR\tT", b"c1\t2\t.\tG\tT",
            b"c1\t12\t.\tGTA\tG", b"c1\t14\t.\tA\tT", b"c2\t6\t.\tA\tT", b"c1\t2\t.\tC\tT\t.\tLowQual\tMS=9", b"c1\t2\t.\tC\tT\t.\t\tMS=9",
            b"c1\t2\t.\tC\tT\t.\tpass", b"c1\t2\t.\tC\tc", b"c2\t1\t.\tac\tAC\t.\tPASS", b"c1\t0000000003\t.\tg\tt\t.\tPASS\tDP=1",
            b"c1\t5\t.\tN\tA\t.\t.", b"c2\t4\t.\tTT\tT\t.\t.\tMS=0", b"c1\t2\t.\tC\tT,\t.\t.", b"c1\t2\t.\tC\t,T", b"c1\t2\t.\tC\tT,,G", b"c1\t2\t.\tC\tT,<X>",
            b"c2\t2\t.\tcgt\tCTA\t.\t.\tMS=4;\tGT\t1|1", b"c2\t1\t.\tA\tG\t.\t.\t.\tGT:DP\t0|1:3\t1|0", b"c1\t7\t.\tC\tG,T\t.\t.\t.\tGT\t2|.\t.|1",
            b"c1\t8\t.\tG\tC\t.\t.\t.\tDP:GT\t1:1|1", b"c1\t8\t.\tG\tC\t.\t.\t.\tGT\t1|1|1", b"c1\t9\t.\tT\tC\t.\t.\t.\tGT\t3", b"\t", b"c1"]
    text = b"#head\n\n" + b"\n".join(rows) + b"\n"
    r = check(ctx, text, genome)
    assert all(getattr(r, c) > 0 for c in M.CLASSES if c not in ("no_call", "ref_allele")) and r.overlap > 0 and r.applied > 0
    for h, sample in ((1, 0), (2, 0), (1, 1), (2, 1)):
        r = check(ctx, text, genome, haplotype=h, sample=sample, modes=(1,))
        assert r.applied > 0 and r.malformed > 30 and (r.no_call or r.ref_allele)
    crlf = text.replace(b"\n", b"\r\n")
    for t in (crlf, text[:-1], crlf[:-2], crlf[:-1], crlf + b"\r", b"\r", b"\r\n\r\n"):
        check(ctx, t, genome, modes=(1,))
        if len(t) > 4:                              # (a file whose only data line is a lone \r has no sample column: refused)
            check(ctx, t, genome, modes=(0,), haplotype=2)


def test_a_header_only_file_and_an_empty_file(ctx):
    for t in (HEAD, b"", b"\n", b"#", HEAD[:-1]):
        for h in (0, 1):
            r = check(ctx, t, WORKED_GENOME, haplotype=h, sample=5)
            assert r.lines == 0 and r.bases_out == r.bases_in == 28 and r.fasta == b">c1\nACGTACGTACGTACGTACGTACGT\n>c2\n>c3\nTTGA\n" and r.text == M.TEXT_HEADER
    with pytest.raises(P.PbsimError, match="pbsim_vcf_apply: no data line has a sample column 2"):
        ctx.apply_vcf(WORKED_VCF, WORKED_GENOME, haplotype=1, sample=2)
    with pytest.raises(P.PbsimError, match="pbsim_vcf_apply: no data line has a sample column 0"):
        ctx.apply_vcf(b"c1\t2\t.\tC\tT\n", WORKED_GENOME, haplotype=2)
    assert ctx.apply_vcf(b"c1\t2\t.\tC\tT\n", WORKED_GENOME, sample=7)[0]["applied"] == 1      # (haplotype 0 reads no sample)
    check(ctx, WORKED_VCF, WORKED_GENOME)


# ---------------------------------------------------------------- round trips against the stages that exist
RATES = dict(snv_ppm=150000, ins_ppm=100000, del_ppm=150000, ext_ppm=600000, max_indel=9)


@pytest.mark.parametrize("line_width", [60, 0, 7])
def test_the_mutate_stages_vcf_applied_is_its_fasta(ctx, line_width):
    genome = four_records() + [("c", harness.synth_bases(2000, 17).tobytes())]
    result, _, fasta, text, records, origins = ctx.mutate_genome(genome, origin=True, line_width=line_width, **RATES)
    assert min(result["types"].values()) > 20 and result["merged"] > 0 and result["dropped"] > 0
    got = ctx.apply_vcf(text, genome, line_width=line_width, origin=True, lines="all")
    assert got[2] == fasta
    assert got[3] == records and all(np.array_equal(a, b) for a, b in zip(got[5], origins)) and len(got[5]) == len(origins)
    assert got[0]["applied"] == got[0]["lines"] == result["variants"] and got[0]["longest_cluster"] == 1
    assert (got[0]["inserted"], got[0]["deleted"], got[0]["substituted"]) == (result["inserted"], result["deleted"], result["substituted"])
    assert got[4].count(b"\tapplied\t0\n") == result["variants"]
    if line_width == 60:
        check(ctx, text, genome, modes=(0,))


def test_the_call_stages_vcf_applied_is_the_consensus(ctx):
    genome = [("a", harness.synth_bases(3000, 81).tobytes()), ("b", (b"AC" * 40 + b"GGGGGGGGTTTTTTTTTT" + b"CAG" * 30) * 6)]
    result, _, fasta, _, _, origins = ctx.mutate_genome(genome, origin=True, line_width=0, snv_ppm=100000, ins_ppm=150000, del_ppm=150000, ext_ppm=300000)
    stream, _ = spelling_reads(genome, fasta, origins)
    bam = B.contain(stream)
    called = ctx.bam_call(bam, genome, max_ins=65535)
    consensus = ctx.bam_consensus(bam, genome, fill="ref", max_ins=65535)
    got = ctx.apply_vcf(called[2], genome)
    assert got[2] == consensus[2]
    assert got[0]["applied"] == got[0]["lines"] == called[0]["variants"] > 100 and min(got[0]["types"][t] for t in ("snv", "ins", "del")) > 10
    assert [(a, b) for a, b, _ in got[3]] == [tuple(x) for x in consensus[3]]


# ---------------------------------------------------------------- seams
def seam_rows(name, seq, at):
    """lines whose starts, ends and X lie around buffer position `at` of a record that begins on a tile's edge: an insertion on each
    of at - 1, at, at + 1, a span that ends on at - 1, on at and on at + 1, one that begins on each, and an X that runs over the seam"""
    rows = []
    for p in (at - 1, at, at + 1):
        rows.append((name, p, chr(seq[p - 1]), chr(seq[p - 1]) + "TTG"))                                   # an insertion at p
    for k, end in enumerate((at - 1, at, at + 1)):
        s = at - 20 + 5 * k
        rows.append((name, s + 1, seq[s:end].decode(), flip(chr(seq[s])) + flip(chr(seq[end - 1]))))           # the span [s, end)
    rows.append((name, at + 2, seq[at + 1:at + 4].decode(), flip(chr(seq[at + 1])) + "ACGTACGTACGTACGT" * 20))     # begins behind the seam, a long X
    return rows


def test_spans_and_insertions_on_the_seams_of_the_position_tiles(ctx):
    seq = harness.synth_bases(3 * TILE + 11, 5).tobytes()
    genome = [("g", seq)]
    for at in (TILE, 2 * TILE):
        r = check(ctx, vcf(seam_rows("g", seq, at)), genome, modes=(1,))
        assert r.applied >= 5 and r.overlap >= 1
    # every line alone, its start on each of the three positions: nothing collides
    for at in (TILE, 2 * TILE):
        for p in (at - 1, at, at + 1):
            for d, x in ((0, "GATTACA"), (1, ""), (3, "T"), (TILE + 3, ""), (2, "ACGT" * (TILE // 2)), (TILE - 1, "AC" * TILE)):
                ref = seq[p - 1:p + d].decode()
                r = check(ctx, vcf([("g", p, ref, ref[0] + x)]), genome, modes=(0,))
                assert r.applied == 1 and r.rows[0]["s"] >= p


def test_the_first_and_last_bases_of_records(ctx):
    a, b = harness.synth_bases(TILE, 6).tobytes(), harness.synth_bases(64, 7).tobytes()
    genome = [("a", a), ("none", b""), ("b", b), ("none2", b""), ("c", a[:63]), ("d", a[:65])]
    rows = []
    for name, seq in genome:
        if not seq:
            continue
        n = len(seq)
        rows += [(name, 1, chr(seq[0]), flip(chr(seq[0])) * 2 + chr(seq[0])),         # an insertion in front of the record's first base
                 (name, n - 2, seq[n - 3:n].decode(), flip(chr(seq[n - 3])) + flip(chr(seq[n - 1]))),   # a span that ends on the record's last base
                 (name, n, chr(seq[n - 1]), chr(seq[n - 1]) + "TTT"),                  # an insertion at l_ref, behind an applied span
                 (name, 1, seq[:2].decode(), flip(chr(seq[0])))]                       # a span at position 0, behind the insertion there
    r = check(ctx, vcf(rows), genome)
    assert verdicts(r) == ["applied"] * len(rows) and r.per_record[1] == (0, 0, 0) and r.per_record[3] == (0, 0, 0)
    assert [o[0] for o in r.origins if len(o)] == [-2 ** 31] * 4 and [o[-1] for o in r.origins if len(o)] == [-len(s) for _, s in genome if s]
    # an insertion at l_ref where the span in front ends one short of the last base, and nothing else
    rows = [("a", TILE, chr(a[-1]), chr(a[-1]) + "C"), ("b", 64, chr(b[-1]), chr(b[-1]) + "C"), ("a", TILE - 2, a[-3:-1].decode(), flip(chr(a[-3])))]
    assert check(ctx, vcf(rows), genome).applied == 3
    with pytest.raises(P.PbsimError, match="pbsim_vcf_apply: the genome holds two records named"):
        ctx.apply_vcf(vcf(rows), genome + [("a", b"AC")])
    check(ctx, vcf(rows), genome, modes=(0,))


BODY = b"c1\t2\t.\tC\tT\n\n#c\nc1\t6\t.\tC\tCA\r\n\r\n#\nc1\t8\t.\tTAC\tT\n\nc1\t14\t.\tC\tG"


@pytest.mark.parametrize("first", [TEXT_TILE - 30, TEXT_TILE - 12])
def test_lines_on_the_seams_of_the_line_tables_tiles(ctx, first):
    """the body -- data lines, empty lines with and without \\r, # lines, a last line without its line feed -- behind a # line of
    `first` + 0 .. 17 bytes: every one of its bytes comes to lie on a tile's last byte and on the next one's first"""
    for k in range(18):
        pad = b"#" + b"x" * (first + k - 2) + b"\n"
        assert len(pad) == first + k
        r = check(ctx, pad + BODY, WORKED_GENOME, modes=(1,))
        assert verdicts(r) == ["applied"] * 4
    for n in (TEXT_TILE - 1, TEXT_TILE, TEXT_TILE + 1, 2 * TEXT_TILE):
        text = b"#" + b"x" * (n - len(BODY) - 2) + b"\n" + BODY
        assert len(text) == n and verdicts(check(ctx, text, WORKED_GENOME, modes=(1,))) == ["applied"] * 4


def test_a_line_and_an_x_longer_than_a_tile(ctx):
    seq = harness.synth_bases(9000, 3).tobytes()
    long_x = "ACGT" * 700 + "AAC"
    rows = [("long", 11, seq[10:10 + 3 * TEXT_TILE + 5].decode(), seq[10:11].decode()), ("long", 5000, seq[4999:5000].decode(), seq[4999:5000].decode() + long_x),
            ("long", 8000, seq[7999:8003].decode(), flip(chr(seq[7999])) + long_x + flip(chr(seq[8002])), "2|1"),
            ("long", 8500, seq[8499:8500].decode(), "<X>," + seq[8499:8500].decode() + long_x[:TILE + 1], "2|0")]
    for h in (0, 1, 2):
        r = check(ctx, vcf(rows), [("long", seq)], haplotype=h, line_width=(60, 0, 1000)[h])
        assert r.applied == 3 and (r.unsupported, r.malformed, r.ref_allele) == ((1, 0, 0), (0, 1, 0), (0, 0, 1))[h]


# ---------------------------------------------------------------- clusters
def chain(name, seq, first, n):
    """n spans of three positions, each two behind the one before: every one overlaps the next"""
    return [(name, first + 2 * k + 1, seq[first + 2 * k:first + 2 * k + 3].decode(), flip(chr(seq[first + 2 * k])) + flip(chr(seq[first + 2 * k + 2])))
            for k in range(n)]


@pytest.mark.parametrize("n", [2, 63, 64, 65, THREADS + 1])
def test_a_chain_of_overlapping_lines(ctx, n):
    seq = harness.synth_bases(5 * THREADS, 40 + n).tobytes()
    rows = chain("g", seq, 2 * THREADS, n)
    head = [("g", q + 1, chr(seq[q]), flip(chr(seq[q]))) for q in range(0, 2 * (THREADS - 40), 2)]      # the chain begins near the first workgroup's end
    for lead in ([], head):
        r = check(ctx, vcf(rows[::-1] + lead), [("g", seq)], modes=(1,))
        assert verdicts(r)[:n][::-1] == ["applied", "overlap"] * (n // 2) + ["applied"] * (n % 2) and r.longest_cluster == n
        assert [row["by"] for row in r.rows[:n]][::-1] == [0 if k % 2 == 0 else n - k + 1 for k in range(n)]


def test_a_cluster_that_ends_with_its_record(ctx):
    a, b = harness.synth_bases(TILE + 9, 51).tobytes(), harness.synth_bases(90, 52).tobytes()
    n = len(a)
    rows = chain("a", a, n - 9, 4)                                                                     # [n-9, n-6) [n-7, n-4) [n-5, n-2) [n-3, n)
    rows += [("b", 1, b[:2].decode(), flip(chr(b[0]))), ("b", 1, chr(b[0]), flip(chr(b[0])) + chr(b[0])), ("a", n, chr(a[-1]), chr(a[-1]) + "GG")]
    r = check(ctx, vcf(rows), [("a", a), ("b", b)])
    assert verdicts(r) == ["applied", "overlap", "applied", "overlap", "applied", "applied", "applied"] and r.longest_cluster == 4
    r = check(ctx, vcf(rows[:3] + rows[4:]), [("a", a), ("b", b)])
    assert verdicts(r) == ["applied", "overlap", "applied", "applied", "applied", "applied"] and r.longest_cluster == 3


def test_insertions_at_one_site_and_at_the_ends_of_a_span(ctx):
    seq = harness.synth_bases(400, 9).tobytes()
    ins = lambda p, x: ("g", p, chr(seq[p - 1]), chr(seq[p - 1]) + x)
    rows = [ins(100, "A"), ins(100, "C"), ins(100, "A"), ("g", 101, seq[100:110].decode(), flip(chr(seq[100])) + flip(chr(seq[109]))), ins(105, "T"),
            ins(110, "GG"), ins(110, "T"), ("g", 110, seq[109:112].decode(), chr(seq[109])), ins(112, "C")]      # (the deletion [110, 112) with its padding base)
    r = check(ctx, vcf(rows), [("g", seq)])
    assert verdicts(r) == ["applied", "overlap", "overlap", "applied", "overlap", "applied", "overlap", "applied", "applied"]
    assert [row["by"] for row in r.rows] == [0, 1, 1, 0, 4, 0, 6, 0, 0] and r.longest_cluster == 3


# ---------------------------------------------------------------- genotypes
def test_genotypes(ctx):
    seq = b"ACGT" * (len(GENOTYPES) + 4)
    rows = [("c", 4 * k + 2, "C", "G,T", gt) for k, (gt, _, _) in enumerate(GENOTYPES)]
    rows += [("c", 4 * len(GENOTYPES) + 2, "C", "G", "1|1", ".", fmt) for fmt in ("GT:DP", "DP:GT", "GTX", "")]
    text = vcf(rows)
    outs = []
    for h in (1, 2):
        r = check(ctx, text, [("c", seq)], haplotype=h)
        for (gt, *want), row in zip(GENOTYPES, r.rows):
            w = want[h - 1]
            assert row["cls"] == ("malformed" if w == "malformed" else "no_call" if w is None else "ref_allele" if w == 0 else "applied"), (gt, h)
        assert verdicts(r)[-4:] == ["applied", "malformed", "malformed", "malformed"]
        outs.append(r.fasta)
    assert outs[0] != outs[1]
    # three samples: columns 0 and 2
    three = HEAD[:-1] + b"\tNA3\n" + b"".join(b"c\t%d\t.\tC\tG,T\t.\t.\t.\tGT\t%s\t9|9\t%s\n" % (4 * k + 2, a, b)
                                              for k, (a, b) in enumerate(((b"0|1", b"2|0"), (b"1|1", b"."), (b"2", b"1/2"), (b".|2", b"0|0"))))
    seen = set()
    for sample in (0, 2):
        for h in (1, 2):
            seen.add(check(ctx, three, [("c", seq)], haplotype=h, sample=sample, modes=(1,)).fasta)
    assert len(seen) == 4 and check(ctx, three, [("c", seq)], haplotype=1, sample=1, modes=(1,)).malformed == 4
    assert ctx.apply_vcf(three, [("c", seq)], haplotype=2, sample="NA3")[2] == M.apply(three, [("c", seq)], haplotype=2, sample=2).fasta


# ---------------------------------------------------------------- the sink
def test_pieces_of_seven_bytes_and_a_sink_that_stops(ctx):
    want = M.apply(WORKED_VCF, WORKED_GENOME, lines=1)
    pieces = ([], [])

    def take(which):
        def f(user, ptr, n, offset):
            pieces[which].append((offset, C.string_at(ptr, n)))
            return 1
        return f
    keep = [(nm.encode(), bytes(lines)) for nm, lines in WORKED_GENOME]
    refs = (P.ErrorsRef * 3)(*[P.ErrorsRef(nm, C.cast(C.c_char_p(lines), C.c_void_p), len(lines)) for nm, lines in keep])
    opts, res = P.ApplyOpts(0, 0, 1, 60, 7), P.ApplyResult()
    sink = P.ApplySink(None, P.APPLY_TEXT_CB(take(0)), P.APPLY_TEXT_CB(take(1)), P.APPLY_RECORD_CB(), P.APPLY_ORIGIN_CB())
    args = (ctx.h, refs, 3, None, WORKED_VCF, len(WORKED_VCF), C.byref(opts))
    assert ctx.lib.pbsim_vcf_apply(*args, C.byref(sink), C.byref(res)) == 1
    for got, text in zip(pieces, (want.fasta, want.text)):
        at = 0
        for offset, p in got:
            assert offset == at and 1 <= len(p) <= 7
            at += len(p)
        assert b"".join(p for _, p in got) == text and len(got) == -(-len(text) // 7)
    assert res.fasta_bytes == len(want.fasta) and res.text_bytes == len(want.text)
    # a sink that stops: the call fails, the result is zeroed, the context stays usable
    for stop in (P.ApplySink(None, P.APPLY_TEXT_CB(lambda *a: 0), P.APPLY_TEXT_CB(), P.APPLY_RECORD_CB(), P.APPLY_ORIGIN_CB()),
                 P.ApplySink(None, P.APPLY_TEXT_CB(), P.APPLY_TEXT_CB(lambda *a: 0), P.APPLY_RECORD_CB(), P.APPLY_ORIGIN_CB()),
                 P.ApplySink(None, P.APPLY_TEXT_CB(), P.APPLY_TEXT_CB(), P.APPLY_RECORD_CB(lambda *a: 0), P.APPLY_ORIGIN_CB()),
                 P.ApplySink(None, P.APPLY_TEXT_CB(), P.APPLY_TEXT_CB(), P.APPLY_RECORD_CB(), P.APPLY_ORIGIN_CB(lambda *a: 0))):
        assert ctx.lib.pbsim_vcf_apply(*args, C.byref(stop), C.byref(res)) == 0
        assert b"sink aborted" in ctx.lib.pbsim_last_error() and res.lines == 0 and res.fasta_bytes == 0
    check(ctx, WORKED_VCF, WORKED_GENOME)


def test_ref_names(ctx):
    names = ["chr_c1", "chr_c2", "chr_c3"]
    renamed = b"".join((b"chr_" + l if not l.startswith(b"#") else l) + b"\n" for l in WORKED_VCF.split(b"\n") if l)
    r = check(ctx, renamed, WORKED_GENOME, ref_names=names)
    assert r.fasta == WORKED_FASTA[0]                                                 # (the FASTA keeps the records' own names)
    assert check(ctx, WORKED_VCF, WORKED_GENOME, ref_names=names).unknown_contig == 18


# ---------------------------------------------------------------- through the command line
def test_cli_applies_the_mutate_modes_vcf(ctx, tmp_path):
    genome = [(n, lines) for n, lines in four_records(12) if len(lines) > 100]      # (the command line's loader takes records of 100 bases or more)
    fa = b"".join(b">" + n.encode() + b" a description\n" + lines + (b"" if lines.endswith(b"\n") or not lines else b"\n") for n, lines in genome)
    (tmp_path / "genome.fa").write_bytes(fa)
    cmd = [CLI, "--mutate-genome", "genome.fa", "--mutate-out", "variant.fa", "--mutate-vcf", "truth.vcf", "--mutate-seed", "77", "--mutate-snv-ppm", "40000",
           "--mutate-ins-ppm", "20000", "--mutate-del-ppm", "20000", "--mutate-line-width", "50"]
    r = subprocess.run(cmd, capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    truth = (tmp_path / "truth.vcf").read_bytes()
    (tmp_path / "truth.vcf.gz").write_bytes(W.bgzf(truth, block=700))
    (tmp_path / "genome.fa.gz").write_bytes(W.bgzf(fa, block=900))
    want = M.apply(truth, genome, line_width=50, lines=1)
    for gz in ("", ".gz"):
        cmd = [CLI, "--apply-vcf", "truth.vcf" + gz, "--apply-genome", "genome.fa" + gz, "--apply-out", "applied.fa", "--apply-line-width", "50",
               "--apply-origin", "origin.bin", "--apply-report", "lines.tsv", "--apply-lines", "all"]
        r = subprocess.run(cmd, capture_output=True, cwd=str(tmp_path), timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        assert (tmp_path / "applied.fa").read_bytes() == (tmp_path / "variant.fa").read_bytes() == want.fasta
        assert r.stdout == want.report and (tmp_path / "lines.tsv").read_bytes() == want.text and want.applied > 50
        origin = (tmp_path / "origin.bin").read_bytes()
        assert len(origin) == 4 * want.bases_out and origin == b"".join(o.astype("<i4").tobytes() for o in want.origins)
        for name in ("applied.fa", "origin.bin", "lines.tsv"):
            os.unlink(str(tmp_path / name))
    # a sample by name, a haplotype without any sample column, names that do not fit: a failure leaves no file behind
    phased = b"##x\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tmum\tkid\n" + b"".join(
        l + b"\tGT\t%s\t%s\n" % ((b"0|1", b"1|0")[k % 2], (b"1|1", b"0|1", b".|0")[k % 3]) for k, l in enumerate(lines_of(truth)))
    (tmp_path / "phased.vcf").write_bytes(phased)
    for h, sample, column in ((2, "kid", 1), (1, "0", 0)):
        cmd = [CLI, "--apply-vcf", "phased.vcf", "--apply-genome", "genome.fa", "--apply-out", "h.fa", "--apply-haplotype", str(h), "--apply-sample", sample]
        r = subprocess.run(cmd, capture_output=True, cwd=str(tmp_path), timeout=300)
        want = M.apply(phased, genome, haplotype=h, sample=column)
        assert r.returncode == 0 and r.stdout == want.report and (tmp_path / "h.fa").read_bytes() == want.fasta and 0 < want.applied < want.lines, r.stderr[-2000:]
    base = [CLI, "--apply-genome", "genome.fa", "--apply-out", "bad.fa", "--apply-report", "bad.tsv", "--apply-origin", "bad.bin"]
    for extra, word in ((["--apply-vcf", "truth.vcf", "--apply-haplotype", "1"], b"no data line has a sample column 0"),
                        (["--apply-vcf", "phased.vcf", "--apply-haplotype", "1", "--apply-sample", "dad"], b"(apply-sample: dad)"),
                        (["--apply-vcf", "truth.vcf", "--apply-ref-names", "a"], b"(apply-ref-names): 1 names for 2 genome records")):
        r = subprocess.run(base + extra, capture_output=True, cwd=str(tmp_path), timeout=300)
        assert r.returncode != 0 and word in r.stderr and not any((tmp_path / n).exists() for n in ("bad.fa", "bad.tsv", "bad.bin")), (extra, r.stderr[-2000:])
