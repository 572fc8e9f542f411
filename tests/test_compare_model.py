"""tests/compare_model.py (the rule of `pbsim --compare-vcf`) held to a case worked out by hand and to the properties of the canonical
form; and the places where the feature shows without a GPU: the ABI's declarations with their ctypes mirror and the built library's
symbols, pbsim_compare_report against the model, the option mirror with the command line's refusals, the checks in front of any
device work, and the HIP-free rule file under the sanitizers."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import compare_model as M
import harness
import mutate_model as G
import pbsim3_amd as P
from pbsim3_amd import args as A

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def vcf(rows, head=b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"):
    """rows of (chrom, pos, ref, alt[, info[, filter]]) as a VCF text"""
    out = [head]
    for row in rows:
        chrom, pos, ref, alt = row[:4]
        info, fil = (row[4] if len(row) > 4 else "."), (row[5] if len(row) > 5 else ".")
        out.append(("%s\t%s\t.\t%s\t%s\t.\t%s\t%s\n" % (chrom, pos, ref, alt, fil, info)).encode())
    return b"".join(out)


# ---------------------------------------------------------------- the worked case of the rule
# c1 = GCAAAATCGTGTGA.  The truth's `6 A AA` loses its last A (s = 5) and walks left through the As to s = 2: (2, 0, A), three steps;
# `8 CGT C` loses its first C: (8, 2, ), and C in front of it is not T.  Of the calls `3 A AA` is (2, 0, A) with no step; `10 TGT T`
# loses its last T, is TG at s = 9 and takes one step (the G at 8) to (8, 2, ); `4 AAAT AT` loses T and A, is AA at s = 3 and takes one
# step to (2, 2, ): no truth line has that form, but the truth's insertion lies at the same (r, s) = (c1, 2), so by the rule it is
# fp_site, as `2 C G` is beside the truth's `2 C T`; `12 T TC` is (12, 0, C), where nothing of the truth lies: fp.
WORKED_GENOME = [("c1", b"GCAAAAT\nCGTGTGA\n")]
WORKED_TRUTH = vcf([("c1", 2, "C", "T", "TYPE=snv"), ("c1", 6, "A", "AA", "TYPE=ins"), ("c1", 8, "CGT", "C", "TYPE=del"), ("c1", 14, "A", "C", "TYPE=snv")])
WORKED_CALLS = vcf([("c1", 2, "C", "T", "DP=3;MS=3;TYPE=snv"), ("c1", 3, "A", "AA", "DP=3;MS=2;TYPE=ins"), ("c1", 10, "TGT", "T", "DP=3;MS=3;TYPE=del"),
                    ("c1", 2, "C", "G", "DP=3;MS=1;TYPE=snv"), ("c1", 12, "T", "TC", "DP=3;MS=70;TYPE=ins"), ("c1", 5, "AA", "AA", "DP=3;MS=3;TYPE=snv"),
                    ("c1", 4, "AAAT", "AT", "DP=3;MS=2;TYPE=del")])
WORKED_FORMS = [[(1, 1, b"T"), (2, 0, b"A"), (8, 2, b""), (13, 1, b"C")],
                [(1, 1, b"T"), (2, 0, b"A"), (8, 2, b""), (1, 1, b"G"), (12, 0, b"C"), None, (2, 2, b"")]]
WORKED_VERDICTS = [["found", "found", "found", "missed"], ["tp", "tp", "tp", "fp_site", "fp", "no_change", "fp_site"]]
WORKED_MATES = [[1, 2, 3, 0], [1, 2, 3, 0, 0, 0, 0]]
WORKED_REPORT = (b"#\tlines\tmalformed\tunknown_contig\tunsupported\tref_mismatch\tfiltered\tno_change\tdup\tcompared\tshifted\tlongest_shift\n"
                 b"T\t4\t0\t0\t0\t0\t0\t0\t0\t4\t1\t3\n"
                 b"C\t7\t0\t0\t0\t0\t0\t1\t0\t6\t2\t1\n"
                 b"P\tsnv\t2\t1\t2\t1\t1\t1\t500000\t500000\n"
                 b"P\tins\t1\t1\t2\t1\t1\t0\t1000000\t500000\n"
                 b"P\tdel\t1\t1\t2\t1\t1\t1\t1000000\t500000\n"
                 b"P\tcomplex\t0\t0\t0\t0\t0\t0\t0\t0\n"
                 b"P\tall\t4\t3\t6\t3\t3\t2\t750000\t500000\n"
                 b"L\tins\t1\t1\t1\t2\t1\n"
                 b"L\tdel\t2-5\t1\t1\t2\t1\n"
                 b"Q\t1\t0\t1\t3\t3\n"
                 b"Q\t2\t1\t1\t3\t2\n"
                 b"Q\t3\t2\t0\t2\t1\n"
                 b"Q\t63\t0\t1\t0\t1\n")
WORKED_HEADER = b"#file\tline\tCHROM\tPOS\tREF\tALT\ttype\tstart\tref_len\talt\tverdict\tmate\n"
WORKED_CONCORDANT = [b"T\t1\tc1\t2\tC\tT\tsnv\t2\t1\tT\tfound\t1\n", b"T\t2\tc1\t6\tA\tAA\tins\t3\t0\tA\tfound\t2\n", b"T\t3\tc1\t8\tCGT\tC\tdel\t9\t2\t.\tfound\t3\n",
                     b"C\t1\tc1\t2\tC\tT\tsnv\t2\t1\tT\ttp\t1\n", b"C\t2\tc1\t3\tA\tAA\tins\t3\t0\tA\ttp\t2\n", b"C\t3\tc1\t10\tTGT\tT\tdel\t9\t2\t.\ttp\t3\n"]
WORKED_DISCORDANT = [b"T\t4\tc1\t14\tA\tC\tsnv\t14\t1\tC\tmissed\t0\n", b"C\t4\tc1\t2\tC\tG\tsnv\t2\t1\tG\tfp_site\t0\n",
                     b"C\t5\tc1\t12\tT\tTC\tins\t13\t0\tC\tfp\t0\n", b"C\t6\tc1\t5\tAA\tAA\t.\t.\t.\t.\tno_change\t0\n",
                     b"C\t7\tc1\t4\tAAAT\tAT\tdel\t3\t2\t.\tfp_site\t0\n"]
WORKED_TEXT = WORKED_HEADER + b"".join(WORKED_DISCORDANT)
WORKED_TEXT_ALL = WORKED_HEADER + b"".join(WORKED_CONCORDANT[:3] + WORKED_DISCORDANT[:1] + WORKED_CONCORDANT[3:] + WORKED_DISCORDANT[1:])


def test_the_worked_case():
    r = M.compare(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME)
    forms = [[None if row[1] in M.CLASSES else (row[3], row[4], row[5]) for row in rows] for rows in r.rows]
    assert forms == WORKED_FORMS
    assert [[row[8] for row in rows] for rows in r.rows] == WORKED_VERDICTS and [[row[9] for row in rows] for rows in r.rows] == WORKED_MATES
    assert r.report == WORKED_REPORT and r.text == WORKED_TEXT and r.text_bytes == len(WORKED_TEXT) and M.TEXT_HEADER == WORKED_HEADER
    everything = M.compare(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME, lines=1)
    assert everything.text == WORKED_TEXT_ALL and everything.report == WORKED_REPORT and everything.text_bytes == len(WORKED_TEXT_ALL)
    assert len(M.flat(r)) == 215 and M.flat(r)[:-1] == M.flat(everything)[:-1]
    # min_ms 3 filters the calls with MS 2 and 1: two of the truth's lines are missed now
    strict = M.compare(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME, min_ms=3)
    assert strict.files[1][5:9] == [3, 1, 0, 3] and [row[8] for row in strict.rows[0]] == ["found", "missed", "found", "missed"]
    assert [row[8] for row in strict.rows[1]] == ["tp", "filtered", "tp", "filtered", "fp", "no_change", "filtered"]
    assert b"Q\t3\t2\t0\t2\t1\n" in strict.report and b"Q\t2\t" not in strict.report


# ---------------------------------------------------------------- the properties of the form
def random_line(rng, seq, letters):
    """a line whose REF is the genome's: (pos, ref, alt) with REF and ALT of 1 .. 6 bases that differ"""
    while True:
        n = rng.randrange(1, 7)
        s = rng.randrange(0, len(seq) - n + 1)
        ref, alt = seq[s:s + n], bytes(rng.choice(letters) for _ in range(rng.randrange(1, 7)))
        if ref != alt:
            return s + 1, ref, alt


@pytest.mark.parametrize("letters", [b"AC", b"ACGT"])
def test_the_form_applied_to_the_genome_is_the_line_applied(letters):
    rng = random.Random(len(letters))
    moved = 0
    for _ in range(200):
        seq = bytes(rng.choice(letters) for _ in range(rng.randrange(6, 40)))
        for _ in range(20):
            pos, ref, alt = random_line(rng, seq, letters)
            s, d, x, shift = M.form_of(pos, ref, alt, seq)
            assert seq[:s] + x + seq[s + d:] == seq[:pos - 1] + alt + seq[pos - 1 + len(ref):], (seq, pos, ref, alt)
            assert (s, d, x) == M.form_of(pos, ref, alt, seq, suffix_first=False)[:3], (seq, pos, ref, alt)
            assert M.form_of(s + 1, seq[s:s + d], x, seq) == (s, d, x, 0), (seq, pos, ref, alt)      # the form is its own form
            assert not (d and x) or (seq[s] != x[0] and seq[s + d - 1] != x[-1])                        # nothing is left to trim
            assert (d and x) or s == 0 or seq[s - 1] != (x or seq[s:s + d])[-1]                         # and nothing to move
            moved += shift > 0
    assert moved > 50                                   # (the left move is exercised: more than one line in a hundred of the 4000)


def test_two_placements_of_one_indel_have_one_form():
    seq = b"GCAAAATCGTGTGACACACAG"
    assert M.form_of(6, b"A", b"AA", seq)[:3] == M.form_of(3, b"A", b"AA", seq)[:3] == M.form_of(2, b"C", b"CA", seq)[:3] == (2, 0, b"A")
    assert M.form_of(8, b"CGT", b"C", seq)[:3] == M.form_of(10, b"TGT", b"T", seq)[:3] == M.form_of(9, b"GTG", b"G", seq)[:3] == (8, 2, b"")
    # an inserted CA anywhere in the run ACACACA at 13 .. 19 (0-based): the leftmost placement spells it AC, in front of the run's first A
    assert {M.form_of(p, seq[p - 1:p], seq[p - 1:p] + (b"AC" if seq[p - 1:p] == b"C" else b"CA"), seq)[:3] for p in range(14, 21)} == {(13, 0, b"AC")}
    assert M.form_of(20, b"A", b"ACA", seq)[3] == 6 and M.form_of(16, b"A", b"ACA", seq)[3] == 2 and M.form_of(13, b"G", b"GAC", seq)[3] == 0


def test_a_shift_stops_at_position_0_and_does_not_look_in_front():
    genome = [("a", b"TTTT"), ("b", b"TTTTTC")]
    truth = vcf([("b", 5, "T", "TT"), ("b", 4, "TT", "T"), ("a", 4, "T", "TTT")])
    r = M.compare(truth, vcf([("b", 1, "T", "TT"), ("b", 1, "TT", "T"), ("a", 1, "T", "TTT")]), genome)
    assert [tuple(row[2:7]) for row in r.rows[0]] == [(1, 0, 0, b"T", 4), (1, 0, 1, b"", 3), (0, 0, 0, b"TT", 3)]
    assert [row[8] for row in r.rows[0]] == ["found"] * 3 and [row[8] for row in r.rows[1]] == ["tp"] * 3
    assert r.files[0][9:] == [3, 4] and r.files[1][9:] == [0, 0]


def test_a_mutate_models_truth_against_itself_is_all_found():
    genome = [("a", harness.synth_bases(3000, 7).tobytes() + b"\n"), ("none", b""), ("b", harness.synth_bases(777, 8).tobytes())]
    t = G.mutate(genome, snv_ppm=50000, ins_ppm=30000, del_ppm=30000)
    r = M.compare(t.vcf, t.vcf, genome, lines=1)
    assert r.files[0] == r.files[1] and r.files[0][0] == t.variants == r.files[0][8] and sum(r.files[0][1:8]) == 0
    assert [v[0] for v in r.types[:3]] == t.types and r.types[3] == [0] * 6
    assert all(v[0] == v[1] == v[2] == v[3] and v[4] == v[5] == 0 for v in r.types)
    assert {row[8] for row in r.rows[0]} == {"found"} and {row[8] for row in r.rows[1]} == {"tp"} and r.files[0][9] > 10
    assert [row[9] for row in r.rows[0]] == list(range(1, t.variants + 1))
    assert M.compare(t.vcf, t.vcf, genome).text == M.TEXT_HEADER


def test_every_class_by_one_line():
    genome = [("c1", b"ACGTNACGTACGT"), ("c2", b"acgtt")]
    rows = [b"c1\t2\t.\tC", b"\t2\t.\tC\tT", b"c1\t2\t.\t\tT", b"c1\t2\t.\tC\t", b"c1\t0\t.\tC\tT", b"c1\t2147483648\t.\tC\tT", b"c1\t2x\t.\tC\tT",
            b"c1\t\t.\tC\tT", b"c1\t+2\t.\tC\tT",                                                   # malformed: 9
            b"c3\t2\t.\tC\tT", b"c\t2\t.\tC\tT", b"c11\t2\t.\tC\tT", b"C1\t2\t.\tC\tT",                # unknown_contig: 4
            b"c1\t2\t.\tC\tT,G", b"c1\t2\t.\tC\t<DEL>", b"c1\t2\t.\tC\t*", b"c1\t2\t.\tC\t.", b"c1\t2\t.\tR\tT",   # unsupported: 5
            b"c1\t2\t.\tG\tT", b"c1\t12\t.\tGTA\tG", b"c1\t14\t.\tA\tT", b"c2\t6\t.\tA\tT",            # ref_mismatch: 4
            b"c1\t2\t.\tC\tT\t.\tLowQual\tMS=9", b"c1\t2\t.\tC\tT\t.\t\tMS=9", b"c1\t2\t.\tC\tT\t.\tpass",   # filtered: 3
            b"c1\t2\t.\tC\tc", b"c2\t1\t.\tac\tAC\t.\tPASS",                                          # no_change: 2
            b"c1\t0000000002\t.\tc\tt\t.\tPASS\tDP=1;XMS=5;MS=7x;MS=9", b"c1\t5\t.\tN\tA\t.\t.", b"c2\t4\t.\tTT\tT\t.\t.\tMS=;MS=4",
            b"c1\t2\t.\tC\tT\t.\t.\tMS=99999999999\textra\tcolumns"]                                  # compared: 3, and a dup
    text = b"\n".join(rows) + b"\n"
    r = M.compare(text, text, genome, lines=1, min_ms=1)
    assert r.files[0] == [31, 9, 4, 5, 4, 3, 2, 1, 3, 0, 0]
    assert r.files[1] == [31, 9, 4, 5, 4, 7, 0, 1, 1, 0, 0]                                            # MS 0 is below min_ms: lines 26, 27, 29 and 30
    assert [row[7] for row in r.rows[1][27:]] == [7, 0, 0, 2147483647]
    assert [tuple(row[2:7]) for row in r.rows[0][27:]] == [(0, 1, 1, b"T", 0), (0, 4, 1, b"A", 0), (1, 3, 1, b"", 0), (0, 1, 1, b"T", 0)]
    assert [row[8] for row in r.rows[0][27:]] == ["found", "missed", "missed", "dup"] and [row[8] for row in r.rows[1][27:]] == ["tp", "filtered", "filtered", "dup"]
    assert [row[9] for row in r.rows[0][27:]] == [28, 0, 0, 0] and [row[9] for row in r.rows[1][27:]] == [28, 0, 0, 0]
    lines = r.text.split(b"\n")
    assert lines[1] == b"T\t1\tc1\t2\tC\t.\t.\t.\t.\t.\tmalformed\t0" and lines[2] == b"T\t2\t.\t2\tC\tT\t.\t.\t.\t.\tmalformed\t0"
    assert lines[28] == b"T\t28\tc1\t0000000002\tc\tt\tsnv\t2\t1\tT\tfound\t28" and lines[31] == b"T\t31\tc1\t2\tC\tT\tsnv\t2\t1\tT\tdup\t0"
    assert r.ms[7] == [1, 0] and sum(sum(v) for v in r.ms) == 1


def test_line_ends():
    genome = [("c1", b"ACGTACGT")]
    plain = b"#h\nc1\t2\t.\tC\tT\n\nc1\t3\t.\tG\tGA\t.\tPASS\n"
    want = M.compare(plain, plain, genome, lines=1)
    assert want.files[0][0] == 2 and want.files[0][8] == 2
    crlf = plain.replace(b"\n", b"\r\n")
    assert crlf.count(b"\r\n") == 4
    for text in (crlf, plain[:-1], crlf[:-2], b"\n\n" + plain + b"#\n\r\n"):
        got = M.compare(text, plain, genome, lines=1)
        assert got.report == want.report and got.text == want.text, text
    # without the \n behind it the \r belongs to the last column: PASS\r is no PASS, and an ALT of GA\r is unsupported
    assert M.compare(crlf[:-1], plain, genome).files[0][5] == 1
    assert M.compare(plain[:-8] + b"\r", plain, genome).files[0][3] == 1 and M.compare(b"\r", plain, genome).files[0][:2] == [1, 1]
    assert M.compare(b"", b"#only\n", genome, lines=1).text == M.TEXT_HEADER and M.compare(b"", b"", genome).files == [[0] * 11, [0] * 11]


def test_ref_names_map_the_contigs_to_the_records():
    genome = [("x", b"ACGT"), ("y", b"TTGCA")]
    text = vcf([("x", 2, "C", "T"), ("y", 3, "G", "T")])
    assert M.compare(text, text, genome).files[0][8] == 2
    swapped = M.compare(text, text, genome, ref_names=["y", "x"])                  # x is the record TTGCA now: its T at 2 is no C; ACGT has its G at 3
    assert swapped.files[0][4] == 1 and swapped.files[0][8] == 1 and swapped.rows[0][1][2] == 0
    renamed = M.compare(text.replace(b"x\t", b"chr1\t"), text.replace(b"x\t", b"chr1\t"), genome, ref_names=["chr1", "y"])
    assert renamed.files[0][8] == 2
    for bad in (["x"], ["x", ""], ["x", "x"]):
        with pytest.raises(ValueError):
            M.compare(text, text, genome, ref_names=bad)


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_calls_and_the_library_has_them():
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        h = f.read()
    assert re.search(r"int pbsim_vcf_compare\(pbsim_ctx \*ctx, const pbsim_errors_ref \*refs, int n_refs, const char \*const \*ref_names, const void \*truth, "
                     r"int64_t n_truth,\s*const void \*calls, int64_t n_calls, const pbsim_compare_opts \*opts, const pbsim_compare_sink \*sink,\s*"
                     r"pbsim_compare_result \*result\);", h)
    assert re.search(r"int64_t pbsim_compare_report\(const pbsim_compare_result \*result, char \*buf, int64_t cap\);", h)
    opts = re.search(r"typedef struct pbsim_compare_opts \{(.*?)\} pbsim_compare_opts;", h, re.S).group(1)
    assert re.findall(r"^\s*(\w+ [\w, ]+);", opts, re.M) == ["int32_t lines", "int32_t min_ms", "int64_t piece_bytes"]
    body = re.search(r"typedef struct pbsim_compare_result \{(.*?)\} pbsim_compare_result;", h, re.S).group(1)
    declared = [(name, [int(d) for d in re.findall(r"\[(\d+)\]", dims)]) for name, dims in re.findall(r"int64_t (\w+)((?:\[\d+\])*);", body)]
    assert declared == [("files", [2, 11]), ("types", [4, 6]), ("lengths", [2, 5, 4]), ("ms", [64, 2]), ("text_bytes", [])]
    assert [n for n, _ in P.CompareResult._fields_] == [n for n, _ in declared] and C.sizeof(P.CompareResult) == 8 * 215
    assert {n: list(s) for n, s in P.COMPARE_SHAPES.items()} == {n: d for n, d in declared if d}
    assert (len(M.FILE_NAMES), len(M.TYPES), len(M.TYPE_NAMES), len(M.BINS), len(M.LENGTH_NAMES), M.MS_BINS) == (11, 4, 6, 5, 4, 64)
    sink = re.search(r"typedef struct pbsim_compare_sink \{(.*?)\} pbsim_compare_sink;", h, re.S).group(1)
    assert re.findall(r"\(\*(\w+)\)", sink) == ["on_text"] == [n for n, _ in P.CompareSink._fields_[1:]]
    assert [n for n, _ in P.CompareOpts._fields_] == ["lines", "min_ms", "piece_bytes"] and C.sizeof(P.CompareOpts) == 16
    bound = [name for name, _, _ in P.API]
    assert "pbsim_vcf_compare" in bound and "pbsim_compare_report" in bound
    assert callable(getattr(P.Context, "compare_vcf")) and callable(P.compare_report) and P.COMPARE_LINES == {"discordant": 0, "all": 1}
    lib = P.load()
    assert hasattr(lib, "pbsim_vcf_compare") and hasattr(lib, "pbsim_compare_report")


def as_dict(r):
    return dict(files=r.files, types=r.types, lengths=r.lengths, ms=r.ms, text_bytes=r.text_bytes)


Numbers = __import__("collections").namedtuple("Numbers", "files types lengths ms text_bytes")


def random_numbers(rng):
    pick = lambda: rng.choice([0, 0, 0, 1, 10 ** 12, rng.randrange(2 ** 40)])
    return Numbers([[pick() for _ in range(11)] for _ in range(2)], [[pick() for _ in range(6)] for _ in range(4)],
                   [[[pick() for _ in range(4)] for _ in range(5)] for _ in range(2)], [[pick() for _ in range(2)] for _ in range(64)], pick())


ZERO_REPORT = (WORKED_REPORT.split(b"\n")[0] + b"\nT" + b"\t0" * 11 + b"\nC" + b"\t0" * 11 + b"\n" +
               b"".join(b"P\t%s" % t + b"\t0" * 8 + b"\n" for t in (b"snv", b"ins", b"del", b"complex", b"all")))


def test_report_of_the_library_is_the_models_without_a_device():
    r = M.compare(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME)
    assert P.compare_report(as_dict(r)) == WORKED_REPORT
    assert P.compare_report({}) == ZERO_REPORT == M.report([[0] * 11] * 2, [[0] * 6] * 4, [[[0] * 4] * 5] * 2, [[0, 0]] * 64)
    rng = random.Random(53)
    for _ in range(30):
        x = random_numbers(rng)
        assert P.compare_report(as_dict(x)) == M.report(x.files, x.types, x.lengths, x.ms)
    assert P.load().pbsim_compare_report(None, None, 0) == -1
    with pytest.raises(ValueError, match="types has the shape"):
        P.compare_report(dict(types=[[0] * 6] * 3))


# ---------------------------------------------------------------- the option mirror and the command line
GOOD = ["--compare-vcf", "calls.vcf", "--compare-truth", "truth.vcf", "--compare-genome", "g.fa"]
TAKES = "--compare-vcf takes --compare-truth, --compare-genome, --compare-out, --compare-lines, --compare-min-ms, --compare-ref-names and --device"
REFUSED = [
    (GOOD + ["--depth", "3"], "(--depth): " + TAKES),
    (GOOD + ["--call-out", "x"], "(--call-out): " + TAKES),
    (GOOD + ["--genome", "x"], "(--genome): " + TAKES),
    (GOOD + ["--mutate-genome", "x"], "(--compare-vcf): --mutate-genome takes"),
    (["--compare-truth", "t", "--compare-vcf"], "needs a value"),
    (["--compare-vcf", "c", "--compare-genome", "g"], "--compare-vcf needs --compare-truth VCF"),
    (["--compare-vcf", "c", "--compare-truth", "t"], "--compare-vcf needs --compare-genome FASTA"),
    (GOOD + ["--compare-lines", "some"], "(compare-lines: some): discordant or all."),
    (GOOD + ["--compare-min-ms", "-1"], "(compare-min-ms: -1): a whole number, 0 .. 2147483647."),
    (GOOD + ["--compare-min-ms", "2147483648"], "(compare-min-ms: 2147483648): a whole number, 0 .. 2147483647."),
    (GOOD + ["--compare-min-ms", "1e3"], "(compare-min-ms: 1e3): a whole number"),
    (GOOD + ["--compare-ref-names", "a,,b"], "(compare-ref-names): an empty name."),
    (GOOD + ["--devices", "0,1"], "--compare-vcf runs on one GPU"),
    (GOOD + ["--processes", "2"], "--compare-vcf runs on one GPU"),
]


def test_option_mirror_accepts_and_rejects():
    assert A.compare_vcf(GOOD) == dict(calls="calls.vcf", truth="truth.vcf", genome="g.fa", out=None, lines="discordant", min_ms=0, ref_names=None)
    got = A.compare_vcf(["--compare-out", "o", "--compare-min-ms", "2147483647", "--device", "1", "--compare-genome", "g", "--compare-lines", "all",
                         "--compare-ref-names", "a,b", "--compare-truth", "t", "--compare-vcf", "c"])
    assert got == dict(calls="c", truth="t", genome="g", out="o", lines="all", min_ms=2147483647, ref_names=["a", "b"])
    for argv, message in REFUSED + [(["--compare-truth", "t"], "--compare-vcf CALLS: name the call set")]:
        if "--mutate-genome" in argv:
            continue                                # (the binary hands that line to the mutate stage's mode, which refuses it)
        with pytest.raises(ValueError) as e:
            A.compare_vcf(argv)
        assert message in str(e.value), argv


def test_cli_refuses_from_the_command_line_alone(tmp_path):
    """the same refusals by the binary, with the mirror's words, before a device or a file is touched"""
    import pbsim3_amd.build as b
    b.build()
    for argv, message in REFUSED:
        r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and r.stdout == "" and message in r.stderr, (argv, r.stderr[-500:])
    r = subprocess.run([CLI] + GOOD + ["--compare-out", "o.tsv"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "Cannot open file: calls.vcf" in r.stderr
    assert os.listdir(tmp_path) == []
    r = subprocess.run([CLI], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert "--compare-vcf CALLS --compare-truth TRUTH --compare-genome FASTA" in r.stderr + r.stdout
    assert "--compare-vcf" in (r.stderr + r.stdout).split("--mutate-genome FASTA")[1].split("pbsim --compare-vcf")[0]   # the mutate mode points here


# ---------------------------------------------------------------- the checks in front of any device work
REFUSED_OPTS = [(dict(lines=2), "lines must be 0"), (dict(lines=-1), "lines must be 0"), (dict(min_ms=-1), "min_ms must be 0 .. 2147483647"),
                (dict(piece_bytes=-1), "piece_bytes must not be negative")]


def test_bad_arguments_fail_before_device_work():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), -1) as c:
        for kw, word in REFUSED_OPTS:
            with pytest.raises(P.PbsimError, match="pbsim_vcf_compare: " + word):
                c.compare_vcf(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME, **kw)
        with pytest.raises(P.PbsimError, match="pbsim_vcf_compare: bad argument"):
            c.compare_vcf(WORKED_TRUTH, WORKED_CALLS, [])
        with pytest.raises(P.PbsimError, match=r"pbsim_vcf_compare: the genome holds two records named \"c1\" \(records 0 and 1\)"):
            c.compare_vcf(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME + [("c1", b"AC")])
        with pytest.raises(P.PbsimError, match=r"pbsim_vcf_compare: ref_names: two genome records are named \"a\" \(records 0 and 1\)"):
            c.compare_vcf(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME + [("c2", b"AC")], ref_names=["a", "a"])
        with pytest.raises(P.PbsimError, match="pbsim_vcf_compare: ref_names: genome record 0 has no name"):
            c.compare_vcf(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME, ref_names=[""])
        with pytest.raises(ValueError, match="one entry per genome record"):
            c.compare_vcf(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME, ref_names=["a", "b"])
        for kw in (dict(min_ms=2 ** 31), dict(lines=2 ** 40)):
            with pytest.raises(ValueError, match="does not fit its 32-bit field"):
                c.compare_vcf(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME, **kw)
        # a missing text with a length, through the library itself
        refs = (P.ErrorsRef * 1)(P.ErrorsRef(b"c1", None, 0))
        res = P.CompareResult()
        assert c.lib.pbsim_vcf_compare(c.h, refs, 1, None, None, 5, b"", 0, None, None, C.byref(res)) == 0
        assert b"pbsim_vcf_compare: bad argument" in c.lib.pbsim_last_error()
        # good arguments reach the device check: a tables-only context refuses as pbsim_inflate_buffer does, and stays usable
        for kw in (dict(), dict(text=False), dict(lines="all", min_ms=2 ** 31 - 1, piece_bytes=7, ref_names=["c1"]), dict(lines=1)):
            with pytest.raises(P.PbsimError, match="no HIP device"):
                c.compare_vcf(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME, **kw)
        with pytest.raises(P.PbsimError, match="no HIP device"):
            c.compare_vcf(b"", b"", WORKED_GENOME)


# ---------------------------------------------------------------- the host's decisions under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("asan") / "vcf_compare_rule_driver")
    p = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(harness.ROOT, "tests", "asan", "vcf_compare_rule_driver.cpp"), os.path.join(csrc, "vcf_compare_rule.cpp"),
                        "-o", exe], capture_output=True, text=True)
    if p.returncode != 0 and "sanitize" in p.stderr:
        pytest.skip("no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def drive(exe, *argv):
    p = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, timeout=60)
    assert p.returncode == 0, (argv, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout


def fnv1a(name):
    h = 0xcbf29ce484222325
    for c in name:
        h = ((h ^ c) * 0x100000001b3) % 2 ** 64
    return h


def test_rule_code_under_asan(driver):
    assert drive(driver, "opts", "-") == b"opts 0 0 8388608\n"
    assert drive(driver, "opts", 1, 2147483647, 7) == b"opts 1 2147483647 7\n"
    for bad, word in (((2, 0, 0), b"lines"), ((-1, 0, 0), b"lines"), ((0, -1, 0), b"min_ms"), ((0, 0, -1), b"piece_bytes")):
        assert drive(driver, "opts", *bad).startswith(b"opts refused: " + word), bad
    names = ["chr%d" % k for k in range(40)] + ["x" * 300, "c1"]
    want = sorted((fnv1a(n.encode()), r, n) for r, n in enumerate(names))
    assert fnv1a(b"") == 0xcbf29ce484222325 and fnv1a(b"a") == 0xaf63dc4c8601ec8c
    for how in ("own", "given"):
        assert drive(driver, "names", how, *names) == b"".join(b"%016x %d %s\n" % (h, r, n.encode()) for h, r, n in want)
        assert drive(driver, "names", how, "a", "b", "a").startswith(b"names refused: " + (b"ref_names: " if how == "given" else b"") + b"two genome records are named \"a\" (records 0 and 2)")
        assert drive(driver, "names", how, "a", "-").startswith(b"names refused: " + (b"ref_names: " if how == "given" else b"") + b"genome record 1 has no name")
    assert drive(driver, "names", "own") == b""
    assert drive(driver, "report", *M.flat(M.compare(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME))) == WORKED_REPORT
    assert drive(driver, "report", *([0] * 215)) == ZERO_REPORT
    rng = random.Random(54)
    for _ in range(5):
        x = random_numbers(rng)
        assert drive(driver, "report", *M.flat(x)) == M.report(x.files, x.types, x.lengths, x.ms)
