"""tests/mapeval_model.py (the rule of `pbsim --eval-bam`) held to values worked out by hand, and the places where the feature
shows without a GPU: the ABI's declarations with their ctypes mirror and the built library's symbols, pbsim_eval_report against
the model's text, the option mirror with the command line's refusals, and the host's HIP-free decisions
(pbsim3_amd/csrc/bam_eval_rule.cpp) under ASan + UBSan."""
import os
import re
import shutil
import subprocess

import pytest

import bam_writer as B
import harness
import mapeval_model as M
import pbsim3_amd as P
from pbsim3_amd import args as A

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def rec(name, flag=0, ref=0, pos=0, span=100, mapq=60, offset=0):
    return dict(name=name, flag=flag, ref_id=ref, pos=pos, span=span, mapq=mapq, offset=offset)


def one(truth_rec, query_recs, permille=100, t_refs=(b"chr",), q_refs=(b"chr",)):
    counts, hist, verdicts = M.evaluate_parsed([(list(t_refs), [truth_rec])], (list(q_refs), query_recs), None, permille)
    return dict(zip(M.COUNT_NAMES, counts)), hist, verdicts


# ---------------------------------------------------------------- literals
def test_overlap_boundary_is_exactly_the_permille():
    """truth [0, 1000); a query [0, 100) has inter 100, union 1000: 100 * 1000 >= 100 * 1000 holds, with one base less
    (99 000 < 100 000) or one permille more (100 000 < 101 000) it does not"""
    t = rec(b"r", span=1000)
    assert one(t, [rec(b"r", span=100)])[2] == bytes([M.CORRECT])
    assert one(t, [rec(b"r", span=99)])[2] == bytes([M.WRONG])
    assert one(t, [rec(b"r", span=100)], permille=101)[2] == bytes([M.WRONG])
    assert one(t, [rec(b"r", pos=900, span=1000)], permille=53)[2] == bytes([M.WRONG])     # inter 100, union 1900: 52.6 permille
    assert one(t, [rec(b"r", pos=900, span=1000)], permille=52)[2] == bytes([M.CORRECT])
    assert one(t, [rec(b"r", span=1000)], permille=1000)[2] == bytes([M.CORRECT])


def test_touching_intervals_do_not_overlap():
    """[0, 100) and [100, 200): inter == 0 is wrong whatever the permille; one base of overlap in a union of 199 is 5 permille"""
    assert not M.overlaps((0, 100), (100, 200), 0) and not M.overlaps((0, 100), (150, 200), 0)
    t = rec(b"r", span=100)
    c, hist, v = one(t, [rec(b"r", pos=100, span=100, mapq=7)], permille=1)
    assert v == bytes([M.WRONG]) and c["wrong"] == 1 and c["scored"] == 1 and hist[7] == [1, 1]
    assert one(t, [rec(b"r", pos=99, span=100)], permille=5)[2] == bytes([M.CORRECT])
    assert one(t, [rec(b"r", pos=99, span=100)], permille=6)[2] == bytes([M.WRONG])


def test_a_span_of_zero_is_one_base():
    assert M.interval(rec(b"r", pos=50, span=0)) == (50, 51)
    assert one(rec(b"r", pos=50, span=0), [rec(b"r", pos=50, span=0)], permille=1000)[2] == bytes([M.CORRECT])
    assert one(rec(b"r", pos=50, span=0), [rec(b"r", pos=51, span=0)], permille=1)[2] == bytes([M.WRONG])


def test_placeholder_cigar_gives_the_span_of_its_n():
    """a CG-tagged record: <q>S<span>N in the CIGAR field, the real operations in the tag, which is not read"""
    import struct
    cg = B.record("cg", 16, 0, 1000, cigar=[(250_000, "S"), (210_000, "N")], seq="", qual=b"",
                  tags=[("CG", "BI", [(3 << 4) | 0] * 70_000)])
    mixed = B.record("mixed", 0, 0, 7, cigar=[(5, "S"), (10, "M"), (3, "I"), (4, "D"), (6, "N"), (2, "="), (1, "X"), (9, "H"), (8, "P")],
                     seq="", qual=b"")
    refs, recs = M.parse(B.stream([cg, mixed], refs=[("chr", 400_000)]))
    assert refs == [b"chr"] and [r["name"] for r in recs] == [b"cg", b"mixed"]
    assert recs[0]["span"] == 210_000 and M.interval(recs[0]) == (1000, 211_000) and recs[0]["flag"] == 16
    assert recs[1]["span"] == 10 + 4 + 6 + 2 + 1 and recs[1]["offset"] == recs[0]["offset"] + 4 + struct.unpack_from("<I", B.record_bytes(cg))[0]


def test_the_first_primary_is_the_one_at_the_smallest_offset():
    t = rec(b"r", span=100)
    good, bad = rec(b"r", span=100, mapq=40), rec(b"r", pos=5000, span=100, mapq=3)
    for order in (0, 1):                    # whatever the order of the list: the offset decides
        a, b = dict(good, offset=100), dict(bad, offset=500)
        c, hist, v = one(t, [a, b][::1 - 2 * order])
        assert v == bytes([M.CORRECT]) and c["duplicate"] == 1 and c["primary"] == 2 and hist[40] == [1, 0] and hist[3] == [0, 0]
        a, b = dict(good, offset=500), dict(bad, offset=100)
        c, hist, v = one(t, [a, b][::1 - 2 * order])
        assert v == bytes([M.WRONG]) and c["duplicate"] == 1 and hist[3] == [1, 1] and hist[40] == [0, 0]
    # secondary and supplementary records of the name are neither first nor duplicate; flag 0x900 counts as secondary
    c, _, v = one(t, [dict(bad, flag=0x100, offset=1), dict(bad, flag=0x800, offset=2), dict(bad, flag=0x900, offset=3), dict(good, offset=9)])
    assert v == bytes([M.CORRECT]) and (c["secondary"], c["supplementary"], c["primary"], c["duplicate"]) == (2, 1, 1, 0)


def test_classes_and_references_by_name():
    truths = [([b"ref"], [rec(b"a", pos=10), rec(b"b", flag=16, pos=10), rec(b"c", pos=10)]),
              ([b"x", b"y"], [rec(b"d", ref=1, pos=10), rec(b"e", ref=0, pos=10), rec(b"f", pos=10)])]
    q_refs = [b"y", b"other", b"chrA", b"x"]
    query = [rec(b"a", ref=2, pos=10, offset=1),                  # chrA is what truth file 0 was told its "ref" is called
             rec(b"b", ref=2, pos=10, offset=2, mapq=20),         # the truth is on the other strand
             rec(b"c", flag=4, ref=-1, pos=-1, offset=3),         # unmapped by flag
             rec(b"d", ref=0, pos=10, offset=4),                  # y by name: refID 0 here, 1 in the truth
             rec(b"e", ref=1, pos=10, offset=5, mapq=20),         # a reference no truth file names
             rec(b"zz", ref=0, pos=10, offset=6)]                 # unknown; f is missing
    counts, hist, v = M.evaluate_parsed(truths, (q_refs, query), [b"chrA", None])
    assert v == bytes([3, 2, 1, 3, 2, 0])
    assert counts == [6, 6, 6, 0, 0, 1, 0, 1, 4, 2, 2, 1]
    assert hist[60] == [2, 0] and hist[20] == [2, 2]
    with pytest.raises(ValueError, match="exactly one"):
        M.evaluate_parsed(truths, (q_refs, query), [None, b"chrB"])
    with pytest.raises(M.DuplicateName) as e:
        M.evaluate_parsed(truths + [([b"ref"], [rec(b"q"), rec(b"b")])], (q_refs, query))
    assert e.value.name == b"b" and e.value.files == (0, 2)


REPORT = (b"# truth_records=10 query_records=12 primary=11 secondary=1 supplementary=0 unknown=1 duplicate=0 unmapped=0 scored=10 "
          b"correct=7 wrong=3 missing=0\n"
          b"Q\t60\t5\t0\t5\t0\t0\t500000\n"
          b"Q\t30\t3\t1\t8\t1\t125000\t800000\n"
          b"Q\t0\t2\t2\t10\t3\t300000\t1000000\n")
REPORT_COUNTS = [10, 12, 11, 1, 0, 1, 0, 0, 10, 7, 3, 0]


def report_hist():
    hist = [[0, 0] for _ in range(256)]
    hist[60], hist[30], hist[0] = [5, 0], [3, 1], [2, 2]
    return hist


def test_report_bytes_of_three_mapqs():
    assert M.report(REPORT_COUNTS, report_hist()) == REPORT
    assert M.report([3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3], [[0, 0]] * 256) == \
        b"# truth_records=3 query_records=0 primary=0 secondary=0 supplementary=0 unknown=0 duplicate=0 unmapped=0 scored=0 correct=0 wrong=0 missing=3\n"


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_calls_and_the_library_has_them():
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        h = f.read()
    assert re.search(r"int pbsim_truth_bam_eval\(pbsim_ctx \*ctx, const pbsim_eval_truth \*truth, int n_truth, const void \*query, int64_t n,\s*"
                     r"const pbsim_eval_opts \*opts, const pbsim_eval_sink \*sink, int64_t counts\[12\], int64_t hist\[512\]\);", h)
    assert re.search(r"int64_t pbsim_eval_report\(const int64_t counts\[12\], const int64_t hist\[512\], char \*buf, int64_t cap\);", h)
    assert re.search(r"typedef struct pbsim_eval_truth \{\s*const void \*bytes;\s*int64_t n;\s*const char \*ref_name;", h)
    assert re.search(r"typedef struct pbsim_eval_opts \{\s*int32_t overlap_permille;\s*int32_t hash_bits;\s*\}", h)
    assert re.search(r"typedef struct pbsim_eval_sink \{\s*void \*user;\s*int \(\*on_verdicts\)\(void \*user, const unsigned char \*bytes, int64_t n\);", h)
    bound = [name for name, _, _ in P.API]
    assert "pbsim_truth_bam_eval" in bound and "pbsim_eval_report" in bound
    assert [n for n, _ in P.EvalTruth._fields_] == ["bytes", "n", "ref_name"]
    assert [n for n, _ in P.EvalOpts._fields_] == ["overlap_permille", "hash_bits"]
    assert [n for n, _ in P.EvalSink._fields_] == ["user", "on_verdicts"]
    assert P.EVAL_COUNTS == M.COUNT_NAMES and callable(getattr(P.Context, "eval_bam"))
    lib = P.load()
    assert hasattr(lib, "pbsim_truth_bam_eval") and hasattr(lib, "pbsim_eval_report")


def test_report_of_the_library_is_the_models_without_a_device():
    import random
    assert P.eval_report(REPORT_COUNTS, report_hist()) == REPORT
    assert P.eval_report(dict(zip(M.COUNT_NAMES, REPORT_COUNTS)), report_hist()) == REPORT
    rng = random.Random(12)
    for _ in range(20):
        hist = [[0, 0] for _ in range(256)]
        for q in rng.sample(range(256), rng.randrange(0, 40)) + [0, 255][:rng.randrange(3)]:
            n = rng.choice([1, 2, 999, 10 ** 6, 10 ** 9])
            hist[q] = [n, rng.randrange(n + 1)]
        scored = sum(n for n, _ in hist)
        counts = [scored + rng.randrange(5)] + [rng.randrange(10 ** 10) for _ in range(11)]
        counts[0] = max(counts[0], 1)
        assert P.eval_report(counts, hist) == M.report(counts, hist)
    lib = P.load()
    assert lib.pbsim_eval_report(None, None, None, 0) == -1


# ---------------------------------------------------------------- the option mirror and the command line
GOOD = ["--eval-bam", "q.bam", "--truth-bam", "a.aln.bam", "--truth-bam", "b.aln.bam"]
REFUSED = [
    (GOOD + ["--truth-ref-names", "chrA"], "1 names for 2 --truth-bam files"),
    (GOOD + ["--truth-ref-names", "chrA,chrB,chrC"], "3 names for 2 --truth-bam files"),
    (GOOD + ["--truth-ref-names", "chrA,"], "an empty name"),
    (GOOD + ["--eval-overlap", "0"], "in (0, 1]"),
    (GOOD + ["--eval-overlap", "1.5"], "in (0, 1]"),
    (GOOD + ["--eval-overlap", "-0.1"], "in (0, 1]"),
    (GOOD + ["--eval-overlap", "half"], "in (0, 1]"),
    (["--eval-bam", "q.bam"], "--eval-bam needs the truth"),
    (["--truth-bam", "a.aln.bam", "--eval-bam"], "needs a value"),
    (GOOD + ["--depth", "3"], "(--depth): --eval-bam takes"),
    (GOOD + ["--devices", "0,1"], "--eval-bam runs on one GPU"),
    (GOOD + ["--processes", "2"], "--eval-bam runs on one GPU"),
    (GOOD + ["--rank", "0", "--world", "2", "--rendezvous", "f"], "--eval-bam runs on one GPU"),
]


def test_option_mirror_accepts_and_rejects():
    got = A.eval_bam(GOOD)
    assert got == dict(query="q.bam", truth=["a.aln.bam", "b.aln.bam"], ref_names=None, overlap=0.1, out=None)
    got = A.eval_bam(["--truth-bam", "a", "--eval-out", "r.txt", "--eval-bam", "q", "--truth-ref-names", "chr1", "--eval-overlap", "1"])
    assert got == dict(query="q", truth=["a"], ref_names=["chr1"], overlap=1.0, out="r.txt")
    for argv, message in REFUSED:
        with pytest.raises(ValueError) as e:
            A.eval_bam(argv)
        assert message in str(e.value), argv


def test_cli_refuses_from_the_command_line_alone(tmp_path):
    """the same refusals by the binary, with the mirror's words, before a device or a file is touched"""
    import pbsim3_amd.build as b
    b.build()
    for argv, message in REFUSED:
        r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and r.stdout == "" and message in r.stderr, (argv, r.stderr[-500:])
    r = subprocess.run([CLI] + GOOD, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "Cannot open file: a.aln.bam" in r.stderr
    assert not os.listdir(tmp_path)


# ---------------------------------------------------------------- the host's decisions under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("asan") / "bam_eval_rule_driver")
    p = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        "-I" + os.path.join(harness.ROOT, "include"), os.path.join(harness.ROOT, "tests", "asan", "bam_eval_rule_driver.cpp"),
                        os.path.join(csrc, "bam_eval_rule.cpp"), os.path.join(csrc, "bam_chain.cpp"), "-o", exe], capture_output=True, text=True)
    if p.returncode != 0 and "sanitize" in p.stderr:
        pytest.skip("no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def drive(exe, *argv):
    p = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, timeout=60)
    assert p.returncode == 0, (argv, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout


def test_rule_code_under_asan(driver, tmp_path):
    f = tmp_path / "h.bam"
    f.write_bytes(B.stream([B.record("r", 0, 0, 5, cigar=[(3, "M")], qual=b"\x10" * 3)], refs=[("chr1", 100), ("a" * 300, 7), ("z", 1)],
                           text=b"@HD\tVN:1.6\n"))
    assert drive(driver, "names", f) == b"names 3 [chr1] [%s] [z]\n" % (b"a" * 300)
    f.write_bytes(B.stream([], refs=[]))
    assert drive(driver, "names", f) == b"names 0\n"
    # numbers by first appearance; "ref" of file 0 is called chrA, the second file repeats a name of the first
    assert drive(driver, "tables", "T", "chrA", "ref", "T", "-", "x", "chrA", "y", "Q", "y", "ref", "chrA", "nobody", "x") == \
        b"tables [0] [1 0 2] | 2 -1 0 -1 1\n"
    assert drive(driver, "tables", "T", "-", "ref", "Q") == b"tables [0] |\n"
    assert drive(driver, "tables", "T", "-", "a", "T", "name", "x", "y", "Q", "a").startswith(b"tables refused: truth file 1 has 2 references")
    assert drive(driver, "tables", "T", "name", "Q", "a").startswith(b"tables refused: truth file 0 has 0 references")
    assert [drive(driver, "file_of", k, 0, 3, 3, 10) for k in (0, 2, 3, 9, 10, 500)] == \
        [b"file_of 0\n", b"file_of 0\n", b"file_of 2\n", b"file_of 2\n", b"file_of 3\n", b"file_of 3\n"]
    assert drive(driver, "report", *REPORT_COUNTS, "60:5:0", "30:3:1", "0:2:2") == REPORT
    big = [2 ** 62] * 12
    assert drive(driver, "report", *big, "255:%d:%d" % (9 * 10 ** 12, 9 * 10 ** 12)) == M.report(big, [[0, 0]] * 255 + [[9 * 10 ** 12, 9 * 10 ** 12]])
