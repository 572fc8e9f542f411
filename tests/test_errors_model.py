"""tests/errors_model.py (the rule of `pbsim --errors-bam`) held to values worked out by hand, and the places where the feature shows
without a GPU: the model's parse against the specification reader, the ABI's declarations with their ctypes mirror and the built
library's symbols, pbsim_errors_report and the fit against the model, the option mirror with the command line's refusals, the
checks in front of any device work, and the HIP-free rule file under the sanitizers."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import bam_spec_reader as R
import bam_writer as B
import errors_model as M
import harness
import pbsim3_amd as P
from pbsim3_amd import args as A

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def rec(name, pos, cigar, seq="", flag=0, ref=0, mapq=60, qual=None, tags=()):
    """qual None: no qualities (0xFF)"""
    ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    return B.record(name, flag, ref, pos, cigar=ops, seq=seq, qual=bytes([255] * len(seq)) if qual is None else qual, tags=tags, mapq=mapq)


# ---------------------------------------------------------------- the worked case of the rule
# The genome's one record, prepared: A C G T T T G C A N N A C G T, classes 1 1 1 3 3 3 1 1 1 1 1 1 1 1 1 (the N run has class 1).
# r1 at 1, 3M1I2M1D2M: C/C G/G T/A | +G | T/T T/T | -G | C/C A/A: 6 matches, 1 sub (in the run of three), NM 3 agrees: 6/9.
# r2 at 8, 1S2M2=1X, no qualities, no NM: A/A N/C | N/= A/= | C/G: 2 matches, 2 ambiguous, 1 sub: 2/5.
# r3 at 8, 1M2D1M, mapq 7: A/A | -N -N | A/A: 2 matches, NM 2 agrees: 2/4; qualities 30 and 40.
# u1 unaligned, s1 secondary, z1 on a reference the genome lacks; f1 runs past l_ref, f2 has one base too many, n1 has none.
# The fit: class 1 has 14 columns and 3 deletions, class 3 has 3 and 0: W 17, Sx 6, Sxx 12, Sy 3, Sxy 0: Num -18, Den 36:
# 1000 + floor(-162000 / 36) = -3500.  Q 10: 7 columns, 1 sub: -10 log10(1 / 7) = 8.4509.
GENOME = [("c1", b"ACGTTTGCA\nNNacgt\n")]
WORKED_REFS = [("c1", 15), ("zz", 50)]
WORKED = [rec("r1", 1, "3M1I2M1D2M", "CGAGTTCA", qual=bytes([10] * 8), tags=[("NM", "C", 3)]),
          rec("r2", 8, "1S2M2=1X", "TAC==G"),
          rec("u1", -1, "", "ACG", flag=4, ref=-1),
          rec("s1", 1, "3M", "CGT", flag=0x100),
          rec("f1", 13, "5M", "GTACG", tags=[("NM", "C", 0)]),
          rec("n1", 0, "3M", ""),
          rec("f2", 0, "3M", "ACGT"),
          rec("z1", 0, "3M", "ACG", ref=1),
          rec("r3", 8, "1M2D1M", "AA", qual=bytes([30, 40]), tags=[("NM", "C", 2)], mapq=7)]
WORKED_TEXT = (b"r1\tS\t8\t9\t6\t1\t0\t1\t1\t0\t3\t3\t666666\n"
               b"r2\tS\t6\t5\t2\t1\t2\t0\t0\t1\t*\t1\t400000\n"
               b"f1\tF\t5\t5\t*\t*\t*\t0\t0\t0\t0\t*\t*\n"
               b"n1\tN\t0\t3\t*\t*\t*\t0\t0\t0\t*\t*\t*\n"
               b"f2\tF\t4\t3\t*\t*\t*\t0\t0\t0\t*\t*\t*\n"
               b"r3\tS\t2\t4\t2\t0\t0\t0\t2\t0\t2\t2\t500000\n")
WORKED_REPORT = (b"# records=9 skipped_flag=1 unaligned=1 skipped_mapq=0 skipped_ref=1 aligned=6 no_seq=1 misfit=2 scored=3 no_nm=1 nm_unchecked=0 "
                 b"nm_agree=2 nm_differ=0 with_qual=2\n"
                 b"E\t18\t10\t2\t2\t1\t3\t1\t2\t1\t0\t111111\t55555\t166666\t522222\n"
                 b"M\tA\t5\t0\t0\t0\t0\nM\tC\t0\t2\t1\t0\t0\nM\tG\t0\t0\t1\t0\t0\nM\tT\t1\t0\t0\t2\t0\nM\tN\t0\t1\t0\t0\t1\n"
                 b"HP\t1\t14\t1\t3\t214285\nHP\t3\t3\t1\t0\t0\n"
                 b"B\t1\t-3500\t1000\n"
                 b"IL\t1\t1\nDL\t1\t1\nDL\t2\t1\n"
                 b"IB\t0\t0\t1\t0\t0\nDB\t0\t0\t1\t0\t2\n"
                 b"QC\t10\t7\t1\t1\t8450\nQC\t30\t1\t0\t0\t*\nQC\t40\t1\t0\t0\t*\n"
                 b"HI\t400\t1\nHI\t500\t1\nHI\t666\t1\n")


def sparse(values):
    return {k: v for k, v in enumerate(values) if v}


def test_the_worked_case():
    r = M.errors(B.stream(WORKED, WORKED_REFS), GENOME)
    assert r.counts == [9, 1, 1, 0, 1, 6, 1, 2, 3, 1, 0, 2, 0, 2]
    assert r.totals == [18, 10, 2, 2, 1, 3, 1, 2, 1, 0, 666666 + 400000 + 500000]
    assert r.pair == [5, 0, 0, 0, 0, 0, 2, 1, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 2, 0, 0, 1, 0, 0, 1]
    assert sparse(r.hp_cols) == {1: 14, 3: 3} and sparse(r.hp_sub) == {1: 1, 3: 1} and sparse(r.hp_del) == {1: 3}
    assert sparse(r.ins_len) == {1: 1} and sparse(r.del_len) == {1: 1, 2: 1}
    assert r.ins_base == [0, 0, 1, 0, 0] and r.del_base == [0, 0, 1, 0, 2]
    assert sparse(r.qcal) == {30: 7, 31: 1, 32: 1, 90: 1, 120: 1}
    assert sparse(r.hist_identity) == {400: 1, 500: 1, 666: 1}
    assert r.fit == [1, -3500, 1000]
    assert r.text == WORKED_TEXT and r.report == WORKED_REPORT
    # the secondary counts without the default filter; min_mapq at the boundary keeps or skips r3
    assert M.errors(B.stream(WORKED, WORKED_REFS), GENOME, exclude_flags=0).counts[:9] == [9, 0, 1, 0, 1, 7, 1, 2, 4]
    assert M.errors(B.stream(WORKED, WORKED_REFS), GENOME, min_mapq=7).counts == r.counts
    assert M.errors(B.stream(WORKED, WORKED_REFS), GENOME, min_mapq=8).counts[:9] == [9, 1, 1, 1, 1, 5, 1, 2, 2]
    # two files give what one gives; a file's only reference goes by the name given for it
    two = M.errors([B.stream(WORKED[:2], WORKED_REFS), B.stream(WORKED[2:], WORKED_REFS)], GENOME)
    assert two == r
    named = M.errors(B.stream([w for w in WORKED if w["name"] != "z1"], [("ref", 15)]), GENOME, ref_names=["c1"])
    assert named.counts == [8, 1, 1, 0, 0, 6, 1, 2, 3, 1, 0, 2, 0, 2] and named.text == WORKED_TEXT
    assert M.errors(B.stream(WORKED, [("ref", 15), ("zz", 50)]), GENOME).counts[4:6] == [7, 0]
    with pytest.raises(ValueError, match="exactly one"):
        M.errors(B.stream(WORKED, WORKED_REFS), GENOME, ref_names=["c1"])
    with pytest.raises(ValueError, match="l_ref 16, 15 bases"):
        M.errors(B.stream(WORKED, [("c1", 16), ("zz", 50)]), GENOME)
    with pytest.raises(ValueError, match="two records named"):
        M.errors(B.stream(WORKED, WORKED_REFS), GENOME + [("c1", b"AC")])
    # preparation is per record: the second record's A run does not join the first one's
    g2 = [("a", b"CAA"), ("b", b"AAC")]
    r2 = M.errors(B.stream([rec("x", 1, "2M", "AA"), rec("y", 0, "2M", "AA", ref=1)], [("a", 3), ("b", 3)]), g2)
    assert sparse(r2.hp_cols) == {2: 4}


def test_the_models_parse_agrees_with_the_specification_reader():
    rng = random.Random(2)
    recs = [rec("q%d" % k, rng.randrange(50), "%dM2I%dS" % (k + 1, k % 3 + 1), "".join(rng.choice("ACGTN=RY") for _ in range(k + 3 + k % 3 + 1)),
                qual=bytes(rng.randrange(60) for _ in range(k + 3 + k % 3 + 1)), tags=[("NM", "C", 2), ("XZ", "Z", "t%d" % k)], mapq=k)
            for k in range(20)]
    raw = B.bam(recs, WORKED_REFS)
    refs, mine = M.parse(M.inflate(raw))
    _, their_refs, theirs = R.read_bam(raw)
    assert refs == [(b"c1", 15), (b"zz", 50)] and len(their_refs) == 2
    assert len(mine) == len(theirs) == 20
    for a, b, w in zip(mine, theirs, recs):
        assert (a["name"].decode(), a["flag"], a["ref_id"], a["pos"], a["mapq"], a["l_seq"], a["qual"]) == \
               (b["read_name"], b["flag"], b["refID"], b["pos"], b["mapq"], b["l_seq"], b["qual"])
        assert [(n, "MIDNSHP=X"[op]) for n, op in a["cigar"]] == b["cigar"]
        codes = [(a["seq"][k // 2] >> (0 if k % 2 else 4)) & 15 for k in range(a["l_seq"])]
        assert "".join("=ACMGRSVTWYHKDBN"[c] for c in codes) == w["seq"] == b["seq"]


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_calls_and_the_library_has_them():
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        h = f.read()
    assert re.search(r"int pbsim_bam_errors\(pbsim_ctx \*ctx, const pbsim_errors_ref \*refs, int n_refs, const pbsim_errors_file \*files, int n_files,\s*"
                     r"const pbsim_errors_opts \*opts, const pbsim_errors_sink \*sink, pbsim_errors_result \*result\);", h)
    assert re.search(r"int64_t pbsim_errors_report\(const pbsim_errors_result \*result, char \*buf, int64_t cap\);", h)
    assert re.search(r"typedef struct pbsim_errors_opts \{[^;]*int32_t exclude_flags, min_mapq;\s*int64_t piece_bytes;", h)
    body = re.search(r"typedef struct pbsim_errors_result \{(.*?)\} pbsim_errors_result;", h, re.S).group(1)
    declared = []
    for typ, names in re.findall(r"(int64_t) ([^;]+);", body):
        for item in names.split(","):
            name, dims = re.match(r"\s*(\w+)((?:\[\d+\])*)", item).groups()
            size = 1
            for d in re.findall(r"\[(\d+)\]", dims):
                size *= int(d)
            declared.append((name, size))
    mirrored = [(n, C.sizeof(t) // 8) for n, t in P.ErrorsResult._fields_]
    assert declared == mirrored and C.sizeof(P.ErrorsResult) == 8 * sum(n for _, n in declared)
    assert mirrored == [("counts", 14), ("totals", 11)] + M.ARRAYS + [(n, 1) for n in M.FIT_NAMES]
    bound = [name for name, _, _ in P.API]
    assert "pbsim_bam_errors" in bound and "pbsim_errors_report" in bound
    assert [n for n, _ in P.ErrorsOpts._fields_] == ["exclude_flags", "min_mapq", "piece_bytes"] and C.sizeof(P.ErrorsOpts) == 16
    assert [n for n, _ in P.ErrorsRef._fields_] == ["name", "lines", "bytes"] and [n for n, _ in P.ErrorsFile._fields_] == ["bam", "n", "ref_name"]
    assert [n for n, _ in P.ErrorsSink._fields_] == ["user", "on_text"]
    assert (P.ERRORS_COUNTS, P.ERRORS_TOTALS, P.ERRORS_ARRAYS, P.ERRORS_FIT) == (M.COUNT_NAMES, M.TOTAL_NAMES, M.ARRAYS, M.FIT_NAMES)
    assert callable(getattr(P.Context, "bam_errors")) and callable(P.errors_report)
    lib = P.load()
    assert hasattr(lib, "pbsim_bam_errors") and hasattr(lib, "pbsim_errors_report")
    with open(os.path.join(harness.ROOT, "pbsim3_amd", "csrc", "bam_errors.h")) as f:
        internal = f.read()
    assert int(re.search(r"constexpr int kErrSegOps = (\d+);", internal).group(1)) % 64 == 0
    assert int(re.search(r"constexpr int kErrSegCols = (\d+);", internal).group(1)) >= 64


def as_dict(counts, totals, arrays):
    out = dict(counts=counts, totals=totals)
    out.update(arrays)
    return out


def random_result(rng, hp=None):
    counts = [rng.randrange(2 ** 31) for _ in range(14)]
    totals = [rng.choice([0, 1, rng.randrange(2 ** 40), rng.randrange(2 ** 60)]) for _ in range(11)]
    totals[0] = sum(totals[1:6]) + rng.choice([0, 1, rng.randrange(2 ** 60)])          # cols = match + sub + ambiguous + ins + del, at least
    arrays = {name: [rng.choice([0, 0, 0, 1, 10 ** 12, rng.randrange(2 ** 50)]) for _ in range(n)] for name, n in M.ARRAYS}
    arrays["hp_cols"] = [s + d + rng.choice([0, 1, rng.randrange(2 ** 50)]) for s, d in zip(arrays["hp_sub"], arrays["hp_del"])]
    if hp is not None:
        arrays["hp_cols"], arrays["hp_del"] = hp
        arrays["hp_sub"] = [0] * 12
    return counts, totals, arrays


def library_fit(hp_cols, hp_del):
    """the fit as the built library makes it: the B line of its report"""
    arrays = {name: [0] * n for name, n in M.ARRAYS}
    arrays["hp_cols"], arrays["hp_del"] = list(hp_cols), list(hp_del)
    text = P.errors_report(as_dict([0] * 14, [0] * 11, arrays))
    return [int(v) for v in re.search(rb"^B\t(-?\d+)\t(-?\d+)\t(-?\d+)$", text, re.M).groups()]


# hp_cols, hp_del over the classes 0 .. 11, and what the fit must say where it is worked out by hand
FIT_CASES = [
    # the deletion rate rises from 1 % to 10 %, linearly in the class: slope / intercept = 1, the bias 10
    ([0] + [1000] * 10 + [0], [0] + [10 * (1 + x) for x in range(10)] + [0], [1, 10000, 10000]),
    # a flat rate: Num = 0, the bias 1
    ([0] + [500] * 10 + [7], [9] + [5] * 10 + [3], [1, 1000, 1000]),
    # a falling rate: Num < 0, and the quotient is floored, not truncated: -162000 / 36 = -4500 exactly, -162001 / 36 would be -4501
    ([0, 14, 0, 3] + [0] * 8, [0, 3] + [0] * 10, [1, -3500, 1000]),
    ([0, 7, 5, 0, 3] + [0] * 7, [0, 2, 1, 0, 0] + [0] * 7, None),
    # no deletions at all: Sy == 0
    ([0] + [100] * 10 + [0], [0] * 12, [0, 0, 0]),
    # a single class that is not empty (class 1: Sxx = 0, Den = 0; class 4: Den = Sxx Sy - Sx Sxy = 9 c d - 3 c 3 d = 0)
    ([0, 100] + [0] * 10, [0, 9] + [0] * 10, [0, 0, 0]),
    ([0, 0, 0, 0, 100] + [0] * 7, [0, 0, 0, 0, 9] + [0] * 7, [0, 0, 0]),
    # classes 0 and 11 take no part
    ([10 ** 9] + [0] * 10 + [10 ** 9], [10 ** 6] + [0] * 10 + [10 ** 6], [0, 0, 0]),
    # deletions only in the highest class: Den = Sxx Sy - Sx Sxy < 0
    ([0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1000, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 50, 0], None),
    # counts near 2^50: the products pass 2^64 and 2^100
    ([0] + [2 ** 50 - k for k in range(10)] + [0], [0] + [2 ** 40 + (2 ** 37) * k + k for k in range(10)] + [0], None),
    ([0] + [2 ** 50 + 3 * k for k in range(10)] + [0], [0] + [2 ** 49 - (2 ** 45) * k - 1 for k in range(10)] + [0], None),
]


def test_the_fit_by_hand_and_of_the_library():
    for hp_cols, hp_del, want in FIT_CASES:
        got = M.fit(hp_cols, hp_del)
        if want is not None:
            assert got == want, (hp_cols, hp_del)
        assert library_fit(hp_cols, hp_del) == got, (hp_cols, hp_del)
    assert M.fit(*FIT_CASES[3][:2])[1] < 1000 and M.fit(*FIT_CASES[8][:2]) == [0, 0, 0]
    big, falling = M.fit(*FIT_CASES[9][:2]), M.fit(*FIT_CASES[10][:2])
    assert big[0] == 1 and big[1] > 1000 and falling[0] == 1 and falling[1] < 1000
    # the floor: a remainder below zero rounds down
    assert M.fit([0, 36, 0, 0] + [0] * 8, [0, 1, 0, 0] + [0] * 8) == [0, 0, 0]
    hp_cols, hp_del = [0, 13, 0, 4] + [0] * 8, [0, 3, 0, 0] + [0] * 8          # Num = -24, Den = 48 ... + a remainder
    hp_cols[2], hp_del[2] = 1, 0                                            # W 18, Sx 9, Sxx 17, Sy 3, Sxy 0: Num -27, Den 51
    assert M.fit(hp_cols, hp_del) == [1, 1000 + (-243000 // 51), 1000] and -243000 // 51 == -4765 and int(-243000 / 51) == -4764
    assert library_fit(hp_cols, hp_del) == [1, -3765, 1000]
    rng = random.Random(5)
    for _ in range(200):
        hp_cols = [rng.choice([0, 1, rng.randrange(1000), rng.randrange(2 ** 50)]) for _ in range(12)]
        hp_del = [rng.choice([0, 0, 1, rng.randrange(1000), rng.randrange(2 ** 50)]) for _ in range(12)]
        assert library_fit(hp_cols, hp_del) == M.fit(hp_cols, hp_del), (hp_cols, hp_del)


def test_report_of_the_library_is_the_models_without_a_device():
    r = M.errors(B.stream(WORKED, WORKED_REFS), GENOME)
    arrays = {name: getattr(r, name) for name, _ in M.ARRAYS}
    assert P.errors_report(as_dict(r.counts, r.totals, arrays)) == WORKED_REPORT
    assert P.errors_report(as_dict(dict(zip(M.COUNT_NAMES, r.counts)), dict(zip(M.TOTAL_NAMES, r.totals)), arrays)) == WORKED_REPORT
    rng = random.Random(31)
    for k in range(20):
        hp = FIT_CASES[k % len(FIT_CASES)][:2] if k % 2 else None
        counts, totals, arrays = random_result(rng, hp)
        assert P.errors_report(as_dict(counts, totals, arrays)) == M.report(counts, totals, *[arrays[name] for name, _ in M.ARRAYS])
    zero = {name: [0] * n for name, n in M.ARRAYS}
    text = P.errors_report(as_dict([0] * 14, [0] * 11, zero))
    assert text == M.report([0] * 14, [0] * 11, *[zero[name] for name, _ in M.ARRAYS])
    assert text.endswith(b"E" + b"\t0" * 14 + b"\n" + b"".join(b"M\t%s" % c + b"\t0" * 5 + b"\n" for c in (b"A", b"C", b"G", b"T", b"N")) +
                         b"B\t0\t0\t0\nIB" + b"\t0" * 5 + b"\nDB" + b"\t0" * 5 + b"\n")
    assert P.load().pbsim_errors_report(None, None, 0) == -1
    with pytest.raises(ValueError, match="pair has 24 values"):
        P.errors_report(as_dict([0] * 14, [0] * 11, dict(zero, pair=[0] * 24)))


# ---------------------------------------------------------------- the option mirror and the command line
GOOD = ["--errors-bam", "in.bam", "--errors-genome", "g.fa"]
REFUSED = [
    (GOOD + ["--depth", "3"], "(--depth): --errors-bam takes"),
    (GOOD + ["--stats-out", "x"], "(--stats-out): --errors-bam takes"),
    (["--errors-out", "o", "--errors-bam"], "needs a value"),
    (["--errors-bam", "in.bam"], "--errors-bam needs --errors-genome FASTA"),
    (GOOD + ["--errors-min-mapq", "256"], "(errors-min-mapq: 256): a whole number, 0 .. 255"),
    (GOOD + ["--errors-min-mapq", "-1"], "(errors-min-mapq: -1): a whole number, 0 .. 255"),
    (GOOD + ["--errors-exclude-flags", "0xZZ"], "(errors-exclude-flags: 0xZZ): decimal or 0x hexadecimal"),
    (GOOD + ["--errors-exclude-flags", "65536"], "(errors-exclude-flags: 65536): decimal or 0x hexadecimal"),
    (GOOD + ["--errors-ref-names", "a,b"], "(errors-ref-names): 2 names for 1 --errors-bam files"),
    (GOOD + ["--errors-bam", "b.bam", "--errors-ref-names", "a,"], "(errors-ref-names): an empty name"),
    (GOOD + ["--devices", "0,1"], "--errors-bam runs on one GPU"),
    (GOOD + ["--processes", "2"], "--errors-bam runs on one GPU"),
]


def test_option_mirror_accepts_and_rejects():
    assert A.errors_bam(GOOD) == dict(bams=["in.bam"], genome="g.fa", ref_names=None, out=None, min_mapq=0, exclude_flags=0x900)
    got = A.errors_bam(["--errors-out", "o", "--errors-bam", "a", "--errors-min-mapq", "255", "--errors-bam", "b", "--errors-exclude-flags", "0xF04",
                        "--errors-genome", "g", "--errors-ref-names", "x,y", "--device", "1"])
    assert got == dict(bams=["a", "b"], genome="g", ref_names=["x", "y"], out="o", min_mapq=255, exclude_flags=0xF04)
    assert A.errors_bam(GOOD + ["--errors-exclude-flags", "2304"])["exclude_flags"] == 0x900
    for argv, message in REFUSED + [(["--errors-genome", "g"], "--errors-bam FILE: name the BAM file")]:
        with pytest.raises(ValueError) as e:
            A.errors_bam(argv)
        assert message in str(e.value), argv


def test_cli_refuses_from_the_command_line_alone(tmp_path):
    """the same refusals by the binary, with the mirror's words, before a device or a file is touched"""
    import pbsim3_amd.build as b
    b.build()
    for argv, message in REFUSED:
        r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and r.stdout == "" and message in r.stderr, (argv, r.stderr[-500:])
    r = subprocess.run([CLI] + GOOD + ["--errors-out", "o.tsv"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "Cannot open file: in.bam" in r.stderr
    (tmp_path / "in.bam").write_bytes(B.bam(WORKED, WORKED_REFS))
    r = subprocess.run([CLI] + GOOD + ["--errors-out", "o.tsv"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "--errors-genome g.fa: Cannot open file: g.fa" in r.stderr
    assert os.listdir(tmp_path) == ["in.bam"]
    r = subprocess.run([CLI], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert "--errors-bam FILE [--errors-bam FILE ...] --errors-genome FASTA" in r.stderr + r.stdout


# ---------------------------------------------------------------- the checks in front of any device work
def test_bad_arguments_fail_before_device_work():
    data = B.bam(WORKED, WORKED_REFS)
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), -1) as c:
        with pytest.raises(P.PbsimError, match="pbsim_bam_errors: min_mapq must be 0 .. 255"):
            c.bam_errors(data, GENOME, min_mapq=256)
        with pytest.raises(P.PbsimError, match="pbsim_bam_errors: exclude_flags must be 0 .. 65535"):
            c.bam_errors(data, GENOME, exclude_flags=65536)
        with pytest.raises(P.PbsimError, match="pbsim_bam_errors: piece_bytes must not be negative"):
            c.bam_errors(data, GENOME, piece_bytes=-1)
        with pytest.raises(P.PbsimError, match="pbsim_bam_errors: bad argument"):
            c.bam_errors([], GENOME)
        with pytest.raises(P.PbsimError, match="pbsim_bam_errors: bad argument"):
            c.bam_errors(data, [])
        with pytest.raises(P.PbsimError, match=r"pbsim_bam_errors: the genome holds two records named \"c1\" \(records 0 and 2\)"):
            c.bam_errors(data, GENOME + [("other", b"ACGT"), ("c1", b"AC")])
        with pytest.raises(ValueError, match="one entry per file"):
            c.bam_errors(data, GENOME, ref_names=["a", "b"])
        # good arguments reach the device check: a tables-only context refuses as pbsim_inflate_buffer does, and stays usable
        for kw in (dict(), dict(text=True), dict(min_mapq=255, exclude_flags=0, ref_names=["c1", None])):
            with pytest.raises(P.PbsimError, match="no HIP device"):
                c.bam_errors([data, data], GENOME, **kw)


# ---------------------------------------------------------------- the host's decisions under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("asan") / "bam_errors_rule_driver")
    p = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(harness.ROOT, "tests", "asan", "bam_errors_rule_driver.cpp"), os.path.join(csrc, "bam_errors_rule.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if p.returncode != 0 and "sanitize" in p.stderr:
        pytest.skip("no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def drive(exe, *argv):
    p = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, timeout=60)
    assert p.returncode == 0, (argv, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout


def report_args(counts, totals, arrays):
    return list(counts) + list(totals) + [x for name, _ in M.ARRAYS for k, v in enumerate(arrays[name]) if v for x in (name, k, v)]


def test_rule_code_under_asan(driver):
    assert drive(driver, "opts", "-") == b"opts 2304 0 8388608\n"
    assert drive(driver, "opts", 0, 255, 7) == b"opts 0 255 7\n"
    for bad, word in (((65536, 0, 0), b"exclude_flags"), ((-1, 0, 0), b"exclude_flags"), ((4, 256, 0), b"min_mapq"), ((4, -1, 0), b"min_mapq"),
                      ((4, 0, -1), b"piece_bytes")):
        assert drive(driver, "opts", *bad).startswith(b"opts refused: " + word)
    assert drive(driver, "genome", "a", "b", "ab") == b"genome ok\n"
    assert drive(driver, "genome", "a", "b", "a").startswith(b"genome refused: the genome holds two records named \"a\" (records 0 and 2)")
    assert drive(driver, "refmap", "-", 3, "x", "y", "z", 4, "z", "q", "x", "x") == b"refmap 2 -1 0 0\n"
    assert drive(driver, "refmap", "y", 3, "x", "y", "z", 1, "ref") == b"refmap 1\n"
    assert drive(driver, "refmap", "nope", 3, "x", "y", "z", 1, "x") == b"refmap -1\n"
    assert drive(driver, "refmap", "y", 3, "x", "y", "z", 2, "x", "y").startswith(b"refmap refused: file 3 has 2 references")
    assert drive(driver, "refmap", "y", 1, "y", 0).startswith(b"refmap refused: file 3 has 0 references")
    for hp_cols, hp_del, _ in FIT_CASES:
        assert drive(driver, "fit", *(list(hp_cols) + list(hp_del))) == b"fit %d %d %d\n" % tuple(M.fit(hp_cols, hp_del)), (hp_cols, hp_del)
    r = M.errors(B.stream(WORKED, WORKED_REFS), GENOME)
    assert drive(driver, "report", *report_args(r.counts, r.totals, {name: getattr(r, name) for name, _ in M.ARRAYS})) == WORKED_REPORT
    rng = random.Random(32)
    for k in range(5):
        counts, totals, arrays = random_result(rng, FIT_CASES[9 + k % 2][:2] if k else None)
        assert drive(driver, "report", *report_args(counts, totals, arrays)) == M.report(counts, totals, *[arrays[name] for name, _ in M.ARRAYS])
