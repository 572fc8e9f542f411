"""tests/consensus_model.py (the rule of `pbsim --consensus-bam`) held to a case worked out by hand and to the pileup's model on the
same streams, and the places where the feature shows without a GPU: the ABI's declarations with their ctypes mirror and the built
library's symbols, pbsim_consensus_report against the model, the option mirror with the command line's refusals, the checks in
front of any device work, and the HIP-free rule file under the sanitizers."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import bam_writer as B
import consensus_model as K
import harness
import pbsim3_amd as P
import pileup_model as M
from pbsim3_amd import args as A
from test_pileup_model import GENOME as PILE_GENOME, WORKED as PILE_WORKED, WORKED_REFS as PILE_REFS, rec, small_case

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")

# ---------------------------------------------------------------- the worked case of the rule
# c1, prepared: A C G T A C G T A C; c2: G G R T T (R has class 4: a ref_n site).  No read has qualities.
# c1 0        r1 .. r4 say A: depth 4.  r1 and r2 insert T behind it: 2 n == 4 == depth: no ins_site, nothing emitted.
# c1 1        r1 r2 r4 say T, r3 C: a sub_site, T.
# c1 2        G.
# c1 3        r1 and r2 delete it, r3 says T: a del_site, nothing emitted.
# c1 4, 5     A C; behind 5 r1 inserts GAT, r2 GA, r3 TA: offset 0 has G 2 T 1, n = 3: G; offset 1 A 3: A; offset 2 has T 1,
#             2 n = 2 is not above depth 3: the third base, in a minority, is not emitted.
# c1 6, 7     G T; behind 7 r1 inserts C and r2 A: n = 2, 4 > 3; A 1 C 1, a tie the first wins: A.
# c1 8        A; behind it r1 inserts `=` (code 0) and r2 N (code 15): both other, the four cells 0: N.
# c1 9        no read: low: N, or with fill "ref" the genome's C.
# c2 0, 1     r5 1I2M: the insertion in front is unanchored and adds nowhere; G G.
# c2 2 .. 4   r6 A T T: the genome's R is a ref_n site whatever lies there: N, or with fill "ref" R; T T.
# discordant 5 of called 13: 384615 ppm, -10 log10(5 / 13) = 4.1497.
GENOME = [("c1", b"ACGTAC\nGTAC\n"), ("c2", b"GGRTT\n")]
REFS = [("c1", 10), ("c2", 5)]
WORKED = [rec("r1", 0, "1M1I2M1D2M3I2M1I1M1I", "ATTGACGATGTCA="),
          rec("r2", 0, "1M1I2M1D2M2I2M1I1M1I", "ATTGACGAGTAAN"),
          rec("r3", 0, "6M2I3M", "ACGTACTAGTA"),
          rec("r4", 0, "2M", "AT"),
          rec("r5", 0, "1I2M", "AGG", ref=1),
          rec("r6", 2, "3M", "ATT", ref=1)]
WORKED_FASTA = b">c1\nATGACGAGTAANN\n>c2\nGGNTT\n"
WORKED_FASTA_REF = b">c1\nATGACGAGTAANC\n>c2\nGGRTT\n"
WORKED_FASTA_5 = b">c1\nATGAC\nGAGTA\nANN\n>c2\nGGNTT\n"
WORKED_FASTA_MAX_1 = b">c1\nATGACGGTAANN\n>c2\nGGNTT\n"
WORKED_REPORT = (b"# records=6 skipped_flag=0 unaligned=0 skipped_mapq=0 skipped_ref=0 aligned=6 no_seq=0 misfit=0 scored=6\n"
                 b"S\t15\t1\t1\t13\t11\t1\t1\t3\t5\t384615\t4149\n"
                 b"K\t18\t11\t1\t4\t2\t1\t3\t2\t0\n"
                 b"IL\t1\t2\nIL\t2\t1\n")
# the options moved off their defaults, one at a time (dicts of the model's keyword arguments)
WORKED_OPTIONS = [dict(fill="ref"), dict(line_width=5), dict(line_width=0), dict(line_width=1), dict(line_width=13), dict(max_ins=1), dict(max_ins=2),
                  dict(min_depth=4), dict(min_depth=0), dict(min_mapq=61), dict(exclude_flags=0), dict(min_baseq=1),
                  dict(fill="ref", line_width=7, max_ins=1, min_depth=2, min_mapq=60, exclude_flags=0x10)]


def worked(**kw):
    return K.consensus(B.stream(WORKED, REFS), GENOME, **kw)


def test_the_worked_case():
    r = worked()
    assert r.text == WORKED_FASTA and r.report == WORKED_REPORT and r.text_bytes == len(WORKED_FASTA) and r.lengths == [(10, 13), (5, 5)]
    assert r.counts == [6, 0, 0, 0, 0, 6, 0, 0, 6] and r.sites == [15, 1, 1, 13, 11, 1, 1, 3, 5] and (r.ins_unanchored, r.max_depth) == (1, 4)
    assert r.bases == [18, 11, 1, 4, 2, 1] and (r.ins_sites, r.ins_longest, r.ins_capped) == (3, 2, 0)
    assert {k: v for k, v in enumerate(r.ins_len) if v} == {1: 2, 2: 1}
    ref = worked(fill="ref")
    assert ref.text == WORKED_FASTA_REF and ref[:10] == r[:10] and ref.report == r.report
    assert worked(line_width=5).text == WORKED_FASTA_5 and worked(line_width=0).text == WORKED_FASTA and worked(line_width=13).text == WORKED_FASTA
    assert worked(line_width=1).text == b">c1\n" + b"".join(bytes([c]) + b"\n" for c in b"ATGACGAGTAANN") + b">c2\nG\nG\nN\nT\nT\n"
    one = worked(max_ins=1)
    assert one.text == WORKED_FASTA_MAX_1 and one.bases == [17, 11, 1, 3, 2, 1] and (one.ins_sites, one.ins_longest, one.ins_capped) == (3, 1, 3)
    assert worked(max_ins=2).text == WORKED_FASTA and worked(max_ins=2).ins_capped == 1
    # at min_depth 4 only the first two sites of c1 are called; with the reads' own flags excluded nothing changes
    assert worked(min_depth=4).text == b">c1\nAT" + b"N" * 8 + b"\n>c2\nNNNNN\n" and worked(exclude_flags=0).text == WORKED_FASTA
    # at min_depth 0 the bare site is called as the genome's base
    assert worked(min_depth=0).text == b">c1\nATGACGAGTAANC\n>c2\nGGNTT\n" and worked(min_depth=0).bases == [18, 12, 1, 4, 1, 1]
    assert worked(min_mapq=61).text == b">c1\n" + b"N" * 10 + b"\n>c2\nNNNNN\n" and worked(min_mapq=61).counts[3] == 6
    # two files give what one gives, in either order
    two = K.consensus([B.stream(WORKED[3:], REFS), B.stream(WORKED[:3], REFS)], GENOME)
    assert two == r
    # a record of no bases, and one whose consensus has none: the header line alone
    gen = GENOME + [("none", b""), ("gone", b"A\n")]
    gone = K.consensus(B.stream(WORKED + [rec("d", 0, "2S1D", "AC", ref=2)], REFS + [("gone", 1)]), gen)
    assert gone.text == WORKED_FASTA + b">none\n>gone\n" and gone.lengths[2:] == [(0, 0), (1, 0)] and gone.bases[5] == 2


def test_counts_and_sites_are_the_pileups_on_the_same_streams():
    for streams, genome in (([B.stream(WORKED, REFS)], GENOME), ([B.stream(PILE_WORKED, PILE_REFS)], PILE_GENOME)):
        for kw in (dict(), dict(min_depth=2), dict(min_baseq=20, min_mapq=8), dict(exclude_flags=0)):
            k, m = K.consensus(streams, genome, **kw), M.pileup(streams, genome, **kw)
            assert (k.counts, k.sites, k.ins_unanchored, k.max_depth) == (m.counts, m.sites, m.ins_unanchored, m.max_depth)
    r = K.consensus(B.stream(PILE_WORKED, PILE_REFS), PILE_GENOME)
    assert r.text == b">g1\nACGTCCGTTTCNACGT\n>g2\nGGCNNTAC\n" and r.bases == [24, 18, 1, 2, 3, 1]
    genome, refs, recs, _ = small_case(3)
    k, m = K.consensus(B.stream(recs, refs), genome, line_width=50), M.pileup(B.stream(recs, refs), genome)
    assert (k.counts, k.sites, k.ins_unanchored, k.max_depth) == (m.counts, m.sites, m.ins_unanchored, m.max_depth) and k.ins_sites == m.sites[7] > 0
    assert all(len(line) <= 50 for line in k.text.split(b"\n")) and k.text.count(b">") == 2 and k.text_bytes == len(k.text)


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_calls_and_the_library_has_them():
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        h = f.read()
    assert re.search(r"int pbsim_bam_consensus\(pbsim_ctx \*ctx, const pbsim_errors_ref \*refs, int n_refs, const pbsim_errors_file \*files, int n_files,\s*"
                     r"const pbsim_consensus_opts \*opts, const pbsim_consensus_sink \*sink, pbsim_consensus_result \*result\);", h)
    assert re.search(r"int64_t pbsim_consensus_report\(const pbsim_consensus_result \*result, char \*buf, int64_t cap\);", h)
    assert re.search(r"typedef struct pbsim_consensus_opts \{[^;]*int32_t exclude_flags, min_mapq, min_baseq;\s*int32_t fill;[^;]*\s*int64_t min_depth;\s*"
                     r"int32_t max_ins;[^;]*\s*int32_t line_width;[^;]*\s*int64_t piece_bytes;", h)
    body = re.search(r"typedef struct pbsim_consensus_result \{(.*?)\} pbsim_consensus_result;", h, re.S).group(1)
    declared = []
    for names in re.findall(r"int64_t ([^;]+);", body):
        for item in names.split(","):
            name, dims = re.match(r"\s*(\w+)((?:\[\d+\])*)", item).groups()
            declared.append((name, int(dims[1:-1]) if dims else 1))
    mirrored = [(n, C.sizeof(t) // 8) for n, t in P.ConsensusResult._fields_]
    assert declared == mirrored and C.sizeof(P.ConsensusResult) == 8 * sum(n for _, n in declared)
    assert mirrored == [("counts", 9), ("sites", 9), ("ins_unanchored", 1), ("max_depth", 1), ("bases", 6), ("ins_sites", 1), ("ins_longest", 1),
                        ("ins_capped", 1), ("ins_len", 64), ("text_bytes", 1)]
    bound = [name for name, _, _ in P.API]
    assert "pbsim_bam_consensus" in bound and "pbsim_consensus_report" in bound
    assert [n for n, _ in P.ConsensusOpts._fields_] == ["exclude_flags", "min_mapq", "min_baseq", "fill", "min_depth", "max_ins", "line_width", "piece_bytes"]
    assert C.sizeof(P.ConsensusOpts) == 40 and [n for n, _ in P.ConsensusSink._fields_] == ["user", "on_text", "on_record"]
    assert P.CONSENSUS_BASES == K.BASE_NAMES and list(P.CONSENSUS_FILL) == list(K.FILLS)
    assert callable(getattr(P.Context, "bam_consensus")) and callable(P.consensus_report)
    lib = P.load()
    assert hasattr(lib, "pbsim_bam_consensus") and hasattr(lib, "pbsim_consensus_report")


def as_dict(r):
    return dict(counts=r[0], sites=r[1], ins_unanchored=r[2], max_depth=r[3], bases=r[4], ins_sites=r[5], ins_longest=r[6], ins_capped=r[7],
                ins_len=r[8], text_bytes=r[9])


def for_report(r):
    return (r[0], r[1], r[4], r[5], r[6], r[7], r[8])


def random_result(rng):
    pick = lambda: rng.choice([0, 0, 1, 10 ** 12, rng.randrange(2 ** 50)])
    sites = [pick() for _ in range(9)]
    sites[3] = sites[8] + pick()                    # called >= discordant, as a result has it: the ppm value stays inside 64 bits
    return [[rng.randrange(2 ** 31) for _ in range(9)], sites, pick(), pick(), [pick() for _ in range(6)], pick(), pick(), pick(),
            [pick() for _ in range(64)], pick()]


ZERO = [[0] * 9, [0] * 9, 0, 0, [0] * 6, 0, 0, 0, [0] * 64, 0]
ZERO_REPORT = (b"# records=0 skipped_flag=0 unaligned=0 skipped_mapq=0 skipped_ref=0 aligned=0 no_seq=0 misfit=0 scored=0\n"
               b"S" + b"\t0" * 10 + b"\t*\nK" + b"\t0" * 9 + b"\n")


def test_report_of_the_library_is_the_models_without_a_device():
    r = worked()
    assert P.consensus_report(as_dict(r)) == WORKED_REPORT
    by_name = as_dict(r)
    by_name.update(counts=dict(zip(K.COUNT_NAMES, r.counts)), sites=dict(zip(K.SITE_NAMES, r.sites)), bases=dict(zip(K.BASE_NAMES, r.bases)))
    assert P.consensus_report(by_name) == WORKED_REPORT
    assert K.report(*for_report(ZERO)) == ZERO_REPORT == P.consensus_report(as_dict(ZERO))
    rng = random.Random(43)
    for _ in range(30):
        x = random_result(rng)
        assert P.consensus_report(as_dict(x)) == K.report(*for_report(x))
    # the first two lines are the pileup report's
    m = M.pileup(B.stream(WORKED, REFS), GENOME)
    assert WORKED_REPORT.split(b"\n")[:2] == m.report.split(b"\n")[:2]
    assert P.load().pbsim_consensus_report(None, None, 0) == -1
    with pytest.raises(ValueError, match="bases has 5 values"):
        P.consensus_report(dict(as_dict(ZERO), bases=[0] * 5))


# ---------------------------------------------------------------- the option mirror and the command line
GOOD = ["--consensus-bam", "in.bam", "--consensus-genome", "g.fa", "--consensus-out", "out.fa"]
REFUSED = [
    (GOOD + ["--depth", "3"], "(--depth): --consensus-bam takes"),
    (GOOD + ["--pileup-out", "x"], "(--pileup-out): --consensus-bam takes"),
    (GOOD + ["--pileup-bam", "x"], "(--consensus-bam): --pileup-bam takes"),
    (["--consensus-out", "o", "--consensus-bam"], "needs a value"),
    (["--consensus-bam", "in.bam", "--consensus-out", "o"], "--consensus-bam needs --consensus-genome FASTA"),
    (["--consensus-bam", "in.bam", "--consensus-genome", "g.fa"], "--consensus-bam needs --consensus-out FILE"),
    (GOOD + ["--consensus-min-mapq", "256"], "(consensus-min-mapq: 256): a whole number, 0 .. 255"),
    (GOOD + ["--consensus-min-baseq", "-1"], "(consensus-min-baseq: -1): a whole number, 0 .. 255"),
    (GOOD + ["--consensus-min-depth", "x"], "(consensus-min-depth: x): a whole number"),
    (GOOD + ["--consensus-exclude-flags", "65536"], "(consensus-exclude-flags: 65536): decimal or 0x hexadecimal, 0 .. 65535"),
    (GOOD + ["--consensus-exclude-flags", "0xg"], "(consensus-exclude-flags: 0xg): decimal or 0x hexadecimal"),
    (GOOD + ["--consensus-fill", "N"], "(consensus-fill: N): n or ref"),
    (GOOD + ["--consensus-max-ins", "0"], "(consensus-max-ins: 0): a whole number, 1 .. 65535"),
    (GOOD + ["--consensus-max-ins", "65536"], "(consensus-max-ins: 65536): a whole number, 1 .. 65535"),
    (GOOD + ["--consensus-line-width", "1048577"], "(consensus-line-width: 1048577): a whole number, 0 .. 1048576"),
    (GOOD + ["--consensus-line-width", "-1"], "(consensus-line-width: -1): a whole number, 0 .. 1048576"),
    (GOOD + ["--consensus-ref-names", "a,b"], "(consensus-ref-names): 2 names for 1 --consensus-bam files"),
    (GOOD + ["--consensus-bam", "b.bam", "--consensus-ref-names", "a,"], "(consensus-ref-names): an empty name"),
    (GOOD + ["--devices", "0,1"], "--consensus-bam runs on one GPU"),
    (GOOD + ["--processes", "2"], "--consensus-bam runs on one GPU"),
]


def test_option_mirror_accepts_and_rejects():
    assert A.consensus_bam(GOOD) == dict(bams=["in.bam"], genome="g.fa", ref_names=None, out="out.fa", min_mapq=0, min_baseq=0, min_depth=1,
                                         exclude_flags=0x900, fill="n", max_ins=1024, line_width=60)
    got = A.consensus_bam(["--consensus-out", "o", "--consensus-bam", "a", "--consensus-min-mapq", "255", "--consensus-bam", "b", "--consensus-min-baseq",
                           "20", "--consensus-genome", "g", "--consensus-ref-names", "x,y", "--device", "1", "--consensus-fill", "ref",
                           "--consensus-min-depth", "0", "--consensus-exclude-flags", "0x10", "--consensus-max-ins", "65535", "--consensus-line-width", "0"])
    assert got == dict(bams=["a", "b"], genome="g", ref_names=["x", "y"], out="o", min_mapq=255, min_baseq=20, min_depth=0, exclude_flags=16, fill="ref",
                       max_ins=65535, line_width=0)
    for argv, message in REFUSED + [(["--consensus-genome", "g"], "--consensus-bam FILE: name the BAM file")]:
        if "--pileup-bam" in argv:
            continue                                # (the binary hands that line to the pileup's mode, which refuses it)
        with pytest.raises(ValueError) as e:
            A.consensus_bam(argv)
        assert message in str(e.value), argv


def test_cli_refuses_from_the_command_line_alone(tmp_path):
    """the same refusals by the binary, with the mirror's words, before a device or a file is touched"""
    import pbsim3_amd.build as b
    b.build()
    for argv, message in REFUSED:
        r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and r.stdout == "" and message in r.stderr, (argv, r.stderr[-500:])
    r = subprocess.run([CLI] + GOOD, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "Cannot open file: in.bam" in r.stderr
    (tmp_path / "in.bam").write_bytes(B.bam(WORKED, REFS))
    r = subprocess.run([CLI] + GOOD, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "--consensus-genome g.fa: Cannot open file: g.fa" in r.stderr
    assert os.listdir(tmp_path) == ["in.bam"]
    r = subprocess.run([CLI], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert "--consensus-bam FILE [--consensus-bam FILE ...] --consensus-genome FASTA --consensus-out FILE" in r.stderr + r.stdout


# ---------------------------------------------------------------- the checks in front of any device work
REFUSED_OPTS = [(dict(min_mapq=256), "min_mapq must be 0 .. 255"), (dict(exclude_flags=65536), "exclude_flags must be 0 .. 65535"),
                (dict(min_baseq=256), "min_baseq must be 0 .. 255"), (dict(min_baseq=-1), "min_baseq must be 0 .. 255"),
                (dict(min_depth=-1), "min_depth must not be negative"), (dict(piece_bytes=-1), "piece_bytes must not be negative"),
                (dict(max_ins=0), "max_ins must be 1 .. 65535"), (dict(max_ins=65536), "max_ins must be 1 .. 65535"),
                (dict(line_width=-1), "line_width must be 0 .. 1048576"), (dict(line_width=(1 << 20) + 1), "line_width must be 0 .. 1048576")]


def test_bad_arguments_fail_before_device_work():
    data = B.bam(WORKED, REFS)
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), -1) as c:
        for kw, word in REFUSED_OPTS:
            with pytest.raises(P.PbsimError, match="pbsim_bam_consensus: " + word):
                c.bam_consensus(data, GENOME, **kw)
        with pytest.raises(ValueError, match="fill must be n or ref"):
            c.bam_consensus(data, GENOME, fill="N")
        refs = (P.ErrorsRef * 1)(P.ErrorsRef(b"g", C.cast(C.c_char_p(b"ACGT"), C.c_void_p), 4))
        arr = (P.ErrorsFile * 1)(P.ErrorsFile(C.cast(C.c_char_p(data), C.c_void_p), len(data), None))
        res = P.ConsensusResult()
        for fill in (2, -1):
            opts = P.ConsensusOpts(0x900, 0, 0, fill, 1, 1024, 60, 0)
            assert c.lib.pbsim_bam_consensus(c.h, refs, 1, arr, 1, C.byref(opts), None, C.byref(res)) == 0
            assert b"pbsim_bam_consensus: fill must be 0 (N) or 1 (the genome's base)" in c.lib.pbsim_last_error()
        with pytest.raises(P.PbsimError, match="pbsim_bam_consensus: bad argument"):
            c.bam_consensus([], GENOME)
        with pytest.raises(P.PbsimError, match="pbsim_bam_consensus: bad argument"):
            c.bam_consensus(data, [])
        with pytest.raises(P.PbsimError, match=r"pbsim_bam_consensus: the genome holds two records named \"c1\" \(records 0 and 2\)"):
            c.bam_consensus(data, GENOME + [("c1", b"AC")])
        with pytest.raises(ValueError, match="one entry per file"):
            c.bam_consensus(data, GENOME, ref_names=["a", "b"])
        # good arguments reach the device check: a tables-only context refuses as pbsim_inflate_buffer does, and stays usable
        for kw in (dict(), dict(text=False), dict(min_mapq=255, min_baseq=255, min_depth=0, fill="ref", max_ins=65535, line_width=1 << 20,
                                                  ref_names=["c1", None])):
            with pytest.raises(P.PbsimError, match="no HIP device"):
                c.bam_consensus([data, data], GENOME, **kw)


# ---------------------------------------------------------------- the host's decisions under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("asan") / "bam_consensus_rule_driver")
    p = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(harness.ROOT, "tests", "asan", "bam_consensus_rule_driver.cpp"), os.path.join(csrc, "bam_consensus_rule.cpp"),
                        os.path.join(csrc, "bam_pileup_rule.cpp"), "-o", exe], capture_output=True, text=True)
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
    assert drive(driver, "opts", "-") == b"opts 2304 0 0 0 1 1024 60 8388608\n"
    assert drive(driver, "opts", 0, 255, 255, 1, 0, 65535, 1 << 20, 7) == b"opts 0 255 255 1 0 65535 1048576 7\n"
    assert drive(driver, "opts", 4, 0, 0, 0, 1, 1, 0, 0) == b"opts 4 0 0 0 1 1 0 8388608\n"
    for bad, word in (((65536, 0, 0, 0, 1, 1024, 60, 0), b"exclude_flags"), ((-1, 0, 0, 0, 1, 1024, 60, 0), b"exclude_flags"),
                      ((4, 256, 0, 0, 1, 1024, 60, 0), b"min_mapq"), ((4, -1, 0, 0, 1, 1024, 60, 0), b"min_mapq"),
                      ((4, 0, 256, 0, 1, 1024, 60, 0), b"min_baseq"), ((4, 0, -1, 0, 1, 1024, 60, 0), b"min_baseq"),
                      ((4, 0, 0, 2, 1, 1024, 60, 0), b"fill"), ((4, 0, 0, -1, 1, 1024, 60, 0), b"fill"), ((4, 0, 0, 0, -1, 1024, 60, 0), b"min_depth"),
                      ((4, 0, 0, 0, 1, 0, 60, 0), b"max_ins"), ((4, 0, 0, 0, 1, 65536, 60, 0), b"max_ins"), ((4, 0, 0, 0, 1, -5, 60, 0), b"max_ins"),
                      ((4, 0, 0, 0, 1, 1024, -1, 0), b"line_width"), ((4, 0, 0, 0, 1, 1024, (1 << 20) + 1, 0), b"line_width"),
                      ((4, 0, 0, 0, 1, 1024, 60, -1), b"piece_bytes")):
        assert drive(driver, "opts", *bad).startswith(b"opts refused: " + word), bad
    assert drive(driver, "report", *flat(list(worked()[:10]))) == WORKED_REPORT
    assert drive(driver, "report", *flat(ZERO)) == ZERO_REPORT
    rng = random.Random(44)
    for _ in range(5):
        x = random_result(rng)
        assert drive(driver, "report", *flat(x)) == K.report(*for_report(x))
