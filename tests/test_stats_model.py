"""tests/stats_model.py (the rule of `pbsim --stats-bam`) held to values worked out by hand, and the places where the feature shows
without a GPU: the table E against 80-digit decimals, the ABI's declarations with their ctypes mirror and the built library's
symbols, pbsim_stats_report against the model's text, the option mirror with the command line's refusals, the option check in
front of any device work, and the HIP-free rule file under the sanitizers."""
import ctypes as C
import decimal
import os
import random
import re
import subprocess

import pytest

import bam_spec_reader as R
import bam_writer as B
import harness
import pbsim3_amd as P
import stats_model as M
from pbsim3_amd import args as A

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def rec(name, pos, cigar, flag=0, ref=0, mapq=60, qual=b"", tags=()):
    ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    return B.record(name, flag, ref, pos, cigar=ops, qual=qual, tags=tags, mapq=mapq)


# ---------------------------------------------------------------- the worked case of the rule
# r1: 6 columns, NM 2 = 1 inserted base + 1 substitution: identity 4/6; six bases of Q10: esum = 6 E[10], accuracy 0.9
# r2: 1S2M2D1M: 5 columns, NM 2 = the 2 deleted bases: identity 3/5; Q 0 20 20 30: mean error (1 + 0.01 + 0.01 + 0.001) / 4 = 0.25525
# u1: unaligned, no qualities; s1: secondary, skipped; r3: aligned, no bases, no NM
# lengths 6 4 3: 13 bases, mean 4.333, variance (3 x 61 - 169) / 9 = 1.55: sd 1; median 4; descending 6 | 10 | 13 of 13:
# 6 suffices up to 40 % (600 >= 520), 10 up to 70 % (1000 >= 910), 13 for the rest
WORKED = [rec("r1", 2, "3M1I2M", qual=bytes([10] * 6), tags=[("NM", "C", 2)]),
          rec("r2", 4, "1S2M2D1M", qual=bytes([0, 20, 20, 30]), tags=[("NM", "i", 2)]),
          rec("u1", -1, "", flag=4, ref=-1, qual=b"\xff" * 3),
          rec("s1", 7, "3M", flag=0x100, qual=bytes([5] * 3)),
          rec("r3", 9, "5M")]
WORKED_TEXT = (b"r1\tA\t6\t6\t2\t1\t0\t0\t666666\t10000\t900000\n"
               b"r2\tA\t4\t5\t2\t0\t2\t1\t600000\t17500\t744751\n"
               b"u1\tU\t3\t*\t*\t*\t*\t*\t*\t*\t*\n"
               b"r3\tA\t0\t5\t*\t0\t0\t0\t*\t*\t*\n")
WORKED_REPORT = (b"# records=5 skipped_flag=1 unaligned=1 skipped_mapq=0 aligned=3 no_seq=1 no_qual=1 no_nm=1 nm_bad=0 scored=2\n"
                 b"L\t3\t13\t3\t6\t4333\t1\t4\t6\t6\t6\t6\t4\t4\t4\t3\t3\n"
                 b"E\t1\t1\t2\t11\t90909\t90909\t181818\t250\t250\t500\t633333\n"
                 b"Q\t822375\t13000\n"
                 b"HQ\t0\t1\nHQ\t10\t6\nHQ\t20\t2\nHQ\t30\t1\nHI\t600\t1\nHI\t666\t1\nHA\t744\t1\nHA\t900\t1\n")
WORKED_REFS = [("c", 100)]


def test_the_worked_case():
    r = M.stats(B.stream(WORKED, WORKED_REFS))
    assert r.counts == [5, 1, 1, 0, 3, 1, 1, 1, 0, 2]
    assert r.len_row == [3, 13, 3, 6, 4333, 1, 4, 6, 6, 6, 6, 4, 4, 4, 3, 3]
    assert r.totals == [11, 1, 1, 2, 1, 1, 1, 0, 666666 + 600000, 900000 + 744751, 2, 130]
    assert r.text == WORKED_TEXT and r.report == WORKED_REPORT
    # the secondary counts without the default filter; min_mapq at the boundary skips or keeps the aligned three
    assert M.stats(B.stream(WORKED, WORKED_REFS), exclude_flags=0).counts[:5] == [5, 0, 1, 0, 4]
    assert M.stats(B.stream(WORKED, WORKED_REFS), min_mapq=60).counts[:5] == [5, 1, 1, 0, 3]
    assert M.stats(B.stream(WORKED, WORKED_REFS), min_mapq=61).counts == [5, 1, 1, 3, 0, 0, 1, 0, 0, 0]
    two = M.stats([B.stream(WORKED[:2], WORKED_REFS), B.stream(WORKED[2:], [])])
    assert two == r


def test_the_models_parse_agrees_with_the_specification_reader():
    rng = random.Random(2)
    recs = [rec("q%d" % k, rng.randrange(50), "%dM2I%dS" % (k + 1, k % 3 + 1), qual=bytes(rng.randrange(60) for _ in range(k + 3 + k % 3 + 1)),
                tags=[("NM", "C", 2), ("XZ", "Z", "t%d" % k)], mapq=k) for k in range(20)]
    raw = B.bam(recs, WORKED_REFS)
    mine = M.parse(M.inflate(raw))
    _, _, theirs = R.read_bam(raw)
    assert len(mine) == len(theirs) == 20
    for a, b in zip(mine, theirs):
        assert (a["name"].decode(), a["flag"], a["ref_id"], a["pos"], a["mapq"], a["l_seq"], a["qual"]) == \
               (b["read_name"], b["flag"], b["refID"], b["pos"], b["mapq"], b["l_seq"], b["qual"])
        assert [(n, "MIDNSHP=X"[op]) for n, op in a["cigar"]] == b["cigar"]
        assert M.aux_walk(a["aux"], 0, False, True)[1] == dict((t, v) for t, _, v in b["aux"])["NM"]


def test_nm_rules_by_hand():
    def one(cigar, tags, n_qual=4):
        return M.stats(B.stream([rec("x", 0, cigar, qual=bytes([20] * n_qual), tags=tags)], WORKED_REFS))
    assert one("4M", [("NM", "c", -1)]).counts[7:] == [1, 0, 0]                       # negative: no_nm
    assert one("4M", [("NM", "Z", "3")]).counts[7:] == [1, 0, 0]                      # no integer type: not NM
    assert one("4M", [("NM", "Z", "3"), ("NM", "S", 1), ("NM", "C", 4)]).totals[1] == 1   # the first integer NM; the second is ignored
    assert one("2M2I", [("NM", "C", 1)]).counts[7:] == [0, 1, 0]                      # nm < ins + del
    assert one("2M1I1S", [("NM", "C", 4)], 4).counts[7:] == [0, 1, 0]                 # nm - ins - del > m
    assert one("4S", [("NM", "C", 0)]).counts[7:] == [0, 1, 0]                        # cols == 0
    assert one("4S", []).counts[7:] == [1, 0, 0]                                      # no NM comes first
    r = one("2M0I1D0D2=1X3H", [("NM", "I", 2)], 5)
    assert r.counts[7:] == [0, 0, 1] and r.totals[:9] == [6, 1, 0, 1, 0, 1, 0, 3, 666666]


def test_malformed_records_name_their_offset():
    first = rec("a", 0, "1M", qual=b"\x05", tags=[("NM", "C", 0)])
    at = len(B.stream([first], WORKED_REFS))
    with pytest.raises(M.Malformed) as e:
        M.stats(B.stream([first, rec("b", 1, "2M", tags=[])], WORKED_REFS)[:-4] + (9 | 2 << 4).to_bytes(4, "little"))
    assert e.value.offset == at
    cut = B.record_bytes(rec("b", 1, "2M", tags=[("XZ", "Z", "runs on")]))
    cut = (len(cut) - 4 - 1).to_bytes(4, "little") + cut[4:-1]                  # the Z string loses its NUL
    with pytest.raises(M.Malformed) as e:
        M.stats(B.stream([first], WORKED_REFS) + cut)
    assert e.value.offset == at
    # behind NM the fields are not looked at; in an unaligned record none is
    behind = B.record_bytes(rec("b", 1, "2M", tags=[("NM", "C", 0), ("XQ", "C", 7)])).replace(b"XQC", b"XQq")
    assert M.stats(B.stream([first], WORKED_REFS) + behind).counts[9] == 2
    unal = B.record_bytes(rec("b", 1, "2M", flag=4, tags=[("XQ", "C", 7)])).replace(b"XQC", b"XQq")
    assert M.stats(B.stream([first], WORKED_REFS) + unal).counts[:5] == [2, 0, 1, 0, 1]
    front = B.record_bytes(rec("b", 1, "2M", tags=[("XQ", "C", 7), ("NM", "C", 0)])).replace(b"XQC", b"XQq")
    with pytest.raises(M.Malformed):
        M.stats(B.stream([first], WORKED_REFS) + front)


def test_length_row_ties_and_extremes():
    assert M.length_row([]) == [0] * 16
    assert M.length_row([7]) == [1, 7, 7, 7, 7000, 0, 7] + [7] * 9
    assert M.length_row([5] * 4) == [4, 20, 5, 5, 5000, 0, 5] + [5] * 9
    # descending 10 10 5 5: the running sums 10 20 25 30: 10 % = 3 is reached by the first, 70 % = 21 by the third
    assert M.length_row([5, 10, 5, 10]) == [4, 30, 5, 10, 7500, 2, 5, 10, 10, 10, 10, 10, 10, 5, 5, 5]
    top = 2 ** 31 - 1
    assert M.length_row([top, 1])[:7] == [2, top + 1, 1, top, (top + 1) * 500, (top - 1) // 2, 1]


# ---------------------------------------------------------------- the table E
def test_the_table_against_80_digit_decimals():
    decimal.getcontext().prec = 80
    assert len(M.E) == 128 and (M.E[0], M.E[1], M.E[93], M.E[127]) == (4294967296, 3411613790, 2, 0)
    for q in range(128):
        exact = decimal.Decimal(2) ** 32 * decimal.Decimal(10) ** (decimal.Decimal(-q) / 10)
        assert abs(exact - int(exact) - decimal.Decimal("0.5")) > decimal.Decimal("0.003"), q       # no entry near a rounding tie
        assert M.E[q] == int(exact.to_integral_value(rounding=decimal.ROUND_HALF_EVEN)), q
    with open(os.path.join(harness.ROOT, "pbsim3_amd", "csrc", "bam_stats_rule.cpp")) as f:
        body = re.search(r"kStatsE\[kStatsQBins\] = \{(.*?)\};", f.read(), re.S).group(1)
    assert [int(v) for v in re.findall(r"(\d+)ull", body)] == M.E


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_calls_and_the_library_has_them():
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        h = f.read()
    assert re.search(r"int pbsim_bam_stats\(pbsim_ctx \*ctx, const pbsim_stats_file \*files, int n_files, const pbsim_stats_opts \*opts,\s*"
                     r"const pbsim_stats_sink \*sink, int64_t counts\[10\], int64_t len_row\[16\], int64_t totals\[12\],\s*"
                     r"int64_t hist_q\[128\], int64_t hist_identity\[1001\], int64_t hist_qacc\[1001\]\);", h)
    assert re.search(r"int64_t pbsim_stats_report\(const int64_t counts\[10\], const int64_t len_row\[16\], const int64_t totals\[12\],\s*"
                     r"const int64_t hist_q\[128\], const int64_t hist_identity\[1001\], const int64_t hist_qacc\[1001\],\s*"
                     r"char \*buf, int64_t cap\);", h)
    assert re.search(r"typedef struct pbsim_stats_opts \{[^;]*int32_t exclude_flags, min_mapq;\s*int64_t piece_bytes;", h)
    bound = [name for name, _, _ in P.API]
    assert "pbsim_bam_stats" in bound and "pbsim_stats_report" in bound
    assert [n for n, _ in P.StatsOpts._fields_] == ["exclude_flags", "min_mapq", "piece_bytes"] and C.sizeof(P.StatsOpts) == 16
    assert [n for n, _ in P.StatsFile._fields_] == ["bam", "n"] and [n for n, _ in P.StatsSink._fields_] == ["user", "on_text"]
    assert (P.STATS_COUNTS, P.STATS_LEN_ROW, P.STATS_TOTALS) == (M.COUNT_NAMES, M.LEN_NAMES, M.TOTAL_NAMES)
    assert callable(getattr(P.Context, "bam_stats")) and callable(P.stats_report)
    lib = P.load()
    assert hasattr(lib, "pbsim_bam_stats") and hasattr(lib, "pbsim_stats_report")


def random_result(rng):
    top = 2 ** 31 - 1
    counts = [rng.randrange(2 ** 31) for _ in range(10)]
    len_row = [rng.choice([0, 1, top, rng.randrange(2 ** 62)]) for _ in range(16)]
    totals = [rng.choice([0, 1, rng.randrange(2 ** 40), rng.randrange(2 ** 60)]) for _ in range(12)]
    totals[0] = sum(totals[1:4]) + rng.choice([0, 1, rng.randrange(2 ** 60)])       # cols = sub + ins + del + the matches
    hists = [[rng.choice([0, 0, 0, 1, 10 ** 12]) for _ in range(n)] for n in (128, 1001, 1001)]
    return counts, len_row, totals, hists


def test_report_of_the_library_is_the_models_without_a_device():
    r = M.stats(B.stream(WORKED, WORKED_REFS))
    assert P.stats_report(r.counts, r.len_row, r.totals, r.hist_q, r.hist_identity, r.hist_qacc) == WORKED_REPORT
    assert P.stats_report(dict(zip(M.COUNT_NAMES, r.counts)), dict(zip(M.LEN_NAMES, r.len_row)), dict(zip(M.TOTAL_NAMES, r.totals)),
                          r.hist_q, r.hist_identity, r.hist_qacc) == WORKED_REPORT
    rng = random.Random(31)
    for _ in range(20):
        counts, len_row, totals, hists = random_result(rng)
        assert P.stats_report(counts, len_row, totals, *hists) == M.report(counts, len_row, totals, *hists)
    zero = P.stats_report([0] * 10, [0] * 16, [0] * 12, [0] * 128, [0] * 1001, [0] * 1001)
    assert zero == M.report([0] * 10, [0] * 16, [0] * 12, [0] * 128, [0] * 1001, [0] * 1001)
    assert zero.endswith(b"E\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\nQ\t0\t0\n")
    assert P.load().pbsim_stats_report(None, None, None, None, None, None, None, 0) == -1


# ---------------------------------------------------------------- the option mirror and the command line
GOOD = ["--stats-bam", "in.bam"]
REFUSED = [
    (GOOD + ["--depth", "3"], "(--depth): --stats-bam takes"),
    (GOOD + ["--depth-out", "x"], "(--depth-out): --stats-bam takes"),
    (["--stats-out", "o", "--stats-bam"], "needs a value"),
    (GOOD + ["--stats-min-mapq", "256"], "(stats-min-mapq: 256): a whole number, 0 .. 255"),
    (GOOD + ["--stats-min-mapq", "-1"], "(stats-min-mapq: -1): a whole number, 0 .. 255"),
    (GOOD + ["--stats-exclude-flags", "0xZZ"], "(stats-exclude-flags: 0xZZ): decimal or 0x hexadecimal"),
    (GOOD + ["--stats-exclude-flags", "65536"], "(stats-exclude-flags: 65536): decimal or 0x hexadecimal"),
    (GOOD + ["--devices", "0,1"], "--stats-bam runs on one GPU"),
    (GOOD + ["--processes", "2"], "--stats-bam runs on one GPU"),
]


def test_option_mirror_accepts_and_rejects():
    assert A.stats_bam(GOOD) == dict(bams=["in.bam"], out=None, min_mapq=0, exclude_flags=0x900)
    got = A.stats_bam(["--stats-out", "o", "--stats-bam", "a", "--stats-min-mapq", "255", "--stats-bam", "b", "--stats-exclude-flags", "0xF04",
                       "--device", "1"])
    assert got == dict(bams=["a", "b"], out="o", min_mapq=255, exclude_flags=0xF04)
    assert A.stats_bam(GOOD + ["--stats-exclude-flags", "2304"])["exclude_flags"] == 0x900
    assert A.stats_bam(GOOD + ["--stats-exclude-flags", "0"])["exclude_flags"] == 0
    for argv, message in REFUSED + [(["--stats-out", "o"], "--stats-bam FILE: name the BAM file")]:
        with pytest.raises(ValueError) as e:
            A.stats_bam(argv)
        assert message in str(e.value), argv


def test_cli_refuses_from_the_command_line_alone(tmp_path):
    """the same refusals by the binary, with the mirror's words, before a device or a file is touched"""
    import pbsim3_amd.build as b
    b.build()
    for argv, message in REFUSED:
        r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and r.stdout == "" and message in r.stderr, (argv, r.stderr[-500:])
    r = subprocess.run([CLI] + GOOD + ["--stats-out", "o.tsv", "--stats-exclude-flags", "0x4"], capture_output=True, text=True, cwd=str(tmp_path),
                       timeout=120)
    assert r.returncode != 0 and "Cannot open file: in.bam" in r.stderr
    assert not os.listdir(tmp_path)
    r = subprocess.run([CLI], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert "--stats-bam FILE [--stats-bam FILE ...]" in r.stderr + r.stdout


# ---------------------------------------------------------------- the option check comes before any device work
def test_bad_options_fail_before_device_work():
    data = B.bam(WORKED, WORKED_REFS)
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), -1) as c:
        with pytest.raises(P.PbsimError, match="pbsim_bam_stats: min_mapq must be 0 .. 255"):
            c.bam_stats(data, min_mapq=256)
        with pytest.raises(P.PbsimError, match="pbsim_bam_stats: min_mapq must be 0 .. 255"):
            c.bam_stats(data, min_mapq=-1)
        with pytest.raises(P.PbsimError, match="pbsim_bam_stats: exclude_flags must be 0 .. 65535"):
            c.bam_stats(data, exclude_flags=65536)
        with pytest.raises(P.PbsimError, match="pbsim_bam_stats: piece_bytes must not be negative"):
            c.bam_stats(data, piece_bytes=-1)
        with pytest.raises(P.PbsimError, match="pbsim_bam_stats: bad argument"):
            c.bam_stats([])
        # good options reach the device check: a tables-only context refuses as pbsim_inflate_buffer does, and stays usable
        for kw in (dict(), dict(text=True), dict(min_mapq=255, exclude_flags=0)):
            with pytest.raises(P.PbsimError, match="no HIP device"):
                c.bam_stats([data, data], **kw)


# ---------------------------------------------------------------- the host's decisions under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("asan") / "bam_stats_rule_driver")
    p = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(harness.ROOT, "tests", "asan", "bam_stats_rule_driver.cpp"), os.path.join(csrc, "bam_stats_rule.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if p.returncode != 0 and "sanitize" in p.stderr:
        pytest.skip("no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def drive(exe, *argv):
    p = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, timeout=60)
    assert p.returncode == 0, (argv, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout


def sd_args(lengths_with_counts):
    """N BASES SQ_LO SQ_HI as the device carries them, for a multiset given as (length, how many)"""
    n = sum(k for _, k in lengths_with_counts)
    bases = sum(l * k for l, k in lengths_with_counts)
    lo = sum((l * l & 0xFFFFFFFF) * k for l, k in lengths_with_counts)
    hi = sum((l * l >> 32) * k for l, k in lengths_with_counts)
    assert lo < 2 ** 64 and hi < 2 ** 64
    return n, bases, lo, hi


def test_rule_code_under_asan(driver):
    assert drive(driver, "opts", "-") == b"opts 2304 0 8388608\n"
    assert drive(driver, "opts", 0, 255, 7) == b"opts 0 255 7\n"
    assert drive(driver, "opts", 65535, 0, 0) == b"opts 65535 0 8388608\n"
    for bad, word in (((65536, 0, 0), b"exclude_flags"), ((-1, 0, 0), b"exclude_flags"), ((4, 256, 0), b"min_mapq"), ((4, -1, 0), b"min_mapq"),
                      ((4, 0, -1), b"piece_bytes")):
        assert drive(driver, "opts", *bad).startswith(b"opts refused: " + word)
    assert drive(driver, "table") == b"table " + " ".join(str(v) for v in M.E).encode() + b"\n"
    top = 2 ** 31 - 1
    for lengths in ([(6, 1), (4, 1), (3, 1)], [(7, 1)], [(top, top)], [(top, top - 1), (1, 1)], [(top, 2 ** 30), (1, 2 ** 30 - 1)],
                    [(5, 2), (10, 2)], [(46341, 1000), (46340, 999)]):
        n, bases, lo, hi = sd_args(lengths)
        sumsq = sum(l * l * k for l, k in lengths)
        assert drive(driver, "sd", n, bases, lo, hi) == b"sd %d\n" % M.isqrt((n * sumsq - bases * bases) // (n * n)), lengths
    assert drive(driver, "sd", *sd_args([(top, top)])) == b"sd 0\n"
    assert drive(driver, "sd", 0, 0, 0, 0) == b"sd 0\n"
    assert drive(driver, "muldiv", 2 ** 62 - 1, 1000, 2 ** 31 - 1) == b"muldiv %d\n" % ((2 ** 62 - 1) * 1000 // (2 ** 31 - 1))
    r = M.stats(B.stream(WORKED, WORKED_REFS))

    def hist_args(tag, h):
        return [x for k, v in enumerate(h) if v for x in (tag, k, v)]
    argv = r.counts + r.len_row + r.totals + hist_args("HQ", r.hist_q) + hist_args("HI", r.hist_identity) + hist_args("HA", r.hist_qacc)
    assert drive(driver, "report", *argv) == WORKED_REPORT
    rng = random.Random(32)
    for _ in range(5):
        counts, len_row, totals, hists = random_result(rng)
        argv = counts + len_row + totals + hist_args("HQ", hists[0]) + hist_args("HI", hists[1]) + hist_args("HA", hists[2])
        assert drive(driver, "report", *argv) == M.report(counts, len_row, totals, *hists)
