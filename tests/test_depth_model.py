"""tests/depth_model.py (the rule of `pbsim --depth-bam`) held to values worked out by hand, and the places where the feature
shows without a GPU: the ABI's declarations with their ctypes mirror and the built library's symbols, pbsim_depth_report against
the model's text, the option mirror with the command line's refusals, and the option check in front of any device work."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import bam_writer as B
import depth_model as M
import harness
import pbsim3_amd as P
from pbsim3_amd import args as A

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def rec(pos, cigar, ref=0, flag=0, mapq=60, name="r", **kw):
    """cigar: "3M1I2M" """
    ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    return B.record(name, flag, ref, pos, cigar=ops, seq=kw.pop("seq", ""), qual=kw.pop("qual", b""), mapq=mapq, **kw)


def run(recs, refs, **kw):
    return M.depth(B.stream(recs, refs), **kw)


def lines(text):
    return [tuple(l.split(b"\t")) for l in text.split(b"\n")[:-1]]


# ---------------------------------------------------------------- the worked case of the rule
WORKED = [rec(2, "3M1I2M", name="A"), rec(4, "2M2D1M", name="B"), rec(8, "5M", name="C")]
WORKED_REPORT = (b"# records=3 counted=3 skipped_flag=0 skipped_unplaced=0 skipped_mapq=0 clipped=1\n"
                 b"R\tc\t10\t8\t12\t2\t1200\nH\t0\t2\nH\t1\t4\nH\t2\t4\n")


def test_the_worked_case():
    r = run(WORKED, [("c", 10)])
    assert r.arrays == [[0, 0, 1, 1, 2, 2, 2, 1, 2, 1]]
    assert r.text == b"c\t0\t2\t0\nc\t2\t4\t1\nc\t4\t7\t2\nc\t7\t8\t1\nc\t8\t9\t2\nc\t9\t10\t1\n"
    assert r.counts == [3, 3, 0, 0, 0, 1]
    assert r.refs == [(b"c", 10, 8, 12, 2)]
    assert {d: n for d, n in enumerate(r.hist) if n} == {0: 2, 1: 4, 2: 4}
    assert r.report == WORKED_REPORT
    w = run(WORKED, [("c", 10)], fmt="window", window=4)
    assert w.text == b"c\t0\t4\t2\t500\nc\t4\t8\t7\t1750\nc\t8\t10\t3\t1500\n"
    assert (w.counts, w.refs, w.hist, w.report) == (r.counts, r.refs, r.hist, r.report)
    n = run(WORKED, [("c", 10)], deletions=False)
    assert n.arrays == [[0, 0, 1, 1, 2, 2, 1, 0, 2, 1]]
    assert n.text == b"c\t0\t2\t0\nc\t2\t4\t1\nc\t4\t6\t2\nc\t6\t7\t1\nc\t7\t8\t0\nc\t8\t9\t2\nc\t9\t10\t1\n"
    assert n.refs == [(b"c", 10, 7, 10, 2)] and n.counts == [3, 3, 0, 0, 0, 1]
    assert run(WORKED, [("c", 10)], fmt="window", window=4, deletions=False).text == b"c\t0\t4\t2\t500\nc\t4\t8\t5\t1250\nc\t8\t10\t3\t1500\n"


# ---------------------------------------------------------------- more by hand
def test_touching_intervals_are_one_run():
    r = run([rec(0, "4M"), rec(4, "3=2X"), rec(9, "1M")], [("c", 10)])
    assert r.arrays == [[1] * 10] and r.text == b"c\t0\t10\t1\n" and r.counts == [3, 3, 0, 0, 0, 0]


def test_n_splits_a_record_and_a_span_of_zero_covers_nothing():
    r = run([rec(1, "2M3N2M"), rec(5, "4S2I3H1P"), rec(7, "0M")], [("c", 10)])
    assert r.arrays == [[0, 1, 1, 0, 0, 0, 1, 1, 0, 0]]
    assert r.counts == [3, 3, 0, 0, 0, 0] and r.refs == [(b"c", 10, 4, 4, 1)]


def test_the_cg_placeholder_with_and_without_its_tag():
    cg = [(3 << 4) | 0, (2 << 4) | 2, (1 << 4) | 8]                   # 3M2D1X
    front = [("XA", "A", "q"), ("Xc", "c", -3), ("XC", "C", 200), ("Xs", "s", -300), ("XS", "S", 60000), ("Xi", "i", -70000),
             ("XI", "I", 4000000000), ("Xf", "f", 1.5), ("XZ", "Z", "text"), ("XH", "H", "1AE3"), ("XB", "Bs", [-1, 2, 3]),
             ("CG", "Z", "not this one")]
    with_tag = rec(2, "5S6N", seq="ACGTA", qual=b"\x10" * 5, tags=front + [("CG", "BI", cg)])
    r = run([with_tag], [("c", 10)])
    assert r.arrays == [[0, 0, 1, 1, 1, 1, 1, 1, 0, 0]] and r.counts == [1, 1, 0, 0, 0, 0]
    assert run([with_tag], [("c", 10)], deletions=False).arrays == [[0, 0, 1, 1, 1, 0, 0, 1, 0, 0]]
    without = rec(2, "5S6N", seq="ACGTA", qual=b"\x10" * 5, tags=front)
    r = run([without], [("c", 10)])
    assert r.arrays == [[0] * 10] and r.counts == [1, 1, 0, 0, 0, 0]
    # an S that is not l_seq long is no placeholder: the tag is not read
    other = rec(2, "4S6N", seq="ACGTA", qual=b"\x10" * 5, tags=[("CG", "BI", cg)])
    assert run([other], [("c", 10)]).arrays == [[0] * 10]


def test_malformed_records_name_their_offset():
    refs = [("c", 10)]
    first = rec(0, "1M")
    at = len(B.stream([first], refs))
    with pytest.raises(M.Malformed) as e:
        M.depth(B.stream([first, rec(1, "2M")], refs)[:-4] + (9 | 2 << 4).to_bytes(4, "little"))
    assert e.value.offset == at
    cut = B.record_bytes(rec(2, "5S6N", seq="ACGTA", qual=b"\x10" * 5, tags=[("XZ", "Z", "runs on")]))
    cut = (len(cut) - 4 - 1).to_bytes(4, "little") + cut[4:-1]                  # the Z string loses its NUL
    with pytest.raises(M.Malformed) as e:
        M.depth(B.stream([first], refs) + cut)
    assert e.value.offset == at
    bad_type = B.record_bytes(rec(2, "5S6N", seq="ACGTA", qual=b"\x10" * 5, tags=[("XQ", "C", 7)])).replace(b"XQC", b"XQq")
    with pytest.raises(M.Malformed):
        M.depth(B.stream([first], refs) + bad_type)
    # the same bytes in a skipped record, or in one that is no placeholder, are never looked at
    skipped = B.record_bytes(rec(2, "5S6N", flag=4, seq="ACGTA", qual=b"\x10" * 5, tags=[("XQ", "C", 7)])).replace(b"XQC", b"XQq")
    assert M.depth(B.stream([first], refs) + skipped).counts == [2, 1, 1, 0, 0, 0]


def test_skip_classes_in_their_order():
    refs = [("c", 10)]
    recs = [rec(0, "2M", flag=4, ref=-1),           # flagged and unplaced: the flag comes first
            rec(0, "2M", flag=0x100), rec(0, "2M", flag=0x200), rec(0, "2M", flag=0x400),
            rec(-1, "2M", ref=0), rec(3, "2M", ref=-1),
            rec(0, "2M", mapq=9), rec(0, "2M", mapq=10), rec(0, "2M", flag=0x800 | 16, mapq=11)]
    r = run(recs, refs, min_mapq=10)
    assert r.counts == [9, 2, 4, 2, 1, 0] and r.arrays == [[2, 2] + [0] * 8]
    assert run(recs, refs).counts == [9, 3, 4, 2, 0, 0]
    r = run(recs, refs, exclude_flags=0)
    assert r.counts == [9, 6, 0, 3, 0, 0] and r.arrays[0][0] == 6         # the secondary counts, flag 4 with refID -1 is now unplaced
    assert run(recs, refs, exclude_flags=0x800).counts == [9, 5, 1, 3, 0, 0]


def test_a_reference_of_length_zero_between_two_others():
    r = run([rec(0, "2M", ref=0), rec(0, "2M", ref=1), rec(1, "5M", ref=2)], [("a", 3), ("empty", 0), ("b", 4)])
    assert r.text == b"a\t0\t2\t1\na\t2\t3\t0\nb\t0\t1\t0\nb\t1\t4\t1\n"
    assert r.refs == [(b"a", 3, 2, 2, 1), (b"empty", 0, 0, 0, 0), (b"b", 4, 3, 3, 1)]
    assert r.counts == [3, 3, 0, 0, 0, 2] and [len(a) for a in r.arrays] == [3, 0, 4]
    assert r.report == (b"# records=3 counted=3 skipped_flag=0 skipped_unplaced=0 skipped_mapq=0 clipped=2\n"
                        b"R\ta\t3\t2\t2\t1\t666\nR\tb\t4\t3\t3\t1\t750\nH\t0\t2\nH\t1\t5\n")
    assert run([], [("a", 3), ("empty", 0)], fmt="window", window=2).text == b"a\t0\t2\t0\t0\na\t2\t3\t0\t0\n"


def test_windows_larger_than_the_reference_and_not_dividing_it():
    recs = [rec(1, "8M"), rec(3, "3M")]
    assert run(recs, [("c", 10)], fmt="window", window=11).text == b"c\t0\t10\t11\t1100\n"
    assert run(recs, [("c", 10)], fmt="window", window=10).text == b"c\t0\t10\t11\t1100\n"
    assert run(recs, [("c", 10)], fmt="window", window=3).text == b"c\t0\t3\t2\t666\nc\t3\t6\t6\t2000\nc\t6\t9\t3\t1000\nc\t9\t10\t0\t0\n"
    assert run(recs, [("c", 10)], fmt="window", window=1).text == b"".join(
        b"c\t%d\t%d\t%d\t%d\n" % (p, p + 1, d, 1000 * d) for p, d in enumerate([0, 1, 1, 2, 2, 2, 1, 1, 1, 0]))


def test_the_last_histogram_bin_takes_a_depth_of_300():
    r = run([rec(1, "2M", name="s%d" % k) for k in range(300)] + [rec(2, "2M")], [("c", 5)])
    assert r.arrays == [[0, 300, 301, 1, 0]] and r.hist[255] == 2 and r.hist[0] == 2 and r.hist[1] == 1 and sum(r.hist) == 5
    assert r.refs == [(b"c", 5, 3, 602, 301)]
    assert r.report.endswith(b"R\tc\t5\t3\t602\t301\t120400\nH\t0\t2\nH\t1\t1\nH\t255\t2\n")


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_calls_and_the_library_has_them():
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        h = f.read()
    assert re.search(r"int pbsim_bam_depth\(pbsim_ctx \*ctx, const void \*bam, int64_t n, const pbsim_depth_opts \*opts,\s*"
                     r"const pbsim_depth_sink \*sink, int64_t counts\[6\], int64_t hist\[256\]\);", h)
    assert re.search(r"int64_t pbsim_depth_report\(const int64_t counts\[6\], int32_t n_ref, const char \*const \*names, const int64_t \*rows,\s*"
                     r"const int64_t hist\[256\], char \*buf, int64_t cap\);", h)
    assert re.search(r"typedef struct pbsim_depth_opts \{[^;]*int32_t exclude_flags, min_mapq, count_deletions;\s*int32_t format;[^;]*"
                     r"int64_t window;[^;]*int64_t piece_bytes;", h)
    assert re.search(r"typedef struct pbsim_depth_sink \{\s*void \*user;\s*int \(\*on_text\)\(void \*user, const char \*bytes, int64_t n, int64_t offset\);", h)
    bound = [name for name, _, _ in P.API]
    assert "pbsim_bam_depth" in bound and "pbsim_depth_report" in bound
    assert [n for n, _ in P.DepthOpts._fields_] == ["exclude_flags", "min_mapq", "count_deletions", "format", "window", "piece_bytes"]
    assert C.sizeof(P.DepthOpts) == 32
    assert [n for n, _ in P.DepthSink._fields_] == ["user", "on_text", "on_refs", "on_depth"]
    assert P.DEPTH_COUNTS == M.COUNT_NAMES and callable(getattr(P.Context, "bam_depth")) and callable(P.depth_report)
    lib = P.load()
    assert hasattr(lib, "pbsim_bam_depth") and hasattr(lib, "pbsim_depth_report")


def test_report_of_the_library_is_the_models_without_a_device():
    r = run(WORKED, [("c", 10)])
    assert P.depth_report(r.counts, r.refs, r.hist) == WORKED_REPORT
    assert P.depth_report(dict(zip(M.COUNT_NAMES, r.counts)), r.refs, r.hist) == WORKED_REPORT
    rng = random.Random(31)
    for _ in range(20):
        refs = []
        for k in range(rng.randrange(0, 6)):
            l_ref = rng.choice([0, 1, 7, 10 ** 6, 2 ** 31 - 1])
            total = rng.choice([0, 1, l_ref, l_ref * (2 ** 31 - 1), rng.randrange(l_ref * 2 ** 31)]) if l_ref else 0      # (a depth is an int32)
            refs.append((b"ref%d|x" % k, l_ref, rng.randrange(l_ref + 1), total, rng.randrange(2 ** 31)))
        hist = [rng.choice([0, 0, 1, 10 ** 12]) for _ in range(256)]
        counts = [rng.randrange(2 ** 31) for _ in range(6)]
        assert P.depth_report(counts, refs, hist) == M.report(counts, refs, hist)
    assert P.depth_report([0] * 6, [], [0] * 256) == b"# records=0 counted=0 skipped_flag=0 skipped_unplaced=0 skipped_mapq=0 clipped=0\n"
    assert P.load().pbsim_depth_report(None, 0, None, None, None, None, 0) == -1


# ---------------------------------------------------------------- the option mirror and the command line
GOOD = ["--depth-bam", "in.bam", "--depth-out", "out.bedgraph"]
REFUSED = [
    (GOOD + ["--depth", "3"], "(--depth): --depth-bam takes"),
    (GOOD + ["--eval-out", "x"], "(--eval-out): --depth-bam takes"),
    (["--depth-bam", "in.bam"], "--depth-bam needs --depth-out FILE"),
    (["--depth-out", "o", "--depth-bam"], "needs a value"),
    (GOOD + ["--depth-format", "window", "--depth-window", "0"], "(depth-window: 0): a whole number of at least 1"),
    (GOOD + ["--depth-format", "window", "--depth-window", "-5"], "(depth-window: -5): a whole number of at least 1"),
    (GOOD + ["--depth-format", "window", "--depth-window", "1e3"], "(depth-window: 1e3): a whole number of at least 1"),
    (GOOD + ["--depth-format", "window"], "--depth-format window needs --depth-window N"),
    (GOOD + ["--depth-window", "100"], "--depth-window N goes with --depth-format window"),
    (GOOD + ["--depth-format", "bedgraph", "--depth-window", "100"], "--depth-window N goes with --depth-format window"),
    (GOOD + ["--depth-format", "bed"], "(depth-format: bed): bedgraph or window"),
    (GOOD + ["--depth-min-mapq", "256"], "(depth-min-mapq: 256): a whole number, 0 .. 255"),
    (GOOD + ["--depth-exclude-flags", "0xZZ"], "(depth-exclude-flags: 0xZZ): decimal or 0x hexadecimal"),
    (GOOD + ["--depth-exclude-flags", "65536"], "(depth-exclude-flags: 65536): decimal or 0x hexadecimal"),
    (GOOD + ["--devices", "0,1"], "--depth-bam runs on one GPU"),
    (GOOD + ["--processes", "2"], "--depth-bam runs on one GPU"),
]


def test_option_mirror_accepts_and_rejects():
    assert A.depth_bam(GOOD) == dict(bam="in.bam", out="out.bedgraph", format="bedgraph", window=0, min_mapq=0, exclude_flags=0x704,
                                     deletions=True)
    got = A.depth_bam(["--depth-out", "o", "--depth-no-deletions", "--depth-format", "window", "--depth-window", "4096", "--depth-bam", "i",
                       "--depth-min-mapq", "255", "--depth-exclude-flags", "0xF04", "--device", "1"])
    assert got == dict(bam="i", out="o", format="window", window=4096, min_mapq=255, exclude_flags=0xF04, deletions=False)
    assert A.depth_bam(GOOD + ["--depth-exclude-flags", "1796"])["exclude_flags"] == 0x704
    assert A.depth_bam(GOOD + ["--depth-exclude-flags", "0"])["exclude_flags"] == 0
    for argv, message in REFUSED:
        with pytest.raises(ValueError) as e:
            A.depth_bam(argv)
        assert message in str(e.value), argv


def test_cli_refuses_from_the_command_line_alone(tmp_path):
    """the same refusals by the binary, with the mirror's words, before a device or a file is touched"""
    import pbsim3_amd.build as b
    b.build()
    for argv, message in REFUSED:
        r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and r.stdout == "" and message in r.stderr, (argv, r.stderr[-500:])
    r = subprocess.run([CLI] + GOOD + ["--depth-no-deletions", "--depth-exclude-flags", "0x4"], capture_output=True, text=True, cwd=str(tmp_path),
                       timeout=120)
    assert r.returncode != 0 and "Cannot open file: in.bam" in r.stderr
    assert not os.listdir(tmp_path)
    r = subprocess.run([CLI], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert "--depth-bam FILE --depth-out FILE" in r.stderr + r.stdout


# ---------------------------------------------------------------- the option check comes before any device work
def test_bad_options_fail_before_device_work():
    data = B.bam(WORKED, [("c", 10)])
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), -1) as c:
        with pytest.raises(P.PbsimError, match="pbsim_bam_depth: window must be at least 1"):
            c.bam_depth(data, fmt="window", window=0)
        with pytest.raises(P.PbsimError, match="pbsim_bam_depth: min_mapq must be 0 .. 255"):
            c.bam_depth(data, min_mapq=256)
        with pytest.raises(P.PbsimError, match="pbsim_bam_depth: min_mapq must be 0 .. 255"):
            c.bam_depth(data, min_mapq=-1)
        with pytest.raises(P.PbsimError, match="pbsim_bam_depth: piece_bytes must not be negative"):
            c.bam_depth(data, piece_bytes=-1)
        counts, hist = (C.c_int64 * 6)(), (C.c_int64 * 256)()
        for fmt in (2, -1):
            opts = P.DepthOpts(0x704, 0, 1, fmt, 0, 0)
            assert c.lib.pbsim_bam_depth(c.h, data, len(data), C.byref(opts), None, counts, hist) == 0
            assert b"format must be 0 (bedgraph) or 1 (window)" in c.lib.pbsim_last_error()
        with pytest.raises(ValueError):
            c.bam_depth(data, fmt="bed")
        # good options reach the device check: a tables-only context refuses as pbsim_inflate_buffer does, and stays usable
        for kw in (dict(), dict(fmt="window", window=4)):
            with pytest.raises(P.PbsimError, match="no HIP device"):
                c.bam_depth(data, **kw)
        assert c.lib.pbsim_bam_depth(c.h, data, len(data), None, None, counts, hist) == 0
        assert b"no HIP device" in c.lib.pbsim_last_error()


# ---------------------------------------------------------------- the host's decisions under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("asan") / "bam_depth_rule_driver")
    p = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(harness.ROOT, "tests", "asan", "bam_depth_rule_driver.cpp"), os.path.join(csrc, "bam_depth_rule.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if p.returncode != 0 and "sanitize" in p.stderr:
        pytest.skip("no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def drive(exe, *argv):
    p = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, timeout=60)
    assert p.returncode == 0, (argv, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout


def test_rule_code_under_asan(driver):
    assert drive(driver, "opts", "-") == b"opts 1796 0 1 0 0 8388608\n"
    assert drive(driver, "opts", 0, 255, 0, 1, 1, 7) == b"opts 0 255 0 1 1 7\n"
    assert drive(driver, "opts", 4, 0, 1, 0, 99, 0) == b"opts 4 0 1 0 0 8388608\n"           # a window beside bedgraph is not used
    for bad, word in (((4, 0, 1, 2, 0, 0), b"format"), ((4, 0, 1, 1, 0, 0), b"window"), ((4, 256, 1, 0, 0, 0), b"min_mapq"),
                      ((4, -1, 1, 0, 0, 0), b"min_mapq"), ((4, 0, 1, 0, 0, -1), b"piece_bytes")):
        assert drive(driver, "opts", *bad).startswith(b"opts refused: " + word)
    assert drive(driver, "offsets", 0, 10, 0, 3) == b"offsets 0 11 12 16 |\n"
    assert drive(driver, "offsets", 4, 10, 0, 3, 8) == b"offsets 0 11 12 16 25 | 0 3 3 4 6\n"
    assert drive(driver, "offsets", 1, 2 ** 31 - 1, 2 ** 31 - 1) == b"offsets 0 2147483648 4294967296 | 0 2147483647 4294967294\n"
    assert drive(driver, "offsets", 0) == b"offsets 0 |\n"
    assert drive(driver, "offsets", 0, 5, -1).startswith(b"offsets refused: reference 1 has the negative length -1")
    assert drive(driver, "report", 3, 3, 0, 0, 0, 1, "R", "c", 10, 8, 12, 2, "H", 0, 2, "H", 1, 4, "H", 2, 4) == WORKED_REPORT
    top = 2 ** 31 - 1
    refs = [(b"a|b", top, top, top * top, top), (b"empty", 0, 0, 0, 0), (b"z", 1, 0, 0, 0)]
    hist = [0] * 255 + [2 ** 40]
    argv = [2 ** 31 - 1] * 6 + [x for r in refs for x in ("R", r[0].decode()) + r[1:]] + ["H", 255, 2 ** 40]
    assert drive(driver, "report", *argv) == M.report([2 ** 31 - 1] * 6, refs, hist)
