"""`pbsim --stats-bam` (pbsim_bam_stats; pbsim3_amd/csrc/bam_stats.hip, bam_stats.cpp): the reads of BAM files summarised on the
GPU.  Files built here with tests/bam_writer.py go through Context.bam_stats, and the counts, the length row, the totals, the three
histograms, the text and the report must be what tests/stats_model.py says, byte for byte; then the product's own truth files
through the command line, and the simulation's own statistics beside them."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import pytest

import bam_writer as B
import harness
import pbsim3_amd as P
import stats_model as M
from cases import CASES
from pbsim3_amd import args as A
from test_gpu_bam_depth import EVERY_AUX

pytestmark = pytest.mark.gpu

OPS = "MIDNSHP=X"
with open(os.path.join(harness.ROOT, "pbsim3_amd", "csrc", "bam_stats.h")) as _f:
    TILE = int(re.search(r"constexpr int kStatsTile = (\d+);", _f.read()).group(1))
REFS = [("chr", 1_000_000), ("other", 9000)]


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


def check(ctx, streams, container="bgzf", block=B.W.BGZIP_BLOCK, piece_bytes=0, **kw):
    """inflated streams -> through the product in `container`, every output against the model, with the text and without it;
    returns the model's result"""
    if isinstance(streams, (bytes, bytearray)):
        streams = [streams]
    want = M.stats(streams, **kw)
    files = [B.contain(s, container, block) for s in streams]
    counts, len_row, totals, hist_q, hist_identity, hist_qacc, report, text = ctx.bam_stats(files, text=True, piece_bytes=piece_bytes, **kw)
    assert [counts[n] for n in M.COUNT_NAMES] == want.counts
    assert [len_row[n] for n in M.LEN_NAMES] == want.len_row
    assert [totals[n] for n in M.TOTAL_NAMES] == want.totals
    assert hist_q.tolist() == want.hist_q
    assert hist_identity.tolist() == want.hist_identity
    assert hist_qacc.tolist() == want.hist_qacc
    assert text == want.text
    assert report == want.report
    bare = ctx.bam_stats(files, **kw)
    assert len(bare) == 7 and bare[:3] == (counts, len_row, totals) and bare[6] == report
    return want


def quals(rng, n, top=60):
    return bytes(rng.randrange(top) for _ in range(n))


def sums(ops):
    m = sum(n for n, op in ops if op in "M=X")
    return m, sum(n for n, op in ops if op == "I"), sum(n for n, op in ops if op == "D")


def aligned(name, ops, qual=b"\x14\x15\x16", sub=1, nm_type=None, front=(), back=(), pos=5, ref=0, flag=0, mapq=60):
    """an aligned record whose NM is its inserted and deleted bases and `sub` substitutions (as many as the matches allow)"""
    m, ins, dele = sums(ops)
    nm = ins + dele + min(sub, m)
    tags = list(front) + [("NM", nm_type or R_smallest(nm), nm)] + list(back)
    return B.record(name, flag, ref, pos, cigar=ops, qual=qual, tags=tags, mapq=mapq)


def R_smallest(v):
    return "C" if v < 256 else "S" if v < 65536 else "I"


def unaligned(name, qual, flag=4):
    return B.record(name, flag, -1, -1, qual=qual)


def mixed_ops(rng, n):
    """n ops of all nine kinds, most of them short, a few of length 0"""
    out = []
    for k in range(n):
        op = OPS[k % 9] if k % 5 else rng.choice(OPS)
        out.append((rng.choice([0, 1, 1, 2, 3, 7]) if k % 11 == 0 else rng.randrange(1, 5), op))
    return out


def placeholder(name, ops, qual=b"\x11" * 5, sub=2, front=(), nm_first=True, **kw):
    """the record SAMv1 4.2.2 writes for a CIGAR that does not fit the field: <l_seq>S<span>N, the ops in CG:B,I"""
    span = sum(n for n, op in ops if op in "MDN=X")
    m, ins, dele = sums(ops)
    nm = ("NM", "I", ins + dele + min(sub, m))
    cg = ("CG", "BI", [n << 4 | OPS.index(op) for n, op in ops])
    tags = list(front) + ([nm, cg] if nm_first else [cg, nm])
    return B.record(name, kw.pop("flag", 0), 0, 7, cigar=[(len(qual), "S"), (span, "N")], qual=qual, tags=tags, mapq=60, **kw)


# ---------------------------------------------------------------- the worked case, on the device
def test_the_worked_case(ctx):
    from test_stats_model import WORKED, WORKED_REFS, WORKED_REPORT, WORKED_TEXT
    stream = B.stream(WORKED, WORKED_REFS)
    r = check(ctx, stream)
    assert r.report == WORKED_REPORT and r.text == WORKED_TEXT
    assert check(ctx, stream, exclude_flags=0).counts[:5] == [5, 0, 1, 0, 4]
    assert check(ctx, stream, min_mapq=60).counts[:5] == [5, 1, 1, 0, 3]
    assert check(ctx, stream, min_mapq=61).counts[:5] == [5, 1, 1, 3, 0]


def test_no_records_and_only_skipped_records(ctx):
    r = check(ctx, B.stream([], REFS))
    assert r.counts == [0] * 10 and r.len_row == [0] * 16 and r.text == b""
    assert check(ctx, B.stream([], [])).text == b""
    skipped = [aligned("s%d" % k, [(3, "M")], flag=0x100 if k % 2 else 0x800) for k in range(300)]
    r = check(ctx, B.stream(skipped, REFS))
    assert r.counts == [300, 300] + [0] * 8 and r.len_row == [0] * 16 and r.text == b""
    assert check(ctx, [B.stream([], REFS), B.stream(skipped, REFS), B.stream([], [])]).counts[0] == 300


# ---------------------------------------------------------------- where the quality field lies, and how long it is
L_SEQS = [0, 1, 15, 16, 17, 63, 64, 65, TILE - 1, TILE, TILE + 1]


def test_quality_fields_at_every_alignment_and_length(ctx):
    """read names of 1 .. 16 characters put the quality field at every address mod 16; the lengths lie on either side of a
    sixteen-byte word, of a lane's 64 bytes and of a tile; one read of 300 007 bases spans nineteen tiles"""
    rng = random.Random(1)
    recs = []
    for name_len in range(1, 17):
        for k, l in enumerate(L_SEQS):
            name = "n" * name_len
            recs.append(aligned(name, [(max(l, 1), "M"), (2, "I")], qual=quals(rng, l)) if (k + name_len) % 2 else unaligned(name, quals(rng, l)))
    recs.insert(40, unaligned("long", quals(rng, 300_007)))
    r = check(ctx, B.stream(recs, REFS), container="none")
    assert r.counts[5] == 16 and r.len_row[0] == 16 * 10 + 1 and r.len_row[3] == 300_007 and sum(r.hist_q) == r.len_row[1]


def test_a_thousand_short_reads_share_tiles_with_a_long_one(ctx):
    rng = random.Random(2)
    recs = [unaligned("s%d" % k, quals(rng, 1 + (k * 7) % 40)) for k in range(1000)]
    recs.insert(500, aligned("long", [(3 * TILE + 77, "M")], qual=quals(rng, 3 * TILE + 77)))
    recs.insert(200, unaligned("none", b""))
    recs.insert(700, unaligned("noq", b"\xff" * 50))
    r = check(ctx, B.stream(recs, REFS), block=4000)
    assert r.counts[5:7] == [1, 1] and r.len_row[0] == 1002


def test_quality_values(ctx):
    """no qualities (a first byte 0xFF, whatever follows); 0xFF behind the first byte is a quality; 93, 94, 127, 128 and 254 --
    what lies above 127 counts as 127; all-zero qualities, as ERRHMM truth records carry them"""
    recs = [unaligned("noq", b"\xff" * 20), unaligned("noq2", b"\xff" + bytes(range(19))), unaligned("late", bytes([40]) + b"\xff" * 19),
            unaligned("high", bytes([93, 94, 127, 128, 254]) * 30), unaligned("top", bytes([254]) * 70),
            aligned("zero", [(5000, "M")], qual=bytes(5000)), unaligned("one", bytes([1]) * 3), unaligned("q93", bytes([93]) * 1000)]
    r = check(ctx, B.stream(recs, REFS))
    assert r.counts[6] == 2 and r.hist_q[127] == 19 + 90 + 70 and r.hist_q[0] == 5000 and r.hist_q[94] == 30
    lines = dict(l.split(b"\t", 1) for l in r.text.split(b"\n")[:-1])
    assert lines[b"zero"].endswith(b"\t0\t0") and lines[b"top"].endswith(b"\t127000\t1000000") and lines[b"noq"].endswith(b"\t*\t*")


# ---------------------------------------------------------------- CIGARs and NM
def test_op_counts_on_either_side_of_the_wave_path(ctx):
    """CIGARs of 0 ops (unaligned), 1, 64, 65 and 65 535 ops of all nine kinds with ops of length 0 among them, neighbours in one
    wave, and 70 000 ops through the CG placeholder, NM in front of the tag and behind it"""
    rng = random.Random(5)
    recs = [B.record("n0", 0, 0, 5, qual=b"\x20" * 4, tags=[("NM", "C", 0)])]
    recs += [aligned("n%d" % n, mixed_ops(rng, n), sub=3) for n in (1, 64, 65, 128, 129, 65_535)]
    recs += [aligned("w1", mixed_ops(rng, 200)), aligned("w2", mixed_ops(rng, 300), flag=16)]
    recs += [placeholder("cg3", [(3, "M"), (2, "D"), (4, "X")]), placeholder("cg70000", mixed_ops(rng, 70_000)),
             placeholder("cgback", mixed_ops(rng, 90), nm_first=False), placeholder("cgaux", [(30, "="), (10, "N"), (5, "M")], front=EVERY_AUX),
             B.record("notag", 0, 0, 7, cigar=[(5, "S"), (40, "N")], qual=b"\x11" * 5, tags=EVERY_AUX + [("NM", "C", 0)]),   # no CG: 5S40N itself
             B.record("nope", 0, 0, 7, cigar=[(4, "S"), (40, "N")], qual=b"\x11" * 5, tags=[("CG", "BI", [50 << 4]), ("NM", "C", 0)])]
    for order in (recs, recs[::-1]):
        r = check(ctx, B.stream(order, REFS), block=1024)
    assert r.counts[2] == 1 and r.counts[4] == len(recs) - 1 and r.counts[8] >= 2 and r.counts[9] >= len(recs) - 5
    lines = dict(l.split(b"\t", 1) for l in r.text.split(b"\n")[:-1])
    assert all(lines[n].split(b"\t")[7] != b"*" for n in (b"n65535", b"cg70000", b"cgback", b"cgaux", b"w1", b"w2"))
    nine = [(k + 1, op) for k, op in enumerate(OPS)] + [(0, "I"), (0, "D"), (0, "M")]
    r = check(ctx, B.stream([aligned("nine", nine, sub=4)], REFS), container="none")
    assert r.totals[:9] == [1 + 8 + 9 + 2 + 3, 4, 2, 3, 1, 1, 5, 6, (23 - 9) * 1000000 // 23]


def test_nm_in_every_type_and_place(ctx):
    recs = [aligned("t" + t, [(50, "M"), (1, "I")], sub=3, nm_type=t) for t in "cCsSiI"]
    recs += [aligned("neg" + t, [(50, "M")], nm_type=t) for t in "csi"]
    for r in recs[6:]:
        r["tags"] = tuple((tag, typ, -1) for tag, typ, _ in r["tags"])
    recs += [aligned("behind%d" % k, [(20, "M"), (2, "D")], front=EVERY_AUX[:k + 1]) for k in range(len(EVERY_AUX))]
    recs += [aligned("twice", [(9, "M")], sub=2, back=[("NM", "C", 7)]), aligned("text", [(9, "M")], sub=2, front=[("NM", "Z", "5"), ("NM", "f", 1.5)]),
             B.record("none", 0, 0, 5, cigar=[(4, "M")], qual=b"\x10" * 4, tags=EVERY_AUX),
             B.record("low", 0, 0, 5, cigar=[(4, "M"), (2, "I"), (1, "D")], qual=b"\x10" * 6, tags=[("NM", "C", 2)]),          # nm < ins + del
             B.record("high", 0, 0, 5, cigar=[(4, "M"), (2, "I")], qual=b"\x10" * 6, tags=[("NM", "C", 7)]),                    # nm - ins - del > m
             B.record("edge", 0, 0, 5, cigar=[(4, "M"), (2, "I")], qual=b"\x10" * 6, tags=[("NM", "C", 6)]),                    # every match a substitution
             B.record("clip", 0, 0, 5, cigar=[(6, "S"), (3, "H")], qual=b"\x10" * 6, tags=[("NM", "C", 0)]),                    # cols == 0
             B.record("big", 0, 0, 5, cigar=[(4, "M")], qual=b"\x10" * 4, tags=[("NM", "I", 4_000_000_000)])]
    r = check(ctx, B.stream(recs, REFS))
    n = len(recs)
    assert r.counts[4] == n and r.counts[7] == 4 and r.counts[8] == 4 and r.counts[9] == n - 8
    lines = dict(l.split(b"\t", 1) for l in r.text.split(b"\n")[:-1])
    assert lines[b"twice"].split(b"\t")[3] == b"2" and lines[b"text"].split(b"\t")[3] == b"2" and lines[b"negc"].split(b"\t")[3] == b"*"
    assert lines[b"edge"].split(b"\t")[7] == b"0" and lines[b"big"].split(b"\t")[3] == b"4000000000"


# ---------------------------------------------------------------- lengths
@pytest.mark.parametrize("lengths", [[7], [5] * 300, [5, 10, 5, 10], [10] * 10, [1, 1, 1, 97], [9, 1] * 5, list(range(1, 400)),
                                     [1000] * 9 + [999] * 10 + [1001], [3, 3, 4, 4, 4, 5, 5, 90, 90, 91] * 30])
def test_length_ties_around_the_median_and_the_nx(ctx, lengths):
    """[10] x 10: every running sum 10 k of 100 lies exactly on a threshold; [5, 10, 5, 10], [9, 1] x 5 and the others put equal
    lengths on either side of the median and of the thresholds"""
    recs = [unaligned("r%d" % k, bytes([30]) * l) for k, l in enumerate(lengths)]
    r = check(ctx, B.stream(recs, []), container="none")
    assert r.len_row == M.length_row(lengths) and r.len_row[:4] == [len(lengths), sum(lengths), min(lengths), max(lengths)]


# ---------------------------------------------------------------- files, containers, pieces, filters
def random_records(rng, n):
    out = []
    for k in range(n):
        kind = k % 23
        flag = [0, 16, 0x800, 0x100, 0x400, 4, 0x200][kind % 7 if kind < 14 else 0]
        l = rng.choice([0, 1, 5, 40, 100, 700]) if kind != 19 else rng.randrange(3000)
        q = quals(rng, l, 94) if kind != 18 else b"\xff" * l
        ops = mixed_ops(rng, rng.choice([1, 2, 3, 5, 8, 30, 63, 64, 65, 66, 150]))
        if kind == 21:
            out.append(placeholder("p%d" % k, ops, qual=q, flag=flag, nm_first=k % 2 == 0))
        elif kind == 22:
            out.append(B.record("u%d" % k, 4 if k % 2 else 0, -1, -1, qual=q))
        else:
            rec = aligned("q%d" % k, ops, qual=q, sub=rng.randrange(4), flag=flag, mapq=rng.randrange(60), ref=rng.randrange(2), pos=rng.randrange(8000))
            if kind == 17:
                rec["tags"] = ()
            out.append(rec)
    return out


def test_three_files_and_every_container(ctx):
    rng = random.Random(9)
    streams = [B.stream(random_records(rng, 400), REFS, text=b"@HD\tVN:1.6\n"), B.stream(random_records(rng, 90), REFS[::-1]),
               B.stream(random_records(rng, 700), REFS)]
    r = check(ctx, streams, block=1024)
    assert r.counts[0] == 1190 and r.counts[4] > 500 and r.counts[9] > 300
    for container in ("stored", "gzip", "none"):
        check(ctx, streams[:2], container=container, block=1024)
    check(ctx, streams, exclude_flags=0, min_mapq=30)
    check(ctx, streams[0], exclude_flags=0x904, min_mapq=59)


def deliver(ctx, datas, piece_bytes, stop_after=None):
    pieces = []

    def on_text(user, ptr, n, offset):
        pieces.append((offset, C.string_at(ptr, n)))
        return 0 if stop_after is not None and len(pieces) >= stop_after else 1
    sink = P.StatsSink(None, P.STATS_TEXT_CB(on_text))
    opts = P.StatsOpts(0x900, 0, piece_bytes)
    arr = (P.StatsFile * len(datas))(*[P.StatsFile(C.cast(C.c_char_p(d), C.c_void_p), len(d)) for d in datas])
    out = [(C.c_int64 * k)() for k in (10, 16, 12, 128, 1001, 1001)]
    ok = ctx.lib.pbsim_bam_stats(ctx.h, arr, len(datas), C.byref(opts), C.byref(sink), *out)
    return ok, pieces


def test_delivery_in_pieces(ctx):
    rng = random.Random(14)
    streams = [B.stream(random_records(rng, 40), REFS), B.stream(random_records(rng, 25), REFS)]
    want = M.stats(streams).text
    assert 500 < len(want) < 8192
    datas = [B.contain(s) for s in streams]
    for piece in (0, 1, 7, 4096):
        ok, pieces = deliver(ctx, datas, piece)
        assert ok == 1 and b"".join(p for _, p in pieces) == want
        at = 0
        for offset, p in pieces:
            assert offset == at and 1 <= len(p) <= (piece or len(want))
            at += len(p)
    assert any(not p.endswith(b"\n") for _, p in deliver(ctx, datas, 7)[1])          # a piece ends inside a line
    ok, pieces = deliver(ctx, datas, 7, stop_after=3)
    assert ok == 0 and len(pieces) == 3 and b"sink aborted (text)" in ctx.lib.pbsim_last_error()
    check(ctx, streams, piece_bytes=7)
    # and a text of many pieces of 4096 bytes
    check(ctx, B.stream([unaligned("r%d" % k, b"\x05" * (k % 9)) for k in range(15_000)], []), piece_bytes=4096, container="none")


@pytest.mark.parametrize("seed", [11, 12])
def test_randomized_twice(ctx, seed):
    rng = random.Random(seed)
    stream = B.stream(random_records(rng, 3000), REFS)
    data = B.contain(stream, "bgzf", [1024, B.W.BGZIP_BLOCK][seed % 2])
    first = ctx.bam_stats(data, text=True)
    again = ctx.bam_stats(data, text=True)
    assert first[:3] == again[:3] and first[6:] == again[6:] and all((a == b).all() for a, b in zip(first[3:6], again[3:6]))
    r = check(ctx, stream, block=[1024, B.W.BGZIP_BLOCK][seed % 2])
    assert first[6] == r.report and first[7] == r.text


# ---------------------------------------------------------------- failures
def test_failures_name_the_offset_and_leave_the_context_usable(ctx):
    good = [aligned("g%d" % k, [(5, "M"), (2, "D"), (5, "M")], qual=b"\x1e" * 10) for k in range(50)]
    head = B.stream(good, REFS)

    def usable():
        assert check(ctx, head).counts[9] == 50

    bad_op = B.record_bytes(B.record("b", 0, 0, 1, cigar=[(2, "M")]))[:-4] + struct.pack("<I", 2 << 4 | 9)
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_stats: the record at inflated byte offset %d is malformed" % len(head)):
        ctx.bam_stats(B.contain(head + bad_op + B.record_bytes(good[0]), "bgzf"))
    usable()
    long_bad = B.record_bytes(B.record("b", 0, 0, 1, cigar=[(1, "M")] * 99 + [(1, "P")]))[:-4] + struct.pack("<I", 1 << 4 | 12)     # in the wave path
    with pytest.raises(P.PbsimError, match=r"inflated byte offset %d is malformed" % (len(head) + len(bad_op))):
        ctx.bam_stats(B.contain(head + B.record_bytes(B.record("b", 0, 0, 1, cigar=[(2, "M")])) + long_bad, "none"))
    usable()
    cut = B.record_bytes(B.record("b", 0, 0, 1, cigar=[(3, "M")], qual=b"\x05" * 3, tags=[("XZ", "Z", "runs on")]))
    z_at = cut.index(b"XZZ")
    cut = cut[:z_at] + b"XZZ" + cut[z_at + 3:].replace(b"\0", b"x")                       # no NUL up to the record's end
    with pytest.raises(P.PbsimError, match=r"inflated byte offset %d is malformed: .* an aux field that runs past the record" % len(head)):
        ctx.bam_stats(B.contain(head + cut + B.record_bytes(good[0]), "bgzf"))
    usable()
    unknown = B.record_bytes(B.record("b", 0, 0, 1, cigar=[(3, "M")], tags=[("XQ", "C", 7), ("NM", "C", 0)])).replace(b"XQC", b"XQq")
    with pytest.raises(P.PbsimError, match=r"inflated byte offset %d is malformed" % len(head)):
        ctx.bam_stats(B.contain(head + unknown, "stored"))
    # the same bytes behind NM, in an unaligned record or in a skipped one are not looked at
    behind = B.record_bytes(B.record("b", 0, 0, 1, cigar=[(3, "M")], tags=[("NM", "C", 0), ("XQ", "C", 7)])).replace(b"XQC", b"XQq")
    unal = B.record_bytes(B.record("b", 4, 0, 1, cigar=[(3, "M")], tags=[("XQ", "C", 7)])).replace(b"XQC", b"XQq")
    skipped = B.record_bytes(B.record("b", 0x100, 0, 1, cigar=[(3, "M")], tags=[("XQ", "C", 7)])).replace(b"XQC", b"XQq")
    assert check(ctx, head + behind + unal + skipped).counts == [53, 1, 1, 0, 51, 2, 0, 0, 0, 51]
    # in the second of two files: the message names the file, and no text has been delivered
    ok, pieces = deliver(ctx, [B.contain(head), B.contain(head + bad_op, "none")], 64)
    assert ok == 0 and pieces == []
    assert re.search(rb"pbsim_bam_stats: file 1: the record at inflated byte offset %d is malformed" % len(head), ctx.lib.pbsim_last_error())
    with pytest.raises(P.PbsimError, match="pbsim_bam_stats: neither BGZF, gzip nor an uncompressed BAM"):
        ctx.bam_stats(b"@HD\tVN:1.6\n")
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_stats: the record at inflated byte offset %d does not fit" % len(head)):
        ctx.bam_stats(B.contain(head + b"\0" * 40 + b"\x07" * 30, "bgzf"))
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


def _simulation_stats(case):
    """pbsim_get_stats of every unit of the case, simulated in this process"""
    argv = harness.resolve(CASES[case]["args"])
    p, a = A.parse(argv)
    out = []
    with P.Context(p, 0) as c:
        if p.method == P.METHOD_ERR:
            c.load_errhmm(a["--errhmm"])
        else:
            c.load_qshmm(a["--qshmm"])
        c.set_truth_bam(True)
        if p.strategy == P.STRATEGY_WGS:
            for i, r in enumerate(A.read_fasta(a["--genome"])[0], 1):
                c.set_reference(r, i)
                c.simulate_wgs()
                out.append(c.stats())
        else:
            c.load_transcript_file(a["--transcript"])
            c.simulate_trans()
            out.append(c.stats())
    return [{f: getattr(s, f) for f in ("res_pass_num", "res_len_total", "res_len_min", "res_len_max", "res_sub_num", "res_ins_num", "res_del_num")}
            for s in out]


@pytest.mark.parametrize("case", ["wgs_qshmm_rsii_pass1", "trans_errhmm_sequel"])
def test_cli_on_the_products_own_truth_files(tmp_path, case):
    alns = _simulate(case, str(tmp_path / "u"))
    assert alns and (len(alns) > 1) == case.startswith("wgs")
    streams = []
    for aln in alns:
        with open(aln, "rb") as f:
            streams.append(M.inflate(f.read()))
    want = M.stats(streams)
    out = str(tmp_path / "reads.tsv")
    r = _run([CLI] + [x for aln in alns for x in ("--stats-bam", aln)] + ["--stats-out", out], str(tmp_path))
    with open(out, "rb") as f:
        assert f.read() == want.text
    assert r.stdout == want.report
    assert _run([CLI] + [x for aln in alns for x in ("--stats-bam", aln)], str(tmp_path)).stdout == want.report          # no text asked for
    counts, row, totals = dict(zip(M.COUNT_NAMES, want.counts)), dict(zip(M.LEN_NAMES, want.len_row)), dict(zip(M.TOTAL_NAMES, want.totals))
    assert counts["scored"] == counts["aligned"] == counts["records"] > 0
    # independently of the model: what the simulation itself counted
    sim = _simulation_stats(case)
    print(case, "stats", row, totals, "simulation", sim)
    assert row["n"] == sum(s["res_pass_num"] for s in sim)
    assert row["bases"] == sum(s["res_len_total"] for s in sim)
    assert row["min"] == min(s["res_len_min"] for s in sim) and row["max"] == max(s["res_len_max"] for s in sim)
    nm = sum(M.aux_walk(rec["aux"], 0, False, True)[1] for s in streams for rec in M.parse(s))
    walk = [sum(s[k] for s in sim) for k in ("res_sub_num", "res_ins_num", "res_del_num")]
    assert nm == sum(walk) == totals["sub"] + totals["ins"] + totals["del"]
    assert [totals["sub"], totals["ins"], totals["del"]] == walk
    mapq = _run([CLI, "--stats-bam", alns[0], "--stats-min-mapq", "255", "--stats-exclude-flags", "0x904"], str(tmp_path)).stdout
    assert mapq == M.stats(streams[0], min_mapq=255, exclude_flags=0x904).report


def test_cli_failure_leaves_no_output(tmp_path):
    bad = tmp_path / "bad.bam"
    bad.write_bytes(B.bam([aligned("a", [(2, "M")])], REFS)[:-40])
    out = tmp_path / "o.tsv"
    r = _run([CLI, "--stats-bam", str(bad), "--stats-out", str(out)], str(tmp_path), ok=False)
    assert b"pbsim_bam_stats: " in r.stderr and r.stdout == b"" and not out.exists()
