"""`pbsim --depth-bam` (pbsim_bam_depth; pbsim3_amd/csrc/bam_depth.hip, bam_depth.cpp): the depth of coverage of a BAM on the GPU.
Files built here with tests/bam_writer.py go through Context.bam_depth, and the text, the counts, the references' rows, the
histogram, the report and the per-base arrays must be what tests/depth_model.py says, byte for byte; then the product's own truth
files through the command line."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import pytest

import bam_spec_reader as R
import bam_writer as B
import depth_model as M
import harness
import pbsim3_amd as P
from cases import CASES

pytestmark = pytest.mark.gpu

OPS = "MIDNSHP=X"


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


def check(ctx, stream, container="bgzf", block=B.W.BGZIP_BLOCK, piece_bytes=0, **kw):
    """an inflated stream -> through the product in `container`, every output against the model; returns the model's result"""
    want = M.depth(stream, **kw)
    text, counts, refs, hist, report, arrays = ctx.bam_depth(B.contain(stream, container, block), arrays=True, piece_bytes=piece_bytes, **kw)
    assert [counts[n] for n in M.COUNT_NAMES] == want.counts
    assert refs == want.refs
    assert hist.tolist() == want.hist
    assert [a.tolist() for a in arrays] == want.arrays
    assert text == want.text
    assert report == want.report
    return want


def rec(pos, cigar, ref=0, flag=0, mapq=60, name="r", **kw):
    """cigar: "3M1I2M", or a list of (length, op letter)"""
    ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)] if isinstance(cigar, str) else list(cigar)
    return B.record(name, flag, ref, pos, cigar=ops, seq=kw.pop("seq", ""), qual=kw.pop("qual", b""), mapq=mapq, **kw)


def mixed_ops(rng, n):
    """n ops of all nine kinds, most of them short, none of length 0 except a few"""
    out = []
    for k in range(n):
        op = OPS[k % 9] if k % 5 else rng.choice(OPS)
        out.append((rng.choice([0, 1, 1, 2, 3, 7]) if k % 11 == 0 else rng.randrange(1, 5), op))
    return out


def placeholder(pos, ops, ref=0, l_seq=5, front=(), **kw):
    """the record SAMv1 4.2.2 writes for a CIGAR that does not fit the field: <l_seq>S<span>N, the ops in CG:B,I"""
    span = sum(n for n, op in ops if op in "MDN=X")
    tags = list(front) + [("CG", "BI", [n << 4 | OPS.index(op) for n, op in ops])]
    return rec(pos, [(l_seq, "S"), (span, "N")], ref=ref, seq="ACGTA"[:l_seq], qual=b"\x11" * l_seq, tags=tags, **kw)


EVERY_AUX = [("XA", "A", "q"), ("Xc", "c", -3), ("XC", "C", 200), ("Xs", "s", -300), ("XS", "S", 60000), ("Xi", "i", -70000),
             ("XI", "I", 4000000000), ("Xf", "f", 1.5), ("XZ", "Z", "some text"), ("XH", "H", "1AE3"), ("Xb", "Bc", [-1, 2]),
             ("XB", "BC", b"\x01\x02\x03"), ("Xt", "Bs", [-1, 2, 3]), ("XT", "BS", [1, 2]), ("Xj", "Bi", [-5]), ("XF", "Bf", [0.5, 2.0]),
             ("CG", "Z", "not this one"), ("CG", "Bi", [16, 32])]


# ---------------------------------------------------------------- the worked case, on the device
def test_the_worked_case(ctx):
    stream = B.stream([rec(2, "3M1I2M"), rec(4, "2M2D1M"), rec(8, "5M")], [("c", 10)])
    r = check(ctx, stream)
    assert r.text == b"c\t0\t2\t0\nc\t2\t4\t1\nc\t4\t7\t2\nc\t7\t8\t1\nc\t8\t9\t2\nc\t9\t10\t1\n" and r.counts[5] == 1
    assert check(ctx, stream, fmt="window", window=4).text == b"c\t0\t4\t2\t500\nc\t4\t8\t7\t1750\nc\t8\t10\t3\t1500\n"
    assert check(ctx, stream, deletions=False).arrays == [[0, 0, 1, 1, 2, 2, 1, 0, 2, 1]]
    check(ctx, stream, fmt="window", window=4, deletions=False)


# ---------------------------------------------------------------- shapes that break kernels
LENGTHS = [1, 63, 64, 65, 0, 4095, 4096, 4097, 300_007]


def edge_records(rng, refs, per_ref=12):
    """on every reference: records that start at 0, end exactly at l_ref, one base past it and wholly past it, a record at
    pos -1, and a few inside"""
    out = []
    for r, (_, l) in enumerate(refs):
        out += [rec(0, [(max(l // 2, 1), "M")], ref=r), rec(max(l - 3, 0), [(min(l, 3), "M")], ref=r), rec(max(l - 3, 0), [(min(l, 3) + 1, "M")], ref=r),
                rec(l, "4M", ref=r), rec(l + 5, "2M1D2M", ref=r), rec(-1, "5M", ref=r), rec(0, [(l + 1, "M")], ref=r)]
        for _ in range(per_ref if l > 8 else 0):
            a = rng.randrange(l - 4)
            out.append(rec(a, [(rng.randrange(1, min(l - a, 5000)), "M"), (2, "I"), (1, "D"), (3, "N"), (2, "=")], ref=r))
    rng.shuffle(out)
    return out


def test_reference_lengths_across_scan_blocks_and_tiles(ctx):
    rng = random.Random(3)
    refs = [("L%d" % l, l) for l in LENGTHS]
    stream = B.stream(edge_records(rng, refs), refs)
    r = check(ctx, stream)
    assert r.counts[3] == len(refs) and r.counts[5] >= 4 * len(refs) and [row[1] for row in r.refs] == LENGTHS
    check(ctx, stream, fmt="window", window=4096, deletions=False)


def test_many_references_share_a_tile(ctx):
    """3000 references of 1 to 40 positions: a tile of the runs pass holds two hundred of them, more than its LDS cells"""
    rng = random.Random(4)
    refs = [("t%d" % k, 1 + (k * 7) % 40) for k in range(3000)]
    recs = []
    for k in range(0, 3000, 2):
        l = refs[k][1]
        a = rng.randrange(l)
        recs += [rec(a, [(rng.randrange(1, l - a + 2), "M")], ref=k)] * (1 + k % 3)
    stream = B.stream(recs, refs)
    r = check(ctx, stream)
    assert sum(1 for row in r.refs if row[2]) == 1500
    check(ctx, stream, fmt="window", window=7)


def test_op_counts_on_either_side_of_the_wave_path(ctx):
    """CIGARs of 1, 64, 65, 128, 129 and 65 535 ops (all the field holds) of all nine kinds; a CG placeholder with a 3-op tag and
    one with 70 000 ops; a placeholder whose tag lies behind tags of every aux type, among them a CG that is no B,I"""
    rng = random.Random(5)
    refs = [("chr", 400_000), ("other", 9000)]
    recs = [rec(rng.randrange(1000), mixed_ops(rng, n), name="n%d" % n) for n in (1, 64, 65, 128, 129, 65_535)]
    recs += [rec(150_000, mixed_ops(rng, 200), name="w1"), rec(150_100, mixed_ops(rng, 300), name="w2", flag=16)]       # neighbours in one wave
    recs += [placeholder(77, [(3, "M"), (2, "D"), (4, "X")]), placeholder(200_000, mixed_ops(rng, 70_000)),
             placeholder(5000, [(30, "="), (10, "N"), (5, "M")], front=EVERY_AUX, ref=1),
             placeholder(8990, mixed_ops(rng, 90), ref=1),                                                                # clipped in the wave path
             rec(10, "5S40N", seq="ACGTA", qual=b"\x11" * 5, tags=EVERY_AUX),                                             # no tag: covers nothing
             rec(10, "4S40N", seq="ACGTA", qual=b"\x11" * 5, tags=[("CG", "BI", [50 << 4])])]                            # no placeholder
    for order in (recs, recs[::-1]):
        stream = B.stream(order, refs)
        r = check(ctx, stream, block=1024)
        check(ctx, stream, deletions=False, container="none")
    assert r.counts == [14, 14, 0, 0, 0, 1] and r.arrays[0][10:50] == M.depth(B.stream(recs[:8], refs)).arrays[0][10:50]


def test_stacking_and_colliding_events(ctx):
    """300 records on one position (hist[255], the maximum), and records whose +1 and -1 meet on one slot"""
    refs = [("c", 1000)]
    recs = [rec(500, "3M")] * 300 + [rec(100 + 10 * k, "10M") for k in range(20)] + [rec(300, "10M"), rec(290, "10M2N10M")] * 7
    r = check(ctx, B.stream(recs, refs))
    assert r.hist[255] == 3 and r.refs[0][4] == 300 and r.arrays[0][100:290] == [1] * 190
    assert r.arrays[0][288:314] == [1, 1] + [8] * 10 + [7, 7] + [14] * 8 + [7, 7] + [0, 0]
    check(ctx, B.stream(recs, refs), fmt="window", window=1)


def test_line_widths(ctx):
    """runs whose start and end go from 9 to 10, 99 to 100 and 99 999 to 100 000, and depths that do: 100 000 records of one base"""
    refs = [("c", 100_010)]
    recs = [rec(p, "1M") for p in (9, 10, 99, 100, 99_999, 100_000, 100_009)] + [rec(3, "1M")] * 9 + [rec(4, "1M")] * 10 + \
           [rec(5, "1M")] * 99 + [rec(6, "1M")] * 100
    stream = B.stream(recs, refs) + B.record_bytes(rec(7, "2M")) * 99_999 + B.record_bytes(rec(8, "1M"))
    r = check(ctx, stream, container="none")
    for line in (b"c\t3\t4\t9\n", b"c\t4\t5\t10\n", b"c\t5\t6\t99\n", b"c\t6\t7\t100\n", b"c\t7\t8\t99999\n", b"c\t8\t9\t100000\n",
                 b"c\t9\t11\t1\n", b"c\t99\t101\t1\n", b"c\t101\t99999\t0\n", b"c\t99999\t100001\t1\n", b"c\t100009\t100010\t1\n"):
        assert line in r.text
    assert check(ctx, stream, container="none", fmt="window", window=9).text.startswith(b"c\t0\t9\t200217\t22246333\nc\t9\t18\t2\t222\n")


@pytest.mark.parametrize("window", [1, 7, 4096, 10_000, 10_001])
def test_window_sizes(ctx, window):
    rng = random.Random(8)
    refs = [("a", 1), ("b", 63), ("c", 4097), ("empty", 0), ("d", 10_000)]
    check(ctx, B.stream(edge_records(rng, refs, 30), refs), fmt="window", window=window, deletions=bool(window % 2))


def test_containers_and_members_of_one_kibibyte(ctx):
    rng = random.Random(9)
    refs = [("a", 5000), ("b", 300)]
    stream = B.stream(edge_records(rng, refs, 200) + [placeholder(40, mixed_ops(rng, 700), front=EVERY_AUX)], refs, text=b"@HD\tVN:1.6\n")
    for container in ("bgzf", "stored", "gzip", "none"):
        check(ctx, stream, container=container, block=1024)


def test_order_independence(ctx):
    rng = random.Random(10)
    refs = [("a", 20_000), ("b", 3000)]
    recs = edge_records(rng, refs, 300)
    first = ctx.bam_depth(B.bam(recs, refs), arrays=True)
    for seed in (1, 2):
        random.Random(seed).shuffle(recs)
        again = ctx.bam_depth(B.bam(recs, refs), arrays=True)
        assert again[:3] == first[:3] and again[3].tolist() == first[3].tolist() and again[4] == first[4]
        assert all((a == b).all() for a, b in zip(again[5], first[5]))
    check(ctx, B.stream(recs, refs))


def random_records(rng, refs, n):
    out = []
    for k in range(n):
        r = rng.randrange(len(refs))
        l = refs[r][1]
        kind = k % 23
        flag = [0, 16, 0x800, 0x100, 0x400, 4, 0x200][kind % 7 if kind < 14 else 0]
        pos = rng.randrange(-1, l + 3) if kind == 20 else rng.randrange(max(l - 1, 1))
        ops = mixed_ops(rng, rng.choice([1, 2, 3, 5, 8, 30, 63, 64, 65, 66, 150]))
        if kind == 21:
            out.append(placeholder(pos, ops, ref=r, mapq=rng.randrange(60), flag=flag))
        else:
            out.append(rec(pos, ops, ref=r if kind != 22 else -1, flag=flag, mapq=rng.randrange(60), name="q%d" % k,
                           seq="ACGT"[k % 4] * (k % 7), qual=bytes([k % 40]) * (k % 7), tags=(("NM", "C", k % 200),) if k % 3 else ()))
    return out


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_randomized(ctx, seed):
    rng = random.Random(seed)
    refs = [("r%d" % k, rng.choice([50, 700, 5000, 20_000])) for k in range(rng.randrange(1, 6))]
    stream = B.stream(random_records(rng, refs, 3000), refs)
    check(ctx, stream, block=[1024, 4000, B.W.BGZIP_BLOCK][seed % 3], min_mapq=seed % 2 * 20)
    check(ctx, stream, deletions=False, exclude_flags=[0, 0x704, 0xF04][seed % 3])
    check(ctx, stream, fmt="window", window=[100, 333, 4096][seed % 3], container="none")
    check(ctx, stream, fmt="window", window=64, deletions=False, min_mapq=30)


def test_no_records_and_no_references(ctx):
    assert check(ctx, B.stream([], [("a", 5), ("z", 0)])).text == b"a\t0\t5\t0\n"
    assert check(ctx, B.stream([], [])).text == b""
    assert check(ctx, B.stream([rec(-1, "", ref=-1, flag=4)], []), fmt="window", window=3).counts == [1, 0, 1, 0, 0, 0]
    assert check(ctx, B.stream([rec(0, "1M")], [("z", 0)])).counts == [1, 1, 0, 0, 0, 1]


# ---------------------------------------------------------------- the text's way to the sink
def deliver(ctx, data, piece_bytes, stop_after=None):
    pieces = []

    def on_text(user, ptr, n, offset):
        pieces.append((offset, C.string_at(ptr, n)))
        return 0 if stop_after is not None and len(pieces) >= stop_after else 1
    sink = P.DepthSink(None, P.DEPTH_TEXT_CB(on_text), P.DEPTH_REFS_CB(), P.DEPTH_ARRAY_CB())
    opts = P.DepthOpts(0x704, 0, 1, 0, 0, piece_bytes)
    counts, hist = (C.c_int64 * 6)(), (C.c_int64 * 256)()
    ok = ctx.lib.pbsim_bam_depth(ctx.h, data, len(data), C.byref(opts), C.byref(sink), counts, hist)
    return ok, pieces


def test_delivery_in_pieces(ctx):
    rng = random.Random(14)
    refs = [("a", 900), ("b", 70)]
    stream = B.stream(edge_records(rng, refs, 25), refs)
    want = M.depth(stream).text
    assert 200 < len(want) < 4096
    data = B.contain(stream)
    for piece in (0, 1, 7, 4096):
        ok, pieces = deliver(ctx, data, piece)
        assert ok == 1 and b"".join(p for _, p in pieces) == want
        at = 0
        for offset, p in pieces:
            assert offset == at and 1 <= len(p) <= (piece or len(want))
            at += len(p)
        assert len(pieces) == (-(-len(want) // piece) if piece else 1)
    ok, pieces = deliver(ctx, data, 7, stop_after=3)
    assert ok == 0 and len(pieces) == 3 and b"sink aborted (text)" in ctx.lib.pbsim_last_error()
    check(ctx, stream, piece_bytes=7)
    # and a text of many pieces of 4096 bytes
    big = B.stream([rec(2 * k, "1M") for k in range(15_000)], [("c", 30_001)])
    check(ctx, big, piece_bytes=4096, container="none")


# ---------------------------------------------------------------- failures
def test_failures_name_the_offset_and_leave_the_context_usable(ctx):
    refs = [("c", 1000)]
    good = [rec(10 * k, "5M2D5M") for k in range(50)]
    head = B.stream(good, refs)

    def usable():
        assert check(ctx, head).counts == [50, 50, 0, 0, 0, 0]

    bad_op = B.record_bytes(rec(1, "2M"))[:-4] + struct.pack("<I", 2 << 4 | 9)
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_depth: the record at inflated byte offset %d is malformed" % len(head)):
        ctx.bam_depth(B.contain(head + bad_op + B.record_bytes(good[0]), "bgzf"))
    usable()
    long_bad = B.record_bytes(rec(1, [(1, "M")] * 99 + [(1, "P")]))[:-4] + struct.pack("<I", 1 << 4 | 12)          # in the wave path
    with pytest.raises(P.PbsimError, match=r"inflated byte offset %d is malformed" % (len(head) + len(bad_op))):
        ctx.bam_depth(B.contain(head + B.record_bytes(rec(1, "2M")) + long_bad, "none"))
    usable()
    cut = B.record_bytes(placeholder(2, [(3, "M")], front=[("XZ", "Z", "runs on")]))
    z_at = cut.index(b"XZZ")
    cut = cut[:z_at] + b"XZZ" + cut[z_at + 3:].replace(b"\0", b"x")                       # no NUL up to the record's end
    with pytest.raises(P.PbsimError, match=r"inflated byte offset %d is malformed: .* an aux field that runs past the record" % len(head)):
        ctx.bam_depth(B.contain(head + cut + B.record_bytes(good[0]), "bgzf"))
    usable()
    count_at = B.record_bytes(placeholder(2, [(3, "M")])).index(b"CGBI") + 4
    over = bytearray(B.record_bytes(placeholder(2, [(3, "M")])))
    over[count_at:count_at + 4] = struct.pack("<I", 2)                                       # an array of two where one is there
    with pytest.raises(P.PbsimError, match=r"inflated byte offset %d is malformed" % len(head)):
        ctx.bam_depth(B.contain(head + bytes(over), "gzip"))
    unknown = B.record_bytes(placeholder(2, [(3, "M")], front=[("XQ", "C", 7)])).replace(b"XQC", b"XQq")
    with pytest.raises(P.PbsimError, match=r"inflated byte offset %d is malformed" % len(head)):
        ctx.bam_depth(B.contain(head + unknown, "stored"))
    # the same bytes in a skipped record are not looked at
    skipped = B.record_bytes(placeholder(2, [(3, "M")], front=[("XQ", "C", 7)], flag=0x400)).replace(b"XQC", b"XQq")
    assert check(ctx, head + skipped).counts == [51, 50, 1, 0, 0, 0]
    with pytest.raises(P.PbsimError, match="pbsim_bam_depth: neither BGZF, gzip nor an uncompressed BAM"):
        ctx.bam_depth(b"@HD\tVN:1.6\n")
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_depth: the record at inflated byte offset %d does not fit" % len(head)):
        ctx.bam_depth(B.contain(head + b"\0" * 40 + b"\x07" * 30, "bgzf"))
    usable()


# ---------------------------------------------------------------- the product's own files, through the command line
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def _run(cmd, workdir, ok=True):
    r = subprocess.run(cmd, capture_output=True, cwd=workdir, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr[-4000:]
    return r


def _simulate(case, workdir, more=()):
    import pbsim3_amd.build as b
    b.build()
    os.makedirs(workdir, exist_ok=True)
    _run([CLI] + harness.resolve(CASES[case]["args"]) + ["--prefix", os.path.join(workdir, "out"), "--truth-format", "bam"] + list(more), workdir)
    return sorted(os.path.join(workdir, n) for n in os.listdir(workdir) if n.endswith(".aln.bam"))


def _inflate(path):
    with open(path, "rb") as f:
        return b"".join(R.blocks(f.read()))


def _depth_cli(aln, workdir, more=()):
    out = aln + ".depth.txt"
    r = _run([CLI, "--depth-bam", aln, "--depth-out", out] + list(more), workdir)
    with open(out, "rb") as f:
        return f.read(), r.stdout


@pytest.mark.parametrize("case", ["wgs_errhmm-ont_quirk", "trans_errhmm_sequel", "wgs_errhmm_sequel_pass3"])
def test_cli_on_the_products_own_truth_files(tmp_path, case):
    alns = _simulate(case, str(tmp_path / "u"))
    srts = _simulate(case, str(tmp_path / "s"), ["--truth-sort", "coordinate"])
    assert alns and len(alns) == len(srts)
    for aln, srt in zip(alns, srts):
        stream = _inflate(aln)
        want = M.depth(stream)
        assert want.counts[1] == want.counts[0] > 0 and want.counts[5] == 0
        text, report = _depth_cli(aln, str(tmp_path))
        assert text == want.text and report == want.report
        # nothing is clipped in a truth file: the depths add up to the records' covered spans
        spans = sum(e - s for r in M.parse(stream)[1] for s, e in M.covered(r))
        assert sum(row[3] for row in want.refs) == spans > 0
        assert _inflate(srt) != stream or len(M.parse(stream)[1]) < 2
        assert _depth_cli(srt, str(tmp_path))[0] == text
        w = M.depth(stream, fmt="window", window=500, deletions=False, min_mapq=1)
        text, report = _depth_cli(aln, str(tmp_path), ["--depth-format", "window", "--depth-window", "500", "--depth-no-deletions", "--depth-min-mapq", "1",
                                                      "--depth-exclude-flags", "0x704"])
        assert text == w.text and report == w.report


def test_cli_failure_leaves_no_output(tmp_path):
    bad = tmp_path / "bad.bam"
    bad.write_bytes(B.bam([rec(1, "2M")], [("c", 10)])[:-40])
    out = tmp_path / "o.bedgraph"
    r = _run([CLI, "--depth-bam", str(bad), "--depth-out", str(out)], str(tmp_path), ok=False)
    assert b"pbsim_bam_depth: " in r.stderr and r.stdout == b"" and not out.exists()
