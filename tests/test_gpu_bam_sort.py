"""`--truth-sort coordinate` (pbsim_truth_bam_sort; pbsim3_amd/csrc/bam_scan.hip, bam_sort.hip, bam_sort.cpp): a finished truth BAM comes
back coordinate-sorted with a CSI index.  Synthetic files built here go through Context.sort_truth_bam and must come back as
tests/csi_model.py says, byte for byte: the header with SO:coordinate, the records in stable (refID, pos) order, the index
of the very members the file has, and region queries through that index that find what a scan of every record finds.  Then
the same through the command line, against the same command without the option."""
import os
import random
import struct
import subprocess

import pytest

import csi_model as M
import harness
import pbsim3_amd as P
from cases import CASES

pytestmark = pytest.mark.gpu

TILE = 4096                     # bytes per workgroup of the record scan (bam_scan.h kBamTile)
SIZES = [65280, 1, 777, 4095, 32768, 3, 12345]       # uneven input members: no record start is aligned to anything


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


def framed(stream, sizes=SIZES, level=1):
    """stream as BGZF members of the given text sizes, in turn, and the EOF block"""
    import bgzf_writer as W
    out, at, k = [], 0, 0
    while at < len(stream):
        n = sizes[k % len(sizes)]
        out.append(W.member(stream[at:at + n], level=level))
        at += n
        k += 1
    return b"".join(out) + W.EOF_MARKER


def sized(ref, pos, name, size, span=1):
    """a record of exactly `size` bytes: one M op, no bases, opaque filler behind the fixed part"""
    fixed = 4 + 32 + len(name) + 1 + 4
    assert size >= fixed, (size, fixed)
    return M.record(ref, pos, name, [(span, "M")], 0, aux=b"a" * (size - fixed))


def queries(refs, recs, seed):
    """twenty regions: seeded ones around the records, a zero-length region, one that touches only a record's last base, one
    just past it, and one on a reference without records where there is one"""
    rng = random.Random(seed)
    f = [M.fields(r) for r in recs]
    out = []
    empty = sorted(set(range(len(refs))) - {x[0] for x in f})
    if empty:
        out.append((empty[len(empty) // 2], 0, refs[empty[len(empty) // 2]][1]))
    if f:
        r, p, e = f[rng.randrange(len(f))]
        out += [(r, e - 1, e), (r, e, e + 1), (r, p, p), (r, max(0, p - 1), p)]
    while len(out) < 20:
        if f:
            r, p, e = f[rng.randrange(len(f))]
            beg = max(0, p + rng.choice([-20000, -1, 0, 1, (e - p) // 2, e - p, 70000]))
            out.append((r, beg, beg + rng.choice([1, 10, 16384, 200000, 1 << 27])))
        else:
            out.append((rng.randrange(len(refs)), 0, 1000) if refs else None)
    return [q for q in out if q]


def check(ctx, refs, recs, sizes=SIZES, text=None, seed=0):
    head = M.header(refs, text)
    raw = framed(head + b"".join(recs), sizes)
    seen = []
    bam, csi, stats = ctx.sort_truth_bam(raw, on_index=seen.append)
    table = M.members(bam)                      # the container rules, on both files
    csi_text = b"".join(t for _, _, t in M.members(csi))
    assert seen == [csi]
    want = M.stable_sort(recs)
    new_head = M.sorted_header(head)
    stream = b"".join(t for _, _, t in table)
    assert stream[:len(new_head)] == new_head
    assert stream[len(new_head):] == b"".join(want), "records: not the stable sort of the input"
    want_csi = M.csi_bytes(refs, want, len(new_head), [(c, len(t)) for c, _, t in table])
    assert csi_text == want_csi
    index = M.read_csi(csi_text)
    n_bins = sum(len(b) - 1 for b in index["refs"] if b)
    assert stats == (len(recs), sum(1 for b in index["refs"] if b), sum(len(r) for r in recs), n_bins)
    for ref, beg, end in queries(refs, want, seed):
        assert M.query(index, bam, ref, beg, end, table) == M.brute(want, ref, beg, end), (ref, beg, end)
    return bam, csi, index


# ---------------------------------------------------------------- the scan
def test_record_starts_around_every_tile_boundary(ctx):
    """record starts at every offset from -40 to +4 around a boundary of the scan's tiles (its halo is 64 bytes: the 36
    fixed bytes of a start 40 bytes before the boundary end 4 bytes before it, those of one 4 bytes behind it lie in the next
    tile), members of uneven sizes, 65 280 and 1 byte among them"""
    refs = [(b"chrA", 5_000_000), (b"chrB", 1000)]
    head_len = len(M.header(refs))
    rng = random.Random(3)
    recs, at, starts = [], head_len, []
    for k, d in enumerate(range(-40, 5)):
        target = (head_len // TILE + 2 + k) * TILE + d
        recs.append(sized(0, rng.randrange(4_000_000), b"fill%d" % k, target - at))
        starts.append(target)
        recs.append(sized(k % 2, rng.randrange(900), b"probe%d" % k, 60 + k % 7))
        at = target + len(recs[-1])
    assert sorted(s % TILE if s % TILE < 100 else s % TILE - TILE for s in starts) == list(range(-40, 5))
    check(ctx, refs, recs, sizes=SIZES + [65536])


def test_a_header_laid_inside_a_record_is_not_a_record(ctx):
    """a complete fake record header inside QUAL whose block_size leads exactly to the next true record, and the natural
    form: SEQ that ends in sixteen 'N' in front of zero qualities -- here with the SEQ bytes before them spelling fields that
    pass every test of the scan.  Both are candidates; neither is on the chain."""
    refs = [(b"ref", 100_000)]
    qual = bytearray(400)
    fake_at = 100
    x_fixed = 4 + 32 + 2 + 4 + 200                     # what lies in front of QUAL in record x
    x_size = x_fixed + 400
    fake = struct.pack("<IiiBBHHHiiii", x_size - (x_fixed + fake_at) - 4, 0, 7, 5, 60, 0, 1, 0, 10, -1, -1, 0)
    qual[fake_at:fake_at + 36] = fake
    x = M.record(0, 5000, b"x", [(400, "M")], 400, seq=bytes([0x12]) * 200, qual=bytes(qual))
    assert len(x) == x_size
    seq = bytes(32) + struct.pack("<IiiBBHHHi", 60, 0, 3, 1, 0, 0, 0, 0, 0) + b"\xff" * 8      # ... 16 x 'N'
    y = M.record(0, 300, b"y", [(128, "M")], 128, seq=seq, qual=bytes(128))
    recs = [sized(0, 9000, b"a", 80), x, sized(0, 100, b"b", 64), y, sized(0, 7000, b"c", 333)]
    bam, _, _ = check(ctx, refs, recs)
    names = [M.name_of(r) for r in M.split_stream(M.inflate(bam))[4]]
    assert names == [b"b", b"y", b"x", b"c", b"a"]


def test_a_broken_chain_is_refused_and_the_context_lives_on(ctx):
    refs = [(b"ref", 100_000)]
    rng = random.Random(8)
    recs = [sized(0, rng.randrange(90_000), b"r%d" % k, 50 + rng.randrange(3000)) for k in range(200)]
    head = M.header(refs)
    bad_at = len(head) + sum(len(r) for r in recs[:120])
    broken = list(recs)
    broken[120] = struct.pack("<I", len(recs[120]) - 4 + 1) + recs[120][4:]
    seen = []
    with pytest.raises(P.PbsimError, match=r"offset %d\b" % bad_at):
        ctx.sort_truth_bam(framed(head + b"".join(broken)), on_index=seen.append)
    assert seen == []
    with pytest.raises(P.PbsimError, match=r"offset %d\b" % len(head)):      # the first record itself
        ctx.sort_truth_bam(framed(head + b"\0" * 50), on_index=seen.append)
    with pytest.raises(P.PbsimError, match="BGZF"):
        ctx.sort_truth_bam(b"not a gzip member at all", on_index=seen.append)
    assert seen == []
    check(ctx, refs, recs)


def test_the_largest_record_and_one_byte_more(ctx):
    """the sort packs offset << 24 | block_size: a record with a block_size of 2^24 - 1 is sorted and indexed, the same record one
    byte longer is refused at its own offset, and the context sorts the good file afterwards"""
    refs = [(b"ref", 100_000)]
    small = [sized(0, 90_000 - 7 * k, b"s%d" % k, 50 + 11 * k) for k in range(6)]
    head = M.header(refs)
    at = len(head) + sum(len(r) for r in small[:3])

    def recs(block_size):
        return small[:3] + [sized(0, 5000, b"largest", 4 + block_size, span=30)] + small[3:]

    seen = []
    with pytest.raises(P.PbsimError, match=r"offset %d\b" % at):
        ctx.sort_truth_bam(framed(head + b"".join(recs(1 << 24)), [65280]), on_index=seen.append)
    assert seen == []
    good = recs((1 << 24) - 1)
    assert struct.unpack_from("<I", good[3])[0] == (1 << 24) - 1
    check(ctx, refs, good, sizes=[65280])


@pytest.fixture(scope="module")
def many_records():
    """5 000 records of about 2 KB on two references, seeded: more than 2 x 2048 records and more than 2048 tiles of stream"""
    rng = random.Random(24)
    refs = [(b"one", 3_000_000), (b"two", 500_000)]
    recs = [sized(k % 2, rng.randrange(refs[k % 2][1] - 100), b"m%d" % k, 1900 + rng.randrange(400), span=1 + rng.randrange(60))
            for k in range(5000)]
    return refs, recs


def test_more_tiles_and_more_records_than_one_tile_of_the_exclusive_scan(ctx, many_records):
    """both exclusive scans -- of the scan's per-tile counts and of the sorted sizes -- run over more than two of their own
    tiles of 2048 elements"""
    refs, recs = many_records
    assert len(recs) > 2 * 2048 and sum(len(r) for r in recs) > 2048 * TILE
    check(ctx, refs, recs, sizes=[65280])


# ---------------------------------------------------------------- keys and order
def test_keys_wider_than_one_digit(ctx):
    """70 000 references, records on refIDs 0, 255, 256, 65 535, 65 536 and 69 999 with empty references between them; the
    last reference is 2 000 000 000 long (depth 6) and holds positions on both sides of bits 24, 29 and 30"""
    refs = [(b"s%d" % k, 1000 + k) for k in range(69_999)] + [(b"long", 2_000_000_000)]
    recs = []
    for k, r in enumerate([65_536, 0, 69_999, 255, 65_535, 256, 0, 255]):
        recs.append(sized(r, 500 - k if r < 69_999 else 77, b"n%d" % k, 70 + k))
    for k, pos in enumerate([1_999_999_000, 1 << 24, 0, (1 << 30) + 5, (1 << 24) - 1, 1 << 29]):
        recs.append(sized(69_999, pos, b"p%d" % k, 90 + k, span=900))
    bam, _, index = check(ctx, refs, recs)
    assert index["depth"] == 6
    got = [M.fields(r)[:2] for r in M.split_stream(M.inflate(bam))[4]]
    assert got == sorted(got) and got[-1] == (69_999, 1_999_999_000)


def test_ties_keep_input_order(ctx):
    refs = [(b"ref", 100_000)]
    recs = [sized(0, 4242, b"t%04d" % ((k * 389) % 1000), 48 + k % 50) for k in range(1000)]
    recs.insert(500, sized(0, 4241, b"before", 60))
    bam, _, _ = check(ctx, refs, recs)
    names = [M.name_of(r) for r in M.split_stream(M.inflate(bam))[4]]
    assert names == [b"before"] + [b"t%04d" % ((k * 389) % 1000) for k in range(1000)]


# ---------------------------------------------------------------- sizes
def test_no_record_and_one_record(ctx):
    refs = [(b"a", 1000), (b"b", 2000)]
    _, _, index = check(ctx, refs, [])
    assert index["refs"] == [{}, {}]
    check(ctx, refs, [sized(1, 5, b"only", 61)])
    check(ctx, [], [], text=b"@CO\tno @HD line here\n")          # (and the @HD line is put in front)


def test_every_source_and_destination_residue(ctx):
    """record sizes 45 .. 108 in a shuffled order: every source and every destination offset mod 16, in both the vector and
    the byte-wise path of the gather (records shorter and longer than a few vectors)"""
    refs = [(b"ref", 1_000_000)]
    rng = random.Random(16)
    recs = [sized(0, rng.randrange(900_000), b"z%d" % k, 45 + (k * 37) % 64) for k in range(640)]
    recs += [sized(0, rng.randrange(900_000), b"big%d" % k, 5000 + 17 * k) for k in range(48)]
    rng.shuffle(recs)
    check(ctx, refs, recs)


def test_one_huge_record_among_small_ones(ctx):
    """a 1 000 000-base read (about 1.5 MB) among records of 40-base reads"""
    refs = [(b"ref", 3_000_000)]
    rng = random.Random(4)
    seq = bytes(rng.randrange(256) for _ in range(4096)) * 123
    big = M.record(0, 1_500_000, b"huge", [(1_000_000, "M")], 1_000_000, seq=seq[:500_000], qual=bytes(range(40)) * 25_000,
                   aux=b"NMI" + struct.pack("<I", 7))
    small = [M.record(0, rng.randrange(2_999_000), b"s%d" % k, [(40, "M")], 40, seq=bytes([17 * (k % 15)]) * 20, qual=bytes(40))
             for k in range(3000)]
    recs = small[:1700] + [big] + small[1700:]
    check(ctx, refs, recs)


# ---------------------------------------------------------------- CIGARs and bins
def test_cg_tag_record_ends_where_its_n_says(ctx):
    refs = [(b"ref", 400_000)]
    runs = struct.pack("<70000I", *([(3 << 4)] * 70_000))
    cg = M.record(0, 1000, b"cg", [(250_000, "S"), (210_000, "N")], 250_000, aux=b"NMI" + struct.pack("<I", 9) + b"CGBI" +
                  struct.pack("<I", 70_000) + runs)
    assert M.fields(cg) == (0, 1000, 211_000)
    recs = [sized(0, 150_000, b"mid", 99, span=10), cg, sized(0, 20, b"first", 64, span=5)]
    _, _, index = check(ctx, refs, recs)
    assert M.reg2bin(1000, 211_000) in index["refs"][0]


def test_bins_at_every_level(ctx):
    refs = [(b"ref", 300_000_000)]
    spans = [(100, 50), ((1 << 14) - 5, 10), ((1 << 17) - 5, 10), ((1 << 20) - 5, 10), ((1 << 23) - 5, 10), ((1 << 26) - 5, 10),
             (1000, 200_000_000), (120, 30), ((1 << 14) + 1, 3)]
    recs = [sized(0, p, b"b%d" % k, 70 + 3 * k, span=s) for k, (p, s) in enumerate(spans)]
    _, _, index = check(ctx, refs, recs[::-1])
    assert {4681, 4682, 585, 73, 9, 1, 0} <= set(index["refs"][0])


# ---------------------------------------------------------------- through the command line
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def _run(cmd, workdir, ok=True):
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=workdir, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr[-4000:]
    return r


def _cli(args, workdir, extra=()):
    import pbsim3_amd.build as b
    b.build()
    os.makedirs(workdir, exist_ok=True)
    r = _run([CLI] + harness.resolve(args) + ["--prefix", os.path.join(workdir, "out")] + list(extra), workdir)
    files = {}
    for n in sorted(os.listdir(workdir)):
        if n.startswith("out"):
            with open(os.path.join(workdir, n), "rb") as f:
                files[n[3:]] = f.read()
    return files, harness.strip_report(r.stderr)


@pytest.mark.parametrize("case", ["wgs_errhmm-ont_quirk", "wgs_qshmm_rsii_pass3", "trans_errhmm_sequel", "wgs_sample_plain"])
def test_cli_sorts_and_indexes_its_own_files(case, tmp_path):
    args = CASES[case]["args"]
    plain, err_plain = _cli(args, str(tmp_path / "u"), extra=("--truth-format", "bam"))
    srt, err_srt = _cli(args, str(tmp_path / "s"), extra=("--truth-format", "bam", "--truth-sort", "coordinate"))
    assert err_srt == err_plain
    alns = [n for n in plain if n.endswith(".aln.bam")]
    assert alns and sorted(srt) == sorted(list(plain) + [n + ".csi" for n in alns])       # no .tmp, one index per file
    for n in plain:
        if n not in alns:
            assert srt[n] == plain[n], n               # read files, .ref
    for n in alns:
        head, l_text, text, refs, recs = M.split_stream(M.inflate(plain[n]))
        table = M.members(srt[n])
        new_head, new_l_text, new_text, new_refs, got = M.split_stream(b"".join(t for _, _, t in table))
        # the header differs only in SO: (and in the l_text that counts it); the reference list after the text is verbatim
        assert text.count(b"SO:unknown") == 1 and new_text == text.replace(b"SO:unknown", b"SO:coordinate")
        assert new_l_text == len(new_text) and new_head[8 + new_l_text:] == head[8 + l_text:]
        assert new_head == M.sorted_header(head)
        assert new_refs == refs and sorted(got) == sorted(recs)
        want = M.stable_sort(recs)
        assert got == want
        if "pass3" in case:        # the passes of one read share a position: ties the product makes itself
            keys = [M.fields(r)[:2] for r in want]
            assert len(set(keys)) < len(keys)
        csi_text = M.inflate(srt[n + ".csi"])
        assert csi_text == M.csi_bytes(refs, want, len(new_head), [(c, len(t)) for c, _, t in table])
        index = M.read_csi(csi_text)
        for ref, beg, end in queries(refs, want, 1):
            assert M.query(index, srt[n], ref, beg, end, table) == M.brute(want, ref, beg, end), (n, ref, beg, end)
    # the standalone mode on the unsorted files: the same two files
    names = [str(tmp_path / "u" / ("out" + n)) for n in alns]
    _run([CLI, "--sort-truth-bam"] + names, str(tmp_path / "u"))
    left = sorted(os.listdir(tmp_path / "u"))
    assert left == sorted(os.listdir(tmp_path / "s"))
    for n in alns:
        for m in (n, n + ".csi"):
            with open(tmp_path / "u" / ("out" + m), "rb") as f:
                assert f.read() == srt[m], m


def test_cli_refuses_what_it_cannot_do(tmp_path):
    args = harness.resolve(CASES["wgs_errhmm-ont_quirk"]["args"]) + ["--prefix", str(tmp_path / "out")]
    r = _run([CLI] + args + ["--truth-format", "bam", "--truth-sort", "coordinate", "--devices", "0,0"], str(tmp_path), ok=False)
    assert "--sort-truth-bam" in r.stderr and not os.listdir(tmp_path)
    r = _run([CLI] + args + ["--truth-sort", "coordinate"], str(tmp_path), ok=False)
    assert "--truth-format bam" in r.stderr
    r = _run([CLI] + args + ["--truth-format", "bam", "--truth-sort", "name"], str(tmp_path), ok=False)
    assert "coordinate" in r.stderr
    # a file that is no truth BAM: it stays as it is, nothing is left beside it, and the exit status says so
    bad = tmp_path / "bad.aln.bam"
    bad.write_bytes(framed(M.header([(b"ref", 1000)]) + b"\0" * 80))
    before = bad.read_bytes()
    r = _run([CLI, "--sort-truth-bam", str(bad)], str(tmp_path), ok=False)
    assert "offset" in r.stderr and bad.read_bytes() == before and sorted(os.listdir(tmp_path)) == ["bad.aln.bam"]
