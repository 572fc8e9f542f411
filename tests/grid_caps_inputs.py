"""The inputs of test_gpu_sample_grid_caps.py and test_gpu_inflate_grid_caps.py, which take the strided loops of the sample
profile builders (sample_profile.hip, sample_bam.hip), of the inflate (inflate.hip) and of the scan (kernels.hip: k_scan_single)
into a second trip, and the facts about them that need no device; test_grid_caps_inputs.py checks those facts where there is no
GPU.  Every size comes from the caps as the sources state them.

    f1()      FASTQ: more records than one trip of the pool pass takes
    f2()      FASTQ: more records than one trip of the scan's middle kernel takes
    f3(rest)  FASTQ: more tiles than one trip of the count takes, (number of tiles) mod kCountUnroll = rest
    f4()      FASTQ: two windows of more tiles than one trip of the line pass takes, the second behind a carry
    b1()      BAM: more chain records than one trip of the pool pass takes
    i1()      BGZF: more members than one launch of the inflate has workgroups;  i2(kind): one of them damaged
"""
import functools
import os
import random
import re
import types
import zlib

import bam_writer as B
import bgzf_writer as W
from test_gpu_bam_grid_caps import CSRC, constant
from test_gpu_inflate import CL_ORDER, canonical
from test_gpu_sample_profile import host

TILE = constant("kernels.h", "kSpTile")
UNROLL = constant("sample_profile.hip", "kCountUnroll")
WAVES_PER_BLOCK = 4                                         # (the workgroups of these passes have 256 threads)
WAVE_CAP = constant("kernels.h", "kSpBlocksMax") * WAVES_PER_BLOCK    # the tiles or records of one trip of a line or pool pass
COUNT_CAP = WAVE_CAP * UNROLL                               # the tiles of one trip of the count
SCAN_CAP = constant("kernels.hip", "kScanBlock") * constant("kernels.hip", "kScanTile")     # the elements of one trip of k_scan_single
MEMBER_CAP = constant("inflate.hip", "kInflateBlocksMax")   # the members of one trip of k_inflate
LF = 10


def carry_room():
    """kCarryRoom, a `constexpr int64_t a << b`: the first window of a FASTQ begins there in its buffer"""
    with open(os.path.join(CSRC, "sample_profile.cpp")) as f:
        found = re.findall(r"constexpr int64_t kCarryRoom = (\d+) << (\d+);", f.read())
    assert len(found) == 1, "%d definitions of kCarryRoom" % len(found)
    return int(found[0][0]) << int(found[0][1])


def default_piece_bytes():
    """the output (and input) bytes that one piece of an inflate holds when PBSIM_INFLATE_PIECE_KB is not set"""
    with open(os.path.join(CSRC, "inflate_host.cpp")) as f:
        found = re.findall(r"atoll\(e\) : \(int64_t\)(\d+) << 10;", f.read())
    assert len(found) == 1, "%d defaults of the piece size" % len(found)
    return int(found[0]) << 20


def tiles_of(n_bytes):
    """the tiles of a first window of n_bytes (it begins on a tile's edge: kCarryRoom is a multiple of kSpTile)"""
    return -(-n_bytes // TILE)


# ---------------------------------------------------------------- FASTQ
FRONT, BEHIND, LOW = range(5, 25), range(26, 46), range(0, 3)   # phred values: in front of a seam, behind it, and too bad to keep
SHORT = dict(len_min=28, len_max=92, acc_min=0.5, acc_max=1.0)      # of lines of 20 .. 100: drops some at both ends
DEFAULT = dict(len_min=100, len_max=1_000_000, acc_min=0.75, acc_max=1.0)
DENSE = dict(len_min=12, len_max=5000, acc_min=0.5, acc_max=1.0)    # keeps most dense records and no filler line of 100 000
CARRY = dict(len_min=12, len_max=70_000, acc_min=0.5, acc_max=1.0)  # keeps the carried line of f4() as well
FILL = 100_000


def chars(r, n, palette):
    return bytes(33 + r.choice(palette) for _ in range(n))


class Fastq:
    """records one behind the other; `at`: the file offset of the next, `quals`: (offset, line) of every quality line"""

    def __init__(self, seed):
        self.r, self.parts, self.at, self.quals = random.Random(seed), [], 0, []
        self.fill = chars(self.r, 1000, range(10, 41)) * (FILL // 1000)

    def add(self, head, bases, qual):
        self.quals.append((self.at + len(head) + len(bases) + 4, qual))
        self.parts += [head, b"\n", bases, b"\n+\n", qual, b"\n"]
        self.at += len(head) + len(bases) + len(qual) + 5

    def dense(self, upto, palette=FRONT):
        """records of about 60 bytes until the next one begins at `upto` or behind it: a tile holds every line phase many times"""
        r = self.r
        while self.at < upto:
            n = len(self.quals)
            pal = LOW if n % 29 == 3 else palette
            self.add(b"@d%d" % (n % 1000), b"ACGTTGCATGCA"[:3 + n % 10], chars(r, 8 + (n * 7 + r.randrange(3)) % 33, pal))

    def filler(self, upto):
        """lines of FILL characters, then a shorter one that ends the record at `upto` (or up to 8 bytes in front of it)"""
        while self.at + FILL + 8 <= upto:
            self.add(b"@f", b"A", self.fill)
        if upto - self.at > 8:
            self.add(b"@f", b"A", self.fill[:upto - self.at - 8])

    def seam(self, at, style, palette=BEHIND):
        """dense records up to file offset `at`, the first byte of a tile, and over it: a quality line straddles it, a record's
        fourth line feed is that byte, or a header line straddles it; the records from there on of another palette"""
        self.dense(at - 300)
        gap = at - self.at
        assert 230 < gap <= 300
        if style == "straddle":
            self.add(b"@s", b"ACGT", chars(self.r, 2 * (gap - 10) + 1, palette))
        elif style == "fourth_lf":
            self.add(b"@s", b"ACGT", chars(self.r, gap - 10, palette))
            assert self.at == at + 1
        else:
            assert style == "header"
            self.add(b"@" + b"h" * (gap + 40), b"ACGT", chars(self.r, 60, palette))
        assert self.at > at

    def end(self, length, palette=BEHIND):
        """dense records, the last one cut so that the file has `length` bytes"""
        self.dense(length - 200, palette)
        assert 100 < length - self.at <= 200
        self.add(b"@e", b"ACGT", chars(self.r, length - self.at - 11, palette))
        assert self.at == length
        return b"".join(self.parts)


def line_at(fq, at):
    """(the line feeds in front of byte `at`) mod 4 -- 3: `at` lies in a quality line or is its line feed -- and whether the byte is a line feed"""
    return fq.count(b"\n", 0, at) % 4, fq[at] == LF


@functools.lru_cache(maxsize=None)
def f1():
    """WAVE_CAP + 700 records: quality lines of 20 .. 100 characters, headers and base lines of varying lengths; from record
    WAVE_CAP - 4 on another palette; records WAVE_CAP - 1 and WAVE_CAP have lengths that the filter keeps"""
    f = Fastq(WAVE_CAP)
    r = f.r
    for i in range(WAVE_CAP + 700):
        n = {WAVE_CAP - 1: 57, WAVE_CAP: 64}.get(i, 20 + (i * 37 + r.randrange(3)) % 81)
        pal = BEHIND if i >= WAVE_CAP - 4 else LOW if i % 53 == 7 else FRONT
        f.add(b"@%d" % i + b"/1" * (i % 4), b"ACGTTGCAACGTGGCC"[:1 + r.randrange(16)], chars(r, n, pal))
    return types.SimpleNamespace(fq=b"".join(f.parts), quals=f.quals, filter=SHORT, seam=WAVE_CAP)


@functools.lru_cache(maxsize=None)
def f2():
    """SCAN_CAP + 3000 records, most of them four line feeds (a record of length 0); sixty that the filter keeps in front of
    record SCAN_CAP - 1, that record and the next, and forty behind them.  `kept`: index -> quality line"""
    r = random.Random(SCAN_CAP)
    n = SCAN_CAP + 3000
    where = sorted(set(r.sample(range(SCAN_CAP - 1), 60)) | {SCAN_CAP - 1, SCAN_CAP} | set(r.sample(range(SCAN_CAP + 1, n), 40)))
    parts, kept, prev = [], {}, 0
    for k in where:
        kept[k] = chars(r, 100 + r.randrange(200), FRONT if k < SCAN_CAP - 4 else BEHIND)
        parts += [b"\n\n\n\n" * (k - prev), b"@k%d\nACGT\n+\n" % k, kept[k], b"\n"]
        prev = k + 1
    parts.append(b"\n\n\n\n" * (n - prev))
    return types.SimpleNamespace(fq=b"".join(parts), kept=kept, records=n, filter=DEFAULT, seam=SCAN_CAP)


F3_STYLES = {0: "straddle", 1: "fourth_lf", 3: "header"}    # (tiles mod kCountUnroll) -> what lies over both seams


@functools.lru_cache(maxsize=1)                             # (64 MiB each)
def f3(rest):
    """COUNT_CAP + 12 + rest tiles, the last one of 517 bytes: filler lines but for dense records on the eight tiles either side
    of tile WAVE_CAP (the line pass's seam) and of tile COUNT_CAP (the count's), and from there to the end of the file"""
    n_tiles = COUNT_CAP + 3 * UNROLL + rest
    assert n_tiles % UNROLL == rest
    f = Fastq(COUNT_CAP + rest)
    seams = [WAVE_CAP * TILE, COUNT_CAP * TILE]
    for s in seams:
        f.filler(s - 8 * TILE)
        f.seam(s, F3_STYLES[rest])
        f.dense(s + 8 * TILE, BEHIND)
    fq = f.end((n_tiles - 1) * TILE + 517)
    return types.SimpleNamespace(fq=fq, quals=f.quals, filter=DENSE, seams=seams, style=F3_STYLES[rest], tiles=n_tiles)


@functools.lru_cache(maxsize=None)
def f4():
    """two windows of `chunk` = (WAVE_CAP + 64) tiles and a little less: the first ends `carry` bytes into a quality line of odd
    length, which the filter keeps; dense records around the first window's tile WAVE_CAP and around the second's, whose tiles
    begin kSpTile - carry % kSpTile bytes in front of the carried line"""
    chunk, carry, line = (WAVE_CAP + 64) * TILE, 33_333, 66_667
    assert carry % TILE and line % 2 and carry < line < CARRY["len_max"] < FILL
    f = Fastq(WAVE_CAP + 4)
    f.filler(WAVE_CAP * TILE - 8 * TILE)
    f.seam(WAVE_CAP * TILE, "straddle")
    f.dense(WAVE_CAP * TILE + 8 * TILE, BEHIND)
    f.filler(chunk - carry - 10)
    assert f.at == chunk - carry - 10
    f.add(b"@c", b"ACGT", chars(f.r, line, FRONT))
    assert f.quals[-1][0] == chunk - carry
    # the second window's buffer begins at kCarryRoom - carry, its tiles at the tile's edge below: tile WAVE_CAP of them is at
    seam = chunk - -(-carry // TILE) * TILE + WAVE_CAP * TILE
    f.filler(seam - 8 * TILE)
    f.seam(seam, "straddle", FRONT)
    f.dense(seam + 8 * TILE, FRONT)
    fq = f.end(seam + 12 * TILE + 333, FRONT)
    assert chunk < len(fq) <= 2 * chunk
    return types.SimpleNamespace(fq=fq, quals=f.quals, filter=CARRY, chunk=chunk, carry=carry, seams=[WAVE_CAP * TILE, seam],
                                 tiles=[tiles_of(chunk), -(-(-(-carry // TILE) * TILE + len(fq) - chunk) // TILE)])


def kept_by_length(quals, flt):
    return [(at, q) for at, q in quals if flt["len_min"] <= len(q) <= flt["len_max"]]


_WANT = {}


def stdio(driver, tmp_path, name, fq, flt):
    """the stdio parse of input `name` (test_gpu_sample_profile.host), worked out once and left unchanged"""
    if name not in _WANT:
        _WANT[name] = host(driver, tmp_path, fq, flt)
        for left in ("host_in.fastq", "host_kept"):             # (tens of MiB that nothing reads again)
            (tmp_path / left).unlink(missing_ok=True)
    return _WANT[name]


# ---------------------------------------------------------------- BAM
B1_REFS = [("chr1", 1_000_000)]
B1_FLAGS = [0, 0x10, 4, 0x100, 0x800, 0x810]
WIDE = [0, 93, 94, 254, 10, 20, 30]                         # (phred values beyond the FASTQ's alphabet: min(q, 93) + 33)


@functools.lru_cache(maxsize=None)
def b1():
    """WAVE_CAP + 700 records, l_seq 20 .. 100, names of varying lengths, the flags of B1_FLAGS mixed; every fifth of the records
    that `samtools fastq` leaves out has no qualities; from record WAVE_CAP - 4 on another palette; records WAVE_CAP - 2 .. WAVE_CAP + 1
    are forward, reverse, forward, reverse and of lengths that the filter keeps"""
    r = random.Random(WAVE_CAP + 1)
    seam = {WAVE_CAP - 2: (0, 41), WAVE_CAP - 1: (0x10, 57), WAVE_CAP: (0, 64), WAVE_CAP + 1: (0x10, 83)}
    recs = []
    for i in range(WAVE_CAP + 700):
        flag, n = seam.get(i, (B1_FLAGS[r.randrange(6)], 20 + (i * 37 + r.randrange(3)) % 81))
        pal = BEHIND if i >= WAVE_CAP - 4 else LOW if i % 53 == 7 else WIDE if i % 17 == 3 else FRONT
        q = bytes([255]) * n if flag & 0x900 and i % 5 == 0 else bytes(r.choice(pal) for _ in range(n))
        mapped = not flag & 4
        recs.append(B.record("r%d" % i + "/x" * (i % 6), flag, ref_id=0 if mapped else -1, pos=i if mapped else -1,
                             cigar=((n, "M"),) if mapped else (), qual=q, mapq=i % 61, tags=[("NM", "i", i)] if i % 3 == 0 else []))
    return types.SimpleNamespace(recs=recs, stream=B.stream(recs, B1_REFS), fq=B.to_fastq(recs), filter=SHORT, seam=WAVE_CAP)


def fastq_line(rec):
    """the quality line of a record's read in the FASTQ"""
    q = rec["qual"][::-1] if rec["flag"] & 0x10 else rec["qual"]
    return bytes(min(x, 93) + 33 for x in q)


# ---------------------------------------------------------------- BGZF
KINDS = ("stored", "fixed", "dynamic")                      # by BTYPE (RFC 1951 3.2.3)
DEEP_AT = (5, 11, 17)                                       # dynamic members of deep_text(), each with a fixed one behind it on its workgroup


def deep_text():
    """15 symbols of 2^14, 2^13 .. 1 occurrences, shuffled: with the end of the block, a Huffman code of the lengths 1 .. 15.
    (zlib gives test_gpu_deflate.fib_skew() a literal code of the lengths 3 .. 13 only: its 32 KiB are a cut of the whole text.)"""
    s = list(b"".join(bytes([65 + k]) * (1 << (14 - k)) for k in range(15)))
    random.Random(15).shuffle(s)
    return bytes(s)


def kind_of(m):
    """the kind of member m: m and m + MEMBER_CAP differ, and the workgroups that take two trips see every ordered pair"""
    if m < MEMBER_CAP:
        return m % 3
    w = m - MEMBER_CAP
    return (w % 3 + 1 + (w // 3) % 2) % 3


def deflate_as(kind, text):
    if kind == "stored":
        return W.raw_deflate(text, level=0)
    if kind == "deep":                                      # (literals only, and a block that holds all of them: the counts are the text's)
        return W.raw_deflate(text, level=9, strategy=zlib.Z_HUFFMAN_ONLY, mem_level=9)
    return W.raw_deflate(text, level=9, strategy=zlib.Z_FIXED if kind == "fixed" else zlib.Z_DEFAULT_STRATEGY)


def block_kind(cdata):
    """BTYPE of the first block of a deflate stream"""
    return (cdata[0] >> 1) & 3


def literal_lengths(cdata):
    """the code lengths of the literal/length code of a deflate stream's first block, a dynamic one (RFC 1951 3.2.7)"""
    bits, at = int.from_bytes(cdata[:600], "little"), 0

    def take(n):
        nonlocal at
        v = (bits >> at) & ((1 << n) - 1)
        at += n
        return v

    take(1)
    assert take(2) == 2
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = take(3)
    codes = {pair: s for s, pair in canonical(cl).items()}
    lens = []
    while len(lens) < hlit + hdist:
        code, ln = take(1), 1
        while (code, ln) not in codes:
            code, ln = code << 1 | take(1), ln + 1
            assert ln <= 7
        s = codes[(code, ln)]
        lens += [s] if s < 16 else [lens[-1]] * (3 + take(2)) if s == 16 else [0] * (3 + take(3)) if s == 17 else [0] * (11 + take(7))
    assert at <= 8 * min(len(cdata), 600) and len(lens) == hlit + hdist
    return lens[:hlit]


@functools.lru_cache(maxsize=None)
def i1():
    """MEMBER_CAP + 700 members of 1 .. 300 bytes (and three of 32 KiB, DEEP_AT), empty ones at MEMBER_CAP - 1 and MEMBER_CAP.
    `offsets`: where each member begins (and the end); `cdata`, `texts`: every member's deflate data and bytes"""
    r = random.Random(MEMBER_CAP)
    n = MEMBER_CAP + 700
    words = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"a", b"lazy", b"dog", b"ACGTACGT", b"@read/1", b"+", b"!!!!"]
    texts, cdata = [], []
    for m in range(n):
        kind = KINDS[kind_of(m)]
        size = 1 + (m * 7 + r.randrange(5)) % 300
        if m in (MEMBER_CAP - 1, MEMBER_CAP):
            text, kind = b"", "fixed" if kind == "dynamic" else kind        # (zlib writes no dynamic block for nothing)
        elif kind == "dynamic":                                             # few symbols, many of each: the dynamic block is the smallest
            text, kind = (deep_text(), "deep") if m in DEEP_AT else (bytes(r.choice(b"ACGT") for _ in range(max(size, 120))), kind)
        else:
            text = b" ".join(r.choice(words) for _ in range(size // 3 + 1))[:size]
        texts.append(text)
        cdata.append(deflate_as(kind, text))
    members = [W.member(t, cdata=c) for t, c in zip(texts, cdata)]
    offsets = [0]
    for mem in members:
        offsets.append(offsets[-1] + len(mem))
    return types.SimpleNamespace(z=b"".join(members), want=b"".join(texts), offsets=offsets, cdata=cdata, texts=texts, members=n)


DAMAGE = {"crc": ("fixed", "incorrect data check"), "truncated": ("dynamic", "unexpected end")}    # test_gpu_inflate.malformed()'s


@functools.lru_cache(maxsize=None)
def i2(damage):
    """(i1()'s stream with one member of the second trip damaged, that member's index, the reason of the refusal): a wrong CRC
    on a fixed-code member, or a dynamic member's deflate data cut in half"""
    s = i1()
    kind, reason = DAMAGE[damage]
    m = next(m for m in range(MEMBER_CAP + 40, s.members) if KINDS[block_kind(s.cdata[m])] == kind)
    if damage == "crc":
        bad = W.member(s.texts[m], cdata=s.cdata[m], crc=(zlib.crc32(s.texts[m]) ^ 1) & 0xffffffff)
    else:
        bad = W.member(s.texts[m], cdata=s.cdata[m][:len(s.cdata[m]) // 2])
    return s.z[:s.offsets[m]] + bad + s.z[s.offsets[m + 1]:], m, reason
