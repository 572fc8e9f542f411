"""The GPU inflate of BGZF members (pbsim3_amd/csrc/inflate.hip) against zlib, byte for byte, over block types, levels,
strategies and edge cases; and malformed members, one at a time: each is refused with the member's offset, and the
context goes on working."""
import os
import random
import struct
import zlib

import pytest

import bgzf_writer as W
import harness
import pbsim3_amd as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(), 0) as c:
        yield c


def fasta(n, seed=1):
    bases = harness.synth_bases(n, seed).tobytes()
    lines = [bases[i:i + 60] for i in range(0, len(bases), 60)]
    return b">chr1 synthetic\n" + b"\n".join(lines) + b"\n"


def check(ctx, d, **kw):
    z = W.bgzf(d, **kw)
    assert P.inflate_bound(z) == len(d)
    got = ctx.inflate_buffer(z)
    assert got == d, next((i for i, (a, b) in enumerate(zip(got, d)) if a != b), min(len(got), len(d)))


@pytest.mark.parametrize("level", range(10))
def test_levels(ctx, level):
    check(ctx, fasta(300000, level), level=level)


@pytest.mark.parametrize("strategy", [zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED])
def test_strategies(ctx, strategy):
    check(ctx, fasta(200000, 7) + b"A" * 5000 + bytes(range(256)) * 40, strategy=strategy)


def test_many_blocks_per_member(ctx):
    check(ctx, fasta(400000, 3) + os.urandom(70000), mem_level=1, level=9)


def test_random_data_stored_blocks(ctx):
    check(ctx, random.Random(5).randbytes(500000))


def test_runs_of_one_byte(ctx):
    check(ctx, b"N" * 300000 + b"\x00" * 70000 + b"AC" * 40000)


def test_distance_32768(ctx):
    blk = random.Random(9).randbytes(32768)
    check(ctx, blk + blk[:20000] + blk + blk, block=65536)


def test_empty_members_and_sizes(ctx):
    assert ctx.inflate_buffer(W.EOF_MARKER) == b""
    assert ctx.inflate_buffer(b"") == b""
    z = W.member(b"") + W.member(b"x") + W.member(b"") + W.member(b"hello" * 100) + W.EOF_MARKER
    assert ctx.inflate_buffer(z) == b"x" + b"hello" * 100
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 1000, 65279, 65280, 65281, 65536):
        check(ctx, fasta(n, n)[:n], block=65536)
    d = b"".join(fasta(random.Random(i).randrange(0, 3000), i) for i in range(3000))
    check(ctx, d, block=997)                                  # a few thousand members of odd sizes


def test_deflate_round_trip(ctx):
    d = fasta(1 << 20, 11) + b"@r1\nACGT\n+\n!!!!\n" * 5000
    z = ctx.deflate_buffer(d)
    assert ctx.inflate_buffer(z) == d


def test_pieces(ctx, tmp_path):
    """several pieces through the two buffer sets (PBSIM_INFLATE_PIECE_KB: 64 KiB pieces), in a child process"""
    import subprocess
    import sys
    d = fasta(3 << 20, 13)
    (tmp_path / "in.gz").write_bytes(W.bgzf(d))
    code = ("import sys, pbsim3_amd as P\n"
            "with P.Context(P.default_params(), 0) as c:\n"
            "    sys.stdout.buffer.write(c.inflate_buffer(open(sys.argv[1], 'rb').read()))\n")
    env = dict(os.environ, PBSIM_INFLATE_PIECE_KB="64")
    p = subprocess.run([sys.executable, "-c", code, str(tmp_path / "in.gz")], capture_output=True, env=env, timeout=300,
                       cwd=harness.ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout == d


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, val, n):
        self.v |= (val & ((1 << n) - 1)) << self.n
        self.n += n

    def put_rev(self, code, n):        # a Huffman code, most significant bit first
        for i in range(n - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def fixed_lit(b, sym):
    if sym < 144:
        b.put_rev(0x30 + sym, 8)
    elif sym < 256:
        b.put_rev(0x190 + sym - 144, 9)
    elif sym < 280:
        b.put_rev(sym - 256, 7)
    else:
        b.put_rev(0xc0 + sym - 280, 8)


def malformed(kind):
    good = fasta(5000, 2)
    if kind == "crc":
        return W.member(good, crc=(zlib.crc32(good) ^ 1) & 0xffffffff), "incorrect data check"
    if kind == "isize":
        return W.member(good, isize=len(good) + 1), "incorrect length check"
    if kind == "truncated":
        c = W.raw_deflate(good)
        return W.member(good, cdata=c[:len(c) // 2]), "unexpected end"
    if kind == "oversubscribed":       # dynamic block whose code-length code has three codes of one bit
        b = Bits()
        b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(0, 4)
        for ln in (1, 1, 1, 0):
            b.put(ln, 3)
        return W.member(b"ab", cdata=b.bytes() + b"\x00" * 8), "invalid code lengths set"
    if kind == "too_far":             # fixed block: literal 'a', then a match of length 3 at distance 2
        b = Bits()
        b.put(1, 1), b.put(1, 2)
        fixed_lit(b, ord("a"))
        fixed_lit(b, 257)               # length 3
        b.put_rev(1, 5)                 # distance code 1: distance 2
        fixed_lit(b, 256)
        return W.member(b"aaaa", cdata=b.bytes()), "invalid distance too far back"
    if kind == "nlen":
        c = bytes([1]) + struct.pack("<HH", 4, 0x1234) + b"abcd"
        return W.member(b"abcd", cdata=c), "invalid stored block lengths"
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["crc", "isize", "truncated", "oversubscribed", "too_far", "nlen"])
def test_malformed_member(ctx, kind):
    pre = W.bgzf(fasta(150000, 4), eof=False)
    bad, reason = malformed(kind)
    z = pre + bad + W.bgzf(fasta(70000, 5))
    with pytest.raises(P.PbsimError, match=f"gzip member at byte offset {len(pre)}: .*{reason}"):
        ctx.inflate_buffer(z)
    # the context is still good: a buffer inflates, and a simulation runs
    d = fasta(100000, 6)
    assert ctx.inflate_buffer(W.bgzf(d)) == d


def test_simulation_after_refusals(ctx):
    with pytest.raises(P.PbsimError):
        ctx.inflate_buffer(W.member(b"abc", crc=0))
    ctx.load_errhmm(harness.model_path("ERRHMM-ONT.model"))
    ctx.set_reference(harness.synth_bases(20000, 3).tobytes(), 1)
    reads, _ = ctx.simulate_wgs()
    assert reads.startswith(b"@")


# ---- hand-encoded blocks: what zlib's encoder never writes
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def canonical(lens):
    """symbol -> (code, length) of the canonical code with these lengths (RFC 1951 3.2.2)"""
    count = [0] * 16
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for ln in range(1, 16):
        code = (code + count[ln - 1]) << 1
        nxt[ln] = code
    out = {}
    for s, ln in enumerate(lens):
        if ln:
            out[s] = (nxt[ln], ln)
            nxt[ln] += 1
    return out


def dynamic_header(b, lit_lens, dist_lens, hlit=None, first_cl=None):
    """BFINAL=1, BTYPE=2 and the code lengths, through a code-length code that gives 0..15 four bits each"""
    b.put(1, 1), b.put(2, 2)
    b.put((hlit or len(lit_lens)) - 257, 5), b.put(len(dist_lens) - 1, 5), b.put(19 - 4, 4)
    cl = [4] * 16 + [0, 0, 0] if first_cl is None else first_cl
    for s in CL_ORDER:
        b.put(cl[s], 3)
    codes = canonical(cl)
    for ln in lit_lens + dist_lens:
        b.put_rev(*codes[ln])
    return canonical(lit_lens), canonical(dist_lens)


def lits(b, codes, data):
    for x in data:
        b.put_rev(*codes[x])


def lens_of(pairs, n):
    out = [0] * n
    for s, ln in pairs.items():
        out[s] = ln
    return out


def test_match_at_distance_32768(ctx):
    """32768 literals, then a match of 258 at distance 32768 (distance code 29, extra bits 8191), fixed codes"""
    data = random.Random(12).randbytes(32768)
    b = Bits()
    b.put(1, 1), b.put(1, 2)
    for x in data:
        fixed_lit(b, x)
    fixed_lit(b, 285)                 # length 258
    b.put_rev(29, 5)
    b.put(8191, 13)                   # 24577 + 8191 = 32768
    fixed_lit(b, 256)
    want = data + data[:258]
    assert ctx.inflate_buffer(W.member(want, cdata=b.bytes())) == want


def test_block_without_distance_codes(ctx):
    """HDIST = 1 with length 0: a block of literals (RFC 1951 3.2.7; zlib accepts it) -- and refused where a match needs it"""
    lit = lens_of({ord("a"): 1, ord("b"): 2, 256: 2}, 257)
    b = Bits()
    codes, _ = dynamic_header(b, lit, [0])
    lits(b, codes, b"abba")
    b.put_rev(*codes[256])
    assert ctx.inflate_buffer(W.member(b"abba", cdata=b.bytes())) == b"abba"
    lit = lens_of({ord("a"): 1, 256: 2, 257: 2}, 258)
    b = Bits()
    codes, _ = dynamic_header(b, lit, [0])
    lits(b, codes, b"a")
    b.put_rev(*codes[257])            # a match: no distance code to read
    b.put(0, 16)
    with pytest.raises(P.PbsimError, match="gzip member at byte offset 0: invalid distance code"):
        ctx.inflate_buffer(W.member(b"aaaa", cdata=b.bytes() + b"\x00" * 4))


def refusal(kind):
    b = Bits()
    ok_lit = lens_of({ord("a"): 1, 256: 2, 257: 2}, 258)
    if kind == "lit_oversubscribed":
        dynamic_header(b, lens_of({ord("a"): 1, ord("b"): 1, 256: 1}, 257), [1, 1])
        return b.bytes() + b"\x00" * 4, "invalid literal/lengths set"
    if kind == "lit_incomplete":
        dynamic_header(b, lens_of({ord("a"): 2, 256: 2}, 257), [1, 1])
        return b.bytes() + b"\x00" * 4, "invalid literal/lengths set"
    if kind == "dist_incomplete":
        dynamic_header(b, ok_lit, [2, 2])
        return b.bytes() + b"\x00" * 4, "invalid distances set"
    if kind == "dist_oversubscribed":
        dynamic_header(b, ok_lit, [1, 1, 1])
        return b.bytes() + b"\x00" * 4, "invalid distances set"
    if kind == "block_type_3":
        b.put(1, 1), b.put(3, 2)
        return b.bytes() + b"\x00" * 4, "invalid block type"
    if kind == "hlit_287":
        b.put(1, 1), b.put(2, 2), b.put(30, 5), b.put(0, 5), b.put(0, 4)
        return b.bytes() + b"\x00" * 8, "too many length or distance symbols"
    if kind == "no_end_of_block":
        dynamic_header(b, lens_of({ord("a"): 1, ord("b"): 1}, 257), [1, 1])
        return b.bytes() + b"\x00" * 4, "missing end-of-block"
    if kind == "repeat_first":
        cl = [4] * 15 + [0, 4, 0, 0]      # 0..14 and 16: sixteen codes of four bits
        b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(15, 4)
        for s in CL_ORDER:
            b.put(cl[s], 3)
        b.put_rev(*canonical(cl)[16])
        b.put(0, 2)
        return b.bytes() + b"\x00" * 4, "invalid bit length repeat"
    if kind == "trailing":
        return W.raw_deflate(b"abcd") + b"\x00\x00", "ends before the member's trailer"
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["lit_oversubscribed", "lit_incomplete", "dist_incomplete", "dist_oversubscribed",
                                  "block_type_3", "hlit_287", "no_end_of_block", "repeat_first", "trailing"])
def test_refused_block(ctx, kind):
    cdata, reason = refusal(kind)
    pre = W.bgzf(fasta(70000, 8), eof=False)
    z = pre + W.member(b"abcd", cdata=cdata) + W.EOF_MARKER
    with pytest.raises(P.PbsimError, match=f"gzip member at byte offset {len(pre)}: .*{reason}"):
        ctx.inflate_buffer(z)
    d = fasta(20000, 9)
    assert ctx.inflate_buffer(W.bgzf(d)) == d


def test_hand_encoder_against_zlib():
    """the test's own encoder: what it writes, zlib reads (the refusals above differ from a good block in one thing)"""
    lit = lens_of({ord("a"): 1, ord("b"): 2, 256: 2}, 257)
    b = Bits()
    codes, _ = dynamic_header(b, lit, [1, 1])
    lits(b, codes, b"abba")
    b.put_rev(*codes[256])
    assert zlib.decompress(b.bytes(), -15) == b"abba"
    data = random.Random(12).randbytes(32768)
    b = Bits()
    b.put(1, 1), b.put(1, 2)
    for x in data:
        fixed_lit(b, x)
    fixed_lit(b, 285)
    b.put_rev(29, 5)
    b.put(8191, 13)
    fixed_lit(b, 256)
    assert zlib.decompress(b.bytes(), -15) == data + data[:258]
