"""The sampling method's profile from a BAM (pbsim3_amd/csrc/sample_bam.hip, bam_chain.cpp and the BAM half of
sample_profile.cpp: pbsim_load_sample, pbsim_sample_profile_from_bam_bytes / _from_bam_device) against the profile of the
FASTQ `samtools fastq` would write from it (bam_writer.to_fastq): the host's stdio parse of that FASTQ (all twelve statistics,
doubles by their bits, the kept strings and their order, the error texts) and the GPU's FASTQ builder -- over the lengths at
the seams of the kernels, every alignment of the qualities, both strands, skipped records, decoys inside records, every
container and input form, windows with a seam inside every field, the errors, and through the CLI."""
import os
import random
import shutil
import struct
import subprocess

import pytest

import bam_writer as B
import harness
import pbsim3_amd as P
from cases import CASES

pytestmark = pytest.mark.gpu
CSRC = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")
INPUTS = os.path.join(harness.GOLDEN, "inputs")
MANIFEST = harness.load_manifest()
DEFAULT = dict(len_min=100, len_max=1_000_000, acc_min=0.75, acc_max=1.0)
OTHER = dict(len_min=30, len_max=5000, acc_min=0.5, acc_max=0.97)
INTS = ["num", "len_min", "len_max", "len_total", "num_filtered", "len_min_filtered", "len_max_filtered", "len_total_filtered"]
DOUBLES = ["len_mean_filtered", "len_sd_filtered", "accuracy_mean_filtered", "accuracy_sd_filtered"]
LENGTHS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 99, 100, 101, 4999, 5000, 5001]
REFS3 = [("chr1", 1_000_000), ("chr2_with_a_longer_name", 50_000), ("c", 777)]
TOO_LONG = "fastq is too long. Max acceptable length is 1000000."
GOOD = B.stream([B.record("good", 4, qual=bytes([20]) * 200)])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("drv") / "sample_profile_driver")
    p = subprocess.run([cxx, "-O1", "-std=c++17", "-pthread", "-I", CSRC, os.path.join(harness.ROOT, "tests", "sample_profile_driver.cpp"),
                        os.path.join(CSRC, "unit_io.cpp"), "-o", exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def host(driver, tmp_path, fq, f):
    """(ints, double bits, kept strings) of the stdio parse of a FASTQ, or the error text"""
    path = tmp_path / "host_in.fastq"
    path.write_bytes(fq)
    kept = tmp_path / "host_kept"
    p = subprocess.run([driver, str(path), str(f["len_min"]), str(f["len_max"]), float(f["acc_min"]).hex(), float(f["acc_max"]).hex(),
                        str(kept)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    if p.stdout.startswith("error "):
        return p.stdout[6:].rstrip("\n")
    lines = p.stdout.splitlines()
    return [int(x) for x in lines[0].split()[1:]], [int(x, 16) for x in lines[1].split()[1:]], kept.read_bytes().split(b"\n")[:-1]


def unpack(st, ctx):
    ints = [getattr(st, k) for k in INTS]
    bits = [struct.unpack("<Q", struct.pack("<d", getattr(st, k)))[0] for k in DOUBLES]
    return ints, bits, ctx.sample_profile()


_CONTEXTS = {}


@pytest.fixture(scope="module", autouse=True)
def contexts():
    """one context per length filter for the whole module: every build replaces the profile of the one before"""
    yield
    for ctx in _CONTEXTS.values():
        ctx.close()
    _CONTEXTS.clear()


def context(f):
    key = (f["len_min"], f["len_max"])
    if key not in _CONTEXTS:
        _CONTEXTS[key] = P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_SAMPLE, len_min=f["len_min"],
                                                    len_max=f["len_max"]), 0)
    return _CONTEXTS[key]


FORMS = ["bytes", "device", "bgzf", "bgzf300", "stored", "gzip", "none"]


def gpu(stream, f, chunk=0, form="bytes", tmp_path=None):
    """the profile the GPU builds from the inflated BAM bytes `stream`; `form`: how they reach it (the last five: a file in that
    container through load_sample).  An error comes back as its text, after the context has shown that it still works and
    still holds the profile it had."""
    ctx = context(f)
    ctx.set_sample_chunk_bytes(chunk)
    try:
        before = ctx.sample_profile()
    except P.PbsimError:
        before = None
    try:
        if form == "bytes":
            st = ctx.sample_profile_from_bam(stream, f["acc_min"], f["acc_max"])
        elif form == "device":
            import torch
            t = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda() if stream else torch.empty(0, dtype=torch.uint8, device="cuda")
            st = ctx.sample_profile_from_bam(t, f["acc_min"], f["acc_max"])
        else:
            path = tmp_path / ("gpu_in_%s.bam" % form)
            path.write_bytes(B.contain(stream, "bgzf", 300) if form == "bgzf300" else B.contain(stream, form, 65280 if form == "bgzf" else 1000))
            st = ctx.load_sample(str(path), f["acc_min"], f["acc_max"])
    except P.PbsimError as e:
        if before is not None:
            assert ctx.sample_profile() == before, "a failed build changed the context's profile"
        ok = ctx.sample_profile_from_bam(GOOD, 0.0, 1.0)
        assert ok.num == 1 and ok.num_filtered == 1 and ctx.sample_profile() == [b"5" * 200]
        return str(e)
    return unpack(st, ctx)


def gpu_fastq(fq, f):
    """the GPU's FASTQ builder on the converted reads"""
    ctx = context(f)
    ctx.set_sample_chunk_bytes(0)
    try:
        return unpack(ctx.sample_profile_from_fastq(fq, f["acc_min"], f["acc_max"]), ctx)
    except P.PbsimError as e:
        return str(e)


def same(got, want, what):
    if isinstance(want, str) or isinstance(got, str):
        assert got == want, what
        return
    assert got[0] == want[0], (what, "integers", got[0], want[0])
    assert got[1] == want[1], (what, "doubles (bits)", [hex(x) for x in got[1]], [hex(x) for x in want[1]])
    assert len(got[2]) == len(want[2]), (what, "kept strings", len(got[2]), len(want[2]))
    for i, (a, b) in enumerate(zip(got[2], want[2])):
        assert a == b, (what, "kept string", i, a[:60], b[:60])


PALETTES = [list(range(5, 41)), list(range(2, 7)), list(range(30, 61)), [0, 93, 94, 254, 10, 20, 30], list(range(0, 255))]
CIGARS = [(), ((10, "S"), (50, "M"), (2, "I"), (3, "D"), (40, "M"), (7, "H")), ((1, "M"),), tuple((k + 1, "MID"[k % 3]) for k in range(70))]


def quals(r, n, palette=None):
    pal = palette if palette is not None else r.choice(PALETTES)
    return bytes(r.choice(pal) for _ in range(n))


def mixed(seed, refs=REFS3, flags=(0, 4, 16, 4 | 512, 1024 | 16, 0, 16), skipped=(256, 2048, 2048 | 16, 256 | 16)):
    """~60 records: every length of LENGTHS on both strands, names of 1 .. 17 and 254 characters, CIGARs of 0 .. 70 operations,
    tags of many types, and among the last twenty-four every other one a record that `samtools fastq` leaves out"""
    r = random.Random(seed)
    lens = LENGTHS * 2 + [r.choice(LENGTHS + [150, 400, 1500]) for _ in range(24)]
    names = [1, 254] + list(range(2, 18))
    tags = [("RG", "Z", "grp"), ("NM", "i", 7), ("ip", "BC", bytes(r.randrange(256) for _ in range(33))), ("sn", "Bf", [1.5, 2.5, 3.5, 4.5]),
            ("qs", "C", 3), ("zm", "I", 123456), ("xx", "A", "k"), ("hh", "H", "00FF"), ("ss", "Bs", [-5, 5, 7]), ("ff", "f", 0.25)]
    out = []
    for i, n in enumerate(lens):
        strand = 16 if i >= len(LENGTHS) and i < 2 * len(LENGTHS) else 0
        flag = strand if i < 2 * len(LENGTHS) else r.choice(flags)
        if i >= 2 * len(LENGTHS) and i % 2:
            flag = r.choice(skipped)
        mapped = bool(refs) and not flag & 4
        name = "".join(r.choice("abcdefgh/0123456789_") for _ in range(names[i % len(names)]))
        q = quals(r, n)
        if q[:1] == b"\xff":
            q = b"\x00" + q[1:]
        out.append(B.record(name, flag, ref_id=r.randrange(len(refs)) if mapped else -1, pos=r.randrange(40000) if mapped else -1,
                            cigar=r.choice(CIGARS) if mapped or i % 5 == 0 else (), seq="".join(r.choice("ACGTN") for _ in range(n)), qual=q,
                            tags=r.sample(tags, r.randrange(len(tags) + 1)), mapq=r.randrange(61),
                            next_ref_id=r.randrange(-1, len(refs)), next_pos=r.randrange(-1, 5000), tlen=r.randrange(-900, 900)))
    return out


def qual_alignments(records, refs):
    """where every record's first quality byte lies, mod 16, counted from the first record (a one-window buffer starts there)"""
    at, seen = 0, set()
    for rec in records:
        raw = B.record_bytes(rec)
        n = len(rec["seq"])
        seen.add((at + 36 + len(rec["name"]) + 1 + 4 * len(rec["cigar"]) + (n + 1) // 2) % 16)
        at += len(raw)
    return seen


# ---- 1. equivalence

@pytest.mark.parametrize("seed", [2, 4])
def test_profile_equals_that_of_the_converted_fastq(driver, tmp_path, seed):
    recs = mixed(seed)
    assert len(recs) == 60 and sum(1 for x in recs if x["flag"] & 0x900) == 12 and {len(r["seq"]) for r in recs} >= set(LENGTHS)
    assert {len(r["name"]) for r in recs} >= {1, 254} and qual_alignments(recs, REFS3) == set(range(16))
    assert {len(r["seq"]) % 2 for r in recs} == {0, 1}
    assert {0, 93, 94, 254} <= {q for r in recs for q in r["qual"]}
    stream, fq = B.stream(recs, REFS3, b"@HD\tVN:1.6\tSO:unknown\n"), B.to_fastq(recs)
    for f in (DEFAULT, OTHER):
        want = host(driver, tmp_path, fq, f)
        assert not isinstance(want, str) and 0 < want[0][4] < want[0][0], want[0]
        same(gpu(stream, f), want, (seed, f, "BAM against the stdio parse of its FASTQ"))
        same(gpu_fastq(fq, f), want, (seed, f, "FASTQ builder against the stdio parse"))


def test_records_without_bases(driver, tmp_path):
    """l_seq == 0 is a read with an empty quality line: what the stdio parse does with that (it counts, with length 0)"""
    r = random.Random(8)
    recs = [B.record("a", 4, qual=quals(r, 150, PALETTES[0])), B.record("empty", 4), B.record("b", 16, ref_id=0, pos=5, qual=quals(r, 120, PALETTES[0])),
            B.record("empty2", 0, ref_id=0, pos=9), B.record("c", 4, qual=quals(r, 101, PALETTES[0]))]
    stream, fq = B.stream(recs, REFS3), B.to_fastq(recs)
    for f in (DEFAULT, dict(len_min=1, len_max=1000, acc_min=0.0, acc_max=1.0)):
        want = host(driver, tmp_path, fq, f)
        assert not isinstance(want, str) and want[0][0] == 5 and want[0][1] == 0
        same(gpu(stream, f), want, f)


# ---- 2. flags

def _sum(qs):
    prob = 0.0
    for q in qs:
        prob += 10 ** (min(q, 93) / -10)
    return 1.0 - prob / len(qs)


def order_sensitive_quals(seed, n):
    """quality strings whose accuracy has other bits when the probabilities are added from the other end"""
    r = random.Random(seed)
    out = []
    for _ in range(2000):
        q = quals(r, r.choice([100, 137, 250, 1000]), PALETTES[0])
        if _sum(q) != _sum(q[::-1]):
            out.append(q)
            if len(out) == n:
                return out
    raise AssertionError("no order-sensitive quality strings found")


@pytest.mark.parametrize("n_ref", [0, 1, 3])
def test_strands_skipped_records_and_references(driver, tmp_path, n_ref):
    refs = REFS3[:n_ref]
    r = random.Random(20 + n_ref)
    qs = order_sensitive_quals(n_ref, 40)
    recs = []
    for i, q in enumerate(qs):
        mapped = n_ref > 0 and i % 3 != 0
        flag = [0, 16, 16, 0, 16 | 1024, 256, 16, 2048 | 16, 0, 256 | 16][i % 10] | (0 if mapped else 4)
        recs.append(B.record("read%d" % i, flag, ref_id=r.randrange(n_ref) if mapped else -1, pos=r.randrange(700) if mapped else -1,
                             cigar=r.choice(CIGARS[1:]) if mapped else (), qual=q, tags=[("NM", "i", i)]))
    assert sum(1 for x in recs if x["flag"] & 0x900) >= 10 and sum(1 for x in recs if x["flag"] & 0x10 and not x["flag"] & 0x900) >= 10
    stream, fq = B.stream(recs, refs), B.to_fastq(recs)
    assert fq.count(b"\n") == 4 * sum(1 for x in recs if not x["flag"] & 0x900)
    for f in (DEFAULT, OTHER):
        want = host(driver, tmp_path, fq, f)
        same(gpu(stream, f), want, (n_ref, f))
        # the check is one: as if the strand were ignored, and as if nothing were skipped, the profile is another
        forward = host(driver, tmp_path, B.to_fastq([dict(x, flag=x["flag"] & ~0x10) for x in recs]), f)
        assert forward[0] == want[0] and forward[2] != want[2]
        assert host(driver, tmp_path, B.to_fastq([dict(x, flag=x["flag"] & ~0x900) for x in recs]), f)[0][0] > want[0][0]
    # the order of the additions: an accuracy limit that is the larger of a reverse-strand read's two sums keeps that read
    # only when its probabilities are added from the right end -- on the CPU first (the stdio parse of the read turned
    # back against the read as stored), then on the GPU
    reverse = sorted((x for x in recs if x["flag"] & 0x10 and not x["flag"] & 0x900), key=lambda x: _sum(x["qual"]))[:5]
    stored = B.to_fastq([dict(x, flag=x["flag"] & ~0x10) for x in recs])
    for x in reverse:
        assert _sum(x["qual"]) != _sum(x["qual"][::-1])
        f = dict(DEFAULT, acc_min=max(_sum(x["qual"]), _sum(x["qual"][::-1])))
        want, as_stored = host(driver, tmp_path, fq, f), host(driver, tmp_path, stored, f)
        assert not isinstance(want, str) and not isinstance(as_stored, str) and abs(want[0][4] - as_stored[0][4]) >= 1, (want, as_stored)
        same(gpu(stream, f), want, (n_ref, x["name"], "accuracy limit between the two sums"))


# ---- 3. decoys

def test_record_images_inside_records(driver, tmp_path):
    """what the scan takes for records and the chain walk must not: a B:C array that is a whole plausible record (block_size
    included), several of them back to back, arrays and base / quality regions full of 0xFF and 0x00"""
    r = random.Random(31)
    image = B.record_bytes(B.record("decoy", 4, qual=bytes([40]) * 300, tags=[("RG", "Z", "x")]))
    mapped_image = B.record_bytes(B.record("decoy2", 16, ref_id=2, pos=70, cigar=((120, "M"),), qual=bytes([41]) * 120, next_ref_id=1, next_pos=3))
    recs = []
    for i in range(24):
        n = r.choice([100, 150, 333, 1000])
        kind = i % 6
        tags = [("ip", "BC", image)] if kind == 0 else [("ip", "BC", image * 3 + mapped_image)] if kind == 1 else \
            [("pw", "BC", bytes([255]) * 200), ("zz", "BC", bytes(200))] if kind == 2 else [("pw", "BC", mapped_image), ("NM", "i", 3)] if kind == 3 else []
        seq, q = ("N" * n, bytes(n)) if kind == 4 else ("=" * n, bytes([0]) + bytes([254]) * (n - 1)) if kind == 5 else (None, quals(r, n, PALETTES[0]))
        recs.append(B.record("r%d" % i, [4, 16, 0][i % 3], ref_id=-1 if i % 3 == 0 else i % 3, pos=-1 if i % 3 == 0 else 100 + i,
                             cigar=() if i % 3 == 0 else ((n, "M"),), seq=seq, qual=q, tags=tags))
    stream, fq = B.stream(recs, REFS3), B.to_fastq(recs)
    assert stream.count(image) == 4 + 4 * 3 and stream.count(b"\xff" * 200) >= 4 and stream.count(bytes(200)) >= 4
    for f in (DEFAULT, OTHER):
        want = host(driver, tmp_path, fq, f)
        assert want[0][0] == 24
        for chunk in (0, 700):
            same(gpu(stream, f, chunk), want, (f, chunk))


# ---- 4. containers and input forms

@pytest.mark.parametrize("form", FORMS)
def test_containers_and_input_forms(driver, tmp_path, form):
    recs = mixed(3)
    stream = B.stream(recs, REFS3)
    want = host(driver, tmp_path, B.to_fastq(recs), DEFAULT)
    assert not isinstance(want, str)
    for chunk in (0, 20_000):
        same(gpu(stream, DEFAULT, chunk, form, tmp_path), want, (form, chunk))


def test_load_sample_reads_a_fastq_as_load_sample_fastq_does(driver, tmp_path):
    fq = harness.synth_sample_fastq(5, 4)
    want = host(driver, tmp_path, fq, DEFAULT)
    ctx = context(DEFAULT)
    import bgzf_writer as W
    for name, data in (("plain.fastq", fq), ("bgzf.fastq.gz", W.bgzf(fq)), ("gzip.fastq.gz", W.plain_gzip(fq))):
        (tmp_path / name).write_bytes(data)
        same(unpack(ctx.load_sample(str(tmp_path / name)), ctx), want, name)
        same(unpack(ctx.load_sample_fastq(str(tmp_path / name)), ctx), want, name)
    with pytest.raises(P.PbsimError, match="Cannot open file"):
        ctx.load_sample(str(tmp_path / "missing.bam"))


# ---- 5. windows

def small(seed, n=20):
    r = random.Random(seed)
    return [B.record("s%d" % i, [4, 16, 0, 256][i % 4], ref_id=-1 if i % 4 == 0 else 0, pos=-1 if i % 4 == 0 else i,
                     cigar=() if i % 4 == 0 else ((5, "S"), (90, "M")), qual=quals(r, r.choice([99, 100, 101, 130, 257]), PALETTES[0]),
                     tags=[("NM", "i", i)] if i % 2 else []) for i in range(n)]


@pytest.mark.parametrize("chunk", [16, 64, 1000, 5000])
def test_window_sizes(driver, tmp_path, chunk):
    recs = small(5) if chunk < 1000 else mixed(4)
    stream = B.stream(recs, REFS3)
    for f in (DEFAULT, OTHER):
        want = gpu(stream, f, 0)
        same(want, host(driver, tmp_path, B.to_fastq(recs), f), "one window")
        same(gpu(stream, f, chunk), want, (chunk, f))
        same(gpu(stream, f, chunk, "device"), want, (chunk, f, "device"))


def test_a_seam_inside_every_field(driver, tmp_path):
    """three records, windows of 37 .. 37 + (the first record's size) bytes: the first seam walks through every byte of the
    first record, the later ones through the others"""
    r = random.Random(6)
    recs = [B.record("first", 16, ref_id=1, pos=40, cigar=((4, "S"), (100, "M"), (1, "I")), qual=quals(r, 105, PALETTES[0]), tags=[("NM", "i", 1)]),
            B.record("second_read", 4, qual=quals(r, 100, PALETTES[0]), tags=[("ip", "BC", bytes(range(40)))]),
            B.record("3", 0, ref_id=0, pos=1, cigar=((131, "M"),), qual=quals(r, 131, PALETTES[0]))]
    stream = B.stream(recs, REFS3)
    want = host(driver, tmp_path, B.to_fastq(recs), DEFAULT)
    assert want[0][4] == 3
    same(gpu(stream, DEFAULT, 0), want, "one window")
    size = len(B.record_bytes(recs[0]))
    assert 150 < size < 400
    for chunk in range(37, 37 + size + 1):
        same(gpu(stream, DEFAULT, chunk), want, chunk)


_MILLION = {}


def million(n):
    """a read of n bases between two ordinary ones; the bases all 'A' (they are not read), the qualities a repeated pattern"""
    if n not in _MILLION:
        r = random.Random(9)
        pat = quals(r, 1000, list(range(10, 31)))
        recs = [B.record("head", 4, qual=quals(r, 400, PALETTES[0])), B.record("big", 16, ref_id=0, pos=3, cigar=((n, "M"),), seq="A" * n,
                                                                               qual=(pat * (n // 1000 + 1))[:n]),
                B.record("tail", 0, ref_id=0, pos=9, cigar=((150, "M"),), qual=quals(r, 150, PALETTES[0]))]
        _MILLION[n] = (B.stream(recs, REFS3), B.to_fastq(recs))
    return _MILLION[n]


def test_a_record_larger_than_the_window(driver, tmp_path):
    """1 000 000 bases through windows of 64 KiB is kept; 1 000 001 is the reference's error, as its FASTQ line would be"""
    stream, fq = million(1_000_000)
    want = host(driver, tmp_path, fq, DEFAULT)
    assert want[0][2] == 1_000_000 and want[0][6] == 1_000_000 and want[0][4] == 3
    same(gpu(stream, DEFAULT, 64 << 10), want, "1 000 000, 64 KiB windows")
    same(gpu(stream, DEFAULT, 0), want, "1 000 000, one window")
    stream, fq = million(1_000_001)
    assert host(driver, tmp_path, fq, DEFAULT) == TOO_LONG
    assert gpu(stream, DEFAULT, 64 << 10) == TOO_LONG
    assert gpu(stream, DEFAULT, 0) == TOO_LONG


# ---- 6. errors

def test_errors(tmp_path):
    r = random.Random(12)
    recs = small(7, 9)
    head = B.header(REFS3, b"@HD\tVN:1.6\n")
    raw = [B.record_bytes(x) for x in recs]
    starts = [len(head) + sum(len(x) for x in raw[:i]) for i in range(len(raw) + 1)]
    good = head + b"".join(raw)
    assert not isinstance(gpu(good, DEFAULT), str)

    def each_way(stream, text):
        for form, chunk in (("bytes", 0), ("bytes", 100), ("device", 0), ("bgzf300", 0), ("none", 64), ("gzip", 0)):
            label = str(tmp_path / ("gpu_in_%s.bam" % form)) if form not in ("bytes", "device") else "BAM bytes"
            assert gpu(stream, DEFAULT, chunk, form, tmp_path) == label + ": " + text, (form, chunk)

    # the last record cut short, by one byte and in the middle of its fixed fields
    for cut in (1, len(raw[-1]) - 20, len(raw[-1]) - 2):
        each_way(good[:-cut], "malformed or truncated BAM record at inflated offset %d" % starts[-2])
    # a record without qualities: not skipped, not defaulted
    noq = B.record("the/read without", 4, qual=bytes([255]) * 120)
    for k in (0, 4, 9):
        stream = head + b"".join(raw[:k]) + B.record_bytes(noq) + b"".join(raw[k:])
        each_way(stream, "BAM record %d (the/read without) has no qualities" % (k + 1))
    # block_size one less than the record's fixed fields, name, CIGAR, bases and qualities need; zero; beyond the cap
    victim = B.record("victim", 0, ref_id=0, pos=1, cigar=((3, "S"), (117, "M")), qual=quals(r, 120, PALETTES[0]))
    need = 32 + 7 + 8 + 60 + 120
    assert len(B.record_bytes(victim)) == 4 + need
    for size in (need - 1, 0, 31, (64 << 20) + 1, 0xffffffff):
        stream = head + b"".join(raw[:3]) + B.record_bytes(victim, block_size=size) + b"".join(raw[3:])
        each_way(stream, "malformed or truncated BAM record at inflated offset %d" % starts[3])
    # l_read_name == 0, a name without its NUL, a refID that is no reference
    body = bytearray(B.record_bytes(victim))
    for at, val in ((12, 0), (36 + 6, ord("x")), (4, 3), (4, 0xfe)):
        bad = bytearray(body)
        bad[at] = val
        each_way(head + raw[0] + bytes(bad) + raw[1], "malformed or truncated BAM record at inflated offset %d" % starts[1])
    # the header overruns the stream
    for stream in (head[:-3], head[:20], b"BAM\x01", b"BAM\x01" + struct.pack("<i", 1 << 20) + bytes(100),
                   B.header([("chr1", 5)])[:-4] + struct.pack("<i", 999)[:2]):
        each_way(stream, "truncated BAM header")
    for form in ("bytes", "device"):
        assert gpu(b"@r\nACGT\n+\n!!!!\n", DEFAULT, 0, form).startswith("BAM bytes: not a BAM stream")
    # a BAM without reads in range: the FASTQ's text
    assert gpu(head, DEFAULT) == "there is no sample in the valid range of length and accuracy."
    assert gpu(head + B.record_bytes(B.record("short", 4, qual=bytes([30]) * 50)), DEFAULT) == \
        "there is no sample in the valid range of length and accuracy."


# ---- 7. the CLI

def golden_reads():
    with open(os.path.join(INPUTS, "sample.fastq"), "rb") as f:
        lines = f.read().split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [(lines[i][1:].split()[0].decode("ascii"), lines[i + 1].decode("ascii"), bytes(c - 33 for c in lines[i + 3]))
            for i in range(0, len(lines) - 1, 4)]


def golden_ubam():
    return B.bam([B.record(name, 4, seq=seq, qual=q, tags=[("RG", "Z", "golden")]) for name, seq, q in golden_reads()],
                 text=b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:golden\n")


def golden_aligned_bam():
    """every other read on the reverse strand: bases reverse-complemented and qualities reversed, as an aligner stores them"""
    comp = str.maketrans("ACGTN", "TGCAN")
    recs = []
    for i, (name, seq, q) in enumerate(golden_reads()):
        if i % 2:
            recs.append(B.record(name, 16, ref_id=0, pos=10 * i, cigar=((len(seq), "M"),), seq=seq.translate(comp)[::-1], qual=q[::-1], mapq=60))
        else:
            recs.append(B.record(name, 0, ref_id=0, pos=10 * i, cigar=((len(seq), "M"),), seq=seq, qual=q, mapq=60))
        if i % 7 == 0:      # a supplementary piece of the same read: no read of its own
            recs.append(B.record(name, 2048, ref_id=0, pos=5, cigar=((len(seq[:50]), "M"), (len(seq[50:]), "H")), seq=seq[:50], qual=q[:50]))
    return B.bam(recs, [("chr1", 10_000_000)])


@pytest.mark.parametrize("make", [golden_ubam, golden_aligned_bam])
@pytest.mark.parametrize("case", ["wgs_sample_plain", "wgs_sample_quirk", "wgs_sample_store"])
def test_cli_takes_a_bam_for_the_golden_fastq(tmp_path, case, make):
    bam = tmp_path / "sample.bam"
    bam.write_bytes(make())
    args = harness.resolve(CASES[case]["args"])
    at = args.index("--sample") + 1
    assert args[at].endswith("sample.fastq")
    args[at] = str(bam)
    wd = tmp_path / "wd"
    wd.mkdir()
    p = subprocess.run([CLI] + args + ["--prefix", str(wd / "out"), "--no-gzip"], capture_output=True, text=True, cwd=str(wd), timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    outs = harness.collect(str(wd))
    outs[".stderr"] = harness.strip_report(p.stderr).encode()
    want = MANIFEST[f"{case}/philox"]
    assert sorted(outs) == sorted(want), (sorted(outs), sorted(want))
    assert "file name : %s\n" % bam in p.stderr
    if case == "wgs_sample_store":
        assert ".profile_fastq" in outs and ".profile_stats" in outs
    for k, v in outs.items():
        assert harness.sha(v) == want[k]["sha256"], (case, k)


@pytest.mark.parametrize("container", ["bgzf", "none"])
def test_cli_refuses_a_bam_on_a_pipe(tmp_path, container):
    args = harness.resolve(CASES["wgs_sample_plain"]["args"])
    args[args.index("--sample") + 1] = "/dev/stdin"
    data = B.bam([B.record("r", 4, qual=bytes([30]) * 200)], container=container)
    p = subprocess.run([CLI] + args + ["--prefix", str(tmp_path / "out"), "--no-gzip"], input=data, capture_output=True, cwd=str(tmp_path),
                       timeout=600)
    assert p.returncode == 255
    assert b"ERROR: --sample: a BAM must be a regular file" in p.stderr
    assert not any(n.endswith((".fq", ".fastq", ".maf")) for n in os.listdir(tmp_path))
