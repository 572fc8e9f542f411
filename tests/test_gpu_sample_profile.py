"""The sampling method's profile built on the GPU from the FASTQ's bytes (pbsim3_amd/csrc/sample_profile.hip and
sample_profile.cpp: pbsim_sample_profile_from_bytes / _from_device, pbsim_load_sample_fastq) against the host's parsers:
the kept strings and their order against harness.sample_profile, all twelve statistics (doubles by their bits) and the
error texts against the stdio parse (read_sample_fastq_stdio, through tests/sample_profile_driver.cpp) -- over the line
layouts the line logic must get right, over window sizes that put seams inside every line, over the input forms, and
through the pool (simulate_sample) and the CLI."""
import os
import random
import shutil
import struct
import subprocess

import pytest

import bgzf_writer as W
import harness
import pbsim3_amd as P

pytestmark = pytest.mark.gpu
CSRC = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")
INPUTS = os.path.join(harness.GOLDEN, "inputs")
DEFAULT = dict(len_min=100, len_max=1_000_000, acc_min=0.75, acc_max=1.0)
OTHER = dict(len_min=30, len_max=5000, acc_min=0.5, acc_max=0.97)
INTS = ["num", "len_min", "len_max", "len_total", "num_filtered", "len_min_filtered", "len_max_filtered", "len_total_filtered"]
DOUBLES = ["len_mean_filtered", "len_sd_filtered", "accuracy_mean_filtered", "accuracy_sd_filtered"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("drv") / "sample_profile_driver")
    p = subprocess.run([cxx, "-O1", "-std=c++17", "-pthread", "-I", CSRC, os.path.join(harness.ROOT, "tests", "sample_profile_driver.cpp"),
                        os.path.join(CSRC, "unit_io.cpp"), "-o", exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def host(driver, tmp_path, fq, f):
    """(ints, double bits, kept strings) of the stdio parse, or the error text"""
    path = tmp_path / "host_in.fastq"
    path.write_bytes(fq)
    kept = tmp_path / "host_kept"
    p = subprocess.run([driver, str(path), str(f["len_min"]), str(f["len_max"]), float(f["acc_min"]).hex(), float(f["acc_max"]).hex(),
                        str(kept)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    if p.stdout.startswith("error "):
        return p.stdout[6:].rstrip("\n")
    lines = p.stdout.splitlines()
    ints = [int(x) for x in lines[0].split()[1:]]
    bits = [int(x, 16) for x in lines[1].split()[1:]]
    return ints, bits, kept.read_bytes().split(b"\n")[:-1]


def context(f):
    return P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_SAMPLE, len_min=f["len_min"], len_max=f["len_max"]), 0)


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


def gpu(fq, f, chunk=0, form="bytes", tmp_path=None):
    """the same from the GPU builder; `form`: how the bytes reach it"""
    key = (f["len_min"], f["len_max"])
    if key not in _CONTEXTS:
        _CONTEXTS[key] = context(f)
    ctx = _CONTEXTS[key]
    ctx.set_sample_chunk_bytes(chunk)
    try:
        if form == "bytes":
            st = ctx.sample_profile_from_fastq(fq, f["acc_min"], f["acc_max"])
        elif form == "device":
            import torch
            t = torch.frombuffer(bytearray(fq), dtype=torch.uint8).cuda() if fq else torch.empty(0, dtype=torch.uint8, device="cuda")
            st = ctx.sample_profile_from_fastq(t, f["acc_min"], f["acc_max"])
        else:
            path = tmp_path / ("gpu_in." + form)
            path.write_bytes({"path": lambda b: b, "bgzf": W.bgzf, "gzip": W.plain_gzip}[form](fq))
            st = ctx.load_sample_fastq(str(path), f["acc_min"], f["acc_max"])
    except P.PbsimError as e:
        # the context stays usable: the next profile is built as if nothing had happened
        ok = ctx.sample_profile_from_fastq(b"@r\nACGT\n+\n" + b"5" * 200 + b"\n", 0.0, 1.0)
        assert ok.num == 1 and ok.num_filtered == 1 and ctx.sample_profile() == [b"5" * 200]
        return str(e)
    return unpack(st, ctx)


def same(got, want, what):
    if isinstance(want, str) or isinstance(got, str):
        assert got == want, what
        return
    assert got[0] == want[0], (what, "integers", got[0], want[0])
    assert got[1] == want[1], (what, "doubles (bits)", [hex(x) for x in got[1]], [hex(x) for x in want[1]])
    assert len(got[2]) == len(want[2]), (what, "kept strings", len(got[2]), len(want[2]))
    for i, (a, b) in enumerate(zip(got[2], want[2])):
        assert a == b, (what, "kept string", i, a[:60], b[:60])


def rec(r, i, n, lo=5, hi=40, eol=b"\n", head=None, bases=None):
    q = bytes(33 + r.randint(lo, hi) for _ in range(n))
    return (head if head is not None else b"@r%d" % i) + eol + (bases if bases is not None else b"A" * n) + eol + b"+" + eol + q + eol


def mixed(seed, n=60):
    r = random.Random(seed)
    return b"".join(rec(r, i, r.choice([20, 99, 100, 101, 150, 400, 1500, 4999, 5000, 5001]), *r.choice([(5, 40), (2, 6), (30, 60)]))
                    for i in range(n))


def layouts():
    r = random.Random(11)
    base = mixed(1)
    noise = bytes(x for x in (r.randrange(1, 256) for _ in range(40000)) if x != 10)
    out = {
        "plain": base,
        "no_final_line_feed": base[:-1],
        "ends_after_one_line": base + b"@tail\n",
        "ends_after_two_lines": base + b"@tail\nACGT\n",
        "ends_after_three_lines": base + b"@tail\nACGT\n+\n",
        "ends_inside_the_fourth_line": base + b"@tail\nACGT\n+\n" + b"I" * 300,
        "lines_over_10240": b"".join(rec(r, i, n, head=b"@" + b"h" * hn, bases=b"C" * bn)
                                     for i, (n, hn, bn) in enumerate([(10239, 5, 10240), (10240, 10241, 7), (10241, 3, 20481),
                                                                      (30721, 20480, 30720), (200, 10239, 10239), (20479, 1, 1)])),
        "crlf": b"".join(rec(r, i, n, eol=b"\r\n") for i, n in enumerate([99, 100, 101, 250, 3000])),
        "bytes_outside_the_quality_alphabet": b"".join(
            b"@o%d\nA\n+\n" % i + bytes(r.choice([1, 9, 13, 32, 33, 60, 126, 127, 128, 200, 255]) for _ in range(n)) + b"\n"
            for i, n in enumerate([150, 100, 99, 1000, 333])),
        "garbage_in_header_and_base_lines": b"".join(rec(r, i, 200 + 50 * i, head=noise[i * 900:i * 900 + 700 + i],
                                                         bases=noise[20000 + i * 800:20000 + i * 800 + 3 * i]) for i in range(12)),
        "empty_lines": b"\n\n\n\n" + base + b"\n\n\n" + b"5" * 120 + b"\n",
        "nul_byte": base[:5000] + b"\0" + base[5000:],
        "nothing_in_range": b"".join(rec(r, i, n) for i, n in enumerate([5, 50, 99])),
        "empty": b"",
        "one_line_feed": b"\n",
    }
    return out


LAYOUTS = layouts()


@pytest.mark.parametrize("name", sorted(LAYOUTS))
@pytest.mark.parametrize("chunk", [0, 4096, 1000, 61])
def test_layouts_against_the_stdio_parse(driver, tmp_path, name, chunk):
    fq = LAYOUTS[name]
    for f in (DEFAULT, OTHER):
        want = host(driver, tmp_path, fq, f)
        same(gpu(fq, f, chunk), want, (name, chunk, f))
    if name == "nothing_in_range":
        assert host(driver, tmp_path, fq, DEFAULT) == "there is no sample in the valid range of length and accuracy."


def test_seams_inside_every_line(driver, tmp_path):
    """windows of 16 .. 40 bytes over records of ~420 bytes: a seam at every offset of every one of the four lines"""
    r = random.Random(5)
    fq = b"".join(rec(r, i, 100 + i, head=b"@seam%d" % i) for i in range(6))
    want = host(driver, tmp_path, fq, DEFAULT)
    assert not isinstance(want, str) and want[0][4] > 0
    for chunk in range(16, 41):
        same(gpu(fq, DEFAULT, chunk), want, chunk)


@pytest.mark.parametrize("n,seed", [(0, 3), (40, 1), (300, 2)])
def test_synthetic_fastq(driver, tmp_path, n, seed):
    """harness.synth_sample_fastq: its 400-string cluster straddles accuracy 0.75, its 99/100/101-character strings the length filter"""
    fq = harness.synth_sample_fastq(n, seed)
    want = host(driver, tmp_path, fq, DEFAULT)
    assert want[2] == harness.sample_profile(fq)
    assert 0 < want[0][4] < want[0][0]
    longest = max(len(q) for q in fq.split(b"\n")[3::4])
    assert n == 0 or longest > 20_000          # the smaller windows below are shorter than the longest quality line
    for chunk in [0, 1 << 16] + ([4096, 1000] if n <= 40 else [20_000]):
        same(gpu(fq, DEFAULT, chunk), want, (n, chunk))
    same(gpu(fq, OTHER, 1 << 16), host(driver, tmp_path, fq, OTHER), (n, "other filter"))
    assert gpu(fq, OTHER, 0)[2] == harness.sample_profile(fq, **OTHER)


def test_golden_sample_fastq(driver, tmp_path):
    with open(os.path.join(INPUTS, "sample.fastq"), "rb") as f:
        fq = f.read()
    for flt in (DEFAULT, OTHER, dict(len_min=500, len_max=2000, acc_min=0.8, acc_max=0.9)):
        want = host(driver, tmp_path, fq, flt)
        assert want[2] == harness.sample_profile(fq, **flt)
        for chunk in (0, 3000, 777):
            same(gpu(fq, flt, chunk), want, (flt, chunk))
    w = host(driver, tmp_path, fq, DEFAULT)
    assert w[0][0] == 153 and w[0][4] == 124


@pytest.mark.parametrize("chunk", [0, 300_000])
def test_quality_line_of_a_million(driver, tmp_path, chunk):
    """exactly 1 000 000 characters is kept, 1 000 001 is the reference's error -- also when the line has no line feed"""
    r = random.Random(9)
    head = rec(r, 0, 400) + rec(r, 1, 120)
    big = bytes(33 + r.randint(10, 30) for _ in range(1000))

    def one(n):
        return b"@big\nA\n+\n" + (big * (n // 1000 + 1))[:n] + b"\n"

    ok = head + one(1_000_000) + rec(r, 2, 150)
    want = host(driver, tmp_path, ok, DEFAULT)
    assert want[0][2] == 1_000_000 and want[0][6] == 1_000_000
    same(gpu(ok, DEFAULT, chunk), want, "1 000 000")
    for name, bad in (("1 000 001", head + one(1_000_001) + rec(r, 3, 150)),
                      ("1 000 001 without a line feed", head + one(1_000_001)[:-1]),
                      ("1 000 000 without a line feed", head + one(1_000_000)[:-1])):
        want = host(driver, tmp_path, bad, DEFAULT)
        if "1 000 001" in name:
            assert want == "fastq is too long. Max acceptable length is 1000000."
        same(gpu(bad, DEFAULT, chunk), want, name)


@pytest.mark.parametrize("form", ["device", "path", "bgzf", "gzip"])
def test_input_forms(driver, tmp_path, form):
    fq = harness.synth_sample_fastq(25, 7)
    want = gpu(fq, DEFAULT)
    same(want, host(driver, tmp_path, fq, DEFAULT), "bytes")
    for chunk in (0, 50_000):
        same(gpu(fq, DEFAULT, chunk, form, tmp_path), want, (form, chunk))
    nul = fq[:777] + b"\0" + fq[777:]                     # the fallback takes every form too
    same(gpu(nul, DEFAULT, 0, form, tmp_path), host(driver, tmp_path, nul, DEFAULT), (form, "NUL"))
    none = b"@r\nA\n+\n!!!!\n"
    assert gpu(none, DEFAULT, 0, form, tmp_path) == "there is no sample in the valid range of length and accuracy."


def test_failure_keeps_the_profile_the_context_had(tmp_path):
    fq = harness.synth_sample_fastq(5, 4)
    with context(DEFAULT) as ctx:
        ctx.sample_profile_from_fastq(fq)
        before = ctx.sample_profile()
        with pytest.raises(P.PbsimError, match="no sample in the valid range"):
            ctx.sample_profile_from_fastq(b"@r\nA\n+\n!!!!\n")
        with pytest.raises(P.PbsimError, match="Cannot open file"):
            ctx.load_sample_fastq(str(tmp_path / "missing.fastq"))
        assert ctx.sample_profile() == before == harness.sample_profile(fq)


def test_pool_is_the_one_set_sample_profile_leaves():
    """simulate_sample after the GPU builder: the FASTQ + MAF bytes and pbsim_get_stats of set_sample_profile with the same strings"""
    path = os.path.join(INPUTS, "sample.fastq")
    with open(path, "rb") as f:
        fq = f.read()
    from pbsim3_amd import args as A
    genome = A.read_fasta(os.path.join(INPUTS, "plain.fa"))[0][0]
    p = P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_SAMPLE, seed=11, depth=3.0)

    def run(load):
        with P.Context(p, 0) as ctx:
            ctx.set_scratch_bytes(24 << 20)
            load(ctx)
            ctx.set_reference(genome, 1)
            rt, mt = ctx.simulate_sample()
            st = ctx.stats()
            return rt, mt, tuple(getattr(st, f[0]) for f in st._fields_)

    want = run(lambda ctx: ctx.set_sample_profile(harness.sample_profile(fq)))
    assert len(want[0]) > 100_000 and want[2][0] > 0
    assert run(lambda ctx: ctx.sample_profile_from_fastq(fq)) == want
    assert run(lambda ctx: (ctx.set_sample_chunk_bytes(5000), ctx.load_sample_fastq(path))) == want


@pytest.mark.parametrize("devices", ["0", "0,0"])
def test_cli_file_against_pipe(tmp_path, devices):
    """--sample FILE --sample-profile-id X (the GPU builder) against the same FASTQ on a pipe (the host's stdio parse): the
    same profile files, outputs and stderr apart from the `file name` line"""
    fq = harness.synth_sample_fastq(12, 6)
    src = tmp_path / "in.fastq"
    src.write_bytes(fq)
    base = ["--strategy", "wgs", "--method", "sample", "--genome", harness.input_path("plain.fa"), "--depth", "2", "--seed", "5",
            "--sample-profile-id", "X", "--no-gzip", "--devices", devices]

    def run(name, sample, stdin):
        wd = tmp_path / name
        wd.mkdir()
        p = subprocess.run([CLI] + base + ["--sample", sample, "--prefix", str(wd / "out")], input=stdin, capture_output=True, cwd=wd,
                           timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        outs = harness.collect(str(wd))
        outs[".stderr"] = harness.strip_report(p.stderr.decode())
        return outs

    got = run("file", str(src), None)
    base[-1] = "0"                                # (one pipe has one reader: the pipe run is the one-rank run)
    want = run("pipe", "/dev/stdin", fq)
    assert sorted(got) == sorted(want) and ".profile_fastq" in got and ".profile_stats" in got and "_0001.maf" in got
    for k in want:
        assert got[k] == want[k], k
    assert got[".profile_fastq"] == b"".join(q + b"\n" for q in harness.sample_profile(fq))
