"""The BAM input of the sampling method where no device is needed (pbsim_load_sample, pbsim_sample_profile_from_bam_bytes /
_from_bam_device; pbsim3_amd/csrc/sample_profile.cpp, bam_chain.cpp): the entry points exist and check their arguments first,
a tables-only context refuses them and stays usable, and the HIP-free host decisions -- the header parse and the chain walk
over the scan's candidates, which the truth-BAM sort shares with its own packing -- run as a program of their own under
ASan + UBSan (tests/asan/bam_chain_driver.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import bam_writer as B
import harness
import pbsim3_amd as P

CSRC = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
SYMBOLS = ["pbsim_load_sample", "pbsim_sample_profile_from_bam_bytes", "pbsim_sample_profile_from_bam_device"]
BAM = B.stream([B.record("r", 4, qual=bytes([20]) * 200)])
MAX_BLOCK = 64 << 20            # the sampling input's packing: 28 size bits
SORT_MAX_BLOCK = (1 << 24) - 1  # the sort's: 24
REF_LISTS = [[], [("chr1", 1000)], [("a", 5), ("b" * 300, 6), ("chrM", 16569)]]


def params():
    return P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_SAMPLE)


def test_symbols_and_methods_exist():
    lib = P.load()
    bound = {n for n, _, _ in P.API}
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in bound, name
    for name in ("load_sample", "sample_profile_from_bam"):
        assert callable(getattr(P.Context, name)), name
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert "int %s(pbsim_ctx *ctx" % name in header, name
    import pbsim3_amd.build as b
    assert "sample_bam.hip" in b.HIP_SOURCES and "bam_scan.hip" in b.HIP_SOURCES and "bam_chain.cpp" in b.CXX_SOURCES


def test_tables_only_context_refuses_and_stays_usable(tmp_path):
    path = tmp_path / "s.bam"
    path.write_bytes(B.contain(BAM))
    with P.Context(params(), -1) as c:
        for call in (lambda: c.sample_profile_from_bam(BAM), lambda: c.load_sample(str(path)), lambda: c.sample_profile_from_bam(BAM)):
            with pytest.raises(P.PbsimError, match="no HIP device"):
                call()
        st = P.SampleStats()
        assert c.lib.pbsim_sample_profile_from_bam_device(c.h, C.c_void_p(16), 4, 0.75, 1.0, C.byref(st)) == 0
        assert b"no HIP device" in c.lib.pbsim_last_error()
        assert c.sam_header() is not None         # the context still answers


def test_argument_errors_come_first():
    with P.Context(params(), -1) as c:
        st = P.SampleStats()
        for fn, arg in ((c.lib.pbsim_sample_profile_from_bam_bytes, BAM), (c.lib.pbsim_sample_profile_from_bam_device, C.c_void_p(16))):
            assert fn(c.h, arg, -1, 0.75, 1.0, C.byref(st)) == 0                     # a negative size
            assert b"bad argument" in c.lib.pbsim_last_error()
            assert fn(c.h, None, 5, 0.75, 1.0, C.byref(st)) == 0                     # bytes promised, none given
            assert b"bad argument" in c.lib.pbsim_last_error()
            assert fn(c.h, arg, 4, 0.75, 1.0, None) == 0                             # nowhere to put the statistics
            assert b"bad argument" in c.lib.pbsim_last_error()
            assert fn(c.h, arg, 4, 0.9, 0.8, C.byref(st)) == 0
            assert b"accuracy_min exceeds accuracy_max" in c.lib.pbsim_last_error()
        assert c.lib.pbsim_load_sample(c.h, None, 0.75, 1.0, C.byref(st)) == 0
        assert b"pbsim_load_sample: bad argument" in c.lib.pbsim_last_error()
        with pytest.raises(P.PbsimError, match="accuracy_min exceeds accuracy_max"):
            c.sample_profile_from_bam(BAM, 0.9, 0.8)
        with pytest.raises(P.PbsimError, match="accuracy_min exceeds accuracy_max"):
            c.load_sample("/nonexistent", 1.0, 0.5)
        with pytest.raises(TypeError):
            c.sample_profile_from_bam("not bytes")
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), -1) as c:
        with pytest.raises(P.PbsimError, match="no HIP device|method is not sample"):
            c.sample_profile_from_bam(BAM)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """bam_chain.cpp alone (it includes no HIP header) with the stand-alone driver, ASan + UBSan; nothing of it is loaded here"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("bamchain") / "bam_chain_driver")
    p = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        os.path.join(harness.ROOT, "tests", "asan", "bam_chain_driver.cpp"), os.path.join(CSRC, "bam_chain.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def run(driver, *args):
    p = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (args, (p.stdout + p.stderr)[-3000:])
    return p.stdout.splitlines()


def test_hip_free_translation_unit():
    """what the driver is built from includes nothing of HIP and nothing of the library's device side"""
    for name in ("bam_chain.cpp", "bam_chain.h"):
        with open(os.path.join(CSRC, name)) as f:
            includes = [line for line in f if line.startswith("#include")]
        assert includes and not any(w in line for line in includes for w in ("hip", "ctx.h", "kernels.h", "engine")), (name, includes)


@pytest.mark.parametrize("refs", REF_LISTS)
def test_header_parse(driver, tmp_path, refs):
    text = b"@HD\tVN:1.6\n@SQ\tSN:x\tLN:5\n" * 3
    h = B.header(refs, text)
    body = h + B.record_bytes(B.record("r", 4, qual=bytes([30]) * 10))
    path = tmp_path / "h.bin"
    path.write_bytes(body)
    n = len(body)
    # the whole stream: parsed; every shorter view of it: "not enough yet" until the last length that says where the first
    # record lies has been seen (the last reference's l_name: its name and l_ref are only stepped over), parsed from there on
    need = len(h) - (len(refs[-1][0]) + 1 + 4 if refs else 0)
    out = run(driver, "header", path, *["%d:%d" % (n, have) for have in range(n + 1)])
    for have, line in enumerate(out):
        want = "header %d:%d -> 1 %d %d" % (n, have, len(refs), len(h)) if have >= need else "header %d:%d -> 0 -7 -7" % (n, have)
        assert line == want, (have, line)
    # a stream that ends inside the header, at every byte: the header overruns it -- said at the latest when all of it is seen
    pairs = [(n, have) for n in range(len(h)) for have in sorted({0, n // 2, max(n - 1, 0), n})]
    for (n, have), line in zip(pairs, run(driver, "header", path, *["%d:%d" % p for p in pairs])):
        rc = int(line.split()[3])
        assert line.split()[1] == "%d:%d" % (n, have)
        assert rc in (((-1,) if n else (-2,)) if have == n else (-1, 0)), line
    assert run(driver, "header", path, "%d:%d" % (len(h), len(h)))[0].endswith("-> 1 %d %d" % (len(refs), len(h)))   # no records


def test_header_lengths_that_lie(driver, tmp_path):
    import struct
    cases = {
        "no_magic": (b"@r\nACGT\n+\n!!!!\n", -2),
        "gzip_bytes": (b"\x1f\x8b\x08\x04" + bytes(20), -2),
        "negative_l_text": (b"BAM\x01" + struct.pack("<i", -1) + bytes(40), -1),
        "huge_l_text": (b"BAM\x01" + struct.pack("<i", 0x7fffffff) + bytes(40), -1),
        "negative_n_ref": (b"BAM\x01" + struct.pack("<ii", 0, -5) + bytes(40), -1),
        "huge_n_ref": (b"BAM\x01" + struct.pack("<ii", 0, 0x7fffffff) + bytes(3), -1),
        "negative_l_name": (b"BAM\x01" + struct.pack("<iii", 0, 1, -2) + bytes(40), -1),
        "huge_l_name": (b"BAM\x01" + struct.pack("<iii", 0, 2, 0x7ffffff0) + bytes(40), -1),
    }
    for name, (data, want) in cases.items():
        path = tmp_path / name
        path.write_bytes(data)
        assert int(run(driver, "header", path, "%d:%d" % (len(data), len(data)))[0].split()[3]) == want, name


@pytest.mark.parametrize("refs", REF_LISTS)
def test_header_parse_for_the_sort(driver, tmp_path, refs):
    """with the reference lengths wanted: l_text and every l_ref exactly, and not before the last l_ref has been seen"""
    text = b"@HD\tVN:1.6\n@SQ\tSN:x\tLN:5\n" * 3
    h = B.header(refs, text)
    body = h + B.record_bytes(B.record("r", 4, qual=bytes([30]) * 10))
    path = tmp_path / "h.bin"
    path.write_bytes(body)
    n = len(body)
    good = "1 0 0 %d %d %d" % (len(text), len(refs), len(h)) + "".join(" %d" % l for _, l in refs)
    for have, line in enumerate(run(driver, "header+", path, *["%d:%d" % (n, have) for have in range(n + 1)])):
        assert line == "header %d:%d -> %s" % (n, have, good if have >= len(h) else "0 0 0 -7 -7 -7"), (have, line)


def test_header_faults_of_the_sort(driver, tmp_path):
    """one byte string per refusal of pbsim_truth_bam_sort: (return code, fault); and an l_name of 0 is reported, not refused"""
    import struct
    SHORT, MAGIC, TEXT, NREF, REFS = 1, 2, 3, 4, 5
    cases = {
        "short": (b"BAM\x01" + bytes(7), -1, SHORT),
        "short_without_magic": (b"@r\nACGT\n+\n", -2, SHORT),
        "no_magic": (b"@r\nACGT\n+\n!!!!\n", -2, MAGIC),
        "negative_l_text": (b"BAM\x01" + struct.pack("<i", -1) + bytes(40), -1, TEXT),
        "l_text_past_the_end": (b"BAM\x01" + struct.pack("<i", 37) + bytes(40), -1, TEXT),
        "negative_n_ref": (b"BAM\x01" + struct.pack("<ii", 0, -5) + bytes(40), -1, NREF),
        "list_past_the_end": (b"BAM\x01" + struct.pack("<ii", 0, 2) + struct.pack("<i", 2) + b"a\0" + struct.pack("<i", 9), -1, REFS),
        "name_past_the_end": (b"BAM\x01" + struct.pack("<iii", 0, 1, 33) + bytes(36), -1, REFS),
        "negative_l_name": (b"BAM\x01" + struct.pack("<iii", 0, 1, -2) + bytes(40), -1, REFS),
    }
    for name, (data, rc, fault) in cases.items():
        path = tmp_path / name
        path.write_bytes(data)
        for cmd in ("header", "header+"):
            line = run(driver, cmd, path, "%d:%d" % (len(data), len(data)))[0].split()
            assert int(line[3]) == rc, (name, cmd, line)
        assert int(line[4]) == fault and line[5:] == ["0", "-7", "-7", "-7"], (name, line)
    data = b"BAM\x01" + struct.pack("<ii", 0, 2) + struct.pack("<ii", 0, 7) + struct.pack("<i", 2) + b"a\0" + struct.pack("<i", 9) + bytes(5)
    path = tmp_path / "empty_name"
    path.write_bytes(data)
    assert run(driver, "header+", path, "%d:%d" % (len(data), len(data)))[0].endswith("-> 1 0 1 0 2 %d 7 9" % (len(data) - 5))
    assert run(driver, "header", path, "%d:%d" % (len(data), len(data)))[0].endswith("-> 1 2 %d" % (len(data) - 5))


def chain_scenarios(driver, bits):
    max_block = {28: MAX_BLOCK, 24: SORT_MAX_BLOCK}[bits]

    def chain(frm, end, last, hits):
        return run(driver, "chain", bits, frm, end, int(last), *["%d:%d" % h for h in hits])[0]

    # three records of 100, 40 and 60 bytes (block_size + 4) behind offset 10
    true = [(10, 96), (110, 36), (150, 56)]
    assert chain(10, 210, True, true) == "chain -> done 210 3 10:96 110:36 150:56"
    assert chain(10, 210, False, true) == "chain -> done 210 3 10:96 110:36 150:56"
    # decoys: inside a record (a tag that holds a record image), and one that would lead somewhere else
    decoys = sorted(true + [(30, 40), (31, 75), (120, 26), (151, 55)])
    assert chain(10, 210, True, decoys) == "chain -> done 210 3 10:96 110:36 150:56"
    # a missing candidate where the chain lands: malformed behind the last window, never a jump to the next plausible one
    assert chain(10, 210, True, [true[0], true[2]]) == "chain -> malformed 110 1 10:96"
    assert chain(10, 210, True, [true[0], (111, 35), true[2]]) == "chain -> malformed 110 1 10:96"
    assert chain(10, 210, True, true[1:]) == "chain -> malformed 10 0"
    assert chain(10, 210, True, []) == "chain -> malformed 10 0"
    # a window that ends inside the last record: the scan gives no candidate for it, the bytes are carried
    assert chain(10, 190, False, true[:2]) == "chain -> carry 150 2 10:96 110:36"
    assert chain(10, 152, False, true[:2]) == "chain -> carry 150 2 10:96 110:36"      # not even a whole block_size
    assert chain(10, 50, False, []) == "chain -> carry 10 0"
    # ... and the stream that ends there is truncated
    assert chain(10, 190, True, true[:2]) == "chain -> malformed 150 2 10:96 110:36"
    # a candidate that overruns the bytes (the scan gives none) is not followed
    assert chain(10, 190, True, true) == "chain -> malformed 150 2 10:96 110:36"
    assert chain(0, 0, True, []) == "chain -> done 0 0"
    # the cap: a record may be as large as the packing's max_block, a carry never needs to grow beyond one such record
    assert chain(0, 4 + max_block, False, [(0, max_block)]) == "chain -> done %d 1 0:%d" % (4 + max_block, max_block)
    assert chain(10, 14 + max_block, True, [(10, max_block)]) == "chain -> done %d 1 10:%d" % (14 + max_block, max_block)
    if bits == 28:      # (the sort's packing has no bits for a larger size: its cap is the mask)
        assert chain(0, 4 + MAX_BLOCK + 1, True, [(0, MAX_BLOCK + 1)]) == "chain -> malformed 0 0"
    assert chain(0, 4 + max_block - 1, False, []) == "chain -> carry 0 0"
    assert chain(0, 4 + max_block, False, []) == "chain -> malformed 0 0"
    assert chain(100, 100 + 4 + max_block, False, [(0, 96)]) == "chain -> malformed 100 0"
    assert chain(100, 100 + 4 + (1 << bits), True, []) == "chain -> malformed 100 0"


def test_chain_walk(driver):
    chain_scenarios(driver, 28)


def test_chain_walk_with_the_sorts_packing(driver):
    """offset << 24 | block_size: a record of 2^24 - 1 bytes is followed, 4 + 2^24 bytes without a candidate are malformed"""
    chain_scenarios(driver, 24)
