"""`pbsim` on gzip-compressed inputs (--genome / --transcript / --template / --sample, recognised by content): every case of
tests/golden/cases.py with its input files as BGZF (inflated on the GPU) and as plain gzip (zlib on the host) gives the
reference's own output from the plain files, byte for byte."""
import gzip
import hashlib
import os
import shutil
import subprocess
from multiprocessing import Pool

import pytest

import bgzf_writer as W
import harness
from cases import CASES

MANIFEST = harness.load_manifest()
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")
TIMEOUT = 600

pytestmark = pytest.mark.gpu


def compress(data, kind):
    return W.bgzf(data) if kind == "bgzf" else W.plain_gzip(data)


def gz_args(args, indir, kind):
    """INPUT:name -> indir/name, written there compressed under the same name"""
    out = []
    for a in args:
        if a.startswith("INPUT:"):
            name = a[6:]
            dst = os.path.join(indir, name)
            if not os.path.exists(dst):
                with open(harness.input_path(name), "rb") as f:
                    data = f.read()
                with open(dst, "wb") as f:
                    f.write(compress(data, kind))
            out.append(dst)
        elif a.startswith("MODEL:"):
            out.append(harness.model_path(a[6:]))
        else:
            out.append(a)
    return out


def run(args, workdir, extra=(), env=None):
    p = subprocess.run([CLI] + list(args) + ["--prefix", os.path.join(workdir, "out"), "--no-gzip"] + list(extra),
                       capture_output=True, text=True, cwd=workdir, timeout=TIMEOUT, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    outs = harness.collect(workdir)
    outs[".stderr"] = harness.strip_report(p.stderr).encode()
    return outs


def check_golden(case, outs):
    want = MANIFEST[f"{case}/philox"]
    assert sorted(outs) == sorted(want), (sorted(outs), sorted(want))
    for k, v in outs.items():
        assert harness.sha(v) == want[k]["sha256"], f"{case}{k}"


@pytest.fixture(scope="module", autouse=True)
def built():
    import pbsim3_amd.build as b
    b.build()


@pytest.mark.parametrize("kind", ["bgzf", "gzip"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_compressed_inputs_match_golden(case, kind, tmp_path):
    indir, work = tmp_path / "in", tmp_path / "work"
    indir.mkdir()
    work.mkdir()
    spec = CASES[case]
    if spec.get("setup"):
        subprocess.run([CLI] + gz_args(spec["setup"], str(indir), kind) + ["--prefix", str(work / "setup"), "--no-gzip"],
                       capture_output=True, text=True, check=True, cwd=str(work), timeout=TIMEOUT)
        for fn in os.listdir(work):
            if fn.startswith("setup"):
                os.remove(work / fn)
    check_golden(case, run(gz_args(spec["args"], str(indir), kind), str(work)))


def test_committed_gzip_transcript(tmp_path):
    case = "trans_qshmm_rsii_readme"
    args = [harness.input_path("sample.transcript.gz") if a == "INPUT:sample.transcript" else a for a in CASES[case]["args"]]
    check_golden(case, run(harness.resolve(args), str(tmp_path)))


def test_bgzf_genome_two_ranks(tmp_path):
    case = "wgs_errhmm-ont_quirk"
    (tmp_path / "in").mkdir()
    (tmp_path / "w").mkdir()
    check_golden(case, run(gz_args(CASES[case]["args"], str(tmp_path / "in"), "bgzf"), str(tmp_path / "w"),
                           ["--devices", "0,0"]))


def test_sample_from_pbsim_own_fq_gz(tmp_path):
    """the .fq.gz pbsim writes (BGZF members from the GPU deflate) as --sample: the same run as on its inflated bytes"""
    src = CASES["wgs_qshmm_rsii_pass1"]["args"]
    (tmp_path / "a").mkdir()
    p = subprocess.run([CLI] + harness.resolve(src) + ["--prefix", str(tmp_path / "a" / "out")], capture_output=True,
                       text=True, timeout=TIMEOUT)
    assert p.returncode == 0, p.stderr[-2000:]
    fq_gz = str(tmp_path / "a" / "out_0001.fq.gz")
    with gzip.open(fq_gz, "rb") as f:
        plain = f.read()
    (tmp_path / "plain.fastq").write_bytes(plain)
    base = ["--strategy", "wgs", "--method", "sample", "--genome", harness.input_path("plain.fa"), "--depth", "2",
            "--seed", "3"]
    (tmp_path / "x").mkdir()
    (tmp_path / "y").mkdir()
    got = run(base + ["--sample", fq_gz], str(tmp_path / "x"))
    want = run(base + ["--sample", str(tmp_path / "plain.fastq")], str(tmp_path / "y"))
    assert got == want


def _bgzf_block(args):
    data, level = args
    return W.member(data, level=level)


def test_large_bgzf_genome(tmp_path):
    """a 200 Mbp genome (many pieces' worth of members) in BGZF against the plain file, by the outputs' digests"""
    plain = harness.input_path("synth_200000000_21.fa")
    with open(plain, "rb") as f:
        fa = f.read()
    blocks = [(fa[i:i + W.BGZIP_BLOCK], 1) for i in range(0, len(fa), W.BGZIP_BLOCK)]
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        z = b"".join(pool.map(_bgzf_block, blocks, chunksize=256)) + W.EOF_MARKER
    del fa, blocks
    (tmp_path / "gz").mkdir()
    (tmp_path / "gz" / "g.fa").write_bytes(z)
    args = ["--strategy", "wgs", "--method", "errhmm", "--errhmm", harness.model_path("ERRHMM-ONT.model"), "--depth", "0.2",
            "--seed", "5"]
    (tmp_path / "x").mkdir()
    (tmp_path / "y").mkdir()
    got = run(args + ["--genome", str(tmp_path / "gz" / "g.fa")], str(tmp_path / "x"))
    want = run(args + ["--genome", plain], str(tmp_path / "y"))
    assert sorted(got) == sorted(want)
    for k in want:
        assert hashlib.sha256(got[k]).digest() == hashlib.sha256(want[k]).digest(), k


def test_corrupt_bgzf_genome_fails_once(tmp_path):
    """a BGZF genome with a bad member: the run stops with the member's offset and the reference-stats header, once"""
    case = "wgs_errhmm-ont_quirk"
    with open(harness.input_path("quirk.fa"), "rb") as f:
        fa = f.read()
    first = W.member(fa[:1000])
    bad = W.member(fa[1000:2000], crc=0)
    (tmp_path / "quirk.fa").write_bytes(first + bad + W.bgzf(fa[2000:]))
    args = [str(tmp_path / "quirk.fa") if a == "INPUT:quirk.fa" else a for a in CASES[case]["args"]]
    p = subprocess.run([CLI] + harness.resolve(args) + ["--prefix", str(tmp_path / "out"), "--no-gzip"],
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert p.returncode == 255
    assert f"ERROR: {tmp_path / 'quirk.fa'}: gzip member at byte offset {len(first)}: incorrect data check" in p.stderr
    assert p.stderr.count("gzip member at byte offset") == 1 and p.stderr.count(":::: Reference stats ::::") == 1


def test_transcript_through_a_fifo(tmp_path):
    """a named pipe is read as before (never opened by the gzip check): the goldens"""
    import threading
    case = "trans_errhmm_sequel"
    fifo = str(tmp_path / "tiny.transcript")
    os.mkfifo(fifo)
    with open(harness.input_path("tiny.transcript"), "rb") as f:
        data = f.read()

    def feed():
        with open(fifo, "wb") as w:
            w.write(data)

    t = threading.Thread(target=feed, daemon=True)
    t.start()
    args = [fifo if a == "INPUT:tiny.transcript" else a for a in CASES[case]["args"]]
    (tmp_path / "w").mkdir()
    check_golden(case, run(harness.resolve(args), str(tmp_path / "w")))
    t.join(timeout=10)
