"""The digest machinery behind the BASELINE-size reference goldens (tests/golden/fullsize.json), on the CPU:

* the small case of fullsize_cases.py was run by the REFERENCE through the same stubs (crcsum.c in place of gzip): the oracle's
  files for the same command must have exactly those CRC-32s and lengths, and the same stderr report;
* harness.synth_bases_torch (what the GPU box generates the 750 Mbp record with) equals harness.synth_bases (what the reference
  was fed) -- here on torch's CPU device, same integer arithmetic;
* every case of fullsize_cases.py has its digests committed;
* the small generated cases (a --transcript file, a --sample FASTQ: harness.synth_transcripts / synth_sample_fastq) are
  still the bytes the reference was run on (`input_sha256`), and the oracle reproduces the reference's files for them."""
import os
import zlib

import numpy as np
import pytest

import harness
from fullsize_cases import FULLSIZE


def test_every_case_has_reference_digests():
    full = harness.load_fullsize()
    for name, case in FULLSIZE.items():
        assert name in full, "run tests/golden/make_fullsize.py %s" % name
        e = full[name]
        assert e["args"] == case["args"]
        for k in ("record", "transcripts", "sample"):
            assert e.get(k) == (list(case[k]) if k in case else None), (name, k)
        if "transcripts" in case or "sample" in case:
            assert sorted(e["input_sha256"]) == sorted(k for k, c in (("genome", "record"), ("transcript", "transcripts"),
                                                                       ("sample", "sample")) if c in case)
        streams = [k for k in e if k.startswith(".")]
        assert ".maf" in streams and (".fq" in streams or ".sam" in streams)
        for k in streams:
            assert len(e[k]["crc32"]) == 8 and e[k]["bytes"] > 0
        assert "read num. :" in e["stderr"]


def test_oracle_reproduces_the_reference_digest_of_the_small_case(tmp_path):
    name = "t0_errhmm_ont_200k_d5"
    want = harness.load_fullsize()[name]
    length, seed = FULLSIZE[name]["record"]
    seq = harness.synth_bases(length, seed)
    fa = tmp_path / "g.fa"
    with open(fa, "wb") as f:
        f.write(b">synth_%d_%d\n" % (length, seed))
        rows = seq.reshape(-1, 80)
        f.write(np.concatenate([rows, np.full((rows.shape[0], 1), 10, np.uint8)], axis=1).tobytes())
    od = tmp_path / "o"
    od.mkdir()
    got = harness.run_oracle(FULLSIZE[name]["args"] + ["--genome", str(fa)], "philox", str(od))
    for key in (".fq", ".maf"):
        data = got["_0001" + key]
        assert (len(data), "%08x" % zlib.crc32(data)) == (want[key]["bytes"], want[key]["crc32"]), key
    assert got[".stderr"].decode() == want["stderr"]


@pytest.mark.parametrize("name", ["t1_trans_small", "t2_sample_small"])
def test_oracle_reproduces_the_reference_digest_of_the_small_generated_cases(name, tmp_path):
    """the transcript file and the sampling FASTQ of harness.synth_transcripts / synth_sample_fastq: the generators still
    write the bytes the reference was run on, and the oracle's files and report for them are the reference's"""
    want = harness.load_fullsize()[name]
    case = FULLSIZE[name]
    inputs, digests = harness.write_case_inputs(case, str(tmp_path))
    assert digests == want["input_sha256"], "a generator no longer writes the input the reference was run on"
    od = tmp_path / "o"
    od.mkdir()
    got = harness.run_oracle(case["args"] + inputs, "philox", str(od))
    stem = "" if "transcripts" in case else "_0001"
    for key in (".fq", ".maf"):
        data = got[stem + key]
        assert (len(data), "%08x" % zlib.crc32(data)) == (want[key]["bytes"], want[key]["crc32"]), key
    assert got[".stderr"].decode() == want["stderr"]


def test_small_generated_cases_reach_their_edges():
    """what the small cases are there for is in them: every listed edge unit (transcript lines split by fgets, a homopolymer
    across a split, ids cut at TRANS_ID_LEN_MAX, start-position rank 999) and the sampling filter's bounds"""
    tr = harness.synth_transcripts(*FULLSIZE["t1_trans_small"]["transcripts"])
    lines = tr.split(b"\n")[:-1]
    assert len(lines) == 200 + len(harness.transcript_edge_units(5))
    by_len = {len(x) + 1 for x in lines}
    assert {10238, 10239, 10240, 10241, 10242, 20479, 20480} <= by_len
    hp = next(x for x in lines if b"_line20479\t" in x)
    assert hp[10230:10247] == b"G" * 17
    assert max(len(x.split(b"\t")[3]) for x in lines) == 999_000
    ids = [x.split(b"\t")[0] for x in lines]
    assert max(map(len, ids)) == 200 and harness.TRANS_ID_LEN_MAX in map(len, ids)
    seqs = [x.split(b"\t")[3] for x in lines]
    assert any(s[:1].islower() for s in seqs) and any(b"N" * 300 in s for s in seqs)
    fq = harness.synth_sample_fastq(*FULLSIZE["t2_sample_small"]["sample"])
    quals = fq.split(b"\n")[3::4]
    kept = harness.sample_profile(fq)
    accs = sorted(1 - sum(10 ** ((c - 33) / -10) for c in q) / len(q) for q in quals[300:700])
    assert accs[0] < 0.75 < accs[-1]                              # the cluster straddles --accuracy-min
    assert {99, 100, 101} <= set(map(len, quals)) and 99 not in set(map(len, kept))
    assert min(min(q) for q in quals) == ord("!") and max(max(q) for q in quals) == ord("~")


def test_sample_profile_equals_the_python_filter(tmp_path):
    """harness.sample_profile (numpy, sequential cumsum) keeps exactly the strings pbsim3_amd.args.read_sample_fastq keeps"""
    from pbsim3_amd import args as A
    fq = harness.synth_sample_fastq(300, 6)
    p = tmp_path / "s.fq"
    p.write_bytes(fq)
    assert harness.sample_profile(fq) == A.read_sample_fastq(str(p))


@pytest.mark.parametrize("n,seed", [(1, 1), (1000, 7), ((1 << 22) + 12345, 101), (3_000_000, 104)])
def test_synth_bases_torch_equals_numpy(n, seed):
    import torch
    a = harness.synth_bases(n, seed)
    b = harness.synth_bases_torch(n, seed, device="cpu").numpy()
    assert np.array_equal(a, b)
