"""The truth stream as aligned BAM records made on the GPU (pbsim_set_truth_bam; k_cigar_rows / k_aln_finish in
pbsim3_amd/csrc/kernels.hip): read back with tests/bam_spec_reader.py, every record must be what tests/cigar_model.py makes
of the MAF block of the same task, the MAF coming from the same inputs and seed in MAF mode (and, for the golden cases,
pinned to the reference's digests first).  The read stream and the statistics must not notice the switch."""
import gzip
import math
import os
import subprocess

import pytest

import bam_spec_reader as R
import bgzf_writer as W
import cigar_model as M
import harness
import maf_truth
import pbsim3_amd as P
from cases import CASES
from pbsim3_amd import args as A

pytestmark = pytest.mark.gpu

MANIFEST = harness.load_manifest()
VERSION = P.load().pbsim_version().decode()


# ---------------------------------------------------------------- running a command in either mode
def _stats(s):
    return {f: getattr(s, f) for f, _ in P.Stats._fields_}


def _same_stats(x, y, what):
    for k in x:
        a, b = x[k], y[k]
        assert a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b)), (what, k, a, b)


def run(argv, truth_bam, scratch_mb=None, deflate=0, arrays=False):
    """one dict per unit (wgs: record; trans / templ: the unit set): read text, truth bytes, stats, the truth BAM header
    (BAM mode), reference list expected in it, and -- arrays=True, where pbsim_simulate_arrays runs -- per-task n_sub + n_ins + n_del"""
    p, a = A.parse(argv)
    out = []
    with P.Context(p, 0) as ctx:
        if scratch_mb:
            ctx.set_scratch_bytes(scratch_mb << 20)
        if deflate:
            ctx.set_deflate(deflate)
        if p.method == P.METHOD_ERR:
            ctx.load_errhmm(a["--errhmm"])
        elif p.method == P.METHOD_QS:
            ctx.load_qshmm(a["--qshmm"])
        else:
            ctx.load_sample_fastq(a["--sample"], int(float(a["--accuracy-min"]) * 100) * 0.01 if "--accuracy-min" in a else 0.75,
                                  int(float(a["--accuracy-max"]) * 100) * 0.01 if "--accuracy-max" in a else 1.0)
        if p.strategy == P.STRATEGY_WGS:
            recs = A.read_fasta(a["--genome"])[0]
            if p.hp_del_bias != 1:
                for r in recs:
                    ctx.add_hp_census(r)
                ctx.finish_hp_census()
            units = [(lambda r=r, i=i: ctx.set_reference(r, i), i, [(b"ref", len(r))]) for i, r in enumerate(recs, 1)]
        elif p.strategy == P.STRATEGY_TRANS:
            with open(a["--transcript"], "rb") as f:
                rows = [ln.split(b"\t") for ln in f.read().split(b"\n") if ln.strip()]
            refs = [(M.sn_cut(r[0][:128]), len(r[3].strip())) for r in rows]
            units = [(lambda: ctx.load_transcript_file(a["--transcript"]), None, refs)]
        else:
            with open(a["--template"], "rb") as f:
                ids = [ln[1:].rstrip(b"\r")[:128] for ln in f.read().split(b"\n") if ln.startswith(b">")]
            refs = [(M.sn_cut(i), len(s)) for i, s in zip(ids, A.read_fasta(a["--template"])[0])]
            units = [(lambda: ctx.load_template_file(a["--template"]), None, refs)]
        if truth_bam:
            ctx.set_truth_bam(True)
        for load, rec, refs in units:
            load()
            u = dict(rec=rec, refs=refs)
            if p.method == P.METHOD_SAMPLE:
                u["read"], u["truth"] = ctx.simulate_sample()
            elif rec:
                u["read"], u["truth"] = ctx.simulate_wgs()
            else:
                u["read"], u["truth"] = ctx.simulate_trans()
            u["stats"] = _stats(ctx.stats())
            u["sam_header"] = ctx.sam_header() if p.pass_num > 1 else b""
            if truth_bam:
                u["header"] = ctx.truth_bam_header()
            if arrays and p.method != P.METHOD_SAMPLE:
                b = ctx.simulate_arrays(labels=False)
                u["nm"] = (b.n_sub + b.n_ins + b.n_del).cpu().numpy()
                u["unit"] = b.unit.cpu().numpy()
            out.append(u)
    return p, out


def parse_truth(header, records):
    """(text, refs, alignments) of header + records, through the spec reader (which wants BGZF: framed here with zlib)"""
    return R.read_bam(W.bgzf(header + records))


def expected_records(p, unit_maf, unit_read, nm=None, ref_ids=None, max_ops=M.MAX_OPS):
    blocks = maf_truth.parse_maf(unit_maf)
    reads = maf_truth.parse_reads(unit_read, p.pass_num)
    assert len(blocks) == len(reads)
    quality = p.method != P.METHOD_ERR
    out = []
    for t, (blk, (rid, _, ql)) in enumerate(zip(blocks, reads)):
        assert rid == blk[4]
        out.append(M.record(blk, ref_id=0 if ref_ids is None else int(ref_ids[t]), qual=ql if quality else None,
                            nm=None if nm is None else nm[t], max_ops=max_ops))
    return blocks, out


def compare_records(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for t, (g, w) in enumerate(zip(got, want)):
        if g != w:
            bad = [k for k in w if g.get(k) != w[k]]
            k = bad[0]
            raise AssertionError(f"{what}: record {t} ({w['read_name']}, flag {w['flag']}) differs in {bad}: "
                                 f"{k} got {str(g.get(k))[:300]} want {str(w[k])[:300]}")


def check_unit(p, maf_u, bam_u, what, ref_ids=None):
    """everything test 1 asks of one unit's pair of runs; returns the MAF blocks"""
    assert bam_u["read"] == maf_u["read"], what
    _same_stats(maf_u["stats"], bam_u["stats"], what)
    text, refs, got = parse_truth(bam_u["header"], bam_u["truth"])
    assert text == M.header_text(bam_u["refs"], VERSION), (what, text[:300])
    assert refs == [(sn.decode(), ln) for sn, ln in bam_u["refs"]], what
    blocks, want = expected_records(p, maf_u["truth"], maf_u["read"], ref_ids=ref_ids)
    compare_records(got, want, what)
    if "nm" in maf_u:
        assert [g["aux"][0][2] for g in got] == [int(x) for x in maf_u["nm"]], what
    if ref_ids is not None:       # the MAF name of every task is its reference's, cut
        assert [refs[g["refID"]][0].encode() for g in got] == [M.sn_cut(b[0]) for b in blocks], what
    return blocks


# ---------------------------------------------------------------- 1. the golden cases
def _golden_argv(case):
    c = CASES[case]
    argv = list(c["args"])
    if "--sample" not in argv and "sample" in case:      # wgs_sample_reuse: the stored profile is its setup's --sample, filtered
        s = c["setup"]
        argv += ["--sample", s[s.index("--sample") + 1]]
        for opt in ("--accuracy-min", "--accuracy-max", "--length-min", "--length-max"):     # (what the setup filtered with)
            if opt in s:
                argv += [opt, s[s.index(opt) + 1]]
        k = argv.index("--sample-profile-id")
        del argv[k:k + 2]
    elif "--sample-profile-id" in argv:
        k = argv.index("--sample-profile-id")
        del argv[k:k + 2]
    return harness.resolve(argv)


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_golden_case_record_by_record(case):
    argv = _golden_argv(case)
    gold = MANIFEST[f"{case}/philox"]
    p, maf = run(argv, False, arrays=True)
    _, bam = run(argv, True)
    assert len(maf) == len(bam) > 0
    for mu, bu in zip(maf, bam):
        rec = mu["rec"]
        name = ("_%04d" % rec if rec else "") + (".fq" if p.pass_num == 1 else ".sam")
        maf_name = ("_%04d" % rec if rec else "") + ".maf"
        assert harness.sha(mu["truth"]) == gold[maf_name]["sha256"], (case, maf_name)
        assert harness.sha(mu["sam_header"] + mu["read"]) == gold[name]["sha256"], (case, name)
        check_unit(p, mu, bu, f"{case}{maf_name}", ref_ids=mu.get("unit") if not rec else None)


# ---------------------------------------------------------------- 2. seams
GENOME_LEN = 4000
SEAM_L = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023]


def _read_orientation_runs(blk):
    """[(first column, length, op)] of a block's runs in READ orientation (the scratch rows' and so the kernels' columns)"""
    runs = M.cigar_runs(blk[3], blk[6])
    if blk[5] == b"-":
        runs = runs[::-1]
    out, at = [], 0
    for k, op in runs:
        out.append((at, k, op))
        at += k
    return out


def _spans(blocks, step):
    """does some run hold columns c - 1 and c for a multiple c of `step`"""
    for blk in blocks:
        for at, k, _ in _read_orientation_runs(blk):
            if (at // step + 1) * step <= at + k - 1:
                return True
    return False


@pytest.mark.parametrize("coop", ["-1", "0"])
@pytest.mark.parametrize("L", SEAM_L)
def test_seams(L, coop, tmp_path, monkeypatch):
    """fixed read length L on a 4000-base record, both strands, a 1 MiB scratch pool (several batches), lane and wave walker"""
    monkeypatch.setenv("PBSIM_COOP_LEN", coop)
    qs = SEAM_L.index(L) % 2 == 1
    per_read = (3 if qs else 2) * ((2 * L + 64) * 1.12) + 64        # what a batch charges a read (batch_capacity_for)
    n_reads = int(2.5 * (1 << 20) / per_read) + 2
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">g\n" + harness.synth_bases(GENOME_LEN, 3).tobytes() + b"\n")
    argv = ["--strategy", "wgs", "--genome", str(fa), "--length-min", str(L), "--length-max", str(L), "--length-mean", str(L),
            "--length-sd", "0", "--accuracy-mean", "0.85", "--seed", str(40 + L), "--depth", repr(n_reads * L / GENOME_LEN)]
    argv += ["--method", "qshmm", "--qshmm", harness.model_path("QSHMM-RSII.model")] if qs else \
            ["--method", "errhmm", "--errhmm", harness.model_path("ERRHMM-ONT.model")]
    p, maf = run(argv, False, scratch_mb=1, arrays=True)
    _, bam = run(argv, True, scratch_mb=1)
    blocks = check_unit(p, maf[0], bam[0], f"L={L} coop={coop}")
    assert maf[0]["stats"]["res_num"] > 2 * int(1 << 20) / per_read       # several batches
    strands = {b[5] for b in blocks}
    assert strands == {b"+", b"-"}
    # the shapes this case is about are there (else: another seed)
    ends = [(_read_orientation_runs(b)[0][2], _read_orientation_runs(b)[-1][2]) for b in blocks if b[5] == b"-" and b[3]]
    assert any(a in "ID" or z in "ID" for a, z in ends), "no '-' task starts or ends in a gap run"
    if L >= 65:
        assert _spans(blocks, 64), "no run crosses a 64-column word"
    if L >= 255:
        assert _spans(blocks, 256), "no run crosses a 256-column tile"
    if L >= 17:
        assert _spans(blocks, 16), "no run crosses a 16-column chunk"


# ---------------------------------------------------------------- 3. CIGAR overflow
def test_cigar_overflow_moves_into_the_cg_tag(tmp_path):
    """reads of up to 400 000 bases at accuracy 0.85 beside short ones (QSHMM-RSII at its default 6:55:39: nearly every error
    is an indel, about a run per four columns; ERRHMM-ONT's substitutions leave a 400 000-base read at ~42 000 runs): more than
    65535 runs -> <q>S<span>N + CG:B,I"""
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">g\n" + harness.synth_bases(450_000, 9).tobytes() + b"\n")
    argv = ["--strategy", "wgs", "--method", "qshmm", "--qshmm", harness.model_path("QSHMM-RSII.model"), "--genome", str(fa),
            "--length-min", "100", "--length-max", "400000", "--length-mean", "300000", "--length-sd", "150000",
            "--accuracy-mean", "0.85", "--seed", "2", "--depth", "2.6"]
    p, maf = run(argv, False, arrays=True)
    _, bam = run(argv, True)
    blocks = check_unit(p, maf[0], bam[0], "overflow")
    n_runs = [len(M.cigar_runs(b[3], b[6])) for b in blocks]
    assert max(n_runs) > 65535 and min(n_runs) < 65535, n_runs
    _, _, got = parse_truth(bam[0]["header"], bam[0]["truth"])
    for g, n in zip(got, n_runs):
        if n > 65535:
            assert g["n_cigar_op"] == 2 and [op for _, op in g["cigar"]] == ["S", "N"] and [a[0] for a in g["aux"]] == ["NM", "CG"]
            assert len(g["aux"][1][2]) == n
        else:
            assert g["n_cigar_op"] == n and [a[0] for a in g["aux"]] == ["NM"]


# ---------------------------------------------------------------- 4. delivery
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def test_deflated_members_are_the_same_stream():
    argv = harness.resolve(CASES["wgs_qshmm_rsii_pass3"]["args"])
    _, plain = run(argv, True, scratch_mb=4)
    _, packed = run(argv, True, scratch_mb=4, deflate=3)
    with P.Context(A.parse(argv)[0], 0) as ctx:
        for u, z in zip(plain, packed):
            assert z["truth"] != u["truth"]
            head = ctx.deflate_buffer(u["header"])
            whole = head + z["truth"] + P.BGZF_EOF
            assert b"".join(R.blocks(whole)) == u["header"] + u["truth"]
            assert b"".join(R.blocks(z["truth"] + P.BGZF_EOF)) == u["truth"]
            text, refs, recs = R.read_bam(whole)
            assert refs == [("ref", u["refs"][0][1])] and len(recs) == u["stats"]["res_pass_num"]


def _cli(args, workdir, extra=(), ranks=1, scratch_mb=None):
    import pbsim3_amd.build as b
    b.build()
    e = dict(os.environ)
    if scratch_mb:
        e["PBSIM_SCRATCH_MB"] = str(scratch_mb)
    os.makedirs(workdir, exist_ok=True)
    cmd = [CLI] + harness.resolve(args) + ["--prefix", os.path.join(workdir, "out")] + list(extra)
    if ranks > 1:
        cmd += ["--devices", ",".join(["0"] * ranks)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=workdir, env=e, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    files = {}
    for n in sorted(os.listdir(workdir)):
        if n.startswith("out") and not n.endswith(".ref"):
            with open(os.path.join(workdir, n), "rb") as f:
                files[n[3:]] = f.read()
    return files, harness.strip_report(r.stderr)


@pytest.mark.parametrize("case,scratch_mb", [("wgs_errhmm-ont_quirk", 3), ("trans_errhmm_rsii_readme", None),
                                             ("wgs_sample_plain", None)])
def test_cli_writes_aln_bam_on_one_and_three_ranks(case, scratch_mb, tmp_path):
    """--truth-format bam: <prefix>[_NNNN].aln.bam = header member, record members, EOF marker; no .maf file; the records are
    the MAF's of the same command; one rank and three ranks on the one GPU write the same inflated bytes"""
    args = CASES[case]["args"]
    p = A.parse(harness.resolve(args))[0]
    maf, err_maf = _cli(args, str(tmp_path / "m"), extra=("--no-gzip",))
    gold = MANIFEST[f"{case}/philox"]
    for k, v in maf.items():      # without the flag: the parent's bytes
        assert harness.sha(v) == gold[k]["sha256"], (case, k)
    one, err_one = _cli(args, str(tmp_path / "b1"), extra=("--truth-format", "bam"), scratch_mb=scratch_mb)
    three, err_three = _cli(args, str(tmp_path / "b3"), extra=("--truth-format", "bam"), ranks=3, scratch_mb=scratch_mb)
    assert err_one == err_maf == err_three
    assert sorted(one) == sorted(three) and not [n for n in one if ".maf" in n]
    alns = [n for n in one if n.endswith(".aln.bam")]
    assert len(alns) == len([n for n in maf if n.endswith(".maf")]) > 0
    for n in alns:
        stem = n[:-len(".aln.bam")]
        assert one[n].endswith(P.BGZF_EOF) and three[n].endswith(P.BGZF_EOF)
        stream = b"".join(R.blocks(one[n]))
        assert b"".join(R.blocks(three[n])) == stream, (case, n)
        text, refs, got = R.read_bam(one[n])
        read_name = stem + (".fq" if p.pass_num == 1 else ".sam")
        blocks = maf_truth.parse_maf(maf[stem + ".maf"])
        if p.strategy == P.STRATEGY_WGS:
            assert [r[0] for r in refs] == ["ref"] and text.startswith(b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:ref\tLN:%d\n@PG" % refs[0][1])
            ref_ids = None
        else:
            names = [r[0].encode() for r in refs]
            assert len(set(names)) == len(names)
            ref_ids = [names.index(M.sn_cut(b[0])) for b in blocks]
        _, want = expected_records(p, maf[stem + ".maf"], maf[read_name], ref_ids=ref_ids)
        compare_records(got, want, f"{case}{n}")
    for n in one:                 # the read stream does not notice
        if n.endswith(".fq.gz"):
            assert gzip.decompress(one[n]) == maf[n[:-3]] == gzip.decompress(three[n])


# ---------------------------------------------------------------- reference names SAM does not allow
@pytest.mark.parametrize("ids,word", [([b"t1 x", b"t2", b"t1 y"], "unit 3"), ([b"ok", b"=bad"], "unit 2"), ([b"a", b" lead"], "unit 2"),
                                      ([b"a,b"], "unit 1")])
def test_unit_names_outside_rname_are_refused(ids, word, tmp_path):
    fa = tmp_path / "t.fa"
    fa.write_bytes(b"".join(b">" + i + b"\n" + harness.synth_bases(300, k).tobytes() + b"\n" for k, i in enumerate(ids)))
    p = P.default_params(strategy=P.STRATEGY_TEMPL, method=P.METHOD_ERR, seed=1)
    with P.Context(p, 0) as ctx:
        ctx.load_errhmm(harness.model_path("ERRHMM-ONT.model"))
        ctx.load_template_file(str(fa))
        with pytest.raises(P.PbsimError, match=word):
            ctx.set_truth_bam(True)
        rt, mt = ctx.simulate_trans()           # still MAF, still usable
        assert mt.startswith(b"a\ns ")
    with P.Context(p, 0) as ctx:                # the switch first, the units afterwards: the first simulate call fails
        ctx.load_errhmm(harness.model_path("ERRHMM-ONT.model"))
        ctx.set_truth_bam(True)
        ctx.load_template_file(str(fa))
        with pytest.raises(P.PbsimError, match=word):
            ctx.simulate_trans()
