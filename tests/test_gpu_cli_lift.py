"""`pbsim --lift-bam` on the device: files on disk in, the lifted file equal to Context.lift_bam's, the report on stdout, and no output
file after a refused line, a genome that is not the reads' or a VCF that is not the variant genome's."""
import os
import subprocess

import numpy as np
import pytest

import harness
import lift_model as L
import pbsim3_amd as P
from stats_model import inflate
from test_gpu_bam_lift import E2E, METHODS, e2e_genome, fasta_records

pytestmark = pytest.mark.gpu

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def run(cmd, cwd, ok=True):
    r = subprocess.run([CLI] + cmd, capture_output=True, cwd=str(cwd), timeout=300)
    assert (r.returncode == 0) == ok, r.stderr[-3000:]
    return r


def test_cli_lifts_the_truth_files_of_a_variant_genome(tmp_path):
    import pbsim3_amd.build as b
    b.build()
    genome = e2e_genome()
    with open(tmp_path / "genome.fa", "wb") as f:
        for name, seq in genome:
            f.write(b">" + name.encode() + b" the original\n" + b"".join(seq[k:k + 70] + b"\n" for k in range(0, len(seq), 70)))
    opts = [x for k, v in E2E.items() for x in ("--mutate-" + k.replace("_", "-"), str(v))]
    run(["--mutate-genome", "genome.fa", "--mutate-out", "variant.fa", "--mutate-vcf", "truth.vcf"] + opts, tmp_path)
    run(harness.resolve(["--strategy", "wgs"] + METHODS["errhmm"] + ["--genome", "variant.fa", "--depth", "6", "--seed", "9", "--length-mean", "400",
                                                                     "--length-sd", "100", "--length-min", "100", "--length-max", "900", "--prefix", "sd",
                                                                     "--truth-format", "bam"]), tmp_path)
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as ctx:
        origins = ctx.mutate_genome(genome, origin=True, **E2E)[5]
        for k, (name, _) in enumerate(genome):
            truth = "sd_%04d.aln.bam" % (k + 1)
            base = ["--lift-bam", truth, "--lift-genome", "genome.fa", "--lift-vcf", "truth.vcf", "--lift-ref-name", name]
            r = run(base + ["--lift-out", "lifted%d.bam" % k], tmp_path)
            with open(tmp_path / truth, "rb") as f:
                want = ctx.lift_bam(f.read(), genome, origins, ref_name=name)
            with open(tmp_path / ("lifted%d.bam" % k), "rb") as f:
                assert f.read() == want[2]
            assert r.stdout == want[1] and want[0]["moved"] > 0 and want[0]["lifted"] > 20
            if k:
                continue
            # no output file after a refused line, a genome that is not the reads', a VCF of another variant genome
            run(base + ["--lift-out", "no.bam", "--lift-haplotype", "3"], tmp_path, ok=False)
            r = run(["--lift-bam", truth, "--lift-genome", "genome.fa", "--lift-vcf", "truth.vcf", "--lift-ref-name", genome[1 - k][0],
                     "--lift-out", "no.bam"], tmp_path, ok=False)
            assert b"this is not the genome these reads came from" in r.stderr
            r = run(["--lift-bam", truth, "--lift-genome", "variant.fa", "--lift-vcf", "truth.vcf", "--lift-ref-name", name, "--lift-out", "no.bam"],
                    tmp_path, ok=False)
            assert r.stderr.startswith(b"ERROR: ")
            assert not os.path.exists(tmp_path / "no.bam")
