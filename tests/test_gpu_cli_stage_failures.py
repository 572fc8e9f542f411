"""What the stand-alone modes of the `pbsim` binary leave behind when their stage refuses the run after the outputs are opened: the
message, the input files named where there are several, no output file, nothing on the standard output.  --depth-bam, --stats-bam
and --errors-bam have this as test_cli_failure_leaves_no_output beside their own tests."""
import os
import subprocess

import pytest

import bam_writer as B
import harness

pytestmark = pytest.mark.gpu

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def _refused(argv, workdir):
    r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(workdir), timeout=300)
    assert r.returncode != 0 and r.stdout == "", r.stderr[-2000:]
    return r.stderr


@pytest.mark.parametrize("mode", ["pileup", "consensus", "call"])
def test_a_genome_of_another_length_leaves_no_output(tmp_path, mode):
    """two files of one 128-base reference and one record each, against a genome whose record of that name has 127 bases (the command
    line takes no genome record of fewer than 100 bases, so 64 against 63 does not reach the stage)"""
    for k in (0, 1):
        rec = B.record("r%d" % k, flag=0, ref_id=0, pos=3, cigar=((8, "M"),), seq="ACGTACGT", qual=bytes([30] * 8), mapq=60)
        (tmp_path / ("in%d.bam" % k)).write_bytes(B.bam([rec], [("chrA", 128)]))
    (tmp_path / "genome.fa").write_bytes(b">chrA\n" + b"ACGTTGCA" * 15 + b"ACGTTGC\n")
    before = sorted(os.listdir(tmp_path))
    err = _refused(["--%s-bam" % mode, "in0.bam", "--%s-bam" % mode, "in1.bam", "--%s-genome" % mode, "genome.fa", "--%s-out" % mode, "out.txt"], tmp_path)
    assert "this is not the genome the reads were aligned to" in err
    assert "ERROR: file 0 is in0.bam\n" in err and "ERROR: file 1 is in1.bam\n" in err
    assert sorted(os.listdir(tmp_path)) == before


TWICE = b">a\n" + b"ACGTACGTAC" * 10 + b"\n>b\n" + b"TTGACA" * 20 + b"\n>a again\n" + b"ACGT" * 25 + b"\n"


def test_mutate_refused_by_its_stage_leaves_neither_output(tmp_path):
    (tmp_path / "twice.fa").write_bytes(TWICE)
    err = _refused(["--mutate-genome", "twice.fa", "--mutate-out", "m.fa", "--mutate-vcf", "m.vcf"], tmp_path)
    assert "pbsim_genome_mutate: the genome holds two records named \"a\"" in err
    assert sorted(os.listdir(tmp_path)) == ["twice.fa"]


def test_apply_refused_by_its_stage_leaves_none_of_three_outputs(tmp_path):
    (tmp_path / "twice.fa").write_bytes(TWICE)
    (tmp_path / "in.vcf").write_bytes(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\na\t2\t.\tC\tG\t.\t.\t.\n")
    err = _refused(["--apply-vcf", "in.vcf", "--apply-genome", "twice.fa", "--apply-out", "a.fa", "--apply-report", "a.tsv", "--apply-origin", "a.bin"], tmp_path)
    assert "pbsim_vcf_apply: the genome holds two records named \"a\"" in err
    assert sorted(os.listdir(tmp_path)) == ["in.vcf", "twice.fa"]
