"""`pbsim --lift-bam` timed through the command line: a synthetic record, `--mutate-genome` at its default rates, reads
simulated from the variant FASTA at `--depth` with `--truth-format bam`, and that truth BAM lifted back to the original record.  The
phases are the stage's own `PBSIM_TRACE` lines (HIP events on its stream); the wall time of each process stands beside them.  The
yardstick is `pbsim --sort-truth-bam` on a copy of the same file: its gather and its deflate-and-deliver phases move the same bytes
that the lift's write and deliver phases move, without the column passes.

    python tools/lift_rate.py [--bases 100000000] [--depth 20] [--method errhmm] [--dir DIR] [--runs 2]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import harness  # noqa: E402

CLI = os.path.join(ROOT, "pbsim3_amd", "bin", "pbsim")
METHODS = {"errhmm": ["--method", "errhmm", "--errhmm", "MODEL:ERRHMM-RSII.model"], "qshmm": ["--method", "qshmm", "--qshmm", "MODEL:QSHMM-RSII.model"]}


def run(cmd, cwd):
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, cwd=cwd, env=dict(os.environ, PBSIM_TRACE="1"))
    wall = time.time() - t0
    if r.returncode != 0:
        sys.exit("%s failed:\n%s" % (" ".join(cmd), r.stderr.decode()[-3000:]))
    return r, wall


def trace(stderr, stage):
    """the stage's trace lines"""
    return "\n".join(l for l in stderr.splitlines() if l.startswith("[pbsim %s]" % stage))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=100_000_000)
    ap.add_argument("--depth", default="20")
    ap.add_argument("--method", default="errhmm", choices=sorted(METHODS))
    ap.add_argument("--dir", default=None)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        seq = harness.synth_bases(a.bases, 1).tobytes()
        with open(os.path.join(d, "genome.fa"), "wb") as f:
            f.write(b">synth\n")
            f.write(b"\n".join(seq[k:k + 60] for k in range(0, len(seq), 60)) + b"\n")
        del seq
        r, wall = run([CLI, "--mutate-genome", "genome.fa", "--mutate-out", "variant.fa", "--mutate-vcf", "truth.vcf"], d)
        print("---- --mutate-genome: %.2f s of wall" % wall)
        print(r.stdout.decode().rstrip())
        r, wall = run([CLI] + harness.resolve(["--strategy", "wgs"] + METHODS[a.method] + ["--genome", "variant.fa", "--depth", a.depth, "--seed", "7",
                                                                                           "--prefix", "sd", "--truth-format", "bam"]), d)
        truth = os.path.join(d, "sd_0001.aln.bam")
        print("---- the simulation from the variant genome: %.2f s of wall, %d bytes of truth BAM" % (wall, os.path.getsize(truth)))
        for k in range(a.runs):
            r, wall = run([CLI, "--lift-bam", "sd_0001.aln.bam", "--lift-out", "lifted.bam", "--lift-genome", "genome.fa", "--lift-vcf", "truth.vcf",
                           "--lift-ref-name", "synth"], d)
            print("---- --lift-bam, run %d: %.2f s of wall, %d bytes of lifted BAM" % (k + 1, wall, os.path.getsize(os.path.join(d, "lifted.bam"))))
            print(trace(r.stderr.decode(), "apply"))
            print(trace(r.stderr.decode(), "lift"))
            if k == 0:
                print(r.stdout.decode().rstrip())
        for k in range(a.runs):
            shutil.copyfile(truth, os.path.join(d, "copy.aln.bam"))
            r, wall = run([CLI, "--sort-truth-bam", "copy.aln.bam"], d)
            print("---- --sort-truth-bam on a copy of the same file, run %d: %.2f s of wall" % (k + 1, wall))
            print(trace(r.stderr.decode(), "sort"))
        r, wall = run([CLI, "--errors-bam", "lifted.bam", "--errors-genome", "genome.fa", "--errors-ref-names", "synth"], d)
        counts = dict(re.findall(r"(\w+)=(\d+)", r.stdout.decode().splitlines()[0]))
        print("---- --errors-bam of the lifted file against the original genome: scored %s, nm_agree %s, nm_differ %s, nm_unchecked %s"
              % tuple(counts.get(k) for k in ("scored", "nm_agree", "nm_differ", "nm_unchecked")))


if __name__ == "__main__":
    main()
