"""`pbsim --apply-vcf` timed through the command line: the truth VCF of `--mutate-genome` at its defaults on a synthetic
record applied to that record; the file it writes must be the mutate mode's own.  The phases are the stages' own `PBSIM_TRACE` lines
(HIP events on their streams); the wall time of each process stands beside them.  The yardstick of the FASTA passes (`bases` and
`fasta`) are the same two phases of `--mutate-genome` on the same record in the same session: both write the same bytes from the same
genome.

    python tools/apply_rate.py [--bases 750000000] [--dir DIR] [--runs 2]
"""
import argparse
import filecmp
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import harness  # noqa: E402

CLI = os.path.join(ROOT, "pbsim3_amd", "bin", "pbsim")


def run(cmd, cwd):
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, cwd=cwd, env=dict(os.environ, PBSIM_TRACE="1"))
    wall = time.time() - t0
    if r.returncode != 0:
        sys.exit("%s failed:\n%s" % (" ".join(cmd), r.stderr.decode()[-3000:]))
    return r, wall


def phases(stderr, stage):
    """{phase: ms} of the stage's trace lines"""
    return {name: float(ms) for ms, name in re.findall(r"\[pbsim %s\]\s+([0-9.]+) ms  (\w+)$" % stage, stderr, re.M)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=750_000_000)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        seq = harness.synth_bases(a.bases, 1).tobytes()
        with open(os.path.join(d, "genome.fa"), "wb") as f:
            f.write(b">synth\n")
            f.write(b"\n".join(seq[k:k + 60] for k in range(0, len(seq), 60)) + b"\n")
        del seq
        best = {}
        for k in range(a.runs):
            r, wall = run([CLI, "--mutate-genome", "genome.fa", "--mutate-out", "variant.fa", "--mutate-vcf", "truth.vcf"], d)
            print("---- --mutate-genome, run %d: %.2f s of wall" % (k + 1, wall))
            print(r.stderr.decode().rstrip())
            got = phases(r.stderr.decode(), "mutate")
            best["mutate"] = min(best.get("mutate", 1e30), got["bases"] + got["fasta"])
        with open(os.path.join(d, "truth.vcf"), "rb") as f:
            n = sum(1 for l in f if l.strip() and not l.startswith(b"#"))
        print("genome: %d bases; truth.vcf: %d lines, %d bytes" % (a.bases, n, os.path.getsize(os.path.join(d, "truth.vcf"))))
        for k in range(a.runs):
            r, wall = run([CLI, "--apply-vcf", "truth.vcf", "--apply-genome", "genome.fa", "--apply-out", "applied.fa"], d)
            same = filecmp.cmp(os.path.join(d, "applied.fa"), os.path.join(d, "variant.fa"), shallow=False)
            print("---- --apply-vcf, run %d: %.2f s of wall, %d bytes of FASTA, %s --mutate-out" %
                  (k + 1, wall, os.path.getsize(os.path.join(d, "applied.fa")), "identical to" if same else "DIFFERS FROM"))
            print(r.stderr.decode().rstrip())
            if k == 0:
                print(r.stdout.decode().rstrip())
            got = phases(r.stderr.decode(), "apply")
            best["apply"] = min(best.get("apply", 1e30), got["bases"] + got["fasta"])
            if not same:
                sys.exit("--apply-out differs from --mutate-out")
        print("the FASTA passes (bases + fasta, the faster run): --mutate-genome %.2f ms, --apply-vcf %.2f ms, ratio %.2f"
              % (best["mutate"], best["apply"], best["apply"] / best["mutate"]))


if __name__ == "__main__":
    main()
