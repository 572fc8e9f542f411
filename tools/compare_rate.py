"""`pbsim --compare-vcf` timed through the command line: the truth VCF of `--mutate-genome` at its defaults on a synthetic
record against itself, and against a copy whose indels this script rewrites to their rightmost placement.  The phases are the
stage's own `PBSIM_TRACE` lines (HIP events on its stream); the wall time of each process stands beside them.

    python tools/compare_rate.py [--bases 750000000] [--dir DIR] [--runs 2]
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import harness  # noqa: E402

CLI = os.path.join(ROOT, "pbsim3_amd", "bin", "pbsim")


def rightmost(text, seq):
    """the VCF's indels at their rightmost placement, one padding base in front; (text, lines moved)"""
    out, moved = [], 0
    for line in text.split(b"\n"):
        f = line.split(b"\t")
        if line.startswith(b"#") or not line or len(f[3]) == len(f[4]):
            out.append(line)
            continue
        s = int(f[1])
        x, d, s0 = f[4][1:], len(f[3]) - 1, s
        if x:
            while s < len(seq) and seq[s] == x[0]:
                x, s = x[1:] + x[:1], s + 1
        else:
            while s + d < len(seq) and seq[s] == seq[s + d]:
                s += 1
        moved += s != s0
        f[1], f[3], f[4] = b"%d" % s, seq[s - 1:s + d], seq[s - 1:s] + x
        out.append(b"\t".join(f))
    return b"\n".join(out), moved


def run(cmd, cwd, trace=True):
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, cwd=cwd, env=dict(os.environ, PBSIM_TRACE="1") if trace else None)
    wall = time.time() - t0
    if r.returncode != 0:
        sys.exit("%s failed:\n%s" % (" ".join(cmd), r.stderr.decode()[-3000:]))
    return r, wall


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
        _, wall = run([CLI, "--mutate-genome", "genome.fa", "--mutate-out", "variant.fa", "--mutate-vcf", "truth.vcf"], d, trace=False)
        os.remove(os.path.join(d, "variant.fa"))
        with open(os.path.join(d, "truth.vcf"), "rb") as f:
            truth = f.read()
        right, moved = rightmost(truth, seq)
        with open(os.path.join(d, "right.vcf"), "wb") as f:
            f.write(right)
        n = sum(1 for l in truth.split(b"\n") if l and not l.startswith(b"#"))
        print("genome: %d bases; truth.vcf: %d lines, %d bytes (--mutate-genome: %.1f s of wall); right.vcf: %d lines moved, %d bytes"
              % (a.bases, n, len(truth), wall, moved, len(right)))
        for what, calls in (("truth against itself", "truth.vcf"), ("truth against its rightmost copy", "right.vcf")):
            for k in range(a.runs):
                r, wall = run([CLI, "--compare-vcf", calls, "--compare-truth", "truth.vcf", "--compare-genome", "genome.fa", "--compare-out", "out.tsv",
                               "--compare-lines", "all"], d)
                print("---- %s, run %d: %.2f s of wall, %d bytes of annotated text" % (what, k + 1, wall, os.path.getsize(os.path.join(d, "out.tsv"))))
                print(r.stderr.decode().rstrip())
                if k == 0:
                    print(r.stdout.decode().rstrip())


if __name__ == "__main__":
    main()
