"""The phases of `pbsim --errors-bam` on one MI355X: a truth BAM of product size (--bases uniform bases, depth 20, --method errhmm
with ERRHMM-ONT or qshmm with QSHMM-ONT, --truth-format bam, made here by the command line) through Context.bam_errors in one
process: one warm-up call, then --runs calls, the phases taken from the stage's own HIP events (PBSIM_TRACE).  Beside them, in the
same warm process, the phases of Context.bam_stats on the same bytes.  From the phase times the column pass as columns per second,
and at 4 bytes per column (a reference byte, a class byte, half a byte of bases, a quality byte, the CIGAR's share) against the HBM
rate a streaming kernel reaches.  Prints the table that profiles/bam_errors_phases.txt holds.

    python tools/errors_rate.py [--bases 100000000] [--depth 20] [--method errhmm] [--runs 3] [--dir DIR]
"""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_ACHIEVABLE_TBS = 6.3    # HBM3E of the MI355X: 8.0 TB/s specified, a float4 copy measures 6.29 TB/s
BYTES_PER_COLUMN = 4


def child(aln, fasta, runs):
    import pbsim3_amd as P
    with open(aln, "rb") as f:
        raw = f.read()
    with open(fasta, "rb") as f:
        lines = f.read().split(b"\n", 1)[1]
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        for k in range(runs + 1):
            t = time.perf_counter()
            result, report = c.bam_errors(raw, [("g", lines)], ref_names=["g"])
            sys.stderr.write("[wall] %.1f ms\n" % ((time.perf_counter() - t) * 1e3))
        sys.stdout.write("\n".join(report.decode().split("\n")[:22]) + "\n")
        for k in range(runs + 1):
            c.bam_stats(raw)
    assert result["counts"]["nm_agree"] == result["counts"]["records"] > 0


def table(rows):
    for name in rows[0]:
        v = [c.get(name, float("nan")) for c in rows[1:]]
        print("  %-28s" % name + "".join("%10.2f" % x for x in v) + "   median %9.2f   spread %8.2f" % (statistics.median(v), max(v) - min(v)))
    return {name: statistics.median([c.get(name, float("nan")) for c in rows[1:]]) for name in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=100_000_000)
    ap.add_argument("--depth", default="20")
    ap.add_argument("--method", default="errhmm", choices=["errhmm", "qshmm"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.runs)
    import numpy as np
    import harness
    work = a.dir or tempfile.mkdtemp(prefix="pbsim_errors_", dir="/dev/shm" if os.access("/dev/shm", os.W_OK) else None)
    os.makedirs(work, exist_ok=True)
    fa = os.path.join(work, "g.fa")
    t = time.time()
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, a.bases)]
    pad = (-a.bases) % 80
    lines = np.concatenate([seq, np.full(pad, ord("A"), np.uint8)]).reshape(-1, 80)
    with open(fa, "wb") as f:
        f.write(b">g\n")
        f.write(np.concatenate([lines, np.full((len(lines), 1), 10, np.uint8)], axis=1).tobytes())
    cli = os.path.join(ROOT, "pbsim3_amd", "bin", "pbsim")
    model = ["--method", "errhmm", "--errhmm", harness.model_path("ERRHMM-ONT.model")] if a.method == "errhmm" else \
        ["--method", "qshmm", "--qshmm", harness.model_path("QSHMM-ONT.model")]
    cmd = [cli, "--strategy", "wgs"] + model + ["--genome", fa, "--depth", a.depth, "--seed", "1", "--prefix", os.path.join(work, "out"),
                                                "--truth-format", "bam"]
    subprocess.run(cmd, check=True, cwd=work, capture_output=True, timeout=900)
    aln = os.path.join(work, "out_0001.aln.bam")
    print("input: %d uniform bases x depth %s, %s, --truth-format bam: %s, %d bytes BGZF, made in %.0f s"
          % (a.bases, a.depth, model[2][2:].upper() + "-ONT", os.path.basename(aln), os.path.getsize(aln), time.time() - t))
    sys.stdout.flush()
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", aln, fa, "--runs", str(a.runs)], capture_output=True, text=True,
                       env=dict(os.environ, PBSIM_TRACE="1"), timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        return 1
    errors, stats, cur, size = [], [], {}, ""
    for line in p.stderr.splitlines():
        m = re.match(r"\[pbsim (errors|stats)\]\s+([0-9.]+) ms  (.*)", line)
        if m and m.group(3).startswith("total"):
            cur["total"] = float(m.group(2))
            if m.group(1) == "stats":
                stats.append(cur)
                cur = {}
            else:
                size = m.group(3)
        elif m:
            cur[m.group(3)] = float(m.group(2))
        m = re.match(r"\[wall\] ([0-9.]+) ms", line)
        if m:
            cur["wall of the call"] = float(m.group(1))
            errors.append(cur)
            cur = {}
    print("Context.bam_errors, without the per-read text, %s" % size)
    print(" warm-up call: " + ", ".join("%s %.1f" % kv for kv in errors[0].items()))
    print(" ms per phase (HIP events on the stage's stream), calls 1-%d after the warm-up, median, max - min" % a.runs)
    med = table(errors)
    print(p.stdout.rstrip())
    print("Context.bam_stats on the same bytes in the same process: ms per phase, calls 1-%d after the warm-up" % a.runs)
    med_stats = table(stats)
    cols = int(re.search(r"(\d+) columns", size).group(1))
    rate = cols / med["columns"] / 1e9
    print("the column pass takes %d columns in %.2f ms = %.3f T columns/s; at %d bytes per column %.2f TB/s, %.0f %% of the %.1f TB/s a streaming "
          "kernel reaches; the two walks over the CIGARs (records + segments) %.2f ms; the stage's inflate %.1f ms against stats's %.1f ms"
          % (cols, med["columns"], rate, BYTES_PER_COLUMN, rate * BYTES_PER_COLUMN, 100 * rate * BYTES_PER_COLUMN / HBM_ACHIEVABLE_TBS, HBM_ACHIEVABLE_TBS,
             med["records"] + med["segments"], med["inflate"], med_stats["inflate"]))
    if not a.dir:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
