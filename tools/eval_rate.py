"""The phases of `pbsim --eval-bam` on one MI355X: a truth BAM of about 2 GB inflated (the job of profiles/bam_scan_unified_ab.txt:
50 000 000 uniform bases, depth 20, ERRHMM-ONT, --truth-format bam) evaluated against itself, in one process: one warm-up call,
then --runs calls, the phases taken from the stage's own HIP events (PBSIM_TRACE).  Then the same through fresh processes of
the command line, alternating with `pbsim --sort-truth-bam` on a copy of the file: the sort's scan and chain phases are the
yardstick of the evaluation's scan + chain, since the kernel is the same.  Prints the table that profiles/bam_eval_phases.txt holds.

    python tools/eval_rate.py [--bases 50000000] [--depth 20] [--runs 5] [--dir DIR]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def child(path, runs):
    import pbsim3_amd as P
    with open(path, "rb") as f:
        raw = f.read()
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        for k in range(runs + 1):
            t = time.perf_counter()
            counts, hist, report = c.eval_bam(raw, raw)
            sys.stderr.write("[wall] %.1f ms\n" % ((time.perf_counter() - t) * 1e3))
    sys.stdout.write(report.decode())
    assert counts["correct"] == counts["truth_records"] == counts["query_records"] > 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=50_000_000)
    ap.add_argument("--depth", default="20")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.runs)
    import numpy as np
    import harness
    work = a.dir or tempfile.mkdtemp(prefix="pbsim_eval_", dir="/dev/shm" if os.access("/dev/shm", os.W_OK) else None)
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
    cmd = [cli, "--strategy", "wgs", "--method", "errhmm", "--errhmm", harness.model_path("ERRHMM-ONT.model"), "--genome", fa, "--depth", a.depth,
           "--seed", "1", "--prefix", os.path.join(work, "out"), "--truth-format", "bam"]
    subprocess.run(cmd, check=True, cwd=work, capture_output=True, timeout=900)
    aln = os.path.join(work, "out_0001.aln.bam")
    print("input: %d uniform bases x depth %s, ERRHMM-ONT, --truth-format bam: %s, %d bytes BGZF, made in %.0f s; evaluated against itself"
          % (a.bases, a.depth, os.path.basename(aln), os.path.getsize(aln), time.time() - t))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", aln, "--runs", str(a.runs)], capture_output=True, text=True,
                       env=dict(os.environ, PBSIM_TRACE="1"), timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        return 1
    calls, cur = [], {}
    for line in p.stderr.splitlines():
        m = re.match(r"\[pbsim eval\]\s+([0-9.]+) ms  (.*)", line)
        if m and m.group(2).startswith("total"):
            cur["total"] = float(m.group(1))
            size = m.group(2)
        elif m:
            cur[m.group(2)] = float(m.group(1))
        m = re.match(r"\[wall\] ([0-9.]+) ms", line)
        if m:
            cur["wall of the call (with the copies ctypes makes)"] = float(m.group(1))
            calls.append(cur)
            cur = {}
    print(size)
    print("warm-up call: " + ", ".join("%s %.1f" % kv for kv in calls[0].items()))
    print("ms per phase (HIP events on the stage's stream), calls 1-%d after the warm-up, median, max - min" % a.runs)
    for name in calls[0]:
        v = [c[name] for c in calls[1:]]
        print("  %-52s" % name + "".join("%9.1f" % x for x in v) + "   median %8.1f   spread %7.1f" % (statistics.median(v), max(v) - min(v)))
    print(p.stdout.rstrip())
    # ---- fresh processes: the command line, alternating with the sort of a copy
    import shutil
    env = dict(os.environ, PBSIM_TRACE="1")
    ev, so = [], []
    for k in range(a.runs + 1):
        r = subprocess.run([cli, "--eval-bam", aln, "--truth-bam", aln, "--eval-out", os.path.join(work, "report.txt")], capture_output=True, text=True,
                           env=env, cwd=work, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            return 1
        ev.append({m.group(2).split(":")[0]: float(m.group(1)) for m in re.finditer(r"\[pbsim eval\]\s+([0-9.]+) ms  (.*)", r.stderr)})
        copy = os.path.join(work, "copy.aln.bam")
        shutil.copy(aln, copy)
        r = subprocess.run([cli, "--sort-truth-bam", copy], capture_output=True, text=True, env=env, cwd=work, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            return 1
        so.append({m.group(2).strip(): float(m.group(1)) for m in re.finditer(r"\[pbsim sort\]\s+([0-9.]+) ms  ([a-z +]+?)(?:\s{2,}.*)?$", r.stderr, re.M)})
    print("fresh processes, PBSIM_TRACE=1, alternating, run 0 a warm-up of the page cache: ms per phase, runs 1-%d, median, max - min" % a.runs)
    for label, rows in (("pbsim --eval-bam F --truth-bam F", ev), ("pbsim --sort-truth-bam COPY", so)):
        print(" " + label)
        for name in rows[0]:
            v = [c.get(name, float("nan")) for c in rows[1:]]
            print("  %-52s" % name + "".join("%9.1f" % x for x in v) + "   median %8.1f   spread %7.1f" % (statistics.median(v), max(v) - min(v)))
    if not a.dir:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
