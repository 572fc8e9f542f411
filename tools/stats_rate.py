"""The phases of `pbsim --stats-bam` on one MI355X: a truth BAM of product size (--bases uniform bases, depth 20, --method errhmm
with ERRHMM-ONT or qshmm with QSHMM-ONT, --truth-format bam, made here by the command line) through Context.bam_stats in one
process: one warm-up call, then --runs calls without the per-read text and --runs with it, the phases taken from the stage's own
HIP events (PBSIM_TRACE).  Beside them, in the same warm process, the phases of Context.bam_depth on the same bytes: the existing
stage that inflates and locates them, its inflate time the yardstick.  From the phase times the quality pass as bytes read over
time, against the HBM rate a streaming kernel reaches.  Prints the table that profiles/bam_stats_phases.txt holds.

    python tools/stats_rate.py [--bases 100000000] [--depth 20] [--method errhmm] [--runs 3] [--dir DIR]
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


def child(path, runs):
    import pbsim3_amd as P
    with open(path, "rb") as f:
        raw = f.read()
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        for text in (False, True):
            for k in range(runs + 1):
                t = time.perf_counter()
                out = c.bam_stats(raw, text=text)
                sys.stderr.write("[wall] %.1f ms %s\n" % ((time.perf_counter() - t) * 1e3, "text" if text else "plain"))
            sys.stdout.write("%s: %d bytes of text\n" % ("text" if text else "plain", len(out[7]) if text else 0))
        sys.stdout.write(out[6].decode()[:700] + "\n")
        for k in range(runs + 1):
            c.bam_depth(raw)
    assert out[0]["scored"] == out[0]["records"] > 0


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
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.runs)
    import numpy as np
    import harness
    work = a.dir or tempfile.mkdtemp(prefix="pbsim_stats_", dir="/dev/shm" if os.access("/dev/shm", os.W_OK) else None)
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
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", aln, "--runs", str(a.runs)], capture_output=True, text=True,
                       env=dict(os.environ, PBSIM_TRACE="1"), timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        return 1
    calls, depth, cur, size = {"plain": [], "text": []}, [], {}, {}
    for line in p.stderr.splitlines():
        m = re.match(r"\[pbsim (stats|depth)\]\s+([0-9.]+) ms  (.*)", line)
        if m and m.group(3).startswith("total"):
            cur["total"] = float(m.group(2))
            cur_size = m.group(3)
            if m.group(1) == "depth":
                depth.append(cur)
                cur = {}
        elif m:
            cur[m.group(3)] = float(m.group(2))
        m = re.match(r"\[wall\] ([0-9.]+) ms (\w+)", line)
        if m:
            cur["wall of the call"] = float(m.group(1))
            calls[m.group(2)].append(cur)
            size[m.group(2)] = cur_size
            cur = {}
    med = {}
    for kind in ("plain", "text"):
        print("Context.bam_stats, %s, %s" % ("with the per-read text" if kind == "text" else "without the per-read text", size[kind]))
        print(" warm-up call: " + ", ".join("%s %.1f" % kv for kv in calls[kind][0].items()))
        print(" ms per phase (HIP events on the stage's stream), calls 1-%d after the warm-up, median, max - min" % a.runs)
        med[kind] = table(calls[kind])
    print(p.stdout.rstrip())
    print("Context.bam_depth (bedgraph) on the same bytes in the same process, the yardstick: ms per phase, calls 1-%d after the warm-up" % a.runs)
    med_depth = table(depth)
    q_bytes = int(re.search(r"(\d+) quality bytes", size["plain"]).group(1))
    inflated = float(re.search(r"([0-9.]+) MB inflated", size["plain"]).group(1)) * 1e6
    rate = q_bytes / med["plain"]["quals"] / 1e9
    print("the quality pass reads %.3f GB of quality bytes (%.0f %% of the %.3f GB inflated) in %.2f ms = %.2f TB/s, %.0f %% of the %.1f TB/s a "
          "streaming kernel reaches; the stage's inflate %.1f ms against depth's %.1f ms"
          % (q_bytes / 1e9, 100 * q_bytes / inflated, inflated / 1e9, med["plain"]["quals"], rate, 100 * rate / HBM_ACHIEVABLE_TBS, HBM_ACHIEVABLE_TBS,
             med["plain"]["inflate"], med_depth["inflate"]))
    if not a.dir:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
