"""The phases of `pbsim --depth-bam` on one MI355X: a truth BAM of product size (--bases uniform bases, depth 20, ERRHMM-ONT,
--truth-format bam, made here by the command line) through Context.bam_depth in one process: one warm-up call, then --runs calls
per format, the phases taken from the stage's own HIP events (PBSIM_TRACE).  Beside them the phases of `pbsim --sort-truth-bam` on
a copy of the file in fresh processes: the existing stage that inflates and locates the same bytes (its code is the parent
commit's).  From the phase times the scan pass and the runs pass as bytes moved over time.  Prints the table that
profiles/bam_depth_phases.txt holds.

    python tools/depth_rate.py [--bases 100000000] [--depth 20] [--runs 3] [--dir DIR]
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

HBM_PEAK_TBS = 8.0          # HBM3E of the MI355X, specified; a float4 copy measures 6.29 TB/s


def child(path, runs):
    import pbsim3_amd as P
    with open(path, "rb") as f:
        raw = f.read()
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        for kw in (dict(), dict(fmt="window", window=1000)):
            for k in range(runs + 1):
                t = time.perf_counter()
                text, counts, refs, hist, report = c.bam_depth(raw, **kw)
                sys.stderr.write("[wall] %.1f ms %s\n" % ((time.perf_counter() - t) * 1e3, kw.get("fmt", "bedgraph")))
            sys.stdout.write("%s: %d bytes of text\n%s\n" % (kw.get("fmt", "bedgraph"), len(text), report.decode()[:600]))
    assert counts["counted"] == counts["records"] > 0


def table(rows, runs):
    for name in rows[0]:
        v = [c.get(name, float("nan")) for c in rows[1:]]
        print("  %-28s" % name + "".join("%10.2f" % x for x in v) + "   median %9.2f   spread %8.2f" % (statistics.median(v), max(v) - min(v)))
    return {name: statistics.median([c.get(name, float("nan")) for c in rows[1:]]) for name in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=100_000_000)
    ap.add_argument("--depth", default="20")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.runs)
    import numpy as np
    import harness
    work = a.dir or tempfile.mkdtemp(prefix="pbsim_depth_", dir="/dev/shm" if os.access("/dev/shm", os.W_OK) else None)
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
    print("input: %d uniform bases x depth %s, ERRHMM-ONT, --truth-format bam: %s, %d bytes BGZF, made in %.0f s"
          % (a.bases, a.depth, os.path.basename(aln), os.path.getsize(aln), time.time() - t))
    sys.stdout.flush()
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", aln, "--runs", str(a.runs)], capture_output=True, text=True,
                       env=dict(os.environ, PBSIM_TRACE="1"), timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        return 1
    calls, cur, size = {"bedgraph": [], "window": []}, {}, {}
    for line in p.stderr.splitlines():
        m = re.match(r"\[pbsim depth\]\s+([0-9.]+) ms  (.*)", line)
        if m and m.group(2).startswith("total"):
            cur["total"] = float(m.group(1))
            cur_size = m.group(2)
        elif m:
            cur[m.group(2)] = float(m.group(1))
        m = re.match(r"\[wall\] ([0-9.]+) ms (\w+)", line)
        if m:
            cur["wall of the call"] = float(m.group(1))
            calls[m.group(2)].append(cur)
            size[m.group(2)] = cur_size
            cur = {}
    med = {}
    for fmt in ("bedgraph", "window"):
        print("Context.bam_depth, %s%s, %s" % (fmt, " (windows of 1000)" if fmt == "window" else "", size[fmt]))
        print(" warm-up call: " + ", ".join("%s %.1f" % kv for kv in calls[fmt][0].items()))
        print(" ms per phase (HIP events on the stage's stream), calls 1-%d after the warm-up, median, max - min" % a.runs)
        med[fmt] = table(calls[fmt], a.runs)
    print(p.stdout.rstrip())
    slots = int(re.search(r"(\d+) reference positions", size["bedgraph"]).group(1)) + 1
    for fmt, passes in (("bedgraph", 2), ("window", 1)):
        scan_b, runs_b = 8 * slots, 4 * slots * passes
        print("%s: the scan pass reads and writes 4 bytes per slot: %.3f GB in %.2f ms = %.2f TB/s; the runs pass reads them %s: %.3f GB in "
              "%.2f ms = %.2f TB/s (its outputs not counted); HBM peak %.1f TB/s"
              % (fmt, scan_b / 1e9, med[fmt]["scan"], scan_b / med[fmt]["scan"] / 1e9, "twice (counts, then the runs)" if passes == 2 else "once",
                 runs_b / 1e9, med[fmt]["runs"], runs_b / med[fmt]["runs"] / 1e9, HBM_PEAK_TBS))
    # ---- the sort of a copy, fresh processes: the stage that inflates and locates the same bytes
    env = dict(os.environ, PBSIM_TRACE="1")
    so, de = [], []
    for k in range(a.runs + 1):
        copy = os.path.join(work, "copy.aln.bam")
        shutil.copy(aln, copy)
        r = subprocess.run([cli, "--sort-truth-bam", copy], capture_output=True, text=True, env=env, cwd=work, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            return 1
        so.append({m.group(2).strip(): float(m.group(1)) for m in re.finditer(r"\[pbsim sort\]\s+([0-9.]+) ms  ([a-z +]+?)(?:\s{2,}.*)?$", r.stderr, re.M)})
        r = subprocess.run([cli, "--depth-bam", aln, "--depth-out", os.path.join(work, "depth.bedgraph")], capture_output=True, text=True, env=env,
                           cwd=work, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            return 1
        de.append({m.group(2).split(":")[0]: float(m.group(1)) for m in re.finditer(r"\[pbsim depth\]\s+([0-9.]+) ms  (.*)", r.stderr)})
    print("fresh processes, PBSIM_TRACE=1, alternating, run 0 a warm-up of the page cache: ms per phase, runs 1-%d, median, max - min" % a.runs)
    for label, rows in (("pbsim --depth-bam F --depth-out OUT (HIP events)", de), ("pbsim --sort-truth-bam COPY (host clock)", so)):
        print(" " + label)
        table(rows, a.runs)
    if not a.dir:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
