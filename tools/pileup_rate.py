"""The phases of `pbsim --pileup-bam` on one MI355X: the truth BAM of product size that tools/errors_rate.py builds (--bases uniform
bases, depth 20, --method errhmm with ERRHMM-ONT or qshmm with QSHMM-ONT, --truth-format bam, made here by the command line) through
Context.bam_pileup in one process: one warm-up call, then --runs calls, the phases taken from the stage's own HIP events
(PBSIM_TRACE).  Beside them, in the same warm process, the phases of Context.bam_errors on the same bytes: its column pass walks the
same segments and tallies into LDS where the pileup's issues one global atomic per column.  From the phase times: the column pass
against k_err_columns, the atomics as added bytes per second (4 per M = X D column) against the chip-wide rate the guide gives for
float atomics, and the site pass at 34 bytes per position (32 of cells, a genome byte, a class byte; a class byte written) against
the HBM rate a streaming kernel reaches.  Prints the table that profiles/bam_pileup_phases.txt holds.

    python tools/pileup_rate.py [--bases 100000000] [--depth 20] [--method errhmm] [--runs 3] [--dir DIR]
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
ATOMIC_TBS = 1.3            # global float atomic adds, chip-wide, in added bytes: measured for f32 in 256-byte wave instructions
BYTES_PER_SITE = 34


def child(aln, fasta, runs):
    import pbsim3_amd as P
    with open(aln, "rb") as f:
        raw = f.read()
    with open(fasta, "rb") as f:
        lines = f.read().split(b"\n", 1)[1]
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        for k in range(runs + 1):
            t = time.perf_counter()
            result, report = c.bam_pileup(raw, [("g", lines)], ref_names=["g"])
            sys.stderr.write("[wall] %.1f ms\n" % ((time.perf_counter() - t) * 1e3))
        sys.stdout.write(report.decode())
        for k in range(runs + 1):
            errors, _ = c.bam_errors(raw, [("g", lines)], ref_names=["g"])
    sums = result["cell_sums"]
    assert result["counts"]["scored"] == result["counts"]["records"] > 0
    assert sum(sums[k] for k in ("A", "C", "G", "T", "other")) == sum(errors["pair"]) and sums["del"] == errors["totals"]["del"]
    assert sums["ins"] + result["ins_unanchored"] == errors["totals"]["ins_events"]
    sys.stdout.write("atomics %d\n" % sum(sums.values()))          # every addition to a cell of the table is one atomic


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
    work = a.dir or tempfile.mkdtemp(prefix="pbsim_pileup_", dir="/dev/shm" if os.access("/dev/shm", os.W_OK) else None)
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
    calls, cur, size = {"pileup": [], "errors": []}, {}, {}
    for line in p.stderr.splitlines():
        m = re.match(r"\[pbsim (pileup|errors)\]\s+([0-9.]+) ms  (.*)", line)
        if m and m.group(3).startswith("total"):
            cur["total"] = float(m.group(2))
            size[m.group(1)] = m.group(3)
            if m.group(1) == "errors":
                calls["errors"].append(cur)
                cur = {}
        elif m:
            cur[m.group(3)] = cur.get(m.group(3), 0.0) + float(m.group(2))
        m = re.match(r"\[wall\] ([0-9.]+) ms", line)
        if m:
            cur["wall of the call"] = float(m.group(1))
            calls["pileup"].append(cur)
            cur = {}
    print("Context.bam_pileup, without the text and the cells, %s" % size["pileup"])
    print(" warm-up call: " + ", ".join("%s %.1f" % kv for kv in calls["pileup"][0].items()))
    print(" ms per phase (HIP events on the stage's stream), calls 1-%d after the warm-up, median, max - min" % a.runs)
    med = table(calls["pileup"])
    out = p.stdout.rstrip().split("\n")
    print("\n".join(out[:-1]))
    print("Context.bam_errors on the same bytes in the same process, %s" % size["errors"])
    print(" ms per phase, calls 1-%d after the warm-up" % a.runs)
    med_errors = table(calls["errors"])
    atomics = int(out[-1].split()[1])
    sites = int(re.search(r"(\d+) positions", size["pileup"]).group(1))
    cols = int(re.search(r"(\d+) columns", size["errors"]).group(1))
    rate = atomics * 4 / med["columns"] / 1e9
    print("the column pass issues %d atomics (one per M = X D column and per anchored I op; the errors stage walks %d columns, the inserted bases "
          "among them) in %.2f ms against k_err_columns' %.2f ms on the same segments: %.2f x; %.3f TB/s of added bytes (4 per atomic), %.0f %% of "
          "the %.1f TB/s the guide gives chip-wide for float atomics in 256-byte wave instructions"
          % (atomics, cols, med["columns"], med_errors["columns"], med["columns"] / med_errors["columns"], rate, 100 * rate / ATOMIC_TBS, ATOMIC_TBS))
    site_rate = sites * BYTES_PER_SITE / med["sites"] / 1e9
    print("the site pass takes %d positions in %.2f ms: at %d bytes per position %.2f TB/s, %.0f %% of the %.1f TB/s a streaming kernel reaches; "
          "zeroing the table (32 bytes per position) %.2f ms"
          % (sites, med["sites"], BYTES_PER_SITE, site_rate, 100 * site_rate / HBM_ACHIEVABLE_TBS, HBM_ACHIEVABLE_TBS, med["zero"]))
    if not a.dir:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
