"""The phases of `pbsim --consensus-bam` on one MI355X beside those of `pbsim --pileup-bam` on the same bytes in the same warm
process: the truth BAM of product size that tools/pileup_rate.py builds (--bases uniform bases, depth 20, --method errhmm with
ERRHMM-ONT or qshmm with QSHMM-ONT, --truth-format bam, made here by the command line) through Context.bam_consensus without the
text, then with it, then through Context.bam_pileup: one warm-up call each, then --runs calls, the phases taken from the stages'
own HIP events (PBSIM_TRACE).  From the phase times: the column pass with the log against the pileup's without it, the log's
entries and bytes, the insertion passes (slots, lengths, tally) per entry, and the two FASTA passes (bases, text) in GB/s of what
they read and write.  Prints the table that profiles/bam_consensus_phases.txt holds.

    python tools/consensus_rate.py [--bases 100000000] [--depth 20] [--method errhmm] [--runs 3] [--dir DIR]
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

BASE_SIZES_BYTES = 1        # the base pass reads a class byte per position; the table's 32 bytes and the cells only at an ins_site
BASE_FILL_BYTES = 2         # the fill pass reads a class byte and writes about a base


def child(aln, fasta, runs):
    import pbsim3_amd as P
    with open(aln, "rb") as f:
        raw = f.read()
    with open(fasta, "rb") as f:
        lines = f.read().split(b"\n", 1)[1]
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        for text in (False, True):
            for k in range(runs + 1):
                t = time.perf_counter()
                got = c.bam_consensus(raw, [("g", lines)], ref_names=["g"], text=text)
                sys.stderr.write("[wall %s] %.1f ms\n" % ("text" if text else "bare", (time.perf_counter() - t) * 1e3))
        result, report, fasta_text, lengths = got
        for k in range(runs + 1):
            t = time.perf_counter()
            pile, _ = c.bam_pileup(raw, [("g", lines)], ref_names=["g"])
            sys.stderr.write("[wall pileup] %.1f ms\n" % ((time.perf_counter() - t) * 1e3))
    assert result["counts"] == pile["counts"] and result["sites"] == pile["sites"] and result["max_depth"] == pile["max_depth"]
    assert result["text_bytes"] == len(fasta_text) and result["ins_sites"] == pile["sites"]["ins_site"]
    genome = lines.replace(b"\n", b"")
    cons = b"".join(fasta_text.split(b"\n")[1:])
    sys.stdout.write(report.decode())
    sys.stdout.write("consensus %d bases for %d of the genome, %d of them differ in count; equal to the genome: %s\n"
                     % (len(cons), len(genome), abs(len(cons) - len(genome)), cons == genome))


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
    work = a.dir or tempfile.mkdtemp(prefix="pbsim_consensus_", dir="/dev/shm" if os.access("/dev/shm", os.W_OK) else None)
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
    calls, cur, size = {"bare": [], "text": [], "pileup": []}, {}, {}
    for line in p.stderr.splitlines():
        m = re.match(r"\[pbsim (consensus|pileup)\]\s+([0-9.]+) ms  (.*)", line)
        if m and m.group(3).startswith("total"):
            cur["total"] = float(m.group(2))
            size[m.group(1)] = m.group(3)
        elif m:
            cur[m.group(3)] = cur.get(m.group(3), 0.0) + float(m.group(2))
        m = re.match(r"\[wall (\w+)\] ([0-9.]+) ms", line)
        if m:
            cur["wall of the call"] = float(m.group(2))
            calls[m.group(1)].append(cur)
            cur = {}

    def table(rows):
        names = list(rows[0])
        for name in names:
            v = [c.get(name, float("nan")) for c in rows[1:]]
            print("  %-28s" % name + "".join("%10.2f" % x for x in v) + "   median %9.2f   spread %8.2f" % (statistics.median(v), max(v) - min(v)))
        return {name: statistics.median([c.get(name, float("nan")) for c in rows[1:]]) for name in names}
    print("Context.bam_consensus, %s" % size["consensus"])
    print(" ms per phase (HIP events on the stage's stream), calls 1-%d after the warm-up, median, max - min; without the text:" % a.runs)
    bare = table(calls["bare"])
    print(" with the text (the FASTA through 8 MB pieces into a Python callback):")
    text = table(calls["text"])
    print(p.stdout.rstrip())
    print("Context.bam_pileup on the same bytes in the same process, %s" % size["pileup"])
    pile = table(calls["pileup"])
    entries = int(re.search(r"(\d+) log entries", size["consensus"]).group(1))
    sites = int(re.search(r"(\d+) positions", size["consensus"]).group(1))
    slots = int(re.search(r"(\d+) ins_sites", size["consensus"]).group(1))
    n_text = float(re.search(r"([0-9.]+) MB of text", size["consensus"]).group(1)) * 1e6
    print("the column pass with the log %.2f ms, the pileup's without it %.2f ms: %+.2f ms (%.2f x) for %d entries, %.1f MB at 8 bytes each"
          % (bare["columns"], pile["columns"], bare["columns"] - pile["columns"], bare["columns"] / pile["columns"], entries, entries * 8 / 1e6))
    ins = bare.get("slots", 0.0) + bare.get("lengths", 0.0) + bare.get("tally", 0.0)
    print("the insertion tally: slots %.2f + lengths %.2f + tally %.2f = %.2f ms for %d ins_sites; the two passes over the log read %.1f MB each: "
          "%.1f GB/s and %.1f GB/s" % (bare.get("slots", 0.0), bare.get("lengths", 0.0), bare.get("tally", 0.0), ins, slots, entries * 8 / 1e6,
                                      entries * 8 / max(bare.get("lengths", 1e-9), 1e-9) / 1e6, entries * 8 / max(bare.get("tally", 1e-9), 1e-9) / 1e6))
    print("the FASTA passes: bases (sizes, counts, the tiles' scan) %.2f ms: %.1f GB/s at %d bytes per position; text (fill) %.2f ms: %.1f GB/s at %d "
          "bytes per position read plus %.0f bytes written"
          % (bare["bases"], sites * BASE_SIZES_BYTES / bare["bases"] / 1e6, BASE_SIZES_BYTES, text["text"],
             (sites * (BASE_FILL_BYTES - 1) + n_text) / text["text"] / 1e6, BASE_FILL_BYTES - 1, n_text))
    print("total without the text %.2f ms against the pileup's %.2f ms: %+.2f ms" % (bare["total"], pile["total"], bare["total"] - pile["total"]))
    if not a.dir:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
