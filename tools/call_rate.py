"""The phases of `pbsim --call-bam` on one MI355X beside those of `pbsim --consensus-bam` on the same bytes in the same warm process:
the truth BAM of product size that tools/pileup_rate.py builds (--bases uniform bases, depth 20, --method errhmm with ERRHMM-ONT
or qshmm with QSHMM-ONT, --truth-format bam, made here by the command line) through Context.bam_call without the text, then with
it, then through Context.bam_consensus with its text: one warm-up call each, then --runs calls, the phases taken from the stages'
own HIP events (PBSIM_TRACE).  The two new passes -- lines (the groups' sizes, the counts, the tiles' scan) and text (the same
walk, writing) -- stand beside the consensus's bases and text passes of the same run: the same lanes and tiles, and on the path
nearly every lane takes the class bytes alone.  Prints the table that profiles/bam_call_phases.txt holds.

    python tools/call_rate.py [--bases 100000000] [--depth 20] [--method errhmm] [--runs 3] [--dir DIR]
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

LINE_BYTES = 3              # a lane of the line pass reads its class byte and its two neighbours' (one cache line); 8 bytes per tile written
CONS_BYTES = 1              # the consensus's base pass reads a class byte per position


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
                got = c.bam_call(raw, [("g", lines)], ref_names=["g"], text=text)
                sys.stderr.write("[wall %s] %.1f ms\n" % ("text" if text else "bare", (time.perf_counter() - t) * 1e3))
        result, report, vcf, records = got
        for k in range(runs + 1):
            t = time.perf_counter()
            cons, _, fasta_text, _ = c.bam_consensus(raw, [("g", lines)], ref_names=["g"], fill="ref", line_width=0)
            sys.stderr.write("[wall consensus] %.1f ms\n" % ((time.perf_counter() - t) * 1e3))
    assert result["counts"] == cons["counts"] and result["sites"] == cons["sites"] and result["max_depth"] == cons["max_depth"]
    assert result["text_bytes"] == len(vcf) and records == [(len(lines.replace(b"\n", b"")), result["variants"])]
    # the records applied to the genome give the consensus with fill ref
    genome, out, at = lines.replace(b"\n", b""), [], 0
    for line in vcf[result["header_bytes"]:].split(b"\n")[:-1]:
        f = line.split(b"\t")
        pos = int(f[1]) - 1
        assert pos >= at and genome[pos:pos + len(f[3])] == f[3]
        out += [genome[at:pos], f[4]]
        at = pos + len(f[3])
    out.append(genome[at:])
    sys.stdout.write(report.decode())
    sys.stdout.write("%d records, %d bytes of VCF of which %d header; applied to the genome they give the consensus with fill ref: %s\n"
                     % (result["variants"], len(vcf), result["header_bytes"], b"".join(out) == fasta_text.split(b"\n")[1]))


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
    work = a.dir or tempfile.mkdtemp(prefix="pbsim_call_", dir="/dev/shm" if os.access("/dev/shm", os.W_OK) else None)
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
    calls, cur, size = {"bare": [], "text": [], "consensus": []}, {}, {}
    for line in p.stderr.splitlines():
        m = re.match(r"\[pbsim (call|consensus)\]\s+([0-9.]+) ms  (.*)", line)
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
    print("Context.bam_call, %s" % size["call"])
    print(" ms per phase (HIP events on the stage's stream), calls 1-%d after the warm-up, median, max - min; without the text:" % a.runs)
    bare = table(calls["bare"])
    print(" with the text (the VCF through 8 MB pieces into a Python callback):")
    text = table(calls["text"])
    print(p.stdout.rstrip())
    print("Context.bam_consensus (fill ref, one line, with its text) on the same bytes in the same process, %s" % size["consensus"])
    cons = table(calls["consensus"])
    sites = int(re.search(r"(\d+) positions", size["call"]).group(1))
    variants = int(re.search(r"(\d+) variants", size["call"]).group(1))
    n_text = float(re.search(r"([0-9.]+) MB of text", size["call"]).group(1)) * 1e6
    print("the line passes: lines (sizes, counts, the tiles' scan) %.2f ms: %.1f GB/s at %d class bytes per position, 8 bytes per tile written; text "
          "(the same walk, writing) %.2f ms for %d records, %.0f bytes of VCF"
          % (bare["lines"], sites * LINE_BYTES / bare["lines"] / 1e6, LINE_BYTES, text["text"], variants, n_text))
    print("the consensus's passes in the same run: bases (sizes, counts, the scan, the records' places) %.2f ms at %d class byte per position; text "
          "(fill) %.2f ms: lines / bases %.2f x, text / text %.2f x; the call stage's own bases (the sizes alone, no scan) %.2f ms"
          % (cons["bases"], CONS_BYTES, cons["text"], bare["lines"] / cons["bases"], text["text"] / cons["text"], bare["bases"]))
    print("total without the text %.2f ms, with it %.2f ms, against the consensus's %.2f ms with its text: %+.2f ms"
          % (bare["total"], text["total"], cons["total"], text["total"] - cons["total"]))
    if not a.dir:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
