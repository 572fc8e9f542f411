"""A/B of `pbsim --sort-truth-bam` (GPU box): this tree's CLI against another build's (the parent commit's), on one truth BAM
of about 2 GB inflated made with this tree's CLI; a warm-up round, then five sorts by each, alternating, under PBSIM_TRACE=1.
Prints the phase clocks of every run, their medians and spreads, whether each median of this tree lies within the other
build's spread (max - min), and whether the sorted files and indices are the same bytes.
usage: python tools/closed_ab/bam_scan_ab.py --parent-cli PATH [--out FILE]      (profiles/bam_scan_unified_ab.txt)"""
import argparse, hashlib, os, re, shutil, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import harness
ap = argparse.ArgumentParser()
ap.add_argument("--parent-cli", required=True)
ap.add_argument("--out")
a = ap.parse_args()
CLI = {"this": os.path.join(ROOT, "pbsim3_amd", "bin", "pbsim"), "parent": os.path.abspath(a.parent_cli)}
lines = []
def say(s=""):
    print(s, flush=True); lines.append(s)
    if a.out:
        with open(a.out, "w") as f: f.write("\n".join(lines) + "\n")
def run(cmd, limit, **kw):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, **kw)
    if p.returncode != 0:
        say("FAILED (%d): %s\n%s" % (p.returncode, " ".join(cmd), p.stderr[-3000:])); sys.exit(1)
    return p
with tempfile.TemporaryDirectory(dir="/dev/shm") as d:
    bp = 50_000_000
    rng = np.random.default_rng(1)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, bp)].reshape(-1, 80)
    with open(os.path.join(d, "g.fa"), "wb") as f:
        f.write(b">chr1\n" + np.concatenate([s, np.full((s.shape[0], 1), 10, np.uint8)], axis=1).tobytes())
    model = harness.model_path("ERRHMM-ONT.model")
    args = ["--strategy", "wgs", "--method", "errhmm", "--errhmm", model, "--genome", os.path.join(d, "g.fa"), "--depth", "20", "--seed", "1",
            "--prefix", os.path.join(d, "out"), "--truth-format", "bam"]
    say("input: pbsim " + " ".join(a.replace(d, "DIR").replace(os.path.dirname(model), "MODELS") for a in args))
    say("       g.fa: one record of 50 000 000 uniform bases, numpy default_rng(1), 80 per line (the benchmark's sample genome)")
    t0 = time.time(); run([CLI["this"]] + args, 900, cwd=d)
    alns = sorted(n for n in os.listdir(d) if n.endswith(".aln.bam"))
    src = os.path.join(d, alns[0])
    say("       %s: %d bytes BGZF, made in %.0f s" % (alns[0], os.path.getsize(src), time.time() - t0))
    work = os.path.join(d, "w.aln.bam")
    res = {"this": [], "parent": []}; digest = {}
    for r in range(6):                       # round 0 warms both up (code objects, page cache) and is not counted
        for tag in ("this", "parent"):
            shutil.copyfile(src, work)
            p = run([CLI[tag], "--sort-truth-bam", work], 600, cwd=d, env=dict(os.environ, PBSIM_TRACE="1"))
            ph = {m.group(2).strip(): float(m.group(1)) for m in re.finditer(r"\[pbsim sort\] +([0-9.]+) ms  ([a-z ]+?) *(?:  [^\n]*)?$", p.stderr, re.M)}
            mb = re.search(r"inflate\s+([0-9.]+) MB", p.stderr)
            h = hashlib.sha256()
            for n in (work, work + ".csi"):
                with open(n, "rb") as f: h.update(f.read())
            os.remove(work + ".csi")
            digest.setdefault(tag, set()).add(h.hexdigest())
            if r == 0:
                say("warm-up %s: inflated stream %s MB; phases %s" % (tag, mb.group(1) if mb else "?", ph))
            else:
                res[tag].append(ph)
    keys = ["inflate", "scan", "chain", "keys and sort", "gather", "deflate and deliver", "index", "total"]
    for tag in ("parent", "this"):
        say(); say("%s, ms per phase, runs 1-5 (alternating with the other), median, max - min" % tag)
        for k in keys:
            v = [x.get(k, float("nan")) for x in res[tag]]
            say("  %-20s %s   median %9.1f   spread %7.1f" % (k, " ".join("%9.1f" % x for x in v), statistics.median(v), max(v) - min(v)))
    say(); say("verdict (median of this <= median of parent + parent's spread):")
    for k in ("scan", "chain", "keys and sort", "gather", "total"):
        t = [x[k] for x in res["this"]]; b = [x[k] for x in res["parent"]]
        ok = statistics.median(t) <= statistics.median(b) + (max(b) - min(b))
        say("  %-20s this %9.1f  parent %9.1f + %7.1f  %s" % (k, statistics.median(t), statistics.median(b), max(b) - min(b), "inside" if ok else "OUTSIDE"))
    say(); say("sorted BAM + CSI, sha256 over all runs: this %s, parent %s -> %s" % (sorted(digest["this"]), sorted(digest["parent"]),
        "identical" if digest["this"] == digest["parent"] and len(digest["this"]) == 1 else "DIFFERENT"))
