"""Measures the sampling method's input side (GPU box): a --sample FASTQ of N strings (the generator of tools/e2e_sample.sh:
gamma lengths, mean 9 000, clipped to 100 .. 60 000; 100 000 strings = 1.8 GB, the file of DESIGN 8c) in /dev/shm, then
  - the floor: the file's bytes pinned host -> device in one copy (torch), GB/s, best of three;
  - "profile ready in HBM" through the library: Context.load_sample_fastq (the GPU builder: upload + line table + sums + pool),
    and the same from bytes already in HBM (a uint8 tensor); wall time per call, the first call and the best of the rest
    (the host route it replaces has no entry point of its own: it is timed through the parent's CLI below);
  - the CLI's PBSIM_TRACE phase clock around `pbsim --method sample` on a small genome, for this build and -- with
    --parent-cli -- for another build's binary (the parent commit's), alternated, --rounds times;
  - with --rocprof DIR: one load_sample_fastq in a child of its own under `rocprofv3 --kernel-trace --memory-copy-trace --stats`,
    for the split: the k_sp_* kernels, the scans, the copies (--trace-child --fastq PATH is that child).
  - with --bam: the BAM input instead -- the same strings once as an unaligned BAM (BGZF, every third record marked
    reverse-strand) and once as a BGZF FASTQ, both inflated on the GPU: Context.load_sample of the BAM beside
    Context.load_sample_fastq of the FASTQ, wall time per call, and the same from the inflated BAM bytes already in HBM;
usage: python tools/sample_profile_rate.py [--bam] [--strings 100000] [--dir /dev/shm] [--rounds 3] [--parent-cli PATH] [--rocprof DIR] [--json OUT]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def write_inputs(d, n, genome_bp):
    import numpy as np
    rng = np.random.default_rng(1)
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, genome_bp)].reshape(-1, 80)
    with open(os.path.join(d, "g.fa"), "wb") as f:
        f.write(b">chr1\n" + np.concatenate([s, np.full((s.shape[0], 1), 10, np.uint8)], axis=1).tobytes())
    k = (9000.0 / 7000.0) ** 2
    lens = np.clip(rng.gamma(k, 9000.0 / k, n), 100, 60000).astype(np.int64)
    level = rng.integers(8, 31, n)
    with open(os.path.join(d, "s.fastq"), "wb") as f:
        for i in range(n):
            ln = int(lens[i])
            q = (np.clip(level[i] + rng.integers(-5, 6, ln), 0, 93).astype(np.uint8) + 33).tobytes()
            f.write(b"@r%d\n" % i + b"A" * ln + b"\n+\n" + q + b"\n")
    return os.path.getsize(os.path.join(d, "s.fastq"))


def h2d_floor(path):
    import torch
    with open(path, "rb") as f:
        data = f.read()
    host = torch.frombuffer(bytearray(data), dtype=torch.uint8).pin_memory()
    dev = torch.empty_like(host, device="cuda")
    best = None
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.copy_(host, non_blocking=True)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    return best, dev


def library(path, dev, reps, windows_mb):
    import pbsim3_amd as P
    p = P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_SAMPLE)
    out = {"load_sample_fastq_s": [], "from_device_s": [], "by_window_mb": {}}
    with P.Context(p, 0) as ctx:
        for mb in windows_mb:                       # the window of the pass through HBM (the default is among them)
            ctx.set_sample_chunk_bytes(mb << 20)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                ctx.load_sample_fastq(path)
                ts.append(time.perf_counter() - t0)
            td = []
            for _ in range(reps):
                t0 = time.perf_counter()
                ctx.sample_profile_from_fastq(dev)
                td.append(time.perf_counter() - t0)
            out["by_window_mb"][mb] = {"load_sample_fastq_s": ts, "from_device_s": td}
            print(f"window {mb} MiB: file {['%.3f' % x for x in ts]} s, from HBM {['%.3f' % x for x in td]} s", flush=True)
        ctx.set_sample_chunk_bytes(0)
        for _ in range(reps):
            t0 = time.perf_counter()
            st = ctx.load_sample_fastq(path)
            out["load_sample_fastq_s"].append(time.perf_counter() - t0)
        out["num"], out["num_filtered"], out["len_total_filtered"] = st.num, st.num_filtered, st.len_total_filtered
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.sample_profile_from_fastq(dev)
            out["from_device_s"].append(time.perf_counter() - t0)
    return out


def bam_inputs(d, n):
    """s.bam and s.fastq.gz (both BGZF, zlib level 1) of the same n strings; returns the inflated sizes"""
    import struct
    import numpy as np
    import bgzf_writer as W
    rng = np.random.default_rng(1)
    k = (9000.0 / 7000.0) ** 2
    lens = np.clip(rng.gamma(k, 9000.0 / k, n), 100, 60000).astype(np.int64)
    level = rng.integers(8, 31, n)
    bam, fq = [b"BAM\x01" + struct.pack("<ii", 0, 0)], []
    for i in range(n):
        ln = int(lens[i])
        q = np.clip(level[i] + rng.integers(-5, 6, ln), 0, 93).astype(np.uint8)
        name = b"r%d\0" % i
        flag = 4 | (16 if i % 3 == 0 else 0)
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 0, 4680, 0, flag, ln, -1, -1, 0) + name + \
            b"\x11" * (ln // 2) + (b"\x10" if ln % 2 else b"") + q.tobytes()
        bam.append(struct.pack("<I", len(body)) + body)
        fq.append(b"@r%d\n" % i + (b"T" if flag & 16 else b"A") * ln + b"\n+\n" + ((q[::-1] if flag & 16 else q) + 33).tobytes() + b"\n")
    bam, fq = b"".join(bam), b"".join(fq)
    with open(os.path.join(d, "s.bam"), "wb") as f:
        f.write(W.bgzf(bam, level=1))
    with open(os.path.join(d, "s.fastq.gz"), "wb") as f:
        f.write(W.bgzf(fq, level=1))
    return bam, len(fq)


def bam_mode(a):
    import torch
    import pbsim3_amd as P
    res = {}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        t0 = time.time()
        bam, fq_bytes = bam_inputs(d, a.strings)
        res["strings"], res["bam_bytes"], res["fastq_bytes"] = a.strings, len(bam), fq_bytes
        res["bam_file_bytes"], res["fastq_gz_file_bytes"] = (os.path.getsize(os.path.join(d, x)) for x in ("s.bam", "s.fastq.gz"))
        print(f"{a.strings} strings: BAM {len(bam) / 1e6:.1f} MB inflated ({res['bam_file_bytes'] / 1e6:.1f} MB BGZF), FASTQ "
              f"{fq_bytes / 1e6:.1f} MB inflated ({res['fastq_gz_file_bytes'] / 1e6:.1f} MB BGZF), written in {time.time() - t0:.0f} s", flush=True)
        dev = torch.frombuffer(bytearray(bam), dtype=torch.uint8).cuda()
        with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_SAMPLE), 0) as ctx:
            for key, call in (("load_sample_bam_s", lambda: ctx.load_sample(os.path.join(d, "s.bam"))),
                              ("load_sample_fastq_bgzf_s", lambda: ctx.load_sample_fastq(os.path.join(d, "s.fastq.gz"))),
                              ("bam_from_device_s", lambda: ctx.sample_profile_from_bam(dev))):
                ts, kept = [], []
                for _ in range(a.rounds):
                    t0 = time.perf_counter()
                    st = call()
                    ts.append(time.perf_counter() - t0)
                    kept.append((st.num, st.num_filtered, st.len_total_filtered))
                res[key], res[key + "_kept"] = ts, kept[-1]
                print(f"{key}: {['%.4f' % x for x in ts]} s; reads {kept[-1][0]}, kept {kept[-1][1]} ({kept[-1][2]} bases)", flush=True)
        res["same_profile_numbers"] = res["load_sample_bam_s_kept"] == res["load_sample_fastq_bgzf_s_kept"] == res["bam_from_device_s_kept"]
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def cli_phases(cli, d, tag):
    out = os.path.join(d, "out_" + tag)
    os.makedirs(out, exist_ok=True)
    t0 = time.perf_counter()
    p = subprocess.run([cli, "--strategy", "wgs", "--method", "sample", "--sample", os.path.join(d, "s.fastq"), "--genome",
                        os.path.join(d, "g.fa"), "--depth", "20", "--seed", "1", "--prefix", os.path.join(out, "out")],
                       capture_output=True, text=True, timeout=600, cwd=out, env=dict(os.environ, PBSIM_TRACE="1"))
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        print(p.stderr[-3000:])
        sys.exit(1)
    phases = [(float(m.group(1)), m.group(2)) for m in re.finditer(r"\[pbsim cli\]\s+([0-9.]+) ms\s+(.*)", p.stderr)]
    sizes = {fn: os.path.getsize(os.path.join(out, fn)) for fn in sorted(os.listdir(out))}
    for fn in os.listdir(out):
        os.remove(os.path.join(out, fn))
    return {"wall_s": wall, "phases_ms": phases, "output_sizes": sizes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strings", type=int, default=100000)
    ap.add_argument("--genome-bp", type=int, default=50_000_000)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--windows-mb", default="", help="also time these window sizes (pbsim_set_sample_chunk_bytes), e.g. 16,64,256")
    ap.add_argument("--parent-cli")
    ap.add_argument("--json")
    ap.add_argument("--rocprof", metavar="DIR", help="also run one load_sample_fastq in a child under rocprofv3, its output into DIR")
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--fastq", help="(--trace-child) an existing FASTQ instead of a generated one")
    ap.add_argument("--bam", action="store_true", help="time the BAM input beside the BGZF FASTQ of the same strings, and nothing else")
    a = ap.parse_args()
    if a.bam:
        return bam_mode(a)
    if a.trace_child and a.fastq:
        import pbsim3_amd as P
        with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_SAMPLE), 0) as ctx:
            t0 = time.perf_counter()
            st = ctx.load_sample_fastq(a.fastq)
            print(f"load_sample_fastq: {time.perf_counter() - t0:.3f} s, kept {st.num_filtered} of {st.num}", flush=True)
        return
    res = {}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        t0 = time.time()
        size = write_inputs(d, a.strings, a.genome_bp - a.genome_bp % 80)
        print(f"sample FASTQ: {a.strings} strings, {size / 1e9:.3f} GB, written in {time.time() - t0:.0f} s", flush=True)
        path = os.path.join(d, "s.fastq")
        res["fastq_bytes"] = size
        if a.trace_child:
            sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child", "--fastq", path], cwd=ROOT).returncode)
        t, dev = h2d_floor(path)
        res["h2d_floor"] = {"s": t, "GBps": size / t / 1e9}
        print(f"floor: pinned host -> device {t * 1e3:.1f} ms ({size / t / 1e9:.1f} GB/s)", flush=True)
        res["library"] = library(path, dev, a.rounds, [int(x) for x in a.windows_mb.split(",") if x])
        del dev
        lib = res["library"]
        best = min(lib["load_sample_fastq_s"][1:] or lib["load_sample_fastq_s"])
        res["ratio_to_floor"] = best / t
        print(f"load_sample_fastq: {['%.3f' % x for x in lib['load_sample_fastq_s']]} s -> best {best * 1e3:.1f} ms = {best / t:.2f} x the floor; "
              f"from bytes in HBM: {['%.3f' % x for x in lib['from_device_s']]} s; kept {lib['num_filtered']} of {lib['num']}", flush=True)
        clis = {"this": os.path.join(ROOT, "pbsim3_amd", "bin", "pbsim")}
        if a.parent_cli:
            clis["parent"] = os.path.abspath(a.parent_cli)
        res["cli"] = {k: [] for k in clis}
        for r in range(a.rounds):
            for tag, cli in clis.items():
                c = cli_phases(cli, d, tag)
                res["cli"][tag].append(c)
                print(f"cli round {r} {tag}: wall {c['wall_s']:.2f} s; " + "; ".join(f"{ms:.0f} ms {what}" for ms, what in c["phases_ms"]), flush=True)
        if a.rocprof:
            q = subprocess.run(["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--stats", "-d", a.rocprof, "--", sys.executable,
                                os.path.abspath(__file__), "--trace-child", "--fastq", path], cwd=ROOT, capture_output=True, text=True,
                               timeout=600)
            print("rocprofv3 child:", q.returncode, q.stdout.strip()[-300:], flush=True)
        if a.parent_cli:
            res["outputs_same_sizes"] = res["cli"]["this"][0]["output_sizes"] == res["cli"]["parent"][0]["output_sizes"]
            print("output sizes identical to the parent's:", res["outputs_same_sizes"], flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
