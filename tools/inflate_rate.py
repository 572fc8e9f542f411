"""Measures the gzip input path (GPU box): the BASELINE configs[1] genome -- 4 records x 750 Mbp of harness.synth_bases,
80 bases per line -- written plain, as BGZF (level 6, bgzip's 65280-byte members) and as plain gzip (level 6 members of
64 MiB without the 'BC' field, so it takes the host path), compressed on at most 16 processes.  Reports:
  - the GPU inflate of the BGZF bytes (Context.inflate_buffer, PBSIM_INFLATE_TRACE): kernel time from device events, in
    GB/s of output and of compressed input, and the call's wall time;
  - zlib on the host, one thread, on the same BGZF bytes and on the plain-gzip file;
  - `pbsim` end to end (FASTA -> .fq.gz + .maf.gz + .ref) on the three forms, alternated, --rounds times.
usage: python tools/inflate_rate.py [--dir /dev/shm] [--rounds 2] [--json OUT]"""
import argparse
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import bgzf_writer as W  # noqa: E402
import harness  # noqa: E402

RECORDS, RECORD_LEN = 4, 750_000_000


def genome():
    out = []
    for r in range(RECORDS):
        b = harness.synth_bases(RECORD_LEN, r + 1)
        lines = b.reshape(-1, 80)
        import numpy as np
        body = np.concatenate([lines, np.full((lines.shape[0], 1), 10, np.uint8)], axis=1).tobytes()
        out.append(b">chr%d\n" % (r + 1) + body)
    return b"".join(out)


def _bgzf(args):
    path, a, e = args
    with open(path, "rb") as f:
        f.seek(a)
        d = f.read(e - a)
    return b"".join(W.member(d[i:i + W.BGZIP_BLOCK], level=6) for i in range(0, len(d), W.BGZIP_BLOCK))


def _gzip(args):
    path, a, e = args
    with open(path, "rb") as f:
        f.seek(a)
        return W.plain_gzip(f.read(e - a), level=6)


def host_zlib_bgzf(data):
    """seconds of one-thread zlib over the BGZF members of data: walked by BSIZE, each member's raw deflate data
    decompressed from a memoryview slice (no copy of the input)"""
    mv = memoryview(data)
    t0 = time.perf_counter()
    n, p = 0, 0
    while p < len(data):
        xlen = struct.unpack_from("<H", data, p + 10)[0]
        bsize = struct.unpack_from("<H", data, p + 16)[0] + 1   # (the writer puts BC first)
        n += len(zlib.decompress(mv[p + 12 + xlen:p + bsize - 8], -15))
        p += bsize
    return time.perf_counter() - t0, n


def host_zlib_gzip(data):
    """seconds of one-thread zlib over the concatenated gzip members of data, fed 1 MiB memoryview slices at a time"""
    mv = memoryview(data)
    t0 = time.perf_counter()
    n, p, chunk = 0, 0, 1 << 20
    d = zlib.decompressobj(31)
    while p < len(data):
        n += len(d.decompress(mv[p:p + chunk]))
        p += chunk
        while d.eof:                       # (a member's end: what is left of this chunk starts the next one)
            rest = d.unused_data
            d = zlib.decompressobj(31)
            if rest:
                n += len(d.decompress(rest))
    return time.perf_counter() - t0, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--json")
    a = ap.parse_args()
    res = {}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        plain = os.path.join(d, "plain", "g.fa")
        for sub in ("plain", "bgzf", "gzip"):
            os.makedirs(os.path.join(d, sub))
        t0 = time.time()
        with open(plain, "wb") as f:
            f.write(genome())
        size = os.path.getsize(plain)
        print(f"genome: {size / 1e9:.2f} GB in {time.time() - t0:.0f} s", flush=True)
        t0 = time.time()
        step = 256 * W.BGZIP_BLOCK
        with Pool(16) as pool:
            parts = pool.map(_bgzf, [(plain, i, min(size, i + step)) for i in range(0, size, step)])
            with open(os.path.join(d, "bgzf", "g.fa"), "wb") as f:
                for p in parts:
                    f.write(p)
                f.write(W.EOF_MARKER)
            del parts
            parts = pool.map(_gzip, [(plain, i, min(size, i + (64 << 20))) for i in range(0, size, 64 << 20)])
            with open(os.path.join(d, "gzip", "g.fa"), "wb") as f:
                for p in parts:
                    f.write(p)
            del parts
        zb, zg = os.path.getsize(os.path.join(d, "bgzf", "g.fa")), os.path.getsize(os.path.join(d, "gzip", "g.fa"))
        print(f"compressed in {time.time() - t0:.0f} s: BGZF {zb / 1e9:.3f} GB, gzip {zg / 1e9:.3f} GB", flush=True)
        res.update(plain_bytes=size, bgzf_bytes=zb, gzip_bytes=zg)
        # ---- the GPU inflate alone, in a child (its own context), twice: the first call pays the allocations
        code = ("import sys, time, pbsim3_amd as P\n"
                "z = open(sys.argv[1], 'rb').read()\n"
                "with P.Context(P.default_params(), 0) as c:\n"
                "    for i in range(3):\n"
                "        t0 = time.perf_counter(); out = c.inflate_buffer(z); t = time.perf_counter() - t0\n"
                "        print('wall', t, len(out), flush=True)\n")
        p = subprocess.run([sys.executable, "-c", code, os.path.join(d, "bgzf", "g.fa")], capture_output=True, text=True,
                           timeout=600, cwd=ROOT, env=dict(os.environ, PBSIM_INFLATE_TRACE="1"))
        if p.returncode != 0:
            print(p.stderr[-3000:])
            sys.exit(1)
        walls = [float(l.split()[1]) for l in p.stdout.splitlines() if l.startswith("wall")]
        kms = [float(m.group(1)) for m in re.finditer(r"kernels ([0-9.]+) ms", p.stderr)]
        res["gpu_inflate"] = {"wall_s": walls, "kernel_ms": kms,
                              "out_GBps_kernel": [size / k / 1e6 for k in kms],
                              "in_GBps_kernel": [zb / k / 1e6 for k in kms],
                              "out_GBps_wall": [size / w / 1e9 for w in walls]}
        print("GPU inflate:", json.dumps(res["gpu_inflate"]), flush=True)
        with open(os.path.join(d, "bgzf", "g.fa"), "rb") as f:
            t, n = host_zlib_bgzf(f.read())
        res["host_zlib_bgzf"] = {"s": t, "out_GBps": n / t / 1e9}
        with open(os.path.join(d, "gzip", "g.fa"), "rb") as f:
            t, n = host_zlib_gzip(f.read())
        res["host_zlib_gzip"] = {"s": t, "out_GBps": n / t / 1e9}
        print("host zlib:", res["host_zlib_bgzf"], res["host_zlib_gzip"], flush=True)
        # ---- pbsim end to end, the three forms alternated
        cli = os.path.join(ROOT, "pbsim3_amd", "bin", "pbsim")
        model = harness.model_path("ERRHMM-ONT.model")
        res["e2e_s"] = {"plain": [], "bgzf": [], "gzip": []}
        outputs = {}
        for r in range(a.rounds):
            for form in ("plain", "bgzf", "gzip"):
                out = os.path.join(d, "out")
                os.makedirs(out, exist_ok=True)
                t0 = time.perf_counter()
                q = subprocess.run([cli, "--strategy", "wgs", "--method", "errhmm", "--errhmm", model, "--genome",
                                    os.path.join(d, form, "g.fa"), "--depth", "20", "--seed", "1", "--prefix",
                                    os.path.join(out, "out")], capture_output=True, text=True, timeout=300)
                t = time.perf_counter() - t0
                if q.returncode != 0:
                    print(q.stderr[-3000:])
                    sys.exit(1)
                if r == 0:  # the three forms must give the same files: every size, and the .ref files' CRC-32s
                    sig = {}
                    for fn in sorted(os.listdir(out)):
                        sig[fn] = os.path.getsize(os.path.join(out, fn))
                        if fn.endswith(".ref"):
                            with open(os.path.join(out, fn), "rb") as f:
                                sig[fn] = (sig[fn], zlib.crc32(f.read()))
                    outputs[form] = sig
                for fn in os.listdir(out):
                    os.remove(os.path.join(out, fn))
                res["e2e_s"][form].append(t)
                print(f"e2e round {r} {form}: {t:.2f} s", flush=True)
        res["outputs_identical"] = outputs["plain"] == outputs["bgzf"] == outputs["gzip"]
        print("outputs identical across the three forms:", res["outputs_identical"], flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
