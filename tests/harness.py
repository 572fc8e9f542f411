"""Test harness: runs the CHECKER (oracle/pbsim_oracle, the compiled reference
under oracle/_ref when present) and canonicalises outputs for comparison.
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg use it."""
import hashlib
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ORACLE = os.path.join(ROOT, "oracle", "pbsim_oracle")
REF_GLIBC = os.path.join(ROOT, "oracle", "_ref", "pbsim_ref")
REF_PHILOX = os.path.join(ROOT, "oracle", "_ref", "pbsim_ref_philox")
# model files are inputs (format contract): committed gzip-compressed, unpacked on first use (cached_file)
MODEL_GZ_DIR = os.path.join(ROOT, "tests", "golden", "models")
MODEL_CACHE = os.path.join(MODEL_GZ_DIR, "_unpacked")


def cached_file(cache, name, make, src=None):
    """cache/<name>, written by make(path) on first use.  When the tree cannot be written to (a checkout owned by another
    user, a read-only mount) the file goes to a directory of this user's under the system's temporary directory instead,
    keyed by the content of `src` (the committed file it is made from; without one, of this file, which generates it) so that
    a later checkout never reads a stale copy."""
    p = os.path.join(cache, name)
    if os.path.exists(p):
        return p
    try:
        return _write_cached(cache, p, make)
    except OSError:
        if os.path.exists(p):
            return p
    top = os.path.join(tempfile.gettempdir(), "pbsim3_amd-%d" % os.getuid())
    os.makedirs(top, mode=0o700, exist_ok=True)
    if os.stat(top).st_uid != os.getuid():
        raise PermissionError("%s belongs to another user" % top)
    key = hashlib.sha1(open(src or os.path.abspath(__file__), "rb").read()).hexdigest()[:16]
    d = os.path.join(top, os.path.relpath(cache, ROOT), key)
    q = os.path.join(d, name)
    return q if os.path.exists(q) else _write_cached(d, q, make)


def _write_cached(d, p, make):
    os.makedirs(d, exist_ok=True)
    tmp = p + ".%d.tmp" % os.getpid()
    try:
        make(tmp)
        os.replace(tmp, p)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return p


def gunzip_to(src):
    """make() of cached_file: the decompressed bytes of `src`"""
    def make(dst):
        import gzip
        with gzip.open(src, "rb") as f, open(dst, "wb") as g:
            g.write(f.read())
    return make


def model_path(name):
    """FIC-HMM model files are INPUT DATA (format contract); the six
    used by the tests are committed gzip-compressed and unpacked on first use."""
    src = os.path.join(MODEL_GZ_DIR, name + ".gz")
    if not os.path.exists(os.path.join(MODEL_CACHE, name)) and not os.path.exists(src):
        raise FileNotFoundError(name)
    return cached_file(MODEL_CACHE, name, gunzip_to(src), src)


INPUT_CACHE = os.path.join(GOLDEN, "inputs", "_unpacked")


def synth_bases_at(first, n, seed):
    """bytes first .. first + n - 1 of synth_bases(.., seed): a pure function of the position"""
    import numpy as np
    out = np.empty(n, dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    step = 1 << 22
    with np.errstate(over="ignore"):
        for a in range(first, first + n, step):
            x = (np.arange(a, min(first + n, a + step), dtype=np.uint64) + np.uint64(seed * 0x632BE59BD9B4E019 & (2**64 - 1))) * np.uint64(0x9E3779B97F4A7C15)
            x ^= x >> np.uint64(30)
            x *= np.uint64(0xBF58476D1CE4E5B9)
            x ^= x >> np.uint64(27)
            x *= np.uint64(0x94D049BB133111EB)
            x ^= x >> np.uint64(31)
            out[a - first:a - first + len(x)] = lut[(x >> np.uint64(61)).astype(np.int64) & 3]
    return out


def synth_bases(n, seed):
    """n pseudo-random A/C/G/T bytes from plain 64-bit integer arithmetic (splitmix64 of the position), so the file is
    the same on every box and numpy version without being committed."""
    return synth_bases_at(0, n, seed)


def synth_bases_torch(n, seed, device="cuda"):
    """synth_bases on a torch device (the GPU box: 3 Gbp in a second instead of a minute): the same splitmix64 in int64
    arithmetic -- products wrap like uint64's, logical right shifts are arithmetic ones with the sign bits masked off.
    tests/test_fullsize_digests.py checks it against synth_bases on the CPU."""
    import torch

    def i64(v):                    # a uint64 constant as the int64 with the same bits
        v &= (1 << 64) - 1
        return v - (1 << 64) if v >= (1 << 63) else v

    def lsr(x, k):
        return (x >> k) & ((1 << (64 - k)) - 1)

    out = torch.empty(n, dtype=torch.uint8, device=device)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=device)
    step = 1 << 26
    add = i64(seed * 0x632BE59BD9B4E019)
    for a in range(0, n, step):
        x = (torch.arange(a, min(n, a + step), dtype=torch.int64, device=device) + add) * i64(0x9E3779B97F4A7C15)
        x = x ^ lsr(x, 30)
        x = x * i64(0xBF58476D1CE4E5B9)
        x = x ^ lsr(x, 27)
        x = x * i64(0x94D049BB133111EB)
        x = x ^ lsr(x, 31)
        out[a:a + x.numel()] = lut[lsr(x, 61) & 3]
    return out


def _words(n, seed, stream):
    """n splitmix64 words of (index, seed, stream) as Python ints: the same integer arithmetic as synth_bases_at"""
    import numpy as np
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x632BE59BD9B4E019 + stream * 0xD1B54A32D192ED03) & (2**64 - 1))) * \
            np.uint64(0x9E3779B97F4A7C15)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


BUF_SIZE = 10240         # the reference's fgets buffer: a line of more than BUF_SIZE - 1 bytes is read in several pieces
TRANS_ID_LEN_MAX = 128


def transcript_edge_units(seed):
    """The listed edge units synth_transcripts appends after its bulk: [(name, id, plus, minus, seq)].  `name` says what each
    one is there for; the sequences are synth_bases_at of a stream of their own."""
    units, at = [], [0]

    def bases(n, s=None):
        b = synth_bases_at(at[0], n, seed + 7_000_001).tobytes() if s is None else s
        at[0] += n
        return b

    def add(name, plus, minus, seq, tid=None):
        units.append((name, tid or "E%d_%s" % (len(units), name), plus, minus, seq))

    # read lengths around the start-position ranks ceil(len / 1000) (pbsim.cpp:4516-4522).  Not 1 or 2: there the start-position
    # draw often leaves an empty read, and the reference then indexes its accuracy histogram with (int)NaN and crashes
    # (pbsim.cpp:4691-4695).  A 5-base transcript does so only rarely; the committed cases are ones the reference completed.
    for n in (5, 99, 100, 101, 999, 1000, 1001, 2000, 2001):
        add("len%d" % n, 3, 1, bases(n))
    # LINES (id, three tabs, sequence, newline) of these many bytes: around the 10 239-byte pieces of fgets(BUF_SIZE)
    for line in (10238, 10239, 10240, 10241, 10242, 20479, 20480):
        tid = "E%d_line%d" % (len(units), line)
        head = "%s\t2\t1\t" % tid
        seq = bytearray(bases(line - len(head) - 1))
        if line == 20479:          # a homopolymer of 17 across the end of the first piece (bytes 10 230 .. 10 246 of the line)
            a = 10230 - len(head)
            seq[a:a + 17] = b"G" * 17
        add("line%d" % line, 2, 1, bytes(seq), tid)
    # long transcripts: start-position ranks far beyond the bulk's 12 (TR_RANK_MAX 1000; TRANS_LEN_MAX 1 000 000)
    for n, p, m in ((15_000, 1, 1), (50_000, 2, 1), (200_000, 1, 2), (500_000, 1, 1), (999_000, 2, 1)):
        add("long%d" % n, p, m, bases(n))
    # expression values: none, one strand only, and one unit of 5 000 reads
    add("exp0_0", 0, 0, bases(3000))
    add("exp4_0", 4, 0, bases(3000))
    add("exp0_4", 0, 4, bases(3000))
    add("exp4000_1000", 4000, 1000, bases(2500))
    # lower case (the reference upper-cases from the SECOND base on, pbsim.cpp:4457-4459) and runs of N
    add("lower_all", 3, 2, bases(4000).lower())
    s = bytearray(bases(4000))
    s[0:1] = s[0:1].lower()
    s[1000:1100] = s[1000:1100].lower()
    add("lower_first", 3, 2, bytes(s))
    s = bytearray(bases(5000))
    s[0:20] = b"N" * 20
    s[2000:2300] = b"N" * 300
    s[4990:5000] = b"n" * 10
    add("n_runs", 3, 2, bytes(s))
    # ids: exactly TRANS_ID_LEN_MAX characters, and a longer one (cut at TRANS_ID_LEN_MAX, pbsim.cpp:4432-4433)
    add("id128", 2, 1, bases(3000), ("I128_" + "x" * 200)[:TRANS_ID_LEN_MAX])
    add("id200", 2, 1, bases(3000), ("I200_" + "y" * 200)[:200])
    return units


def synth_transcripts(n, seed, bases=None):
    """The bytes of a --transcript file (`id\\tplus\\tminus\\tseq\\n` per line): n transcripts of the benchmark's shape, then
    transcript_edge_units(seed).  Bulk: lengths 300 .. 12 000 with a long tail (300 + 11 700 u^3, mean ~3 200), plus
    expression 0 .. 40 (mean 20), minus 1 for one transcript in ten (mean 0.1), sequences consecutive slices of
    synth_bases(total, seed).  Integer arithmetic only: the same bytes on every box.  `bases(n, seed)` may stand in for
    synth_bases (harness.synth_bases_torch on a GPU box: the same bytes, faster)."""
    import numpy as np
    w = [x.tolist() for x in (_words(n, seed, s) for s in (1, 2, 3, 4))]
    lens = [300 + 11700 * ((u >> 44) ** 3) // (1 << 60) for u in w[0]]
    plus = [(a >> 40) % 21 + (b >> 40) % 21 for a, b in zip(w[1], w[2])]
    minus = [1 if (u >> 40) % 10 == 0 else 0 for u in w[3]]
    allseq = np.asarray((bases or synth_bases)(sum(lens), seed)).tobytes()
    out, at = [], 0
    for i in range(n):
        out.append(b"T%d\t%d\t%d\t" % (i, plus[i], minus[i]) + allseq[at:at + lens[i]] + b"\n")
        at += lens[i]
    for name, tid, p, m, seq in transcript_edge_units(seed):
        out.append(b"%s\t%d\t%d\t" % (tid.encode(), p, m) + seq + b"\n")
    return b"".join(out)


def synth_sample_fastq(n, seed):
    """The bytes of a 4-line FASTQ for --method sample: n strings of lengths 100 .. 60 000 (100 + 59 900 u^6, mean ~8 700),
    each with its own quality level and a +-5 jitter per character, clipped to '!' .. '~' (one string in twenty at a level
    of 40 .. 93); then a cluster of 400 strings whose accuracy straddles the default --accuracy-min 0.75 (characters
    Q5 or Q7, about 43 % Q5), and strings of 99, 100 and 101 characters around --length-min 100.  The bases are not read
    by the sampling method: a fixed pattern.  Integer arithmetic only."""
    import numpy as np
    w = [x.tolist() for x in (_words(n, seed, s) for s in (11, 12))]
    lens = [100 + 59900 * ((u >> 54) ** 6) // (1 << 60) for u in w[0]]
    level = [40 + (u >> 40) % 54 if (u >> 20) % 20 == 0 else 3 + (u >> 40) % 35 for u in w[1]]
    cl = _words(400, seed, 13).tolist()
    cl_lens = [300 + (u >> 40) % 1700 for u in cl]
    cl_thr = [104 + (u >> 20) % 16 for u in cl]        # byte < thr: Q5 (p 0.316), else Q7 (p 0.200): accuracy ~0.745 .. 0.756
    edge_lens = [99, 100, 101, 99, 100, 101]
    total = sum(lens) + sum(cl_lens) + sum(edge_lens)
    jb = _words((total + 7) // 8, seed, 14).view(np.uint8)[:total].astype(np.int16)
    pat = np.frombuffer(b"ACGT" * 15001, dtype=np.uint8)
    out, at = [], 0

    def rec(k, q):
        out.append(b"@s%d\n%s\n+\n%s\n" % (k, pat[:len(q)].tobytes(), q.tobytes()))

    for i in range(n):
        j = jb[at:at + lens[i]]
        rec(i, (np.clip(level[i] + j % 11 - 5, 0, 93) + 33).astype(np.uint8))
        at += lens[i]
    for i in range(len(cl)):
        j = jb[at:at + cl_lens[i]]
        rec(n + i, np.where(j < cl_thr[i], 38, 40).astype(np.uint8))
        at += cl_lens[i]
    for i, ln in enumerate(edge_lens):
        j = jb[at:at + ln]
        rec(n + len(cl) + i, (np.clip((25 if i < 3 else 4) + j % 11 - 5, 0, 93) + 33).astype(np.uint8))
        at += ln
    return b"".join(out)


def sample_profile(fq, len_min=100, len_max=1_000_000, acc_min=0.75, acc_max=1.0):
    """The filtered quality strings of get_sample_inf (pbsim.cpp:1216-1283) for a well-formed 4-line FASTQ, as
    pbsim3_amd.args.read_sample_fastq, with numpy: per-character values of the reference's table qc[q].prob = pow(10, q / -10)
    (libm pow, as the reference's), summed in file order from 0.0 by a sequential cumsum (np.sum adds pairwise)."""
    import numpy as np
    table = np.array([10 ** (q / -10) for q in range(94)], dtype=np.float64)
    lines = fq.split(b"\n")
    out = []
    for q in lines[3::4]:
        n = len(q)
        if not (len_min <= n <= len_max):
            continue
        prob = np.cumsum(table[np.frombuffer(q, dtype=np.uint8) - 33])[-1]
        acc = 1.0 - float(prob) / n
        if acc_min <= acc <= acc_max:
            out.append(q)
    return out


def write_fasta(path, length, seed, bases=None):
    """one FASTA record `>synth_<length>_<seed>` of synth_bases(length, seed) (or of `bases`, the same bytes), 80 per line"""
    import numpy as np
    seq = np.asarray(synth_bases(length, seed) if bases is None else bases)
    with open(path, "wb") as f:
        f.write(b">synth_%d_%d\n" % (length, seed))
        width = 80
        full = length // width * width
        step = width * (1 << 16)
        for a in range(0, full, step):
            rows = seq[a:min(full, a + step)].reshape(-1, width)
            f.write(np.concatenate([rows, np.full((rows.shape[0], 1), 10, np.uint8)], axis=1).tobytes())
        if full < length:
            f.write(seq[full:].tobytes() + b"\n")


def write_case_inputs(case, d, bases=None):
    """The generated inputs of a fullsize_cases.py case, written into directory d: (the reference's command line
    for them, {input: sha256 of the file}).  `bases(n, seed)` may stand in for synth_bases (the same bytes)."""
    argv, digests = [], {}
    todo = []
    if "record" in case:
        length, seed = case["record"]
        todo.append(("genome", "g.fa", lambda p: write_fasta(p, length, seed, None if bases is None else bases(length, seed))))
    if "transcripts" in case:
        todo.append(("transcript", "tr.txt", lambda p: open(p, "wb").write(synth_transcripts(*case["transcripts"], bases=bases))))
    if "sample" in case:
        todo.append(("sample", "s.fq", lambda p: open(p, "wb").write(synth_sample_fastq(*case["sample"]))))
    for opt, fn, make in todo:
        p = os.path.join(d, fn)
        make(p)
        h = hashlib.sha256()
        with open(p, "rb") as f:
            for blk in iter(lambda: f.read(1 << 24), b""):
                h.update(blk)
        argv += ["--" + opt, p]
        digests[opt] = h.hexdigest()
    return argv, digests


def load_fullsize():
    """tests/golden/fullsize.json: CRC-32 + length of the streams the REFERENCE wrote for the BASELINE-size cases
    (tests/golden/make_fullsize.py), plus its stderr report"""
    with open(os.path.join(GOLDEN, "fullsize.json")) as f:
        return json.load(f)


def input_path(name):
    """tests/golden/inputs/<name>: committed as is, committed gzip-compressed (the reference's own sample files: data),
    or generated on first use -- `synth_<bases>_<seed>.fa`: one FASTA record of that many synth_bases, 80 per line."""
    import re
    p = os.path.join(GOLDEN, "inputs", name)
    if os.path.exists(p):
        return p
    m = re.fullmatch(r"synth_(\d+)_(\d+)\.fa", name)
    if os.path.exists(p + ".gz"):
        return cached_file(INPUT_CACHE, name, gunzip_to(p + ".gz"), p + ".gz")
    if m:
        def make(tmp):
            import numpy as np
            n, seed = int(m.group(1)), int(m.group(2))
            b = synth_bases(n, seed)
            full = n // 80 * 80
            lines = np.empty((full // 80, 81), dtype=np.uint8)
            lines[:, :80] = b[:full].reshape(-1, 80)
            lines[:, 80] = 10
            with open(tmp, "wb") as g:
                g.write(b">synth_%d_%d\n" % (n, seed))
                g.write(lines.tobytes())
                if full < n:
                    g.write(b[full:].tobytes() + b"\n")
        return cached_file(INPUT_CACHE, name, make)
    raise FileNotFoundError(name)
    return q


def build_oracle():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    return ORACLE


def strip_report(err: str) -> str:
    keep = []
    for line in err.splitlines():
        if line.startswith((":::: System utilization", "CPU time(s)", "Elapsed time(s)", "oracle draws")):
            continue
        if line.split(" : ")[0] in ("prefix", "genome", "transcript", "errhmm", "qshmm", "file name", "template", "sample"):
            continue
        keep.append(line)
    return "\n".join(keep).rstrip("\n") + "\n"


def resolve(args):
    out = []
    for a in args:
        if a.startswith("MODEL:"):
            out.append(model_path(a[6:]))
        elif a.startswith("INPUT:"):
            out.append(input_path(a[6:]))
        else:
            out.append(a)
    return out


def collect(workdir, prefix="out"):
    res = {}
    for fn in sorted(os.listdir(workdir)):
        if fn.startswith("sample_profile_"):     # --sample-profile-id writes into the working directory (pbsim.cpp:1590)
            with open(os.path.join(workdir, fn), "rb") as f:
                res[".profile_" + fn.rsplit(".", 1)[1]] = f.read()
        if fn.startswith(prefix) and os.path.isfile(os.path.join(workdir, fn)):
            key = fn[len(prefix):]
            key = key.replace(".fq.gz", ".fq").replace(".maf.gz", ".maf").replace(".bam", ".sam")
            with open(os.path.join(workdir, fn), "rb") as f:
                res[key] = f.read()
    return res


def run_setup(exe_and_flags, case, workdir, env=None):
    """A case may name a command that must have run before it in the same directory (a stored sample profile)."""
    if case and case.get("setup"):
        subprocess.run(exe_and_flags[:1] + resolve(case["setup"]) + ["--prefix", os.path.join(workdir, "setup")] +
                       exe_and_flags[1:], capture_output=True, text=True, check=True, cwd=workdir, env=env)
        for fn in os.listdir(workdir):
            if fn.startswith("setup"):
                os.remove(os.path.join(workdir, fn))


def run_oracle(args, mode, workdir, extra=(), case=None):
    build_oracle()
    run_setup([ORACLE, "--rng", mode], case, workdir)
    p = subprocess.run([ORACLE] + resolve(args) + ["--prefix", os.path.join(workdir, "out"), "--rng", mode] + list(extra),
                       capture_output=True, text=True, cwd=workdir)
    if p.returncode != 0:
        raise RuntimeError(f"oracle failed ({p.returncode}): {p.stderr[-2000:]}")
    outs = collect(workdir)
    outs[".stderr"] = strip_report(p.stderr).encode()
    return outs


def make_stubs(d):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "gzip"), "w") as f:
        f.write("#!/bin/sh\nexec cat\n")
    with open(os.path.join(d, "samtools"), "w") as f:
        f.write('#!/bin/sh\nexec cat > "$4"\n')
    for n in ("gzip", "samtools"):
        os.chmod(os.path.join(d, n), 0o755)


def run_reference(args, mode, workdir, case=None):
    exe = REF_GLIBC if mode == "glibc" else REF_PHILOX
    args = resolve(args)
    seed = args[args.index("--seed") + 1]
    stubs = os.path.join(workdir, "stubs")
    make_stubs(stubs)
    env = dict(os.environ, PATH=stubs + ":" + os.environ["PATH"], PBSHIM_SEED=seed, PBSHIM_MODE="philox")
    run_setup([exe], case, workdir, env)
    p = subprocess.run([exe] + args + ["--prefix", os.path.join(workdir, "out")], env=env,
                       capture_output=True, text=True, check=True, cwd=workdir)
    outs = collect(workdir)
    outs[".stderr"] = strip_report(p.stderr).encode()
    return outs


def sha(b):
    return hashlib.sha256(b).hexdigest()


def load_manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)
