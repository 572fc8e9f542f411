"""The two benchmarked per-unit jobs at their benchmarked size, content-checked against what the REFERENCE ITSELF wrote
(tests/golden/fullsize.json, tests/golden/make_fullsize.py):

  c3_trans_errhmm_sequel_100k  BASELINE configs[3]: trans, ERRHMM-SEQUEL, 100 000 transcripts of bench.py --workload trans's
                               shape + the edge units of harness.transcript_edge_units (~2 M reads)
  s_sample_100m_d20            bench.py --workload sample's job: a 100 Mbp record at depth 20 sampled from 50 000 quality
                               strings (~5.4 sweeps over the filtered profile, the quota reached mid-sweep)

Their inputs are generated here (harness.synth_transcripts / synth_sample_fastq: integer arithmetic, the bytes the reference
was run on -- checked by sha256 first).  Every leg must reproduce the reference's CRC-32 and length of both streams (gzip
members walked and folded as in test_gpu_fullsize.py; plain text folded with zlib.crc32 piece by piece) and its Simulation
stats block, through: the GPU's compression and the plain sink (the unit driver's two pipelines), a small scratch pool (many
batches), the lane walker alone, the CLI's transcript parser and the benchmark's set_transcripts, three ranks on the one GPU,
and the `pbsim` binary itself."""
import ctypes as C
import mmap
import os
import shutil
import subprocess
import threading
import zlib

import pytest

import harness
from fullsize_cases import FULLSIZE
from test_gpu_fullsize import MemberSink, helper, thread_comms, walk_piece

pytestmark = pytest.mark.gpu

TRANS = "c3_trans_errhmm_sequel_100k"
SAMPLE = "s_sample_100m_d20"
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


class StreamFold:
    """a pbsim_sink of the per-unit drivers: the pieces of each stream arrive in read order (one thread per stream at most), so
    they are folded as they come -- gzip members walked (`members`), or plain text through zlib.crc32 without a copy"""

    def __init__(self, P, members):
        self.st = [[0, 0, 0, 0], [0, 0, 0, 0]]   # per stream: CRC-32 of the text, its length, bytes received, members
        self.err = []
        helper()

        def put(which):
            def cb(user, text, n):
                try:
                    s = self.st[which]
                    if members:
                        k, crc, ln = walk_piece(C.cast(text, C.c_void_p), n)
                        s[0] = helper().fold(s[0], crc, ln)
                    else:
                        k, ln = 0, n
                        s[0] = zlib.crc32((C.c_char * n).from_address(C.cast(text, C.c_void_p).value), s[0])
                    s[1] += ln
                    s[2] += n
                    s[3] += k
                    return 1
                except Exception as e:     # (an exception cannot cross the C callback: the sink aborts the job instead)
                    self.err.append(repr(e))
                    return 0
            return cb
        self._cbs = (P.SINK_CB(put(0)), P.SINK_CB(put(1)))
        self.sink = P.Sink(None, *self._cbs)

    def digest(self):
        assert not self.err, self.err
        return [(s[0], s[1]) for s in self.st]


def fold_ranks(folds):
    """the streams of ranks that took consecutive read ranges, concatenated in rank order"""
    out = []
    for which in (0, 1):
        crc = ln = 0
        for f in folds:
            c, n = f.digest()[which]
            crc, ln = helper().fold(crc, c, n), ln + n
        out.append((crc, ln))
    return out


def torch_bases(n, seed):
    """harness.synth_bases on the GPU (the same bytes: tests/test_fullsize_digests.py), back in host memory"""
    import torch
    t = harness.synth_bases_torch(n, seed, "cuda")
    torch.cuda.synchronize()
    return t.cpu().numpy()


def want_of(name):
    e = harness.load_fullsize()[name]
    return [(int(e[k]["crc32"], 16), e[k]["bytes"]) for k in (".fq", ".maf")], e["stderr"]


def case_inputs(name, d):
    """the case's generated input files in d, checked against the sha256 the reference's run recorded"""
    argv, digests = harness.write_case_inputs(FULLSIZE[name], str(d), bases=torch_bases)
    assert digests == harness.load_fullsize()[name]["input_sha256"], "input differs from the one the reference was run on"
    return argv


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------ trans ------------------------------------------------------------------

@pytest.fixture(scope="module")
def trans_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("trans")
    argv = case_inputs(TRANS, d)
    path = argv[argv.index("--transcript") + 1]
    # the benchmark's path: the units handed over by pbsim_set_transcripts (ids cut at TRANS_ID_LEN_MAX as the reference's
    # strncpy does; the upper-casing is the library's, as for the file parser)
    ids, plus, minus, seqs = [], [], [], []
    with open(path, "rb") as f:
        for line in f:
            i, p, m, s = line.rstrip(b"\n").split(b"\t")
            ids.append(i[:harness.TRANS_ID_LEN_MAX].decode())
            plus.append(int(p))
            minus.append(int(m))
            seqs.append(s)
    yield dict(path=path, units=(ids, plus, minus, seqs), reads=sum(plus) + sum(minus),
               bases=sum((p + m) * len(s) for p, m, s in zip(plus, minus, seqs)))


def trans_ctx(P, inp, loader, scratch_mb=None):
    p = P.default_params(strategy=P.STRATEGY_TRANS, method=P.METHOD_ERR, seed=1)
    ctx = P.Context(p, 0)
    ctx.load_errhmm(harness.model_path("ERRHMM-SEQUEL.model"))
    if scratch_mb:
        ctx.set_scratch_bytes(scratch_mb << 20)
    if loader == "file":
        assert ctx.load_transcript_file(inp["path"]) == (len(inp["units"][0]), inp["reads"])
    else:
        ctx.set_transcripts(*inp["units"])
    return ctx


def check_trans(ctx, digest, inp):
    want, ref_report = want_of(TRANS)
    assert digest == want, "the trans job differs from the reference's own output"
    st = ctx.stats()
    assert ctx.format_stats(st, 0).rstrip("\n") in ref_report
    # sanity: a trans job draws exactly plus + minus reads per transcript; they are at most as long as their transcript
    assert st.res_num == inp["reads"] and 0.3 * inp["bases"] < st.res_len_total < 1.2 * inp["bases"]


TRANS_LEGS = {
    "members, set_transcripts": dict(deflate=7, loader="set"),               # the benchmarked path
    "plain text, set_transcripts": dict(deflate=0, loader="set"),            # the multi-batch plain-sink pipeline
    "members, 256 MiB scratch pool": dict(deflate=7, loader="set", scratch_mb=256),
    "members, lane walker only": dict(deflate=7, loader="set", env={"PBSIM_COOP_LEN": "-1"}),
    "members, load_transcript_file": dict(deflate=7, loader="file"),         # the CLI's parser: fgets pieces, id cut
    "plain text, load_transcript_file, 256 MiB scratch pool": dict(deflate=0, loader="file", scratch_mb=256),
}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("leg", list(TRANS_LEGS))
def test_trans_100k_equals_the_reference(trans_inputs, leg):
    import pbsim3_amd as P
    kw = TRANS_LEGS[leg]

    def run():
        ctx = trans_ctx(P, trans_inputs, kw["loader"], kw.get("scratch_mb"))
        try:
            ctx.set_deflate(kw["deflate"])
            fold = StreamFold(P, members=kw["deflate"] != 0)
            P._check(ctx.lib.pbsim_simulate_trans(ctx.h, C.byref(fold.sink)))
            check_trans(ctx, fold.digest(), trans_inputs)
            if kw["deflate"]:
                assert all(s[3] > 0 for s in fold.st)
        finally:
            ctx.close()
    with_env(kw.get("env", {}), run)


@pytest.mark.timeout(900)
def test_trans_100k_three_ranks_equal_the_reference(trans_inputs):
    """three contexts on the one GPU: rank r takes the r-th block of the read numbering (pbsim_simulate_units_range, as the CLI's
    --devices does), keeps its statistics' values and merges them over a host communicator; the blocks' streams concatenated
    in rank order are the reference's, and every rank reports the merged statistics"""
    import pbsim3_amd as P
    world = 3
    ctxs = [trans_ctx(P, trans_inputs, "set") for _ in range(world)]
    try:
        R = ctxs[0].unit_reads()
        assert R == trans_inputs["reads"]
        per = (R + world - 1) // world
        comms = thread_comms(P, world)
        folds = [StreamFold(P, members=True) for _ in range(world)]
        errs = [None] * world

        def one(r):
            try:
                c = ctxs[r]
                c.set_deflate(7)
                c.stats_keep_values(True)
                first = 1 + r * per
                P._check(c.lib.pbsim_simulate_units_range(c.h, first, min(per, R - first + 1), C.byref(folds[r].sink)))
                c.stats_merge(comms[r])
            except Exception as e:
                errs[r] = repr(e)
        th = [threading.Thread(target=one, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert errs == [None] * world, errs
        assert all(f.st[0][3] > 0 and f.st[1][3] > 0 for f in folds)       # members on every rank
        reports = [c.format_stats(c.stats(), 0) for c in ctxs]
        assert reports == [reports[0]] * world
        check_trans(ctxs[0], fold_ranks(folds), trans_inputs)
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------ sample ------------------------------------------------------------------

@pytest.fixture(scope="module")
def sample_inputs(tmp_path_factory):
    import torch
    d = tmp_path_factory.mktemp("sample")
    argv = case_inputs(SAMPLE, d)
    fq = argv[argv.index("--sample") + 1]
    with open(fq, "rb") as f:
        quals = harness.sample_profile(f.read())         # the reference's filter (pbsim.cpp:1216-1283), its arithmetic
    length, seed = FULLSIZE[SAMPLE]["record"]
    rec = harness.synth_bases_torch(length, seed, "cuda")
    torch.cuda.synchronize()
    yield dict(argv=argv, quals=quals, record=rec, depth=20.0, length=length)
    del rec


def sample_ctx(P, inp):
    p = P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_SAMPLE, seed=1, depth=inp["depth"])
    ctx = P.Context(p, 0)
    ctx.set_sample_profile(inp["quals"])
    ctx.set_reference_device(inp["record"].data_ptr(), inp["record"].numel(), 1)
    return ctx


def check_sample(ctx, digest, inp, st):
    want, ref_report = want_of(SAMPLE)
    assert digest == want, "the sampling job differs from the reference's own output"
    assert ctx.format_stats(st, 1).rstrip("\n") in ref_report
    # sanity: the quota is depth x record length; the filtered profile (370 M characters) is swept about 5.4 times
    target = inp["depth"] * inp["length"]
    assert target <= st.res_len_total < target * 1.001
    profile = sum(map(len, inp["quals"]))
    assert 5.0 < st.res_len_total / profile < 6.0


SAMPLE_LEGS = {
    "members": dict(deflate=7),
    "plain text": dict(deflate=0),
    "members, lane walker only": dict(deflate=7, env={"PBSIM_COOP_LEN": "-1"}),
    "plain text, wave walker for every string": dict(deflate=0, env={"PBSIM_COOP_LEN": "0"}),
}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("leg", list(SAMPLE_LEGS))
def test_sample_2g_equals_the_reference(sample_inputs, leg):
    import pbsim3_amd as P
    kw = SAMPLE_LEGS[leg]

    def run():
        ctx = sample_ctx(P, sample_inputs)
        try:
            ctx.set_deflate(kw["deflate"])
            fold = StreamFold(P, members=kw["deflate"] != 0)
            P._check(ctx.lib.pbsim_simulate_sample(ctx.h, C.byref(fold.sink)))
            check_sample(ctx, fold.digest(), sample_inputs, ctx.stats())
        finally:
            ctx.close()
    with_env(kw.get("env", {}), run)


@pytest.mark.timeout(900)
def test_sample_2g_three_ranks_equal_the_reference(sample_inputs):
    """pbsim_simulate_sample_comm on three contexts of the one GPU (host communicator): the pieces, folded by offset, and the
    merged statistics every rank reports"""
    import pbsim3_amd as P
    world = 3
    ctxs = [sample_ctx(P, sample_inputs) for _ in range(world)]
    try:
        msink = MemberSink(P)
        comms = thread_comms(P, world)
        sinks = [msink.sink_for(r) for r in range(world)]
        errs = [None] * world

        def one(r):
            c = ctxs[r]
            c.set_deflate(7)
            if not c.lib.pbsim_simulate_sample_comm(c.h, C.byref(comms[r]), C.byref(sinks[r])):
                errs[r] = c.lib.pbsim_last_error().decode(errors="replace")
        th = [threading.Thread(target=one, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert errs == [None] * world, errs
        digest = msink.digest()
        st = msink.done[0][0]
        reports = [ctxs[0].format_stats(msink.done[r][0], 1) for r in range(world)]
        assert reports == [reports[0]] * world
        check_sample(ctxs[0], [d[:2] for d in digest], sample_inputs, st)
        assert all(d[3] > 0 for d in digest)
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------------ the CLI ------------------------------------------------------------------

def walk_file(path):
    """(CRC-32, length) of the text the gzip members of a file hold"""
    n = os.path.getsize(path)
    with open(path, "rb") as f, mmap.mmap(f.fileno(), n, access=mmap.ACCESS_COPY) as m:
        buf = (C.c_char * n).from_buffer(m)
        try:
            k, crc, ln = walk_piece(C.addressof(buf), n)
        finally:
            del buf
    assert k > 0
    return crc, ln


def run_cli(name, argv, d, extra=()):
    """the `pbsim` binary with its default GPU gzip into d: [(crc, length) of the reads' text, of the MAF], stripped stderr"""
    case = FULLSIZE[name]
    import pbsim3_amd.build as b
    b.build()
    out = os.path.join(d, "out")
    p = subprocess.run([CLI] + harness.resolve(case["args"]) + argv + ["--prefix", out] + list(extra), capture_output=True,
                       text=True, cwd=d)
    assert p.returncode == 0, p.stderr[-4000:]
    stem = out if "transcripts" in case else out + "_0001"
    got = []
    for ext in (".fq.gz", ".maf.gz"):
        got.append(walk_file(stem + ext))
        os.remove(stem + ext)
    return got, harness.strip_report(p.stderr)


def need_room(d, gib):
    free = shutil.disk_usage(d).free
    if free < gib << 30:
        pytest.skip("the CLI legs write %d GiB of gzip output; %s has %.1f GiB free" % (gib, d, free / (1 << 30)))


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("name,gib", [(TRANS, 8), (SAMPLE, 4)])
def test_cli_equals_the_reference(name, gib, tmp_path, request):
    """the `pbsim` binary on the generated files (trans: its fgets-compatible parser; sample: its own quality filter), one
    rank and --devices 0,0,0: the files' members and the WHOLE stripped report (transcript / sample stats, parameters)"""
    inp = request.getfixturevalue("trans_inputs" if name == TRANS else "sample_inputs")
    argv = ["--transcript", inp["path"]] if name == TRANS else inp["argv"]
    need_room(str(tmp_path), gib)
    e = harness.load_fullsize()[name]
    want = [(int(e[k]["crc32"], 16), e[k]["bytes"]) for k in (".fq", ".maf")]
    for extra in ((), ("--devices", "0,0,0")):
        d = tmp_path / ("m" if extra else "one")
        d.mkdir()
        got, report = run_cli(name, argv, str(d), extra)
        assert got == want, extra
        assert report == e["stderr"], extra
