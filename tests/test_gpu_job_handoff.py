"""The job pipeline's lane hand-off (csrc/job.cpp, deflate_host.cpp): a delivery lane that has launched the last
piece of its round launches the head of the NEXT round's compression on the shared lane stream, so that the next round's
lane calls start with a copy.  Whatever the hand-off does -- head taken, head not taken in time, head launched for a round
that is then cut short, dropped or written again -- the members a job delivers inflate (CRC-32 and ISIZE of every member
checked) to exactly the text of the same job with PBSIM_JOB_HANDOFF=0 and of the same job delivered as plain text, and the
statistics are equal.  PBSIM_TRACE shows whether heads were handed off at all, so the tests cannot pass with the feature
silently off."""
import ctypes as C
import os
import subprocess
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import harness

pytestmark = pytest.mark.gpu
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")
HANDED = "found its head handed off"


class Stream:
    """one output stream of one record, written at the offsets the sink is given (a growing numpy buffer: no per-piece objects)"""

    def __init__(self, cap):
        self.buf = np.empty(max(cap, 1 << 16), dtype=np.uint8)
        self.n = 0

    def put(self, ptr, n, off):
        if off + n > self.buf.size:
            self.buf = np.concatenate([self.buf, np.empty(max(self.buf.size, off + n - self.buf.size), dtype=np.uint8)])
        C.memmove(self.buf.ctypes.data + off, ptr, n)
        self.n = max(self.n, off + n)
        return 1

    def view(self):
        return self.buf[:self.n]


def run_job(P, ctx, n_recs, cap):
    """the context's job through a sink of this test's: {record: (read Stream, maf Stream)}, {record: (Stats fields, bytes, bytes)}"""
    out = {r + 1: (Stream(cap), Stream(cap)) for r in range(n_recs)}
    done = {}

    def fin(user, rec, st, rb, mb):
        s = P.Stats()
        C.memmove(C.byref(s), st, C.sizeof(P.Stats))
        done[rec] = (bytes(s), rb, mb)
        return 1

    cbs = (P.REC_TEXT_CB(lambda u, r, t, n, o: out[r][0].put(t, n, o)), P.REC_TEXT_CB(lambda u, r, t, n, o: out[r][1].put(t, n, o)),
           P.REC_DONE_CB(fin))
    sink = P.RecordSink(None, *cbs)
    P._check(ctx.lib.pbsim_job_run(ctx.h, None, C.byref(sink)))
    for rec, (_, rb, mb) in done.items():
        assert (out[rec][0].n, out[rec][1].n) == (rb, mb), rec
    return out, done


def member_table(gz):
    """[(offset, size, text offset, text size)] of a stream of BGZF-framed gzip members, from the framing and the trailers alone"""
    tab, at, tat = [], 0, 0
    n = gz.size
    while at < n:
        assert bytes(gz[at:at + 4]) == b"\x1f\x8b\x08\x04" and bytes(gz[at + 10:at + 16]) == b"\x06\x00BC\x02\x00", "member header at %d" % at
        size = int(gz[at + 16]) + (int(gz[at + 17]) << 8) + 1
        assert at + size <= n, "BSIZE at %d" % at
        isize = int.from_bytes(bytes(gz[at + size - 4:at + size]), "little")
        tab.append((at, size, tat, isize))
        at += size
        tat += isize
    return tab, tat


def check_members_against(gz, text, what):
    """every member of gz inflates, its CRC-32 and ISIZE verify, and the inflated stream equals `text` byte for byte"""
    tab, total = member_table(gz)
    assert total == text.size, (what, total, text.size)
    gzb, tb = memoryview(gz), memoryview(text)

    def group(rows):
        for at, size, tat, isize in rows:
            d = zlib.decompressobj(-15)
            t = d.decompress(gzb[at + 18:at + size - 8])
            assert d.eof and d.unused_data == b"", (what, "deflate stream and trailer at %d" % at)
            assert len(t) == isize and zlib.crc32(t) == int.from_bytes(gzb[at + size - 8:at + size - 4], "little"), (what, "CRC-32 / ISIZE at %d" % at)
            assert t == tb[tat:tat + isize], (what, "text at %d" % tat)
        return len(rows)

    step = 512
    with ThreadPoolExecutor(16) as ex:            # (zlib releases the interpreter lock)
        assert sum(ex.map(group, [tab[i:i + step] for i in range(0, len(tab), step)])) == len(tab)
    return len(tab)


def three_ways(monkeypatch, capfd, G, depth, target, seed=3, clear=None, n_recs=1, want_handed=True, len_mean=None):
    """the job with the hand-off, without it, and delivered as plain text: members, text and statistics compared"""
    import torch
    import pbsim3_amd as P
    kw = dict(len_mean=len_mean, len_sd=0.7 * len_mean) if len_mean else {}
    p = P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=seed, depth=depth, **kw)
    monkeypatch.setenv("PBSIM_JOB_TARGET_RANKS", str(target))
    monkeypatch.setenv("PBSIM_TRACE", "1")
    if clear is not None:
        monkeypatch.setenv("PBSIM_JOB_CLEAR", clear)
    recs = [harness.synth_bases_torch(G, 40 + i) for i in range(n_recs)]
    torch.cuda.synchronize()
    res = {}
    cap = int(G * depth * 1.3) + (1 << 20)
    with P.Context(p, 0) as ctx:
        ctx.load_errhmm(harness.model_path("ERRHMM-ONT.model"))
        for t in recs:
            ctx.job_add_record_device(t.data_ptr(), G)
        for mode in ("on", "off", "text"):
            ctx.set_deflate(0 if mode == "text" else 7)
            monkeypatch.setenv("PBSIM_JOB_HANDOFF", "0" if mode == "off" else "1")
            capfd.readouterr()
            out, done = run_job(P, ctx, n_recs, (3 * cap) if mode == "text" else cap)
            res[mode] = (out, done, capfd.readouterr().err, ctx.job_counters()["rounds"])
    on, off, text = res["on"], res["off"], res["text"]
    assert HANDED not in off[2] and HANDED not in text[2]
    if want_handed:
        assert HANDED in on[2], on[2][-3000:]
    assert sorted(on[1]) == sorted(off[1]) == sorted(text[1]) == list(range(1, n_recs + 1))
    for rec in on[1]:
        assert on[1][rec][0] == off[1][rec][0] == text[1][rec][0], ("statistics", rec)
        assert on[1][rec][1:] == off[1][rec][1:], ("compressed sizes", rec)
        for w in (0, 1):
            what = (rec, "reads" if w == 0 else "maf")
            a, b, t = on[0][rec][w].view(), off[0][rec][w].view(), text[0][rec][w].view()
            assert t.size > 0
            assert check_members_against(a, t, what) >= 1
            if not np.array_equal(a, b):      # (the same members: checked once; otherwise the other stream is checked as well)
                check_members_against(b, t, what)
    return on


def test_one_piece_per_call(monkeypatch, capfd):
    """rounds of one piece per lane: the tail hook comes up at the end of the call's head start (n_pieces <= ahead) and again
    behind its only copy"""
    on = three_ways(monkeypatch, capfd, G=3_000_000, depth=40.0, target=2e7)
    assert on[3] >= 6


def test_more_than_five_pieces_per_lane_call(monkeypatch, capfd):
    """1.3 Gbases in rounds of a fifth, a half, one and the rest of 6.9e8 bases: the full round's MAF text (1.45 GB) takes six
    pieces of 256 MiB, so its lane's hook fires from inside the piece loop -- with a round behind it to take -- and the lane's
    dense buffers are re-used while the next round's head is queued behind them"""
    monkeypatch.setenv("PBSIM_DEFLATE_TRACE", "1")
    on = three_ways(monkeypatch, capfd, G=26_000_000, depth=50.0, target=6.4e8)
    assert on[3] >= 4
    mb = [float(l.split("[deflate] ")[1].split(" MB")[0]) for l in on[2].splitlines() if l.startswith("[deflate] ") and " MB -> " in l]
    assert max(mb) * 1e6 > 5 * (256 << 20), mb          # a lane call of six pieces or more


@pytest.mark.parametrize("clear", ["0", "1"])
def test_cutting_and_clear_missed_rounds(clear, monkeypatch, capfd):
    """PBSIM_JOB_CLEAR=0: every round exchanges first and emits its text behind the cut; =1: every round emits first, and the
    rounds that touch the quota emit again -- the descriptor follows the second emission"""
    on = three_ways(monkeypatch, capfd, G=4_000_000, depth=40.0, target=2e7, clear=clear)
    assert ("cutting" if clear == "0" else "clear-missed") in on[2]


def test_quota_ends_inside_the_first_round(monkeypatch, capfd):
    """two records whose quota the job's first round already passes: the round published behind it is dropped, and the next
    record's rounds take the slot"""
    on = three_ways(monkeypatch, capfd, G=600_000, depth=3.0, target=5e7, n_recs=3, want_handed=False)
    assert on[3] == 3                               # one bulk round per record


def test_two_ranks_discard_a_head(tmp_path):
    """two ranks (contexts on the one GPU, host-barrier communicator of the CLI): the members wait in the lanes' arenas, and the
    block behind a record's cut is void -- a head launched for it is discarded.  Files equal with and without the hand-off, and
    their inflated text equals the files of --no-gzip."""
    import pbsim3_amd.build as b
    b.build()
    G = 3_000_000
    seq = harness.synth_bases(G, 9)
    fa = tmp_path / "g.fa"
    with open(fa, "wb") as f:
        f.write(b">chr1\n")
        lines = seq.reshape(-1, 60)
        f.write(np.concatenate([lines, np.full((lines.shape[0], 1), 10, np.uint8)], axis=1).tobytes())
    args = ["--strategy", "wgs", "--method", "errhmm", "--errhmm", harness.model_path("ERRHMM-ONT.model"), "--genome", str(fa),
            "--depth", "30", "--seed", "11"]
    outs = {}
    for mode in ("on", "off", "text"):
        wd = tmp_path / mode
        wd.mkdir()
        e = dict(os.environ, PBSIM_JOB_TARGET_RANKS="8e6", PBSIM_TRACE="1", PBSIM_JOB_HANDOFF="0" if mode == "off" else "1")
        p = subprocess.run([CLI] + args + ["--prefix", str(wd / "out"), "--devices", "0,0"] + (["--no-gzip"] if mode == "text" else []),
                           capture_output=True, text=True, cwd=str(wd), env=e, timeout=300)
        assert p.returncode == 0, p.stderr[-4000:]
        outs[mode] = (harness.collect(str(wd)), p.stderr)
    assert HANDED not in outs["off"][1] and HANDED not in outs["text"][1]


    def report(err):                                # the statistics, without the trace lines
        return harness.strip_report("\n".join(l for l in err.splitlines() if not l.startswith("[")) + "\n")

    assert report(outs["on"][1]) == report(outs["off"][1]) == report(outs["text"][1])
    assert sorted(outs["on"][0]) == sorted(outs["off"][0]) == sorted(outs["text"][0])
    seen = 0
    for k, v in outs["on"][0].items():              # (harness.collect names a .fq.gz like its .fq)
        assert v == outs["off"][0][k], k
        if k.endswith((".fq", ".maf")):
            assert v[:4] == b"\x1f\x8b\x08\x04", k
            check_members_against(np.frombuffer(v, dtype=np.uint8), np.frombuffer(outs["text"][0][k], dtype=np.uint8), k)
            seen += 1
        else:
            assert v == outs["text"][0][k], k
    assert seen >= 2, sorted(outs["on"][0])
