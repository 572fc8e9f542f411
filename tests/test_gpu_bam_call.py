"""`pbsim --call-bam` (pbsim_bam_call) on the device, held to tests/call_model.py byte for byte: counts, site totals, the variant
counts, the report, the VCF and the per-record counts, with the text and without it."""
import ctypes as C
import os
import random
import subprocess

import pytest

import bam_writer as B
import call_model as V
import harness
import pbsim3_amd as P
from test_call_model import (GENOME, REFS as WORKED_REFS, REFUSED_OPTS, WORKED, WORKED_HEADER, WORKED_LINES, WORKED_OPTIONS, WORKED_REPORT, lines_of)
from test_gpu_bam_consensus import exact
from test_gpu_bam_errors import aligned, fasta_lines, planted
from test_pileup_model import GENOME as PILE_GENOME, WORKED as PILE_WORKED, WORKED_REFS as PILE_REFS, rec, small_case

pytestmark = pytest.mark.gpu

TILE = 256


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


def compare(got, want):
    result, report = got[0], got[1]
    assert [result["counts"][n] for n in V.COUNT_NAMES] == want.counts
    assert [result["sites"][n] for n in V.SITE_NAMES] == want.sites
    assert (result["ins_unanchored"], result["max_depth"]) == (want.ins_unanchored, want.max_depth)
    assert (result["variants"], [result["types"][n] for n in V.TYPE_NAMES]) == (want.variants, want.types)
    assert [result[n] for n in V.SCALARS] == [getattr(want, n) for n in V.SCALARS]
    assert (result["header_bytes"], result["text_bytes"]) == (want.header_bytes, want.text_bytes)
    assert report == want.report


def check(ctx, streams, genome, container="bgzf", block=B.W.BGZIP_BLOCK, piece_bytes=0, want=None, **kw):
    """inflated streams -> through the product in `container`, every output against the model, with the text and without it;
    returns the model's result"""
    if isinstance(streams, (bytes, bytearray)):
        streams = [streams]
    want = want or V.call(streams, genome, **kw)
    files = [B.contain(s, container, block) for s in streams]
    got = ctx.bam_call(files, genome, piece_bytes=piece_bytes, **kw)
    compare(got, want)
    assert got[2] == want.text and got[3] == want.records
    bare = ctx.bam_call(files, genome, text=False, **kw)
    assert len(bare) == 2
    compare(bare, want)
    return want


def say(name, ref, s, e, subs=(), dels=(), inss=(), ref_id=0, clip=0):
    """the record on reference ref_id that covers [s, e) of `ref` and says the alternate sequence there, noise-free and without
    qualities; an insertion may stand behind a deleted position; `clip` soft-clipped bases in front (a record needs one base)"""
    subs, inss = dict(subs), dict(inss)
    ops, seq = [(clip, "S")] * (clip > 0), ["A"] * clip

    def add(n, op):
        if ops and ops[-1][1] == op:
            ops[-1] = (ops[-1][0] + n, op)
        else:
            ops.append((n, op))
    for p in range(s, e):
        if p in dels:
            add(1, "D")
        else:
            add(1, "M")
            seq.append(chr(subs.get(p, ref[p])))
        if p in inss:
            add(len(inss[p]), "I")
            seq.extend(inss[p])
    return exact(name, "".join(seq), s, ops, ref=ref_id)


def places(lengths):
    """where the genome's records begin in the device's buffers: every record's bases rounded up to 64, and 64 behind them"""
    at, out = 0, []
    for n in lengths:
        out.append(at)
        at += (n + 63) // 64 * 64 + 64
    return out


def other(ref, p):
    return b"ACGT"[(b"ACGT".index(ref[p]) + 1) % 4]


# ---------------------------------------------------------------- the worked cases
def test_the_worked_cases(ctx):
    r = check(ctx, B.stream(WORKED, WORKED_REFS), GENOME)
    assert r.text == WORKED_HEADER + WORKED_LINES and r.report == WORKED_REPORT
    assert check(ctx, [B.stream(WORKED[3:], WORKED_REFS), B.stream(WORKED[:3], WORKED_REFS)], GENOME).text == r.text
    assert check(ctx, [B.stream(WORKED[:3], WORKED_REFS), B.stream(WORKED[3:], WORKED_REFS)], GENOME).text == r.text
    # the pileup's worked case: skipped and misfit records, qualities that mask, a deleted base its own insertion puts back
    r = check(ctx, B.stream(PILE_WORKED, PILE_REFS), PILE_GENOME)
    assert r.variants == 2 and r.sites[8] == 4
    check(ctx, B.stream(PILE_WORKED, PILE_REFS), PILE_GENOME, min_baseq=21, min_depth=2)


@pytest.mark.parametrize("kw", WORKED_OPTIONS, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_the_worked_case_with_an_option_moved(ctx, kw):
    moved = check(ctx, B.stream(WORKED, WORKED_REFS), GENOME, **kw)
    plain = V.call(B.stream(WORKED, WORKED_REFS), GENOME)
    # (no insertion is longer; the bare site is called as the genome's base; no flags, no qualities)
    same = kw in (dict(max_ins=2), dict(min_depth=0), dict(exclude_flags=0), dict(min_baseq=1))
    assert (moved.text != plain.text) != same and (moved.report != plain.report) == (kw in (dict(min_depth=4), dict(min_depth=0), dict(min_mapq=61)) or
                                                                                     len(kw) > 1 or kw == dict(max_ins=1))


# ---------------------------------------------------------------- tiles
@pytest.mark.parametrize("l_ref", [255, 256, 257])
@pytest.mark.parametrize("reverse", [False, True], ids=["in order", "reversed"])
def test_groups_at_the_edges_of_tiles_and_records(ctx, l_ref, reverse):
    """e0 ends on an ins_site (at 257 positions: an ins_site on a tile's last position whose deleted neighbour is the next tile's
    first and the record's last); records of one base and of none; e1 with an anchor on the last position of a tile and its
    deletion run in the next, an ins_site there, and a sub_site on a tile's first position"""
    rng = random.Random(l_ref)
    e0, e1 = planted(rng, 400, longest=4)[:l_ref], planted(rng, 900, longest=4)[:700]
    names = [("e0", e0), ("one", b"G"), ("none", b""), ("e1", e1)]
    if reverse:
        names = names[::-1]
    gen = [(n, fasta_lines(s, 50)) for n, s in names]
    order = [n for n, _ in names]
    refs = [(n, len(s)) for n, s in names if n != "none"]           # (a BAM header has no reference of length 0)
    ids = {n: k for k, (n, _) in enumerate(refs)}
    seqs = {ids["e0"]: e0, ids["one"]: b"G", ids["e1"]: e1}
    at = places([len(s) for _, s in names])[order.index("e1")]
    last = [p for p in range(len(e1)) if (at + p) % TILE == TILE - 1]
    assert len(last) >= 2 and last[0] + 5 < last[1] < len(e1) - 10
    a, b = last[0], last[1]
    ops = [(l_ref, "M"), (2, "I")] if l_ref < 257 else [(256, "M"), (2, "I"), (1, "D")]
    recs = [aligned("whole", ops, pos=0, ref=ids["e0"], rng=random.Random(1), seqs=seqs, keep=1.0, qual="none")] * 3
    recs += [aligned("gi", [(1, "M"), (3, "I")], pos=0, ref=ids["one"], rng=random.Random(3), seqs=seqs, keep=1.0, qual="none")] * 2
    subs = {b + 1: other(e1, b + 1), 5: other(e1, 5)}
    recs += [say("run", e1, 0, len(e1), subs=subs, dels=(a + 1, a + 2, a + 3), inss={b: "TT"}, ref_id=ids["e1"])] * 3
    r = check(ctx, B.stream(recs, refs), gen)
    got = lines_of(r.text)
    assert r.records[order.index("none")] == (0, 0) and r.records[order.index("one")] == (1, 1) and r.records[order.index("e1")] == (700, 4)
    assert any(line.startswith(b"e1\t%d\t.\t" % (a + 1) + e1[a:a + 4] + b"\t" + e1[a:a + 1] + b"\t") for line in got)
    assert any(line.startswith(b"e1\t%d\t.\t" % (b + 1) + e1[b:b + 1] + b"\t" + e1[b:b + 1] + b"TT\t") for line in got)
    assert any(line.startswith(b"e1\t%d\t.\t" % (b + 2)) and line.endswith(b"TYPE=snv") for line in got)
    if l_ref == 257:
        assert any(line.startswith(b"e0\t256\t.\t" + e0[255:257] + b"\t" + e0[255:256]) and line.endswith(b"TYPE=complex") for line in got)
    else:
        assert any(line.startswith(b"e0\t%d\t.\t" % l_ref) and line.endswith(b"TYPE=ins") for line in got)


# ---------------------------------------------------------------- a long deletion run
@pytest.mark.parametrize("kind", ["plain", "ins inside", "leading"])
def test_a_deletion_run_of_six_hundred_positions(ctx, kind):
    rng = random.Random(600)
    ref = planted(rng, 1100, longest=4)[:1000]
    gen, refs = [("front", b"ACGTACGT\n"), ("long", fasta_lines(ref))], [("front", 8), ("long", 1000)]
    if kind == "leading":
        recs = [say("d", ref, 0, 800, dels=range(0, 600), ref_id=1)] * 3
    else:
        inss = {400: "GATTACA"} if kind == "ins inside" else {}
        recs = [say("d", ref, 100, 900, dels=range(150, 750), inss=inss, ref_id=1)] * 3
    r = check(ctx, B.stream(recs, refs), gen)
    assert r.variants == 1 and r.longest_ref == 601 and r.sites[6] == 600 and r.records == [(8, 0), (1000, 1)]
    line = lines_of(r.text)[0]
    if kind == "leading":
        kind = b"del" if ref[0] == ref[600] else b"complex"         # (ALT is the base behind the run)
        assert line == b"long\t1\t.\t" + ref[:601] + b"\t" + ref[600:601] + b"\t.\t.\tDP=3;MS=3;TYPE=" + kind
    elif kind == "plain":
        assert line == b"long\t150\t.\t" + ref[149:750] + b"\t" + ref[149:150] + b"\t.\t.\tDP=3;MS=3;TYPE=del"
    else:
        assert line == b"long\t150\t.\t" + ref[149:750] + b"\t" + ref[149:150] + b"GATTACA\t.\t.\tDP=3;MS=3;TYPE=complex"


# ---------------------------------------------------------------- several genome records
def test_deletion_runs_on_both_sides_of_a_records_end(ctx):
    rng = random.Random(31)
    p, q = planted(rng, 200, longest=4)[:128], planted(rng, 200, longest=4)[:130]       # (128: p fills its 64-byte blocks to the last byte)
    gen, refs = [("p", fasta_lines(p)), ("q", fasta_lines(q))], [("p", 128), ("q", 130)]
    recs = [say("p", p, 60, 128, dels=range(120, 128))] * 3 + [say("q", q, 0, 90, dels=range(0, 7), ref_id=1)] * 3
    r = check(ctx, B.stream(recs, refs), gen)
    assert lines_of(r.text) == [b"p\t120\t.\t" + p[119:128] + b"\t" + p[119:120] + b"\t.\t.\tDP=3;MS=3;TYPE=del",
                                b"q\t1\t.\t" + q[:8] + b"\t" + q[7:8] + b"\t.\t.\tDP=3;MS=3;TYPE=complex"]
    assert r.records == [(128, 1), (130, 1)] and check(ctx, B.stream(recs, refs), gen, min_depth=4).variants == 0


def test_a_wholly_deleted_record_between_two_others(ctx):
    rng = random.Random(32)
    a, gone, b = planted(rng, 100, longest=4)[:70], planted(rng, 400, longest=4)[:300], planted(rng, 100, longest=4)[:64]
    gen = [("a", fasta_lines(a)), ("gone", fasta_lines(gone)), ("b", fasta_lines(b))]
    refs = [("a", 70), ("gone", 300), ("b", 64)]
    recs = [say("a", a, 0, 70, dels=range(60, 70))] * 2 + [say("g", gone, 0, 300, dels=range(300), ref_id=1, clip=1)] * 2
    recs += [say("b", b, 0, 64, dels=range(0, 3), subs={3: other(b, 3)}, ref_id=2)] * 2
    r = check(ctx, B.stream(recs, refs), gen)
    assert (r.unplaced_records, r.unplaced_sites, r.variants) == (1, 300, 2) and r.records == [(70, 1), (300, 0), (64, 1)]
    assert lines_of(r.text)[1].startswith(b"b\t1\t.\t" + b[:4] + b"\t" + bytes([other(b, 3)]) + b"\t")
    # every record wholly deleted, one of them a single base
    r = check(ctx, B.stream([say("g", gone, 0, 300, dels=range(300), clip=2)] + [say("o", b"G", 0, 1, dels=(0,), ref_id=1, clip=1)], [("gone", 300), ("o", 1)]),
              [("gone", fasta_lines(gone)), ("o", b"G\n")])
    assert (r.unplaced_records, r.unplaced_sites, r.variants) == (2, 301, 0)


# ---------------------------------------------------------------- insertions
@pytest.mark.parametrize("max_ins", [1, 64, 1024])
def test_an_insertion_of_seventy_bases(ctx, max_ins):
    rng = random.Random(70)
    ref = planted(rng, 700, longest=4)[:600]
    one = aligned("seventy", [(40, "M"), (70, "I"), (40, "M")], pos=300, rng=random.Random(70), keep=1.0, qual="none", seqs={0: ref})
    r = check(ctx, B.stream([one] * 3, [("v", 600)]), [("v", fasta_lines(ref))], max_ins=max_ins)
    assert (r.variants, r.types, r.longest_ref, r.longest_alt) == (1, [0, 1, 0, 0], 1, 1 + min(70, max_ins))


def test_a_sub_site_with_its_insertion_and_a_deletion_behind_is_one_record(ctx):
    recs = [rec("x%d" % k, 0, "2M2I1D1M", "ATGGT") for k in range(3)] + [rec("y", 0, "4M", "ACGT")]
    r = check(ctx, B.stream(recs, [("a", 4)]), [("a", b"ACGT\n")])
    assert lines_of(r.text) == [b"a\t2\t.\tCG\tTGG\t.\t.\tDP=4;MS=3;TYPE=complex"]
    # a leading run behind a soft clip, with and without an insertion at the deleted site
    r = check(ctx, B.stream([rec("x%d" % k, 0, "1S2D2M", "ATT") for k in range(3)], [("a", 4)]), [("a", b"ACGT\n")])
    assert lines_of(r.text) == [b"a\t1\t.\tACG\tT\t.\t.\tDP=3;MS=3;TYPE=complex"]
    r = check(ctx, B.stream([rec("x%d" % k, 0, "1S1D1I3M", "GTCGT") for k in range(3)], [("a", 4)]), [("a", b"ACGT\n")])
    assert lines_of(r.text) == [b"a\t1\t.\tAC\tTC\t.\t.\tDP=3;MS=3;TYPE=complex"]
    assert check(ctx, B.stream([rec("x%d" % k, 0, "1S1D1I3M", "GACGT") for k in range(3)], [("a", 4)]), [("a", b"ACGT\n")]).variants == 0


# ---------------------------------------------------------------- random
@pytest.mark.parametrize("seed,kw", [(0, dict()), (1, dict(min_depth=2)), (2, dict(min_baseq=20, max_ins=2)), (3, dict(min_mapq=30)),
                                     (4, dict(exclude_flags=0x10, min_depth=0)), (5, dict(min_depth=2, min_baseq=10, min_mapq=5, exclude_flags=0))],
                         ids=lambda x: ",".join("%s=%s" % i for i in x.items()) if isinstance(x, dict) else str(x))
def test_random_records_with_the_options_moved(ctx, seed, kw):
    genome, refs, recs, rng = small_case(seed)
    r = check(ctx, B.stream(recs, refs), genome, **kw)
    assert r.variants > 20 and r.types[1] > 0 and r.types[2] > 0
    if seed == 0:                                   # three files, in another order of records
        mixed = list(recs)
        rng.shuffle(mixed)
        check(ctx, [B.stream(part, refs) for part in (mixed[:30], mixed[30:90], mixed[90:])], genome, block=1024, want=r, **kw)


# ---------------------------------------------------------------- the text's delivery
def deliver(ctx, datas, genome, piece_bytes, stop_after=None, stop_records=None):
    pieces, records = [], []

    def on_text(user, ptr, n, offset):
        pieces.append((offset, C.string_at(ptr, n)))
        return 0 if stop_after is not None and len(pieces) >= stop_after else 1

    def on_record(user, ref, l_ref, n_variants):
        records.append((ref, l_ref, n_variants))
        return 0 if stop_records is not None and len(records) >= stop_records else 1
    sink = P.CallSink(None, P.CALL_TEXT_CB(on_text), P.CALL_RECORD_CB(on_record))
    opts = P.CallOpts(0x900, 0, 0, 1024, 1, piece_bytes)
    keep = [(nm.encode(), bytes(lines)) for nm, lines in genome]
    refs = (P.ErrorsRef * len(keep))(*[P.ErrorsRef(nm, C.cast(C.c_char_p(lines), C.c_void_p), len(lines)) for nm, lines in keep])
    arr = (P.ErrorsFile * len(datas))(*[P.ErrorsFile(C.cast(C.c_char_p(d), C.c_void_p), len(d), None) for d in datas])
    res = P.CallResult()
    ok = ctx.lib.pbsim_bam_call(ctx.h, refs, len(keep), arr, len(datas), C.byref(opts), C.byref(sink), C.byref(res))
    return ok, pieces, records, res


def test_delivery_in_pieces_and_the_header_alone(ctx):
    want = V.call(B.stream(WORKED, WORKED_REFS), GENOME)
    datas = [B.bam(WORKED, WORKED_REFS)]
    for piece in (0, 1, 7, 4096):
        ok, pieces, records, res = deliver(ctx, datas, GENOME, piece)
        assert ok == 1 and b"".join(p for _, p in pieces) == want.text and res.text_bytes == len(want.text) and res.header_bytes == want.header_bytes
        assert records == [(k, a, b) for k, (a, b) in enumerate(want.records)]
        at = 0
        for offset, p in pieces:
            assert offset == at and 1 <= len(p) <= (piece or len(want.text))
            at += len(p)
        assert piece not in (1, 7) or len(pieces) == -(-len(want.text) // piece)
    ok, pieces, _, res = deliver(ctx, datas, GENOME, 7, stop_after=3)
    assert ok == 0 and len(pieces) == 3 and b"sink aborted (text)" in ctx.lib.pbsim_last_error() and sum(res.counts) == 0 and res.text_bytes == 0
    ok, _, records, res = deliver(ctx, datas, GENOME, 0, stop_records=1)
    assert ok == 0 and len(records) == 1 and b"sink aborted (records)" in ctx.lib.pbsim_last_error() and sum(res.counts) == 0
    # no records at all: the header alone, in pieces too
    r = check(ctx, B.stream([], WORKED_REFS), GENOME, piece_bytes=7)
    assert r.text == WORKED_HEADER and r.variants == 0 and r.counts == [0] * 9
    for container in ("stored", "gzip", "none"):
        check(ctx, B.stream(WORKED, WORKED_REFS), GENOME, container=container, block=1024, piece_bytes=1, want=want)


# ---------------------------------------------------------------- failures
def test_failures_say_why_and_leave_the_context_usable(ctx):
    def usable():
        assert check(ctx, B.stream(WORKED, WORKED_REFS), GENOME).report == WORKED_REPORT

    data = B.bam(WORKED, WORKED_REFS)
    for kw, word in REFUSED_OPTS:
        with pytest.raises(P.PbsimError, match="pbsim_bam_call: " + word):
            ctx.bam_call(data, GENOME, **kw)
    with pytest.raises(P.PbsimError, match="pbsim_bam_call: bad argument"):
        ctx.bam_call(data, [])
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_call: the genome holds two records named \"c1\""):
        ctx.bam_call(data, GENOME + [("c1", b"AC")])
    usable()
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_call: the reference \"c1\" has l_ref 11 in the file's header, and the genome's record of that "
                                           r"name has 10 bases"):
        ctx.bam_call(B.bam(WORKED, [("c1", 11), ("c2", 5)]), GENOME)
    usable()
    with pytest.raises(P.PbsimError, match="pbsim_bam_call: file 0 has 2 references: a reference name can be given only to a file with exactly one"):
        ctx.bam_call(data, GENOME, ref_names=["c1"])
    usable()
    with pytest.raises(P.PbsimError, match="pbsim_bam_call: neither BGZF, gzip nor an uncompressed BAM"):
        ctx.bam_call(b"@HD\tVN:1.6\n", GENOME)
    usable()


# ---------------------------------------------------------------- through the command line
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def test_cli_writes_the_models_text_and_report(tmp_path):
    genome, refs, recs, _ = small_case(6)
    fasta = tmp_path / "genome.fa"
    fasta.write_bytes(b"".join(b">" + n.encode() + b" a description\n" + lines + b"\n" for n, lines in genome))
    half = len(recs) // 2
    for k, part in enumerate((recs[:half], recs[half:])):
        (tmp_path / ("in%d.bam" % k)).write_bytes(B.bam(part, refs))
    out = tmp_path / "out.vcf"
    cmd = [CLI, "--call-bam", "in0.bam", "--call-bam", "in1.bam", "--call-genome", str(fasta), "--call-out", str(out)]
    r = subprocess.run(cmd, capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    want = V.call([B.stream(recs[:half], refs), B.stream(recs[half:], refs)], genome)
    assert out.read_bytes() == want.text and r.stdout == want.report and want.variants > 20
    r = subprocess.run(cmd + ["--call-min-depth", "2", "--call-max-ins", "1", "--call-min-baseq", "15", "--call-min-mapq", "10", "--call-exclude-flags", "0x10"],
                       capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    want = V.call([B.stream(recs[:half], refs), B.stream(recs[half:], refs)], genome, min_depth=2, max_ins=1, min_baseq=15, min_mapq=10, exclude_flags=0x10)
    assert out.read_bytes() == want.text and r.stdout == want.report
    # a failure leaves no file behind
    r = subprocess.run([CLI, "--call-bam", "in0.bam", "--call-genome", str(fasta), "--call-ref-names", "s0", "--call-out", str(out)], capture_output=True,
                       cwd=str(tmp_path), timeout=300)
    assert r.returncode != 0 and b"a reference name can be given only to a file with exactly one" in r.stderr and not out.exists()
