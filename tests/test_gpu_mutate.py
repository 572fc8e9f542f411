"""`pbsim --mutate-genome` (pbsim_genome_mutate) on the device, held to tests/mutate_model.py byte for byte: the result, the report,
the FASTA, the VCF, the per-record numbers and the origin maps, with the texts and without them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bam_writer as B
import bgzf_writer as W
import harness
import mutate_model as G
import pbsim3_amd as P
from test_call_model import lines_of
from test_gpu_bam_call import places
from test_mutate_model import (REFUSED_OPTS, WORKED_FASTA, WORKED_GENOME, WORKED_HEADER, WORKED_LINES, WORKED_OPTIONS, WORKED_ORIGINS, WORKED_REPORT,
                               bases_of, first_five, four_records, spelling_reads)

pytestmark = pytest.mark.gpu

TILE = 256
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


def compare(got, want):
    result, report = got[0], got[1]
    values = [[result[n][t] for t in G.TYPE_NAMES] if n in ("drawn", "types") else result[n] for n in G.FIELDS]
    assert values == list(want[:20])
    assert report == want.report


def check(ctx, genome, piece_bytes=0, want=None, **kw):
    """the genome through the product, every output against the model, with the texts and the origin maps and without them; returns
    the model's result"""
    want = want or G.mutate(genome, **kw)
    got = ctx.mutate_genome(genome, origin=True, piece_bytes=piece_bytes, **kw)
    assert len(got) == 6
    compare(got, want)
    assert got[2] == want.fasta and got[3] == want.vcf and got[4] == want.per_record
    assert len(got[5]) == len(want.origins) and all(a.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(got[5], want.origins))
    bare = ctx.mutate_genome(genome, text=False, **kw)
    assert len(bare) == 2
    compare(bare, want)
    return want


# ---------------------------------------------------------------- the worked case
def test_the_worked_case(ctx):
    r = check(ctx, WORKED_GENOME, **WORKED_OPTIONS)
    assert r.fasta == WORKED_FASTA and r.vcf == WORKED_HEADER + WORKED_LINES and r.report == WORKED_REPORT
    assert [o.tolist() for o in r.origins] == WORKED_ORIGINS
    # the texts alone, the maps alone
    texts = ctx.mutate_genome(WORKED_GENOME, **WORKED_OPTIONS)
    assert len(texts) == 5 and texts[2:] == (WORKED_FASTA, WORKED_HEADER + WORKED_LINES, [(31, 13, 7), (7, 8, 1)])
    maps = ctx.mutate_genome(WORKED_GENOME, text=False, origin=True, **WORKED_OPTIONS)
    assert len(maps) == 3 and [o.tolist() for o in maps[2]] == WORKED_ORIGINS and maps[1] == WORKED_REPORT


# ---------------------------------------------------------------- tiles
RATES = dict(snv_ppm=250000, ins_ppm=200000, del_ppm=250000, ext_ppm=600000, max_indel=9)
FEATURES = ["del", "merged", "ins", "snv"]
SPOTS = ["a tile's last position", "a tile's first position", "a record's last position"]


def features_of(genome, seed):
    """which of FEATURES x SPOTS the seed puts into the genome, by the model's events"""
    records, found = G.prepared_records(genome), set()
    at = places([len(seq) for _, seq in records])
    opts = dict(G.DEFAULTS, seed=seed, **RATES)
    for r, ((_, seq), first) in enumerate(zip(records, at)):
        n = len(seq)
        if n < 2:
            continue
        _, kind, _, _, deleted, _ = G.sites(seq, r, opts)
        here = {SPOTS[0]: [p for p in range(n - 1) if (first + p) % TILE == TILE - 1], SPOTS[1]: [p for p in range(1, n - 1) if (first + p) % TILE == 0]}
        for spot, where in here.items():
            for p in where:                         # an anchor with its run behind it; a del inside a run; an ins and an snv that are written
                found |= {(f, spot) for f, yes in zip(FEATURES, (kind[p] == G.DEL and not deleted[p], kind[p] == G.DEL and deleted[p],
                                                                 kind[p] == G.INS and not deleted[p], kind[p] == G.SNV and not deleted[p])) if yes}
        # at the record's end: a run that reaches it, the same with a merged del just in front of it, an ins and an snv on the last base
        found |= {(f, SPOTS[2]) for f, yes in zip(FEATURES, (deleted[n - 1], deleted[n - 1] and deleted[n - 2] and kind[n - 2] == G.DEL,
                                                             kind[n - 1] == G.INS and not deleted[n - 1], kind[n - 1] == G.SNV and not deleted[n - 1])) if yes}
    return found


def edge_genome(l_ref):
    e0, e1 = harness.synth_bases(l_ref, 100 + l_ref).tobytes(), harness.synth_bases(700, 7).tobytes()
    return [("e0", e0 + b"\n"), ("one", b"G"), ("none", b""), ("e1", b"\n".join(e1[k:k + 50] for k in range(0, 700, 50)))]


@pytest.mark.parametrize("l_ref", [255, 256, 257])
def test_events_at_the_edges_of_tiles_and_records(ctx, l_ref):
    """records of 255, 256 and 257 bases (the last position of e0 is a tile's last but one, its last and the next one's first), of one
    base and of none, and e1 over three tiles; seeds chosen with the model until a del run, a merged pair of runs, an ins and an snv
    have each been at a tile's last position, at a tile's first and at a record's last"""
    genome = edge_genome(l_ref)
    wanted = {(f, s) for f in FEATURES for s in SPOTS}
    seen, seeds = set(), []
    for seed in range(1, 400):
        new = features_of(genome, seed) - seen
        if new:
            seen |= new
            seeds.append(seed)
        if seen == wanted:
            break
    assert seen == wanted and len(seeds) <= 12, (sorted(wanted - seen), seeds)
    for seed in seeds:
        r = check(ctx, genome, seed=seed, line_width=61, **RATES)
        assert r.per_record[1][0] == 1 and r.per_record[2] == (0, 0, 0) and min(r.types) > 20 and r.merged > 10 and r.dropped > 10


# ---------------------------------------------------------------- the line width
@pytest.mark.parametrize("line_width", [1, 59, 60, 61, 0])
def test_line_widths_with_an_insertion_across_a_line_break(ctx, line_width):
    genome = four_records()
    kw = dict(seed=1, snv_ppm=20000, ins_ppm=40000, del_ppm=20000, ext_ppm=800000, max_indel=40, line_width=line_width)
    r = check(ctx, genome, **kw)
    if line_width:                                  # an insertion that begins on one line and ends on a later one
        origin = r.origins[0]
        starts = np.flatnonzero((origin[1:] < 0) & (origin[:-1] >= 0)) + 1
        ends = np.flatnonzero((origin[:-1] < 0) & (origin[1:] >= 0))
        assert any(a // line_width != b // line_width for a, b in zip(starts, ends))
        assert max(len(line) for line in r.fasta.split(b"\n") if not line.startswith(b">")) == line_width
    assert bases_of(r.fasta) == bases_of(G.mutate(genome, **dict(kw, line_width=7)).fasta)


# ---------------------------------------------------------------- the rates at their limits
def test_no_rates_give_the_prepared_genome_and_the_header(ctx):
    genome = four_records()
    r = check(ctx, genome, snv_ppm=0, ins_ppm=0, del_ppm=0, line_width=0)
    prepared = G.prepared_records(genome)
    assert r.fasta == b"".join(b">" + name + b"\n" + (seq.tobytes() + b"\n" if len(seq) else b"") for name, seq in prepared)
    assert r.vcf == G.header([(name, len(seq)) for name, seq in prepared], snv_ppm=0, ins_ppm=0, del_ppm=0) and r.variants == 0
    assert all(np.array_equal(o, np.arange(len(o))) for o in r.origins)


def test_every_position_a_deletion(ctx):
    """del_ppm 1000000 on 1000 bases with two N runs: one record per stretch of A C G T, one lane walking each long group"""
    seq = bytearray(harness.synth_bases(1000, 9).tobytes())
    seq[300:303], seq[650:651] = b"NNN", b"R"
    r = check(ctx, [("d", bytes(seq))], snv_ppm=0, ins_ppm=0, del_ppm=1000000)
    assert [line.split(b"\t")[1] for line in lines_of(r.vcf)] == [b"1", b"304", b"652"] and r.longest_ref == 349
    assert bases_of(r.fasta)[b"d"] == bytes(seq[0:1] + seq[300:304] + seq[650:652]) and r.merged == r.drawn[2] - 3 and r.void_del == 3


def test_the_longest_indels(ctx):
    """ext_ppm 999999 and max_indel 65535 on 2000 bases: insertions of 65535 bases written by one lane each, a deletion to the record's end"""
    genome = [("g", harness.synth_bases(2000, 5).tobytes())]
    r = check(ctx, genome, ins_ppm=2000, del_ppm=0, ext_ppm=999999, max_indel=65535)
    assert r.longest_alt == 65536 and r.inserted > 65535
    r = check(ctx, genome, ins_ppm=2000, del_ppm=2000, ext_ppm=999999, max_indel=65535)
    assert r.variants >= 1 and r.deleted > 1000
    r = check(ctx, genome, ins_ppm=0, del_ppm=2000, ext_ppm=999999, max_indel=65535)
    assert r.variants == 1 and r.longest_ref == r.deleted + 1


# ---------------------------------------------------------------- delivery
def test_pieces_of_seven_bytes(ctx):
    genome = four_records()
    want = check(ctx, genome, piece_bytes=7, snv_ppm=50000, ins_ppm=20000, del_ppm=20000)
    pieces, records = {"fasta": [], "vcf": []}, []

    def on(which):
        def take(user, ptr, n, offset):
            pieces[which].append((offset, C.string_at(ptr, n)))
            return 1
        return take

    def on_record(user, ref, l_ref, l_out, n_variants):
        records.append((ref, l_ref, l_out, n_variants, len(pieces["fasta"]), len(pieces["vcf"])))
        return 1
    sink = P.MutateSink(None, P.MUTATE_TEXT_CB(on("fasta")), P.MUTATE_TEXT_CB(on("vcf")), P.MUTATE_RECORD_CB(on_record), P.MUTATE_ORIGIN_CB())
    opts = P.MutateOpts(1, 50000, 20000, 20000, 500000, 50, 60, 7)
    keep = [(nm.encode(), bytes(lines)) for nm, lines in genome]
    refs = (P.ErrorsRef * len(keep))(*[P.ErrorsRef(nm, C.cast(C.c_char_p(lines), C.c_void_p), len(lines)) for nm, lines in keep])
    res = P.MutateResult()
    assert ctx.lib.pbsim_genome_mutate(ctx.h, refs, len(keep), C.byref(opts), C.byref(sink), C.byref(res)) == 1
    for which, text in (("fasta", want.fasta), ("vcf", want.vcf)):
        at = 0
        for offset, p in pieces[which]:
            assert offset == at and 1 <= len(p) <= 7
            at += len(p)
        assert b"".join(p for _, p in pieces[which]) == text and len(pieces[which]) == -(-len(text) // 7)
    # the records come after both texts
    assert records == [(k, a, b, c, len(pieces["fasta"]), len(pieces["vcf"])) for k, (a, b, c) in enumerate(want.per_record)]
    assert (res.fasta_bytes, res.vcf_bytes) == (len(want.fasta), len(want.vcf))
    # a sink that stops: the call fails, the result is zeroed, the context stays usable
    stop = P.MutateSink(None, P.MUTATE_TEXT_CB(lambda *a: 0), P.MUTATE_TEXT_CB(), P.MUTATE_RECORD_CB(), P.MUTATE_ORIGIN_CB())
    assert ctx.lib.pbsim_genome_mutate(ctx.h, refs, len(keep), C.byref(opts), C.byref(stop), C.byref(res)) == 0
    assert b"sink aborted (text)" in ctx.lib.pbsim_last_error() and res.records == 0 and res.vcf_bytes == 0
    check(ctx, WORKED_GENOME, **WORKED_OPTIONS)


# ---------------------------------------------------------------- the records' order
def test_two_records_in_both_orders(ctx):
    """a record's draws depend on its index alone: in the other order every record is what the model gives it under the swapped index"""
    a, b = ("a", harness.synth_bases(900, 21).tobytes()), ("b", b"acgtn" * 100 + harness.synth_bases(300, 22).tobytes())
    kw = dict(snv_ppm=50000, ins_ppm=30000, del_ppm=30000, line_width=0)
    ab, ba = check(ctx, [a, b], **kw), check(ctx, [b, a], **kw)
    swapped = G.mutate([a, b], indices=[1, 0], **kw)
    assert bases_of(ba.fasta) == bases_of(swapped.fasta) != bases_of(ab.fasta) and sorted(lines_of(ba.vcf)) == sorted(lines_of(swapped.vcf))
    assert ba.per_record == swapped.per_record[::-1]
    with pytest.raises(P.PbsimError, match="pbsim_genome_mutate: the genome holds two records named \"a\""):
        ctx.mutate_genome([a, b, a])
    for bad, word in REFUSED_OPTS[:3]:
        with pytest.raises(P.PbsimError, match="pbsim_genome_mutate: " + word):
            ctx.mutate_genome([a, b], **bad)
    check(ctx, [a, b], want=ab, **kw)


# ---------------------------------------------------------------- back through the call stage
@pytest.mark.parametrize("kw", [dict(), dict(snv_ppm=300000, ins_ppm=300000, del_ppm=300000)], ids=["defaults", "high rates"])
def test_reads_that_spell_the_variant_genome_are_called_as_the_truth(ctx, kw):
    genome = four_records()
    result, _, fasta, vcf, _, origins = ctx.mutate_genome(genome, origin=True, line_width=0, **kw)
    stream, _ = spelling_reads(genome, fasta, origins)
    called = ctx.bam_call(B.contain(stream), genome, max_ins=65535)
    assert first_five(called[2]) == first_five(vcf) and called[0]["variants"] == result["variants"] > 0
    assert [called[0]["types"][t] for t in ("snv", "ins", "del", "complex")] == [result["types"][t] for t in G.TYPE_NAMES] + [0]


# ---------------------------------------------------------------- through the command line
def test_cli_writes_the_apis_bytes_from_a_bgzf_fasta(ctx, tmp_path):
    genome = [(n, lines) for n, lines in four_records(12) if len(lines) > 100]      # (the command line's loader takes records of 100 bases or more)
    text = b"".join(b">" + n.encode() + b" a description\n" + lines + (b"" if lines.endswith(b"\n") or not lines else b"\n") for n, lines in genome)
    (tmp_path / "genome.fa.gz").write_bytes(W.bgzf(text, block=700))
    kw = dict(seed=77, snv_ppm=40000, ins_ppm=20000, del_ppm=20000, ext_ppm=700000, max_indel=12, line_width=50)
    api = ctx.mutate_genome(genome, **kw)
    cmd = [CLI, "--mutate-genome", "genome.fa.gz", "--mutate-out", "out.fa", "--mutate-vcf", "out.vcf"]
    cmd += [x for name, v in kw.items() for x in ("--mutate-" + name.replace("_", "-"), str(v))]
    r = subprocess.run(cmd, capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert (tmp_path / "out.fa").read_bytes() == api[2] and (tmp_path / "out.vcf").read_bytes() == api[3] and r.stdout == api[1]
    want = G.mutate(genome, **kw)
    assert (api[2], api[3], api[1]) == (want.fasta, want.vcf, want.report) and want.variants > 50
    # the defaults, from the plain file; a failure leaves no file behind
    (tmp_path / "genome.fa").write_bytes(text)
    r = subprocess.run([CLI, "--mutate-genome", "genome.fa", "--mutate-out", "d.fa", "--mutate-vcf", "d.vcf"], capture_output=True, cwd=str(tmp_path), timeout=300)
    want = G.mutate(genome)
    assert r.returncode == 0 and (tmp_path / "d.fa").read_bytes() == want.fasta and (tmp_path / "d.vcf").read_bytes() == want.vcf and r.stdout == want.report
    (tmp_path / "twice.fa").write_bytes(text + b">a again\n" + genome[0][1])
    r = subprocess.run([CLI, "--mutate-genome", "twice.fa", "--mutate-out", "t.fa", "--mutate-vcf", "t.vcf"], capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode != 0 and b"the genome holds two records named \"a\"" in r.stderr and not (tmp_path / "t.fa").exists() and not (tmp_path / "t.vcf").exists()
