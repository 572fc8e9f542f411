"""`pbsim --pileup-bam` (pbsim_bam_pileup) on the device, held to tests/pileup_model.py byte for byte: counts, site totals, cell sums,
the per-class arrays, the report, the text in both formats and the cells themselves, with the text and without it."""
import ctypes as C
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bam_writer as B
import harness
import pbsim3_amd as P
import pileup_model as M
from test_gpu_bam_errors import CHR, GEN, OTHER, REFS, SEG_COLS, SEG_OPS, SEQS, aligned, fasta_lines, noisy_ops, planted
from test_pileup_model import GENOME, WORKED, WORKED_ALL_TEXT, WORKED_CELLS, WORKED_OPTIONS, WORKED_REFS, WORKED_REPORT, WORKED_SITES_TEXT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


def compare(got, want):
    result, report = got[0], got[1]
    assert [result["counts"][n] for n in M.COUNT_NAMES] == want.counts
    assert [result["sites"][n] for n in M.SITE_NAMES] == want.sites
    assert [result["cell_sums"][n] for n in M.CELL_NAMES] == want.cell_sums
    assert (result["ins_unanchored"], result["max_depth"]) == (want.ins_unanchored, want.max_depth)
    for name in M.HP_ARRAYS:
        assert result[name] == getattr(want, name), name
    assert report == want.report


def check(ctx, streams, genome=GEN, container="bgzf", block=B.W.BGZIP_BLOCK, piece_bytes=0, fmts=M.FORMATS, wants=None, **kw):
    """inflated streams -> through the product in `container`, every output against the model: per format with the text and the
    cells, and once without either; returns the model's result of the first format"""
    if isinstance(streams, (bytes, bytearray)):
        streams = [streams]
    kw.pop("fmt", None)
    wants = wants or dict(zip(M.FORMATS, M.pileup(streams, genome, fmt="both", **kw)))
    files = [B.contain(s, container, block) for s in streams]
    for fmt in fmts:
        want = wants[fmt]
        got = ctx.bam_pileup(files, genome, text=True, arrays=True, fmt=fmt, piece_bytes=piece_bytes, **kw)
        compare(got, want)
        assert got[2] == want.text
        assert len(got[3]) == len(want.cells)
        for mine, theirs in zip(got[3], want.cells):
            assert tuple(mine.shape) == theirs.shape and str(mine.dtype) == "torch.uint32" and np.array_equal(mine.numpy(), theirs)
    bare = ctx.bam_pileup(files, genome, **kw)
    assert len(bare) == 2
    compare(bare, wants[fmts[0]])
    return wants[fmts[0]]


# ---------------------------------------------------------------- the worked case and the options
def test_the_worked_case(ctx):
    stream = B.stream(WORKED, WORKED_REFS)
    r = check(ctx, stream, GENOME)
    assert r.report == WORKED_REPORT and r.text == WORKED_SITES_TEXT and [c.tolist() for c in r.cells] == WORKED_CELLS
    got = ctx.bam_pileup(B.bam(WORKED, WORKED_REFS), GENOME, text=True, fmt="all")
    assert got[2] == WORKED_ALL_TEXT and got[1] == WORKED_REPORT
    assert check(ctx, [B.stream(WORKED[9:], WORKED_REFS), B.stream(WORKED[:9], WORKED_REFS)], GENOME).text == WORKED_SITES_TEXT


@pytest.mark.parametrize("kw", WORKED_OPTIONS, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_the_worked_case_with_an_option_moved(ctx, kw):
    moved = check(ctx, B.stream(WORKED, WORKED_REFS), GENOME, **kw)
    plain = M.pileup(B.stream(WORKED, WORKED_REFS), GENOME)
    assert (moved.counts, moved.sites, moved.cell_sums, moved.text) != (plain.counts, plain.sites, plain.cell_sums, plain.text) or kw == dict(fmt="all")


def test_no_records_and_only_skipped_records(ctx):
    r = check(ctx, B.stream([], WORKED_REFS), GENOME)
    assert r.counts == [0] * 9 and r.sites == [23, 1, 22, 0, 0, 0, 0, 0, 0] and r.text == b""
    r = check(ctx, B.stream([w for w in WORKED if w["name"] in ("u1", "s1", "m1", "z1")], WORKED_REFS), GENOME)
    assert r.counts == [4, 1, 1, 0, 1, 1, 0, 1, 0] and r.max_depth == 0


# ---------------------------------------------------------------- segment cuts
def test_cuts_inside_ops_and_insertions_at_the_cuts(ctx):
    """one record of more than SEG_OPS ops and more than SEG_COLS columns: a cut inside an M op and one inside a D op, an I op that
    is the first column of a segment inside a block, a block of SEG_OPS ops that ends on an I, and the next block beginning with one"""
    assert SEG_COLS >= 1000 and SEG_OPS >= 8
    ops = [(SEG_COLS + 900, "M"), (SEG_COLS - 100, "D")]                    # cuts at SEG_COLS (in M) and at 2 SEG_COLS (in D)
    ops += [(3 * SEG_COLS - sum(n for n, _ in ops), "M"), (2, "I")]         # the I op begins at column 3 SEG_COLS
    ops += [(3, "M"), (1, "I")] * ((SEG_OPS - len(ops)) // 2)               # .. and op SEG_OPS - 1 is an I
    assert len(ops) == SEG_OPS and ops[-1][1] == "I"
    ops += [(2, "I"), (7, "M"), (1, "D"), (2, "M"), (1, "I"), (5, "M")]     # the next block begins with an I
    rng = random.Random(5)
    for pos in (0, 77):
        r = check(ctx, B.stream([aligned("long", ops, pos=pos, rng=rng)], REFS), fmts=("sites",))
        assert r.counts[8] == 1 and r.cell_sums[6] == SEG_OPS // 2 + 1 and r.ins_unanchored == 0 and r.cell_sums[5] == SEG_COLS - 99
    lead = [(1, "I")] + ops                                                 # shifted by one op, and the first insertion has no anchor
    r = check(ctx, B.stream([aligned("lead", lead, pos=3, rng=rng, placeholder=True)], REFS), fmts=("sites",))
    assert r.ins_unanchored == 1 and r.cell_sums[6] == SEG_OPS // 2 + 1


@pytest.mark.parametrize("n_ops", [64, 65, SEG_OPS, SEG_OPS + 1])
def test_op_counts_around_a_round_and_a_block(ctx, n_ops):
    rng = random.Random(n_ops)
    recs = [aligned("r%d" % k, noisy_ops(rng, n_ops), pos=50 * k, rng=rng, placeholder=k == 2) for k in range(3)]
    recs.append(aligned("ends_on_i", noisy_ops(rng, n_ops - 2) + [(1, "I"), (2, "S")], pos=10, rng=rng))
    r = check(ctx, B.stream(recs, REFS), fmts=("sites",))
    assert r.counts[8] == 4 and r.cell_sums[6] > n_ops // 4


# ---------------------------------------------------------------- contention
def test_three_thousand_records_on_the_same_hundred_positions(ctx):
    rng = random.Random(6)
    gen = [("hot", fasta_lines(CHR[:300]))]
    recs = [aligned("h%d" % k, [(100, "M")] if k % 3 else [(50, "M"), (1, "I"), (1, "D"), (49, "M")], pos=100, rng=rng, qual="none") for k in range(3000)]
    recs += [aligned("one%d" % k, [(1, "M")], pos=220 + k, rng=rng, keep=1.0, qual="none") for k in range(64)]
    r = check(ctx, B.stream(recs, [("hot", 300)]), gen)
    assert r.max_depth == 3000 and r.cells[0][100:200, :6].sum(axis=1).tolist() == [3000] * 100 and r.cells[0][149, 6] == 1000
    assert r.cells[0][220:284, :4].sum(axis=1).tolist() == [1] * 64 and r.sites[2] == 300 - 164


# ---------------------------------------------------------------- the edges of the table
@pytest.mark.parametrize("l_ref", [63, 64, 65])
def test_edges_of_the_table(ctx, l_ref):
    """records at pos 0, ending at l_ref, on the last base of a genome record with the next one behind it; genome records of one base
    and of none"""
    rng = random.Random(l_ref)
    e0, e1 = planted(rng, 200)[:l_ref], planted(rng, 200)[:130]
    gen = [("e0", e0 + b"\n"), ("one", b"G\n"), ("none", b""), ("e1", fasta_lines(e1, 50))]
    refs = [("e0", l_ref), ("one", 1), ("e1", 130)]              # (the genome's record of no bases is no reference of the file)
    seqs = {0: e0, 1: b"G", 2: e1}
    recs = [aligned("first", [(4, "M")], pos=0, rng=rng, seqs=seqs), aligned("whole", [(l_ref, "M")], pos=0, rng=rng, seqs=seqs),
            aligned("end", [(3, "M"), (2, "D"), (2, "M")], pos=l_ref - 7, rng=rng, seqs=seqs),
            aligned("last", [(1, "M"), (1, "I")], pos=l_ref - 1, rng=rng, seqs=seqs),
            aligned("last_d", [(2, "S"), (1, "D")], pos=l_ref - 1, rng=rng, seqs=seqs),
            aligned("past", [(2, "M")], pos=l_ref - 1, rng=rng, seqs=seqs),                                  # misfit
            aligned("g", [(1, "M")], pos=0, ref=1, rng=rng, seqs=seqs), aligned("gi", [(1, "M"), (3, "I")], pos=0, ref=1, rng=rng, seqs=seqs),
            aligned("ig", [(1, "I"), (1, "M")], pos=0, ref=1, rng=rng, seqs=seqs),
            aligned("next", [(1, "I"), (5, "M")], pos=0, ref=2, rng=rng, seqs=seqs), aligned("tail", [(6, "M")], pos=124, ref=2, rng=rng, seqs=seqs)]
    r = check(ctx, B.stream(recs, refs), gen)
    assert r.counts[7] == 1 and r.counts[8] == 10 and [len(c) for c in r.cells] == [l_ref, 1, 0, 130]
    assert r.cells[0][l_ref - 1].tolist()[5:7] == [1, 1] and r.cells[0][l_ref - 1, :4].sum() == 3 and r.cells[1][0].tolist()[6] == 1
    assert r.cells[3][0, 6] == 0 and r.cells[3][0, :4].sum() == 1 and r.ins_unanchored == 2 and r.sites[0] == l_ref + 131
    # the same with the genome's records in another order: the padding lies elsewhere
    assert check(ctx, B.stream(recs, refs), gen[::-1]).sites == r.sites


# ---------------------------------------------------------------- references and files
def test_references_by_name(ctx):
    rng = random.Random(13)
    one = [B.stream([aligned("a%d" % k, noisy_ops(rng, 20), pos=rng.randrange(5000), ref=0, rng=rng, seqs={0: SEQS[f]}) for k in range(50)],
                    [("ref", len(SEQS[f]))]) for f in (0, 1)]
    r = check(ctx, one, ref_names=["chr", "other"], fmts=("sites",))
    assert r.counts[8] == 100
    assert check(ctx, one, ref_names=["chr", None], fmts=("sites",)).counts[4] == 50        # "ref" is no record of the genome
    swapped = B.stream([aligned("b%d" % k, noisy_ops(rng, 20), pos=rng.randrange(5000), ref=k % 3, rng=rng, seqs={0: OTHER, 1: CHR, 2: CHR})
                        for k in range(60)], [("other", len(OTHER)), ("chr", len(CHR)), ("unknown", len(CHR))])
    r = check(ctx, swapped, fmts=("sites",))
    assert r.counts[4] == 20 and r.counts[8] == 40
    assert check(ctx, swapped, genome=GEN[::-1], fmts=("sites",)).report == r.report


def test_failures_say_why_and_leave_the_context_usable(ctx):
    def usable():
        assert check(ctx, B.stream(WORKED, WORKED_REFS), GENOME, fmts=("sites",)).report == WORKED_REPORT

    data = B.bam(WORKED, WORKED_REFS)
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_pileup: the reference \"g1\" has l_ref 16 in the file's header, and the genome's record of that "
                                           r"name has 15 bases"):
        ctx.bam_pileup(B.bam(WORKED, [("g1", 16), ("g2", 8), ("zz", 50)]), GENOME)
    usable()
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_pileup: file 1: the reference \"big\" has l_ref 15 .* has 51 bases"):
        ctx.bam_pileup([data, B.bam(WORKED[:1], [("ref", 15)])], GENOME + [("big", b"A" * 51)], ref_names=[None, "big"])
    usable()
    with pytest.raises(P.PbsimError, match="pbsim_bam_pileup: file 0 has 3 references: a reference name can be given only to a file with exactly one"):
        ctx.bam_pileup(data, GENOME, ref_names=["g1"])
    usable()
    good = [aligned("g%d" % k, [(5, "M"), (2, "D"), (5, "M")], pos=k) for k in range(50)]
    head = B.stream(good, REFS)
    bad_op = B.record_bytes(B.record("b", 0, 0, 1, cigar=[(2, "M")], seq="AC", qual=b"\x05\x05"))
    cig_at = 4 + 32 + 2
    bad_op = bad_op[:cig_at] + struct.pack("<I", 2 << 4 | 9) + bad_op[cig_at + 4:]
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_pileup: the record at inflated byte offset %d is malformed" % len(head)):
        ctx.bam_pileup(B.contain(head + bad_op + B.record_bytes(good[0]), "bgzf"), GEN, text=True, arrays=True)
    usable()
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_pileup: file 1: the record at inflated byte offset %d is malformed" % len(head)):
        ctx.bam_pileup([B.contain(head), B.contain(head + bad_op, "none")], GEN, text=True)
    usable()
    with pytest.raises(P.PbsimError, match="pbsim_bam_pileup: neither BGZF, gzip nor an uncompressed BAM"):
        ctx.bam_pileup(b"@HD\tVN:1.6\n", GEN)
    usable()


# ---------------------------------------------------------------- the text's delivery
def deliver(ctx, datas, genome, piece_bytes, fmt=0, stop_after=None):
    pieces = []

    def on_text(user, ptr, n, offset):
        pieces.append((offset, C.string_at(ptr, n)))
        return 0 if stop_after is not None and len(pieces) >= stop_after else 1
    sink = P.PileupSink(None, P.PILEUP_TEXT_CB(on_text), P.PILEUP_CELLS_CB())
    opts = P.PileupOpts(0x900, 0, 0, fmt, 1, piece_bytes)
    keep = [(nm.encode(), bytes(lines)) for nm, lines in genome]
    refs = (P.ErrorsRef * len(keep))(*[P.ErrorsRef(nm, C.cast(C.c_char_p(lines), C.c_void_p), len(lines)) for nm, lines in keep])
    arr = (P.ErrorsFile * len(datas))(*[P.ErrorsFile(C.cast(C.c_char_p(d), C.c_void_p), len(d), None) for d in datas])
    res = P.PileupResult()
    ok = ctx.lib.pbsim_bam_pileup(ctx.h, refs, len(keep), arr, len(datas), C.byref(opts), C.byref(sink), C.byref(res))
    return ok, pieces, res


def test_delivery_in_pieces_and_every_container(ctx):
    rng = random.Random(14)
    gen = [("d0", fasta_lines(CHR[:700])), ("d1", fasta_lines(OTHER[-300:], 31))]
    refs, seqs = [("d0", 700), ("d1", 300)], {0: CHR[:700], 1: OTHER[-300:]}
    streams = [B.stream([aligned("q%d" % (100 * f + k), noisy_ops(rng, 30), pos=rng.randrange(500 if k % 2 == 0 else 150), ref=k % 2, rng=rng, seqs=seqs)
                         for k in range(40)], refs) for f in range(2)]
    sites, every = M.pileup(streams, gen, fmt="both")
    assert 300 < len(sites.text) and 8192 < len(every.text)
    datas = [B.contain(s) for s in streams]
    for fmt, want in ((0, sites.text), (1, every.text)):
        for piece in (0, 1, 7, 4096) if fmt == 0 else (7, 4096):
            ok, pieces, _ = deliver(ctx, datas, gen, piece, fmt)
            assert ok == 1 and b"".join(p for _, p in pieces) == want
            at = 0
            for offset, p in pieces:
                assert offset == at and 1 <= len(p) <= (piece or len(want))
                at += len(p)
            assert piece != 7 or any(not p.endswith(b"\n") for _, p in pieces)                # a piece ends inside a line
    ok, pieces, res = deliver(ctx, datas, gen, 7, stop_after=3)
    assert ok == 0 and len(pieces) == 3 and b"sink aborted (text)" in ctx.lib.pbsim_last_error() and sum(res.counts) == 0
    for container in ("bgzf", "stored", "gzip", "none"):
        check(ctx, streams, gen, container=container, block=1024, piece_bytes=7)
    # a call whose sites text is empty: reads that say what the genome says
    clean = B.stream([aligned("c%d" % k, [(40, "M")], pos=10 * k, rng=rng, keep=1.0, seqs=seqs) for k in range(30)], refs)
    r = check(ctx, clean, gen)
    assert r.text == b"" and r.sites[8] == 0 and r.sites[3] > 300
    ok, pieces, _ = deliver(ctx, [B.contain(clean)], gen, 7)
    assert ok == 1 and pieces == []


# ---------------------------------------------------------------- order
def random_records(rng, n, qual):
    out = []
    for k in range(n):
        kind = k % 23
        flag = [0, 16, 0x800, 0x100, 0x400, 4, 0x200][kind % 7 if kind < 14 else 0]
        ref = rng.randrange(2)
        ops = noisy_ops(rng, rng.choice([1, 2, 3, 5, 8, 30, 63, 64, 65, 66, 150]))
        if kind in (3, 15):
            ops = [(rng.randrange(3), "S"), (1, "I")] + ops
        q = qual if qual != "mixed" else ("none" if k % 3 == 0 else "random")
        rec = aligned("q%d" % k, ops, pos=rng.randrange(len(SEQS[ref]) - 2000), ref=ref, rng=rng, flag=flag, mapq=rng.randrange(60),
                      placeholder=kind in (20, 21), qual=q)
        if kind == 22:
            rec = B.record("u%d" % k, 4 if k % 2 else 0, -1, -1, seq="ACGT", qual=b"\x05" * 4)
        out.append(rec)
    return out


@pytest.mark.parametrize("qual", ["random", "none", "mixed"])
def test_two_thousand_records_in_any_order(ctx, qual):
    rng = random.Random(len(qual))
    recs = random_records(rng, 2000, qual)
    kw = dict(min_baseq=25, min_mapq=5) if qual != "none" else dict()
    wants = dict(zip(M.FORMATS, M.pileup(B.stream(recs, REFS), GEN, fmt="both", **kw)))
    r = check(ctx, B.stream(recs, REFS), fmts=("all",) if qual == "mixed" else ("sites",), wants=wants, **kw)
    assert r.counts[8] > 1000 and r.ins_unanchored > 50 and (r.cell_sums[7] > 1000) == (qual != "none") and r.sites[8] > 1000
    # the same records shuffled and split over three files, in either order of the files
    mixed = list(recs)
    rng.shuffle(mixed)
    files = [B.contain(B.stream(part, REFS), "bgzf", 1024) for part in (mixed[:300], mixed[300:1700], mixed[1700:])]
    for order in (files, files[::-1]):
        got = ctx.bam_pileup(order, GEN, text=True, arrays=True, **kw)
        compare(got, r)
        assert got[2] == wants["sites"].text and all(np.array_equal(a.numpy(), b) for a, b in zip(got[3], r.cells))


# ---------------------------------------------------------------- planted variants
# with this seed the model lists the six planted sites and two more: worked out with tests/pileup_model.py on the CPU
VARIANT_SEED, VARIANT_OTHER_SITES = 2026, 2


def planted_variants():
    """a genome of 20 kb; reads of 600 bases at depth 40 written from a copy of it with three substitutions, a deletion of two bases
    and an insertion of one, with their true CIGARs against the unaltered genome; keep 0.9"""
    rng = random.Random(VARIANT_SEED)
    ref = planted(rng, 20_000, longest=6)
    subs = {3000: None, 9001: None, 15500: None}
    alt = bytearray(ref)
    for p in subs:
        subs[p] = alt[p] = rng.choice([c for c in b"ACGT" if c != ref[p]])
    dele, ins_after = (6000, 6001), 12000                       # the inserted base follows position 12000
    recs = []
    for k in range(40 * len(ref) // 600):
        pos = rng.randrange(len(ref) - 600)
        if pos in (dele[0], dele[1], ins_after + 1):
            pos += 3                                            # (no read begins inside the deletion or on the insertion)
        end, ops, at = pos + 600, [], pos
        for cut, op in sorted([(dele[0], (2, "D")), (ins_after + 1, (1, "I"))]):
            if at < cut < end:
                if op[1] == "D" and cut + 2 >= end:
                    end = cut                                   # (the read ends in front of the deletion)
                    break
                ops += [(cut - at, "M"), op]
                at = cut + (2 if op[1] == "D" else 0)
        ops.append((end - at, "M"))
        recs.append(aligned("v%d" % k, ops, pos=pos, rng=rng, keep=0.9, seqs={0: bytes(alt)}))
    return ref, subs, dele, ins_after, recs


def test_planted_variants_are_listed_with_their_calls(ctx):
    ref, subs, dele, ins_after, recs = planted_variants()
    gen = [("v", fasta_lines(ref))]
    r = check(ctx, B.stream(recs, [("v", len(ref))]), gen, fmts=("sites",))
    lines = {int(f[1]) - 1: f for f in (ln.split(b"\t") for ln in r.text.splitlines())}
    for p, base in subs.items():
        assert lines[p][12] == bytes([base]) and lines[p][13] == b"sub" and lines[p][2] == ref[p:p + 1]
    for p in dele:
        assert lines[p][12] == b"*" and lines[p][13] == b"del"
    assert lines[ins_after][13] == b"match+ins" and int(lines[ins_after][10]) * 2 > int(lines[ins_after][3])
    assert min(int(lines[p][3]) for p in list(subs) + list(dele) + [ins_after]) >= 20 and r.sites[2] < 200
    print("planted variants: %d discordant sites, %d beside the planted six" % (r.sites[8], r.sites[8] - 6))
    assert r.sites[8] - 6 == VARIANT_OTHER_SITES


# ---------------------------------------------------------------- the product's own files, through the command line
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def _run(cmd, workdir):
    r = subprocess.run(cmd, capture_output=True, cwd=workdir, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return r


@pytest.mark.parametrize("method", ["errhmm", "qshmm"])
def test_cli_on_the_products_own_truth_files(tmp_path, method):
    """the pileup of the simulator's own truth files against the genome they were made from: every record scored, the sums those of
    --errors-bam and --depth-bam on the same files, and the sorted files give the same bytes as the unsorted"""
    from test_gpu_bam_errors import product_genome, simulate
    fasta = str(tmp_path / "genome.fa")
    genome = product_genome(fasta, 23, 100_000)
    _, alns, _ = simulate(str(tmp_path / "u"), fasta, method, 7, depth="6")
    assert len(alns) == 2
    names = ["--pileup-genome", fasta, "--pileup-ref-names", "chrA,chrB"]
    out = str(tmp_path / "sites.tsv")
    r = _run([CLI] + [x for aln in alns for x in ("--pileup-bam", aln)] + names + ["--pileup-out", out], str(tmp_path))
    streams = []
    for aln in alns:
        with open(aln, "rb") as f:
            streams.append(M.inflate(f.read()))
    want = M.pileup(streams, genome, ref_names=["chrA", "chrB"])
    with open(out, "rb") as f:
        text = f.read()
    assert r.stdout == want.report and text == want.text
    counts, sites = dict(zip(M.COUNT_NAMES, want.counts)), dict(zip(M.SITE_NAMES, want.sites))
    print(method, counts, sites, want.cell_sums, want.ins_unanchored, want.max_depth)
    assert counts["scored"] == counts["aligned"] == counts["records"] > 20
    assert sites["called"] + sites["low"] + sites["ref_n"] == sites["sites"] == sum(len(c) for c in want.cells) and sites["called"] > 150_000
    e = _run([CLI] + [x for aln in alns for x in ("--errors-bam", aln)] + ["--errors-genome", fasta, "--errors-ref-names", "chrA,chrB"], str(tmp_path))
    totals = [int(v) for v in re.search(rb"^E\t(.*)$", e.stdout, re.M).group(1).split(b"\t")]
    assert sum(want.cell_sums[:5]) == totals[1] + totals[2] + totals[3] and want.cell_sums[5] == totals[5] and want.cell_sums[7] == 0
    assert want.cell_sums[6] + want.ins_unanchored == totals[6]
    depth_sum = 0
    for k, aln in enumerate(alns):
        d = _run([CLI, "--depth-bam", aln, "--depth-out", str(tmp_path / ("d%d.bg" % k))], str(tmp_path))
        depth_sum += sum(int(ln.split(b"\t")[4]) for ln in d.stdout.splitlines() if ln.startswith(b"R\t"))
    assert depth_sum == sum(want.cell_sums[:6])
    # the sorted truth files give the same bytes
    copies = []
    for k, aln in enumerate(alns):
        copies.append(str(tmp_path / ("sorted%d.aln.bam" % k)))
        shutil.copy(aln, copies[-1])
    _run([CLI, "--sort-truth-bam"] + copies, str(tmp_path))
    out2 = str(tmp_path / "sites2.tsv")
    r2 = _run([CLI] + [x for c in copies for x in ("--pileup-bam", c)] + names + ["--pileup-out", out2, "--pileup-format", "sites"], str(tmp_path))
    with open(out2, "rb") as f:
        assert f.read() == text and r2.stdout == r.stdout
