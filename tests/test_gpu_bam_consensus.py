"""`pbsim --consensus-bam` (pbsim_bam_consensus) on the device, held to tests/consensus_model.py byte for byte: counts, site totals,
the base counts, the insertion lengths, the report, the FASTA and the per-record lengths, with the text and without it."""
import ctypes as C
import os
import random
import shutil
import struct
import subprocess

import pytest

import bam_writer as B
import consensus_model as K
import harness
import pbsim3_amd as P
from test_consensus_model import (GENOME, REFS as WORKED_REFS, REFUSED_OPTS, WORKED, WORKED_FASTA, WORKED_FASTA_REF, WORKED_OPTIONS, WORKED_REPORT)
from test_gpu_bam_errors import CHR, GEN, OTHER, REFS, SEG_COLS, SEG_OPS, SEQS, aligned, fasta_lines, noisy_ops, planted
from test_pileup_model import GENOME as PILE_GENOME, WORKED as PILE_WORKED, WORKED_REFS as PILE_REFS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


def compare(got, want):
    result, report = got[0], got[1]
    assert [result["counts"][n] for n in K.COUNT_NAMES] == want.counts
    assert [result["sites"][n] for n in K.SITE_NAMES] == want.sites
    assert (result["ins_unanchored"], result["max_depth"]) == (want.ins_unanchored, want.max_depth)
    assert [result["bases"][n] for n in K.BASE_NAMES] == want.bases
    assert (result["ins_sites"], result["ins_longest"], result["ins_capped"]) == (want.ins_sites, want.ins_longest, want.ins_capped)
    assert result["ins_len"] == want.ins_len and result["text_bytes"] == want.text_bytes
    assert report == want.report


def check(ctx, streams, genome=GEN, container="bgzf", block=B.W.BGZIP_BLOCK, piece_bytes=0, want=None, **kw):
    """inflated streams -> through the product in `container`, every output against the model, with the text and without it;
    returns the model's result"""
    if isinstance(streams, (bytes, bytearray)):
        streams = [streams]
    want = want or K.consensus(streams, genome, **kw)
    files = [B.contain(s, container, block) for s in streams]
    got = ctx.bam_consensus(files, genome, piece_bytes=piece_bytes, **kw)
    compare(got, want)
    assert got[2] == want.text and got[3] == want.lengths
    bare = ctx.bam_consensus(files, genome, text=False, **kw)
    assert len(bare) == 2
    compare(bare, want)
    return want


def exact(name, seq, pos, ops, ref=0):
    """a record without qualities that says `seq`"""
    return B.record(name, 0, ref, pos, cigar=ops, seq=seq, qual=b"\xff" * len(seq), mapq=60)


# ---------------------------------------------------------------- the worked case and the options
def test_the_worked_case(ctx):
    r = check(ctx, B.stream(WORKED, WORKED_REFS), GENOME)
    assert r.text == WORKED_FASTA and r.report == WORKED_REPORT
    got = ctx.bam_consensus(B.bam(WORKED, WORKED_REFS), GENOME, fill="ref")
    assert got[2] == WORKED_FASTA_REF and got[1] == WORKED_REPORT and got[3] == [(10, 13), (5, 5)]
    assert check(ctx, [B.stream(WORKED[3:], WORKED_REFS), B.stream(WORKED[:3], WORKED_REFS)], GENOME).text == WORKED_FASTA
    # the pileup's worked case: skipped and misfit records, qualities that mask, two I ops at one anchor
    assert check(ctx, B.stream(PILE_WORKED, PILE_REFS), PILE_GENOME).text == b">g1\nACGTCCGTTTCNACGT\n>g2\nGGCNNTAC\n"
    check(ctx, B.stream(PILE_WORKED, PILE_REFS), PILE_GENOME, min_baseq=21, min_depth=2, fill="ref")


@pytest.mark.parametrize("kw", WORKED_OPTIONS, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_the_worked_case_with_an_option_moved(ctx, kw):
    moved = check(ctx, B.stream(WORKED, WORKED_REFS), GENOME, **kw)
    plain = K.consensus(B.stream(WORKED, WORKED_REFS), GENOME)
    same = kw in (dict(line_width=0), dict(line_width=13), dict(exclude_flags=0), dict(min_baseq=1))    # (one line either way; no flags, no qualities)
    assert (moved != plain) != same


def test_no_records_and_only_skipped_records(ctx):
    r = check(ctx, B.stream([], WORKED_REFS), GENOME)
    assert r.counts == [0] * 9 and r.text == b">c1\nNNNNNNNNNN\n>c2\nNNNNN\n" and r.bases == [15, 0, 0, 0, 15, 0]
    assert check(ctx, B.stream([], WORKED_REFS), GENOME, fill="ref", min_depth=0).text == b">c1\nACGTACGTAC\n>c2\nGGRTT\n"
    r = check(ctx, B.stream([w for w in PILE_WORKED if w["name"] in ("u1", "s1", "m1", "z1")], PILE_REFS), PILE_GENOME)
    assert r.counts == [4, 1, 1, 0, 1, 1, 0, 1, 0] and r.max_depth == 0


# ---------------------------------------------------------------- line wrapping
@pytest.mark.parametrize("width", [7, 0, 1, 60])
def test_line_wrapping(ctx, width):
    """records whose consensus has width - 1, width, width + 1, 0 and 1 bases (w = 7), one of them through an insertion, one
    through a deletion"""
    rng = random.Random(7)
    seqs = {0: planted(rng, 30)[:6], 1: planted(rng, 30)[:7], 2: planted(rng, 30)[:8], 3: b"A", 4: b"G", 5: planted(rng, 30)[:5]}
    gen = [("w6", seqs[0] + b"\n"), ("w7", seqs[1] + b"\n"), ("w8", seqs[2][:3] + b"\n" + seqs[2][3:] + b"\n"), ("none", b""), ("gone", b"A\n"),
           ("one", b"G\n"), ("w5", seqs[5] + b"\n")]
    refs = [("w6", 6), ("w7", 7), ("w8", 8), ("gone", 1), ("one", 1), ("w5", 5)]
    recs = [aligned("a%d" % k, [(len(seqs[k]), "M")], ref=k, rng=rng, keep=1.0, seqs=seqs, qual="none") for k in (0, 1, 2, 4)]
    recs.append(exact("d", "AC", 0, [(2, "S"), (1, "D")], ref=3))                                    # the only site is deleted
    recs.append(exact("i", seqs[5][:3].decode() + "TT" + seqs[5][3:].decode(), 0, [(3, "M"), (2, "I"), (2, "M")], ref=5))   # 5 + 2 = 7 bases
    r = check(ctx, B.stream(recs, refs), gen, line_width=width)
    assert r.lengths == [(6, 6), (7, 7), (8, 8), (0, 0), (1, 0), (1, 1), (5, 7)] and b">none\n>gone\n>one\nG\n>w5\n" in r.text
    if width == 7:
        assert r.text.startswith(b">w6\n" + seqs[0] + b"\n>w7\n" + seqs[1] + b"\n>w8\n" + seqs[2][:7] + b"\n" + seqs[2][7:] + b"\n>none\n")


# ---------------------------------------------------------------- tiles
@pytest.mark.parametrize("l_ref", [255, 256, 257])
def test_tiles_and_the_records_places(ctx, l_ref):
    """an insertion on the last position of a tile and on the last position of the record; several genome records behind it, one of
    one base and one of none: the 64-aligned places and the padding"""
    rng = random.Random(l_ref)
    e0, e1 = planted(rng, 400)[:l_ref], planted(rng, 200)[:130]
    gen = [("e0", fasta_lines(e0)), ("one", b"G\n"), ("none", b""), ("e1", fasta_lines(e1, 50))]
    refs = [("e0", l_ref), ("one", 1), ("e1", 130)]
    seqs = {0: e0, 1: b"G", 2: e1}
    ops = [(l_ref, "M"), (2, "I")] if l_ref < 257 else [(256, "M"), (3, "I"), (1, "M"), (2, "I")]
    recs = [aligned("whole", ops, pos=0, rng=random.Random(1), seqs=seqs, keep=1.0, qual="none")] * 3
    recs += [aligned("tile", [(2, "M"), (1, "I"), (2, "M")], pos=254 - 1, rng=random.Random(2), seqs=seqs, keep=1.0, qual="none")] * (l_ref >= 257)
    recs += [aligned("gi", [(1, "M"), (3, "I")], pos=0, ref=1, rng=random.Random(3), seqs=seqs, qual="none")] * 2
    recs += [aligned("next", [(1, "I"), (5, "M"), (1, "I"), (3, "M")], pos=0, ref=2, rng=random.Random(4), seqs=seqs, qual="none")] * 2
    recs += [aligned("tail", [(6, "M"), (4, "I")], pos=124, ref=2, rng=random.Random(5), seqs=seqs, qual="none")]
    r = check(ctx, B.stream(recs, refs), gen, line_width=64)
    assert r.ins_sites == (5 if l_ref >= 257 else 4) and r.ins_unanchored == 2 and r.lengths[1:3] == [(1, 4), (0, 0)]
    assert r.lengths[0] == (l_ref, l_ref + (5 if l_ref >= 257 else 2)) and r.lengths[3] == (130, 130 + 1 + 4)
    # the same with the genome's records in another order: the padding lies elsewhere
    assert check(ctx, B.stream(recs, refs), gen[::-1], line_width=64).bases == r.bases


# ---------------------------------------------------------------- segment cuts
def test_insertions_at_the_cuts_of_a_long_record(ctx):
    """one record of more than SEG_OPS ops and more than SEG_COLS columns, laid over itself three times so that its insertions win:
    an I op that is the first column of a segment, a block of SEG_OPS ops that ends on an I, and the next block beginning with one"""
    assert SEG_COLS >= 1000 and SEG_OPS >= 8
    ops = [(SEG_COLS + 900, "M"), (SEG_COLS - 100, "D")]
    ops += [(3 * SEG_COLS - sum(n for n, _ in ops), "M"), (2, "I")]         # the I op begins at column 3 SEG_COLS
    ops += [(3, "M"), (1, "I")] * ((SEG_OPS - len(ops)) // 2)               # .. and op SEG_OPS - 1 is an I
    assert len(ops) == SEG_OPS and ops[-1][1] == "I"
    ops += [(2, "I"), (7, "M"), (1, "D"), (2, "M"), (1, "I"), (5, "M")]     # the next block begins with an I
    for pos in (0, 77):
        one = aligned("long", ops, pos=pos, rng=random.Random(5), keep=1.0)
        r = check(ctx, B.stream([one] * 3, REFS))
        # SEG_OPS / 2 + 1 I ops at SEG_OPS / 2 anchors: the two at the blocks' seam share theirs, and each counts from its own offset 0
        assert r.counts[8] == 3 and r.ins_sites == SEG_OPS // 2 and r.ins_longest == 2 and r.bases[5] == SEG_COLS - 99
        assert r.ins_len[1] == SEG_OPS // 2 - 2 and r.ins_len[2] == 2 and r.bases[3] == SEG_OPS // 2 + 2
    lead = aligned("lead", [(1, "I")] + ops, pos=3, rng=random.Random(6), placeholder=True, keep=1.0)
    r = check(ctx, B.stream([lead] * 3, REFS))
    assert r.ins_unanchored == 3 and r.ins_sites == SEG_OPS // 2


def test_an_insertion_longer_than_a_segment(ctx):
    """an I op of more than SEG_COLS columns that crosses a cut, under the default max_ins and the largest"""
    ops = [(100, "M"), (SEG_COLS + 50, "I"), (100, "M")]
    one = aligned("wide", ops, pos=1000, rng=random.Random(8), keep=1.0, qual="none")
    for max_ins in (1024, 65535):
        r = check(ctx, B.stream([one] * 3, REFS), max_ins=max_ins)
        assert r.ins_sites == 1 and r.ins_longest == min(max_ins, SEG_COLS + 50) and r.ins_capped == (max_ins == 1024) and r.ins_len[63] == 1


@pytest.mark.parametrize("n_ops", [64, 65, SEG_OPS, SEG_OPS + 1])
def test_op_counts_around_a_round_and_a_block(ctx, n_ops):
    rng = random.Random(n_ops)
    recs = [aligned("r%d" % k, noisy_ops(rng, n_ops, long_ops=k == 1), pos=50 * k, rng=rng, placeholder=k == 2) for k in range(3)]
    recs.append(aligned("ends_on_i", noisy_ops(rng, n_ops - 2) + [(1, "I"), (2, "S")], pos=10, rng=rng))
    r = check(ctx, B.stream(recs + recs[:2], REFS), max_ins=5)
    assert r.counts[8] == 6 and r.ins_sites > n_ops // 10 and (r.ins_capped >= 1) == (n_ops != 64) and r.ins_longest <= 5


# ---------------------------------------------------------------- max_ins
@pytest.mark.parametrize("max_ins", [1, 64, 1024])
def test_an_insertion_of_seventy_bases(ctx, max_ins):
    one = aligned("seventy", [(40, "M"), (70, "I"), (40, "M")], pos=500, rng=random.Random(70), keep=1.0, qual="none")
    r = check(ctx, B.stream([one] * 3, REFS), max_ins=max_ins)
    assert r.ins_sites == 1 and r.ins_longest == min(70, max_ins) and r.ins_capped == (max_ins < 70) and r.bases[3] == min(70, max_ins)
    assert r.ins_len[63] == (max_ins > 63) and r.ins_len[1] == (max_ins == 1)


# ---------------------------------------------------------------- contention
def test_four_thousand_records_insert_at_one_anchor(ctx):
    ref = CHR[:300]
    gen = [("hot", fasta_lines(ref))]
    body = ref[100:200].decode()
    recs = [exact("a%d" % k, body[:50] + "AC" + body[50:], 100, [(50, "M"), (2, "I"), (50, "M")]) for k in range(3000)]
    recs += [exact("g%d" % k, body[:50] + "G" + body[50:], 100, [(50, "M"), (1, "I"), (50, "M")]) for k in range(1000)]
    r = check(ctx, B.stream(recs, [("hot", 300)]), gen, line_width=0)
    assert r.max_depth == 4000 and r.ins_sites == 1 and r.ins_longest == 2
    assert r.text == b">hot\n" + b"N" * 100 + ref[100:150] + b"AC" + ref[150:200] + b"N" * 100 + b"\n"


# ---------------------------------------------------------------- exact recovery
def spell(ref, s, e, subs=(), dels=(), inss=()):
    """the record that covers [s, e) of ref and says the alternate sequence there, noise-free"""
    subs, inss = dict(subs), dict(inss)
    ops, seq = [], []

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
        if p in inss and p < e - 1:
            add(len(inss[p]), "I")
            seq.extend(inss[p])
    return exact("s%d" % s, "".join(seq), s, ops)


def test_noise_free_reads_spell_the_alternate_sequence(ctx):
    rng = random.Random(2027)
    ref = planted(rng, 2100, longest=5)[:2000]
    other = lambda p: rng.choice([c for c in b"ACGT" if c != ref[p]])
    subs, dels, inss = {300: other(300), 1500: other(1500)}, (705, 706), {1210: "GTA"}
    alt = bytearray()
    for p in range(len(ref)):
        if p not in dels:
            alt.append(subs.get(p, ref[p]))
        alt += inss.get(p, "").encode()
    gen = [("v", fasta_lines(ref))]
    recs = [spell(ref, s, s + 400, subs, dels, inss) for s in range(0, len(ref) - 400 + 1, 20)]
    r = check(ctx, B.stream(recs, [("v", len(ref))]), gen)
    assert r.text == b">v\n" + fasta_lines(bytes(alt)) and r.bases == [2001, 1996, 2, 3, 0, 2] and r.lengths == [(2000, 2001)]
    # noise-free reads of the genome give the genome
    plain = [spell(ref, s, s + 400) for s in range(0, len(ref) - 400 + 1, 20)]
    r = check(ctx, B.stream(plain, [("v", len(ref))]), gen)
    assert r.text == b">v\n" + fasta_lines(ref) and r.bases == [2000, 2000, 0, 0, 0, 0] and r.sites[8] == 0


# ---------------------------------------------------------------- files and order
def random_records(rng, n):
    out = []
    for k in range(n):
        kind = k % 23
        flag = [0, 16, 0x800, 0x100, 0x400, 4, 0x200][kind % 7 if kind < 14 else 0]
        ref = rng.randrange(2)
        ops = noisy_ops(rng, rng.choice([1, 2, 3, 5, 8, 30, 63, 64, 65, 66, 150]))
        if kind in (3, 15):
            ops = [(rng.randrange(3), "S"), (1, "I")] + ops
        rec = aligned("q%d" % k, ops, pos=rng.randrange(3000), ref=ref, rng=rng, flag=flag, mapq=rng.randrange(60), placeholder=kind in (20, 21),
                      qual="none" if k % 3 == 0 else "random")
        if kind == 22:
            rec = B.record("u%d" % k, 4 if k % 2 else 0, -1, -1, seq="ACGT", qual=b"\x05" * 4)
        out.append(rec)
    return out


def test_six_hundred_records_in_any_order_and_over_several_files(ctx):
    rng = random.Random(11)
    gen = [("chr", fasta_lines(CHR[:5000])), ("other", fasta_lines(OTHER[:4000], 71))]
    refs = [("chr", 5000), ("other", 4000)]
    recs = random_records(rng, 600)
    kw = dict(min_baseq=25, min_mapq=5)
    r = check(ctx, B.stream(recs, refs), gen, **kw)
    assert r.counts[8] > 300 and r.ins_unanchored > 10 and r.ins_sites > 100 and r.bases[2] > 10 and r.bases[5] > 10
    mixed = list(recs)
    rng.shuffle(mixed)
    files = [B.contain(B.stream(part, refs), "bgzf", 1024) for part in (mixed[:100], mixed[100:450], mixed[450:])]
    for order in (files, files[::-1]):
        got = ctx.bam_consensus(order, gen, **kw)
        compare(got, r)
        assert got[2] == r.text and got[3] == r.lengths


def test_references_by_name(ctx):
    rng = random.Random(13)
    one = [B.stream([aligned("a%d" % k, noisy_ops(rng, 20), pos=rng.randrange(5000), ref=0, rng=rng, seqs={0: SEQS[f]}) for k in range(50)],
                    [("ref", len(SEQS[f]))]) for f in (0, 1)]
    want = K.consensus(one, GEN, ref_names=["chr", "other"], line_width=0)
    got = ctx.bam_consensus([B.contain(s) for s in one], GEN, ref_names=["chr", "other"], line_width=0)
    compare(got, want)
    assert got[2] == want.text and want.counts[8] == 100 and got[3] == [(len(CHR), want.lengths[0][1]), (len(OTHER), want.lengths[1][1])]
    got = ctx.bam_consensus([B.contain(s) for s in one], GEN, ref_names=["chr", None], text=False)
    assert got[0]["counts"]["skipped_ref"] == 50                                            # "ref" is no record of the genome


# ---------------------------------------------------------------- the text's delivery
def deliver(ctx, datas, genome, piece_bytes, stop_after=None, stop_records=None):
    pieces, lengths = [], []

    def on_text(user, ptr, n, offset):
        pieces.append((offset, C.string_at(ptr, n)))
        return 0 if stop_after is not None and len(pieces) >= stop_after else 1

    def on_record(user, ref, l_ref, l_cons):
        lengths.append((ref, l_ref, l_cons))
        return 0 if stop_records is not None and len(lengths) >= stop_records else 1
    sink = P.ConsensusSink(None, P.CONSENSUS_TEXT_CB(on_text), P.CONSENSUS_RECORD_CB(on_record))
    opts = P.ConsensusOpts(0x900, 0, 0, 0, 1, 1024, 31, piece_bytes)
    keep = [(nm.encode(), bytes(lines)) for nm, lines in genome]
    refs = (P.ErrorsRef * len(keep))(*[P.ErrorsRef(nm, C.cast(C.c_char_p(lines), C.c_void_p), len(lines)) for nm, lines in keep])
    arr = (P.ErrorsFile * len(datas))(*[P.ErrorsFile(C.cast(C.c_char_p(d), C.c_void_p), len(d), None) for d in datas])
    res = P.ConsensusResult()
    ok = ctx.lib.pbsim_bam_consensus(ctx.h, refs, len(keep), arr, len(datas), C.byref(opts), C.byref(sink), C.byref(res))
    return ok, pieces, lengths, res


def test_delivery_in_pieces_and_every_container(ctx):
    rng = random.Random(14)
    gen = [("d0", fasta_lines(CHR[:700])), ("d1", fasta_lines(OTHER[-300:], 31))]
    refs, seqs = [("d0", 700), ("d1", 300)], {0: CHR[:700], 1: OTHER[-300:]}
    streams = [B.stream([aligned("q%d" % (100 * f + k), noisy_ops(rng, 30), pos=rng.randrange(500 if k % 2 == 0 else 150), ref=k % 2, rng=rng, seqs=seqs)
                         for k in range(40)], refs) for f in range(2)]
    want = K.consensus(streams, gen, line_width=31)
    assert len(want.text) > 1000 and want.ins_sites > 2
    datas = [B.contain(s) for s in streams]
    for piece in (0, 1, 7, 4096):
        ok, pieces, lengths, res = deliver(ctx, datas, gen, piece)
        assert ok == 1 and b"".join(p for _, p in pieces) == want.text and res.text_bytes == len(want.text)
        assert lengths == [(k, a, b) for k, (a, b) in enumerate(want.lengths)]
        at = 0
        for offset, p in pieces:
            assert offset == at and 1 <= len(p) <= (piece or len(want.text))
            at += len(p)
        assert piece != 7 or any(not p.endswith(b"\n") for _, p in pieces)                # a piece ends inside a line
    ok, pieces, _, res = deliver(ctx, datas, gen, 7, stop_after=3)
    assert ok == 0 and len(pieces) == 3 and b"sink aborted (text)" in ctx.lib.pbsim_last_error() and sum(res.counts) == 0 and res.text_bytes == 0
    ok, _, lengths, res = deliver(ctx, datas, gen, 0, stop_records=1)
    assert ok == 0 and len(lengths) == 1 and b"sink aborted (records)" in ctx.lib.pbsim_last_error() and sum(res.counts) == 0
    for container in ("bgzf", "stored", "gzip", "none"):
        check(ctx, streams, gen, container=container, block=1024, piece_bytes=7, line_width=31, want=want)


# ---------------------------------------------------------------- failures
def test_failures_say_why_and_leave_the_context_usable(ctx):
    def usable():
        assert check(ctx, B.stream(WORKED, WORKED_REFS), GENOME).report == WORKED_REPORT

    data = B.bam(WORKED, WORKED_REFS)
    for kw, word in REFUSED_OPTS:
        with pytest.raises(P.PbsimError, match="pbsim_bam_consensus: " + word):
            ctx.bam_consensus(data, GENOME, **kw)
    usable()
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_consensus: the reference \"c1\" has l_ref 11 in the file's header, and the genome's record of that "
                                           r"name has 10 bases"):
        ctx.bam_consensus(B.bam(WORKED, [("c1", 11), ("c2", 5)]), GENOME)
    usable()
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_consensus: file 1: the reference \"big\" has l_ref 10 .* has 51 bases"):
        ctx.bam_consensus([data, B.bam(WORKED[:1], [("ref", 10)])], GENOME + [("big", b"A" * 51)], ref_names=[None, "big"])
    usable()
    with pytest.raises(P.PbsimError, match="pbsim_bam_consensus: file 0 has 2 references: a reference name can be given only to a file with exactly one"):
        ctx.bam_consensus(data, GENOME, ref_names=["c1"])
    usable()
    good = [aligned("g%d" % k, [(5, "M"), (2, "I"), (5, "M")], pos=k) for k in range(50)]
    head = B.stream(good, REFS)
    bad_op = B.record_bytes(B.record("b", 0, 0, 1, cigar=[(2, "M")], seq="AC", qual=b"\x05\x05"))
    cig_at = 4 + 32 + 2
    bad_op = bad_op[:cig_at] + struct.pack("<I", 2 << 4 | 9) + bad_op[cig_at + 4:]
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_consensus: the record at inflated byte offset %d is malformed" % len(head)):
        ctx.bam_consensus(B.contain(head + bad_op + B.record_bytes(good[0]), "bgzf"), GEN)
    usable()
    with pytest.raises(P.PbsimError, match=r"pbsim_bam_consensus: file 1: the record at inflated byte offset %d is malformed" % len(head)):
        ctx.bam_consensus([B.contain(head), B.contain(head + bad_op, "none")], GEN)
    usable()
    with pytest.raises(P.PbsimError, match="pbsim_bam_consensus: neither BGZF, gzip nor an uncompressed BAM"):
        ctx.bam_consensus(b"@HD\tVN:1.6\n", GEN)
    usable()


# ---------------------------------------------------------------- the product's own files, through the command line
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


def _run(cmd, workdir):
    r = subprocess.run(cmd, capture_output=True, cwd=workdir, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return r


@pytest.mark.parametrize("method", ["errhmm", "qshmm"])
def test_cli_on_the_products_own_truth_files(tmp_path, method):
    """the consensus of the simulator's own truth files against the genome they were made from: FASTA and report are the model's,
    counts and sites are --pileup-bam's on the same files, and the sorted files give the same bytes"""
    from test_gpu_bam_errors import product_genome, simulate
    fasta = str(tmp_path / "genome.fa")
    genome = product_genome(fasta, 23, 100_000)
    _, alns, _ = simulate(str(tmp_path / "u"), fasta, method, 7, depth="6")
    assert len(alns) == 2
    names = ["--consensus-genome", fasta, "--consensus-ref-names", "chrA,chrB"]
    out = str(tmp_path / "consensus.fa")
    r = _run([CLI] + [x for aln in alns for x in ("--consensus-bam", aln)] + names + ["--consensus-out", out], str(tmp_path))
    streams = []
    for aln in alns:
        with open(aln, "rb") as f:
            streams.append(K.inflate(f.read()))
    want = K.consensus(streams, genome, ref_names=["chrA", "chrB"])
    with open(out, "rb") as f:
        text = f.read()
    assert r.stdout == want.report and text == want.text
    p = _run([CLI] + [x for aln in alns for x in ("--pileup-bam", aln)] + ["--pileup-genome", fasta, "--pileup-ref-names", "chrA,chrB"], str(tmp_path))
    assert p.stdout.split(b"\n")[:2] == r.stdout.split(b"\n")[:2]                          # the counts and the sites
    counts, sites, bases = dict(zip(K.COUNT_NAMES, want.counts)), dict(zip(K.SITE_NAMES, want.sites)), dict(zip(K.BASE_NAMES, want.bases))
    assert counts["scored"] == counts["records"] > 20 and sites["called"] > 150_000 and text.count(b">") == 2
    differ = sum(abs(l_cons - l_ref) for l_ref, l_cons in want.lengths)
    print(method, counts, sites, bases, "ins_sites %d longest %d" % (want.ins_sites, want.ins_longest),
          "the consensus differs from the genome by %d bases in count" % differ)
    # a second run with other options, and the sorted truth files give the same bytes as the unsorted
    copies = []
    for k, aln in enumerate(alns):
        copies.append(str(tmp_path / ("sorted%d.aln.bam" % k)))
        shutil.copy(aln, copies[-1])
    _run([CLI, "--sort-truth-bam"] + copies, str(tmp_path))
    out2 = str(tmp_path / "consensus2.fa")
    r2 = _run([CLI] + [x for c in copies for x in ("--consensus-bam", c)] + names + ["--consensus-out", out2, "--consensus-line-width", "60"], str(tmp_path))
    with open(out2, "rb") as f:
        assert f.read() == text and r2.stdout == r.stdout
    out3 = str(tmp_path / "consensus3.fa")
    r3 = _run([CLI, "--consensus-bam", alns[0], "--consensus-genome", fasta, "--consensus-ref-names", "chrA", "--consensus-out", out3, "--consensus-fill", "ref",
               "--consensus-line-width", "0", "--consensus-max-ins", "1", "--consensus-min-depth", "3"], str(tmp_path))
    want3 = K.consensus(streams[:1], genome, ref_names=["chrA"], fill="ref", line_width=0, max_ins=1, min_depth=3)
    with open(out3, "rb") as f:
        assert f.read() == want3.text and r3.stdout == want3.report
