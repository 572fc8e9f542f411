"""pbsim_bam_lift on the device against tests/lift_model.py, byte for byte: the whole lifted BAM inflated and compared with the
model's stream (header, reference list, records), and read back by the spec reader; then end to end on the product's own genomes,
reads and truth files.  Every test fails without the feature: Context.lift_bam does not exist before it."""
import re

import numpy as np
import pytest

import bam_spec_reader as R
import bam_writer as B
import harness
import lift_model as L
import mutate_model as MM
import pbsim3_amd as P
import pbsim3_amd.args as A
from stats_model import inflate
from test_gpu_bam_grid_caps import constant
from test_lift_model import GENOME, OPS, ORIGIN, header_text, one_record_stream, parse_stream, random_genome, random_origin, random_record, record_fields

pytestmark = pytest.mark.gpu

SEG_OPS, SEG_COLS = constant("bam_errors.h", "kErrSegOps"), constant("bam_errors.h", "kErrSegCols")


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


def check(ctx, stream, genome, origins, container="bgzf", block=B.W.BGZIP_BLOCK, **kw):
    """the stream through the product in this container: the lifted file's inflated bytes, the result and the report are the model's"""
    want, res = L.lift_stream(stream, genome, origins, **kw)
    got = ctx.lift_bam(B.contain(stream, container, block), genome, origins, **kw)
    assert got[0] == res
    assert got[1] == L.report(res)
    assert inflate(got[2]) == want
    text, refs, recs = R.read_bam(got[2])          # (BGZF with the EOF block, every record whole)
    assert len(recs) == res["records"] - res["unsupported"] - res["unplaced"]
    return want, res, got[2]


def random_case(seed, n_records=200, sizes=None, rate_ppm=50000):
    """two genome records, their origin maps from the mutate model at raised rates, records on both variant records"""
    rng = np.random.default_rng(seed)
    genome = random_genome(rng, sizes or [int(rng.integers(300, 2001)) for _ in range(2)])
    origins = MM.mutate(genome, seed=seed, snv_ppm=rate_ppm, ins_ppm=rate_ppm, del_ppm=rate_ppm, max_indel=9).origins
    refs = [(nm, len(o)) for (nm, _), o in zip(genome, origins)]
    recs = []
    for k in range(n_records):
        ref = int(rng.integers(0, 2))
        if k % 23 == 5:
            recs.append(B.record("u%d" % k, flag=4, seq="ACGT", qual=bytes(4)))
        elif k % 29 == 7:
            recs.append(B.record("n%d" % k, flag=0, ref_id=ref, pos=3, cigar=[(4, "M"), (5, "N"), (3, "M")], seq="ACGTACG", qual=bytes(7)))
        else:
            recs.append(random_record(rng, k, ref, refs[ref][1], qual=k % 5 != 0, n_ops=int(rng.integers(1, 90)) if k % 7 else None))
            if k % 31 == 0:
                recs[-1] = dict(recs[-1], seq="", qual=b"")
    return B.stream(recs, refs=refs, text=header_text(refs)), genome, origins


@pytest.mark.parametrize("seed", [1, 2])
def test_random_small_files(ctx, seed):
    stream, genome, origins = random_case(seed)
    want, res, _ = check(ctx, stream, genome, origins)
    for k in ("unaligned", "unsupported", "lifted", "moved", "no_seq", "gap_del", "bases_to_ins", "dels_vanished", "sub", "soft"):
        assert res[k] > 0, (k, res)
    assert b"SO:unsorted" in want and res["lifted"] > 150


def test_every_container_gives_the_same_bytes(ctx):
    stream, genome, origins = random_case(3, n_records=120)
    first = check(ctx, stream, genome, origins)[2]
    for container in ("stored", "gzip", "none"):
        assert check(ctx, stream, genome, origins, container=container)[2] == first
    assert check(ctx, stream, genome, origins, block=777)[2] == first


def ops_record(name, ops, pos=0, seq_of="A"):
    l_seq = sum(n for n, op in ops if op in "MIS=X")
    return B.record(name, flag=0, ref_id=0, pos=pos, cigar=ops, seq=seq_of * l_seq, qual=bytes(l_seq), tags=[("NM", "i", 1), ("zz", "Z", name)])


def test_wave_and_round_seams(ctx):
    rng = np.random.default_rng(4)
    genome = random_genome(rng, [6000])
    origin = random_origin(rng, 6000, rate=0.05)
    recs = []
    for n in (1, 63, 64, 65, 128, 129):
        recs.append(ops_record("n%d" % n, [(2, "M") if k % 2 == 0 else (1, "ID"[(k // 2) % 2]) for k in range(n)], pos=7 * n))
    # one record whose columns cross a block of ops and a segment of columns of the record pass
    long_ops = [(3, "M"), (1, "I"), (2, "M"), (2, "D")] * ((SEG_OPS + 64) // 4) + [(SEG_COLS + 100 - 8 * ((SEG_OPS + 64) // 4), "M")]
    recs.append(ops_record("seam", long_ops, pos=11))
    assert len(long_ops) > SEG_OPS and sum(n for n, _ in long_ops) > SEG_COLS
    refs = [("chr0", len(origin))]
    want, res, _ = check(ctx, B.stream(recs, refs=refs, text=header_text(refs)), genome, [origin])
    assert res["lifted"] == len(recs) and res["moved"] == len(recs)


def placeholder_record(name, ops, pos=0):
    l_seq = sum(n for n, op in ops if op in "MIS")
    span = sum(n for n, op in ops if op in "MD")
    return B.record(name, flag=0, ref_id=0, pos=pos, cigar=[(l_seq, "S"), (span, "N")], seq="A" * l_seq, qual=b"\xff" * l_seq,
                    tags=[("NM", "i", 0), ("CG", "BI", [n << 4 | OPS.index(op) for n, op in ops]), ("zz", "i", 5)])


def test_placeholder_seams(ctx):
    """65 534 ops that lift to more, a placeholder of 65 536 that lifts to fewer, and one that stays above the limit both ways"""
    l_orig = 200000
    origin = list(range(l_orig))
    del origin[50001:50003]                                  # a deletion under an M of the first record: 2 ops more
    at = origin.index(120001)
    origin[at:at] = [-1 - 120000] * 2                        # an insertion under a D of the second record: the D vanishes
    origin = np.array(origin, dtype=np.int32)
    assert L.check_origin(origin, l_orig) is None
    genome = [("c", b"A" * l_orig)]
    up = [(1, "M"), (1, "I")] * 32766 + [(30000, "M"), (1, "I")]       # 65 534 ops; the long M lies over the deletion
    start = 50001 - 32766 - 100
    down_pos = at - 11                                       # eleven M columns, then the D on the two inserted bases
    down = [(1, "M"), (1, "I")] * 10 + [(1, "M"), (2, "D")] + [(1, "I"), (1, "M")] * 32757   # 65 536 ops; the D lies on the inserted bases
    both = [(1, "M"), (1, "I")] * 35000 + [(1, "M")]
    assert len(up) == 65534 and len(down) == 65536
    recs = [ops_record("up", up, pos=start), placeholder_record("down", down, pos=down_pos), placeholder_record("both", both, pos=130000)]
    refs = [("c", len(origin))]
    want, res, _ = check(ctx, B.stream(recs, refs=refs, text=header_text(refs)), genome, [origin])
    got = [record_fields(r) for r in parse_stream(want)[1]]
    assert res["long_cigar_in"] == 2 and res["long_cigar_out"] == 2 and res["lifted"] == 3
    assert got[0]["cigar"].endswith("N") and got[0]["tags"] == ["NM", "CG", "zz"]
    assert not got[1]["cigar"].endswith("N") and got[1]["cigar"].count("M") + got[1]["cigar"].count("I") == 65535 and got[1]["tags"] == ["NM", "zz"]
    assert got[2]["cigar"].endswith("N") and got[2]["tags"] == ["NM", "CG", "zz"]


def test_member_seams(ctx):
    """records whose sizes change across the 32 KiB boundaries of the output's members"""
    stream, genome, origins = random_case(5, n_records=1500, sizes=[1500, 1800])
    want, res, lifted = check(ctx, stream, genome, origins)
    assert len(want) > 3 * 32768 and res["bytes_in"] != res["bytes_out"]
    assert len(list(R.blocks(lifted))) >= 4


def test_an_empty_file_and_only_unmapped_records(ctx):
    refs = [("c", len(ORIGIN))]
    want, res, _ = check(ctx, B.stream([], refs=refs, text=header_text(refs)), GENOME, [ORIGIN])
    assert res == dict.fromkeys(L.COUNTS + L.TOTALS, 0) and b"LN:8" in want
    recs = [B.record("u%d" % k, flag=4, seq="ACGT" * k, qual=bytes(4 * k), tags=[("NM", "C", k)]) for k in range(70)]
    stream = B.stream(recs, refs=refs, text=header_text(refs))
    want, res, _ = check(ctx, stream, GENOME, [ORIGIN])
    assert res["records"] == res["unaligned"] == 70 and parse_stream(want)[1] == parse_stream(stream)[1]


def test_failures_leave_the_context_usable(ctx):
    good = one_record_stream(flag=0, ref_id=0, pos=0, cigar=[(9, "M")], seq="ACGACTTGT", qual=bytes(9))

    def usable():
        assert check(ctx, good, GENOME, [ORIGIN])[1]["lifted"] == 1
    usable()
    with pytest.raises(P.PbsimError, match=r"the reference \"c\" has l_ref 9 .* has 8 bases: this is not the genome these reads came from"):
        ctx.lift_bam(good, GENOME, [ORIGIN[:8]])
    usable()
    with pytest.raises(P.PbsimError, match="the genome has no record named \"c\""):
        ctx.lift_bam(good, [("d", b"ACGTACGT")], [ORIGIN])
    assert ctx.lift_bam(good, [("d", b"ACGTACGT")], [ORIGIN], ref_name="d")[0]["lifted"] == 1
    assert ctx.lift_bam(good, [("d", b"ACGTACGT")], [ORIGIN], ref_names=["c"])[0]["lifted"] == 1
    for bad, at in (([0, 1, 2, 4, 5, -6, -6, 6, 8], 8), ([0, 1, 2, 4, 4, -5, -5, 6, 7], 4), ([0, 1, 2, 4, 5, -5, -6, 6, 7], 5),
                    ([-1, 1, 2, 4, 5, -6, -6, 6, 7], 0), ([0, 1, 2, 4, 5, -6, L.FRONT, 6, 7], 6), ([0, 1, 3, 2, 5, -6, -6, 6, 7], 3)):
        with pytest.raises(L.LiftError):
            L.lift_stream(good, GENOME, [bad])
        with pytest.raises(P.PbsimError, match="the origin map of \"c\" is not one: variant position %d:" % at):
            ctx.lift_bam(good, GENOME, [bad])
        usable()
    for kw in (dict(pos=8, cigar=[(2, "M")], seq="AC"), dict(pos=0, cigar=[(3, "M")], seq="AC")):
        with pytest.raises(P.PbsimError, match="is malformed: its CIGAR runs past its reference, or its query length is not l_seq"):
            ctx.lift_bam(one_record_stream(flag=0, ref_id=0, qual=bytes(2), **kw), GENOME, [ORIGIN])
        usable()
    with pytest.raises(P.PbsimError, match="neither BGZF, gzip nor an uncompressed BAM stream"):
        ctx.lift_bam(b"not a BAM", GENOME, [ORIGIN])
    usable()


# ---------------------------------------------------------------- end to end, on the product's own genome, reads and truth files
# seed 3, 4 000 and 3 000 bases, snv 2 %, ins and del 0.5 % each with runs of at most 6: the model alone leaves
# unplaced + unsupported = 0 of the records of both methods below (reads of 100 bases and more never lie inside 6 inserted bases).
E2E = dict(seed=3, snv_ppm=20000, ins_ppm=5000, del_ppm=5000, ext_ppm=400000, max_indel=6)
METHODS = {"errhmm": ["--method", "errhmm", "--errhmm", "MODEL:ERRHMM-RSII.model"], "qshmm": ["--method", "qshmm", "--qshmm", "MODEL:QSHMM-RSII.model"]}


def e2e_genome():
    rng = np.random.default_rng(17)
    return [("chrA", bytes(rng.choice(list(b"ACGT"), 4000).astype(np.uint8))), ("chrB", bytes(rng.choice(list(b"ACGT"), 3000).astype(np.uint8)))]


def simulate_truth(method, records, arrays=False):
    """per variant record its truth BAM stream (header and records, inflated) and, on request, the per-base reference positions"""
    argv = harness.resolve(["--strategy", "wgs"] + METHODS[method] + ["--depth", "6", "--seed", "9", "--length-mean", "400", "--length-sd", "100",
                                                                      "--length-min", "100", "--length-max", "900"])
    p, a = A.parse(argv)
    out = []
    with P.Context(p, 0) as c:
        c.load_errhmm(a["--errhmm"]) if method == "errhmm" else c.load_qshmm(a["--qshmm"])
        c.set_truth_bam(True)
        for i, seq in enumerate(records, 1):
            c.set_reference(seq, i)
            _, truth = c.simulate_wgs()
            stream = c.truth_bam_header() + truth
            batch = c.simulate_arrays(labels=True) if arrays else None
            out.append((stream, batch))
    return out


def fasta_records(fasta):
    return [b"".join(part.split(b"\n")[1:]) for part in fasta.split(b">")[1:]]


@pytest.mark.parametrize("method", ["errhmm", "qshmm"])
def test_end_to_end(ctx, method):
    genome = e2e_genome()
    m = ctx.mutate_genome(genome, origin=True, **E2E)
    fasta, vcf, origins = m[2], m[3], m[5]
    variant = fasta_records(fasta)
    assert [len(v) for v in variant] == [len(o) for o in origins] and len(variant[0]) != len(genome[0][1])
    applied = ctx.apply_vcf(vcf, genome, origin=True, fasta=False, text=False)[2]
    assert all(np.array_equal(a, b) for a, b in zip(applied, origins))      # 3. the VCF is the chain: the same maps, so the same bytes
    for k, (stream, batch) in enumerate(simulate_truth(method, variant, arrays=True)):
        name = genome[k][0]
        want, res = L.lift_stream(stream, genome, origins, ref_name=name)
        got = ctx.lift_bam(B.W.bgzf(stream), genome, origins, ref_name=name)
        assert got[0] == res and inflate(got[2]) == want
        assert ctx.lift_bam(B.W.bgzf(stream), genome, applied, ref_name=name)[2] == got[2]
        print(method, name, res)
        # 1. every lifted record's NM is what the errors stage finds against the ORIGINAL genome; unlifted it is not
        assert res["moved"] > 0 and res["records"] > 20
        assert 100 * (res["unplaced"] + res["unsupported"]) <= res["records"]
        prof = ctx.bam_errors(got[2], genome, ref_names=[name])[0]["counts"]
        assert prof["nm_differ"] == 0 and prof["nm_agree"] == prof["scored"] == res["lifted"] > 0
        try:                                                                # (the same records against the original genome, unlifted)
            assert ctx.bam_errors(B.W.bgzf(stream), genome, ref_names=[name])[0]["counts"]["nm_differ"] > 0
        except P.PbsimError as e:
            assert "this is not the genome the reads were aligned to" in str(e)
        # 2. the per-base reference positions of simulate_arrays, taken through the origin map, give pos and pos + span - 1
        lifted = [record_fields(r) for r in parse_stream(want)[1]]
        ref_pos, offsets = batch.ref_pos.cpu().numpy(), batch.offsets.cpu().numpy()
        assert len(lifted) == len(offsets) - 1 == res["lifted"]
        origin = origins[k]
        for t, f in enumerate(lifted):
            placed = np.sort(ref_pos[offsets[t]:offsets[t + 1]])
            kept = origin[placed[placed >= 0]]
            kept = kept[kept >= 0]
            ops = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDSH])", f["cigar"])]
            span = sum(n for n, op in ops if op in "MD")
            assert (f["pos"], f["pos"] + span - 1) == (int(kept[0]), int(kept[-1])), (t, f)
        # 4. the lifted file as truth and as query, held to the same interval (overlap 1): every read correct; with the unlifted
        # file as truth the reads behind the first indel lie elsewhere, so they are not
        counts = ctx.eval_bam(got[2], got[2], ref_names=[None], overlap=1.0)[0]
        assert counts["correct"] == counts["scored"] == res["lifted"] and counts["wrong"] == counts["missing"] == 0
        try:
            counts = ctx.eval_bam(B.W.bgzf(stream), got[2], ref_names=[None], overlap=1.0)[0]
            assert counts["correct"] < counts["scored"]
        except P.PbsimError as e:                                           # (its header speaks of another l_ref)
            assert len(variant[k]) != len(genome[k][1]), str(e)
