"""tests/mutate_model.py (the rule of `pbsim --mutate-genome`) held to Philox's known answers, to a case worked out by hand, to its
own plain statement, to the applier and the caller of the call stage's model; and the places where the feature shows without a GPU:
the ABI's declarations with their ctypes mirror and the built library's symbols, pbsim_mutate_report against the model, the option
mirror with the command line's refusals, the checks in front of any device work, and the HIP-free rule file under the sanitizers."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import bam_writer as B
import call_model as V
import harness
import mutate_model as G
import pbsim3_amd as P
from pbsim3_amd import args as A
from test_abi_and_tables import KAT
from test_call_model import apply, lines_of
from test_gpu_bam_call import say

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")


# ---------------------------------------------------------------- Philox
def test_the_models_philox_has_the_known_answers():
    for ctr, key, want in KAT:
        assert tuple(int(w) for w in G.philox(*ctr, *key)) == want
    # arrays in, the same words out; a draw is a word shifted right by one
    got = G.philox(np.array([0, 0x243f6a88]), np.array([0, 0x85a308d3]), np.array([0, 0x13198a2e]), np.array([0, 0x03707344]), 0, 0)
    assert [int(w[0]) for w in got] == list(KAT[0][2])
    assert G.STREAM == int.from_bytes(b"MUTA", "big")
    block = G.philox(1, 2, 3, 4, 5, G.STREAM)                           # ctr = (j // 4, sub, p, r), key = (seed, the stream)
    assert [G.draw(5, 4, 3, 2, 4 + k) for k in range(4)] == [int(w) >> 1 for w in block]


# ---------------------------------------------------------------- the worked case of the rule
# w = ACGTTGCANNgattacaGGCTTAACCGGTAT (31 bases, an N run at 8 .. 9, lower case at 10 .. 16), x = TTGACCA; seed 31177, 100000 / 60000 /
# 120000 ppm, ext 500000, max_indel 5.  e = D(r, p, 0, 0) % 1000000 is below 100000 (snv), 160000 (ins), 280000 (del) at:
#   w 0   del, L 1: covers 1.                            w 1   del, L 1 (covers 2), itself deleted: merged.
#   w 2   del, L 2 (3 .. 4): merged.                     w 3   snv, deleted: dropped.
#   w 4   del, L 4: 5 .. 8, cut in front of the N at 8: 5 .. 7; merged.
#   w 5   snv: dropped.                                  w 6   del, L 4: 7 .. 10, cut to 7; merged.
#         The deleted run behind the anchor 0 is 1 .. 7:                                  w 1  ACGTTGCA -> A
#   w 12  ins, L 1, D(0, 12, 2, 0) % 4 = 1:                                               w 13 T -> TC
#   w 13  snv of T (i = 3), D(0, 13, 0, 1) = 253887765, % 3 = 0: "ACGT"[(3 + 1 + 0) % 4]  w 14 T -> A
#   w 14  del, L 1 (15):                                                                  w 15 AC -> A
#   w 16  del, L 4 (17 .. 20); the snvs at 17 and 19 are dropped:                         w 17 AGGCT -> A
#   w 22  del, L 2 (23 .. 24); 23 snv, dropped; 24 del, L 2 (25 .. 26), merged; 26 ins, dropped:   w 23 AACCG -> A
#   w 27  del, L 5 (max_indel): 28 .. 32, cut at the record's end to 28 .. 30:            w 28 GTAT -> G
#   x 6   ins on the last base, L 1, D(1, 6, 2, 0) % 4 = 1:                               x 7  A -> AC
WORKED_GENOME = [("w", b"ACGTTGCANNgattacaGGC\nTTAACCGGTAT\n"), ("x", b"TTGACCA")]
WORKED_OPTIONS = dict(seed=31177, snv_ppm=100000, ins_ppm=60000, del_ppm=120000, ext_ppm=500000, max_indel=5, line_width=5)
WORKED_FASTA = b">w\nANNGA\nTCAAA\nTAG\n>x\nTTGAC\nCAC\n"
WORKED_HEADER = (b"##fileformat=VCFv4.2\n##source=pbsim3_amd\n"
                 b"##pbsim_mutate=seed=31177;snv_ppm=100000;ins_ppm=60000;del_ppm=120000;ext_ppm=500000;max_indel=5\n"
                 b"##contig=<ID=w,length=31>\n##contig=<ID=x,length=7>\n"
                 b"##INFO=<ID=TYPE,Number=1,Type=String,Description=\"snv, ins, del or complex\">\n"
                 b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
WORKED_LINES = (b"w\t1\t.\tACGTTGCA\tA\t.\t.\tTYPE=del\n"
                b"w\t13\t.\tT\tTC\t.\t.\tTYPE=ins\n"
                b"w\t14\t.\tT\tA\t.\t.\tTYPE=snv\n"
                b"w\t15\t.\tAC\tA\t.\t.\tTYPE=del\n"
                b"w\t17\t.\tAGGCT\tA\t.\t.\tTYPE=del\n"
                b"w\t23\t.\tAACCG\tA\t.\t.\tTYPE=del\n"
                b"w\t28\t.\tGTAT\tG\t.\t.\tTYPE=del\n"
                b"x\t7\t.\tA\tAC\t.\t.\tTYPE=ins\n")
WORKED_ORIGINS = [[0, 8, 9, 10, 11, 12, -13, 13, 14, 16, 21, 22, 27], [0, 1, 2, 3, 4, 5, 6, -7]]
WORKED_NUMBERS = dict(records=2, bases_in=38, eligible=36, bases_out=21, drawn=[6, 3, 10], void_del=0, dropped=6, merged=5, substituted=1, inserted=2,
                      deleted=19, variants=8, types=[1, 2, 5], ref_bases=27, alt_bases=10, longest_ref=8, longest_alt=2, header_bytes=305, vcf_bytes=516,
                      fasta_bytes=32)
WORKED_REPORT = (b"#\trecords\tbases_in\teligible\tbases_out\tdrawn_snv\tdrawn_ins\tdrawn_del\tvoid_del\tdropped\tmerged\tsubstituted\tinserted\tdeleted\t"
                 b"variants\tsnv\tins\tdel\tref_bases\talt_bases\tlongest_ref\tlongest_alt\theader_bytes\tvcf_bytes\tfasta_bytes\n"
                 b"M\t2\t38\t36\t21\t6\t3\t10\t0\t6\t5\t1\t2\t19\t8\t1\t2\t5\t27\t10\t8\t2\t305\t516\t32\n")


def same(a, b):
    """two results of the model, the origin maps (arrays) included"""
    return a[:-2] == b[:-2] and a.report == b.report and len(a.origins) == len(b.origins) and all(np.array_equal(x, y) for x, y in zip(a.origins, b.origins))


@pytest.mark.parametrize("run", [G.mutate_plain, G.mutate], ids=["plain", "vectorised"])
def test_the_worked_case(run):
    r = run(WORKED_GENOME, **WORKED_OPTIONS)
    assert r.fasta == WORKED_FASTA and r.vcf == WORKED_HEADER + WORKED_LINES and r.report == WORKED_REPORT
    assert {k: getattr(r, k) for k in WORKED_NUMBERS} == WORKED_NUMBERS and len(WORKED_HEADER) == 305
    assert r.per_record == [(31, 13, 7), (7, 8, 1)] and [o.tolist() for o in r.origins] == WORKED_ORIGINS and all(o.dtype == np.int32 for o in r.origins)
    # the draws the comment above quotes
    assert G.draw(31177, 0, 13, 0, 1) == 253887765 and G.draw(31177, 0, 12, 2, 0) % 4 == 1 and G.draw(31177, 1, 6, 2, 0) % 4 == 1
    assert [G.draw(31177, 0, 4, 1, j) % 1000000 < 500000 for j in range(4)] == [True, True, True, False]
    assert all(G.draw(31177, 0, 27, 1, j) % 1000000 < 500000 for j in range(4))             # (L stops at max_indel)
    # the line width moves the line feeds only; max_indel 3 shortens the runs of 4, 6, 16 and 27
    assert run(WORKED_GENOME, **dict(WORKED_OPTIONS, line_width=0)).fasta == b">w\nANNGATCAAATAG\n>x\nTTGACCAC\n"
    short = run(WORKED_GENOME, **dict(WORKED_OPTIONS, max_indel=3))
    assert lines_of(short.vcf)[0] == b"w\t1\t.\tACGTTGCA\tA\t.\t.\tTYPE=del" and b"w\t17\t.\tAGGC\tA\t.\t.\tTYPE=del\n" in short.vcf and short.longest_ref == 8


# ---------------------------------------------------------------- properties
def bases_of(fasta):
    """name -> the bases of a FASTA's records"""
    out, name = {}, None
    for line in fasta.split(b"\n"):
        if line.startswith(b">"):
            name = line[1:]
            out[name] = b""
        elif line:
            out[name] += line
    return out


def rough_record(rng, n):
    return "".join(rng.choice("ACGTACGTACGTACGTNacgtnRy") for _ in range(n)).encode()


def four_records(seed=11):
    rng = random.Random(seed)
    a, b = rough_record(rng, 1004), rough_record(rng, 513)
    a = a[:300] + b"N" * 40 + a[340:]
    return [("a", b"\n".join(a[k:k + 70] for k in range(0, len(a), 70)) + b"\n"), ("none", b""), ("one", b"A\n"), ("b", b + b"\n")]


OPTION_SETS = [dict(), dict(snv_ppm=300000, ins_ppm=300000, del_ppm=300000), dict(seed=7, snv_ppm=100000, ins_ppm=50000, del_ppm=50000, ext_ppm=900000,
               max_indel=7, line_width=0), dict(seed=3, snv_ppm=0, ins_ppm=0, del_ppm=1000000, line_width=61)]


@pytest.mark.parametrize("kw", OPTION_SETS, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "defaults")
def test_the_vectorised_model_is_the_plain_statement(kw):
    genome = four_records()
    plain, fast = G.mutate_plain(genome, **kw), G.mutate(genome, **kw)
    assert same(plain, fast)
    r = fast
    # the identities (the model asserts them too), and what the texts say
    assert r.variants == sum(r.types) == sum(r.drawn) - r.dropped - r.merged == len(lines_of(r.vcf)) == sum(n for _, _, n in r.per_record)
    assert r.bases_out == r.bases_in + r.inserted - r.deleted == sum(n for _, n, _ in r.per_record) and r.substituted == r.types[0]
    assert (r.records, r.bases_in, r.header_bytes, r.vcf_bytes, r.fasta_bytes) == (4, 1004 + 1 + 513, r.vcf.index(b"#CHROM") + len(V.COLUMNS), len(r.vcf), len(r.fasta))
    assert r.vcf.startswith(G.header([("a", 1004), ("none", 0), ("one", 1), ("b", 513)], **{k: v for k, v in dict(G.DEFAULTS, **kw).items() if k != "line_width"}))
    assert b">none\n>one\nA\n>b\n" in r.fasta
    for line in lines_of(r.vcf):
        f = line.split(b"\t")
        assert f[2] == f[5] == f[6] == b"." and f[7] == b"TYPE=" + V.kind_of(f[3], f[4]).encode() != b"TYPE=complex"
    # the origin map: a kept base is the genome's, a substituted one is not, an inserted one points behind its anchor
    prepared, spelt = dict(G.prepared_records(genome)), bases_of(r.fasta)
    for (name, _), origin, (l_ref, l_out, _) in zip(genome, r.origins, r.per_record):
        seq, bases = prepared[name.encode()], np.frombuffer(spelt[name.encode()], dtype=np.uint8)
        assert len(origin) == l_out == len(bases) and len(seq) == l_ref
        own = origin >= 0
        assert np.all(np.diff(origin[own]) > 0) and int((bases[own] != seq[origin[own]]).sum()) <= r.substituted
        assert np.all(origin[1:][~own[1:]] <= -1) and (not len(origin) or own[0])
        anchor = np.maximum.accumulate(np.where(own, origin, -1))
        assert np.array_equal(-1 - origin[~own], anchor[~own])
    if kw.get("del_ppm") == 1000000:
        assert r.drawn[:2] == [0, 0] and r.inserted == 0 and all(line.endswith(b"TYPE=del") for line in lines_of(r.vcf)) and r.merged > 500


@pytest.mark.parametrize("kw", OPTION_SETS, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "defaults")
def test_the_truth_applied_to_the_genome_gives_the_variant_genome(kw):
    genome = four_records()
    r = G.mutate(genome, **dict(kw, line_width=0))
    assert apply(r.vcf, genome) == r.fasta


def spelling_reads(genome, fasta, origins):
    """three identical reads per record with bases that spell the variant genome, from the origin map alone: (stream, refs)"""
    prepared = dict(G.prepared_records(genome))
    refs = [(n, len(prepared[n.encode()])) for n, _ in genome if len(prepared[n.encode()])]          # (a BAM header has no reference of length 0)
    ids = {n: k for k, (n, _) in enumerate(refs)}
    recs, spelt = [], bases_of(fasta)
    for (name, _), origin in zip(genome, origins):
        if name not in ids:
            continue
        ref = prepared[name.encode()].tobytes()
        out = spelt[name.encode()]
        subs, inss, kept = {}, {}, set()
        for ch, o in zip(out, origin.tolist()):
            if o >= 0:
                kept.add(o)
                if ref[o] != ch:
                    subs[o] = ch
            else:
                inss[-1 - o] = inss.get(-1 - o, "") + chr(ch)
        dels = [p for p in range(len(ref)) if p not in kept]
        recs += [say("%s.%d" % (name, k), ref, 0, len(ref), subs=subs, dels=dels, inss=inss, ref_id=ids[name]) for k in range(3)]
    return B.stream(recs, refs), refs


def first_five(text):
    return [line.split(b"\t")[:5] for line in lines_of(text)]


@pytest.mark.parametrize("kw", OPTION_SETS[:3], ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "defaults")
def test_reads_that_spell_the_variant_genome_are_called_as_the_truth(kw):
    genome = four_records()
    r = G.mutate(genome, **dict(kw, line_width=0))
    stream, _ = spelling_reads(genome, r.fasta, r.origins)
    called = V.call(stream, genome, max_ins=65535)
    assert first_five(called.text) == first_five(r.vcf) and called.types[:3] == r.types and called.types[3] == 0 and called.variants == r.variants


def test_a_record_does_not_depend_on_the_others():
    genome = four_records()
    kw = dict(snv_ppm=100000, ins_ppm=50000, del_ppm=50000)
    whole = G.mutate(genome, **kw)
    b_alone = G.mutate(genome[3:], indices=[3], **kw)
    assert b_alone.per_record == whole.per_record[3:] and np.array_equal(b_alone.origins[0], whole.origins[3])
    assert b_alone.fasta == whole.fasta[whole.fasta.index(b">b\n"):] and lines_of(b_alone.vcf) == [l for l in lines_of(whole.vcf) if l.startswith(b"b\t")]
    # another record in front with the index kept: the same; the index moved: other draws
    front = G.mutate([("front", b"ACGTACGTAC")] + genome[3:], indices=[0, 3], **kw)
    assert front.per_record[1] == whole.per_record[3] and front.fasta.endswith(b_alone.fasta) and lines_of(front.vcf)[-b_alone.variants:] == lines_of(b_alone.vcf)
    assert G.mutate(genome[3:], **kw).fasta != b_alone.fasta
    # in the other order with the indices swapped accordingly: every record as before
    turned = G.mutate(genome[::-1], indices=[3, 2, 1, 0], **kw)
    assert turned.per_record == whole.per_record[::-1] and sorted(lines_of(turned.vcf)) == sorted(lines_of(whole.vcf))
    with pytest.raises(ValueError, match="two records named"):
        G.mutate(genome + [("a", b"AC")])


def test_the_length_rule_at_its_limits():
    genome = [("g", harness.synth_bases(2000, 5).tobytes())]
    r = G.mutate(genome, ins_ppm=2000, del_ppm=0, ext_ppm=999999, max_indel=65535)
    assert r.longest_alt == 65536 and r.drawn[1] >= 2 and r.inserted > 65535
    r = G.mutate(genome, ins_ppm=0, del_ppm=2000, ext_ppm=999999, max_indel=65535)          # the first run reaches the record's end
    assert r.drawn[2] >= 2 and r.variants == 1 and r.merged == r.drawn[2] - 1 and r.longest_ref == r.deleted + 1 == 2000 - r.bases_out + 1
    r = G.mutate(genome, ins_ppm=50000, del_ppm=50000, ext_ppm=0)
    assert r.longest_alt == 2 and r.inserted == r.types[1] and r.deleted <= r.drawn[2]        # (every run is one base; merged ones make a longer REF)
    r = G.mutate(genome, ins_ppm=50000, del_ppm=50000, ext_ppm=999999, max_indel=1)
    assert r.longest_alt == 2 and r.inserted == r.types[1] and r.deleted <= r.drawn[2]        # (every run is one base; merged ones make a longer REF)
    assert same(G.mutate(genome, ins_ppm=20000, ext_ppm=990000, max_indel=300), G.mutate_plain(genome, ins_ppm=20000, ext_ppm=990000, max_indel=300))
    none = G.mutate(genome, snv_ppm=0, ins_ppm=0, del_ppm=0)
    assert none.variants == 0 and none.vcf == G.header([("g", 2000)], snv_ppm=0, ins_ppm=0, del_ppm=0) and none.fasta == b">g\n" + G.wrap(genome[0][1], 60)


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_calls_and_the_library_has_them():
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        h = f.read()
    assert re.search(r"int pbsim_genome_mutate\(pbsim_ctx \*ctx, const pbsim_errors_ref \*refs, int n_refs, const pbsim_mutate_opts \*opts, "
                     r"const pbsim_mutate_sink \*sink,\s*pbsim_mutate_result \*result\);", h)
    assert re.search(r"int64_t pbsim_mutate_report\(const pbsim_mutate_result \*result, char \*buf, int64_t cap\);", h)
    opts = re.search(r"typedef struct pbsim_mutate_opts \{(.*?)\} pbsim_mutate_opts;", h, re.S).group(1)
    assert re.findall(r"^\s*(\w+ [\w, ]+);", opts, re.M) == ["uint32_t seed", "int32_t snv_ppm, ins_ppm, del_ppm", "int32_t ext_ppm", "int32_t max_indel",
                                                             "int32_t line_width", "int64_t piece_bytes"]
    body = re.search(r"typedef struct pbsim_mutate_result \{(.*?)\} pbsim_mutate_result;", h, re.S).group(1)
    declared = []
    for names in re.findall(r"int64_t ([^;]+);", body):
        for item in names.split(","):
            name, dims = re.match(r"\s*(\w+)((?:\[\d+\])*)", item).groups()
            declared.append((name, int(dims[1:-1]) if dims else 1))
    mirrored = [(n, C.sizeof(t) // 8) for n, t in P.MutateResult._fields_]
    assert declared == mirrored and C.sizeof(P.MutateResult) == 8 * sum(n for _, n in declared) == 8 * len(G.REPORT_NAMES)
    assert [n for n, _ in mirrored] == G.FIELDS and [k for n, k in mirrored if k > 1] == [3, 3]
    sink = re.search(r"typedef struct pbsim_mutate_sink \{(.*?)\} pbsim_mutate_sink;", h, re.S).group(1)
    assert re.findall(r"\(\*(\w+)\)", sink) == ["on_fasta", "on_vcf", "on_record", "on_origin"] == [n for n, _ in P.MutateSink._fields_[1:]]
    assert "int (*on_record)(void *user, int32_t ref, int64_t l_ref, int64_t l_out, int64_t n_variants);" in sink
    assert "int (*on_origin)(void *user, int32_t ref, const int32_t *origin, int64_t l_out);" in sink
    bound = [name for name, _, _ in P.API]
    assert "pbsim_genome_mutate" in bound and "pbsim_mutate_report" in bound
    assert [n for n, _ in P.MutateOpts._fields_] == ["seed", "snv_ppm", "ins_ppm", "del_ppm", "ext_ppm", "max_indel", "line_width", "piece_bytes"]
    assert C.sizeof(P.MutateOpts) == 40 and P.MutateOpts.piece_bytes.offset == 32 and P.MUTATE_TYPES == G.TYPE_NAMES
    assert callable(getattr(P.Context, "mutate_genome")) and callable(P.mutate_report)
    lib = P.load()
    assert hasattr(lib, "pbsim_genome_mutate") and hasattr(lib, "pbsim_mutate_report")


def as_dict(values):
    """the model's numbers (FIELDS order, drawn and types as lists) as the dict mutate_report takes"""
    return dict(zip(G.FIELDS, values))


def random_numbers(rng):
    pick = lambda: rng.choice([0, 0, 1, 10 ** 12, rng.randrange(2 ** 62)])
    return [[pick() for _ in range(3)] if name in ("drawn", "types") else pick() for name in G.FIELDS]


ZERO_REPORT = WORKED_REPORT.split(b"\n")[0] + b"\nM" + b"\t0" * 24 + b"\n"


def test_report_of_the_library_is_the_models_without_a_device():
    r = G.mutate(WORKED_GENOME, **WORKED_OPTIONS)
    assert P.mutate_report(as_dict(r[:20])) == WORKED_REPORT == G.report(r[:20])
    by_name = as_dict(r[:20])
    by_name.update(drawn=dict(zip(G.TYPE_NAMES, r.drawn)), types=dict(zip(G.TYPE_NAMES, r.types)))
    assert P.mutate_report(by_name) == WORKED_REPORT
    assert P.mutate_report(dict(drawn=[0] * 3, types=[0] * 3)) == ZERO_REPORT
    rng = random.Random(47)
    for _ in range(30):
        x = random_numbers(rng)
        assert P.mutate_report(as_dict(x)) == G.report(x)
    assert P.load().pbsim_mutate_report(None, None, 0) == -1
    with pytest.raises(ValueError, match="types has 4 values"):
        P.mutate_report(dict(drawn=[0] * 3, types=[0] * 4))


# ---------------------------------------------------------------- the option mirror and the command line
GOOD = ["--mutate-genome", "g.fa", "--mutate-out", "out.fa", "--mutate-vcf", "out.vcf"]
TAKES = "--mutate-genome takes --mutate-out, --mutate-vcf, --mutate-seed, --mutate-snv-ppm"
REFUSED = [
    (GOOD + ["--depth", "3"], "(--depth): " + TAKES),
    (GOOD + ["--call-out", "x"], "(--call-out): " + TAKES),
    (GOOD + ["--genome", "x"], "(--genome): " + TAKES),
    (GOOD + ["--call-bam", "x"], "(--mutate-genome): --call-bam takes"),
    (["--mutate-out", "o", "--mutate-genome"], "needs a value"),
    (["--mutate-genome", "g.fa", "--mutate-vcf", "v"], "--mutate-genome needs --mutate-out FASTA"),
    (["--mutate-genome", "g.fa", "--mutate-out", "o"], "--mutate-genome needs --mutate-vcf FILE"),
    (GOOD + ["--mutate-seed", "4294967296"], "(mutate-seed: 4294967296): a whole number, 0 .. 4294967295"),
    (GOOD + ["--mutate-seed", "-1"], "(mutate-seed: -1): a whole number"),
    (GOOD + ["--mutate-snv-ppm", "1000001"], "(mutate-snv-ppm: 1000001): a whole number, 0 .. 1000000"),
    (GOOD + ["--mutate-ins-ppm", "x"], "(mutate-ins-ppm: x): a whole number, 0 .. 1000000"),
    (GOOD + ["--mutate-del-ppm", "1e3"], "(mutate-del-ppm: 1e3): a whole number, 0 .. 1000000"),
    (GOOD + ["--mutate-snv-ppm", "500000", "--mutate-del-ppm", "500000"], "the three rates sum to more than 1000000"),
    (GOOD + ["--mutate-ext-ppm", "1000000"], "(mutate-ext-ppm: 1000000): a whole number, 0 .. 999999"),
    (GOOD + ["--mutate-max-indel", "0"], "(mutate-max-indel: 0): a whole number, 1 .. 65535"),
    (GOOD + ["--mutate-max-indel", "65536"], "(mutate-max-indel: 65536): a whole number, 1 .. 65535"),
    (GOOD + ["--mutate-line-width", "1048577"], "(mutate-line-width: 1048577): a whole number, 0 .. 1048576"),
    (GOOD + ["--devices", "0,1"], "--mutate-genome runs on one GPU"),
    (GOOD + ["--processes", "2"], "--mutate-genome runs on one GPU"),
]


def test_option_mirror_accepts_and_rejects():
    assert A.mutate_genome(GOOD) == dict(genome="g.fa", out="out.fa", vcf="out.vcf", seed=1, snv_ppm=1000, ins_ppm=100, del_ppm=100, ext_ppm=500000,
                                         max_indel=50, line_width=60)
    got = A.mutate_genome(["--mutate-vcf", "v", "--mutate-seed", "4294967295", "--mutate-out", "o", "--mutate-snv-ppm", "0", "--mutate-ins-ppm", "400000",
                           "--device", "1", "--mutate-del-ppm", "600000", "--mutate-genome", "g", "--mutate-ext-ppm", "999999", "--mutate-max-indel", "65535",
                           "--mutate-line-width", "0"])
    assert got == dict(genome="g", out="o", vcf="v", seed=4294967295, snv_ppm=0, ins_ppm=400000, del_ppm=600000, ext_ppm=999999, max_indel=65535,
                       line_width=0)
    for argv, message in REFUSED + [(["--mutate-out", "o"], "--mutate-genome FASTA: name the genome")]:
        if "--call-bam" in argv:
            continue                                # (the binary hands that line to the call stage's mode, which refuses it)
        with pytest.raises(ValueError) as e:
            A.mutate_genome(argv)
        assert message in str(e.value), argv


def test_cli_refuses_from_the_command_line_alone(tmp_path):
    """the same refusals by the binary, with the mirror's words, before a device or a file is touched"""
    import pbsim3_amd.build as b
    b.build()
    for argv, message in REFUSED:
        r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and r.stdout == "" and message in r.stderr, (argv, r.stderr[-500:])
    r = subprocess.run([CLI] + GOOD, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "--mutate-genome g.fa: Cannot open file: g.fa" in r.stderr
    assert os.listdir(tmp_path) == []
    r = subprocess.run([CLI], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert "--mutate-genome FASTA --mutate-out FASTA --mutate-vcf FILE" in r.stderr + r.stdout


# ---------------------------------------------------------------- the checks in front of any device work
REFUSED_OPTS = [(dict(snv_ppm=-1), "snv_ppm must be 0 .. 1000000"), (dict(ins_ppm=1000001), "ins_ppm must be 0 .. 1000000"),
                (dict(del_ppm=-5), "del_ppm must be 0 .. 1000000"), (dict(snv_ppm=400000, ins_ppm=400000, del_ppm=200001), r"snv_ppm \+ ins_ppm \+ del_ppm must not be above 1000000"),
                (dict(ext_ppm=1000000), "ext_ppm must be 0 .. 999999"), (dict(ext_ppm=-1), "ext_ppm must be 0 .. 999999"),
                (dict(max_indel=0), "max_indel must be 1 .. 65535"), (dict(max_indel=65536), "max_indel must be 1 .. 65535"),
                (dict(line_width=-1), "line_width must be 0 .. 1048576"), (dict(line_width=1048577), "line_width must be 0 .. 1048576"),
                (dict(piece_bytes=-1), "piece_bytes must not be negative")]


def test_bad_arguments_fail_before_device_work():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), -1) as c:
        for kw, word in REFUSED_OPTS:
            with pytest.raises(P.PbsimError, match="pbsim_genome_mutate: " + word):
                c.mutate_genome(WORKED_GENOME, **kw)
        with pytest.raises(P.PbsimError, match="pbsim_genome_mutate: bad argument"):
            c.mutate_genome([])
        with pytest.raises(P.PbsimError, match=r"pbsim_genome_mutate: the genome holds two records named \"w\" \(records 0 and 2\)"):
            c.mutate_genome(WORKED_GENOME + [("w", b"AC")])
        for kw in (dict(seed=-1), dict(seed=2 ** 32), dict(snv_ppm=2 ** 32 + 5), dict(max_indel=2 ** 31)):
            with pytest.raises(ValueError, match="does not fit its 32-bit field"):
                c.mutate_genome(WORKED_GENOME, **kw)
        # a missing name, through the library itself
        refs = (P.ErrorsRef * 1)(P.ErrorsRef(None, None, 0))
        res = P.MutateResult()
        assert c.lib.pbsim_genome_mutate(c.h, refs, 1, None, None, C.byref(res)) == 0
        assert b"pbsim_genome_mutate: bad argument (genome record 0)" in c.lib.pbsim_last_error()
        # good arguments reach the device check: a tables-only context refuses as pbsim_inflate_buffer does, and stays usable
        for kw in (dict(), dict(text=False), dict(origin=True), dict(seed=2 ** 32 - 1, snv_ppm=0, ins_ppm=0, del_ppm=1000000, ext_ppm=999999,
                                                                      max_indel=65535, line_width=0, piece_bytes=7)):
            with pytest.raises(P.PbsimError, match="no HIP device"):
                c.mutate_genome(WORKED_GENOME, **kw)


# ---------------------------------------------------------------- the host's decisions under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("asan") / "genome_mutate_rule_driver")
    p = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(harness.ROOT, "tests", "asan", "genome_mutate_rule_driver.cpp"), os.path.join(csrc, "genome_mutate_rule.cpp"),
                        "-o", exe], capture_output=True, text=True)
    if p.returncode != 0 and "sanitize" in p.stderr:
        pytest.skip("no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def drive(exe, *argv):
    p = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, timeout=60)
    assert p.returncode == 0, (argv, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout


def test_rule_code_under_asan(driver):
    assert drive(driver, "opts", "-") == b"opts 1 1000 100 100 500000 50 60 8388608\n"
    assert drive(driver, "opts", 4294967295, 0, 400000, 600000, 999999, 65535, 0, 7) == b"opts 4294967295 0 400000 600000 999999 65535 0 7\n"
    assert drive(driver, "opts", 0, 1000000, 0, 0, 0, 1, 1048576, 0) == b"opts 0 1000000 0 0 0 1 1048576 8388608\n"
    good = [1, 1000, 100, 100, 500000, 50, 60, 0]
    for at, value, word in ((1, -1, b"snv_ppm"), (1, 1000001, b"snv_ppm"), (2, -1, b"ins_ppm"), (2, 1000001, b"ins_ppm"), (3, -1, b"del_ppm"),
                            (3, 1000001, b"del_ppm"), (3, 999000, b"snv_ppm + ins_ppm + del_ppm"), (4, -1, b"ext_ppm"), (4, 1000000, b"ext_ppm"),
                            (5, 0, b"max_indel"), (5, 65536, b"max_indel"), (5, -7, b"max_indel"), (6, -1, b"line_width"), (6, 1048577, b"line_width"),
                            (7, -1, b"piece_bytes")):
        bad = list(good)
        bad[at] = value
        assert drive(driver, "opts", *bad).startswith(b"opts refused: " + word), bad
    assert drive(driver, "header", 31177, 100000, 60000, 120000, 500000, 5, "w", 31, "x", 7) == WORKED_HEADER
    assert drive(driver, "header", 1, 1000, 100, 100, 500000, 50) == G.header([])
    assert drive(driver, "header", 4294967295, 0, 0, 1000000, 999999, 65535, "x" * 300, 10 ** 15, "", 0) == \
        G.header([("x" * 300, 10 ** 15), ("", 0)], seed=4294967295, snv_ppm=0, ins_ppm=0, del_ppm=1000000, ext_ppm=999999, max_indel=65535)
    assert drive(driver, "report", *G.flat(G.mutate(WORKED_GENOME, **WORKED_OPTIONS)[:20])) == WORKED_REPORT
    assert drive(driver, "report", *([0] * 24)) == ZERO_REPORT
    rng = random.Random(48)
    for _ in range(5):
        x = random_numbers(rng)
        assert drive(driver, "report", *G.flat(x)) == G.report(x)
