"""tests/apply_model.py (the rule of `pbsim --apply-vcf`) held to a case worked out by hand, to a naive splice and to the mutate
model's own FASTA; and the places where the feature shows without a GPU: the ABI's declarations with their ctypes mirror and the built
library's symbols, pbsim_apply_report and pbsim_apply_sample against the model, the option mirror with the command line's refusals,
the checks in front of any device work, and the HIP-free rule file under the sanitizers."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import apply_model as M
import harness
import mutate_model as G
import pbsim3_amd as P
from pbsim3_amd import args as A
from test_mutate_model import OPTION_SETS, four_records

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")
HEAD = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA1\tNA2\n"


def vcf(rows, head=HEAD):
    """rows of (chrom, pos, ref, alt[, gt[, filter[, format]]]) as a VCF text with two samples, the second one's genotype `0|0`"""
    out = [head]
    for row in rows:
        chrom, pos, ref, alt = row[:4]
        gt, fil, fmt = (row[4] if len(row) > 4 else "1|1"), (row[5] if len(row) > 5 else "."), (row[6] if len(row) > 6 else "GT")
        out.append(("%s\t%s\t.\t%s\t%s\t.\t%s\t.\t%s\t%s\t0|0\n" % (chrom, pos, ref, alt, fil, fmt, gt)).encode())
    return b"".join(out)


# ---------------------------------------------------------------- the worked case of the rule
# c1 = ACGT six times, positions 0 .. 23; c2 is empty; c3 = TTGA.  The forms, haplotype 0 (the first ALT), by line number:
#    1  `1 ACGTACGTAC T`     no first or last byte in common: (0, 10, T), the span [0, 10)
#    2  `6 CGTACGTACGTACGT A`  (5, 15, A), [5, 20)             3  `16 TAC G`  (15, 3, G), [15, 18)
#    4  `1 A GA`   the first bytes differ, the last A goes: (0, 0, G), an insertion in front of the record's first base
#    5  `10 C CTT` the first C goes: (10, 0, TT), at the end of line 1's span     6  `3 G GA` (3, 0, A), strictly inside it
#    7  `22 C CA`  (22, 0, A)       8  `22 C CG` (22, 0, G), the same site        9  `24 T TGG` (24, 0, GG), behind the last base
#   10  `21 A C`   (20, 1, C)      11  `19 GT G` (19, 1, ), a deletion
#   12 .. 17: POS 0 malformed, cX unknown_contig, <DEL> unsupported, `1 C A` ref_mismatch, FILTER q10 filtered, `2 c C` no_change
#   18  `23 G A,GCC`  allele 1: (22, 1, A); allele 2 loses its first G: (23, 0, CC)         19  `c3 1 T C`  (0, 1, C) of record 2
# In order of (s, insertions first, line) with end = 0: 4 applied; 1 applied, end = 10; 6 (3 < 10) and 2 (5 < 10) overlap by 1; 5
# (10 >= 10) applied; 3 (15 >= 10: line 2 lost and blocks nothing) applied, end = 18; 11 applied, end = 20; 10 applied, end = 21; 7
# applied; 8 overlap by 7; 18 applied, end = 23; 9 (24 >= 23) applied.  The clusters: 4 | 1 6 2 5 3 11 (each begins in front of 10
# or 20) | 10 | 7 8 | 18 | 9 | 19: the longest has 6 lines.
# c1 spells G T (0 .. 9) TT G TACG (10 .. 14) G (15 .. 17) G (18) - (19) C (20) C (21) A A (22) T (23) GG = 18 bases;
# inserted 1 + 2 + 1 + 2 = 6, deleted 9 + 2 + 1 = 12, substituted 1 + 1 + 1 + 1 (lines 1, 3, 10, 18) + 1 (line 19) = 5; 24 + 6 - 12 = 18.
# Haplotype 1: line 10 (0|1) is ref_allele and line 11 (.|1) no_call, so 19 and 20 keep T and A; line 18 (1|2) takes allele 1.
# Haplotype 2: 10 and 11 are applied; line 18 takes allele 2, an insertion at 23: ... C C A G CC T GG.
WORKED_GENOME = [("c1", b"ACGTACGTACGT\nACGTACGTACGT\n"), ("c2", b""), ("c3", b"TTGA\n")]
WORKED_VCF = vcf([("c1", 1, "ACGTACGTAC", "T"), ("c1", 6, "CGTACGTACGTACGT", "A"), ("c1", 16, "TAC", "G"), ("c1", 1, "A", "GA"), ("c1", 10, "C", "CTT"),
                  ("c1", 3, "G", "GA"), ("c1", 22, "C", "CA"), ("c1", 22, "C", "CG"), ("c1", 24, "T", "TGG"), ("c1", 21, "A", "C", "0|1"),
                  ("c1", 19, "GT", "G", ".|1"), ("c1", 0, "A", "C"), ("cX", 1, "A", "C"), ("c1", 1, "A", "<DEL>"), ("c1", 1, "C", "A"),
                  ("c1", 2, "C", "A", "1|1", "q10"), ("c1", 2, "c", "C"), ("c1", 23, "G", "A,GCC", "1|2"), ("c3", 1, "T", "C", "1", ".", "GT:DP")])
WORKED_FORMS = [(0, 0, 10, b"T"), (0, 5, 15, b"A"), (0, 15, 3, b"G"), (0, 0, 0, b"G"), (0, 10, 0, b"TT"), (0, 3, 0, b"A"), (0, 22, 0, b"A"), (0, 22, 0, b"G"),
                (0, 24, 0, b"GG"), (0, 20, 1, b"C"), (0, 19, 1, b""), None, None, None, None, None, None, (0, 22, 1, b"A"), (2, 0, 1, b"C")]
CLASSES_12_17 = ["malformed", "unknown_contig", "unsupported", "ref_mismatch", "filtered", "no_change"]
WORKED_VERDICTS = {0: ["applied", "overlap", "applied", "applied", "applied", "overlap", "applied", "overlap", "applied", "applied", "applied"] + CLASSES_12_17 +
                      ["applied", "applied"]}
WORKED_VERDICTS[1] = WORKED_VERDICTS[0][:9] + ["ref_allele", "no_call"] + WORKED_VERDICTS[0][11:]
WORKED_VERDICTS[2] = WORKED_VERDICTS[0]
WORKED_BY = [0, 1, 0, 0, 0, 1, 0, 7] + [0] * 11
WORKED_FASTA = {0: b">c1\nGTTTGTACGGGCCAATGG\n>c2\n>c3\nCTGA\n", 1: b">c1\nGTTTGTACGGGTACAATGG\n>c2\n>c3\nCTGA\n", 2: b">c1\nGTTTGTACGGGCCAGCCTGG\n>c2\n>c3\nCTGA\n"}
WORKED_ORIGINS = [[-2 ** 31, 0, -10, -10, 10, 11, 12, 13, 14, 15, 18, 20, 21, -22, 22, 23, -24, -24], [], [0, 1, 2, 3]]
WORKED_REPORT = (b"#\tlines\tmalformed\tunknown_contig\tno_call\tref_allele\tunsupported\tref_mismatch\tfiltered\tno_change\toverlap\tapplied\tsnv\tins\tdel\tcomplex"
                 b"\tbases_in\tbases_out\tinserted\tdeleted\tsubstituted\tlongest_cluster\tfasta_bytes\ttext_bytes\n"
                 b"A\t19\t1\t1\t0\t0\t1\t1\t1\t1\t3\t10\t3\t4\t1\t2\t28\t22\t6\t12\t5\t6\t36\t404\n")
WORKED_HEADER = b"#line\tCHROM\tPOS\tREF\tALT\tallele\ttype\tstart\tref_len\talt\tverdict\tby\n"
WORKED_TEXT = WORKED_HEADER + (b"2\tc1\t6\tCGTACGTACGTACGT\tA\t1\tcomplex\t6\t15\tA\toverlap\t1\n"
                               b"6\tc1\t3\tG\tGA\t1\tins\t4\t0\tA\toverlap\t1\n"
                               b"8\tc1\t22\tC\tCG\t1\tins\t23\t0\tG\toverlap\t7\n"
                               b"12\tc1\t0\tA\tC\t.\t.\t.\t.\t.\tmalformed\t0\n"
                               b"13\tcX\t1\tA\tC\t1\t.\t.\t.\t.\tunknown_contig\t0\n"
                               b"14\tc1\t1\tA\t<DEL>\t1\t.\t.\t.\t.\tunsupported\t0\n"
                               b"15\tc1\t1\tC\tA\t1\t.\t.\t.\t.\tref_mismatch\t0\n"
                               b"16\tc1\t2\tC\tA\t1\t.\t.\t.\t.\tfiltered\t0\n"
                               b"17\tc1\t2\tc\tC\t1\t.\t.\t.\t.\tno_change\t0\n")


def test_the_worked_case():
    r = M.apply(WORKED_VCF, WORKED_GENOME)
    assert [None if row["cls"] in M.CLASSES else (row["r"], row["s"], row["d"], row["x"]) for row in r.rows] == WORKED_FORMS
    assert [row["cls"] for row in r.rows] == WORKED_VERDICTS[0] and [row["by"] for row in r.rows] == WORKED_BY
    assert r.fasta == WORKED_FASTA[0] and [o.tolist() for o in r.origins] == WORKED_ORIGINS and r.per_record == [(24, 18, 9), (0, 0, 0), (4, 4, 1)]
    assert M.TEXT_HEADER == WORKED_HEADER and r.text == WORKED_TEXT and len(WORKED_TEXT) == 404 and r.report == WORKED_REPORT
    assert (r.inserted, r.deleted, r.substituted, r.longest_cluster, r.types) == (6, 12, 5, 6, [3, 4, 1, 2])
    assert r.bases_out == r.bases_in + r.inserted - r.deleted == 22 and len(M.flat(r)) == 23
    everything = M.apply(WORKED_VCF, WORKED_GENOME, lines=1)
    assert [l.split(b"\t")[0] for l in everything.text.split(b"\n")[1:-1]] == [b"%d" % k for k in range(1, 20)]
    assert all(l in everything.text for l in WORKED_TEXT.split(b"\n")) and b"\n18\tc1\t23\tG\tA,GCC\t1\tsnv\t23\t1\tA\tapplied\t0\n" in everything.text
    assert M.flat(everything)[:-1] == M.flat(r)[:-1]
    # the haplotypes of the first sample; the second sample is 0|0 all through
    for h in (1, 2):
        x = M.apply(WORKED_VCF, WORKED_GENOME, haplotype=h, lines=1)
        assert [row["cls"] for row in x.rows] == WORKED_VERDICTS[h] and x.fasta == WORKED_FASTA[h]
    assert b"\n18\tc1\t23\tG\tA,GCC\t2\tins\t24\t0\tCC\tapplied\t0\n" in x.text and b"\n11\tc1\t19\tGT\tG\t1\tdel\t20\t1\t.\tapplied\t0\n" in x.text
    one = M.apply(WORKED_VCF, WORKED_GENOME, haplotype=1, lines=1)
    assert b"\n10\tc1\t21\tA\tC\t0\t.\t.\t.\t.\tref_allele\t0\n" in one.text and b"\n11\tc1\t19\tGT\tG\t.\t.\t.\t.\t.\tno_call\t0\n" in one.text
    other = M.apply(WORKED_VCF, WORKED_GENOME, haplotype=2, sample=1)
    assert other.ref_allele == 17 and other.applied == 0 and other.fasta == b">c1\nACGTACGTACGTACGTACGTACGT\n>c2\n>c3\nTTGA\n"
    assert M.sample_column(WORKED_VCF, "NA2") == 1 and M.sample_column(WORKED_VCF, "NA3") is None and M.sample_column(b"c1\t1\n", "NA1") is None
    with pytest.raises(ValueError, match="no data line has a sample column 2"):
        M.apply(WORKED_VCF, WORKED_GENOME, haplotype=1, sample=2)
    assert M.apply(HEAD, WORKED_GENOME, haplotype=1, sample=2).lines == 0


def test_the_greedy_rule_lets_a_loser_block_nothing():
    # [0, 10), [5, 20), [15, 18): the first and the third
    assert M.greedy([(0, 0, 10, 1), (0, 5, 15, 2), (0, 15, 3, 3)]) == ({1: (True, 0), 2: (False, 1), 3: (True, 0)}, 3)
    # end starts again with every record; the line number breaks ties among spans; an insertion goes in front of a span of its site
    assert M.greedy([(1, 0, 1, 1), (0, 0, 9, 2), (0, 0, 2, 3), (0, 0, 0, 4)])[0] == {4: (True, 0), 2: (True, 0), 3: (False, 2), 1: (True, 0)}
    assert M.greedy([])[1] == 0 and M.greedy([(0, 7, 0, 1)])[1] == 1


GENOTYPES = [("0|1", 0, 1), ("1|0", 1, 0), ("1/2", 1, 2), ("2|1", 2, 1), ("1", 1, 1), (".", None, None), ("./1", None, 1), ("0/0", 0, 0), ("01|002", 1, 2),
             ("1|2|1", "malformed", "malformed"), ("1|", "malformed", "malformed"), ("|1", "malformed", "malformed"), ("", "malformed", "malformed"),
             ("1|x", "malformed", "malformed"), ("3|1", "malformed", 1), ("1|3", 1, "malformed"), ("99999999999999999999|.", "malformed", None),
             ("1:7", 1, 1), ("1|2:7:x", 1, 2), ("-1", "malformed", "malformed"), ("1//2", "malformed", "malformed")]


def test_genotypes():
    genome = [("c", b"ACGT")]
    for gt, *want in GENOTYPES:
        for h in (1, 2):
            text = vcf([("c", 2, "C", "G,T", gt)])
            row = M.apply(text, genome, haplotype=h).rows[0]
            w = want[h - 1]
            assert (row["cls"], row["allele"]) == (("malformed", None) if w == "malformed" else ("no_call", None) if w is None else
                                                   ("ref_allele", 0) if w == 0 else ("applied", w)), (gt, h)
            assert row["cls"] != "applied" or row["x"] == b"GT"[w - 1:w]
    # GT must lead FORMAT
    for fmt, cls in (("GT", "applied"), ("GT:DP", "applied"), ("DP:GT", "malformed"), ("GTX", "malformed"), ("G", "malformed"), ("", "malformed")):
        assert M.apply(vcf([("c", 2, "C", "G", "1|1", ".", fmt)]), genome, haplotype=1).rows[0]["cls"] == cls, fmt
    # only the chosen allele has to be supported; an empty allele is malformed under every haplotype
    assert [M.apply(vcf([("c", 2, "C", "G,<X>", "1|2")]), genome, haplotype=h).rows[0]["cls"] for h in (0, 1, 2)] == ["applied", "applied", "unsupported"]
    for alt in ("G,", ",G", "G,,T", ","):
        assert [M.apply(vcf([("c", 2, "C", alt)]), genome, haplotype=h).rows[0]["cls"] for h in (0, 1)] == ["malformed"] * 2, alt
    # a line without the sample column beside one that has it
    text = vcf([("c", 2, "C", "G")]) + b"c\t3\t.\tG\tA\n" + b"c\t3\t.\tG\tA\t.\t.\t.\tGT\n"
    assert [row["cls"] for row in M.apply(text, genome, haplotype=1).rows] == ["applied", "malformed", "malformed"]
    assert [row["cls"] for row in M.apply(text, genome).rows] == ["applied", "applied", "overlap"]


# ---------------------------------------------------------------- properties
def random_case(rng, letters=b"ACGT", n_records=2, n_lines=25):
    genome = [("r%d" % k, bytes(rng.choice(letters) for _ in range(rng.randrange(1, 40)))) for k in range(n_records)]
    rows = []
    for _ in range(n_lines):
        name, seq = rng.choice(genome)
        pos = rng.randrange(1, len(seq) + 2)
        ref = seq[pos - 1:pos - 1 + rng.choice([1, 1, 1, 2, 3, 6])] or b"A"
        if rng.random() < 0.1:
            ref = ref.lower()
        alts = []
        for _ in range(rng.choice([1, 1, 2, 3])):
            kind = rng.random()
            alt = bytes(rng.choice(letters) for _ in range(rng.choice([1, 1, 2, 4])))
            if kind < 0.4:
                alt = ref[:1] + alt                      # an insertion or a substitution behind the padding base
            elif kind < 0.6:
                alt = ref[:1]                            # a deletion (or no change)
            alts.append(alt)
        gt = rng.choice(["0|1", "1|0", "1|1", "1|2", "2|1", ".|1", "1", "2|3", "0/0"])
        rows.append((name if rng.random() < 0.95 else "zz", pos, ref.decode(), b",".join(alts).decode(), gt, rng.choice([".", ".", "PASS", "q"])))
    return genome, vcf(rows)


def splice(seq, rows, r):
    """the rows the model marked applied, as Python slices from the right: at one start the span first, then the insertion in front"""
    for row in sorted((row for row in rows if row["cls"] == "applied" and row["r"] == r), key=lambda row: (row["s"], row["d"] > 0), reverse=True):
        seq = seq[:row["s"]] + row["x"] + seq[row["s"] + row["d"]:]
    return seq


@pytest.mark.parametrize("haplotype", [0, 1, 2])
@pytest.mark.parametrize("letters", [b"AC", b"ACGT"])
def test_the_fasta_is_a_naive_splice_and_the_origin_map_points_home(haplotype, letters):
    rng = random.Random(haplotype * 7 + len(letters))
    seen = collections_counter()
    for _ in range(60):
        genome, text = random_case(rng, letters)
        res = M.apply(text, genome, haplotype=haplotype, line_width=rng.choice([0, 7, 60]))
        seen.update(row["cls"] for row in res.rows)
        assert res.bases_out == res.bases_in + res.inserted - res.deleted and res.lines == len(res.rows) == sum(M.flat(res)[1:11])
        at = 0
        for r, (name, seq) in enumerate(genome):
            want = splice(seq, res.rows, r)
            head = b">" + name.encode() + b"\n"
            assert res.fasta[at:at + len(head)] == head
            body = res.fasta[at + len(head):].split(b">")[0]
            assert body.replace(b"\n", b"") == want
            at += len(head) + len(body)
            origin = res.origins[r].tolist()
            assert len(origin) == len(want) == res.per_record[r][1]
            inside = set()
            for row in res.rows:
                if row["cls"] == "applied" and row["r"] == r:
                    inside.update(range(row["s"], row["s"] + min(row["d"], len(row["x"]))))
            kept = [(i, o) for i, o in enumerate(origin) if o >= 0 and o not in inside]
            assert all(want[i] == seq[o] for i, o in kept) and [o for _, o in kept] == sorted(o for _, o in kept)
            gone = sum(row["d"] for row in res.rows if row["cls"] == "applied" and row["r"] == r)
            assert len(kept) == len(seq) - gone
        assert at == len(res.fasta)
    assert seen["applied"] > 100 and seen["overlap"] > 50 and seen["ref_mismatch"] and seen["filtered"] and seen["no_change"] and seen["unknown_contig"]


def collections_counter():
    import collections
    return collections.Counter()


@pytest.mark.parametrize("kw", OPTION_SETS, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "defaults")
def test_a_mutate_models_vcf_applied_is_its_fasta(kw):
    genome = four_records()
    m = G.mutate(genome, **kw)
    r = M.apply(m.vcf, genome, line_width=dict(G.DEFAULTS, **kw)["line_width"])
    assert r.fasta == m.fasta and r.applied == r.lines == m.variants and r.longest_cluster <= 1
    assert all(np.array_equal(a, b) for a, b in zip(r.origins, m.origins)) and len(r.origins) == len(m.origins)
    assert (r.inserted, r.deleted, r.substituted, r.types) == (m.inserted, m.deleted, m.substituted, list(m.types) + [0])
    assert r.per_record == m.per_record


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_calls_and_the_library_has_them():
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        h = f.read()
    assert re.search(r"int pbsim_vcf_apply\(pbsim_ctx \*ctx, const pbsim_errors_ref \*refs, int n_refs, const char \*const \*ref_names, const void \*vcf, "
                     r"int64_t n_vcf,\s*const pbsim_apply_opts \*opts, const pbsim_apply_sink \*sink, pbsim_apply_result \*result\);", h)
    assert re.search(r"int64_t pbsim_apply_report\(const pbsim_apply_result \*result, char \*buf, int64_t cap\);", h)
    assert re.search(r"int32_t pbsim_apply_sample\(const void \*vcf, int64_t n_vcf, const char \*name\);", h)
    opts = re.search(r"typedef struct pbsim_apply_opts \{(.*?)\} pbsim_apply_opts;", h, re.S).group(1)
    assert re.findall(r"^\s*(\w+ \w+);", opts, re.M) == ["int32_t haplotype", "int32_t sample", "int32_t lines", "int32_t line_width", "int64_t piece_bytes"]
    assert [n for n, _ in P.ApplyOpts._fields_] == ["haplotype", "sample", "lines", "line_width", "piece_bytes"] and C.sizeof(P.ApplyOpts) == 24
    body = re.search(r"typedef struct pbsim_apply_result \{(.*?)\} pbsim_apply_result;", h, re.S).group(1)
    declared = []
    for names in re.findall(r"int64_t ([\w\[\], ]+);", body):
        declared += [n.strip() for n in names.split(",")]
    assert declared == [n + "[4]" if n == "types" else n for n in M.FIELDS] == [n + "[4]" if n == "types" else n for n, _ in P.ApplyResult._fields_]
    assert C.sizeof(P.ApplyResult) == 8 * 23 == 8 * len(M.REPORT_NAMES) and P.APPLY_TYPES == M.REPORT_NAMES[11:15]
    assert sorted(P.APPLY_SCALARS + ["types"]) == sorted(M.FIELDS)
    sink = re.search(r"typedef struct pbsim_apply_sink \{(.*?)\} pbsim_apply_sink;", h, re.S).group(1)
    assert re.findall(r"\(\*(\w+)\)", sink) == ["on_fasta", "on_text", "on_record", "on_origin"] == [n for n, _ in P.ApplySink._fields_[1:]]
    bound = [name for name, _, _ in P.API]
    assert "pbsim_vcf_apply" in bound and "pbsim_apply_report" in bound and "pbsim_apply_sample" in bound
    assert callable(getattr(P.Context, "apply_vcf")) and callable(P.apply_report) and P.APPLY_LINES == {"discordant": 0, "all": 1}
    lib = P.load()
    assert hasattr(lib, "pbsim_vcf_apply") and hasattr(lib, "pbsim_apply_report") and hasattr(lib, "pbsim_apply_sample")


def as_dict(values):
    return dict(zip(M.FIELDS, values))


def random_numbers(rng):
    pick = lambda: rng.choice([0, 0, 1, 10 ** 12, rng.randrange(2 ** 40)])
    return [[pick() for _ in range(4)] if name == "types" else pick() for name in M.FIELDS]


ZERO_REPORT = WORKED_REPORT.split(b"\n")[0] + b"\nA" + b"\t0" * 23 + b"\n"


def test_report_and_sample_of_the_library_are_the_models_without_a_device():
    r = M.apply(WORKED_VCF, WORKED_GENOME)
    assert P.apply_report(as_dict([getattr(r, k) for k in M.FIELDS])) == WORKED_REPORT
    assert P.apply_report({}) == ZERO_REPORT == M.report([[0] * 4 if k == "types" else 0 for k in M.FIELDS])
    rng = random.Random(61)
    for _ in range(30):
        x = random_numbers(rng)
        assert P.apply_report(as_dict(x)) == M.report(x)
    assert P.apply_report(dict(types=dict(snv=1, ins=2, complex=4, **{"del": 3}))).split(b"\n")[1].split(b"\t")[12:16] == [b"1", b"2", b"3", b"4"]
    assert P.load().pbsim_apply_report(None, None, 0) == -1
    with pytest.raises(ValueError, match="types has 3 values"):
        P.apply_report(dict(types=[0] * 3))
    for text in (WORKED_VCF, WORKED_VCF.replace(b"\n", b"\r\n"), HEAD[:-1], b"", b"#CHROM", b"c1\t1\n", b"##x\n#CHROMOSOME\tP\tI\tR\tA\tQ\tF\tI\tF\tNA2\n" + HEAD):
        for name in ("NA1", "NA2", "NA", "NA22", "FORMAT", ""):
            want = M.sample_column(text, name)
            assert P.apply_sample(text, name) == (-1 if want is None else want), (text[:30], name)


# ---------------------------------------------------------------- the option mirror and the command line
GOOD = ["--apply-vcf", "in.vcf", "--apply-genome", "g.fa", "--apply-out", "out.fa"]
TAKES = ("--apply-vcf takes --apply-genome, --apply-out, --apply-ref-names, --apply-haplotype, --apply-sample, --apply-report, --apply-lines, "
         "--apply-line-width, --apply-origin and --device")
REFUSED = [
    (GOOD + ["--depth", "3"], "(--depth): " + TAKES),
    (GOOD + ["--genome", "x"], "(--genome): " + TAKES),
    (GOOD + ["--compare-out", "x"], "(--compare-out): " + TAKES),
    (GOOD + ["--mutate-genome", "x"], "(--apply-vcf): --mutate-genome takes"),
    (GOOD + ["--compare-vcf", "x"], "(--apply-vcf): --compare-vcf takes"),
    (GOOD + ["--call-bam", "x"], "(--apply-vcf): --call-bam takes"),
    (["--apply-genome", "g", "--apply-vcf"], "needs a value"),
    (["--apply-vcf", "v", "--apply-out", "o"], "--apply-vcf needs --apply-genome FASTA"),
    (["--apply-vcf", "v", "--apply-genome", "g"], "--apply-vcf needs --apply-out FASTA"),
    (GOOD + ["--apply-lines", "some"], "(apply-lines: some): discordant or all."),
    (GOOD + ["--apply-haplotype", "3"], "(apply-haplotype: 3): 0 (the first ALT of every line), 1 or 2."),
    (GOOD + ["--apply-haplotype", "-1"], "(apply-haplotype: -1): 0 (the first ALT of every line), 1 or 2."),
    (GOOD + ["--apply-haplotype", "x"], "(apply-haplotype: x)"),
    (GOOD + ["--apply-sample", ""], "(apply-sample): a 0-based sample column or a sample's name."),
    (GOOD + ["--apply-line-width", "1048577"], "(apply-line-width: 1048577): a whole number, 0 .. 1048576"),
    (GOOD + ["--apply-line-width", "1e3"], "(apply-line-width: 1e3): a whole number"),
    (GOOD + ["--apply-ref-names", "a,,b"], "(apply-ref-names): an empty name."),
    (GOOD + ["--devices", "0,1"], "--apply-vcf runs on one GPU"),
    (GOOD + ["--processes", "2"], "--apply-vcf runs on one GPU"),
]
OTHER_MODES = ("--mutate-genome", "--compare-vcf", "--call-bam")


def test_option_mirror_accepts_and_rejects():
    assert A.apply_vcf(GOOD) == dict(vcf="in.vcf", genome="g.fa", out="out.fa", ref_names=None, haplotype=0, sample=0, report=None, lines="discordant",
                                     line_width=60, origin=None)
    got = A.apply_vcf(["--apply-out", "o", "--apply-sample", "NA12878", "--device", "1", "--apply-genome", "g", "--apply-lines", "all", "--apply-haplotype",
                       "2", "--apply-ref-names", "a,b", "--apply-report", "r", "--apply-origin", "m", "--apply-line-width", "0", "--apply-vcf", "v"])
    assert got == dict(vcf="v", genome="g", out="o", ref_names=["a", "b"], haplotype=2, sample="NA12878", report="r", lines="all", line_width=0, origin="m")
    assert A.apply_vcf(GOOD + ["--apply-sample", "2"])["sample"] == 2 and A.apply_vcf(GOOD + ["--apply-sample", "2147483648"])["sample"] == "2147483648"
    for argv, message in REFUSED + [(["--apply-genome", "g"], "--apply-vcf VCF: name the variants")]:
        if any(m in argv for m in OTHER_MODES):
            continue                                # (the binary hands that line to the other stage's mode, which refuses it)
        with pytest.raises(ValueError) as e:
            A.apply_vcf(argv)
        assert message in str(e.value), argv


def test_cli_refuses_from_the_command_line_alone(tmp_path):
    """the same refusals by the binary, with the mirror's words, before a device or a file is touched"""
    import pbsim3_amd.build as b
    b.build()
    for argv, message in REFUSED:
        r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and r.stdout == "" and message in r.stderr, (argv, r.stderr[-500:])
    r = subprocess.run([CLI] + GOOD + ["--apply-report", "o.tsv", "--apply-origin", "o.bin"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "Cannot open file: in.vcf" in r.stderr
    assert os.listdir(tmp_path) == []
    r = subprocess.run([CLI], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert "--apply-vcf VCF --apply-genome FASTA --apply-out FASTA" in r.stderr + r.stdout


# ---------------------------------------------------------------- the checks in front of any device work
REFUSED_OPTS = [(dict(haplotype=3), "haplotype must be 0"), (dict(haplotype=-1), "haplotype must be 0"), (dict(sample=-1), "sample must be 0 .. 2147483647"),
                (dict(lines=2), "lines must be 0"), (dict(lines=-1), "lines must be 0"), (dict(line_width=-1), "line_width must be 0 .. 1048576"),
                (dict(line_width=1048577), "line_width must be 0 .. 1048576"), (dict(piece_bytes=-1), "piece_bytes must not be negative")]


def test_bad_arguments_fail_before_device_work():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), -1) as c:
        for kw, word in REFUSED_OPTS:
            with pytest.raises(P.PbsimError, match="pbsim_vcf_apply: " + word):
                c.apply_vcf(WORKED_VCF, WORKED_GENOME, **kw)
        with pytest.raises(P.PbsimError, match="pbsim_vcf_apply: bad argument"):
            c.apply_vcf(WORKED_VCF, [])
        with pytest.raises(P.PbsimError, match=r"pbsim_vcf_apply: the genome holds two records named \"c1\" \(records 0 and 3\)"):
            c.apply_vcf(WORKED_VCF, WORKED_GENOME + [("c1", b"AC")])
        with pytest.raises(P.PbsimError, match=r"pbsim_vcf_apply: ref_names: two genome records are named \"a\" \(records 0 and 1\)"):
            c.apply_vcf(WORKED_VCF, WORKED_GENOME, ref_names=["a", "a", "b"])
        with pytest.raises(P.PbsimError, match="pbsim_vcf_apply: ref_names: genome record 1 has no name"):
            c.apply_vcf(WORKED_VCF, WORKED_GENOME, ref_names=["a", "", "b"])
        with pytest.raises(ValueError, match="one entry per genome record"):
            c.apply_vcf(WORKED_VCF, WORKED_GENOME, ref_names=["a", "b"])
        with pytest.raises(ValueError, match="names no sample"):
            c.apply_vcf(WORKED_VCF, WORKED_GENOME, haplotype=1, sample="NA3")
        for kw in (dict(haplotype=2 ** 31), dict(lines=2 ** 40), dict(sample=2 ** 31), dict(line_width=-2 ** 31 - 1)):
            with pytest.raises(ValueError, match="does not fit its 32-bit field"):
                c.apply_vcf(WORKED_VCF, WORKED_GENOME, **kw)
        # a missing text with a length, through the library itself
        refs = (P.ErrorsRef * 1)(P.ErrorsRef(b"c1", None, 0))
        res = P.ApplyResult()
        assert c.lib.pbsim_vcf_apply(c.h, refs, 1, None, None, 5, None, None, C.byref(res)) == 0
        assert b"pbsim_vcf_apply: bad argument" in c.lib.pbsim_last_error()
        # good arguments reach the device check: a tables-only context refuses as pbsim_inflate_buffer does, and stays usable
        for kw in (dict(), dict(text=False, fasta=False), dict(lines="all", haplotype=2, sample="NA2", piece_bytes=7, ref_names=["c1", "c2", "c3"]),
                   dict(origin=True, line_width=0)):
            with pytest.raises(P.PbsimError, match="no HIP device"):
                c.apply_vcf(WORKED_VCF, WORKED_GENOME, **kw)
        with pytest.raises(P.PbsimError, match="no HIP device"):
            c.apply_vcf(b"", WORKED_GENOME)


# ---------------------------------------------------------------- the host's decisions under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("asan") / "vcf_apply_rule_driver")
    p = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(harness.ROOT, "tests", "asan", "vcf_apply_rule_driver.cpp"), os.path.join(csrc, "vcf_apply_rule.cpp"),
                        "-o", exe], capture_output=True, text=True)
    if p.returncode != 0 and "sanitize" in p.stderr:
        pytest.skip("no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def drive(exe, *argv):
    p = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, timeout=60)
    assert p.returncode == 0, (argv, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout


def test_rule_code_under_asan(driver, tmp_path):
    assert drive(driver, "opts", "-") == b"opts 0 0 0 60 8388608\n"
    assert drive(driver, "opts", 2, 2147483647, 1, 1048576, 7) == b"opts 2 2147483647 1 1048576 7\n"
    for bad, word in (((3, 0, 0, 60, 0), b"haplotype"), ((-1, 0, 0, 60, 0), b"haplotype"), ((0, -1, 0, 60, 0), b"sample"), ((0, 0, 2, 60, 0), b"lines"),
                      ((0, 0, 0, -1, 0), b"line_width"), ((0, 0, 0, 1048577, 0), b"line_width"), ((0, 0, 0, 60, -1), b"piece_bytes")):
        assert drive(driver, "opts", *bad).startswith(b"opts refused: " + word), bad
    for k, text in enumerate((WORKED_VCF, WORKED_VCF.replace(b"\n", b"\r\n"), HEAD[:-1], HEAD[:-1] + b"\r", b"", b"#CHROM", b"#CHROM\t", b"\n\n#CHRO",
                              b"#CHROM\tP\tI\tR\tA\tQ\tF\tI\tF\t\tNA1\t")):
        (tmp_path / ("%d.vcf" % k)).write_bytes(text)
        for name in ("NA1", "NA2", "NA", "FORMAT"):
            want = M.sample_column(text, name)
            assert drive(driver, "sample", tmp_path / ("%d.vcf" % k), name) == b"sample %d\n" % (-1 if want is None else want), (k, name)
    assert drive(driver, "report", *M.flat(M.apply(WORKED_VCF, WORKED_GENOME))) == WORKED_REPORT
    assert drive(driver, "report", *([0] * 23)) == ZERO_REPORT
    rng = random.Random(62)
    for _ in range(5):
        x = random_numbers(rng)
        assert drive(driver, "report", *M.flat(as_dict(x))) == M.report(x)
