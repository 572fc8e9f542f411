"""The rule of `pbsim --apply-vcf` (pbsim_vcf_apply) in plain Python: the lines of a VCF applied to a genome, per haplotype, the
result written as FASTA with an origin map.  This file is the contract; the product's kernels (pbsim3_amd/csrc/vcf_apply.hip) must
give the same numbers, report, FASTA, annotated text and origin maps, byte for byte.  No code is shared with the product.

    apply(vcf, genome, ref_names=None, haplotype=0, sample=0, lines=0, line_width=60) -> Result
    form_of(pos, ref, allele) -> (s, d, X)              the form of upper-cased REF and allele that differ
    greedy(forms) -> per form (applied, by)             the order and the collisions, one line after the other
    sample_column(vcf, name) -> the 0-based sample column of `name` in the #CHROM line, or None

1. Inputs.  A VCF text and a genome, a list of (name, sequence lines), prepared as tests/errors_model.py prepares it.  ref_names as
   tests/compare_model.py has them.
2. Lines and columns.  Exactly compare_model's: a line ends at \\n, a \\r in front of it is dropped, the last line needs no \\n;
   empty lines and lines that begin with # are not data lines; data lines are numbered from 1; columns are separated by tabs.
   Column 9 is FORMAT, column 10 + sample the sample.
3. The allele.  ALT is split at commas into alleles 1 .. k.  With haplotype 0 the allele is 1.  With haplotype h = 1 or 2 FORMAT
   must be `GT` or begin with `GT:`; the genotype is the sample column up to its first `:`, one or two fields of `.` or decimal
   digits separated by one `/` or `|`; a genotype of one field serves both haplotypes; the allele is the value of field h.
4. Classes.  The first that applies takes the line out:
   malformed       compare_model's conditions, or an empty allele between commas; with h != 0 also: the sample column is missing,
                   FORMAT is not as above, the genotype is not of that shape, the allele number is above k.
   unknown_contig  as compare_model.
   no_call         the field is `.`.
   ref_allele      the field's value is 0.
   unsupported     REF or the chosen allele, upper-cased, holds a byte outside ACGTN; the line's other alleles are not looked at.
   ref_mismatch    as compare_model.
   filtered        FILTER is present and neither `.` nor `PASS`.
   no_change       REF equals the allele (both upper-cased).
5. The form (r, s, d, X): s = POS - 1; while REF and the allele both have bytes and their first bytes agree, both lose the first
   byte and s grows by 1; then, while both have bytes and their last bytes agree, both lose the last byte.  d is what is left of
   REF, X what is left of the allele, upper-cased.  No left move.  Types as compare_model.  s = l_ref with d = 0 is legal.
6. Order and collisions.  The lines that are left are taken in order of (r, s, insertions before spans, line number), with end = 0
   at the start of each record: an insertion (d = 0) is applied where s >= end and no insertion at this (r, s) has been applied; a
   span (d > 0) is applied where s >= end, and then end = s + d; every other line is `overlap`, its `by` the number of the applied
   line it ran into: the span that owns end, or the earlier insertion.  A line that lost blocks nothing.
7. What comes out.  Per record, for p = 0 .. l_ref: the X of the insertion applied at p; then, for p < l_ref, the X of the span
   applied at p, or nothing where p lies inside an applied span behind its start, or the prepared genome byte.  The FASTA layout is
   mutate_model's.
8. Origin map, one int32 per written base: p for a kept base; s + i for byte i < min(d, |X|) of a span's X; -1 - (s + d - 1) for
   the rest of a span's X; -1 - (s - 1) for the bytes of an insertion at s >= 1; -2^31 for those of an insertion at s = 0.
9. Numbers: lines, the eight classes, overlap, applied; types[snv, ins, del, complex] of the applied lines; bases_in, bases_out,
   inserted (sum of |X| - min(d, |X|)), deleted (sum of d - min), substituted (sum of min), all over the applied lines;
   longest_cluster: the lines of the longest run of sorted lines in which every line but the first begins in front of the largest
   s + d of the lines before it in the run, or is an insertion at the (r, s) of an insertion just before it (0: no line is left);
   fasta_bytes; text_bytes under `lines`.  bases_out = bases_in + inserted - deleted.
10. The annotated text: the header line, then one line per data line in file order: the line's number, CHROM, POS, REF, ALT as in
   the file (`.` for a column the line lacks or that is empty), the allele's number (`.` for a malformed line and a no_call), the
   type, s + 1, d, X (`.` where X is empty; all four `.` for a line a class took out), `applied`, `overlap` or the class, `by` (0
   except for overlap).  lines 0 leaves out `applied`; lines 1 writes every data line.
11. With h != 0, a file that has data lines none of which has the sample column is refused."""
import collections

import numpy as np

from compare_model import POS_MAX, TYPES, UPPER, data_lines, type_of
from errors_model import prepare_genome
from mutate_model import wrap

CLASSES = ["malformed", "unknown_contig", "no_call", "ref_allele", "unsupported", "ref_mismatch", "filtered", "no_change"]
FIELDS = ["lines"] + CLASSES + ["overlap", "applied", "types", "bases_in", "bases_out", "inserted", "deleted", "substituted", "longest_cluster",
                                "fasta_bytes", "text_bytes"]
REPORT_NAMES = ["lines"] + CLASSES + ["overlap", "applied"] + TYPES + ["bases_in", "bases_out", "inserted", "deleted", "substituted", "longest_cluster",
                                                                      "fasta_bytes", "text_bytes"]
TEXT_HEADER = b"#line\tCHROM\tPOS\tREF\tALT\tallele\ttype\tstart\tref_len\talt\tverdict\tby\n"
ALLELE_MAX = 2 ** 31 - 1
INS_AT_START = -2 ** 31

Result = collections.namedtuple("Result", " ".join(FIELDS) + " fasta text per_record origins report rows")


def form_of(pos, ref, allele):
    s = pos - 1
    while ref and allele and ref[0] == allele[0]:
        ref, allele, s = ref[1:], allele[1:], s + 1
    while ref and allele and ref[-1] == allele[-1]:
        ref, allele = ref[:-1], allele[:-1]
    return s, len(ref), allele


def genotype_field(gt, h):
    """the field of haplotype h of a genotype: b".", digits, or None where the genotype is not of the shape"""
    fields = gt.replace(b"|", b"/").split(b"/")
    if len(fields) > 2 or any(f != b"." and not (f and all(48 <= c <= 57 for c in f)) for f in fields):
        return None
    return fields[h - 1] if len(fields) == 2 else fields[0]


def sample_column(vcf, name):
    name = name.encode() if isinstance(name, str) else bytes(name)
    for line in bytes(vcf).split(b"\n"):
        if line.startswith(b"#CHROM"):
            cols = (line[:-1] if line.endswith(b"\r") else line).split(b"\t")[9:]
            return cols.index(name) if name in cols else None
    return None


def parse(vcf, names, seqs, haplotype, sample):
    """per data line a dict: shown (CHROM, POS, REF, ALT for the text), cls (None: left), allele (None: `.`), r, s, d, x;
    and whether any data line has the sample column"""
    rows, any_sample = [], False
    for line in data_lines(vcf):
        f = line.split(b"\t")
        row = dict(shown=[f[k] if k < len(f) and f[k] else b"." for k in (0, 1, 3, 4)], cls=None, allele=None, r=0, s=0, d=0, x=b"", by=0)
        rows.append(row)
        any_sample = any_sample or len(f) > 9 + sample
        pos = 0
        if len(f) >= 5 and f[1] and all(48 <= c <= 57 for c in f[1]):
            pos = int(f[1]) if len(f[1].lstrip(b"0")) <= 10 else POS_MAX + 1
        if len(f) < 5 or not f[0] or not f[3] or not f[4] or not 1 <= pos <= POS_MAX:
            row["cls"] = "malformed"
            continue
        alleles = f[4].split(b",")
        if b"" in alleles:
            row["cls"] = "malformed"
            continue
        number = 1
        if haplotype:
            if len(f) <= 9 + sample or not (f[8] == b"GT" or f[8].startswith(b"GT:")):
                row["cls"] = "malformed"
                continue
            field = genotype_field(f[9 + sample].split(b":")[0], haplotype)
            if field is None:
                row["cls"] = "malformed"
                continue
            number = None if field == b"." else min(int(field), ALLELE_MAX)
            if number is not None and number > len(alleles):
                row["cls"] = "malformed"
                continue
        row["allele"] = number
        r = names.get(f[0])
        if r is None:
            row["cls"] = "unknown_contig"
            continue
        if number is None:
            row["cls"] = "no_call"
            continue
        if number == 0:
            row["cls"] = "ref_allele"
            continue
        ref, allele = f[3].translate(UPPER), alleles[number - 1].translate(UPPER)
        if ref.strip(b"ACGTN") or allele.strip(b"ACGTN"):
            row["cls"] = "unsupported"
            continue
        seq = seqs[r]
        if pos - 1 + len(ref) > len(seq) or seq[pos - 1:pos - 1 + len(ref)] != ref:
            row["cls"] = "ref_mismatch"
            continue
        if len(f) >= 7 and f[6] not in (b".", b"PASS"):
            row["cls"] = "filtered"
            continue
        if ref == allele:
            row["cls"] = "no_change"
            continue
        s, d, x = form_of(pos, ref, allele)
        row.update(r=r, s=s, d=d, x=x)
    return rows, any_sample


def greedy(forms):
    """forms: (r, s, d, number) of the lines that are left -> {number: (applied, by)} and the longest cluster"""
    out, longest, run = {}, 0, 0
    state = None                                          # (r, end, the span that owns end, (s, the insertion applied there))
    reach = (-1, 0)                                       # the largest (r, s + d) so far: what the clusters are cut by
    before = None
    for r, s, d, number in sorted(forms, key=lambda v: (v[0], v[1], v[2] > 0, v[3])):
        if state is None or state[0] != r:
            state = [r, 0, 0, (-1, 0)]
        chained = before is not None and d == 0 and before == (r, s, 0)
        run = run + 1 if (r, s) < reach or chained else 1
        longest = max(longest, run)
        reach, before = max(reach, (r, s + d)), (r, s, d)
        if s < state[1]:
            out[number] = (False, state[2])
        elif d == 0 and state[3][0] == s:
            out[number] = (False, state[3][1])
        else:
            out[number] = (True, 0)
            if d == 0:
                state[3] = (s, number)
            else:
                state[1], state[2] = s + d, number
    return out, longest


def report(values):
    flat = []
    for v in values:
        flat += [int(x) for x in v] if isinstance(v, (list, tuple)) else [int(v)]
    assert len(flat) == len(REPORT_NAMES)
    return ("#\t" + "\t".join(REPORT_NAMES) + "\nA\t" + "\t".join("%d" % v for v in flat) + "\n").encode()


def apply(vcf, genome, ref_names=None, haplotype=0, sample=0, lines=0, line_width=60):
    assert haplotype in (0, 1, 2) and sample >= 0 and lines in (0, 1) and 0 <= line_width <= 1048576
    prepared = prepare_genome(genome)                   # (refuses two equal names)
    own = [n.encode() if isinstance(n, str) else bytes(n) for n, _ in genome]
    seqs = [prepared[n][0].tobytes() for n in own]
    used = own if ref_names is None else [n.encode() if isinstance(n, str) else bytes(n) for n in ref_names]
    if len(used) != len(own) or b"" in used or len(set(used)) != len(used):
        raise ValueError("ref_names: one name per genome record, none empty, no two equal")
    rows, any_sample = parse(vcf, {n: r for r, n in enumerate(used)}, seqs, haplotype, sample)
    if haplotype and rows and not any_sample:
        raise ValueError("no data line has a sample column %d" % sample)
    verdicts, longest = greedy([(row["r"], row["s"], row["d"], k + 1) for k, row in enumerate(rows) if row["cls"] is None])
    n = dict.fromkeys(FIELDS, 0)
    n["types"] = [0, 0, 0, 0]
    n["lines"], n["longest_cluster"] = len(rows), longest
    ins_at, span_at = [{} for _ in seqs], [{} for _ in seqs]
    text = [TEXT_HEADER]
    for k, row in enumerate(rows):
        form_cols = b".\t.\t.\t."
        if row["cls"] is None:
            applied, row["by"] = verdicts[k + 1]
            row["cls"] = "applied" if applied else "overlap"
            s, d, x = row["s"], row["d"], row["x"]
            form_cols = b"%s\t%d\t%d\t%s" % (TYPES[type_of(d, x)].encode(), s + 1, d, x or b".")
            if applied:
                (span_at if d else ins_at)[row["r"]][s] = row
                both = min(d, len(x))
                n["types"][type_of(d, x)] += 1
                n["inserted"], n["deleted"], n["substituted"] = n["inserted"] + len(x) - both, n["deleted"] + d - both, n["substituted"] + both
        n[row["cls"]] += 1
        if lines == 1 or row["cls"] != "applied":
            allele = b"." if row["allele"] is None else b"%d" % row["allele"]
            text.append(b"%d\t%s\t%s\t%s\t%s\t%d\n" % (k + 1, b"\t".join(row["shown"]), allele, form_cols, row["cls"].encode(), row["by"]))
    fasta, per_record, origins = [], [], []
    for r, seq in enumerate(seqs):
        bases, origin, end = [], [], 0
        for p in range(len(seq) + 1):
            row = ins_at[r].get(p)
            if row:
                bases.append(row["x"])
                origin += [-p if p else INS_AT_START] * len(row["x"])
            if p == len(seq):
                break
            row = span_at[r].get(p)
            if row:
                d, x = row["d"], row["x"]
                bases.append(x)
                origin += [p + i if i < d else -(p + d) for i in range(len(x))]
                end = p + d
            elif p >= end:
                bases.append(seq[p:p + 1])
                origin.append(p)
        bases = b"".join(bases)
        fasta.append(b">" + own[r] + b"\n" + wrap(bases, line_width))
        per_record.append((len(seq), len(bases), len(ins_at[r]) + len(span_at[r])))
        origins.append(np.array(origin, dtype=np.int64).astype(np.int32))
        n["bases_in"], n["bases_out"] = n["bases_in"] + len(seq), n["bases_out"] + len(bases)
    fasta, text = b"".join(fasta), b"".join(text)
    n["fasta_bytes"], n["text_bytes"] = len(fasta), len(text)
    assert n["bases_out"] == n["bases_in"] + n["inserted"] - n["deleted"]
    values = [n[k] for k in FIELDS]
    return Result(*values, fasta, text, per_record, origins, report(values), rows)


def flat(r):
    """the 23 numbers of a result in the order of pbsim_apply_result"""
    out = []
    for k in FIELDS:
        v = getattr(r, k) if not isinstance(r, dict) else r[k]
        out += [int(x) for x in v] if isinstance(v, (list, tuple)) else [int(v)]
    return out
