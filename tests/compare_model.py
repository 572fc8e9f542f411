"""The rule of `pbsim --compare-vcf` (pbsim_vcf_compare) in plain Python: a call set scored against the truth variants, both VCF
texts over one genome, with every indel moved to its leftmost placement first.  This file is the contract; the product's kernels
(pbsim3_amd/csrc/vcf_compare.hip) must give the same numbers, report and annotated text, byte for byte.  No code is shared with the
product.

    compare(truth, calls, genome, ref_names=None, lines=0, min_ms=0) -> Result
    form_of(pos, ref, alt, seq) -> (s, d, X, shift)     steps 1 .. 5 of the canonical form, for tests
    report(files, types, lengths, ms) -> the report text

1. Inputs.  Two VCF texts, truth and calls.  The genome is a list of (name, sequence lines), prepared as tests/errors_model.py
   prepares it: the line feeds dropped, a-z upper-cased, each record on its own; two equal names are refused.  ref_names (None: the
   genome's own names) gives per genome record the contig name the VCFs use for it; an empty name and two equal names are refused.
2. Lines.  A line ends at \\n; a \\r just in front of that \\n is dropped; the last line needs no \\n.  Empty lines and lines that
   begin with # are not data lines.  Data lines are numbered from 1 per file.  Columns are separated by tabs: CHROM, POS, ID, REF,
   ALT, QUAL, FILTER, INFO; FILTER is present where the line has seven columns, INFO where it has eight.
3. Classes.  The first that applies takes a data line out:
   malformed       fewer than five columns; an empty CHROM, REF or ALT; a POS that is not one or more digits 0-9 with a value 1 ..
                   2^31 - 1.
   unknown_contig  CHROM is not one of the names (compared byte by byte).
   unsupported     REF or ALT, a-z upper-cased, holds a byte outside ACGTN.
   ref_mismatch    REF runs past the record's end or differs from the prepared genome bytes at POS - 1 (REF upper-cased).
   filtered        FILTER is present and neither `.` nor `PASS`; in the calls also MS < min_ms, MS the value of the leading digits
                   (held to 2^31 - 1) behind the first `MS=` that begins INFO or follows a `;` in it; no MS, no INFO or no digit: 0.
   no_change       REF equals ALT (both upper-cased).
4. The form (r, s, d, X) of a line that is left: r the genome record; s = POS - 1; while REF and ALT both have bytes and their last
   bytes agree, both lose the last byte; while both have bytes and their first bytes agree, both lose the first byte and s grows by
   1; if exactly one of them is empty now, the other, Y, moves left: while s > 0 and the genome's byte at s - 1 equals Y's last
   byte, Y is rotated right by one and s falls by 1 (`shift` counts the steps; the walk stays inside the record).  d is the length
   of what is left of REF, X what is left of ALT, upper-cased.
5. Type: snv where d = 1 and |X| = 1; ins where d = 0; del where |X| = 0; else complex.
6. Duplicates.  Within one file a line whose form equals that of an earlier line of the file is `dup`; the others are compared.
7. Verdicts of the compared lines.  Truth: `found` where a compared call has an equal form, else `missed`.  Calls: `tp` where a
   compared truth line has an equal form; else `fp_site` where one has the same (r, s); else `fp`.  MATE is the number of the line
   with the equal form in the other file, else 0 (also for every line that is not compared).
8. Numbers.  files[truth, calls]: lines, the six classes, dup, compared, shifted (lines with shift > 0, dup ones included),
   longest_shift.  types[snv, ins, del, complex]: truth, found, calls, tp, fp (fp_site included), fp_site.  lengths[ins, del][bin]:
   truth, found, calls, tp, the bin by |X| of an ins and d of a del: 1, 2-5, 6-15, 16-49, 50+.  ms[min(MS, 63)]: tp, fp of the
   compared calls.  text_bytes: the annotated text's size under `lines`.
9. The report: `#` and the names of files[], `T` and `C` with the values; `P\\t<type>` per type and for `all` with the six numbers,
   recall_ppm = found * 1000000 // truth and precision_ppm = tp * 1000000 // calls (0 where the denominator is 0);
   `L\\t<ins|del>\\t<bin>` with the four numbers for the bins that are not all 0; `Q\\t<ms>` with tp, fp and the sums of tp and of fp
   over this bin and all higher ones, for the bins that are not empty.
10. The annotated text: the header line, then one line per data line, truth first, each file in order: T or C, the line's number,
   CHROM, POS, REF, ALT as in the file (`.` for a column the line lacks or that is empty), the type, s + 1, d, X (`.` where X is
   empty; all four `.` for a line a class took out), the verdict or the class, MATE.  lines 0 leaves out `found` and `tp`; lines 1
   writes every data line."""
import collections

from errors_model import prepare_genome

CLASSES = ["malformed", "unknown_contig", "unsupported", "ref_mismatch", "filtered", "no_change"]
FILE_NAMES = ["lines"] + CLASSES + ["dup", "compared", "shifted", "longest_shift"]
TYPES = ["snv", "ins", "del", "complex"]
TYPE_NAMES = ["truth", "found", "calls", "tp", "fp", "fp_site"]
BINS = ["1", "2-5", "6-15", "16-49", "50+"]
LENGTH_NAMES = ["truth", "found", "calls", "tp"]
MS_BINS = 64
POS_MAX = 2 ** 31 - 1
TEXT_HEADER = b"#file\tline\tCHROM\tPOS\tREF\tALT\ttype\tstart\tref_len\talt\tverdict\tmate\n"
UPPER = bytes(c - 32 if 97 <= c <= 122 else c for c in range(256))

Result = collections.namedtuple("Result", "files types lengths ms text_bytes text report rows")


def bin_of(n):
    return 0 if n <= 1 else 1 if n <= 5 else 2 if n <= 15 else 3 if n <= 49 else 4


def data_lines(text):
    pieces = bytes(text).split(b"\n")                   # (a text that ends with \n leaves one empty piece: no data line)
    out = [l[:-1] if k + 1 < len(pieces) and l.endswith(b"\r") else l for k, l in enumerate(pieces)]   # (the last has no \n behind it)
    return [l for l in out if l and not l.startswith(b"#")]


def ms_of(info):
    for item in info.split(b";"):
        if item.startswith(b"MS="):
            n = 0
            for c in item[3:]:
                if not 48 <= c <= 57:
                    break
                n = min(n * 10 + c - 48, POS_MAX)
            return n
    return 0


def form_of(pos, ref, alt, seq, suffix_first=True):
    """steps 1 .. 5 on upper-cased REF and ALT that differ; seq: the record's prepared bytes"""
    s = pos - 1
    for turn in ((0, 1) if suffix_first else (1, 0)):
        if turn == 0:
            while ref and alt and ref[-1] == alt[-1]:
                ref, alt = ref[:-1], alt[:-1]
        else:
            while ref and alt and ref[0] == alt[0]:
                ref, alt, s = ref[1:], alt[1:], s + 1
    shift = 0
    if bool(ref) != bool(alt):
        y = ref or alt
        n, k = len(y), len(y) - 1                         # k: where the rotated Y's last byte lies in the Y of step 3
        while s > 0 and seq[s - 1] == y[k]:
            s, shift, k = s - 1, shift + 1, (k - 1) % n
        y = y[k + 1:] + y[:k + 1]
        if ref:
            ref = y
        else:
            alt = y
    return s, len(ref), alt, shift


def type_of(d, x):
    return 0 if d == 1 and len(x) == 1 else 1 if d == 0 else 2 if not x else 3


def parse(text, is_calls, names, seqs, min_ms):
    """per data line a list: [cols for the text (CHROM, POS, REF, ALT), class or None, r, s, d, X, shift, ms]"""
    rows = []
    for line in data_lines(text):
        f = line.split(b"\t")
        shown = [f[k] if k < len(f) and f[k] else b"." for k in (0, 1, 3, 4)]
        row = [shown, None, 0, 0, 0, b"", 0, 0]
        rows.append(row)
        pos = 0
        if len(f) >= 5 and f[1] and all(48 <= c <= 57 for c in f[1]):
            pos = int(f[1]) if len(f[1].lstrip(b"0")) <= 10 else POS_MAX + 1
        if len(f) < 5 or not f[0] or not f[3] or not f[4] or not 1 <= pos <= POS_MAX:
            row[1] = "malformed"
            continue
        r = names.get(f[0])
        if r is None:
            row[1] = "unknown_contig"
            continue
        ref, alt = f[3].translate(UPPER), f[4].translate(UPPER)
        if ref.strip(b"ACGTN") or alt.strip(b"ACGTN"):
            row[1] = "unsupported"
            continue
        seq = seqs[r]
        if pos - 1 + len(ref) > len(seq) or seq[pos - 1:pos - 1 + len(ref)] != ref:
            row[1] = "ref_mismatch"
            continue
        ms = ms_of(f[7]) if len(f) >= 8 else 0
        row[7] = ms
        if (len(f) >= 7 and f[6] not in (b".", b"PASS")) or (is_calls and ms < min_ms):
            row[1] = "filtered"
            continue
        if ref == alt:
            row[1] = "no_change"
            continue
        s, d, x, shift = form_of(pos, ref, alt, seq)
        row[2:7] = [r, s, d, x, shift]
    return rows


def report(files, types, lengths, ms):
    out = ["#\t" + "\t".join(FILE_NAMES)]
    for tag, v in zip("TC", files):
        out.append(tag + "".join("\t%d" % x for x in v))
    ppm = lambda a, b: a * 1000000 // b if b else 0
    for name, v in zip(TYPES + ["all"], list(types) + [[sum(t[k] for t in types) for k in range(6)]]):
        out.append("P\t%s" % name + "".join("\t%d" % x for x in v) + "\t%d\t%d" % (ppm(v[1], v[0]), ppm(v[3], v[2])))
    for name, table in zip(("ins", "del"), lengths):
        for b, v in zip(BINS, table):
            if any(v):
                out.append("L\t%s\t%s" % (name, b) + "".join("\t%d" % x for x in v))
    for k in range(MS_BINS):
        if ms[k][0] or ms[k][1]:
            out.append("Q\t%d\t%d\t%d\t%d\t%d" % (k, ms[k][0], ms[k][1], sum(m[0] for m in ms[k:]), sum(m[1] for m in ms[k:])))
    return ("\n".join(out) + "\n").encode()


def compare(truth, calls, genome, ref_names=None, lines=0, min_ms=0):
    assert lines in (0, 1) and 0 <= min_ms <= POS_MAX
    prepared = prepare_genome(genome)                   # (refuses two equal names)
    own = [n.encode() if isinstance(n, str) else bytes(n) for n, _ in genome]
    seqs = [prepared[n][0].tobytes() for n in own]
    used = own if ref_names is None else [n.encode() if isinstance(n, str) else bytes(n) for n in ref_names]
    if len(used) != len(own) or b"" in used or len(set(used)) != len(used):
        raise ValueError("ref_names: one name per genome record, none empty, no two equal")
    names = {n: r for r, n in enumerate(used)}
    both = [parse(truth, False, names, seqs, min_ms), parse(calls, True, names, seqs, min_ms)]
    files = [[0] * len(FILE_NAMES) for _ in range(2)]
    first, sites = [{}, {}], set()                      # form -> the number of the file's first line with it; the truth's (r, s)
    for w, rows in enumerate(both):
        n = files[w]
        n[0] = len(rows)
        for k, row in enumerate(rows):
            if row[1]:
                n[1 + CLASSES.index(row[1])] += 1
                continue
            if row[6]:
                n[9], n[10] = n[9] + 1, max(n[10], row[6])
            form = tuple(row[2:6])
            if form in first[w]:
                row[1] = "dup"
                n[7] += 1
                continue
            first[w][form] = k + 1
            n[8] += 1
            if w == 0:
                sites.add(form[:2])
    types = [[0] * 6 for _ in TYPES]
    lengths = [[[0] * 4 for _ in BINS] for _ in range(2)]
    ms = [[0, 0] for _ in range(MS_BINS)]
    text = [TEXT_HEADER]
    for w, rows in enumerate(both):
        for k, row in enumerate(rows):
            shown, cls, r, s, d, x, _, support = row
            mate, form_cols = 0, b".\t.\t.\t."
            if cls is None or cls == "dup":
                t = type_of(d, x)
                form_cols = b"%s\t%d\t%d\t%s" % (TYPES[t].encode(), s + 1, d, x or b".")
            if cls is None:
                mate = first[1 - w].get((r, s, d, x), 0)
                cls = ("found" if mate else "missed") if w == 0 else "tp" if mate else "fp_site" if (r, s) in sites else "fp"
                n = types[t]
                n[2 * w] += 1
                n[2 * w + 1] += mate != 0
                if w == 1 and not mate:
                    n[4] += 1
                    n[5] += cls == "fp_site"
                if t in (1, 2):
                    cell = lengths[t - 1][bin_of(len(x) if t == 1 else d)]
                    cell[2 * w] += 1
                    cell[2 * w + 1] += mate != 0
                if w == 1:
                    ms[min(support, MS_BINS - 1)][0 if mate else 1] += 1
            row.append(cls)
            row.append(mate)
            if lines == 1 or cls not in ("found", "tp"):
                text.append(b"%s\t%d\t%s\t%s\t%s\t%d\n" % (b"TC"[w:w + 1], k + 1, b"\t".join(shown), form_cols, cls.encode(), mate))
    text = b"".join(text)
    return Result(files, types, lengths, ms, len(text), text, report(files, types, lengths, ms), both)


def flat(r):
    """the 215 numbers of a result in the order of pbsim_compare_result"""
    out = [x for v in r.files for x in v] + [x for v in r.types for x in v] + [x for t in r.lengths for v in t for x in v]
    return out + [x for v in r.ms for x in v] + [r.text_bytes]
