"""The rule of `pbsim --call-bam` (pbsim_bam_call) in plain Python and numpy: the differences between the genome and what the pile of
aligned reads of one or more BAM files spells, as VCFv4.2.  This file is the contract; the product's kernels
(pbsim3_amd/csrc/bam_call.hip) must give the same result, text and report, byte for byte.  No code is shared with the product.

    call(streams, genome, ref_names=None, min_mapq=0, exclude_flags=0x900, min_baseq=0, min_depth=1, max_ins=1024) -> Result
    header(genome_lengths) -> the header text;  report(counts, sites, variants, types, ...) -> the report text

1. Front half.  The genome, the files, the references by name, the record classes, the CIGAR resolution, the cells and the sites
   are tests/pileup_model.py's; the insertion cells and the insertion every ins_site emits are tests/consensus_model.py's, with
   max_ins: counts, sites, ins_unanchored and max_depth are those models'.
2. What a position p spells, E(p).  A ref_n or low site spells the prepared genome byte (the consensus with fill "ref"); a called
   site spells its call, or nothing where it calls del; an ins_site -- a del_site that is one included -- then spells its insertion
   as the consensus rule emits it.
3. Groups.  Within one genome record every position that is not a del_site is an anchor.  An anchor's group is the anchor and the
   run of del_sites directly behind it, up to the next anchor or the record's end; the record's first anchor also takes the
   del_sites in front of it (VCF's rule for an event at position 1).  No group crosses into another genome record.  A genome record
   that has positions and no anchor writes nothing: it counts in unplaced_records, its positions in unplaced_sites.
4. Records.  For a group over positions lo .. hi REF is the prepared genome bytes of lo .. hi, ALT is E(lo) .. E(hi) joined; a
   record is written exactly when ALT differs from REF as byte strings.
5. The line: name, POS = lo + 1, `.`, REF, ALT, `.`, `.`, `DP=d;MS=m;TYPE=t`, tab-separated.  DP is the pileup's depth at the
   group's anchor.  MS, the minimum support, is the smallest over the group of: the call's cell at a sub_site, the del cell at
   every del_site, n(p, j) (the sum of the five insertion cells) for every inserted base emitted.  TYPE: snv where both strings have
   one byte; ins where REF has one byte and ALT begins with it; del where ALT has one byte and REF begins with it; else complex.
6. The header: fileformat, source, one contig line per genome record in order (empty records included), the three INFO lines
   below, the column line.  It stands in front of the records and counts in text_bytes.
7. Result: the front half's numbers; variants; types (snv, ins, del, complex); ref_bases and alt_bases, the bytes of all REF and
   all ALT strings; longest_ref, longest_alt; unplaced_records, unplaced_sites; header_bytes; text_bytes.
8. The report: the pileup report's `#` and `S` lines, then `V` with variants, the four types, ref_bases, alt_bases, longest_ref,
   longest_alt, unplaced_records and unplaced_sites."""
import collections

import numpy as np

import consensus_model as K
import pileup_model as M
from pileup_model import COUNT_NAMES, SITE_NAMES, Malformed, inflate, parse, prepare_genome  # noqa: F401

TYPE_NAMES = ["snv", "ins", "del", "complex"]
SCALARS = ["ref_bases", "alt_bases", "longest_ref", "longest_alt", "unplaced_records", "unplaced_sites"]
INFO_LINES = [b'##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth of the pile at the record\'s anchor: A + C + G + T + other + del">\n',
              b'##INFO=<ID=MS,Number=1,Type=Integer,Description="Minimum support: the smallest count behind a substituted, deleted or inserted '
              b'base of the record">\n',
              b'##INFO=<ID=TYPE,Number=1,Type=String,Description="snv, ins, del or complex">\n']
COLUMNS = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"

Result = collections.namedtuple("Result", "counts sites ins_unanchored max_depth variants types ref_bases alt_bases longest_ref longest_alt "
                                          "unplaced_records unplaced_sites header_bytes text_bytes text records report")


def header(genome_lengths):
    """genome_lengths: (name, bases) per genome record"""
    out = [b"##fileformat=VCFv4.2\n", b"##source=pbsim3_amd\n"]
    for name, n in genome_lengths:
        name = name.encode() if isinstance(name, str) else bytes(name)
        out.append(b"##contig=<ID=" + name + b",length=%d>\n" % n)
    return b"".join(out + INFO_LINES + [COLUMNS])


def report(counts, sites, variants, types, ref_bases, alt_bases, longest_ref, longest_alt, unplaced_records, unplaced_sites):
    head = M.report(counts, sites, [0] * 8, 0, 0, [0] * 12, [0] * 12, [0] * 12, [0] * 12).split(b"\n")
    values = [variants] + list(types) + [ref_bases, alt_bases, longest_ref, longest_alt, unplaced_records, unplaced_sites]
    return head[0] + b"\n" + head[1] + b"\n" + ("V" + "".join("\t%d" % v for v in values) + "\n").encode()


def kind_of(ref, alt):
    if len(ref) == 1 and len(alt) == 1:
        return "snv"
    if len(ref) == 1 and alt[:1] == ref:
        return "ins"
    if len(alt) == 1 and ref[:1] == alt:
        return "del"
    return "complex"


def call_parsed(files, genome, ref_names=None, min_mapq=0, exclude_flags=0x900, min_baseq=0, min_depth=1, max_ins=1024):
    """files: a list of (refs, records) as parse() gives them"""
    assert 1 <= max_ins <= 65535
    pile = M.pileup_parsed(files, genome, ref_names, min_mapq=min_mapq, exclude_flags=exclude_flags, min_baseq=min_baseq, min_depth=min_depth)
    ins_cells = K.insertion_cells(files, genome, ref_names, min_mapq, exclude_flags, max_ins)
    prepared = prepare_genome(genome)
    lines, records, lengths = [], [], []
    types = dict.fromkeys(TYPE_NAMES, 0)
    n = dict.fromkeys(SCALARS, 0)
    for (name, _), tab in zip(genome, pile.cells):
        name = name.encode() if isinstance(name, str) else bytes(name)
        seq, hp = prepared[name]
        tab = tab.astype(np.int64)
        depth, call, cls, ins_site = M.classify(tab, seq, hp, min_depth)
        lengths.append((name, len(seq)))
        spelt, support = [], []                                 # E(p), and the counts behind what it spells that is not the genome's
        for p in range(len(seq)):
            e, s = b"", []
            if cls[p] < 2:
                e = bytes([seq[p]])
            elif call[p] == 4:
                s.append(int(tab[p, 5]))
            else:
                e = b"ACGT"[call[p]:call[p] + 1]
                if cls[p] == 3:
                    s.append(int(tab[p, call[p]]))
            if ins_site[p]:
                for j, c in enumerate(ins_cells[name].get(p, [])):
                    c = [v % (1 << 32) for v in c]
                    if j >= max_ins or not 2 * sum(c) > depth[p]:
                        break
                    best = max(c[:4])
                    e += b"N" if best == 0 else b"ACGT"[c[:4].index(best):c[:4].index(best) + 1]
                    s.append(sum(c))
            spelt.append(e)
            support.append(s)
        anchors = [p for p in range(len(seq)) if cls[p] != 4]
        written = 0
        if len(seq) and not anchors:
            n["unplaced_records"] += 1
            n["unplaced_sites"] += len(seq)
        for k, a in enumerate(anchors):
            lo = 0 if k == 0 else a
            hi = anchors[k + 1] - 1 if k + 1 < len(anchors) else len(seq) - 1
            ref, alt = seq[lo:hi + 1].tobytes(), b"".join(spelt[lo:hi + 1])
            if ref == alt:
                continue
            ms, t = min(v for s in support[lo:hi + 1] for v in s), kind_of(ref, alt)
            lines.append(name + b"\t%d\t.\t" % (lo + 1) + ref + b"\t" + alt + b"\t.\t.\tDP=%d;MS=%d;TYPE=%s\n" % (depth[a], ms, t.encode()))
            written += 1
            types[t] += 1
            n["ref_bases"] += len(ref)
            n["alt_bases"] += len(alt)
            n["longest_ref"], n["longest_alt"] = max(n["longest_ref"], len(ref)), max(n["longest_alt"], len(alt))
        records.append((len(seq), written))
    head = header(lengths)
    text = head + b"".join(lines)
    t = [types[k] for k in TYPE_NAMES]
    s = [n[k] for k in SCALARS]
    return Result(pile.counts, pile.sites, pile.ins_unanchored, pile.max_depth, len(lines), t, *s, len(head), len(text), text, records,
                  report(pile.counts, pile.sites, len(lines), t, *s))


def call(streams, genome, ref_names=None, **kw):
    """streams: one inflated stream, or a list of them; genome: a list of (name, sequence lines)"""
    if isinstance(streams, (bytes, bytearray)):
        streams = [streams]
    return call_parsed([parse(s) for s in streams], genome, ref_names, **kw)
