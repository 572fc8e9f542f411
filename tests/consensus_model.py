"""The rule of `pbsim --consensus-bam` (pbsim_bam_consensus) in plain Python and numpy: the sequence the pile of aligned reads of one
or more BAM files spells, per genome record, as FASTA.  This file is the contract; the product's kernels
(pbsim3_amd/csrc/bam_consensus.hip) must give the same result, FASTA and report, byte for byte.  No code is shared with the product.

    consensus(streams, genome, ref_names=None, min_mapq=0, exclude_flags=0x900, min_baseq=0, min_depth=1, fill="n", max_ins=1024,
              line_width=60) -> Result
    report(counts, sites, bases, ins_sites, ins_longest, ins_capped, ins_len) -> the report text

1. Front half.  The genome, the files, the references by name, the record classes, the CIGAR resolution, the cells and the sites
   are tests/pileup_model.py's, with the same options: counts, sites, ins_unanchored and max_depth are that model's.
2. Insertion cells.  An I op of length L >= 1 of a scored record that is anchored at position a (a = q - 1 with q > pos, q the
   record's reference position where the op begins) adds, for every offset j with 0 <= j < min(L, max_ins), 1 to cell b of (a, j):
   b is the read class of the inserted base's 4-bit code, 1 2 4 8 -> 0 .. 3, every other code (0 included) -> 4.  Qualities mask
   nothing.  Cells are unsigned 32-bit, modulo 2^32.  n(a, j) is the sum of the five cells; n(a, 0) is the pileup's ins cell of a
   (asserted).  Unanchored insertions add nowhere.
3. The consensus of position p.  A ref_n or low site emits one byte: `N` with fill "n", the prepared genome byte with fill "ref".
   A called site emits its call (A C G T); a site that calls del emits nothing.  A called site that is an ins_site (2 ins >
   depth) then emits the insertion: for j = 0, 1, .. while j < max_ins and 2 n(p, j) > depth(p), the largest of the A C G T cells
   of (p, j), among equals the first, `N` where all four are 0.
4. The FASTA.  Genome records in their order, each `>name\\n`, then its consensus bases in lines of line_width bases (0: one line),
   `\\n` after every line, the last partial one included; a record of no consensus bases is its header line alone.
5. bases = out, kept (concordant sites), sub, ins (inserted bases emitted), fill, del (called sites that emit nothing);
   ins_sites; ins_longest; ins_capped (ins_sites whose insertion has exactly max_ins bases); ins_len[min(length, 63)]; text_bytes.
   out = kept + sub + ins + fill and sites = kept + sub + del + fill (asserted).
6. The report: the pileup report's `#` and `S` lines; `K` with the six bases, ins_sites, ins_longest, ins_capped; `IL\\t<bin>\\t
   <sites>` for the bins that are not empty."""
import collections

import numpy as np

import errors_model as E
import pileup_model as M
from pileup_model import COUNT_NAMES, SITE_NAMES, Malformed, aux_walk, inflate, parse, prepare_genome  # noqa: F401

BASE_NAMES = ["out", "kept", "sub", "ins", "fill", "del"]
FILLS = ("n", "ref")

Result = collections.namedtuple("Result", "counts sites ins_unanchored max_depth bases ins_sites ins_longest ins_capped ins_len text_bytes "
                                          "text lengths report")


def report(counts, sites, bases, ins_sites, ins_longest, ins_capped, ins_len):
    head = M.report(counts, sites, [0] * 8, 0, 0, [0] * 12, [0] * 12, [0] * 12, [0] * 12).split(b"\n")
    out = [head[0] + b"\n", head[1] + b"\n",
           ("K" + "".join("\t%d" % v for v in bases) + "\t%d\t%d\t%d\n" % (ins_sites, ins_longest, ins_capped)).encode()]
    out += [b"IL\t%d\t%d\n" % (v, n) for v, n in enumerate(ins_len) if n]
    return b"".join(out)


def insertion_cells(files, genome, ref_names, min_mapq, exclude_flags, max_ins):
    """{name: {anchor: [[A C G T other] per offset]}} over the scored records, classed as the pileup's rule classes them"""
    prepared = prepare_genome(genome)
    ref_names = list(ref_names) if ref_names is not None else [None] * len(files)
    cells = {(name.encode() if isinstance(name, str) else bytes(name)): {} for name, _ in genome}
    for k, (refs, recs) in enumerate(files):
        over = ref_names[k]
        if over is not None:
            over = over.encode() if isinstance(over, str) else bytes(over)
        table = [(over if over is not None else name) for name, _ in refs]
        table = [key if key in prepared else None for key in table]
        for rec in recs:
            if rec["flag"] & exclude_flags or rec["flag"] & 4 or not 0 <= rec["ref_id"] < len(refs) or rec["pos"] < 0 or not rec["cigar"]:
                continue
            if rec["mapq"] < min_mapq or table[rec["ref_id"]] is None:
                continue
            key = table[rec["ref_id"]]
            l_seq, cigar, pos = rec["l_seq"], rec["cigar"], rec["pos"]
            placeholder = len(cigar) == 2 and cigar[0] == (l_seq, 4) and cigar[1][1] == 3
            cg, _ = aux_walk(rec["aux"], rec["offset"], placeholder, True)
            if cg is not None:
                cigar = cg
            by_op = [sum(n for n, op in cigar if op == k) for k in range(9)]
            m = by_op[0] + by_op[7] + by_op[8]
            if l_seq == 0 or m + by_op[1] + by_op[4] != l_seq or pos + m + by_op[2] + by_op[3] > len(prepared[key][0]):
                continue                                        # no_seq or misfit: not scored
            packed = np.frombuffer(rec["seq"], np.uint8)
            nib = np.empty(2 * len(packed), np.int64)
            nib[0::2], nib[1::2] = packed >> 4, packed & 15
            q, r = 0, pos
            for n, op in cigar:
                if op == 1 and n >= 1 and r > pos:
                    slot = cells[key].setdefault(r - 1, [])
                    for j in range(min(n, max_ins)):
                        if j == len(slot):
                            slot.append([0] * 5)
                        slot[j][int(E._BCLS[nib[q + j]])] += 1
                if op in (0, 1, 4, 7, 8):
                    q += n
                if op in (0, 2, 3, 7, 8):
                    r += n
    return cells


def wrap(bases, line_width):
    if not bases:
        return b""
    if line_width == 0:
        return bases + b"\n"
    return b"".join(bases[k:k + line_width] + b"\n" for k in range(0, len(bases), line_width))


def consensus_parsed(files, genome, ref_names=None, min_mapq=0, exclude_flags=0x900, min_baseq=0, min_depth=1, fill="n", max_ins=1024,
                     line_width=60):
    """files: a list of (refs, records) as parse() gives them"""
    assert fill in FILLS and 1 <= max_ins <= 65535 and 0 <= line_width <= 1 << 20
    pile = M.pileup_parsed(files, genome, ref_names, min_mapq=min_mapq, exclude_flags=exclude_flags, min_baseq=min_baseq, min_depth=min_depth)
    ins_cells = insertion_cells(files, genome, ref_names, min_mapq, exclude_flags, max_ins)
    prepared = prepare_genome(genome)
    bases = dict.fromkeys(BASE_NAMES, 0)
    ins_sites = ins_longest = ins_capped = 0
    ins_len = [0] * 64
    text, lengths = [], []
    for (name, _), tab in zip(genome, pile.cells):
        name = name.encode() if isinstance(name, str) else bytes(name)
        seq, hp = prepared[name]
        depth, call, cls, ins_site = M.classify(tab.astype(np.int64), seq, hp, min_depth)
        slots = ins_cells[name]
        for a, slot in slots.items():                           # n(a, 0) is the pileup's ins cell; n does not grow with j
            n = [sum(c) for c in slot]
            assert n[0] % (1 << 32) == int(tab[a, 6]) and all(x >= y for x, y in zip(n, n[1:]))
        bare = np.ones(len(seq), bool)
        bare[list(slots)] = False
        assert not tab[bare, 6].any()
        # every site's own byte (0: none), then the insertions behind the ins_sites
        filled, deleted = cls < 2, (cls >= 2) & (call == 4)
        own = np.where(filled, seq if fill == "ref" else ord("N"), np.where(deleted, 0, np.frombuffer(b"ACGTA", np.uint8)[np.maximum(call, 0)]))
        bases["fill"] += int(filled.sum())
        bases["del"] += int(deleted.sum())
        bases["kept"] += int((cls == 2).sum())
        bases["sub"] += int(((cls == 3) & ~deleted).sum())
        out, at = bytearray(), 0
        for p in np.nonzero(ins_site)[0]:
            p = int(p)
            out += own[at:p + 1][own[at:p + 1] != 0].astype(np.uint8).tobytes()
            at = p + 1
            length = 0
            for j, c in enumerate(slots.get(p, [])):
                c = [v % (1 << 32) for v in c]
                if j >= max_ins or not 2 * sum(c) > depth[p]:
                    break
                best = max(c[:4])
                out.append(ord("N") if best == 0 else b"ACGT"[c[:4].index(best)])
                length += 1
            assert length >= 1                                  # its first base is there exactly when the site is an ins_site
            ins_sites += 1
            ins_longest = max(ins_longest, length)
            ins_capped += length == max_ins
            ins_len[min(length, 63)] += 1
            bases["ins"] += length
        out += own[at:][own[at:] != 0].astype(np.uint8).tobytes()
        bases["out"] += len(out)
        lengths.append((len(seq), len(out)))
        text.append(b">" + name + b"\n" + wrap(bytes(out), line_width))
    text = b"".join(text)
    b = [bases[n] for n in BASE_NAMES]
    assert bases["out"] == bases["kept"] + bases["sub"] + bases["ins"] + bases["fill"]
    assert pile.sites[0] == bases["kept"] + bases["sub"] + bases["del"] + bases["fill"] and ins_sites == pile.sites[7]
    return Result(pile.counts, pile.sites, pile.ins_unanchored, pile.max_depth, b, ins_sites, ins_longest, ins_capped, ins_len, len(text), text,
                  lengths, report(pile.counts, pile.sites, b, ins_sites, ins_longest, ins_capped, ins_len))


def consensus(streams, genome, ref_names=None, **kw):
    """streams: one inflated stream, or a list of them; genome: a list of (name, sequence lines)"""
    if isinstance(streams, (bytes, bytearray)):
        streams = [streams]
    return consensus_parsed([parse(s) for s in streams], genome, ref_names, **kw)
