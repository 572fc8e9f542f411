"""The rule of `pbsim --pileup-bam` (pbsim_bam_pileup) in plain Python and numpy: per position of the genome what the aligned reads of
one or more BAM files say there, the call of every site and the sites where the pile does not spell the genome.  This file is the
contract; the product's kernels (pbsim3_amd/csrc/bam_pileup.hip) must give the same result, cells, text and report, byte for byte.
The streams are parsed, the genome is prepared, records are classed and CIGARs resolved exactly as tests/errors_model.py does it
(its parse, prepare_genome and aux walk are used); no code is shared with the product.

    pileup(streams, genome, ref_names=None, min_mapq=0, exclude_flags=0x900, min_baseq=0, min_depth=1, fmt="sites") -> Result
    report(counts, sites, cell_sums, ins_unanchored, max_depth, hp_called, hp_sub, hp_del, hp_ins) -> the report text

Only a scored record adds to the pileup.  Per position p of each genome record eight cells, unsigned 32-bit, additions modulo
2^32: 0 .. 3 A C G T, 4 other, 5 del, 6 ins, 7 masked.  r and b as in the errors rule.  An M, = or X column at p adds 1 to cell b
-- unless the record has qualities (first byte not 0xFF) and the base's quality byte is below min_baseq: then to masked alone.  A
D column adds 1 to del.  An I op of length >= 1 that begins at reference position q adds 1 to ins at q - 1 where q > pos, else to
ins_unanchored.  N only advances; S, H, P and ops of length 0 do nothing.

Sites, over every position: depth = A + C + G + T + other + del; ref_n if the genome's class is 4, else low if depth < min_depth,
else called: the call is the largest of A C G T del, among equals the genome's class if it is one of them, else the first; the
site is concordant (class "match"), a del_site ("del") or a sub_site ("sub"), and besides an ins_site ("+ins") if 2 ins > depth;
discordant = sub_site or del_site or ins_site.  hp_*[v]: the called, sub, del and ins sites by the genome's class byte, min(v, 11).

Text, one line per site (fmt "sites": the discordant ones; "all": every position), genome records in order, positions ascending:
name, pos1, ref, depth, A, C, G, T, N, del, ins, masked, call (A C G T, * for del, . not called), class."""
import collections
import math

import numpy as np

import errors_model as E
from errors_model import Malformed, aux_walk, inflate, parse, prepare_genome  # noqa: F401

COUNT_NAMES = ["records", "skipped_flag", "unaligned", "skipped_mapq", "skipped_ref", "aligned", "no_seq", "misfit", "scored"]
SITE_NAMES = ["sites", "ref_n", "low", "called", "concordant", "sub_site", "del_site", "ins_site", "discordant"]
CELL_NAMES = ["A", "C", "G", "T", "other", "del", "ins", "masked"]
HP_ARRAYS = ["hp_called", "hp_sub", "hp_del", "hp_ins"]
CLASS_NAMES = ["ref_n", "low", "match", "sub", "del"]
FORMATS = ("sites", "all")
CALLS = b"ACGT*"
_CANDIDATES = (0, 1, 2, 3, 5)           # the cells a call is chosen among, in the order of CALLS

Result = collections.namedtuple("Result", "counts sites cell_sums ins_unanchored max_depth hp_called hp_sub hp_del hp_ins cells text report")


def report(counts, sites, cell_sums, ins_unanchored, max_depth, hp_called, hp_sub, hp_del, hp_ins):
    s = dict(zip(SITE_NAMES, sites))
    d, c = s["discordant"], s["called"]
    q = "%d" % math.floor(-10000.0 * math.log10(float(d) / float(c))) if d > 0 and c > 0 else "*"
    out = ["#" + "".join(" %s=%d" % (n, v) for n, v in zip(COUNT_NAMES, counts)) + "\n",
           "S" + "".join("\t%d" % v for v in sites) + "\t%d\t%s\n" % (d * 1000000 // c if c else 0, q),
           "C" + "".join("\t%d" % v for v in cell_sums) + "\t%d\t%d\n" % (ins_unanchored, max_depth)]
    out += ["HP\t%d\t%d\t%d\t%d\t%d\n" % (v, hp_called[v], hp_sub[v], hp_del[v], hp_ins[v]) for v in range(12)
            if hp_called[v] or hp_sub[v] or hp_del[v] or hp_ins[v]]
    return "".join(out).encode("latin-1")


def classify(cells, seq, hp, min_depth):
    """per position: depth, the call (0 .. 4 in the order of CALLS, -1 none), the class (index of CLASS_NAMES), ins_site"""
    c = cells.astype(np.int64)
    depth = c[:, :6].sum(axis=1)
    r = E._RCLS[seq]
    cand = c[:, _CANDIDATES]
    best = cand.max(axis=1) if len(c) else np.zeros(0, np.int64)
    first = np.argmax(cand == best[:, None], axis=1) if len(c) else np.zeros(0, np.int64)
    own = np.minimum(r, 3)
    call = np.where((r < 4) & (cand[np.arange(len(c)), own] == best), own, first)
    called = (r < 4) & (depth >= min_depth)
    cls = np.where(r == 4, 0, np.where(~called, 1, np.where(call == r, 2, np.where(call == 4, 4, 3))))
    ins_site = called & (2 * c[:, 6] > depth)
    return depth, np.where(called, call, -1), cls, ins_site


def pileup_parsed(files, genome, ref_names=None, min_mapq=0, exclude_flags=0x900, min_baseq=0, min_depth=1, fmt="sites"):
    """files: a list of (refs, records) as parse() gives them"""
    assert fmt in FORMATS or fmt == "both"              # both: a pair of results, one per format, from one pass
    prepared = prepare_genome(genome)
    order = [name.encode() if isinstance(name, str) else bytes(name) for name, _ in genome]
    ref_names = list(ref_names) if ref_names is not None else [None] * len(files)
    assert len(ref_names) == len(files)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    cells = {name: np.zeros((len(prepared[name][0]), 8), np.int64) for name in order}
    ins_unanchored = 0
    tables = []
    for k, (refs, _) in enumerate(files):           # every file's references are looked up before any record is read
        over = ref_names[k]
        if over is not None:
            over = over.encode() if isinstance(over, str) else bytes(over)
            if len(refs) != 1:
                raise ValueError("file %d has %d references: a reference name can be given only to a file with exactly one" % (k, len(refs)))
        table = []
        for name, l_ref in refs:
            key = over if over is not None else name
            got = prepared.get(key)
            if got is not None and len(got[0]) != l_ref:
                raise ValueError("l_ref %d, %d bases" % (l_ref, len(got[0])))
            table.append(None if got is None else key)
        tables.append(table)
    for (refs, recs), table in zip(files, tables):
        for rec in sorted(recs, key=lambda r: r["offset"]):
            counts["records"] += 1
            if rec["flag"] & exclude_flags:
                counts["skipped_flag"] += 1
                continue
            if rec["flag"] & 4 or not 0 <= rec["ref_id"] < len(refs) or rec["pos"] < 0 or not rec["cigar"]:
                counts["unaligned"] += 1
                continue
            if rec["mapq"] < min_mapq:
                counts["skipped_mapq"] += 1
                continue
            if table[rec["ref_id"]] is None:
                counts["skipped_ref"] += 1
                continue
            counts["aligned"] += 1
            key = table[rec["ref_id"]]
            seq, tab = prepared[key][0], cells[key]
            l_seq, cigar, pos = rec["l_seq"], rec["cigar"], rec["pos"]
            placeholder = len(cigar) == 2 and cigar[0] == (l_seq, 4) and cigar[1][1] == 3
            cg, _ = aux_walk(rec["aux"], rec["offset"], placeholder, True)
            if cg is not None:
                cigar = cg
            if any(op > 8 for _, op in cigar):
                raise Malformed(rec["offset"], "a CIGAR op code above 8")
            lens = np.array([n for n, _ in cigar], np.int64)
            code = np.array([op for _, op in cigar], np.int64)
            by_op = [int(lens[code == k].sum()) for k in range(9)]
            m, ins, dele, soft = by_op[0] + by_op[7] + by_op[8], by_op[1], by_op[2], by_op[4]
            if l_seq == 0:
                counts["no_seq"] += 1
                continue
            if m + ins + soft != l_seq or pos + m + dele + by_op[3] > len(seq):
                counts["misfit"] += 1
                continue
            counts["scored"] += 1
            q_adv = np.where(np.isin(code, (0, 1, 4, 7, 8)), lens, 0)
            r_adv = np.where(np.isin(code, (0, 2, 3, 7, 8)), lens, 0)
            q_at, r_at = np.cumsum(q_adv) - q_adv, pos + np.cumsum(r_adv) - r_adv
            packed = np.frombuffer(rec["seq"], np.uint8)
            nib = np.empty(2 * len(packed), np.int64)
            nib[0::2], nib[1::2] = packed >> 4, packed & 15
            qual = np.frombuffer(rec["qual"], np.uint8).astype(np.int64)
            has_qual = rec["qual"][0] != 0xFF
            # ---- M = X
            sel = np.isin(code, (0, 7, 8))
            rp, qp = E._expand(r_at[sel], q_at[sel], lens[sel])
            r = E._RCLS[seq[rp]]
            b = np.where(nib[qp] == 0, r, E._BCLS[nib[qp]])
            if has_qual:
                b = np.where(qual[qp] < min_baseq, 7, b)
            np.add.at(tab, (rp, b), 1)
            # ---- D
            sel = (code == 2) & (lens > 0)
            rp, _ = E._expand(r_at[sel], q_at[sel], lens[sel])
            np.add.at(tab, (rp, np.full(len(rp), 5)), 1)
            # ---- I
            for q in r_at[(code == 1) & (lens > 0)]:
                if q > pos:
                    tab[q - 1, 6] += 1
                else:
                    ins_unanchored += 1
    sites = dict.fromkeys(SITE_NAMES, 0)
    hp_arr = {name: [0] * 12 for name in HP_ARRAYS}
    cell_sums = [0] * 8
    max_depth = 0
    text = {f: [] for f in FORMATS}
    out_cells = []
    for name in order:
        seq, hp = prepared[name]
        tab = cells[name] % (1 << 32)
        out_cells.append(tab.astype(np.uint32))
        depth, call, cls, ins_site = classify(tab, seq, hp, min_depth)
        v = np.minimum(hp.astype(np.int64), 11)
        called, sub, dele = cls >= 2, cls == 3, cls == 4
        disc = sub | dele | ins_site
        for key, mask in (("sites", np.ones(len(seq), bool)), ("ref_n", cls == 0), ("low", cls == 1), ("called", called), ("concordant", cls == 2),
                          ("sub_site", sub), ("del_site", dele), ("ins_site", ins_site), ("discordant", disc)):
            sites[key] += int(mask.sum())
        for key, mask in (("hp_called", called), ("hp_sub", sub), ("hp_del", dele), ("hp_ins", ins_site)):
            for k, n in enumerate(np.bincount(v[mask], minlength=12)):
                hp_arr[key][k] += int(n)
        for k in range(8):
            cell_sums[k] += int(tab[:, k].sum())
        if len(seq):
            max_depth = max(max_depth, int(depth.max()))
        for f in FORMATS if fmt == "both" else (fmt,):
            for p in (np.nonzero(disc)[0] if f == "sites" else range(len(seq))):
                word = CLASS_NAMES[cls[p]] + ("+ins" if ins_site[p] else "")
                t = tab[p]
                text[f].append(name + ("\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (
                    p + 1, chr(seq[p]), depth[p], t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7],
                    chr(CALLS[call[p]]) if call[p] >= 0 else ".", word)).encode("latin-1"))
    cl, sl = [int(counts[n]) for n in COUNT_NAMES], [int(sites[n]) for n in SITE_NAMES]
    hps = [hp_arr[n] for n in HP_ARRAYS]
    both = [Result(cl, sl, cell_sums, ins_unanchored, max_depth, *hps, out_cells, b"".join(text[f]),
                   report(cl, sl, cell_sums, ins_unanchored, max_depth, *hps)) for f in FORMATS]
    return tuple(both) if fmt == "both" else both[FORMATS.index(fmt)]


def pileup(streams, genome, ref_names=None, **kw):
    """streams: one inflated stream, or a list of them; genome: a list of (name, sequence lines)"""
    if isinstance(streams, (bytes, bytearray)):
        streams = [streams]
    return pileup_parsed([parse(s) for s in streams], genome, ref_names, **kw)
