"""The rule of `pbsim --errors-bam` (pbsim_bam_errors) in plain Python and numpy: the error profile of the aligned reads of one or
more BAM files against the genome they were aligned to.  This file is the contract; the product's kernels
(pbsim3_amd/csrc/bam_errors.hip) must give the same result, text and report, byte for byte.  It reads inflated BAM streams (SAMv1
4.2) with the primitives of tests/bam_spec_reader.py, walks the aux fields as tests/stats_model.py does, prepares the genome with
tests/ref_prep_model.py and shares no code with the product.

    parse(stream)                 -> ([(reference name, l_ref), ...], [record dict, ...])
    errors(streams, genome, ref_names=None, min_mapq=0, exclude_flags=0x900) -> Result
    fit(hp_cols, hp_del)          -> (fit_ok, fit_bias_milli, fit_suggest_milli)
    report(result values)         -> the report text

The genome is a list of (name, sequence lines); a record's sequence is its lines without the line feeds, prepared by
ref_prep_model.prepare (a-z upper-cased; one class byte 1 .. 11 per base, N has class 1), each record on its own.  Two records of
one name are refused (ValueError).  A BAM reference is looked up by name -- by ref_names[k] in file k where that is given, which
needs a file of exactly one reference; a reference the genome lacks makes its records skipped_ref, one whose l_ref is not the
prepared length is refused (ValueError).

Class of a record, in this order: skipped_flag if flag & exclude_flags; unaligned if flag & 4, refID < 0 (or >= n_ref), pos < 0 or
n_cigar_op == 0; skipped_mapq if mapq < min_mapq; skipped_ref; else aligned.  Of an aligned record the aux fields are walked (NM,
and CG where the CIGAR is the <l_seq>S<span>N placeholder) and the CIGAR's op codes are looked at: a malformed field or an op code
above 8 is Malformed with the record's offset.  An aligned record is no_seq if l_seq == 0, else misfit if the CIGAR's query length
(M I S = X) is not l_seq or pos + its span (M D N = X) > l_ref, else scored.

Columns of a scored record.  r, the reference class: A C G T -> 0 .. 3, every other byte 4.  b, the read class, from the 4-bit
code: 1 2 4 8 -> 0 .. 3, 0 (=) -> r (4 in an inserted base, which has no r), every other code 4.  An M, = or X column adds to
pair[5 r + b] and is ambiguous if r or b is 4, else a match if r == b, else a sub.  hp_cols[v], v the reference base's class byte,
counts the M = X and D columns, hp_sub[v] the sub columns, hp_del[v] the D columns.  An I op of length >= 1 adds to ins_events and
ins_len[min(length, 63)], its bases to ins and ins_base[b]; a D op likewise to del_events, del_len, del and del_base[r].  S adds
to soft, H to hard, N only advances, P and ops of length 0 do nothing.  With qualities (the first byte is not 0xFF), q' = min(q,
127): qcal[q'][0] counts the M = X columns that are not ambiguous, qcal[q'][1] the sub columns, qcal[q'][2] the inserted bases.

Per scored record: cols = m + ins + del; with cols >= 1 identity_ppm = match * 1000000 // cols and hist_identity[identity_ppm //
1000] += 1; nm_derived = sub + ins + del; no_nm where the first integer NM is absent or negative, else nm_unchecked where ambiguous
> 0, else nm_agree or nm_differ."""
import collections
import math
import struct

import numpy as np

import bam_spec_reader as R
import ref_prep_model
from stats_model import Malformed, aux_walk, inflate  # noqa: F401  (the same walk, the same refusal)

COUNT_NAMES = ["records", "skipped_flag", "unaligned", "skipped_mapq", "skipped_ref", "aligned", "no_seq", "misfit", "scored", "no_nm",
               "nm_unchecked", "nm_agree", "nm_differ", "with_qual"]
TOTAL_NAMES = ["cols", "match", "sub", "ambiguous", "ins", "del", "ins_events", "del_events", "soft", "hard", "identity_sum"]
ARRAYS = [("pair", 25), ("hp_cols", 12), ("hp_sub", 12), ("hp_del", 12), ("ins_len", 64), ("del_len", 64), ("ins_base", 5), ("del_base", 5),
          ("qcal", 384), ("hist_identity", 1001)]
FIT_NAMES = ["fit_ok", "fit_bias_milli", "fit_suggest_milli"]
BASES = "ACGTN"

Result = collections.namedtuple("Result", "counts totals pair hp_cols hp_sub hp_del ins_len del_len ins_base del_base qcal hist_identity fit "
                                          "text report")

_RCLS = np.full(256, 4, np.int64)
for _k, _c in enumerate(b"ACGT"):
    _RCLS[_c] = _k
_BCLS = np.full(16, 4, np.int64)
for _k, _c in enumerate((1, 2, 4, 8)):
    _BCLS[_c] = _k
_LIMIT = 2 ** 62


def parse(stream):
    """the references (name, l_ref) and the records of an inflated BAM stream: offset, flag, ref_id, pos, mapq, l_seq, name, cigar
    (a list of (length, op code)), seq (the packed bases), qual, aux"""
    R.need(stream[:4] == b"BAM\x01", "magic")
    at = 8 + R.le(stream, 4, 4)
    n_ref = R.le(stream, at, 4)
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = R.le(stream, at, 4)
        refs.append((stream[at + 4:at + 4 + l_name].split(b"\0")[0], R.le(stream, at + 4 + l_name, 4, True)))
        at += 8 + l_name
    recs = []
    while at < len(stream):
        block_size = R.le(stream, at, 4)
        l_read_name, n_cigar_op, l_seq = stream[at + 12], R.le(stream, at + 16, 2), R.le(stream, at + 20, 4)
        cig_at = at + 36 + l_read_name
        seq_at = cig_at + 4 * n_cigar_op
        qual_at = seq_at + (l_seq + 1) // 2
        ops = struct.unpack_from("<%dI" % n_cigar_op, stream, cig_at)
        recs.append(dict(offset=at, ref_id=R.le(stream, at + 4, 4, True), pos=R.le(stream, at + 8, 4, True), mapq=stream[at + 13],
                         flag=R.le(stream, at + 18, 2), l_seq=l_seq, name=stream[at + 36:cig_at].split(b"\0")[0],
                         cigar=[(v >> 4, v & 15) for v in ops], seq=stream[seq_at:qual_at], qual=stream[qual_at:qual_at + l_seq],
                         aux=stream[qual_at + l_seq:at + 4 + block_size]))
        at += 4 + block_size
    R.need(at == len(stream), "the last record ends where the stream ends")
    return refs, recs


def prepare_genome(genome):
    """name -> (prepared bytes, class bytes); a record without bases has two empty arrays"""
    out = {}
    for name, lines in genome:
        name = name.encode() if isinstance(name, str) else bytes(name)
        if name in out:
            raise ValueError("the genome holds two records named \"%s\"" % name.decode("latin-1"))
        raw = bytes(lines).replace(b"\n", b"")
        if raw:
            seq, hp, _ = ref_prep_model.prepare(raw)
        else:
            seq, hp = np.zeros(0, np.uint8), np.zeros(0, np.uint8)
        out[name] = (seq, hp)
    return out


def fit(hp_cols, hp_del):
    """the weighted least-squares line of the deletion rate on the class, v = 1 .. 10, as slope / intercept: what --hp-del-bias
    would have to be.  Big integers; the quotient is floored toward minus infinity and held to +-2^62."""
    x = range(10)
    c, d = [int(hp_cols[v]) for v in range(1, 11)], [int(hp_del[v]) for v in range(1, 11)]
    w, sx, sxx = sum(c), sum(ci * xi for ci, xi in zip(c, x)), sum(ci * xi * xi for ci, xi in zip(c, x))
    sy, sxy = sum(d), sum(di * xi for di, xi in zip(d, x))
    num, den = w * sxy - sx * sy, sxx * sy - sx * sxy
    if not (sy > 0 and den > 0):
        return [0, 0, 0]
    bias = max(-_LIMIT, min(_LIMIT, 1000 + 9000 * num // den))
    return [1, bias, max(1000, min(10000, bias))]


def report(counts, totals, pair, hp_cols, hp_sub, hp_del, ins_len, del_len, ins_base, del_base, qcal, hist_identity):
    t = dict(zip(TOTAL_NAMES, totals))
    n_identity = sum(hist_identity)
    out = ["#" + "".join(" %s=%d" % (n, v) for n, v in zip(COUNT_NAMES, counts)) + "\n",
           "E" + "".join("\t%d" % v for v in totals[:10]) +
           "".join("\t%d" % (t[k] * 1000000 // t["cols"] if t["cols"] else 0) for k in ("sub", "ins", "del")) +
           "\t%d\n" % (t["identity_sum"] // n_identity if n_identity else 0)]
    out += ["M\t%s" % BASES[r] + "".join("\t%d" % pair[5 * r + b] for b in range(5)) + "\n" for r in range(5)]
    out += ["HP\t%d\t%d\t%d\t%d\t%d\n" % (v, hp_cols[v], hp_sub[v], hp_del[v], hp_del[v] * 1000000 // hp_cols[v]) for v in range(12) if hp_cols[v] > 0]
    out.append("B\t%d\t%d\t%d\n" % tuple(fit(hp_cols, hp_del)))
    out += ["IL\t%d\t%d\n" % (k, v) for k, v in enumerate(ins_len) if v > 0]
    out += ["DL\t%d\t%d\n" % (k, v) for k, v in enumerate(del_len) if v > 0]
    out.append("IB" + "".join("\t%d" % v for v in ins_base) + "\n")
    out.append("DB" + "".join("\t%d" % v for v in del_base) + "\n")
    for q in range(128):
        cols, sub, ins = qcal[3 * q:3 * q + 3]
        if cols > 0 or sub > 0 or ins > 0:
            emp = "%d" % math.floor(-10000.0 * math.log10(float(sub) / float(cols))) if cols > 0 and sub > 0 else "*"
            out.append("QC\t%d\t%d\t%d\t%d\t%s\n" % (q, cols, sub, ins, emp))
    out += ["HI\t%d\t%d\n" % (k, v) for k, v in enumerate(hist_identity) if v > 0]
    return "".join(out).encode("latin-1")


def _expand(first_ref, first_query, lens):
    """the reference and query positions of every column of the ops that begin at (first_ref, first_query) and are lens long"""
    total = int(lens.sum())
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    return np.repeat(first_ref, lens) + within, np.repeat(first_query, lens) + within


def errors_parsed(files, genome, ref_names=None, min_mapq=0, exclude_flags=0x900):
    """files: a list of (refs, records) as parse() gives them"""
    prepared = prepare_genome(genome)
    ref_names = list(ref_names) if ref_names is not None else [None] * len(files)
    assert len(ref_names) == len(files)
    counts = dict.fromkeys(COUNT_NAMES, 0)
    totals = dict.fromkeys(TOTAL_NAMES, 0)
    arr = {name: np.zeros(n, np.int64) for name, n in ARRAYS}
    text = []
    tables = []
    for k, (refs, _) in enumerate(files):           # every file's references are looked up before any record is read
        over = ref_names[k]
        if over is not None:
            over = over.encode() if isinstance(over, str) else bytes(over)
            if len(refs) != 1:
                raise ValueError("file %d has %d references: a reference name can be given only to a file with exactly one" % (k, len(refs)))
        table = []
        for name, l_ref in refs:
            got = prepared.get(over if over is not None else name)
            if got is not None and len(got[0]) != l_ref:
                raise ValueError("l_ref %d, %d bases" % (l_ref, len(got[0])))
            table.append(got)
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
            seq, hp = table[rec["ref_id"]]
            l_seq, cigar = rec["l_seq"], rec["cigar"]
            placeholder = len(cigar) == 2 and cigar[0] == (l_seq, 4) and cigar[1][1] == 3
            cg, nm = aux_walk(rec["aux"], rec["offset"], placeholder, True)
            if cg is not None:
                cigar = cg
            if any(op > 8 for _, op in cigar):
                raise Malformed(rec["offset"], "a CIGAR op code above 8")
            lens = np.array([n for n, _ in cigar], np.int64)
            code = np.array([op for _, op in cigar], np.int64)
            by_op = [int(lens[code == k].sum()) for k in range(9)]
            m, ins, dele, soft, hard = by_op[0] + by_op[7] + by_op[8], by_op[1], by_op[2], by_op[4], by_op[5]
            line = dict(length=l_seq, cols=m + ins + dele, ins=ins, soft=soft)
            line["del"] = dele
            if nm is not None and nm >= 0:
                line["nm_tag"] = nm
            if l_seq == 0:
                counts["no_seq"] += 1
                cls = "N"
            elif m + ins + soft != l_seq or rec["pos"] + m + dele + by_op[3] > len(seq):
                counts["misfit"] += 1
                cls = "F"
            else:
                counts["scored"] += 1
                cls = "S"
                q_adv = np.where(np.isin(code, (0, 1, 4, 7, 8)), lens, 0)
                r_adv = np.where(np.isin(code, (0, 2, 3, 7, 8)), lens, 0)
                q_at, r_at = np.cumsum(q_adv) - q_adv, rec["pos"] + np.cumsum(r_adv) - r_adv
                packed = np.frombuffer(rec["seq"], np.uint8)
                nib = np.empty(2 * len(packed), np.int64)
                nib[0::2], nib[1::2] = packed >> 4, packed & 15
                qual = np.minimum(np.frombuffer(rec["qual"], np.uint8), 127).astype(np.int64)
                has_qual = rec["qual"][0] != 0xFF
                counts["with_qual"] += has_qual
                # ---- M = X
                sel = np.isin(code, (0, 7, 8))
                rp, qp = _expand(r_at[sel], q_at[sel], lens[sel])
                r = _RCLS[seq[rp]]
                b = np.where(nib[qp] == 0, r, _BCLS[nib[qp]])
                amb = (r == 4) | (b == 4)
                sub = ~amb & (r != b)
                match = int((~amb & (r == b)).sum())
                arr["pair"] += np.bincount(5 * r + b, minlength=25)
                arr["hp_cols"] += np.bincount(hp[rp], minlength=12)
                arr["hp_sub"] += np.bincount(hp[rp][sub], minlength=12)
                if has_qual:
                    arr["qcal"][0::3] += np.bincount(qual[qp][~amb], minlength=128)
                    arr["qcal"][1::3] += np.bincount(qual[qp][sub], minlength=128)
                # ---- I
                sel = (code == 1) & (lens > 0)
                _, qp = _expand(r_at[sel], q_at[sel], lens[sel])
                arr["ins_base"] += np.bincount(_BCLS[nib[qp]], minlength=5)           # (= has no r here: 4)
                arr["ins_len"] += np.bincount(np.minimum(lens[sel], 63), minlength=64)
                if has_qual:
                    arr["qcal"][2::3] += np.bincount(qual[qp], minlength=128)
                # ---- D
                sel = (code == 2) & (lens > 0)
                rp, _ = _expand(r_at[sel], q_at[sel], lens[sel])
                arr["del_base"] += np.bincount(_RCLS[seq[rp]], minlength=5)
                arr["del_len"] += np.bincount(np.minimum(lens[sel], 63), minlength=64)
                arr["hp_cols"] += np.bincount(hp[rp], minlength=12)
                arr["hp_del"] += np.bincount(hp[rp], minlength=12)
                n_sub, n_amb, cols = int(sub.sum()), int(amb.sum()), m + ins + dele
                derived = n_sub + ins + dele
                line.update(match=match, sub=n_sub, ambiguous=n_amb, nm_derived=derived)
                for key, v in (("cols", cols), ("match", match), ("sub", n_sub), ("ambiguous", n_amb), ("ins", ins), ("del", dele),
                               ("ins_events", int(((code == 1) & (lens > 0)).sum())), ("del_events", int(((code == 2) & (lens > 0)).sum())),
                               ("soft", soft), ("hard", hard)):
                    totals[key] += v
                if cols >= 1:
                    identity = match * 1000000 // cols
                    arr["hist_identity"][identity // 1000] += 1
                    totals["identity_sum"] += identity
                    line["identity_ppm"] = identity
                counts["no_nm" if nm is None or nm < 0 else "nm_unchecked" if n_amb > 0 else "nm_agree" if nm == derived else "nm_differ"] += 1
            fields = [str(line[k]) if k in line else "*" for k in ("length", "cols", "match", "sub", "ambiguous", "ins", "del", "soft", "nm_tag",
                                                                  "nm_derived", "identity_ppm")]
            text.append(rec["name"] + ("\t%s\t" % cls + "\t".join(fields) + "\n").encode("ascii"))
    cl, tl = [int(counts[n]) for n in COUNT_NAMES], [int(totals[n]) for n in TOTAL_NAMES]
    lists = [[int(v) for v in arr[name]] for name, _ in ARRAYS]
    return Result(cl, tl, *lists, fit(arr["hp_cols"], arr["hp_del"]), b"".join(text), report(cl, tl, *lists))


def errors(streams, genome, ref_names=None, min_mapq=0, exclude_flags=0x900):
    """streams: one inflated stream, or a list of them; genome: a list of (name, sequence lines)"""
    if isinstance(streams, (bytes, bytearray)):
        streams = [streams]
    return errors_parsed([parse(s) for s in streams], genome, ref_names, min_mapq, exclude_flags)
