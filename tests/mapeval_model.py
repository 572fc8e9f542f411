"""The rule of `pbsim --eval-bam` (pbsim_truth_bam_eval) in plain Python: a mapper's BAM scored against truth BAMs, the way
`paftools mapeval` scores a PAF against the read names of a simulator.  This file is the contract; the product's kernels
(pbsim3_amd/csrc/bam_eval.hip) must give the same counts, histogram, verdict bytes and report text, byte for byte.  It reads
inflated BAM streams (SAMv1 4.2) and shares no code with the product.

    parse(stream)                                   -> ([reference name, ...], [record dict, ...])
    evaluate(truths, query, ref_names, permille)    -> (counts[12], hist[256][2], verdict bytes)
    report(counts, hist)                            -> the report text

The rule.  References are matched by NAME (the bytes in front of the NUL), never by refID; a truth file may be given another
name for its reference, legal only when it has exactly one.  Reads are matched by read name (the l_read_name - 1 bytes in front
of the NUL) over all truth files; a name that occurs twice in the truth is refused (DuplicateName).  A query record with
flag & 0x100 is secondary, else with flag & 0x800 supplementary, else primary.  A primary whose name the truth does not have
is unknown.  Of the known primaries of one name the one at the smallest offset of the inflated stream is the first, the others
are duplicates.  A first primary with flag & 4 or refID < 0 is unmapped, every other one is scored: correct when the reference
names are equal, flag & 16 is equal and the intervals overlap enough, else wrong.  The interval of a record is
[pos, pos + max(1, span)), span the sum of its CIGAR's M, D, N, = and X lengths; with inter = min(te, qe) - max(ts, qs) and
union = max(te, qe) - min(ts, qs), enough is inter > 0 and inter * 1000 >= permille * union."""
import struct

COUNT_NAMES = ["truth_records", "query_records", "primary", "secondary", "supplementary", "unknown", "duplicate", "unmapped",
               "scored", "correct", "wrong", "missing"]
MISSING, UNMAPPED, WRONG, CORRECT = 0, 1, 2, 3
_REF_OPS = {0, 2, 3, 7, 8}          # M D N = X of "MIDNSHP=X"


class DuplicateName(Exception):
    """a read name occurs twice in the truth: .name, .files (the two truth file numbers, in order of occurrence)"""

    def __init__(self, name, first_file, second_file):
        Exception.__init__(self, "%r occurs in truth file %d and in truth file %d" % (name, first_file, second_file))
        self.name, self.files = name, (first_file, second_file)


def parse(stream):
    """the references' names and the records of an inflated BAM stream; a record: offset, name, flag, ref_id, pos, mapq, span"""
    assert stream[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", stream, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", stream, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", stream, at)
        refs.append(stream[at + 4:at + 4 + l_name].split(b"\0")[0])
        at += 8 + l_name
    recs = []
    while at < len(stream):
        block_size, ref_id, pos, l_read_name, mapq, _bin, n_cigar_op, flag = struct.unpack_from("<IiiBBHHH", stream, at)
        name = stream[at + 36:at + 36 + l_read_name - 1]
        ops = struct.unpack_from("<%dI" % n_cigar_op, stream, at + 36 + l_read_name)
        span = sum(v >> 4 for v in ops if v & 15 in _REF_OPS)
        recs.append(dict(offset=at, name=name, flag=flag, ref_id=ref_id, pos=pos, mapq=mapq, span=span))
        at += 4 + block_size
    assert at == len(stream)
    return refs, recs


def interval(rec):
    return rec["pos"], rec["pos"] + max(1, rec["span"])


def overlaps(t, q, permille):
    """the third condition of `correct`, on two intervals"""
    inter = min(t[1], q[1]) - max(t[0], q[0])
    union = max(t[1], q[1]) - min(t[0], q[0])
    return inter > 0 and inter * 1000 >= permille * union


def evaluate_parsed(truths, query, ref_names=None, permille=100):
    """truths: [(reference names, records), ...]; query: (reference names, records); ref_names: None, or per truth file a name
    (bytes) or None"""
    ref_names = list(ref_names) if ref_names is not None else [None] * len(truths)
    assert len(ref_names) == len(truths) >= 1
    slot = {}                       # read name -> (truth record number, its file)
    truth = []                      # per truth record: (reference name, record)
    for f, ((names, recs), over) in enumerate(zip(truths, ref_names)):
        if over is not None:
            if len(names) != 1:
                raise ValueError("truth file %d has %d references: a reference name can be given to a file with exactly one" % (f, len(names)))
            names = [over]
        for r in recs:
            if r["name"] in slot:
                raise DuplicateName(r["name"], slot[r["name"]][1], f)
            slot[r["name"]] = (len(truth), f)
            truth.append((names[r["ref_id"]], r))
    q_names, q_recs = query
    counts = dict.fromkeys(COUNT_NAMES, 0)
    counts["truth_records"], counts["query_records"] = len(truth), len(q_recs)
    first = {}
    for r in sorted(q_recs, key=lambda r: r["offset"]):
        if r["flag"] & 0x100:
            counts["secondary"] += 1
        elif r["flag"] & 0x800:
            counts["supplementary"] += 1
        else:
            counts["primary"] += 1
            if r["name"] not in slot:
                counts["unknown"] += 1
            elif slot[r["name"]][0] in first:
                counts["duplicate"] += 1
            else:
                first[slot[r["name"]][0]] = r
    hist = [[0, 0] for _ in range(256)]
    verdicts = bytearray(len(truth))
    for k, (t_ref, t) in enumerate(truth):
        q = first.get(k)
        if q is None:
            counts["missing"] += 1
            verdicts[k] = MISSING
        elif q["flag"] & 4 or q["ref_id"] < 0:
            counts["unmapped"] += 1
            verdicts[k] = UNMAPPED
        else:
            good = q_names[q["ref_id"]] == t_ref and (q["flag"] & 16) == (t["flag"] & 16) and overlaps(interval(t), interval(q), permille)
            counts["scored"] += 1
            counts["correct" if good else "wrong"] += 1
            hist[q["mapq"]][0] += 1
            hist[q["mapq"]][1] += not good
            verdicts[k] = CORRECT if good else WRONG
    return [counts[n] for n in COUNT_NAMES], hist, bytes(verdicts)


def evaluate(truth_streams, query_stream, ref_names=None, permille=100):
    return evaluate_parsed([parse(t) for t in truth_streams], parse(query_stream), ref_names, permille)


def report(counts, hist):
    """integers only: the counts, then per MAPQ with scored records, from 255 down: MAPQ, records, wrong ones, both summed from
    255 down to here, wrong per million of the summed records, summed records per million truth records"""
    out = ["#" + "".join(" %s=%d" % (n, v) for n, v in zip(COUNT_NAMES, counts)) + "\n"]
    cum_n = cum_w = 0
    for q in range(255, -1, -1):
        n, w = hist[q]
        if n == 0:
            continue
        cum_n += n
        cum_w += w
        out.append("Q\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (q, n, w, cum_n, cum_w, cum_w * 1000000 // cum_n, cum_n * 1000000 // counts[0]))
    return "".join(out).encode("ascii")
