"""The aligned BAM record of one task (pbsim_set_truth_bam, include/pbsim3_amd.h) stated with numpy from the task's MAF block:
what tests/bam_spec_reader.py must read back from the record the GPU wrote.  The rules, from the MAF block
(ref_name, start, span, ref_row, read_name, strand, read_row) of tests/maf_truth.parse_maf:

  CIGAR   the MAF lines are in reference orientation already, so the columns are taken in order: '-' on the reference line
          is I, '-' on the read line is D, anything else M; maximal runs of one class, leading and trailing I / D runs kept.
          More than 65535 runs: the record carries <q>S<span>N and the runs go into a CG:B,I tag (len << 4 | op) behind NM.
  SEQ     the read line without its '-' (for a '-' task that is the reverse complement of the FASTQ sequence), each byte as
          the BAM nibble's letter (anything outside "=ACMGRSVTWYHKDBN" reads back as N)
  QUAL    the record's phred values in the same orientation: as they are on '+', reversed on '-'; zeros without a quality
          (ERRHMM: its quality line is all '!')
  pos     the reference line's start; bin = reg2bin(pos, pos + span); flag 0 / 16; mapq 60; no mate
  SN      a unit's MAF name up to its first whitespace byte
  NM      n_sub + n_ins + n_del of the task.  From the block alone: the I and D columns plus the M columns whose two bytes
          differ (a substitution draws from the other bases, pbsim.cpp:3938-3950; tests with the walk's own counters
          at hand compare those as well)
"""
import numpy as np

OPS = "MID"
MAX_OPS = 65535
NT16 = "=ACMGRSVTWYHKDBN"


def column_classes(ref_row: bytes, read_row: bytes):
    """0 M, 1 I, 2 D per MAF column"""
    ref = np.frombuffer(ref_row, dtype=np.uint8)
    rd = np.frombuffer(read_row, dtype=np.uint8)
    assert ref.size == rd.size
    return np.where(ref == ord("-"), 1, np.where(rd == ord("-"), 2, 0)).astype(np.int8)


def runs_of(cls):
    """[(length, op letter)] of the maximal runs of a class array"""
    n = cls.size
    if n == 0:
        return []
    first = np.flatnonzero(np.concatenate(([True], cls[1:] != cls[:-1])))
    length = np.diff(np.concatenate((first, [n])))
    return [(int(k), OPS[int(c)]) for k, c in zip(length, cls[first])]


def cigar_runs(ref_row: bytes, read_row: bytes):
    return runs_of(column_classes(ref_row, read_row))


def runs_by_loop(ref_row: bytes, read_row: bytes):
    """the same, one column at a time (the check of runs_of)"""
    out = []
    for r, q in zip(ref_row, read_row):
        op = "I" if r == ord("-") else "D" if q == ord("-") else "M"
        if out and out[-1][1] == op:
            out[-1][0] += 1
        else:
            out.append([1, op])
    return [(k, op) for k, op in out]


def reg2bin(beg: int, end: int) -> int:
    """SAMv1 5.3: the bin of the zero-based half-open interval [beg, end).  Level l (0 .. 5) has 8^l bins of 2^(29 - 3 l)
    bases, numbered from (8^l - 1) / 7; an interval belongs to the deepest level on which one bin holds it whole."""
    last = end - 1
    for level in (5, 4, 3, 2, 1):
        shift = 29 - 3 * level
        if beg >> shift == last >> shift:
            return (8 ** level - 1) // 7 + (beg >> shift)
    return 0


def sn_cut(name: bytes) -> bytes:
    """a reference name as a FASTA indexer keeps it: up to the first whitespace byte"""
    for i, ch in enumerate(name):
        if ch in b" \t\n\v\f\r":
            return name[:i]
    return name


def smallest_int_type(v: int) -> str:
    return "C" if v < 1 << 8 else "S" if v < 1 << 16 else "I"


def maf_nm(ref_row: bytes, read_row: bytes) -> int:
    ref = np.frombuffer(ref_row, dtype=np.uint8)
    rd = np.frombuffer(read_row, dtype=np.uint8)
    cls = column_classes(ref_row, read_row)
    return int((cls != 0).sum() + ((cls == 0) & (ref != rd)).sum())


def record(block, ref_id=0, qual=None, nm=None, max_ops=MAX_OPS):
    """the alignment dict bam_spec_reader.read_bam returns for the task of one MAF block.  qual: the phred+33 bytes of the
    task's FASTQ / SAM record (read orientation) or None (zeros); nm: the walk's n_sub + n_ins + n_del if known"""
    _, start, span, ref_row, read_name, strand, read_row = block
    runs = cigar_runs(ref_row, read_row)
    seq = read_row.replace(b"-", b"").decode("ascii").upper()
    seq = "".join(c if c in NT16 else "N" for c in seq)
    q = len(seq)
    assert sum(k for k, op in runs if op != "D") == q and sum(k for k, op in runs if op != "I") == span
    if qual is None:
        ph = bytes(q)
    else:
        ph = bytes(b - 33 for b in (qual if strand == b"+" else qual[::-1]))
    assert len(ph) == q
    nm = maf_nm(ref_row, read_row) if nm is None else int(nm)
    aux = [("NM", smallest_int_type(nm), nm)]
    cigar = runs
    if len(runs) > max_ops:
        aux.append(("CG", "BI", [(k << 4) | OPS.index(op) for k, op in runs]))
        cigar = [(q, "S"), (span, "N")]
    name = read_name.decode("ascii")
    return {"refID": ref_id, "pos": start, "l_read_name": len(name) + 1, "mapq": 60, "bin": reg2bin(start, start + span) & 0xffff,
            "n_cigar_op": len(cigar), "flag": 0 if strand == b"+" else 16, "l_seq": q, "next_refID": -1, "next_pos": -1,
            "tlen": 0, "read_name": name, "cigar": cigar, "seq": seq, "qual": ph, "aux": aux}


def header_text(refs, version: str) -> bytes:
    """refs: [(SN bytes, LN)]"""
    t = b"@HD\tVN:1.6\tSO:unknown\n"
    for sn, ln in refs:
        t += b"@SQ\tSN:" + sn + b"\tLN:" + str(ln).encode() + b"\n"
    return t + b"@PG\tID:pbsim3_amd\tPN:pbsim3_amd\tVN:" + version.encode() + b"\n"
