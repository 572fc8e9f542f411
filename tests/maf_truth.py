"""Expected read arrays (include/pbsim3_amd.h, pbsim_read_arrays) derived from the text a run wrote: FASTQ (pass_num 1)
or SAM (pass_num > 1) records plus the MAF blocks, both in read order.  The rule for ref_pos, from one MAF block: with
`start` and `span` from its reference line and q the read length, walk the columns j in order; c_j = start + the
non-'-' reference bytes before j, k_j = the non-'-' read bytes before j.  Every column whose read byte is not '-' holds
read base i = k_j ('+') or q - 1 - k_j ('-'), and ref_pos[i] = c_j, or -1 where the reference byte is '-'."""
import numpy as np


def parse_reads(text: bytes, pass_num: int):
    """[(id, seq, qual)] of the FASTQ or SAM records, in order"""
    out = []
    lines = text.split(b"\n")
    if pass_num == 1:
        for i in range(0, len(lines) - 3, 4):
            assert lines[i][:1] == b"@" and lines[i + 2][:1] == b"+", lines[i:i + 4]
            out.append((lines[i][1:], lines[i + 1], lines[i + 3]))
        return out
    for ln in lines:
        if not ln or ln[:1] == b"@":
            continue
        f = ln.split(b"\t")
        out.append((f[0], f[9], f[10]))
    return out


def parse_maf(text: bytes):
    """[(ref_name, start, size, ref_row, read_name, read_strand, read_row)] of the MAF blocks, in order"""
    out = []
    for block in text.split(b"\n\n"):
        if not block.strip():
            continue
        ln = block.split(b"\n")
        assert ln[0] == b"a", ln[0]
        # "s <name> <start> <size> <strand> <srcsize> <row>", read from the right: a template's name may hold spaces
        r = ln[1].split()
        q = ln[2].split()
        assert r[0] == b"s" and q[0] == b"s" and r[-3] == b"+"
        out.append((b" ".join(r[1:-5]), int(r[-5]), int(r[-4]), r[-1], b" ".join(q[1:-5]), q[-3], q[-1]))
    return out


def block_ref_pos(start: int, span: int, strand: bytes, ref_row: bytes, read_row: bytes):
    """ref_pos of one task from its MAF block (the rule in the module's docstring)"""
    ref = np.frombuffer(ref_row, dtype=np.uint8)
    rd = np.frombuffer(read_row, dtype=np.uint8)
    assert ref.size == rd.size
    ref_gap, rd_gap = ref == ord("-"), rd == ord("-")
    c = start + np.concatenate(([0], np.cumsum(~ref_gap)[:-1]))
    k = np.concatenate(([0], np.cumsum(~rd_gap)[:-1]))
    q = int((~rd_gap).sum())
    assert int((~ref_gap).sum()) == span
    i = k[~rd_gap] if strand == b"+" else q - 1 - k[~rd_gap]
    pos = np.empty(q, dtype=np.int32)
    pos[i] = np.where(ref_gap[~rd_gap], -1, c[~rd_gap])
    return pos


def read_id_numbers(rid: bytes, pass_num: int):
    """(read number, pass) of an id: "<prefix>[<rec>]_<n>" or "<prefix>[<rec>]/<n>/<h>" (pbsim.cpp:4013, 4016)"""
    if pass_num > 1:
        f = rid.split(b"/")
        return int(f[-2]), int(f[-1])
    return int(rid.rsplit(b"_", 1)[1]), 0


def expected_arrays(read_text: bytes, maf_text: bytes, pass_num: int):
    """dict of numpy arrays (the per-task and per-base arrays, offsets included) plus 'ref_name' (per task, bytes) and
    'maf_ins' / 'maf_del' (the gap columns of each block: '-' in the reference / in the read line)"""
    reads = parse_reads(read_text, pass_num)
    blocks = parse_maf(maf_text)
    assert len(reads) == len(blocks), (len(reads), len(blocks))
    seq, qual, pos = [], [], []
    meta = {k: [] for k in ("read_number", "pass_index", "strand", "ref_start", "ref_span", "maf_ins", "maf_del")}
    names, lens = [], []
    for (rid, s, ql), (rname, start, span, rrow, qname, strand, qrow) in zip(reads, blocks):
        assert rid == qname, (rid, qname)
        assert len(s) == len(ql)
        if strand == b"+":     # (a '-' read line is the reverse complement of the read)
            assert qrow.replace(b"-", b"") == s, rid
        n, h = read_id_numbers(rid, pass_num)
        p = block_ref_pos(start, span, strand, rrow, qrow)
        assert p.size == len(s)
        seq.append(np.frombuffer(s, dtype=np.uint8))
        qual.append(np.frombuffer(ql, dtype=np.uint8) - 33)
        pos.append(p)
        lens.append(len(s))
        names.append(rname)
        meta["read_number"].append(n)
        meta["pass_index"].append(h)
        meta["strand"].append(0 if strand == b"+" else 1)
        meta["ref_start"].append(start)
        meta["ref_span"].append(span)
        meta["maf_ins"].append(rrow.count(b"-"))
        meta["maf_del"].append(qrow.count(b"-"))
    cat = (lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt))
    out = dict(seq=cat(seq, np.uint8), qual=cat(qual, np.uint8), ref_pos=cat(pos, np.int32),
               offsets=np.concatenate(([0], np.cumsum(np.asarray(lens, dtype=np.int64)))).astype(np.int64),
               ref_name=names)
    dt = dict(read_number=np.int64, pass_index=np.int32, strand=np.uint8, ref_start=np.int64, ref_span=np.int32,
              maf_ins=np.int64, maf_del=np.int64)
    for k, v in meta.items():
        out[k] = np.asarray(v, dtype=dt[k])
    return out

