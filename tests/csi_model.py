"""A plain model of `--truth-sort coordinate` (pbsim_truth_bam_sort), written from SAMv1 (4.1 BGZF, 4.2 BAM, 5.3 reg2bin)
and the CSIv1 text, not from the C++: what the sorted file and its .csi index must be, byte for byte, and a region query that
uses nothing but the index.  Test infrastructure: no samtools here.

    members(raw)                      -> [(coffset, csize, text)] of a BGZF file, framing / CRC / ISIZE / EOF block checked
    split_stream(stream)              -> (header bytes, l_text, text, refs, [record bytes]) by walking the block_size chain
    fields(rec)                       -> (refID, pos, end): end = pos + reference span of the CIGAR, pos + 1 where that is 0
    stable_sort(records)              -> the records by (refID, pos), ties in input order
    sorted_header(header)             -> the header with SO:coordinate in its @HD line
    reg2bin / reg2bins                -> CSIv1's functions, any depth
    csi_bytes(refs, records, header_len, member_table) -> the index of a file whose members are `member_table`
    read_csi(raw)                     -> dict
    query(index, raw_bam, ref, beg, end) -> the records that overlap [beg, end), found through the index alone
    brute(records, ref, beg, end)     -> the same by looking at every record
"""
import bisect
import struct
import zlib

MIN_SHIFT = 14
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def le(buf, at, n, signed=False):
    return int.from_bytes(buf[at:at + n], "little", signed=signed)


# ---------------------------------------------------------------- BGZF (SAMv1 4.1)
def members(raw):
    """every member: gzip magic, CM 8, FLG 4, XLEN 6, the BC subfield with BSIZE = size - 1 <= 65535, a raw deflate stream
    that ends at the trailer, CRC-32 and ISIZE <= 65536 of the text; the last member is the 28-byte EOF block"""
    out, at = [], 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04", "member magic at %d" % at
        assert raw[at + 10:at + 16] == b"\x06\x00BC\x02\x00", "BC subfield at %d" % at
        size = le(raw, at + 16, 2) + 1
        assert at + size <= len(raw)
        d = zlib.decompressobj(-15)
        text = d.decompress(raw[at + 18:at + size - 8])
        assert d.eof and d.unused_data == b"", "deflate stream and trailer at %d" % at
        assert le(raw, at + size - 8, 4) == zlib.crc32(text) and le(raw, at + size - 4, 4) == len(text) <= 65536
        out.append((at, size, text))
        at += size
    assert out and raw.endswith(EOF_BLOCK) and out[-1][2] == b"", "no EOF block"
    return out


def member_table(raw):
    """[(coffset, text length)] of every member, the EOF block included"""
    return [(c, len(t)) for c, _, t in members(raw)]


def inflate(raw):
    return b"".join(t for _, _, t in members(raw))


# ---------------------------------------------------------------- BAM (SAMv1 4.2)
def split_stream(stream):
    assert stream[:4] == b"BAM\x01"
    l_text = le(stream, 4, 4)
    text = stream[8:8 + l_text]
    at = 8 + l_text
    n_ref = le(stream, at, 4)
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = le(stream, at, 4)
        refs.append((stream[at + 4:at + 4 + l_name - 1], le(stream, at + 4 + l_name, 4)))
        at += 8 + l_name
    header = stream[:at]
    recs = []
    while at < len(stream):
        size = 4 + le(stream, at, 4)
        assert at + size <= len(stream), "record runs past the end"
        recs.append(stream[at:at + size])
        at += size
    return header, l_text, text, refs, recs


REF_OPS = {0, 2, 3, 7, 8}       # M D N = X of "MIDNSHP=X" consume the reference (SAMv1 1.4.6)


def fields(rec):
    ref_id, pos, l_name = le(rec, 4, 4, True), le(rec, 8, 4, True), rec[12]
    n_op = le(rec, 16, 2)
    span = 0
    for k in range(n_op):
        v = le(rec, 36 + l_name + 4 * k, 4)
        if v & 15 in REF_OPS:
            span += v >> 4
    return ref_id, pos, pos + (span if span > 0 else 1)


def name_of(rec):
    return bytes(rec[36:36 + rec[12] - 1])


def stable_sort(records):
    return sorted(records, key=lambda r: fields(r)[:2])      # (sorted() is stable)


def sorted_header(header):
    l_text = le(header, 4, 4)
    text, rest = header[8:8 + l_text], header[8 + l_text:]
    if text[:3] == b"@HD" and text[3:4] in (b"\t", b"\n", b""):
        eol = text.find(b"\n")
        eol = len(text) if eol < 0 else eol
        line = text[:eol].split(b"\t")
        if any(f.startswith(b"SO:") for f in line):
            line = [b"SO:coordinate" if f.startswith(b"SO:") else f for f in line]
        else:
            line.append(b"SO:coordinate")
        text = b"\t".join(line) + text[eol:]
    else:
        text = b"@HD\tVN:1.6\tSO:coordinate\n" + text
    return b"BAM\x01" + struct.pack("<i", len(text)) + text + rest


# ---------------------------------------------------------------- CSIv1
def depth_for(longest):
    d = 5
    while (1 << (MIN_SHIFT + 3 * d)) < longest:
        d += 1
    return d


def reg2bin(beg, end, min_shift=MIN_SHIFT, depth=5):
    """the specification's C function: the loop steps from the deepest level up; t is the first bin of the level"""
    end -= 1
    s, t = min_shift, ((1 << depth * 3) - 1) // 7
    level = depth
    while level > 0:
        if beg >> s == end >> s:
            return t + (beg >> s)
        level -= 1
        s += 3
        t -= 1 << level * 3
    return 0


def reg2bins(beg, end, min_shift=MIN_SHIFT, depth=5):
    """every bin that may hold a record overlapping [beg, end)"""
    out = []
    end -= 1
    s, t = min_shift + depth * 3, 0
    for level in range(depth + 1):
        out.extend(range(t + (beg >> s), t + (end >> s) + 1))
        s -= 3
        t += 1 << level * 3
    return out


def bin_level_start(b, min_shift=MIN_SHIFT, depth=5):
    """(level, first coordinate) of bin b"""
    level, t = 0, 0
    while b >= t + (1 << 3 * level):
        t += 1 << 3 * level
        level += 1
    return level, (b - t) << (min_shift + 3 * (depth - level))


def pseudo_bin(depth):
    return ((1 << 3 * (depth + 1)) - 1) // 7 + 1


class Offsets:
    """virtual offsets in a file whose members are table = [(coffset, text length)], the last one the EOF block"""

    def __init__(self, table):
        self.starts, self.coffsets, self.start_of, at = [], [], {}, 0
        for c, n in table:
            self.start_of[c] = at
            if n:                               # a byte is HELD by a member with text: the low part stays below its length
                self.starts.append(at)
                self.coffsets.append(c)
            at += n
        self.total = at
        self.eof = table[-1][0]

    def voffset(self, o):
        """of the record that starts at byte o of the inflated file; behind the last record: the EOF block"""
        if o >= self.total:
            return self.eof << 16
        m = bisect.bisect_right(self.starts, o) - 1
        return self.coffsets[m] << 16 | (o - self.starts[m])

    def stream_offset(self, v):
        return self.start_of[v >> 16] + (v & 0xffff)


def csi_bytes(refs, records, header_len, table):
    """refs: [(name, length)]; records: the file's records in file order; table: member_table() of the file under test"""
    depth = depth_for(max([ln for _, ln in refs] + [0]))
    off = Offsets(table)
    starts, at = [], header_len
    for r in records:
        starts.append(at)
        at += len(r)
    starts.append(at)
    assert at == off.total
    f = [fields(r) for r in records]
    out = [b"CSI\x01", struct.pack("<iiii", MIN_SHIFT, depth, 0, len(refs))]
    i = 0
    for ref in range(len(refs)):
        a = i
        while i < len(records) and f[i][0] == ref:
            i += 1
        if i == a:
            out.append(struct.pack("<i", 0))
            continue
        bins = {}
        k = a
        while k < i:                                   # maximal runs of one bin, consecutive in file order
            b = reg2bin(f[k][1], f[k][2], MIN_SHIFT, depth)
            e = k
            while e < i and reg2bin(f[e][1], f[e][2], MIN_SHIFT, depth) == b:
                e += 1
            bins.setdefault(b, []).append((off.voffset(starts[k]), off.voffset(starts[e])))
            k = e
        out.append(struct.pack("<i", len(bins) + 1))
        for b in sorted(bins):
            _, s = bin_level_start(b, MIN_SHIFT, depth)
            first = next(k for k in range(a, i) if f[k][2] > s)
            out.append(struct.pack("<IQi", b, off.voffset(starts[first]), len(bins[b])))
            out.extend(struct.pack("<QQ", x, y) for x, y in bins[b])
        out.append(struct.pack("<IQi", pseudo_bin(depth), 0, 2))
        out.append(struct.pack("<QQQQ", off.voffset(starts[a]), off.voffset(starts[i]), i - a, 0))
    assert i == len(records), "records beyond the last reference, or not sorted by refID"
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def read_csi(raw):
    assert raw[:4] == b"CSI\x01"
    min_shift, depth, l_aux = struct.unpack_from("<iii", raw, 4)
    at = 16 + l_aux
    n_ref = le(raw, at, 4)
    at += 4
    refs = []
    for _ in range(n_ref):
        n_bin = le(raw, at, 4)
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, loff, n_chunk = struct.unpack_from("<IQi", raw, at)
            at += 16
            chunks = [struct.unpack_from("<QQ", raw, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            assert b not in bins
            bins[b] = (loff, chunks)
        refs.append(bins)
    n_no_coor = le(raw, at, 8) if at < len(raw) else None
    assert at + (8 if n_no_coor is not None else 0) == len(raw)
    return dict(min_shift=min_shift, depth=depth, refs=refs, n_no_coor=n_no_coor)


def query(index, raw_bam, ref, beg, end, table=None):
    """the names of the records on `ref` that overlap [beg, end), through the index alone: the bins of reg2bins, the loffset
    of the bin of the query's start (its deepest ancestor that the index has) to drop chunks that end before it, a seek to
    every chunk that is left (table: members(raw_bam), for a caller that asks often)"""
    bins = index["refs"][ref]
    depth, ms = index["depth"], index["min_shift"]
    if not bins or end <= beg:
        return []
    min_off = 0
    b = ((1 << depth * 3) - 1) // 7 + (beg >> ms)       # the leaf bin of beg
    while True:
        if b in bins:
            min_off = bins[b][0]
            break
        if b == 0:
            break
        b = (b - 1) >> 3                                    # its parent
    chunks = []
    for b in reg2bins(beg, end, ms, depth):
        if b in bins:
            chunks.extend(c for c in bins[b][1] if c[1] > min_off)
    table = table or members(raw_bam)
    stream = b"".join(t for _, _, t in table)
    off = Offsets([(c, len(t)) for c, _, t in table])
    found = []
    for cb, ce in sorted(set(chunks)):
        at, stop = off.stream_offset(cb), off.stream_offset(ce)
        while at < stop:
            size = 4 + le(stream, at, 4)
            rec = stream[at:at + size]
            r, p, e = fields(rec)
            if r == ref and p < end and e > beg:
                found.append((at, name_of(rec)))
            at += size
        assert at == stop, "a chunk does not end on a record boundary"
    return [n for _, n in sorted(set(found))]


def brute(records, ref, beg, end):
    out = []
    for rec in records:
        r, p, e = fields(rec)
        if r == ref and p < end and e > beg and end > beg:
            out.append(name_of(rec))
    return out


# ---------------------------------------------------------------- building inputs
def record(ref_id, pos, name, cigar, l_seq, seq=None, qual=None, aux=b"", flag=0, mapq=60, bin_field=0):
    """one placed single-end record; cigar: [(length, op letter)]"""
    ops = b"".join(struct.pack("<I", n << 4 | "MIDNSHP=X".index(op)) for n, op in cigar)
    seq = bytes((l_seq + 1) // 2) if seq is None else seq
    qual = bytes(l_seq) if qual is None else qual
    assert len(seq) == (l_seq + 1) // 2 and len(qual) == l_seq and len(cigar) < 65536
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) + 1, mapq, bin_field, len(cigar), flag, l_seq, -1, -1, 0) + \
        name + b"\0" + ops + seq + qual + aux
    return struct.pack("<I", len(body)) + body


def header(refs, text=None):
    if text is None:
        text = b"@HD\tVN:1.6\tSO:unknown\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in refs) + b"@PG\tID:model\n"
    return b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs)) + \
        b"".join(struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", ln) for n, ln in refs)
