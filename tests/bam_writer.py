"""A test-side writer of general BAM files (SAMv1 4.2), independent of the product: a header with references, alignment
records from (name, flag, refID, pos, cigar, seq, qual, tags) with every optional-field type including B arrays, in the
containers of tests/bgzf_writer.py -- and `to_fastq`, the tests' stand-in for `samtools fastq` (default options) where it
matters to the sampling method: which records are reads, and what their quality lines are.

    record(name, flag=4, ref_id=-1, pos=-1, cigar=(), seq="", qual=b"", tags=(), ...)  -> a dict of the record's fields
    stream(records, refs=(), text=b"")   -> the inflated BAM bytes
    bam(records, refs=(), ..., container="bgzf", block=...)  -> the file's bytes
    to_fastq(records)                    -> the FASTQ `samtools fastq` writes from them
"""
import struct

import bgzf_writer as W

_NIBBLE = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
_CIGAR = {c: i for i, c in enumerate("MIDNSHP=X")}
_INT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
_COMPLEMENT = bytes.maketrans(b"ACGTUMRWSYKVHDBNacgtumrwsykvhdbn", b"TGCAAKYWSRMBDHVNtgcaakywsrmbdhvn")


def record(name, flag=4, ref_id=-1, pos=-1, cigar=(), seq=None, qual=b"", tags=(), mapq=0, bin=4680, next_ref_id=-1, next_pos=-1,
           tlen=0):
    """qual: the phred bytes as they lie in the record (0xFF x l_seq: none); seq defaults to 'A' x len(qual); cigar: a tuple of
    (length, op letter); tags: (tag, type, value) with type one of A c C s S i I f Z H or B<subtype>"""
    qual = bytes(qual)
    if seq is None:
        seq = "A" * len(qual)
    assert len(seq) == len(qual)
    return dict(name=name, flag=flag, ref_id=ref_id, pos=pos, cigar=tuple(cigar), seq=seq, qual=qual, tags=tuple(tags), mapq=mapq,
                bin=bin, next_ref_id=next_ref_id, next_pos=next_pos, tlen=tlen)


def tag_bytes(tag, typ, val):
    out = tag.encode("ascii") + typ[:1].encode("ascii")
    if typ == "A":
        return out + val.encode("ascii")
    if typ in _INT:
        return out + struct.pack(_INT[typ], val)
    if typ == "f":
        return out + struct.pack("<f", val)
    if typ in ("Z", "H"):
        return out + val.encode("ascii") + b"\0"
    assert typ[0] == "B" and len(typ) == 2, typ
    sub = typ[1]
    body = bytes(val) if isinstance(val, (bytes, bytearray)) and sub == "C" else \
        b"".join(struct.pack("<f" if sub == "f" else _INT[sub], v) for v in val)
    n = len(body) // (4 if sub == "f" else struct.calcsize(_INT[sub]))
    return out + sub.encode("ascii") + struct.pack("<I", n) + body


def record_bytes(r, block_size=None):
    """block_size and the record behind it; `block_size` overrides the field (malformed records)"""
    name = r["name"].encode("ascii") + b"\0"
    assert 1 <= len(name) <= 255
    seq = r["seq"]
    packed = bytearray((len(seq) + 1) // 2)
    for k, c in enumerate(seq):
        packed[k // 2] |= _NIBBLE[c] << (0 if k % 2 else 4)          # the high nibble first
    cigar = b"".join(struct.pack("<I", n << 4 | _CIGAR[op]) for n, op in r["cigar"])
    body = struct.pack("<iiBBHHHiiii", r["ref_id"], r["pos"], len(name), r["mapq"], r["bin"], len(r["cigar"]), r["flag"], len(seq),
                       r["next_ref_id"], r["next_pos"], r["tlen"])
    body += name + cigar + bytes(packed) + r["qual"] + b"".join(tag_bytes(*t) for t in r["tags"])
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def header(refs=(), text=b""):
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        n = name.encode("ascii") + b"\0"
        out += struct.pack("<i", len(n)) + n + struct.pack("<i", length)
    return out


def stream(records, refs=(), text=b""):
    return header(refs, text) + b"".join(record_bytes(r) for r in records)


def contain(data, container="bgzf", block=W.BGZIP_BLOCK):
    """the inflated bytes in a container: bgzf (members of `block` bytes), stored (BGZF, level 0), gzip (one plain member), none"""
    if container == "bgzf":
        return W.bgzf(data, block=block)
    if container == "stored":
        return W.bgzf(data, block=block, level=0)
    if container == "gzip":
        return W.plain_gzip(data)
    assert container == "none"
    return data


def bam(records, refs=(), text=b"", container="bgzf", block=W.BGZIP_BLOCK):
    return contain(stream(records, refs, text), container, block)


def to_fastq(records):
    """`samtools fastq` with default options, as far as the sampling method reads it: secondary (0x100) and supplementary
    (0x800) records are left out; a reverse-strand record (0x10) comes out in the read's own orientation, bases
    reverse-complemented and qualities reversed; a quality byte q is the character min(q, 93) + 33; a record without bases
    has empty base and quality lines"""
    out = []
    for r in records:
        if r["flag"] & 0x900:
            continue
        seq, qual = r["seq"].encode("ascii"), r["qual"]
        assert not (qual and qual[0] == 0xFF), "a record without qualities has no FASTQ line here"
        if r["flag"] & 0x10:
            seq, qual = seq.translate(_COMPLEMENT)[::-1], qual[::-1]
        out.append(b"@" + r["name"].encode("ascii") + b"\n" + seq + b"\n+\n" + bytes(min(q, 93) + 33 for q in qual) + b"\n")
    return b"".join(out)
