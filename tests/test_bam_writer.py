"""tests/bam_writer.py, the writer behind the BAM input tests, read back field by field with the specification reader
(tests/bam_spec_reader.py), and its `to_fastq` -- the tests' stand-in for `samtools fastq` -- on the rules that matter to the
sampling method: which records are reads, reversed qualities for reverse-strand records, the clamp at 93."""
import random

import pytest

import bam_spec_reader as R
import bam_writer as B

REFS = [("chr1", 100000), ("chrUn_with_a_longer_name", 5000), ("c", 77)]
TAGS = [("XA", "A", "q"), ("Xc", "c", -7), ("XC", "C", 200), ("Xs", "s", -3000), ("XS", "S", 60000), ("Xi", "i", -70000),
        ("XI", "I", 4000000000), ("Xf", "f", 0.5), ("XZ", "Z", "some text"), ("XH", "H", "1AE301"),
        ("Bc", "Bc", [-1, 2, -3]), ("BC", "BC", [0, 255, 7]), ("Bs", "Bs", [-300, 300]), ("BS", "BS", [65535, 1]),
        ("Bi", "Bi", [-70000]), ("BI", "BI", [4000000000, 0]), ("Bf", "Bf", [0.25, -1.5]), ("Be", "BC", [])]


def records():
    r = random.Random(3)
    out = []
    for i, n in enumerate([0, 1, 2, 7, 8, 33, 100]):
        seq = "".join(r.choice("ACGTN") for _ in range(n))
        qual = bytes(r.choice([0, 5, 40, 93, 94, 254]) for _ in range(n))
        if i % 3 == 0:
            out.append(B.record("unmapped/%d" % i, 4, seq=seq, qual=qual, tags=TAGS[:i]))
        else:
            out.append(B.record("m%d" % i, [0, 16, 256, 2048 | 16][i % 4], ref_id=i % 3, pos=100 * i,
                                cigar=((3, "S"), (n, "M"), (2, "D"), (1, "I")) if n else (), seq=seq, qual=qual, mapq=i,
                                next_ref_id=(i + 1) % 3, next_pos=5, tlen=-40, tags=TAGS[i:]))
    out.append(B.record("n" * 254, 4, qual=bytes([255] * 5)))
    return out


@pytest.mark.parametrize("container,block", [("bgzf", 65280), ("bgzf", 300), ("stored", 1000)])
def test_written_files_read_back_field_by_field(container, block):
    recs = records()
    text, refs, got = R.read_bam(B.bam(recs, REFS, b"@HD\tVN:1.6\tSO:unsorted\n", container, block))
    assert text == b"@HD\tVN:1.6\tSO:unsorted\n" and refs == REFS and len(got) == len(recs)
    for a, r in zip(got, recs):
        assert a["read_name"] == r["name"] and a["l_read_name"] == len(r["name"]) + 1
        assert (a["flag"], a["refID"], a["pos"], a["mapq"], a["bin"]) == (r["flag"], r["ref_id"], r["pos"], r["mapq"], r["bin"])
        assert (a["next_refID"], a["next_pos"], a["tlen"]) == (r["next_ref_id"], r["next_pos"], r["tlen"])
        assert a["cigar"] == list(r["cigar"]) and a["seq"] == r["seq"] and a["qual"] == r["qual"] and a["l_seq"] == len(r["seq"])
        assert len(a["aux"]) == len(r["tags"])
        for (tag, typ, val), (t2, y2, v2) in zip(a["aux"], r["tags"]):
            assert (tag, typ) == (t2, y2)
            assert val == (pytest.approx(v2) if "f" in typ else v2), tag


def test_other_containers_hold_the_same_stream():
    import gzip
    recs = records()
    s = B.stream(recs, REFS)
    assert s[:4] == b"BAM\x01"
    assert B.bam(recs, REFS, container="none") == s
    assert gzip.decompress(B.bam(recs, REFS, container="gzip")) == s
    assert gzip.decompress(B.bam(recs, REFS, container="bgzf", block=300)) == s
    assert B.record_bytes(recs[1], block_size=12)[:4] == b"\x0c\0\0\0"


def test_to_fastq():
    fwd = B.record("f", 0, ref_id=0, pos=1, cigar=((4, "M"),), seq="ACGN", qual=bytes([0, 93, 94, 254]))
    rev = B.record("r", 16, ref_id=0, pos=1, cigar=((4, "M"),), seq="AACG", qual=bytes([1, 2, 3, 4]))
    sec = B.record("s", 256, ref_id=0, pos=1, seq="AC", qual=bytes([9, 9]))
    sup = B.record("u", 2048 | 16, ref_id=0, pos=1, seq="AC", qual=bytes([9, 9]))
    odd = B.record("o", 4 | 512 | 1024, seq="T", qual=bytes([40]))          # unmapped, QC fail, duplicate: still a read
    none = B.record("e", 4)
    assert B.to_fastq([fwd, sec, rev, sup, odd, none]) == (b"@f\nACGN\n+\n!~~~\n" b"@r\nCGTT\n+\n%$#\"\n" b"@o\nT\n+\nI\n" b"@e\n\n+\n\n")
    with pytest.raises(AssertionError):
        B.to_fastq([B.record("x", 4, qual=bytes([255, 255]))])
