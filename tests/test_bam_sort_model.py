"""tests/csi_model.py against values worked out by hand from SAMv1 5.3 and the CSIv1 text, its index query against a scan of
every record, and the two places where `--truth-sort coordinate` shows without a GPU: the ABI's declaration with its ctypes
mirror, and the option mirror."""
import os
import random
import re

import pytest

import bam_spec_reader as R
import bgzf_writer as W
import csi_model as M
import harness
import pbsim3_amd as P
from pbsim3_amd import args as A


# ---------------------------------------------------------------- literals
def test_reg2bin_at_depth_5_is_samv1_5_3():
    """the six levels of the BAI scheme: 16 kb bins from 4681, 128 kb from 585, 1 Mb from 73, 8 Mb from 9, 64 Mb from 1, bin 0"""
    assert M.reg2bin(0, 1) == 4681 and M.reg2bin(16383, 16384) == 4681 and M.reg2bin(16384, 16385) == 4682
    assert M.reg2bin(16383, 16385) == 585                       # across a 16 kb boundary: the 128 kb bin
    assert M.reg2bin((1 << 17) - 1, (1 << 17) + 1) == 73        # across a 128 kb boundary: the 1 Mb bin
    assert M.reg2bin((1 << 20) - 1, (1 << 20) + 1) == 9
    assert M.reg2bin((1 << 23) - 1, (1 << 23) + 1) == 1
    assert M.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0
    assert M.reg2bin((1 << 29) - 1, 1 << 29) == 4681 + 32767    # the last leaf
    rng = random.Random(5)
    for _ in range(2000):
        beg = rng.randrange(1 << 29)
        end = min(1 << 29, beg + 1 + rng.choice([0, 3, 20000, 200000, 3 << 20, 100 << 20]))
        assert M.reg2bin(beg, end) == R.reg2bin(beg, end)
        assert M.reg2bin(beg, end) in M.reg2bins(beg, end)


def test_reg2bin_at_depth_6():
    """seven levels over 2^32: the leaves start at (8^6 - 1) / 7 = 37449, the 128 kb bins at 37449 - 8^5 = 4681"""
    assert M.depth_for(1 << 29) == 5 and M.depth_for((1 << 29) + 1) == 6 and M.depth_for(2_000_000_000) == 6 and M.depth_for(0) == 5
    assert M.reg2bin(0, 1, 14, 6) == 37449
    assert M.reg2bin((1 << 30) + 5, (1 << 30) + 6, 14, 6) == 37449 + 65536
    assert M.reg2bin(16383, 16385, 14, 6) == 4681
    assert M.reg2bin((1 << 29) - 1, (1 << 29) + 1, 14, 6) == 0
    assert M.pseudo_bin(5) == 37450 and M.pseudo_bin(6) == 299594
    assert M.bin_level_start(37449 + 65536, 14, 6) == (6, 1 << 30) and M.bin_level_start(4682, 14, 6) == (5, 1 << 17)
    assert M.reg2bins(0, 1, 14, 6) == [0, 1, 9, 73, 585, 4681, 37449]


def test_whole_index_of_a_two_record_file():
    """two references of 1000 and 2000 bases (depth 5), record A (50 bytes) on the first at 100..150, record B (70 bytes) on the
    second at 5..10; the file: a header member at 0 (60 bytes of text), the records' member at 100, the EOF block at 180.
    Virtual offsets: A 100 << 16, B 100 << 16 | 50, end of file 180 << 16.  Both records lie in leaf 4681.  Per reference: the
    bin (loffset = its only record), one chunk, then pseudo-bin 37450 with the same span and (1 mapped, 0 unmapped)."""
    want = bytes.fromhex(
        "435349010e00000005000000000000000200000002000000491200000000640000000000010000000000640000000000"
        "32006400000000004a920000000000000000000002000000000064000000000032006400000000000100000000000000"
        "0000000000000000020000004912000032006400000000000100000032006400000000000000b400000000004a920000"
        "00000000000000000200000032006400000000000000b400000000000100000000000000000000000000000000000000"
        "00000000")
    a = M.record(0, 100, b"A", [(50, "M")], 1, aux=bytes(50 - 44))
    b = M.record(1, 5, b"B", [(5, "M")], 1, aux=bytes(70 - 44))
    assert len(a) == 50 and len(b) == 70
    got = M.csi_bytes([(b"r0", 1000), (b"r1", 2000)], [a, b], 60, [(0, 60), (100, 120), (180, 0)])
    assert got == want
    back = M.read_csi(got)
    assert back["depth"] == 5 and back["n_no_coor"] == 0 and sorted(back["refs"][0]) == [4681, 37450]


# ---------------------------------------------------------------- the query through the index against a scan of every record
def _random_file(seed, refs, n, block):
    rng = random.Random(seed)
    recs = []
    for k in range(n):
        r = rng.choice([k for k, (name, _) in enumerate(refs) if name != b"empty"])
        ln = refs[r][1]
        span = rng.choice([1, 7, 300, 20000, 140000, 1 << 20, 9 << 20])
        pos = rng.randrange(max(1, ln - 1))
        span = max(1, min(span, ln - pos))
        cigar = [(span, "M")] if k % 3 else [(3, "S"), (span // 2 + 1, "M"), (2, "I"), (span - span // 2 - 1, "D")]
        cigar = [c for c in cigar if c[0] > 0]
        recs.append(M.record(r, pos, b"q%d" % k, cigar, rng.randrange(0, 40)))
    recs = M.stable_sort(recs)
    head = M.sorted_header(M.header(refs))
    raw = W.bgzf(head, block=block, eof=False) + W.bgzf(b"".join(recs), block=block)
    return head, recs, raw


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_query_through_the_index_finds_what_a_full_scan_finds(seed):
    refs = [(b"a", 40_000), (b"empty", 1000), (b"b", 300_000_000), (b"c", 900_000_000 if seed == 3 else 5_000_000)]
    head, recs, raw = _random_file(seed, refs, 400, block=[65280, 700, 4096][seed - 1])
    csi = M.csi_bytes(refs, recs, len(head), M.member_table(raw))
    index = M.read_csi(csi)
    assert index["depth"] == (6 if seed == 3 else 5) and index["refs"][1] == {}
    rng = random.Random(100 + seed)
    for _ in range(60):
        r = rng.randrange(len(refs))
        beg = rng.randrange(refs[r][1])
        end = beg + rng.choice([0, 1, 50, 16384, 1 << 20, refs[r][1]])
        assert M.query(index, raw, r, beg, end) == M.brute(recs, r, beg, end), (r, beg, end)
    assert any(M.brute(recs, 0, b, b + 1) for b in range(0, 40_000, 997))


# ---------------------------------------------------------------- the ABI and the option
def test_header_declares_the_call_and_the_ctypes_table_lists_it():
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        h = f.read()
    assert re.search(r"int pbsim_truth_bam_sort\(pbsim_ctx \*ctx, const void \*bam, int64_t n, const pbsim_sorted_bam_sink \*sink, "
                     r"int64_t stats\[4\]\);", h)
    assert re.search(r"typedef struct pbsim_sorted_bam_sink \{\s*void \*user;\s*int \(\*on_bam\)\(void \*user, const char \*bytes, "
                     r"int64_t n, int64_t offset\);[^\n]*\n\s*int \(\*on_index\)\(void \*user, const char \*bytes, int64_t n\);", h)
    assert "pbsim_truth_bam_sort" in [name for name, _, _ in P.API]
    assert [n for n, _ in P.SortedBamSink._fields_] == ["user", "on_bam", "on_index"]
    assert callable(getattr(P.Context, "sort_truth_bam"))


def test_option_mirror_accepts_and_rejects():
    base = ["--strategy", "wgs", "--method", "errhmm"]
    assert A.truth_sort(A.parse(base)[1]) is None
    assert A.truth_sort(A.parse(base + ["--truth-format", "bam", "--truth-sort", "coordinate"])[1]) == "coordinate"
    with pytest.raises(ValueError):
        A.truth_sort(A.parse(base + ["--truth-sort", "coordinate"])[1])
    with pytest.raises(ValueError):
        A.truth_sort(A.parse(base + ["--truth-format", "maf", "--truth-sort", "coordinate"])[1])
    with pytest.raises(ValueError):
        A.truth_sort(A.parse(base + ["--truth-format", "bam", "--truth-sort", "queryname"])[1])
