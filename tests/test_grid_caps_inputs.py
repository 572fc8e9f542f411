"""What test_gpu_sample_grid_caps.py and test_gpu_inflate_grid_caps.py rely on in their inputs (grid_caps_inputs.py) and what
needs no device to be checked: that every input passes the cap it is built for, as the sources state the caps; that the records at
the seams are kept, by the stdio parse; that the seams lie where the builders mean them to; the kinds of the BGZF members by the
first three bits of their deflate data, and zlib's own inflate of them."""
import zlib

import pytest

import grid_caps_inputs as G
from test_gpu_deflate import members
from test_gpu_sample_profile import driver  # noqa: F401  (the fixture that compiles the stdio driver)


def test_the_caps_leave_inputs_of_a_size_that_a_test_can_afford():
    assert G.carry_room() % G.TILE == 0, "tile t of a first window would not begin at file offset t * kSpTile"
    assert G.WAVE_CAP * 80 < 2_000_000, "f1() and b1() would have %d records" % G.WAVE_CAP
    assert G.SCAN_CAP * 4 < 3_000_000, "f2() would have %d records" % G.SCAN_CAP
    assert G.COUNT_CAP * G.TILE < 80 << 20 and G.COUNT_CAP > G.WAVE_CAP, "f3() would have %d tiles" % G.COUNT_CAP
    assert G.COUNT_CAP * G.TILE < 1 << 30, "f3() would not fit one window"
    assert G.MEMBER_CAP * 200 < 5_000_000, "i1() would have %d members" % G.MEMBER_CAP


def kept_once(want, line):
    return want[2].count(line) == 1


def test_f1_records_past_the_pool_pass(driver, tmp_path):  # noqa: F811
    s = G.f1()
    lines = [q for _, q in s.quals]
    assert len(lines) == G.WAVE_CAP + 700 and len(s.fq) < 2_000_000 and G.tiles_of(len(s.fq)) < G.WAVE_CAP
    assert {len(q) for q in lines} == set(range(20, 101))
    in_range = G.kept_by_length(s.quals, s.filter)
    # the pool pass realigns by start & 7, the sums walk up to the first 16-byte edge, and the last word holds len % 8 bytes
    assert {(G.carry_room() + at) & 15 for at, _ in in_range} == set(range(16)) and {len(q) % 8 for _, q in in_range} == set(range(8))
    assert all(set(q) <= {33 + v for v in list(G.FRONT) + list(G.LOW)} for q in lines[:s.seam - 4])
    assert all(set(q) <= {33 + v for v in G.BEHIND} for q in lines[s.seam - 4:])
    want = G.stdio(driver, tmp_path, "f1", s.fq, s.filter)
    assert want[0][0] == len(lines) and (want[0][1], want[0][2]) == (20, 100)
    assert kept_once(want, lines[s.seam - 1]) and kept_once(want, lines[s.seam])
    kept = set(want[2])
    assert min(len(q) for q in kept) == s.filter["len_min"] and max(len(q) for q in kept) == s.filter["len_max"]
    assert 0.8 * len(lines) * 65 / 81 < want[0][4] < len(in_range)          # most are kept; some are dropped for their accuracy
    assert sum(q in kept for q in lines[s.seam:]) > 400


def test_f2_records_past_one_trip_of_the_scan(driver, tmp_path):  # noqa: F811
    s = G.f2()
    assert s.records > G.SCAN_CAP and len(s.fq) < 3_000_000
    assert s.records < 2 * G.SCAN_CAP, "a third trip: the kept records lie around the first seam only"
    want = G.stdio(driver, tmp_path, "f2", s.fq, s.filter)
    assert want[0][0] == s.records and want[0][1] == 0, "four line feeds are a record of length 0"
    assert want[2] == [s.kept[k] for k in sorted(s.kept)]
    assert {s.seam - 1, s.seam} <= set(s.kept) and sum(k < s.seam - 1 for k in s.kept) == 60 and sum(k > s.seam for k in s.kept) == 40


def seam_is(fq, at, style):
    phase, is_lf = G.line_at(fq, at)
    if style == "straddle":
        return phase == 3 and not is_lf and fq[at - 1] != G.LF
    if style == "fourth_lf":
        return phase == 3 and is_lf
    return phase == 0 and not is_lf and fq[at - 1] != G.LF


def dense_around(s, want, at, tiles=8):
    """every tile from `tiles` in front of file offset `at` to `tiles` behind it holds every line phase, and kept lines begin on
    both sides"""
    kept = set(want[2])
    for t in range(at // G.TILE - tiles, at // G.TILE + tiles):
        assert s.fq.count(b"\n", t * G.TILE, (t + 1) * G.TILE) >= 8, t
    before = sum(q in kept for o, q in s.quals if at - tiles * G.TILE <= o < at)
    behind = sum(q in kept for o, q in s.quals if at <= o < at + tiles * G.TILE)
    assert before > 50 and behind > 50, (before, behind)


@pytest.mark.parametrize("rest", sorted(G.F3_STYLES))
def test_f3_tiles_past_the_line_pass_and_the_count(driver, tmp_path, rest):  # noqa: F811
    s = G.f3(rest)
    assert G.tiles_of(len(s.fq)) == s.tiles > G.COUNT_CAP > G.WAVE_CAP and s.tiles % G.UNROLL == rest and len(s.fq) > 64 << 20
    assert s.tiles < G.COUNT_CAP + 4 * G.UNROLL and len(s.fq) % G.TILE, "the last step of the count has tiles behind the last, which is not full"
    assert s.seams == [G.WAVE_CAP * G.TILE, G.COUNT_CAP * G.TILE]
    want = G.stdio(driver, tmp_path, "f3/%d" % rest, s.fq, s.filter)
    assert want[0][0] == len(s.quals) and want[0][2] == G.FILL
    for at in s.seams:
        assert seam_is(s.fq, at, s.style), (at, s.style)
        dense_around(s, want, at)
        if s.style == "straddle":
            (line,) = [q for o, q in s.quals if o < at < o + len(q)]
            assert kept_once(want, line)
    for t in range(s.tiles - 10, s.tiles):                  # the last tiles of the file
        assert s.fq.count(b"\n", t * G.TILE, (t + 1) * G.TILE) >= 4, t
    assert want[2][-1] == s.quals[-1][1]
    assert max(len(q) for q in want[2]) < G.FILL


def test_f4_the_line_pass_seam_behind_a_carry(driver, tmp_path):  # noqa: F811
    s = G.f4()
    assert s.chunk < len(s.fq) <= 2 * s.chunk and len(s.fq) < 40 << 20
    assert s.tiles[0] > G.WAVE_CAP and s.tiles[1] > G.WAVE_CAP
    # the first window ends inside the carried line; the second window's buffer begins with it, off the tiles' edges
    (line,) = [q for o, q in s.quals if o < s.chunk < o + len(q)]
    (at,) = [o for o, q in s.quals if q is line]
    assert s.chunk - at == s.carry and s.carry % G.TILE and len(line) % 2 == 1
    assert (G.carry_room() - s.carry) % G.TILE != 0
    # tile WAVE_CAP of the second window in the file: its tiles begin at buffer offset (kCarryRoom - carry) rounded down
    tile0 = (G.carry_room() - s.carry) // G.TILE * G.TILE
    assert s.seams[1] == s.chunk + (tile0 + G.WAVE_CAP * G.TILE - G.carry_room())
    want = G.stdio(driver, tmp_path, "f4", s.fq, s.filter)
    assert want[0][0] == len(s.quals) and kept_once(want, line)
    for at in s.seams:
        assert seam_is(s.fq, at, "straddle")
        dense_around(s, want, at)


def test_b1_chain_records_past_the_pool_pass(driver, tmp_path):  # noqa: F811
    s = G.b1()
    recs = s.recs
    assert len(recs) == G.WAVE_CAP + 700 and len(s.stream) < 3_500_000
    assert {len(r["qual"]) for r in recs} == set(range(20, 101)) and len({len(r["name"]) for r in recs}) >= 10
    for side in (recs[:s.seam], recs[s.seam:]):
        assert {r["flag"] for r in side} == set(G.B1_FLAGS)
    bare = [r for r in recs if r["qual"][:1] == b"\xff"]
    assert len(bare) > 1000 and all(r["flag"] & 0x900 for r in bare)
    at, starts = 0, set()                                   # where the qualities begin in the window's buffer, whose first byte is the first record's
    for r in recs:
        n = len(r["seq"])
        starts.add((at + 36 + len(r["name"]) + 1 + 4 * len(r["cigar"]) + (n + 1) // 2) % 16)
        at += len(G.B.record_bytes(r))
    assert starts == set(range(16))
    want = G.stdio(driver, tmp_path, "b1", s.fq, s.filter)
    assert want[0][0] == sum(1 for r in recs if not r["flag"] & 0x900) < len(recs) - 5000
    for i, flag in ((s.seam - 2, 0), (s.seam - 1, 0x10), (s.seam, 0), (s.seam + 1, 0x10)):
        assert recs[i]["flag"] == flag and kept_once(want, G.fastq_line(recs[i])), i
        assert recs[i]["qual"] != recs[i]["qual"][::-1]
    assert all(set(r["qual"]) <= set(G.BEHIND) | {255} for r in recs[s.seam - 4:])
    assert not any(set(r["qual"]) <= set(G.BEHIND) for r in recs[:s.seam - 4])
    kept = set(want[2])
    assert sum(G.fastq_line(r) in kept for r in recs[s.seam:] if not r["flag"] & 0x900 and r["qual"][0] != 255) > 200


def test_i1_members_past_the_workgroups():
    s = G.i1()
    cap = G.MEMBER_CAP
    assert s.members == len(s.cdata) == cap + 700 and s.members < 2 * cap
    assert members(s.z) == s.texts and b"".join(s.texts) == s.want          # zlib's inflate, the CRC and ISIZE of every member
    # one piece: a piece ends at the default size of compressed or of inflated bytes, whichever comes first
    assert max(sum(len(c) for c in s.cdata), len(s.want)) < G.default_piece_bytes()
    kinds = [G.block_kind(c) for c in s.cdata]
    assert all(kinds[m] == G.kind_of(m) for m in range(s.members) if m not in (cap - 1, cap))
    assert s.texts[cap - 1] == s.texts[cap] == b"" and {len(t) for t in s.texts} >= set(range(1, 120))
    assert all(kinds[w] != kinds[w + cap] for w in range(700)), "a workgroup decodes the same kind twice"
    pairs = {(G.KINDS[kinds[w]], G.KINDS[kinds[w + cap]]) for w in range(700)}
    assert pairs == {(a, b) for a in G.KINDS for b in G.KINDS if a != b}
    for m in G.DEEP_AT:                                      # a fixed code behind a literal code of all fifteen lengths
        assert m < 700 and G.KINDS[kinds[m]] == "dynamic" and G.KINDS[kinds[m + cap]] == "fixed"
        assert set(G.literal_lengths(s.cdata[m])) >= set(range(1, 16))


@pytest.mark.parametrize("damage", sorted(G.DAMAGE))
def test_i2_one_damaged_member_on_the_second_trip(damage):
    s = G.i1()
    z, m, reason = G.i2(damage)
    assert m >= G.MEMBER_CAP and len(z) <= len(s.z) and z[:s.offsets[m]] == s.z[:s.offsets[m]]
    rest = len(z) - (len(s.z) - s.offsets[m + 1])
    assert z[rest:] == s.z[s.offsets[m + 1]:]
    bad = z[s.offsets[m]:rest]
    d = zlib.decompressobj(31)
    if damage == "crc":
        with pytest.raises(zlib.error, match=reason):
            d.decompress(bad)
    else:                                                   # (zlib runs into the trailer, or out of bytes)
        try:
            d.decompress(bad)
            whole = d.eof
        except zlib.error:
            whole = False
        assert not whole
