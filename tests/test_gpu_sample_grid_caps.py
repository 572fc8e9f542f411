"""The sample profile builders (sample_profile.hip, sample_bam.hip) and the scan (kernels.hip) past the caps of their grids.  The
waves of k_sp_count, k_sp_lines, k_sp_pool and k_sb_pool stride over the tiles or records of a window when there are more than
kSpBlocksMax workgroups of four waves can take, and k_scan_single, one workgroup, strides over the tile sums of a scan.  Every other
test of the builders fills a window with a few MB and a few hundred records, one trip through each loop; the inputs here
(grid_caps_inputs.py) are built from the caps, read from the sources, so that each loop takes a second trip in ONE window, and are
held to the contract of test_gpu_sample_profile.py and test_gpu_sample_bam.py: the eight integers, the four doubles by their bits
and every kept string in order, against the stdio parse (for a BAM, of bam_writer.to_fastq's text).

  kernel          case  what differs across the seam of its two trips
  k_sp_pool       F1    record 16 384 of 17 084: another palette from record cap - 4 on, lines of 20 .. 100 characters at every
                        start & 15 and len % 8, records cap - 1 and cap both kept; off[r] of the second trip comes from the scan
  k_scan_single   F2    element 524 288 of 527 288 (tile sum 256): sixty kept records in front of the seam, so that s_base is not 0
                        when the second trip begins, kept records at the last index of the first trip and the first of the second
                        and forty behind.  THIS IS THE SCAN'S TEST FOR ALL ITS CALLERS (some forty call sites in every stage
                        share launch_exclusive_scan_i64, and none of their tests scans more than one trip's elements).
  k_sp_lines      F3    tile 16 384 (file offset 16 MiB) of 65 548 and more: dense records of every line phase on the eight tiles
                        either side, of another palette behind it; over the seam a quality line, a header line, or a record's
                        fourth line feed as the tile's first byte: tile_base[t] and the record grid by a tile that is not the wave's
  k_sp_count      F3    tile 65 536 (file offset 64 MiB; the default window ends there, a set chunk goes on): the same around it
                        and to the end of the file, whose tiles mod kCountUnroll are 0, 1 and 3 (the guard of the unrolled tail)
  k_sp_lines      F4    tile 16 384 of the second of two windows, which begins with 33 333 carried bytes of a kept line of odd
                        length: b0 is off the tiles' edges and the tiles are shifted against the file
  k_sb_pool       B1    chain record 16 384 of 17 084 (skipped records count: the seam is an index into the chain), a kept
                        forward and a kept reverse record on each side, another palette from record cap - 4 on

Nothing here was tried against planted faults: a skipped trip leaves offsets unwritten, and the pass behind it would address memory
through them.  A wrong stride or base in any of these loops leaves bytes of the pool unwritten or written twice, or a record's
start or end with the first trip's; the palettes, the kept records on both sides and the lengths make such bytes differ from the
stdio parse's.

Each case fixes the window so that the whole input is one (F4: two), and the trace line that the builder prints per window has to
say so: a changed cap or window rule fails here, and does not quietly leave an input in one trip.

Measured on an MI355X, the inputs built and parsed in the same test: F1 0.5 s, B1 0.3 s, F2 0.08 s, each case of F3 0.06 s (64 MiB
up the link and through four kernels), F4 0.05 s; the slowest case of test_gpu_bam_grid_caps.py takes 1.1 s there."""
import re

import pytest

import grid_caps_inputs as G
import test_gpu_sample_bam as SB
import test_gpu_sample_profile as SP
from test_gpu_sample_profile import driver, same  # noqa: F401  (driver: the fixture that compiles the stdio driver)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def contexts():
    """the contexts that SP.gpu and SB.gpu opened for this module's filters"""
    yield
    for module in (SP, SB):
        for ctx in module._CONTEXTS.values():
            ctx.close()
        module._CONTEXTS.clear()


def windows(capfd, monkeypatch, run):
    """run()'s result, and (bytes, records, carry) of every window as the builder's trace states them"""
    monkeypatch.setenv("PBSIM_TRACE", "1")
    capfd.readouterr()
    got = run()
    err = capfd.readouterr().err
    monkeypatch.delenv("PBSIM_TRACE")
    said = re.findall(r"\[pbsim sample profile\] (?:BAM )?window (\d+): (\d+) bytes, (?:\d+ candidates, )?(\d+) records, \d+ pool bytes, carry (\d+)", err)
    assert said and [int(x[0]) for x in said] == list(range(len(said))), err[-2000:]
    return got, [tuple(int(v) for v in x[1:]) for x in said]


def kept_once(want, line):
    return want[2].count(line) == 1


def test_the_windows_begin_on_a_tile():
    assert G.carry_room() % G.TILE == 0, "tile t of a first window would not begin at file offset t * kSpTile"


def test_f1_records_past_the_pool_pass(driver, tmp_path, capfd, monkeypatch):  # noqa: F811
    s = G.f1()
    want = G.stdio(driver, tmp_path, "f1", s.fq, s.filter)
    assert want[0][0] > G.WAVE_CAP and kept_once(want, s.quals[s.seam - 1][1]) and kept_once(want, s.quals[s.seam][1])
    got, said = windows(capfd, monkeypatch, lambda: SP.gpu(s.fq, s.filter, len(s.fq)))
    print("f1:", said)
    assert said == [(len(s.fq), len(s.quals), 0)] and said[0][1] > G.WAVE_CAP
    same(got, want, "f1")
    same(SP.gpu(s.fq, s.filter, len(s.fq), "device"), want, "f1 from the device")


def test_f2_records_past_one_trip_of_the_scan(driver, tmp_path, capfd, monkeypatch):  # noqa: F811
    """the scan's test for all its callers: launch_exclusive_scan_i64 over more than kScanBlock * kScanTile elements, here the
    padded lengths of a window's records, with kept records in front of the seam of k_scan_single's two trips, on it and behind"""
    s = G.f2()
    want = G.stdio(driver, tmp_path, "f2", s.fq, s.filter)
    assert want[0][0] > G.SCAN_CAP and want[2] == [s.kept[k] for k in sorted(s.kept)] and {s.seam - 1, s.seam} <= set(s.kept)
    got, said = windows(capfd, monkeypatch, lambda: SP.gpu(s.fq, s.filter, len(s.fq)))
    print("f2:", said)
    assert said == [(len(s.fq), s.records, 0)] and said[0][1] > G.SCAN_CAP
    same(got, want, "f2")
    same(SP.gpu(s.fq, s.filter, len(s.fq), "device"), want, "f2 from the device")


@pytest.mark.parametrize("rest", sorted(G.F3_STYLES))
def test_f3_tiles_past_the_line_pass_and_the_count(driver, tmp_path, capfd, monkeypatch, rest):  # noqa: F811
    s = G.f3(rest)
    want = G.stdio(driver, tmp_path, "f3/%d" % rest, s.fq, s.filter)
    chunk = len(s.fq) + (0, 1, 0, 4 << 20)[rest]            # the file and no more, or more than the file
    got, said = windows(capfd, monkeypatch, lambda: SP.gpu(s.fq, s.filter, chunk))
    print("f3, %d:" % rest, said, G.tiles_of(said[0][0]), "tiles")
    assert said == [(len(s.fq), len(s.quals), 0)]
    assert G.tiles_of(said[0][0]) > G.COUNT_CAP > G.WAVE_CAP and G.tiles_of(said[0][0]) % G.UNROLL == rest
    same(got, want, ("f3", rest))


def test_f4_the_line_pass_seam_behind_a_carry(driver, tmp_path, capfd, monkeypatch):  # noqa: F811
    s = G.f4()
    want = G.stdio(driver, tmp_path, "f4", s.fq, s.filter)
    got, said = windows(capfd, monkeypatch, lambda: SP.gpu(s.fq, s.filter, s.chunk))
    print("f4:", said)
    assert len(said) == 2 and said[0][0] == s.chunk and said[0][2] == s.carry and said[1][0] == s.carry + len(s.fq) - s.chunk
    assert said[0][1] + said[1][1] == len(s.quals) and said[1][2] == 0
    shift = (G.carry_room() - s.carry) % G.TILE             # the second window's first byte in its first tile
    assert shift != 0
    assert [G.tiles_of(said[0][0]), G.tiles_of(shift + said[1][0])] == s.tiles and min(s.tiles) > G.WAVE_CAP
    same(got, want, "f4")


def test_b1_chain_records_past_the_pool_pass(driver, tmp_path, capfd, monkeypatch):  # noqa: F811
    s = G.b1()
    want = G.stdio(driver, tmp_path, "b1", s.fq, s.filter)
    for i, flag in ((s.seam - 2, 0), (s.seam - 1, 0x10), (s.seam, 0), (s.seam + 1, 0x10)):
        assert s.recs[i]["flag"] == flag and kept_once(want, G.fastq_line(s.recs[i])), i
    got, said = windows(capfd, monkeypatch, lambda: SB.gpu(s.stream, s.filter, len(s.stream)))
    print("b1:", said)
    assert said == [(len(s.stream) - len(G.B.header(G.B1_REFS)), len(s.recs), 0)] and said[0][1] > G.WAVE_CAP
    same(got, want, "b1")
    same(SB.gpu(s.stream, s.filter, len(s.stream), "device"), want, "b1 from the device")
