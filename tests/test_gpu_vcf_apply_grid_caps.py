"""`--apply-vcf` past the caps of its grids, after tests/test_gpu_mutate_grid_caps.py.  The line table's passes stride over the tiles of
bytes, the parse, the walk and the marks over the lines, the reach, the cluster and the text's passes over the tiles of lines, the
base passes over the tiles of positions, all with capped grids, and the one workgroup that scans the tiles' largest values takes
kThreads * kScanPerLane tiles per trip.  Every other test of the stage is small enough for one trip through each loop; the case here
is built from the caps, read from the source, so that each loop takes a second trip, and is held to the same model byte for byte.

One record carries an snv on every second position, written last line first, so that the sorted place of a line is half its
position and the seams of the lines' passes and of the positions' passes fall on the same lines.  Where the seams are, the snvs give
way to what can go wrong there: a chain of six overlapping spans whose walk crosses the seam of the per-line passes (and whose third
span lies over the seam of the base passes; the snv behind the last span, which lost, still belongs to the cluster), a deletion that
covers the seam of the positions' scan, and an insertion with a long X just behind the chain, in the base passes' second trip."""
import functools

import pytest

import harness
import pbsim3_amd as P
from test_gpu_bam_grid_caps import constant
from test_gpu_vcf_apply import check, flip, verdicts

pytestmark = pytest.mark.gpu

THREADS, TILE = constant("bam_pileup_walk.h", "kThreads"), constant("bam_pileup.h", "kPileTile")
TEXT_TILE, LINE_TILE = constant("vcf_apply.h", "kApTile"), constant("vcf_apply.h", "kApLineTile")
TILE_BLOCKS, LANE_BLOCKS, LINE_BLOCKS, BASE_BLOCKS = (constant("vcf_apply.hip", name) for name in ("kTileBlocksMax", "kLaneBlocksMax", "kLineBlocksMax",
                                                                                                 "kBaseBlocksMax"))
SCAN_PER_LANE = constant("vcf_apply.hip", "kScanPerLane")
LANE_SEAM = LANE_BLOCKS * THREADS                   # the first line of the second trip of a per-line pass
BASE_SEAM = BASE_BLOCKS * TILE                      # the first buffer index of the second trip of a base pass
SCAN_SEAM = THREADS * SCAN_PER_LANE * TILE          # the first position whose tile the scan takes in its second trip
N = LANE_SEAM + 700                                 # the snvs' places
MAX_LINES = 400_000


def test_the_caps_are_where_the_case_expects_them():
    assert TILE == LINE_TILE == THREADS and LINE_BLOCKS * LINE_TILE == LANE_SEAM == THREADS * SCAN_PER_LANE * LINE_TILE, \
        "the passes over the lines have different seams: the chain lies over one of them only"
    assert BASE_SEAM == 2 * LANE_SEAM, "the chain would not lie over the seam of the base passes"
    assert SCAN_SEAM + 100 < BASE_SEAM - 100 and N < MAX_LINES, "the case would have %d lines" % N


@functools.lru_cache(maxsize=None)
def case():
    seq = harness.synth_bases(2 * N + 64, 91).tobytes()
    row = lambda p, d, x: b"big\t%d\t.\t%s\t%s\n" % (p + 1, seq[p:p + d], x)
    snv = lambda p: row(p, 1, flip(chr(seq[p])).encode())
    span = lambda p: row(p, 3, (flip(chr(seq[p])) + flip(chr(seq[p + 2]))).encode())
    chain = range(LANE_SEAM - 3, LANE_SEAM + 3)                                    # places; their spans [2k, 2k + 3) overlap one the next
    gap = range(SCAN_SEAM // 2 - 3, SCAN_SEAM // 2 + 4)
    lines = []
    for k in range(N):
        if k in chain:
            lines.append(span(2 * k))
        elif k == gap[0]:
            lines.append(row(2 * k - 1, 12, seq[2 * k - 1:2 * k]))                 # the deletion [2k, 2k + 11) over the scan's seam
        elif k not in gap:
            lines.append(snv(2 * k))
    lines.append(row(BASE_SEAM + 6, 1, seq[BASE_SEAM + 6:BASE_SEAM + 7] + b"ACGGT" * 200))      # an insertion behind the chain
    lines.reverse()
    tail = harness.synth_bases(300, 92).tobytes()
    lines += [b"tail\t%d\t.\t%s\t%s\n" % (p + 1, tail[p:p + 1], flip(chr(tail[p])).encode()) for p in (0, 7, 299)]
    genome = [("big", seq), ("tail", tail)]
    text = b"#CHROM\tPOS\tID\tREF\tALT\n" + b"".join(lines)
    return genome, text


def test_a_file_and_a_genome_past_every_cap():
    genome, text = case()
    n_lines = text.count(b"\n") - 1
    assert n_lines > max(LANE_SEAM, LINE_BLOCKS * LINE_TILE, THREADS * SCAN_PER_LANE * LINE_TILE) + LINE_TILE
    assert len(text) > (TILE_BLOCKS + 8) * TEXT_TILE and len(genome[0][1]) > max(BASE_SEAM, SCAN_SEAM) + 2 * TILE
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as ctx:
        r = check(ctx, text, genome, modes=(0,))
    assert r.lines == n_lines and r.overlap == 3 and r.applied == n_lines - 3 and r.longest_cluster == 7 and r.types == [n_lines - 8, 1, 1, 3]
    by_start = {row["s"]: row for row in r.rows if row["r"] == 0}
    assert [by_start[2 * k]["cls"] for k in range(LANE_SEAM - 3, LANE_SEAM + 3)] == ["applied", "overlap"] * 3
    assert by_start[BASE_SEAM + 7]["cls"] == "applied" and len(by_start[BASE_SEAM + 7]["x"]) == 1000 and by_start[SCAN_SEAM - 6]["d"] == 11
    assert r.origins[0][SCAN_SEAM - 7:SCAN_SEAM - 4].tolist() == [SCAN_SEAM - 7, SCAN_SEAM + 5, SCAN_SEAM + 6]
    assert verdicts(r)[-3:] == ["applied"] * 3 and r.per_record[1] == (300, 300, 3)
