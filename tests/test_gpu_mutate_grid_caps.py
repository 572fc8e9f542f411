"""`--mutate-genome` past the caps of its grids, after tests/test_gpu_bam_grid_caps.py.  The event, base and line passes stride over
the tiles with capped grids, and the one workgroup that scans the tiles' largest ends takes kThreads * kScanPerLane tiles per trip.
Every other test of the stage is small enough for one trip through each loop; the genome here is built from the caps, read from the
source, so that each loop takes a second trip, and is held to the same model byte for byte.

The genome is N nearly everywhere, so that the model's events stay few at rates high enough to put them where they are wanted: A C
G T stands on the first two tiles, around the scan's seam, around the tile passes' seam (the first position of their second trip)
and in a second record behind it.  The seed is looked for with the model: one layout has a merged pair of deletion runs over the
tile passes' seam and a run over the scan's, the other an insertion on the first trip's last position and an snv on the second
trip's first.

Each layout goes once through the command line with PBSIM_TRACE, and the stage's own summary line has to say that it passed the
caps: a changed cap that leaves the genome in one trip fails here, and one that makes it huge fails the size limit below."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import harness
import mutate_model as G
import pbsim3_amd as P
from test_call_model import lines_of
from test_gpu_bam_grid_caps import constant
from test_gpu_mutate import check

pytestmark = pytest.mark.gpu

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")
THREADS, TILE = constant("bam_pileup_walk.h", "kThreads"), constant("bam_pileup.h", "kPileTile")
EVENT_BLOCKS, BASE_BLOCKS, LINE_BLOCKS = (constant("genome_mutate.hip", name) for name in ("kEventBlocksMax", "kBaseBlocksMax", "kLineBlocksMax"))
SCAN_PER_LANE = constant("genome_mutate.hip", "kScanPerLane")
SEAM = EVENT_BLOCKS * TILE                          # the first buffer index of the second trip of a tile pass
SCAN_SEAM = THREADS * SCAN_PER_LANE * TILE          # the first position whose tile the scan takes in its second trip
MAX_POSITIONS = 2_000_000
RATES = dict(snv_ppm=250000, ins_ppm=200000, del_ppm=250000, ext_ppm=600000, max_indel=9)
LAYOUTS = ["merged run", "ins and snv"]


def test_the_caps_are_where_the_genome_expects_them():
    assert TILE == THREADS and EVENT_BLOCKS == BASE_BLOCKS == LINE_BLOCKS, "the tile passes have different caps: the genome has its seam behind one of them only"
    assert 2 * TILE < SCAN_SEAM - 300 and SCAN_SEAM + 300 < SEAM - 300, "the windows of A C G T would overlap"
    assert SEAM + 4 * TILE < MAX_POSITIONS, "the genome would have %d positions" % SEAM


def big_record():
    """N, and A C G T on the first two tiles and 300 positions to either side of both seams (437 behind the tile passes')"""
    n = SEAM + 437
    seq = np.full(n, ord("N"), dtype=np.uint8)
    bases = harness.synth_bases(n, 31)
    for lo, hi in ((0, 2 * TILE), (SCAN_SEAM - 300, SCAN_SEAM + 300), (SEAM - 300, n)):
        seq[lo:hi] = bases[lo:hi]
    return seq


@functools.lru_cache(maxsize=None)
def seam_genome(layout):
    """(genome, seed): the first record begins at buffer index 0, so its positions are buffer indices"""
    seq = big_record()
    for seed in range(1, 2000):
        _, kind, _, _, deleted, _ = G.sites(seq, 0, dict(G.DEFAULTS, seed=seed, **RATES))
        if layout == "merged run":
            merged = [p for p in range(SEAM - 3, SEAM + 2) if kind[p] == G.DEL and deleted[p]]
            if deleted[SEAM - 1] and deleted[SEAM] and merged and deleted[SCAN_SEAM - 1] and deleted[SCAN_SEAM]:
                break
        elif kind[SEAM - 1] == G.INS and not deleted[SEAM - 1] and kind[SEAM] == G.SNV and not deleted[SEAM]:
            break
    else:
        raise AssertionError("no seed below 2000 gives the layout %r" % layout)
    text = seq.tobytes()
    lines = b"\n".join(text[k:k + 100000] for k in range(0, len(text), 100000)) + b"\n"
    return [("big", lines), ("tail", harness.synth_bases(700, 32).tobytes() + b"\n")], seed


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_genome_past_every_cap(layout):
    genome, seed = seam_genome(layout)
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as ctx:
        r = check(ctx, genome, seed=seed, **RATES)
    starts = {int(line.split(b"\t")[1]) - 1: line for line in lines_of(r.vcf) if line.startswith(b"big\t")}
    if layout == "merged run":                      # one line whose REF reaches over the seam, and one over the scan's
        for seam in (SEAM, SCAN_SEAM):
            assert any(p < seam - 1 and p + len(line.split(b"\t")[3]) > seam + 1 for p, line in starts.items()), seam
        assert r.merged > 20
    else:
        assert starts[SEAM - 1].endswith(b"TYPE=ins") and starts[SEAM].endswith(b"TYPE=snv")
        assert {SEAM - 1, -SEAM, SEAM} <= set(r.origins[0].tolist())
    assert r.per_record[0][0] == SEAM + 437 and r.per_record[1][2] > 100 and min(r.types) > 100


@pytest.mark.parametrize("layout", LAYOUTS)
def test_cli_says_that_the_genome_passes_the_caps(tmp_path, layout):
    """a condition, not a measurement: the summary line that the stage prints with PBSIM_TRACE counts more tiles than the tile
    passes have workgroups and than the scan takes in one trip; the same run's report and outputs are the model's"""
    genome, seed = seam_genome(layout)
    want = G.mutate(genome, seed=seed, **RATES)
    (tmp_path / "genome.fa").write_bytes(b"".join(b">" + n.encode() + b"\n" + lines for n, lines in genome))
    cmd = [CLI, "--mutate-genome", "genome.fa", "--mutate-out", "out.fa", "--mutate-vcf", "out.vcf", "--mutate-seed", str(seed)]
    cmd += [x for name, v in RATES.items() for x in ("--mutate-" + name.replace("_", "-"), str(v))]
    r = subprocess.run(cmd, capture_output=True, cwd=str(tmp_path), timeout=300, env=dict(os.environ, PBSIM_TRACE="1"))
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == want.report and (tmp_path / "out.fa").read_bytes() == want.fasta and (tmp_path / "out.vcf").read_bytes() == want.vcf
    said = re.search(rb"\[pbsim mutate\] .* total: (\d+) genome records, (\d+) positions in (\d+) tiles, (\d+) bases out, (\d+) variants", r.stderr)
    assert said, r.stderr[-4000:]
    records, positions, tiles, bases_out, variants = (int(v) for v in said.groups())
    print("%s: %d positions in %d tiles, %d variants" % (layout, positions, tiles, variants))
    assert (records, positions, bases_out, variants) == (2, want.bases_in, want.bases_out, want.variants)
    assert tiles > max(EVENT_BLOCKS, BASE_BLOCKS, LINE_BLOCKS) and tiles > THREADS * SCAN_PER_LANE
