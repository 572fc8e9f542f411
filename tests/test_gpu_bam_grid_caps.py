"""`--errors-bam`, `--pileup-bam`, `--consensus-bam` and `--call-bam` past the caps of their grids.  The kernels whose workgroups are
capped stride over their work: the column passes over the segments, the site, base and line passes over the tiles, the log passes
over the log's entries.  Every other test of these stages is small enough for one trip through each loop; the inputs here are built
from the caps, read from the sources, so that each loop takes a second trip, and are held to the same models byte for byte:

  A  a genome of more than kSiteBlocksMax = kBaseBlocksMax = kLineBlocksMax tiles, with what the passes carry across a tile's edge
     (deletion runs, an ins_site, a sub_site, a leading run, a wholly deleted record) at the seam between the first trip's last tile
     and the second trip's first, and noise on the first two tiles of either trip;
  B  one file of more than kSegBlocksMax * kWaves segments, one record's three segments on both sides of the seam (of the other
     tests only test_gpu_bam_errors' text of 15 000 lines takes a column pass, k_err_columns, into a second trip);
  C  one file of more than kLogBlocksMax * kThreads log entries.

Tried once: counters reset on every trip in k_pile_sites, k_cons_bases and k_call_lines and a wrong stride in k_cons_log and
k_err_columns, of which the four stages' own tests noticed only the last; then k_pile_columns' unanchored cell zeroed on every trip.
The tests here failed for each of the six.

Each input goes once through the command line with PBSIM_TRACE, and the stage's own summary line has to say that it passed its cap: a
changed cap that leaves an input in one trip fails here, and one that makes an input huge fails the size limits below.

Not reached: column_blocks' `least` branch (more than 2^21 segments), the record-strided log-size kernel (more than
kLogSizeBlocksMax * kThreads = 262 144 records: a BAM of 262 444 minimal records has 15.6 MB, twice MAX_STREAM below, and
consensus_model.consensus took 42 s on it), a 32-bit cell's wrap, and a text of more than the default piece of 8 MiB."""
import functools
import os
import random
import re
import subprocess

import pytest

import bam_writer as B
import call_model as V
import consensus_model as K
import errors_model as E
import harness
import pbsim3_amd as P
import pileup_model as M
import test_gpu_bam_call as TV
import test_gpu_bam_consensus as TK
import test_gpu_bam_errors as TE
import test_gpu_bam_pileup as TM
from test_call_model import lines_of
from test_gpu_bam_call import other, places, say
from test_gpu_bam_errors import SEG_COLS, aligned, fasta_lines, planted

pytestmark = pytest.mark.gpu

CSRC = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")


def constant(source, name):
    """`constexpr int name = <number>` or `= kThreads / <number>` as `source` says it"""
    with open(os.path.join(CSRC, source)) as f:
        text = f.read()
    found = re.findall(r"constexpr int %s = (?:(\d+)|kThreads / (\d+));" % name, text)
    assert len(found) == 1, "%s: %d definitions of %s" % (source, len(found), name)
    return int(found[0][0]) if found[0][0] else constant(source, "kThreads") // int(found[0][1])


THREADS, WAVES = constant("bam_pileup_walk.h", "kThreads"), constant("bam_pileup_walk.h", "kWaves")
SEG_BLOCKS = constant("bam_errors.hip", "kSegBlocksMax")
SITE_BLOCKS, LOG_BLOCKS = constant("bam_pileup.hip", "kSiteBlocksMax"), constant("bam_consensus.hip", "kLogBlocksMax")
BASE_BLOCKS, LINE_BLOCKS = constant("bam_consensus.hip", "kBaseBlocksMax"), constant("bam_call.hip", "kLineBlocksMax")
TILE = constant("bam_pileup.h", "kPileTile")
SEG_CAP = SEG_BLOCKS * WAVES            # the segments of one trip of a column pass
LOG_CAP = LOG_BLOCKS * THREADS          # the entries of one trip of a log pass
SEAM = SITE_BLOCKS * TILE               # the first buffer index of the second trip of a tile pass
MAX_POSITIONS, MAX_STREAM = 2_000_000, 8_000_000


def test_the_caps_are_where_the_inputs_expect_them():
    """one seam for the three tile passes and one for the two column passes; an input of a size that a test can afford"""
    assert (constant("bam_errors.hip", "kThreads"), constant("bam_errors.hip", "kWaves")) == (THREADS, WAVES) and TILE == THREADS
    assert constant("bam_pileup_walk.h", "kSegBlocksMax") == SEG_BLOCKS, "the two column passes have different caps: input B fits one of them only"
    assert SITE_BLOCKS == BASE_BLOCKS == LINE_BLOCKS, "the tile passes have different caps: input A has its seam behind one of them only"
    assert SEAM + 4 * TILE < MAX_POSITIONS, "input A would have %d positions" % SEAM
    assert SEG_CAP * 120 < MAX_STREAM and LOG_CAP * 2 < MAX_STREAM, "inputs B and C would have %d and %d bytes" % (SEG_CAP * 120, LOG_CAP * 2)


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


_WANT = {}


def model(stage, name, kw=()):
    """the model's result for an input, worked out once"""
    key = (stage, name, kw)
    if key not in _WANT:
        streams, genome = INPUTS[name]()[:2]
        run = {"errors": E.errors, "pileup": functools.partial(M.pileup, fmt="sites"), "consensus": K.consensus, "call": V.call}[stage]
        _WANT[key] = run(streams, genome, **dict(kw))
    return _WANT[key]


def through(ctx, stage, name, streams=None, **kw):
    """input `name` through the product, every output against the model; with `streams` the same records in other files, which
    have to give the result of the input's own"""
    key = tuple(sorted(kw.items()))
    own, genome = INPUTS[name]()[:2]
    if stage == "errors" and streams is None:               # (this check works the model out itself)
        got = TE.check(ctx, own, genome, **kw)
        assert got == _WANT.setdefault((stage, name, key), got)
        return got
    want = model(stage, name, key)
    if stage == "errors":                                   # (a line per record in the files' order: the same lines in another order)
        got = ctx.bam_errors([B.contain(s) for s in streams], genome, text=True, **kw)
        TE.compare(got, want)
        assert sorted(got[2].split(b"\n")) == sorted(want.text.split(b"\n"))
    elif stage == "pileup":
        TM.check(ctx, streams or own, genome, fmts=("sites",), wants={"sites": want}, **kw)
    else:
        (TK if stage == "consensus" else TV).check(ctx, streams or own, genome, want=want, **kw)
    return want


# ---------------------------------------------------------------- A: a genome past the tile passes' cap
# where the seam falls: on a record's first position; in the padding behind a record; inside a record, once with a deletion run
# over it and once with an ins_site in front of it and a sub_site behind (a position is either deleted or substituted)
LAYOUTS = ["first", "padding", "middle_run", "middle_ins_sub"]
AGREE = 4                                                   # reads that say a planted feature


@functools.lru_cache(maxsize=None)
def seam_input(layout):
    """(streams, genome, lengths by name, the VCF lines' beginnings and types that have to be there): `big` reaches the seam, `tail`
    lies behind it and `gone`, wholly deleted, behind that; sparse clean reads over `big`, noisy ones on the first two tiles of
    either trip"""
    k = LAYOUTS.index(layout)
    rng = random.Random(2048 + k)
    # (a record's bases are rounded up to 64 in the buffers, and 64 lie behind them)
    lens = [[("big", SEAM - 88), ("tail", 700), ("gone", 100)],                 # big fills [0, SEAM) with its padding: tail begins at SEAM
            [("big", SEAM), ("tail", 700), ("gone", 100)],                      # big's last base is the first trip's last position
            [("front", 300), ("big", SEAM + 437), ("tail", 700), ("gone", 100)]][min(k, 2)]
    seq = {n: planted(rng, l + 10, longest=4)[:l] for n, l in lens}
    names = [n for n, _ in lens]
    ids = {n: i for i, n in enumerate(names)}
    at = dict(zip(names, places([l for _, l in lens])))
    seqs = {ids[n]: seq[n] for n in names}
    big, tail, L = seq["big"], seq["tail"], len(seq["big"])
    assert sum(l for _, l in lens) < MAX_POSITIONS and (at["gone"] + 100 + TILE - 1) // TILE > SITE_BLOCKS
    assert at["tail"] >= SEAM and at["gone"] // TILE > SITE_BLOCKS      # tail and gone lie wholly in the second trip
    recs, lines = [], []

    def clean(name, n_reads, length):
        for j in range(n_reads):
            pos = rng.randrange(len(seq[name]) - length)
            recs.append(aligned("c%s%d" % (name, j), [(length, "M")], pos=pos, ref=ids[name], rng=rng, seqs=seqs, keep=1.0, qual="none"))

    def noisy(name, lo, hi):
        """reads of 150 bases side by side, each one twice: what they say stands at depth 2"""
        for j, pos in enumerate(range(lo, hi - 150, 155)):
            ops = [(40 + j % 9, "M"), (1 + j % 2, "I"), (45, "M"), (1 + j % 3, "D"), (50, "M")]
            recs.extend([aligned("n%s%d" % (name, pos), ops, pos=pos, ref=ids[name], rng=rng, seqs=seqs, keep=0.9, mapq=rng.randrange(60))] * 2)

    clean("big", L // 3500, 300)                            # (about 150 reads where the caps are 2048 tiles)
    if k == 0:
        assert at["tail"] == SEAM
        recs += [say("lead", tail, 0, 30, dels=range(0, 5), ref_id=ids["tail"])] * AGREE     # the backward walk leaves the second trip
        lines.append((b"tail\t1\t.\t" + tail[:6] + b"\t" + tail[5:6] + b"\t", None))
        recs += [say("last", big, L - 100, L, inss={L - 1: "GA"})] * AGREE
        lines.append((b"big\t%d\t.\t" % L + big[L - 1:L] + b"\t" + big[L - 1:L] + b"GA\t", b"ins"))
        noisy("big", 20, 520), noisy("tail", 30, 560)
    elif k == 1:
        assert at["big"] + L == SEAM and at["tail"] == SEAM + 64
        # a run up to the base in front of big's last, and big's last an ins_site on the first trip's last position
        recs += [say("end", big, L - 120, L, dels=range(L - 6, L - 1), inss={L - 1: "TT"})] * AGREE
        lines.append((b"big\t%d\t.\t" % (L - 6) + big[L - 7:L - 1] + b"\t" + big[L - 7:L - 6] + b"\t", b"del"))
        lines.append((b"big\t%d\t.\t" % L + big[L - 1:L] + b"\t" + big[L - 1:L] + b"TT\t", b"ins"))
        recs += [say("sub", tail, 0, 10, subs={0: other(tail, 0)}, ref_id=ids["tail"])] * AGREE
        lines.append((b"tail\t1\t.\t" + tail[:1] + b"\t" + bytes([other(tail, 0)]) + b"\t", b"snv"))
        noisy("big", 20, 520), noisy("tail", 10, 500)
    else:
        a = SEAM - at["big"]                                # big[a] is the second trip's first position
        assert at["big"] == 384 and 340 < a < L - 600
        if k == 2:      # the anchor on the first trip, its run over the seam, an insertion behind the first trip's last (deleted) position
            recs += [say("run", big, a - 150, a + 30, dels=range(a - 3, a + 2), inss={a - 1: "GT"}, ref_id=ids["big"])] * AGREE
            lines.append((b"big\t%d\t.\t" % (a - 3) + big[a - 4:a + 2] + b"\t" + big[a - 4:a - 3] + b"GT\t", b"complex"))
        else:
            recs += [say("both", big, a - 150, a + 30, subs={a: other(big, a)}, inss={a - 1: "GT"}, ref_id=ids["big"])] * AGREE
            lines.append((b"big\t%d\t.\t" % a + big[a - 1:a] + b"\t" + big[a - 1:a] + b"GT\t", b"ins"))
            lines.append((b"big\t%d\t.\t" % (a + 1) + big[a:a + 1] + b"\t" + bytes([other(big, a)]) + b"\t", b"snv"))
        recs += [say("sub", tail, 0, 10, subs={0: other(tail, 0)}, ref_id=ids["tail"])] * AGREE
        noisy("front", 5, 300), noisy("big", 0, 330), noisy("big", a + 30, a + 600)
    recs += [say("g", seq["gone"], 0, 100, dels=range(100), ref_id=ids["gone"], clip=1)] * AGREE
    rng.shuffle(recs)
    stream = B.stream(recs, lens)
    assert len(stream) < MAX_STREAM
    return [stream], [(n, fasta_lines(seq[n])) for n in names], dict(lens), lines


A_RUNS = [("pileup", dict()), ("consensus", dict(fill="n", line_width=60)), ("consensus", dict(fill="ref", line_width=60)), ("call", dict()),
          ("call", dict(min_depth=2, min_baseq=20))]


@pytest.mark.parametrize("stage,kw", A_RUNS, ids=lambda x: (",".join("%s=%s" % i for i in x.items()) or "defaults") if isinstance(x, dict) else x)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_genome_of_more_tiles_than_workgroups(ctx, layout, stage, kw):
    """the seam of the two trips on a record's first position, in the padding and inside a record; what the loops carry over it is
    the model's: the sites, the hp arrays, the cell sums and max_depth (pileup), the bases and lengths (consensus), the variants, the
    types, the longest REF and ALT, the unplaced record and the per-record counts (call)"""
    streams, genome, lens, lines = seam_input(layout)
    assert (places(list(lens.values()) + [0])[-1] + TILE - 1) // TILE > max(SITE_BLOCKS, BASE_BLOCKS, LINE_BLOCKS)
    r = through(ctx, stage, layout, **kw)
    names = list(lens)
    if stage == "pileup":
        assert r.sites[0] == sum(lens.values()) and r.sites[6] >= 100 and r.sites[7] >= 1 and r.sites[5] > 20 and r.ins_unanchored == 0
    elif stage == "consensus":
        assert r.lengths[names.index("gone")] == (100, 0) and r.ins_sites >= 1 and r.bases[5] >= 100
    else:
        assert (r.unplaced_records, r.unplaced_sites) == (1, 100) and r.records[names.index("gone")] == (100, 0)
        if not kw:
            got = lines_of(r.text)
            for begin, kind in lines:
                assert any(line.startswith(begin) and b";MS=%d;" % AGREE in line and (kind is None or line.endswith(b"TYPE=" + kind)) for line in got), begin
            assert r.variants > 40 and all(n > 0 for _, n in r.records[:-1])


# ---------------------------------------------------------------- B: one file past the column passes' cap
def segments_of(ops):
    return -(-sum(n for n, op in ops if op in "MID=X") // SEG_COLS)


@functools.lru_cache(maxsize=None)
def segments_input():
    """(streams, genome, the records, the segments of each): SEG_CAP + 100 records of one segment and about 30 bases, every third
    without qualities, some with an insertion in front of their first base; behind SEG_CAP - 1 of them one of three segments"""
    rng = random.Random(SEG_CAP)
    ref = planted(rng, 20_010, longest=6)[:20_000]
    seqs = {0: ref}

    def short(k):
        ops = [(11 + k % 5, "M"), (1 + k % 2, "I"), (8, "M"), (1 + k % 3, "D"), (9, "M")]
        if k % 37 == 5:
            ops = [(k % 3, "S")] * (k % 3 > 0) + [(1 + k % 2, "I")] + ops
        mapq = 3 if k % 211 == 11 else rng.randrange(5, 60)                     # (a smallest mapping quality of 5 leaves the file above the cap)
        return ops, aligned("s%d" % k, ops, pos=rng.randrange(len(ref) - 60), rng=rng, seqs=seqs, mapq=mapq, flag=16 * (k % 2),
                            qual="none" if k % 3 == 0 else "random")
    both = [short(k) for k in range(SEG_CAP - 1)]
    long_ops = [(SEG_COLS + 900, "M"), (1, "I"), (SEG_COLS + 200, "M"), (2, "D"), (50, "M")]
    both.append((long_ops, aligned("long", long_ops, pos=1000, rng=rng, seqs=seqs)))
    both += [short(k) for k in range(SEG_CAP - 1, SEG_CAP + 100)]
    n_seg = [segments_of(ops) for ops, _ in both]
    # the long record's segments are SEG_CAP - 1 (the last wave's, on its first trip), SEG_CAP and SEG_CAP + 1 (the first two waves', on their second)
    assert n_seg[SEG_CAP - 1] == 3 and sum(n_seg[:SEG_CAP - 1]) == SEG_CAP - 1 and set(n_seg) == {1, 3} and sum(n_seg) > SEG_CAP
    recs = [r for _, r in both]
    stream = B.stream(recs, [("g", len(ref))])
    assert len(stream) < MAX_STREAM
    return [stream], [("g", fasta_lines(ref))], recs, n_seg


B_RUNS = [("errors", dict()), ("errors", dict(min_mapq=5)), ("pileup", dict()), ("pileup", dict(min_baseq=25, min_mapq=5)), ("consensus", dict()),
          ("call", dict())]


@pytest.mark.parametrize("stage,kw", B_RUNS, ids=lambda x: (",".join("%s=%s" % i for i in x.items()) or "defaults") if isinstance(x, dict) else x)
def test_a_file_of_more_segments_than_waves(ctx, stage, kw):
    """(--errors-bam has no smallest base quality: its second run moves the mapping quality alone.)  Then the same records shuffled
    over two files, one below the cap and one above it"""
    _, _, recs, n_seg = segments_input()
    r = through(ctx, stage, "segments", **kw)
    assert r.counts[8] == (len(recs) if not kw else r.counts[0] - r.counts[3]) > SEG_CAP and r.counts[0] == len(recs) and (r.counts[3] > 0) == bool(kw)
    if stage == "errors":
        assert r.totals[0] > 30 * SEG_CAP and r.ins_len[1] > SEG_CAP // 4 and r.del_len[2] > SEG_CAP // 4
    else:
        assert r.ins_unanchored > SEG_CAP // 74
    order = list(range(len(recs)))
    random.Random(7).shuffle(order)
    assert sum(n_seg[k] for k in order[:60]) < 100 and sum(n_seg[k] for k in order[60:]) > SEG_CAP
    files = [B.stream([recs[k] for k in part], [("g", 20_000)]) for part in (order[:60], order[60:])]
    through(ctx, stage, "segments", streams=files, **kw)


# ---------------------------------------------------------------- C: one file past the log passes' cap
INS, GROUPS = 1000, 11


@functools.lru_cache(maxsize=None)
def log_input():
    """(streams, genome, the records): LOG_CAP / 1000 + 50 records of 30M 1000I 30M in eleven groups, each group on an anchor of its
    own, the inserted bases random; the last group's records have their I op over the cut at SEG_COLS columns"""
    rng = random.Random(LOG_CAP)
    n = LOG_CAP // INS + 50
    front = SEG_COLS - 400
    ref = planted(rng, 200 * (GROUPS - 1) + front + 110, longest=4)[:200 * (GROUPS - 1) + front + 100]
    recs = []
    for k in range(n):
        group = k * GROUPS // n
        ops = [(30 if group < GROUPS - 1 else front, "M"), (INS, "I"), (30, "M")]
        recs.append(aligned("i%d" % k, ops, pos=200 * group + 20, rng=rng, seqs={0: ref}, keep=1.0, qual="none"))
    assert n * INS > LOG_CAP and front < SEG_COLS < front + INS and n // GROUPS >= 3
    rng.shuffle(recs)
    stream = B.stream(recs, [("g", len(ref))])
    assert len(stream) < MAX_STREAM
    return [stream], [("g", fasta_lines(ref))], recs


@pytest.mark.parametrize("stage", ["consensus", "call"])
def test_a_file_of_more_log_entries_than_lanes(ctx, stage):
    r = through(ctx, stage, "log", max_ins=1024)
    if stage == "consensus":
        assert r.ins_longest == INS and r.ins_sites >= GROUPS and r.ins_len[63] == GROUPS and r.bases[3] >= GROUPS * INS
    else:
        assert r.longest_alt == INS + 1 and r.types[1] >= GROUPS
        inserted = [line.split(b"\t")[4] for line in lines_of(r.text) if line.endswith(b"TYPE=ins")]
        assert len(inserted) >= GROUPS and all(len(set(alt)) == 4 for alt in inserted if len(alt) == INS + 1)   # (votes, not one base repeated)


INPUTS = {"segments": segments_input, "log": log_input}
INPUTS.update({layout: functools.partial(seam_input, layout) for layout in LAYOUTS})


# ---------------------------------------------------------------- the inputs pass their caps: the stages' own summaries
CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")
CLI_RUNS = [("call", LAYOUTS[2], "tiles"), ("errors", "segments", "segments"), ("pileup", "segments", "segments"), ("consensus", "log", "log entries")]


@pytest.mark.parametrize("stage,name,cap", CLI_RUNS, ids=["%s of %s" % (s, c) for s, _, c in CLI_RUNS])
def test_cli_says_that_the_input_passes_its_cap(tmp_path, stage, name, cap):
    """a condition, not a measurement: the summary line that the stage prints with PBSIM_TRACE counts more segments or log entries in
    the one file than one trip takes, and the positions it counts lie in more tiles than the tile passes have workgroups; the same
    run's report and output are the model's"""
    streams, genome = INPUTS[name]()[:2]
    kw = dict(max_ins=1024) if name == "log" else dict()
    want = model(stage, name, tuple(kw.items()))
    fasta, data, out = tmp_path / "genome.fa", tmp_path / "in.bam", tmp_path / "out"
    fasta.write_bytes(b"".join(b">" + n.encode() + b"\n" + lines for n, lines in genome))
    data.write_bytes(B.contain(streams[0]))
    cmd = [CLI, "--%s-bam" % stage, str(data), "--%s-genome" % stage, str(fasta), "--%s-out" % stage, str(out)]
    cmd += [x for name_, v in kw.items() for x in ("--%s-%s" % (stage, name_.replace("_", "-")), str(v))]
    r = subprocess.run(cmd, capture_output=True, cwd=str(tmp_path), timeout=300, env=dict(os.environ, PBSIM_TRACE="1"))
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == want.report and out.read_bytes() == want.text
    said = re.search(rb"(\d+) genome records, (?:(\d+) positions, )?1 files, .* (\d+) segments(?:, (\d+) log entries)?", r.stderr)
    assert said, r.stderr[-4000:]
    positions, segments, logged = [int(v) if v is not None else None for v in said.group(2, 3, 4)]
    print("%s of %s: %s positions, %d segments, %s log entries" % (stage, name, positions, segments, logged))
    if cap == "tiles":
        lens = INPUTS[name]()[2]
        assert positions == sum(lens.values())
        assert (places(list(lens.values()) + [0])[-1] + TILE - 1) // TILE > max(SITE_BLOCKS, BASE_BLOCKS, LINE_BLOCKS)
    elif cap == "segments":
        assert segments > SEG_CAP
    else:
        assert logged > LOG_CAP
