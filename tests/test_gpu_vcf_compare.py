"""`pbsim --compare-vcf` (pbsim_vcf_compare) on the device, held to tests/compare_model.py byte for byte: the result, the report and the
annotated text under both settings of `lines`, with the text and without it."""
import functools
import os
import random
import subprocess

import pytest

import bam_writer as B
import bgzf_writer as W
import compare_model as M
import harness
import mutate_model as G
import pbsim3_amd as P
from test_call_model import lines_of
from test_compare_model import (WORKED_CALLS, WORKED_GENOME, WORKED_REPORT, WORKED_TEXT, WORKED_TEXT_ALL, WORKED_TRUTH, vcf)
from test_gpu_bam_grid_caps import constant
from test_mutate_model import spelling_reads

pytestmark = pytest.mark.gpu

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")
THREADS = constant("bam_pileup_walk.h", "kThreads")
TILE, TEXT_TILE = constant("vcf_compare.h", "kCmpTile"), constant("vcf_compare.h", "kCmpTextTile")
TILE_BLOCKS, LANE_BLOCKS = constant("vcf_compare.hip", "kTileBlocksMax"), constant("vcf_compare.hip", "kLaneBlocksMax")


@pytest.fixture(scope="module")
def ctx():
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR, seed=1), 0) as c:
        yield c


def numbers(result):
    return [x for name in ("files", "types", "lengths", "ms") for x in harness_flat(result[name])] + [result["text_bytes"]]


def harness_flat(v):
    return [x for item in v for x in harness_flat(item)] if isinstance(v, list) else [v]


def check(ctx, truth, calls, genome, modes=(0, 1), piece_bytes=0, **kw):
    """both texts through the product, every output against the model under each setting of `lines`, with the annotated text and
    without it; returns the model's result under the first setting"""
    first = None
    for lines in modes:
        want = M.compare(truth, calls, genome, lines=lines, **kw)
        got = ctx.compare_vcf(truth, calls, genome, lines=lines, piece_bytes=piece_bytes, **kw)
        assert len(got) == 3
        assert numbers(got[0]) == M.flat(want)
        assert got[1] == want.report
        assert got[2] == want.text
        bare = ctx.compare_vcf(truth, calls, genome, lines=("discordant", "all")[lines], text=False, **kw)
        assert len(bare) == 2 and numbers(bare[0]) == M.flat(want) and bare[1] == want.report
        first = first or want
    return first


def verdicts(r, w):
    return [row[8] for row in r.rows[w]]


# ---------------------------------------------------------------- the worked case
def test_the_worked_case(ctx):
    r = check(ctx, WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME)
    assert r.report == WORKED_REPORT and r.text == WORKED_TEXT
    assert ctx.compare_vcf(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME, lines="all")[2] == WORKED_TEXT_ALL
    check(ctx, WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME, min_ms=3)


def test_every_class_and_both_line_ends(ctx):
    genome = [("c1", b"ACGTNACGTACGT"), ("c2", b"acgtt")]
    rows = [b"c1\t2\t.\tC", b"\t2\t.\tC\tT", b"c1\t2\t.\t\tT", b"c1\t2\t.\tC\t", b"c1\t0\t.\tC\tT", b"c1\t2147483648\t.\tC\tT", b"c1\t2x\t.\tC\tT",
            b"c1\t\t.\tC\tT", b"c1\t+2\t.\tC\tT", b"c1\t99999999999999999999999\t.\tC\tT", b"c3\t2\t.\tC\tT", b"c\t2\t.\tC\tT", b"c11\t2\t.\tC\tT",
            b"C1\t2\t.\tC\tT", b"c1\t2\t.\tC\tT,G", b"c1\t2\t.\tC\t<DEL>", b"c1\t2\t.\tC\t*", b"c1\t2\t.\tC\t.", b"c1\t2\t.\tR\tT", b"c1\t2\t.\tG\tT",
            b"c1\t12\t.\tGTA\tG", b"c1\t14\t.\tA\tT", b"c2\t6\t.\tA\tT", b"c1\t2\t.\tC\tT\t.\tLowQual\tMS=9", b"c1\t2\t.\tC\tT\t.\t\tMS=9",
            b"c1\t2\t.\tC\tT\t.\tpass", b"c1\t2\t.\tC\tc", b"c2\t1\t.\tac\tAC\t.\tPASS", b"c1\t0000000002\t.\tc\tt\t.\tPASS\tDP=1;XMS=5;MS=7x;MS=9",
            b"c1\t5\t.\tN\tA\t.\t.", b"c2\t4\t.\tTT\tT\t.\t.\tMS=;MS=4", b"c1\t2\t.\tC\tT\t.\t.\tMS=99999999999\textra\tcolumns", b"c2\t2\t.\tcgt\tCTA\t.\t.\tMS=4;",
            b"c2\t1\t.\tA\tG\t.\t.\tMS=", b"c2\t1\t.\tA\tG\t.\t.\tDP=2;MS=12", b"\t", b"c1"]
    text = b"#head\n\n" + b"\n".join(rows) + b"\n"
    r = check(ctx, text, text, genome, min_ms=1)
    assert r.files[0][:9] == [37, 12, 4, 5, 4, 3, 2, 2, 5] and sum(r.types[3]) > 0
    crlf = text.replace(b"\n", b"\r\n")
    for t, c in ((crlf, text), (text[:-1], crlf[:-2]), (crlf[:-1], crlf + b"\r"), (b"\r", b"\r\n\r\n")):
        check(ctx, t, c, genome)


def test_a_header_only_file_and_an_empty_file(ctx):
    head = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n"
    for t, c in ((head, WORKED_CALLS), (WORKED_TRUTH, head), (b"", WORKED_CALLS), (WORKED_TRUTH, b""), (b"", b""), (head, head), (b"\n", b"#")):
        r = check(ctx, t, c, WORKED_GENOME)
        assert r.files[0][0] == (4 if t == WORKED_TRUTH else 0) and r.files[1][0] == (7 if c == WORKED_CALLS else 0)


# ---------------------------------------------------------------- the line table's tiles
BODY = b"c1\t2\t.\tC\tT\n\n#c\nc1\t6\t.\tA\tAA\r\n\r\n#\nc1\t8\t.\tCGT\tC\n\nc1\t14\t.\tA\tC"


@pytest.mark.parametrize("first", [TILE - 30, TILE - 12])
def test_lines_on_the_seams_of_the_line_tables_tiles(ctx, first):
    """the body -- data lines, empty lines with and without \\r, # lines, a last line without its line feed -- behind a # line of
    `first` + 0 .. 17 bytes: every one of its bytes comes to lie on a tile's last byte and on the next one's first, in the truth, and
    with the calls' own tiles behind a truth that ends on a tile's last byte, one short of it and one past it"""
    for k in range(18):
        pad = b"#" + b"x" * (first + k - 2) + b"\n"
        truth = pad + BODY
        assert len(pad) == first + k
        r = check(ctx, truth, WORKED_CALLS, WORKED_GENOME, modes=(1,))
        assert verdicts(r, 0) == ["found", "found", "found", "missed"]
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE):
        truth = b"#" + b"x" * (n - len(BODY) - 2) + b"\n" + BODY
        assert len(truth) == n
        r = check(ctx, truth, BODY, WORKED_GENOME, modes=(1,))
        assert verdicts(r, 0) == ["found"] * 4 and verdicts(r, 1) == ["tp"] * 4


def test_a_line_longer_than_a_tile(ctx):
    seq = harness.synth_bases(9000, 3).tobytes()
    genome = [("long", seq)]
    truth = vcf([("long", 11, seq[10:10 + 3 * TILE + 5].decode(), seq[10:11].decode()), ("long", 5000, seq[4999:5000].decode(), seq[4999:5000].decode() + "ACGT" * 700),
                 ("long", 8000, seq[7999:8003].decode(), "T" if seq[7999:8000] != b"T" else "G")])
    calls = vcf([("long", 5000, seq[4999:5000].decode(), seq[4999:5000].decode() + "ACGT" * 700, "MS=5"), ("long", 11, seq[10:10 + 3 * TILE + 5].decode(), seq[10:11].decode(), "MS=2"),
                 ("long", 5000, seq[4999:5000].decode(), seq[4999:5000].decode() + "ACGT" * 699 + "ACGA", "MS=1")])
    r = check(ctx, truth, calls, genome)
    assert verdicts(r, 0) == ["found", "found", "missed"] and verdicts(r, 1) == ["tp", "tp", "fp"] and r.lengths[1][4] == [1, 1, 1, 1] and r.lengths[0][4] == [1, 1, 2, 1]


# ---------------------------------------------------------------- runs of lines at one site
def insertions_at_one_site(n, seed):
    """a genome, and n distinct insertions behind one of its bases that all keep their place: (genome, anchor position, lines)"""
    rng = random.Random(seed)
    seq = harness.synth_bases(1500, 40 + seed).tobytes()
    p = 900
    last = [c for c in b"ACGT" if c != seq[p]][0]                   # X ends with it: nothing to trim, no step to the left
    xs = set()
    while len(xs) < n:
        xs.add(bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 7))) + bytes([last]))
    return seq, p, sorted(xs)


@pytest.mark.parametrize("n", [63, 64, 65, 300])
def test_a_run_of_lines_at_one_site(ctx, n):
    """n distinct insertions at one site, some in both files, some in one, with duplicates among them, behind enough snvs in front of
    the site that the run of equal keys begins a few places in front of the end of the match pass's first workgroup"""
    seq, p, xs = insertions_at_one_site(n, n)
    rng = random.Random(n)
    name = "g"
    snvs = [(name, q + 1, chr(seq[q]), "A" if seq[q] != 65 else "C") for q in range(100, 100 + (THREADS - 20) // 2)]
    ins = [(name, p + 1, chr(seq[p]), chr(seq[p]) + x.decode(), "MS=%d" % (k % 70)) for k, x in enumerate(xs)]
    in_truth = [i for k, i in enumerate(ins) if k % 3 != 0]
    in_calls = [i for k, i in enumerate(ins) if k % 3 != 1]
    in_truth += in_truth[::7]                                        # duplicates, scattered through the file
    in_calls += in_calls[::5] + in_calls[::11]
    rng.shuffle(in_truth)
    rng.shuffle(in_calls)
    truth, calls = vcf(snvs + in_truth), vcf(in_calls[:10] + snvs + in_calls[10:])
    r = check(ctx, truth, calls, [(name, seq)])
    both = len([k for k in range(n) if k % 3 == 2])
    assert r.types[1][:4] == [n - (n + 2) // 3, both, n - (n + 1) // 3, both] and r.files[0][7] > 0 and r.files[1][7] > r.files[0][7]
    assert r.types[1][4] == r.types[1][5] == n - (n + 1) // 3 - both


# ---------------------------------------------------------------- the left move
def test_left_moves_through_long_runs(ctx):
    """a homopolymer of 700 bases that begins at a record's position 0, behind a record that ends with the same base; one of 600 inside
    a record; a tandem repeat of 140 units of AC; the same indel written at the runs' right ends, in their middles and at their left
    ends; inserted units whose rotation differs between the files"""
    a, b = b"T" * 700 + harness.synth_bases(300, 5).tobytes(), harness.synth_bases(200, 6).tobytes() + b"G"
    c = b + b"A" * 600 + b"C" + b"AC" * 140 + b"GGT" + b"T" * 40
    genome = [("b", b + b"T" * 5), ("a", a), ("none", b""), ("c", c)]
    at = len(b) + 601                                               # the C in front of the repeat
    truth = vcf([("a", 700, "T", "TT"), ("a", 699, "TT", "T"), ("a", 650, "TTTTT", "TT"), ("c", len(b) + 600, "A", "AAA"), ("c", len(b) + 400, "AAAA", "A"),
                 ("c", at + 280, "C", "CACAC"), ("c", at + 200, "CAC", "C"), ("c", at + 100, "C", "CACACACACACACACACACACACACACACACAC"), ("b", 206, "T", "TT")])
    calls = vcf([("a", 1, "T", "TT", "MS=4"), ("a", 1, "TT", "T", "MS=5"), ("a", 300, "TTTT", "T", "MS=6"), ("c", len(b) + 1, "A", "AAA", "MS=7"),
                 ("c", len(b) + 1, "AAAA", "A", "MS=8"), ("c", at + 1, "A", "ACACA", "MS=9"), ("c", at + 3, "ACA", "A", "MS=10"),
                 ("c", at + 151, "A", "ACACACACACACACACACACACACACACACACA", "MS=11"), ("b", 201, "G", "GT", "MS=12"), ("c", at + 1, "A", "AAC", "MS=3")])
    r = check(ctx, truth, calls, genome)
    assert verdicts(r, 0) == ["found"] * 9 and verdicts(r, 1) == ["tp"] * 9 + ["fp"]
    assert r.files[0][9:] == [9, 699] and r.files[1][9:] == [4, 299] and [row[3] for row in r.rows[0][:3]] == [0, 0, 0]


def test_ref_names_permuted_and_an_empty_record(ctx):
    recs = [("r%d" % k, harness.synth_bases(150 + 37 * k, 60 + k).tobytes()) for k in range(5)]
    genome = recs[:2] + [("void", b"")] + recs[2:]
    t = G.mutate(genome, snv_ppm=60000, ins_ppm=40000, del_ppm=40000)
    calls = b"".join(l + b"\n" for k, l in enumerate(lines_of(t.vcf)) if k % 9)
    r = check(ctx, t.vcf, calls, genome)
    assert r.files[0][8] == t.variants and r.files[1][8] == sum(v[3] for v in r.types) > 50
    # other names for the same records, in the VCFs and in ref_names; the genome's own names no longer count
    names = ["chr_%s" % n for n, _ in genome]
    renamed = lambda text: b"".join((b"chr_" + l if not l.startswith(b"#") else l) + b"\n" for l in text.split(b"\n") if l)
    r2 = check(ctx, renamed(t.vcf), renamed(calls), genome, ref_names=names)
    assert r2.report == r.report
    assert check(ctx, t.vcf, calls, genome, ref_names=names).files[0][2] == t.variants
    # the names turned round: every line is looked up in another record
    turned = [n for n, _ in genome][::-1]
    r3 = check(ctx, t.vcf, calls, genome, ref_names=turned)
    assert r3.files[0][2] == 0 and r3.files[0][4] > 0
    with pytest.raises(P.PbsimError, match="pbsim_vcf_compare: ref_names: two genome records are named"):
        ctx.compare_vcf(t.vcf, calls, genome, ref_names=["a"] * 6)
    check(ctx, WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME)


def test_pieces_of_seven_bytes(ctx):
    import ctypes as C
    want = M.compare(WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME, lines=1)
    check(ctx, WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME, piece_bytes=7)
    pieces = []

    def take(user, ptr, n, offset):
        pieces.append((offset, C.string_at(ptr, n)))
        return 1
    keep = [(nm.encode(), bytes(lines)) for nm, lines in WORKED_GENOME]
    refs = (P.ErrorsRef * 1)(*[P.ErrorsRef(nm, C.cast(C.c_char_p(lines), C.c_void_p), len(lines)) for nm, lines in keep])
    opts, res = P.CompareOpts(1, 0, 7), P.CompareResult()
    sink = P.CompareSink(None, P.COMPARE_TEXT_CB(take))
    args = (ctx.h, refs, 1, None, WORKED_TRUTH, len(WORKED_TRUTH), WORKED_CALLS, len(WORKED_CALLS), C.byref(opts))
    assert ctx.lib.pbsim_vcf_compare(*args, C.byref(sink), C.byref(res)) == 1
    at = 0
    for offset, p in pieces:
        assert offset == at and 1 <= len(p) <= 7
        at += len(p)
    assert b"".join(p for _, p in pieces) == want.text and len(pieces) == -(-len(want.text) // 7) and res.text_bytes == len(want.text)
    # a sink that stops: the call fails, the result is zeroed, the context stays usable
    stop = P.CompareSink(None, P.COMPARE_TEXT_CB(lambda *a: 0))
    assert ctx.lib.pbsim_vcf_compare(*args, C.byref(stop), C.byref(res)) == 0
    assert b"sink aborted (text)" in ctx.lib.pbsim_last_error() and res.text_bytes == 0 and res.files[0][0] == 0
    check(ctx, WORKED_TRUTH, WORKED_CALLS, WORKED_GENOME)


# ---------------------------------------------------------------- past the caps of the grids
@functools.lru_cache(maxsize=None)
def many_lines():
    """a truth of the mutate model at high rates, with more lines than the per-line passes have lanes in one trip and more bytes than
    the line table's passes have tiles; the calls are the truth with one line in every 20000 given another ALT"""
    genome = [("big", harness.synth_bases(LANE_BLOCKS * THREADS * 3 // 4, 71).tobytes())]
    t = G.mutate(genome, snv_ppm=700000, ins_ppm=30000, del_ppm=30000, ext_ppm=100000)
    lines = lines_of(t.vcf)
    changed = []
    for k in range(777, len(lines), 20000):
        f = lines[k].split(b"\t")
        if len(f[3]) == 1 and len(f[4]) == 1:
            f[4] = b"N"
            lines[k] = b"\t".join(f)
            changed.append(k + 1)
    return genome, t.vcf, b"".join(l + b"\n" for l in lines), changed


def test_more_lines_than_one_trip_of_every_pass(ctx):
    genome, truth, calls, changed = many_lines()
    n = len(lines_of(truth))
    assert 2 * n > LANE_BLOCKS * THREADS + 20000 and len(truth) > (TILE_BLOCKS + 8) * TILE and 2 * n > (LANE_BLOCKS + 8) * TEXT_TILE
    assert any(k < LANE_BLOCKS * THREADS - n for k in changed) and any(k > LANE_BLOCKS * THREADS - n for k in changed)    # in both trips of the calls
    r = check(ctx, truth, calls, genome, modes=(0,))
    missed = [k + 1 for k, v in enumerate(verdicts(r, 0)) if v == "missed"]
    assert missed == changed and [k + 1 for k, v in enumerate(verdicts(r, 1)) if v == "fp_site"] == changed
    assert set(verdicts(r, 0)) == {"found", "missed", "dup"} and set(verdicts(r, 1)) == {"tp", "fp_site", "dup"}       # (equal indels in one homopolymer: dup)
    assert r.text.count(b"\n") == 1 + 2 * len(changed) + r.files[0][7] + r.files[1][7]


# ---------------------------------------------------------------- the loop closed on the device
def rightmost(text, genome):
    """the VCF's indels rewritten to their rightmost placement, one padding base in front: another text for the same variants"""
    seqs = {n: s.tobytes() for n, s in G.prepared_records(genome)}
    out, moved = [], 0
    for line in text.split(b"\n"):
        f = line.split(b"\t")
        if line.startswith(b"#") or not line or len(f[3]) == len(f[4]):
            out.append(line)
            continue
        seq, s = seqs[f[0]], int(f[1])                                # (s: the 0-based place behind the anchor)
        x, d = f[4][1:], len(f[3]) - 1
        s0 = s
        if x:
            while s < len(seq) and seq[s] == x[0]:
                x, s = x[1:] + x[:1], s + 1
        else:
            while s + d < len(seq) and seq[s] == seq[s + d]:
                s += 1
        moved += s != s0
        f[1], f[3], f[4] = b"%d" % s, seq[s - 1:s + d], seq[s - 1:s] + x
        out.append(b"\t".join(f))
    return b"\n".join(out), moved


@pytest.mark.parametrize("kw", [dict(snv_ppm=20000, ins_ppm=20000, del_ppm=20000), dict(snv_ppm=100000, ins_ppm=150000, del_ppm=150000, ext_ppm=300000)],
                         ids=["sparse", "dense"])
def test_mutate_call_compare(ctx, kw):
    genome = [("a", harness.synth_bases(3000, 81).tobytes()), ("b", (b"AC" * 40 + b"GGGGGGGGTTTTTTTTTT" + b"CAG" * 30) * 6)]
    result, _, fasta, truth, _, origins = ctx.mutate_genome(genome, origin=True, line_width=0, **kw)
    stream, _ = spelling_reads(genome, fasta, origins)
    called = ctx.bam_call(B.contain(stream), genome, max_ins=65535)
    r = check(ctx, truth, called[2], genome)
    n = result["variants"]
    assert n > 100 and r.files[0][0] == r.files[1][0] == n and sum(r.files[0][1:7]) == sum(r.files[1][1:7]) == 0
    assert set(verdicts(r, 0)) <= {"found", "dup"} and set(verdicts(r, 1)) <= {"tp", "dup"} and r.text == M.TEXT_HEADER + b"".join(
        l for l in M.compare(truth, called[2], genome, lines=1).text.splitlines(True) if b"\tdup\t" in l)
    assert sum(v[4] for v in r.types) == 0 and [v[1] for v in r.types] == [v[0] for v in r.types] == [v[3] for v in r.types]
    # the truth's indels at their rightmost placement: no line of the two files is the same now, every form still is
    right, moved = rightmost(truth, genome)
    assert moved > 20 and len(set(lines_of(right)) & set(lines_of(truth))) < n - moved + 1
    r2 = check(ctx, right, called[2], genome)
    assert M.flat(r2)[22:-1] == M.flat(r)[22:-1] and verdicts(r2, 0) == verdicts(r, 0) and verdicts(r2, 1) == verdicts(r, 1)
    assert r2.files[0][:9] == r.files[0][:9] and r2.files[0][9] > r.files[0][9] and r2.files[0][10] >= r.files[0][10]     # (the trims take part of the way back)


# ---------------------------------------------------------------- through the command line
def test_cli_with_plain_and_bgzf_inputs(ctx, tmp_path):
    genome = [("a", harness.synth_bases(1200, 91).tobytes()), ("b", harness.synth_bases(900, 92).tobytes())]
    t = G.mutate(genome, seed=5, snv_ppm=30000, ins_ppm=30000, del_ppm=30000)
    truth, _ = rightmost(t.vcf, genome)
    calls = b"".join(l + b"\tDP=9;MS=%d\n" % (k % 9) for k, l in enumerate(b"\t".join(l.split(b"\t")[:7]) for l in lines_of(t.vcf)) if k % 7)
    calls += b"a\t5\t.\t%s\tN\t.\t.\tMS=2\n" % genome[0][1][4:5]
    fa = b"".join(b">" + n.encode() + b" words\n" + b"\n".join(s[k:k + 70] for k in range(0, len(s), 70)) + b"\n" for n, s in genome)
    for name, data in (("truth.vcf", truth), ("calls.vcf", calls), ("genome.fa", fa)):
        (tmp_path / name).write_bytes(data)
        (tmp_path / (name + ".gz")).write_bytes(W.bgzf(data, block=900))
    for gz, extra, kw in (("", [], dict()), (".gz", ["--compare-lines", "all", "--compare-min-ms", "3"], dict(lines=1, min_ms=3))):
        want = M.compare(truth, calls, genome, **kw)
        cmd = [CLI, "--compare-vcf", "calls.vcf" + gz, "--compare-truth", "truth.vcf" + gz, "--compare-genome", "genome.fa" + gz, "--compare-out", "out.tsv"]
        r = subprocess.run(cmd + extra, capture_output=True, cwd=str(tmp_path), timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        assert r.stdout == want.report and (tmp_path / "out.tsv").read_bytes() == want.text and want.files[1][8] > 50
        api = ctx.compare_vcf(truth, calls, genome, **kw)
        assert api[1] == r.stdout and api[2] == want.text
    # no --compare-out: the report alone; names turned round by --compare-ref-names; a failure leaves no file behind
    r = subprocess.run([CLI, "--compare-vcf", "calls.vcf", "--compare-truth", "truth.vcf", "--compare-genome", "genome.fa"], capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and r.stdout == M.compare(truth, calls, genome).report
    r = subprocess.run([CLI, "--compare-vcf", "calls.vcf", "--compare-truth", "truth.vcf", "--compare-genome", "genome.fa", "--compare-ref-names", "b,a"],
                       capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and r.stdout == M.compare(truth, calls, genome, ref_names=["b", "a"]).report
    r = subprocess.run([CLI, "--compare-vcf", "calls.vcf", "--compare-truth", "truth.vcf", "--compare-genome", "genome.fa", "--compare-ref-names", "a",
                        "--compare-out", "bad.tsv"], capture_output=True, cwd=str(tmp_path), timeout=300)
    assert r.returncode != 0 and b"(compare-ref-names): 1 names for 2 genome records" in r.stderr and not (tmp_path / "bad.tsv").exists()
