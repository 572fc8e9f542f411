"""tests/lift_model.py, the contract of pbsim_bam_lift, against hand-written cases and against an independent statement of the same
thing: the explicit variant -> original pairwise alignment composed column by column with the read's alignment.  Then what needs no
device: the report, the option mirror and the binary's refusals, the bad arguments, and bam_lift_rule.cpp under the sanitizers."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_writer as B
import harness
import lift_model as L
import pbsim3_amd as P
import pbsim3_amd.args as A

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")
OPS = "MIDNSHP=X"
FRONT = L.FRONT


def cigar(text):
    """'3M1D2I' -> [(3, 0), (1, 2), (2, 1)]"""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n), OPS.index(ch)))
            n = ""
    return out


def spell(ops):
    return "".join("%d%s" % (n, OPS[op]) for n, op in ops)


def lifted(pos, text, origin):
    got = L.lift_record(pos, cigar(text), origin)
    return None if got is None else (got[0], spell(got[1]))


# ---------------------------------------------------------------- generators, shared with the GPU tests
def random_origin(rng, l_orig, rate=0.05, front=False):
    """an origin map over an original record of l_orig bases: deletions and insertions at `rate` each, runs of 1 .. 6"""
    out, p, last = [], 0, -1
    if front:
        out += [FRONT] * int(rng.integers(1, 4))
    while p < l_orig:
        e = rng.random()
        if e < rate and p + 1 < l_orig:
            p += int(rng.integers(1, 7))                    # deleted
            continue
        out.append(p)
        last = p
        p += 1
        if e > 1 - rate:
            out += [-1 - last] * int(rng.integers(1, 7))    # inserted behind it
    return np.array(out, dtype=np.int32)


def random_cigar(rng, room, n_ops, clips=True):
    """ops that span at most `room` reference bases: M = X I D in small runs, clips around them"""
    ops, span = [], 0
    for _ in range(n_ops):
        op = int(rng.choice([0, 0, 0, 7, 8, 1, 2]))
        n = int(rng.integers(1, 6))
        if op != 1:
            n = min(n, room - span)
            if n <= 0:
                break
            span += n
        if ops and ops[-1][1] == op:
            continue
        ops.append((n, op))
    if not ops:
        ops = [(1, 0)] if room >= 1 else [(1, 1)]
    if clips and rng.random() < 0.4:
        ops = [(int(rng.integers(1, 4)), 4)] + ops
        if rng.random() < 0.5:
            ops = [(int(rng.integers(1, 4)), 5)] + ops
    if clips and rng.random() < 0.4:
        ops = ops + [(int(rng.integers(1, 4)), 4)]
        if rng.random() < 0.5:
            ops = ops + [(int(rng.integers(1, 4)), 5)]
    return ops


def random_record(rng, k, ref_id, l_var, n_ops=None, qual=True, extra_tags=True):
    """an aligned record on a variant record of l_var bases, with a wrong NM and other tags around it"""
    pos = int(rng.integers(0, max(l_var - 1, 1)))
    ops = random_cigar(rng, l_var - pos, n_ops or int(rng.integers(1, 30)))
    l_seq = sum(n for n, op in ops if op in (0, 1, 4, 7, 8))
    seq = "".join(rng.choice(list("ACGTACGTACGTN=")) for _ in range(l_seq))
    q = bytes(int(x) for x in rng.integers(0, 60, l_seq)) if qual else b"\xff" * l_seq
    tags = []
    if extra_tags:
        tags = [("RG", "Z", "grp%d" % (k % 3)), ("NM", "C", 7), ("ip", "BC", bytes(range(k % 19))), ("zm", "i", k)][int(rng.integers(0, 3)):]
    return B.record("r%d" % k, flag=int(rng.choice([0, 16])), ref_id=ref_id, pos=pos, cigar=[(n, OPS[op]) for n, op in ops], seq=seq, qual=q,
                    tags=tags, mapq=int(rng.integers(0, 61)))


def random_genome(rng, sizes):
    return [("chr%d" % k, bytes(rng.choice(list(b"ACGTACGTACGTN"), n).astype(np.uint8))) for k, n in enumerate(sizes)]


def header_text(refs, so="coordinate"):
    return ("@HD\tVN:1.6\tSO:%s\n" % so + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) + "@PG\tID:x\tLN:12\n").encode()


def parse_stream(stream):
    """(header bytes, [record bytes]) of an inflated BAM stream"""
    l_text = struct.unpack_from("<i", stream, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    head, recs = stream[:at], []
    while at < len(stream):
        n = 4 + struct.unpack_from("<I", stream, at)[0]
        recs.append(stream[at:at + n])
        at += n
    return head, recs


def record_fields(rec):
    """pos, the CIGAR of the field as text, NM (None without), the tags' names in order"""
    ref_id, pos, l_name, mapq, bin_, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
    at = 36 + l_name
    ops = [(x >> 4, x & 15) for x in struct.unpack_from("<%dI" % n_cigar, rec, at)]
    aux = L._aux_fields(rec, at + 4 * n_cigar + (l_seq + 1) // 2 + l_seq)
    nm = [f for tag, f in aux if tag == b"NM"]
    return dict(pos=pos, cigar=spell(ops), nm=None if not nm else int.from_bytes(nm[0][3:], "little"), tags=[t.decode() for t, _ in aux], bin=bin_,
                flag=flag, mapq=mapq, ref_id=ref_id)


# ---------------------------------------------------------------- the independent statement
def naive(pos, ops, origin, seq=None, bases=None):
    """the explicit pairwise alignment of the variant record with the original one, composed with the read's alignment column by
    column: (pos, CIGAR, NM) or None"""
    pair, last = [], -1                      # (variant base or None, original base or None)
    for v, o in enumerate(origin):
        if o >= 0:
            pair += [(None, p) for p in range(last + 1, int(o))]
            pair.append((v, int(o)))
            last = int(o)
        else:
            pair.append((v, None))
    where = {v: k for k, (v, _) in enumerate(pair) if v is not None}
    read, v, q, left_h, right_h = [], pos, 0, 0, 0
    for n, op in ops:
        for _ in range(n):
            if op in (0, 7, 8):
                read.append((q, v))
                q, v = q + 1, v + 1
            elif op == 1:
                read.append((q, None))
                q += 1
            elif op == 2:
                read.append((None, v))
                v += 1
            elif op == 4:
                q += 1
            elif op == 5:
                if read:
                    right_h += 1
                else:
                    left_h += 1
    composed, before = [], None
    for q1, v1 in read:
        if v1 is None:
            composed.append((q1, None))
            continue
        k = where[v1]
        if before is not None:
            composed += [(None, p) for _, p in pair[before + 1:k]]
        composed.append((q1, pair[k][1]))
        before = k
    composed = [c for c in composed if c != (None, None)]
    both = [k for k, c in enumerate(composed) if c[0] is not None and c[1] is not None]
    if not both:
        return None
    core = composed[both[0]:both[-1] + 1]
    left, right = core[0][0], q - 1 - core[-1][0]
    text, nm = "", 0
    for c in core:
        text += "M" if None not in c else "I" if c[1] is None else "D"
        if None in c:
            nm += 1
        elif seq is not None:
            a, b = bases[c[1]:c[1] + 1].upper(), seq[c[0]]
            nm += a in b"ACGT" and b in "ACGT" and a != b.encode()
    runs = []
    for ch in text:
        if runs and runs[-1][1] == ch:
            runs[-1][0] += 1
        else:
            runs.append([1, ch])
    out = [(left_h, "H"), (left, "S")] + [tuple(r) for r in runs] + [(right, "S"), (right_h, "H")]
    return core[0][1], "".join("%d%s" % r for r in out if r[0]), nm


def test_the_model_agrees_with_the_composed_alignments():
    rng = np.random.default_rng(11)
    seen = dict(none=0, moved=0, same=0)              # (same: the placeholder test below has a record that stays as it is)
    for case in range(300):
        l_orig = int(rng.integers(20, 120))
        genome = random_genome(rng, [l_orig])
        origin = random_origin(rng, l_orig, rate=0.08, front=case % 7 == 0)
        assert L.check_origin(origin, l_orig) is None
        rec = random_record(rng, case, 0, len(origin), n_ops=int(rng.integers(1, 12)))
        ops = [(n, OPS.index(op)) for n, op in rec["cigar"]]
        want = naive(rec["pos"], ops, origin, rec["seq"], genome[0][1])
        stream = B.stream([rec], refs=[("chr0", len(origin))])
        out, res = L.lift_stream(stream, genome, [origin])
        recs = parse_stream(out)[1]
        if want is None:
            assert recs == [] and res["unplaced"] == 1
            seen["none"] += 1
            continue
        f = record_fields(recs[0])
        assert (f["pos"], f["cigar"], f["nm"]) == want, (case, rec["pos"], rec["cigar"], origin.tolist())
        seen["moved" if res["moved"] else "same"] += 1
    assert seen["none"] > 0 and seen["moved"] > 0, seen


# ---------------------------------------------------------------- hand-written cases
#   the original   0 1 2 3 4 5 . . 6 7      3 is deleted, two bases are inserted behind 5
#   the variant    0 1 2   3 4 5 6 7 8
ORIGIN = [0, 1, 2, 4, 5, -6, -6, 6, 7]


def test_hand_written_records():
    same = list(range(9))
    assert lifted(2, "4M", same) == (2, "4M")                              # an SNV changes nothing of the placement
    assert lifted(0, "9M", ORIGIN) == (0, "3M1D2M2I2M")                    # a deletion and an insertion under M
    assert lifted(3, "1M3D1M", ORIGIN) == (4, "1M1D1M")                    # an insertion under D vanishes
    assert lifted(4, "1M2I2M1M", ORIGIN) == (5, "1M4I1M")                  # next to a read's I: the runs merge
    assert lifted(1, "1M2D1M", ORIGIN) == (1, "1M3D1M")                    # a variant deletion inside a read's D
    assert lifted(3, "2M", ORIGIN) == (4, "2M")                            # the deletion just in front of the first column: no D
    assert lifted(0, "3M", ORIGIN) == (0, "3M")                            # ... and just behind the last
    assert lifted(2, "1M1I1M", ORIGIN) == (2, "1M1I1D1M")                  # 2D1I3D-like orders stand: nothing is canonicalised
    assert lifted(2, "1D2M", ORIGIN) == (4, "2M")                          # D columns in front of the first M are dropped, the gap too
    assert lifted(5, "2M2M", ORIGIN) == (6, "2S2M")                        # a read that starts inside the insertion
    assert lifted(3, "2M2M", ORIGIN) == (4, "2M2S")                        # ... and one that ends inside it
    assert lifted(5, "2M", ORIGIN) is None                                 # wholly inside it: unplaced
    assert lifted(5, "1M1D", ORIGIN) is None
    assert lifted(2, "2H3S2M1I1M1S1H", ORIGIN) == (2, "2H3S1M1D1M1I1M1S1H")   # clips stay, H outermost
    assert lifted(4, "1S3M2S", ORIGIN) == (5, "1S1M4S")                    # S merges with the new S
    assert lifted(0, "2=1X", ORIGIN) == (0, "3M")                          # = and X come back as M
    front = [FRONT, FRONT, 0, 1, -2, 2]
    assert L.check_origin(front, 3) is None
    assert lifted(0, "6M", front) == (0, "2S2M1I1M")                       # an insertion in front of position 0
    assert lifted(0, "2M", front) is None
    wide = [0, 1, 50, 51]                                                  # a deletion that spans the read's neighbourhood
    assert lifted(0, "4M", wide) == (0, "2M48D2M")
    assert lifted(1, "1M1I1M", wide) == (1, "1M1I48D1M")


def one_record_stream(**kw):
    rec = B.record("r", **kw)
    return B.stream([rec], refs=[("c", len(ORIGIN))], text=header_text([("c", len(ORIGIN))]))


GENOME = [("c", b"ACGTACGT")]


def test_hand_written_streams():
    # variant bases: A C G A C x x G T ; the read spells the variant with one SNV at variant 1 and N at 4
    stream = one_record_stream(flag=16, ref_id=0, pos=0, cigar=[(9, "M")], seq="ATGANGGGT", qual=bytes(9), tags=[("NM", "C", 1), ("XY", "Z", "k")], mapq=9)
    out, res = L.lift_stream(stream, GENOME, [ORIGIN])
    head, recs = parse_stream(out)
    f = record_fields(recs[0])
    assert (f["pos"], f["cigar"], f["nm"], f["tags"], f["flag"], f["mapq"]) == (0, "3M1D2M2I2M", 1 + 1 + 2, ["NM", "XY"], 16, 9)
    assert f["bin"] == L.reg2bin(0, 8) and res["moved"] == 1 and res["lifted"] == 1 and res["gap_del"] == 1 and res["bases_to_ins"] == 2
    assert b"SO:unsorted" in head and b"SN:c\tLN:8\n" in head and b"@PG\tID:x\tLN:12" in head and head.endswith(b"c\0" + struct.pack("<i", 8))
    assert res["bytes_in"] == len(stream) - len(B.header([("c", 9)], header_text([("c", 9)]))) and res["bytes_out"] == len(recs[0])
    # no bases: no NM; the tags that are not NM or CG stay in order
    out, res = L.lift_stream(one_record_stream(flag=0, ref_id=0, pos=0, cigar=[(9, "M")], seq="", tags=[("AA", "i", -5), ("NM", "i", 3), ("BB", "A", "x")]),
                             GENOME, [ORIGIN])
    f = record_fields(parse_stream(out)[1][0])
    assert f["nm"] is None and f["tags"] == ["AA", "BB"] and res["no_seq"] == 1
    # unmapped records are copied: flag 4, no reference, no CIGAR
    for kw in (dict(flag=4, ref_id=0, pos=0, cigar=[(2, "M")], seq="AC", qual=b"\1\2"), dict(flag=0, ref_id=-1, pos=-1, seq="AC", qual=b"\1\2"),
               dict(flag=0, ref_id=0, pos=3, seq="AC", qual=b"\1\2", tags=[("NM", "C", 1)])):
        stream = one_record_stream(**kw)
        out, res = L.lift_stream(stream, GENOME, [ORIGIN])
        assert parse_stream(out)[1] == parse_stream(stream)[1] and res["unaligned"] == 1 and res["lifted"] == 0
    # N and P ops: dropped
    for ops in ([(2, "M"), (2, "N"), (2, "M")], [(2, "M"), (1, "P"), (2, "M")]):
        out, res = L.lift_stream(one_record_stream(flag=0, ref_id=0, pos=0, cigar=ops, seq="ACGT", qual=bytes(4)), GENOME, [ORIGIN])
        assert parse_stream(out)[1] == [] and res["unsupported"] == 1 and res["records"] == 1
    out, res = L.lift_stream(one_record_stream(flag=0, ref_id=0, pos=5, cigar=[(2, "M")], seq="AC", qual=bytes(2)), GENOME, [ORIGIN])
    assert parse_stream(out)[1] == [] and res["unplaced"] == 1


def test_references_and_origin_maps_that_do_not_fit():
    good = one_record_stream(flag=0, ref_id=0, pos=0, cigar=[(2, "M")], seq="AC", qual=bytes(2))
    with pytest.raises(L.LiftError, match="l_ref 9 .* has 8 bases: this is not the genome these reads came from"):
        L.lift_stream(good, GENOME, [ORIGIN[:8]])
    with pytest.raises(L.LiftError, match="no record named \"c\""):
        L.lift_stream(good, [("d", b"ACGTACGT")], [ORIGIN])
    assert L.lift_stream(good, [("d", b"ACGTACGT")], [ORIGIN], ref_name="d")[1]["lifted"] == 1
    for bad, at in (([0, 1, 2, 4, 5, -6, -6, 6, 8], 8), ([0, 1, 2, 4, 4, -5, -5, 6, 7], 4), ([0, 1, 2, 4, 5, -5, -6, 6, 7], 5),
                    ([-1, 1, 2, 4, 5, -6, -6, 6, 7], 0), ([0, 1, 2, 4, 5, -6, FRONT, 6, 7], 6), ([0, 1, 3, 2, 5, -6, -6, 6, 7], 3)):
        with pytest.raises(L.LiftError, match="the origin map of \"c\" is not one: variant position %d:" % at):
            L.lift_stream(good, GENOME, [bad])
    with pytest.raises(L.LiftError, match="does not fit"):
        L.lift_stream(one_record_stream(flag=0, ref_id=0, pos=8, cigar=[(2, "M")], seq="AC", qual=bytes(2)), GENOME, [ORIGIN])
    with pytest.raises(L.LiftError, match="does not fit"):
        L.lift_stream(one_record_stream(flag=0, ref_id=0, pos=0, cigar=[(3, "M")], seq="AC", qual=bytes(2)), GENOME, [ORIGIN])


def test_the_placeholder_both_ways():
    n = 40000
    same = list(range(2 * n + 2))
    long_ops = [(1, "M"), (1, "I")] * n + [(1, "M")]                       # 80 001 ops
    seq = "A" * (2 * n + 1)
    genome = [("c", b"A" * len(same))]
    rec = B.record("big", flag=0, ref_id=0, pos=0, cigar=[(len(seq), "S"), (n + 1, "N")], seq=seq, qual=bytes(len(seq)),
                   tags=[("CG", "BI", [x << 4 | "MIDNSHP=X".index(op) for x, op in long_ops])])
    out, res = L.lift_stream(B.stream([rec], refs=[("c", len(same))]), genome, [same])
    f = record_fields(parse_stream(out)[1][0])
    assert f["cigar"] == "%dS%dN" % (len(seq), n + 1) and f["tags"] == ["NM", "CG"] and res["long_cigar_in"] == res["long_cigar_out"] == 1 and res["moved"] == 0


# ---------------------------------------------------------------- the report, the mirror, the binary
def test_the_report_needs_no_device():
    rng = np.random.default_rng(5)
    for _ in range(20):
        res = {k: int(rng.integers(0, 2 ** 40)) for k in L.COUNTS + L.TOTALS}
        assert P.lift_report(res) == L.report(res)
    assert P.LIFT_COUNTS == L.COUNTS and P.LIFT_TOTALS == L.TOTALS
    assert P.load().pbsim_lift_report(None, None, 0) == -1


GOOD = ["--lift-bam", "in.bam", "--lift-out", "out.bam", "--lift-genome", "g.fa", "--lift-vcf", "v.vcf"]
TAKES = "--lift-bam takes --lift-out, --lift-genome, --lift-vcf, --lift-haplotype, --lift-sample, --lift-ref-names, --lift-ref-name and --device"
REFUSED = [
    (GOOD + ["--depth", "3"], "(--depth): " + TAKES),
    (GOOD + ["--genome", "x"], "(--genome): " + TAKES),
    (GOOD + ["--mutate-origin", "x"], "(--mutate-origin): " + TAKES),
    (GOOD + ["--apply-vcf", "x"], "(--lift-bam): --apply-vcf takes"),
    (GOOD + ["--mutate-genome", "x"], "(--lift-bam): --mutate-genome takes"),
    (GOOD + ["--errors-bam", "x"], "(--lift-bam): --errors-bam takes"),
    (["--lift-out", "o", "--lift-bam"], "needs a value"),
    (["--lift-bam", "b", "--lift-genome", "g", "--lift-vcf", "v"], "--lift-bam needs --lift-out FILE"),
    (["--lift-bam", "b", "--lift-out", "o", "--lift-vcf", "v"], "--lift-bam needs --lift-genome FASTA"),
    (["--lift-bam", "b", "--lift-out", "o", "--lift-genome", "g"], "--lift-bam needs --lift-vcf VCF"),
    (GOOD + ["--lift-haplotype", "3"], "(lift-haplotype: 3): 0 (the first ALT of every line), 1 or 2."),
    (GOOD + ["--lift-haplotype", "x"], "(lift-haplotype: x): 0 (the first ALT of every line), 1 or 2."),
    (GOOD + ["--lift-sample", ""], "(lift-sample): a 0-based sample column or a sample's name."),
    (GOOD + ["--lift-ref-names", "a,,b"], "(lift-ref-names): an empty name."),
    (GOOD + ["--lift-ref-names", ""], "(lift-ref-names): an empty name."),
]
OTHER_MODES = ("--apply-vcf", "--mutate-genome", "--errors-bam")


def test_option_mirror():
    got = A.lift_bam(GOOD + ["--lift-haplotype", "2", "--lift-sample", "NA1", "--lift-ref-names", "a,b", "--lift-ref-name", "chr1", "--device", "1"])
    assert got == dict(bam="in.bam", out="out.bam", genome="g.fa", vcf="v.vcf", haplotype=2, sample="NA1", ref_names=["a", "b"], ref_name="chr1")
    assert A.lift_bam(GOOD + ["--lift-sample", "3"])["sample"] == 3
    for argv, message in REFUSED + [(["--lift-out", "o"], "--lift-bam IN: name the BAM file")]:
        if any(m in argv for m in OTHER_MODES):
            continue                                # (the binary hands that line to the other stage's mode, which refuses it)
        with pytest.raises(ValueError) as e:
            A.lift_bam(argv)
        assert message in str(e.value), argv


def test_cli_refuses_from_the_command_line_alone(tmp_path):
    """the same refusals by the binary, with the mirror's words, before a device or a file is touched"""
    import pbsim3_amd.build as b
    b.build()
    for argv, message in REFUSED:
        r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
        assert r.returncode != 0 and r.stdout == "" and message in r.stderr, (argv, r.stderr[-500:])
    r = subprocess.run([CLI] + GOOD, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "Cannot open file: in.bam" in r.stderr
    assert os.listdir(tmp_path) == []
    r = subprocess.run([CLI], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert "--lift-bam IN --lift-out OUT --lift-genome FASTA --lift-vcf VCF" in r.stderr + r.stdout


def test_bad_arguments_fail_before_device_work():
    stream = one_record_stream(flag=0, ref_id=0, pos=0, cigar=[(2, "M")], seq="AC", qual=bytes(2))
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), -1) as c:
        with pytest.raises(P.PbsimError, match="pbsim_bam_lift: bad argument"):
            c.lift_bam(stream, [], [])
        with pytest.raises(P.PbsimError, match=r"pbsim_bam_lift: the genome holds two records named \"c\""):
            c.lift_bam(stream, GENOME + GENOME, [ORIGIN, ORIGIN])
        with pytest.raises(ValueError, match="one map per genome record"):
            c.lift_bam(stream, GENOME, [])
        with pytest.raises(ValueError, match="one entry per genome record"):
            c.lift_bam(stream, GENOME, [ORIGIN], ref_names=["a", "b"])
        with pytest.raises(P.PbsimError, match="no HIP device"):
            c.lift_bam(stream, GENOME, [ORIGIN])


# ---------------------------------------------------------------- the host's decisions under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("asan") / "bam_lift_rule_driver")
    p = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(harness.ROOT, "tests", "asan", "bam_lift_rule_driver.cpp"), os.path.join(csrc, "bam_lift_rule.cpp"),
                        "-o", exe], capture_output=True, text=True)
    if p.returncode != 0 and "sanitize" in p.stderr:
        pytest.skip("no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def drive(exe, *argv):
    p = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, timeout=60)
    assert p.returncode == 0, (argv, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout


def test_rule_code_under_asan(driver, tmp_path):
    rng = np.random.default_rng(3)
    for _ in range(5):
        res = {k: int(rng.integers(0, 2 ** 50)) for k in L.COUNTS + L.TOTALS}
        assert drive(driver, "report", *[res[k] for k in L.COUNTS + L.TOTALS]) == L.report(res)
    texts = [header_text([("a", 9), ("b", 7)]), header_text([("a", 9)], so="unknown")[:-1], b"", b"@SQ\tSN:a", b"@CO\t@HD\tSO:x\n@SQ\tLN:5\tSN:b\tLN:6\n\n",
             b"@HD\tVN:1.6\n@SQ\tSN:zz\tLN:3\n", b"@HD\tSO:coordinate\tGO:none\0\0"]
    for k, text in enumerate(texts):
        refs = [("a", 9), ("b", 7)]
        path = tmp_path / ("%d.bin" % k)
        path.write_bytes(B.header(refs, text))
        want = B.header([("a", 100), ("b", 2000000000)], L.rewrite_text(text, [b"a", b"b"], [100, 2000000000]))
        assert drive(driver, "header", path, 100, 2000000000) == want, text
    assert drive(driver, "args", 0, 5) == b"args ok\n"
    assert drive(driver, "args", 1, 5).startswith(b"args refused: origin map 1 is missing")
    assert drive(driver, "args", 2, 5).startswith(b"args refused: origin map 0 has 2147483647 bases")
    assert drive(driver, "args", 3, 5).startswith(b"args refused: bad argument")
    for kind, word in ((1, b"outside the original record"), (2, b"do not rise strictly"), (3, b"does not name the last kept base")):
        assert word in drive(driver, "fault", kind)
