"""tests/call_model.py (the rule of `pbsim --call-bam`) held to a case worked out by hand, to the consensus model through an applier of
its own, and to the edge cases of the grouping; and the places where the feature shows without a GPU: the ABI's declarations with
their ctypes mirror and the built library's symbols, pbsim_call_report against the model, the option mirror with the command line's
refusals, the checks in front of any device work, and the HIP-free rule file under the sanitizers."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import bam_writer as B
import call_model as V
import consensus_model as K
import harness
import pbsim3_amd as P
import pileup_model as M
from pbsim3_amd import args as A
from test_consensus_model import GENOME, REFS, WORKED
from test_pileup_model import GENOME as PILE_GENOME, WORKED as PILE_WORKED, WORKED_REFS as PILE_REFS, rec, small_case

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")

# ---------------------------------------------------------------- the worked case of the rule
# The consensus's worked case (tests/test_consensus_model.py): c1 A C G T A C G T A C, c2 G G R T T.
# c1 1        a sub_site, T, by 3 of depth 4: an snv.
# c1 2, 3     G, then the del_site 3 (del 2): the group of the anchor G at depth 3: GT -> G.
# c1 5        C with the insertion GA behind it, n = 3 and 3: C -> CGA.
# c1 7        T with A behind it, n = 2: T -> TA.           c1 8: A with N behind it, n = 2: A -> AN.
# c1 9, c2    low, ref_n and concordant sites spell the genome: nothing.
WORKED_HEADER = (b"##fileformat=VCFv4.2\n##source=pbsim3_amd\n##contig=<ID=c1,length=10>\n##contig=<ID=c2,length=5>\n"
                 b"##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth of the pile at the record's anchor: A + C + G + T + other + del\">\n"
                 b"##INFO=<ID=MS,Number=1,Type=Integer,Description=\"Minimum support: the smallest count behind a substituted, deleted or inserted base "
                 b"of the record\">\n"
                 b"##INFO=<ID=TYPE,Number=1,Type=String,Description=\"snv, ins, del or complex\">\n"
                 b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
WORKED_LINES = (b"c1\t2\t.\tC\tT\t.\t.\tDP=4;MS=3;TYPE=snv\n"
                b"c1\t3\t.\tGT\tG\t.\t.\tDP=3;MS=2;TYPE=del\n"
                b"c1\t6\t.\tC\tCGA\t.\t.\tDP=3;MS=3;TYPE=ins\n"
                b"c1\t8\t.\tT\tTA\t.\t.\tDP=3;MS=2;TYPE=ins\n"
                b"c1\t9\t.\tA\tAN\t.\t.\tDP=3;MS=2;TYPE=ins\n")
WORKED_REPORT = (b"# records=6 skipped_flag=0 unaligned=0 skipped_mapq=0 skipped_ref=0 aligned=6 no_seq=0 misfit=0 scored=6\n"
                 b"S\t15\t1\t1\t13\t11\t1\t1\t3\t5\t384615\t4149\n"
                 b"V\t5\t1\t3\t1\t0\t6\t9\t2\t3\t0\t0\n")
# the options moved off their defaults, one at a time (dicts of the model's keyword arguments)
WORKED_OPTIONS = [dict(max_ins=1), dict(max_ins=2), dict(min_depth=4), dict(min_depth=0), dict(min_mapq=61), dict(exclude_flags=0), dict(min_baseq=1),
                  dict(max_ins=1, min_depth=2, min_mapq=60, exclude_flags=0x10)]


def worked(**kw):
    return V.call(B.stream(WORKED, REFS), GENOME, **kw)


def lines_of(text):
    return [line for line in text.split(b"\n") if line and not line.startswith(b"#")]


def test_the_worked_case():
    r = worked()
    assert r.text == WORKED_HEADER + WORKED_LINES and r.report == WORKED_REPORT
    assert (r.header_bytes, r.text_bytes) == (len(WORKED_HEADER), len(WORKED_HEADER) + len(WORKED_LINES)) and r.records == [(10, 5), (5, 0)]
    assert r.counts == [6, 0, 0, 0, 0, 6, 0, 0, 6] and r.sites == [15, 1, 1, 13, 11, 1, 1, 3, 5] and (r.ins_unanchored, r.max_depth) == (1, 4)
    assert (r.variants, r.types) == (5, [1, 3, 1, 0]) and (r.ref_bases, r.alt_bases, r.longest_ref, r.longest_alt) == (6, 9, 2, 3)
    assert (r.unplaced_records, r.unplaced_sites) == (0, 0)
    one = worked(max_ins=1)
    assert lines_of(one.text)[2] == b"c1\t6\t.\tC\tCG\t.\t.\tDP=3;MS=3;TYPE=ins" and one.alt_bases == 8 and worked(max_ins=2).text == r.text
    # at min_depth 4 only the first two sites of c1 are called: the snv alone
    assert lines_of(worked(min_depth=4).text) == [WORKED_LINES.split(b"\n")[0]]
    assert worked(min_mapq=61).variants == 0 and worked(min_mapq=61).text == WORKED_HEADER and worked(exclude_flags=0).text == r.text
    # two files give what one gives, in either order
    assert V.call([B.stream(WORKED[3:], REFS), B.stream(WORKED[:3], REFS)], GENOME) == r


def test_the_front_half_is_the_other_models():
    for streams, genome in (([B.stream(WORKED, REFS)], GENOME), ([B.stream(PILE_WORKED, PILE_REFS)], PILE_GENOME)):
        for kw in (dict(), dict(min_depth=2), dict(min_baseq=20, min_mapq=8), dict(exclude_flags=0)):
            v, m = V.call(streams, genome, **kw), M.pileup(streams, genome, **kw)
            assert (v.counts, v.sites, v.ins_unanchored, v.max_depth) == (m.counts, m.sites, m.ins_unanchored, m.max_depth)
            assert v.report.split(b"\n")[:2] == m.report.split(b"\n")[:2]


# ---------------------------------------------------------------- the apply property
def apply(text, genome):
    """the records applied to the prepared genome, as one-line FASTA: knows nothing of groups"""
    prepared = K.prepare_genome(genome)
    edits = {}
    for line in lines_of(text):
        name, pos, _, ref, alt = line.split(b"\t")[:5]
        edits.setdefault(name, []).append((int(pos) - 1, ref, alt))
    out = []
    for name, _ in genome:
        name = name.encode() if isinstance(name, str) else bytes(name)
        seq, got, at = prepared[name][0].tobytes(), b"", 0
        for pos, ref, alt in edits.pop(name, []):
            assert pos >= at and seq[pos:pos + len(ref)] == ref and ref != alt        # ascending, not overlapping, REF is the genome's
            got, at = got + seq[at:pos] + alt, pos + len(ref)
        got += seq[at:]
        out.append(b">" + name + b"\n" + (got + b"\n" if got else b""))
    assert not edits
    return b"".join(out)


def test_the_records_applied_to_the_genome_give_the_consensus():
    for streams, genome in (([B.stream(WORKED, REFS)], GENOME), ([B.stream(PILE_WORKED, PILE_REFS)], PILE_GENOME)):
        for kw in (dict(), dict(min_depth=2, max_ins=1)):
            assert apply(V.call(streams, genome, **kw).text, genome) == K.consensus(streams, genome, fill="ref", line_width=0, **kw).text
    # the pileup's worked case has a deleted base that the insertion at its own site puts back: g2 6 .. 7, T +A then the deleted A
    r = V.call(B.stream(PILE_WORKED, PILE_REFS), PILE_GENOME)
    assert lines_of(r.text) == [b"g1\t5\t.\tA\tC\t.\t.\tDP=2;MS=1;TYPE=snv", b"g1\t10\t.\tT\tTC\t.\t.\tDP=1;MS=1;TYPE=ins"]
    assert r.sites[8] == 4 and r.variants == 2


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_the_apply_property_on_random_inputs(seed):
    genome, refs, recs, _ = small_case(seed)
    stream = B.stream(recs, refs)
    types = [0] * 4
    for kw in (dict(), dict(min_depth=2, min_baseq=20, max_ins=2)):
        r = V.call(stream, genome, **kw)
        assert apply(r.text, genome) == K.consensus(stream, genome, fill="ref", line_width=0, **kw).text
        assert r.variants == len(lines_of(r.text)) == sum(r.types) == sum(n for _, n in r.records) and r.text_bytes == len(r.text)
        for line in lines_of(r.text):
            f = line.split(b"\t")
            info = dict(item.split(b"=") for item in f[7].split(b";"))
            assert f[2] == f[5] == f[6] == b"." and 1 <= int(info[b"MS"]) and 1 <= int(info[b"DP"]) and info[b"TYPE"].decode() == V.kind_of(f[3], f[4])
        types = [a + b for a, b in zip(types, r.types)]
    assert all(n > 5 for n in types[:3]) and types[3] > 0


# ---------------------------------------------------------------- the edges of the grouping
def test_a_leading_run_goes_to_the_records_first_anchor():
    r = V.call(B.stream([rec("x%d" % k, 0, "1S2D2M", "ATT") for k in range(3)], [("a", 4)]), [("a", b"ACGT\n")])
    assert lines_of(r.text) == [b"a\t1\t.\tACG\tT\t.\t.\tDP=3;MS=3;TYPE=complex"] and r.types == [0, 0, 0, 1] and (r.longest_ref, r.longest_alt) == (3, 1)
    # the anchor behind the run is concordant: REF ends with it, ALT is it
    r = V.call(B.stream([rec("x%d" % k, 0, "1S2D2M", "AGT") for k in range(3)], [("a", 4)]), [("a", b"ACGT\n")])
    assert lines_of(r.text) == [b"a\t1\t.\tACG\tG\t.\t.\tDP=3;MS=3;TYPE=complex"]
    # a leading del_site that is an ins_site: its insertion stands in front of the anchor's byte
    r = V.call(B.stream([rec("x%d" % k, 0, "1S1D1I3M", "GTCGT") for k in range(3)], [("a", 4)]), [("a", b"ACGT\n")])
    assert lines_of(r.text) == [b"a\t1\t.\tAC\tTC\t.\t.\tDP=3;MS=3;TYPE=complex"]
    # .. and where that insertion puts the deleted base back, nothing is written
    r = V.call(B.stream([rec("x%d" % k, 0, "1S1D1I3M", "GACGT") for k in range(3)], [("a", 4)]), [("a", b"ACGT\n")])
    assert r.variants == 0 and r.sites[6] == 1 and r.sites[7] == 1


def test_a_wholly_deleted_record_is_unplaced():
    recs = [rec("x%d" % k, 0, "1S2D", "A") for k in range(3)]
    r = V.call(B.stream(recs, [("a", 2), ("b", 3)]), [("a", b"AC\n"), ("none", b""), ("b", b"ACG")])
    assert (r.unplaced_records, r.unplaced_sites, r.variants) == (1, 2, 0) and r.records == [(2, 0), (0, 0), (3, 0)]
    assert r.text == V.header([("a", 2), ("none", 0), ("b", 3)]) and b"##contig=<ID=none,length=0>\n" in r.text
    assert apply(r.text, [("a", b"AC\n")]) != K.consensus(B.stream(recs, [("a", 2)]), [("a", b"AC\n")], fill="ref").text    # (what unplaced means)


def test_a_group_ends_with_its_genome_record():
    """the first record ends in del_sites, the next begins with them: two groups, and neither crosses"""
    genome, refs = [("p", b"ACGT\n"), ("q", b"TGCA\n")], [("p", 4), ("q", 4)]
    recs = [rec("p%d" % k, 0, "2M2D", "AC") for k in range(3)] + [rec("q%d" % k, 0, "1S2D2M", "ACA", ref=1) for k in range(3)]
    r = V.call(B.stream(recs, refs), genome)
    assert lines_of(r.text) == [b"p\t2\t.\tCGT\tC\t.\t.\tDP=3;MS=3;TYPE=del", b"q\t1\t.\tTGC\tC\t.\t.\tDP=3;MS=3;TYPE=complex"]
    assert r.records == [(4, 1), (4, 1)] and apply(r.text, genome) == K.consensus(B.stream(recs, refs), genome, fill="ref", line_width=0).text


def test_a_sub_site_with_its_insertion_and_a_deletion_behind_is_one_record():
    recs = [rec("x%d" % k, 0, "2M2I1D1M", "ATGGT") for k in range(3)] + [rec("y", 0, "4M", "ACGT")]
    r = V.call(B.stream(recs, [("a", 4)]), [("a", b"ACGT\n")])
    assert lines_of(r.text) == [b"a\t2\t.\tCG\tTGG\t.\t.\tDP=4;MS=3;TYPE=complex"]


# ---------------------------------------------------------------- the header and the report
def test_header_and_report_known_answers():
    assert V.header([("c1", 10), ("c2", 5)]) == WORKED_HEADER
    assert V.header([]).count(b"\n") == 6 and V.header([(b"x y", 0)]).count(b"##contig=<ID=x y,length=0>\n") == 1
    assert V.report(*for_report(ZERO)) == ZERO_REPORT
    assert V.report([1] * 9, [2, 0, 0, 2, 1, 1, 0, 0, 1, ], 7, [1, 2, 3, 1], 10, 11, 4, 5, 1, 6).endswith(b"\nV\t7\t1\t2\t3\t1\t10\t11\t4\t5\t1\t6\n")


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_calls_and_the_library_has_them():
    with open(os.path.join(harness.ROOT, "include", "pbsim3_amd.h")) as f:
        h = f.read()
    assert re.search(r"int pbsim_bam_call\(pbsim_ctx \*ctx, const pbsim_errors_ref \*refs, int n_refs, const pbsim_errors_file \*files, int n_files,\s*"
                     r"const pbsim_call_opts \*opts, const pbsim_call_sink \*sink, pbsim_call_result \*result\);", h)
    assert re.search(r"int64_t pbsim_call_report\(const pbsim_call_result \*result, char \*buf, int64_t cap\);", h)
    assert re.search(r"typedef struct pbsim_call_opts \{[^;]*int32_t exclude_flags, min_mapq, min_baseq;\s*int32_t max_ins;[^;]*\s*int64_t min_depth;\s*"
                     r"int64_t piece_bytes;", h)
    body = re.search(r"typedef struct pbsim_call_result \{(.*?)\} pbsim_call_result;", h, re.S).group(1)
    declared = []
    for names in re.findall(r"int64_t ([^;]+);", body):
        for item in names.split(","):
            name, dims = re.match(r"\s*(\w+)((?:\[\d+\])*)", item).groups()
            declared.append((name, int(dims[1:-1]) if dims else 1))
    mirrored = [(n, C.sizeof(t) // 8) for n, t in P.CallResult._fields_]
    assert declared == mirrored and C.sizeof(P.CallResult) == 8 * sum(n for _, n in declared)
    assert mirrored == [("counts", 9), ("sites", 9), ("ins_unanchored", 1), ("max_depth", 1), ("variants", 1), ("types", 4), ("ref_bases", 1),
                        ("alt_bases", 1), ("longest_ref", 1), ("longest_alt", 1), ("unplaced_records", 1), ("unplaced_sites", 1), ("header_bytes", 1),
                        ("text_bytes", 1)]
    bound = [name for name, _, _ in P.API]
    assert "pbsim_bam_call" in bound and "pbsim_call_report" in bound
    assert [n for n, _ in P.CallOpts._fields_] == ["exclude_flags", "min_mapq", "min_baseq", "max_ins", "min_depth", "piece_bytes"]
    assert C.sizeof(P.CallOpts) == 32 and [n for n, _ in P.CallSink._fields_] == ["user", "on_text", "on_record"]
    assert P.CALL_TYPES == V.TYPE_NAMES
    assert callable(getattr(P.Context, "bam_call")) and callable(P.call_report)
    lib = P.load()
    assert hasattr(lib, "pbsim_bam_call") and hasattr(lib, "pbsim_call_report")


FIELDS = ["counts", "sites", "ins_unanchored", "max_depth", "variants", "types", "ref_bases", "alt_bases", "longest_ref", "longest_alt", "unplaced_records",
          "unplaced_sites", "header_bytes", "text_bytes"]


def as_dict(r):
    return dict(zip(FIELDS, r[:14]))


def for_report(r):
    return (r[0], r[1]) + tuple(r[4:12])


def random_result(rng):
    pick = lambda: rng.choice([0, 0, 1, 10 ** 12, rng.randrange(2 ** 50)])
    sites = [pick() for _ in range(9)]
    sites[3] = sites[8] + pick()                    # called >= discordant, as a result has it: the ppm value stays inside 64 bits
    return [[rng.randrange(2 ** 31) for _ in range(9)], sites, pick(), pick(), pick(), [pick() for _ in range(4)]] + [pick() for _ in range(8)]


ZERO = [[0] * 9, [0] * 9, 0, 0, 0, [0] * 4] + [0] * 8
ZERO_REPORT = (b"# records=0 skipped_flag=0 unaligned=0 skipped_mapq=0 skipped_ref=0 aligned=0 no_seq=0 misfit=0 scored=0\n"
               b"S" + b"\t0" * 10 + b"\t*\nV" + b"\t0" * 11 + b"\n")


def test_report_of_the_library_is_the_models_without_a_device():
    r = worked()
    assert P.call_report(as_dict(r)) == WORKED_REPORT
    by_name = as_dict(r)
    by_name.update(counts=dict(zip(V.COUNT_NAMES, r.counts)), sites=dict(zip(V.SITE_NAMES, r.sites)), types=dict(zip(V.TYPE_NAMES, r.types)))
    assert P.call_report(by_name) == WORKED_REPORT
    assert P.call_report(as_dict(ZERO)) == ZERO_REPORT
    rng = random.Random(45)
    for _ in range(30):
        x = random_result(rng)
        assert P.call_report(as_dict(x)) == V.report(*for_report(x))
    assert P.load().pbsim_call_report(None, None, 0) == -1
    with pytest.raises(ValueError, match="types has 3 values"):
        P.call_report(dict(as_dict(ZERO), types=[0] * 3))


# ---------------------------------------------------------------- the option mirror and the command line
GOOD = ["--call-bam", "in.bam", "--call-genome", "g.fa", "--call-out", "out.vcf"]
REFUSED = [
    (GOOD + ["--depth", "3"], "(--depth): --call-bam takes"),
    (GOOD + ["--consensus-out", "x"], "(--consensus-out): --call-bam takes"),
    (GOOD + ["--call-fill", "ref"], "(--call-fill): --call-bam takes"),
    (GOOD + ["--consensus-bam", "x"], "(--call-bam): --consensus-bam takes"),
    (["--call-out", "o", "--call-bam"], "needs a value"),
    (["--call-bam", "in.bam", "--call-out", "o"], "--call-bam needs --call-genome FASTA"),
    (["--call-bam", "in.bam", "--call-genome", "g.fa"], "--call-bam needs --call-out FILE"),
    (GOOD + ["--call-min-mapq", "256"], "(call-min-mapq: 256): a whole number, 0 .. 255"),
    (GOOD + ["--call-min-baseq", "-1"], "(call-min-baseq: -1): a whole number, 0 .. 255"),
    (GOOD + ["--call-min-depth", "x"], "(call-min-depth: x): a whole number"),
    (GOOD + ["--call-exclude-flags", "65536"], "(call-exclude-flags: 65536): decimal or 0x hexadecimal, 0 .. 65535"),
    (GOOD + ["--call-exclude-flags", "0xg"], "(call-exclude-flags: 0xg): decimal or 0x hexadecimal"),
    (GOOD + ["--call-max-ins", "0"], "(call-max-ins: 0): a whole number, 1 .. 65535"),
    (GOOD + ["--call-max-ins", "65536"], "(call-max-ins: 65536): a whole number, 1 .. 65535"),
    (GOOD + ["--call-ref-names", "a,b"], "(call-ref-names): 2 names for 1 --call-bam files"),
    (GOOD + ["--call-bam", "b.bam", "--call-ref-names", "a,"], "(call-ref-names): an empty name"),
    (GOOD + ["--devices", "0,1"], "--call-bam runs on one GPU"),
    (GOOD + ["--processes", "2"], "--call-bam runs on one GPU"),
]


def test_option_mirror_accepts_and_rejects():
    assert A.call_bam(GOOD) == dict(bams=["in.bam"], genome="g.fa", ref_names=None, out="out.vcf", min_mapq=0, min_baseq=0, min_depth=1,
                                    exclude_flags=0x900, max_ins=1024)
    got = A.call_bam(["--call-out", "o", "--call-bam", "a", "--call-min-mapq", "255", "--call-bam", "b", "--call-min-baseq", "20", "--call-genome", "g",
                      "--call-ref-names", "x,y", "--device", "1", "--call-min-depth", "0", "--call-exclude-flags", "0x10", "--call-max-ins", "65535"])
    assert got == dict(bams=["a", "b"], genome="g", ref_names=["x", "y"], out="o", min_mapq=255, min_baseq=20, min_depth=0, exclude_flags=16,
                       max_ins=65535)
    for argv, message in REFUSED + [(["--call-genome", "g"], "--call-bam FILE: name the BAM file")]:
        if "--consensus-bam" in argv:
            continue                                # (the binary hands that line to the consensus's mode, which refuses it)
        with pytest.raises(ValueError) as e:
            A.call_bam(argv)
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
    (tmp_path / "in.bam").write_bytes(B.bam(WORKED, REFS))
    r = subprocess.run([CLI] + GOOD, capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode != 0 and "--call-genome g.fa: Cannot open file: g.fa" in r.stderr
    assert os.listdir(tmp_path) == ["in.bam"]
    r = subprocess.run([CLI], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert "--call-bam FILE [--call-bam FILE ...] --call-genome FASTA --call-out FILE" in r.stderr + r.stdout


# ---------------------------------------------------------------- the checks in front of any device work
REFUSED_OPTS = [(dict(min_mapq=256), "min_mapq must be 0 .. 255"), (dict(exclude_flags=65536), "exclude_flags must be 0 .. 65535"),
                (dict(min_baseq=256), "min_baseq must be 0 .. 255"), (dict(min_baseq=-1), "min_baseq must be 0 .. 255"),
                (dict(min_depth=-1), "min_depth must not be negative"), (dict(piece_bytes=-1), "piece_bytes must not be negative"),
                (dict(max_ins=0), "max_ins must be 1 .. 65535"), (dict(max_ins=65536), "max_ins must be 1 .. 65535")]


def test_bad_arguments_fail_before_device_work():
    data = B.bam(WORKED, REFS)
    with P.Context(P.default_params(strategy=P.STRATEGY_WGS, method=P.METHOD_ERR), -1) as c:
        for kw, word in REFUSED_OPTS:
            with pytest.raises(P.PbsimError, match="pbsim_bam_call: " + word):
                c.bam_call(data, GENOME, **kw)
        with pytest.raises(P.PbsimError, match="pbsim_bam_call: bad argument"):
            c.bam_call([], GENOME)
        with pytest.raises(P.PbsimError, match="pbsim_bam_call: bad argument"):
            c.bam_call(data, [])
        with pytest.raises(P.PbsimError, match=r"pbsim_bam_call: the genome holds two records named \"c1\" \(records 0 and 2\)"):
            c.bam_call(data, GENOME + [("c1", b"AC")])
        with pytest.raises(ValueError, match="one entry per file"):
            c.bam_call(data, GENOME, ref_names=["a", "b"])
        # good arguments reach the device check: a tables-only context refuses as pbsim_inflate_buffer does, and stays usable
        for kw in (dict(), dict(text=False), dict(min_mapq=255, min_baseq=255, min_depth=0, max_ins=65535, ref_names=["c1", None])):
            with pytest.raises(P.PbsimError, match="no HIP device"):
                c.bam_call([data, data], GENOME, **kw)


# ---------------------------------------------------------------- the host's decisions under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = os.path.join(harness.ROOT, "pbsim3_amd", "csrc")
    exe = str(tmp_path_factory.mktemp("asan") / "bam_call_rule_driver")
    p = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + csrc,
                        os.path.join(harness.ROOT, "tests", "asan", "bam_call_rule_driver.cpp"), os.path.join(csrc, "bam_call_rule.cpp"),
                        os.path.join(csrc, "bam_consensus_rule.cpp"), os.path.join(csrc, "bam_pileup_rule.cpp"), "-o", exe], capture_output=True, text=True)
    if p.returncode != 0 and "sanitize" in p.stderr:
        pytest.skip("no sanitizer runtime")
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def drive(exe, *argv):
    p = subprocess.run([exe] + [str(a) for a in argv], capture_output=True, timeout=60)
    assert p.returncode == 0, (argv, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout


def flat(x):
    return [v for part in x for v in (part if isinstance(part, list) else [part])]


def test_rule_code_under_asan(driver):
    assert drive(driver, "opts", "-") == b"opts 2304 0 0 1024 1 8388608\n"
    assert drive(driver, "opts", 0, 255, 255, 65535, 0, 7) == b"opts 0 255 255 65535 0 7\n"
    assert drive(driver, "opts", 4, 0, 0, 1, 1, 0) == b"opts 4 0 0 1 1 8388608\n"
    for bad, word in (((65536, 0, 0, 1024, 1, 0), b"exclude_flags"), ((-1, 0, 0, 1024, 1, 0), b"exclude_flags"), ((4, 256, 0, 1024, 1, 0), b"min_mapq"),
                      ((4, -1, 0, 1024, 1, 0), b"min_mapq"), ((4, 0, 256, 1024, 1, 0), b"min_baseq"), ((4, 0, -1, 1024, 1, 0), b"min_baseq"),
                      ((4, 0, 0, 0, 1, 0), b"max_ins"), ((4, 0, 0, 65536, 1, 0), b"max_ins"), ((4, 0, 0, -5, 1, 0), b"max_ins"),
                      ((4, 0, 0, 1024, -1, 0), b"min_depth"), ((4, 0, 0, 1024, 1, -1), b"piece_bytes")):
        assert drive(driver, "opts", *bad).startswith(b"opts refused: " + word), bad
    assert drive(driver, "header", "c1", 10, "c2", 5) == WORKED_HEADER
    assert drive(driver, "header") == V.header([]) and drive(driver, "header", "x" * 300, 10 ** 15, "", 0) == V.header([("x" * 300, 10 ** 15), ("", 0)])
    assert drive(driver, "report", *flat(list(worked()[:14]))) == WORKED_REPORT
    assert drive(driver, "report", *flat(ZERO)) == ZERO_REPORT
    rng = random.Random(46)
    for _ in range(5):
        x = random_result(rng)
        assert drive(driver, "report", *flat(x)) == V.report(*for_report(x))
