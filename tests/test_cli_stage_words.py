"""The words of the stand-alone modes of the `pbsim` binary (--eval-bam .. --apply-vcf), pinned: every command line the binary
refuses before a device or a file is touched, with its exit status, its stderr and its stdout as tests/golden/cli_stage_words.json
holds them, and the mirror of those refusals in pbsim3_amd/args.py held to the same words.  The lines are the REFUSED lists of the
ten model tests, and for every mode an unknown option, a last option without its value, a names list of the wrong count and one
with an empty name, and two mode options on one line.  (--compare-ref-names and --apply-ref-names are counted against the genome's
records, which are read on the device's side of the context: their wrong count is not among the lines.)

    PYTHONPATH=.:tests/golden python tests/test_cli_stage_words.py        writes the fixture from the binary and the mirror as they are
"""
import json
import os
import subprocess
import sys

import harness
from pbsim3_amd import args as A

import test_apply_model
import test_call_model
import test_compare_model
import test_consensus_model
import test_depth_model
import test_errors_model
import test_mapeval_model
import test_mutate_model
import test_pileup_model
import test_stats_model

CLI = os.path.join(harness.ROOT, "pbsim3_amd", "bin", "pbsim")
FIXTURE = os.path.join(harness.ROOT, "tests", "golden", "cli_stage_words.json")

# the modes in the order pbsim_cli_main looks for them: (leading option, its mirror, what a complete line needs, its names list)
MODES = [
    ("--eval-bam", A.eval_bam, ["--truth-bam", "t0", "--truth-bam", "t1"], "--truth-ref-names"),
    ("--depth-bam", A.depth_bam, ["--depth-out", "o"], None),
    ("--stats-bam", A.stats_bam, ["--stats-bam", "y"], None),
    ("--errors-bam", A.errors_bam, ["--errors-bam", "y", "--errors-genome", "g"], "--errors-ref-names"),
    ("--pileup-bam", A.pileup_bam, ["--pileup-bam", "y", "--pileup-genome", "g"], "--pileup-ref-names"),
    ("--consensus-bam", A.consensus_bam, ["--consensus-bam", "y", "--consensus-genome", "g", "--consensus-out", "o"], "--consensus-ref-names"),
    ("--call-bam", A.call_bam, ["--call-bam", "y", "--call-genome", "g", "--call-out", "o"], "--call-ref-names"),
    ("--mutate-genome", A.mutate_genome, ["--mutate-out", "o", "--mutate-vcf", "v"], None),
    ("--compare-vcf", A.compare_vcf, ["--compare-truth", "t", "--compare-genome", "g"], "--compare-ref-names"),
    ("--apply-vcf", A.apply_vcf, ["--apply-genome", "g", "--apply-out", "o"], "--apply-ref-names"),
]
COUNTED_ON_THE_HOST = ("--eval-bam", "--errors-bam", "--pileup-bam", "--consensus-bam", "--call-bam")


def command_lines():
    lines = []
    for module in (test_mapeval_model, test_depth_model, test_stats_model, test_errors_model, test_pileup_model, test_consensus_model, test_call_model,
                   test_mutate_model, test_compare_model, test_apply_model):
        lines += [list(argv) for argv, _ in module.REFUSED]
    for lead, _, rest, names in MODES:
        good = [lead, "x"] + rest
        lines += [good + ["--bogus", "1"], good + [rest[-2]], good + ["--device"]]
        if names:
            lines.append(good + [names, "n0,,n2"])
            lines.append(good + [names, "n0,"])
            if lead in COUNTED_ON_THE_HOST:
                lines += [good + [names, "n0"], good + [names, "n0,n1,n2"]]
    lines += [["--apply-vcf", "v", "--eval-bam", "q"], ["--call-bam", "x", "--pileup-bam", "y"], ["--compare-vcf", "c", "--mutate-genome", "g", "--depth-bam", "d"]]
    unique = []
    for argv in lines:
        if argv not in unique:
            unique.append(argv)
    return unique


def binary_says(argv, workdir):
    r = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=str(workdir), timeout=120)
    return dict(status=r.returncode, stderr=r.stderr, stdout=r.stdout)


def mirror_says(argv):
    """the ValueError text of the mode's mirror, None where it takes the line"""
    mirror = next(fn for lead, fn, _, _ in MODES if lead in argv)
    try:
        mirror(argv)
    except ValueError as e:
        return str(e)
    return None


def without_lead(stderr):
    """the binary's one line without its `ERROR` / `ERROR:` and the blank behind it"""
    assert stderr.startswith("ERROR") and stderr.endswith("\n") and stderr.count("\n") == 1, stderr
    return stderr[len("ERROR"):-1].lstrip(":").lstrip(" ")


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_binary_says_what_the_fixture_holds(tmp_path):
    import pbsim3_amd.build as b
    b.build()
    held = fixture()
    assert [line["argv"] for line in held] == command_lines()
    for line in held:
        got = binary_says(line["argv"], tmp_path)
        assert got == {k: line[k] for k in ("status", "stderr", "stdout")}, line["argv"]
        assert got["status"] != 0 and got["stdout"] == ""
    assert os.listdir(tmp_path) == []


def test_the_mirror_says_the_binary_s_words():
    """`mirror` in a line of the fixture: what the mirror said where it differed from the binary when the fixture was recorded"""
    for line in fixture():
        want = line["mirror"] if "mirror" in line else without_lead(line["stderr"])
        assert mirror_says(line["argv"]) == want, line["argv"]


if __name__ == "__main__":
    import tempfile
    import pbsim3_amd.build as b
    b.build()
    out = []
    with tempfile.TemporaryDirectory() as work:
        for argv in command_lines():
            line = dict(argv=argv, **binary_says(argv, work))
            said = mirror_says(argv)
            if said != without_lead(line["stderr"]):
                line["mirror"] = said
                sys.stderr.write("the mirror differs: %r\n  binary: %r\n  mirror: %r\n" % (argv, line["stderr"], said))
            out.append(line)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%d command lines -> %s" % (len(out), FIXTURE))
