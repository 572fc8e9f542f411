"""pbsim command line -> pbsim_params: a TEST-SIDE mirror of the option table (tests/product.py drives the C ABI from a
command line with it).  It maps options to fields and nothing more -- the validation of set_sim_param (pbsim.cpp:1451-1688)
lives in csrc/cli.cpp (pbsim_cli_main), which every front-end of the product goes through (the `pbsim` binary,
pbsim3_amd.run_multi)."""
from . import default_params


def parse(argv):
    """argv: ['--strategy', 'wgs', ...] -> (Params, dict of raw options)."""
    a = dict(zip(argv[::2], argv[1::2]))
    kw = {}
    kw["strategy"] = {"wgs": 1, "trans": 2, "templ": 3}[a["--strategy"][:5] if a["--strategy"].startswith("t") else "wgs"]
    kw["method"] = {"qshmm": 1, "errhmm": 2, "sample": 3}[a["--method"]]
    if "--seed" in a:
        kw["seed"] = int(a["--seed"])
    if "--depth" in a:
        kw["depth"] = float(a["--depth"])
    if "--length-mean" in a:
        kw["len_mean"] = float(a["--length-mean"])
    if "--length-sd" in a:
        kw["len_sd"] = float(a["--length-sd"])
    if "--length-min" in a:
        kw["len_min"] = int(a["--length-min"])
    if "--length-max" in a:
        kw["len_max"] = int(a["--length-max"])
    if "--accuracy-mean" in a:
        kw["accuracy_mean"] = int(float(a["--accuracy-mean"]) * 100) * 0.01  # pbsim.cpp:1660
    if "--pass-num" in a:
        kw["pass_num"] = int(a["--pass-num"])
    if "--hp-del-bias" in a:
        kw["hp_del_bias"] = float(a["--hp-del-bias"])
    if "--difference-ratio" in a:
        s, i, d = (int(x) for x in a["--difference-ratio"].split(":"))
        kw.update(sub_ratio=s, ins_ratio=i, del_ratio=d)
    if "--id-prefix" in a:
        kw["id_prefix"] = a["--id-prefix"]
    return default_params(**kw), a


def read_fasta(path):
    """Records as get_genome_inf/get_genome_seq assemble them (pbsim.cpp:914-965, 1014-1033):
    header = line starting with '>', sequence = the concatenated lines up to the next header."""
    recs, ids, cur = [], [], None
    with open(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\n")
            if line.startswith(b">"):
                cur = []
                recs.append(cur)
                ids.append(line[1:129].decode(errors="replace"))
            elif cur is not None:
                cur.append(line)
    return [b"".join(r) for r in recs], ids


def read_sample_fastq(path, len_min=100, len_max=1000000, acc_min=0.75, acc_max=1.0):
    """The filtered quality strings of get_sample_inf (pbsim.cpp:1216-1283) for a well-formed 4-line FASTQ:
    length within [len_min, len_max], accuracy 1 - mean(10^(-Q/10)) within [acc_min, acc_max], file order."""
    out = []
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    for i in range(3, len(lines), 4):
        q = lines[i]
        if not (len_min <= len(q) <= len_max):
            continue
        prob = 0.0
        for ch in q:                      # same summation order as the reference
            prob += 10 ** ((ch - 33) / -10)
        acc = 1.0 - prob / len(q)
        if acc_min <= acc <= acc_max:
            out.append(q)
    return out


def truth_format(a):
    """--truth-format maf|bam from parse()'s raw options (default maf): what the truth file holds, MAF blocks or aligned BAM
    records (pbsim_set_truth_bam).  argv-style flags without a value (--no-gzip, --samtools) are looked up as keys too.  The
    combinations pbsim_cli_main refuses raise ValueError with its message."""
    fmt = a.get("--truth-format", "maf")
    if fmt not in ("maf", "bam"):
        raise ValueError("--truth-format must be maf or bam")
    if fmt == "bam":
        for flag in ("--no-gzip", "--samtools"):
            if flag in a:
                raise ValueError("--truth-format bam cannot be combined with %s (the .aln.bam file is BGZF made on the GPU)" % flag)
    return fmt


def truth_sort(a):
    """--truth-sort coordinate from parse()'s raw options (default: None, the truth file stays in task order): the finished
    <prefix>[_NNNN].aln.bam files are sorted by coordinate and indexed (pbsim_truth_bam_sort).  Valid only with --truth-format
    bam; what pbsim_cli_main refuses raises ValueError with its message."""
    how = a.get("--truth-sort")
    if how is None:
        return None
    if how != "coordinate":
        raise ValueError("--truth-sort must be coordinate")
    if truth_format(a) != "bam":
        raise ValueError("--truth-sort coordinate sorts the .aln.bam file: it needs --truth-format bam")
    return how


# ---------------------------------------------------------------- the stand-alone modes
# The mirror of csrc/cli_stages.cpp, laid out like it: every mode states its options as a table of rows, one walker goes through
# argv in order, and the checks the modes share are written once.  A row is (option, kind, key of the returned dict, lo, hi, words):
# row 0 is the option that selects the mode, the rows behind it stand in the order of the "takes" sentence, which is made from them;
# --device belongs to every mode and has no row.  words: what a refused value is told behind "(name: value): ".
TEXT, TEXTS, NAMES, WHOLE, FLAGS, CHOICE, SWITCH, HOOK = range(8)
#   TEXT    a value                                   NAMES   a comma-separated list of names
#   TEXTS   a value, and the option repeats           WHOLE   a whole number of lo .. hi
#   FLAGS   the same, decimal or 0x hexadecimal       CHOICE  one of the two words lo and hi
#   SWITCH  no value: the key is set to lo            HOOK    a value the mode reads itself: lo(got, v)
_RANKS = ("--devices", "--processes", "--rank", "--world", "--rendezvous", "--comm", "--comm-selftest")
_MAPQ = "a whole number, 0 .. 255."
_FLAG_WORDS = "decimal or 0x hexadecimal, 0 .. 65535."
_DEPTH_WORDS = "a whole number, 0 .. 1000000000000."
_MAX_INS = "a whole number, 1 .. 65535."
_LINE_WIDTH = "a whole number, 0 .. 1048576 (0: one line per record)."
_PPM = "a whole number, 0 .. 1000000."


def _whole(v, base=10):
    """a whole number written with digits only (what the command line takes), or None"""
    body = v[2:] if base == 16 else v
    digits = "0123456789abcdefABCDEF" if base == 16 else "0123456789"
    if not body or any(ch not in digits for ch in body):
        return None
    return int(body, base)


def _walk(argv, rows, got):
    """argv in order into got: the first unknown option or bad value raises"""
    mode = rows[0][0]
    if any(a.split("=")[0] in _RANKS for a in argv):
        raise ValueError("%s runs on one GPU (--device N): no --devices / --processes / --rank / --world / --rendezvous / --comm beside it." % mode)
    by_name = {row[0]: row for row in rows}
    i = 0
    while i < len(argv):
        a = argv[i]
        if a not in by_name and a != "--device":
            raise ValueError("(%s): %s takes %s and --device, and no other option." % (a, mode, ", ".join(row[0] for row in rows[1:])))
        row = by_name.get(a)            # (None: --device, which is the front's and not the mode's)
        kind, key, lo, hi, words = (row[1:] + (None,) * 3)[:5] if row else (None,) * 5
        if kind == SWITCH:
            got[key] = lo
            i += 1
            continue
        if i + 1 >= len(argv):
            raise ValueError("(%s): the option needs a value." % a)
        v = argv[i + 1]
        i += 2
        refused = "(%s: %s): %s" % (a[2:], v, words)
        if kind == TEXT:
            got[key] = v
        elif kind == TEXTS:
            got[key].append(v)
        elif kind == NAMES:
            got[key] = v.split(",")
        elif kind in (WHOLE, FLAGS):
            n = _whole(v, 16 if kind == FLAGS and v[:2] in ("0x", "0X") else 10)
            if n is None or not lo <= n <= hi:
                raise ValueError(refused)
            got[key] = n
        elif kind == CHOICE:
            if v not in (lo, hi):
                raise ValueError(refused)
            got[key] = v
        elif kind == HOOK:
            lo(got, v)
    return got


def _need_file_names(option, names, file_option, n_files):
    if names is not None and len(names) != n_files:
        raise ValueError("(%s): %d names for %d %s files: the k-th name goes to the k-th file." % (option, len(names), n_files, file_option))


def _refuse_empty_name(option, names):
    if names is not None and "" in names:
        raise ValueError("(%s): an empty name." % option)


def eval_bam(argv):
    """`pbsim --eval-bam MAPPED.bam --truth-bam FILE [--truth-bam FILE ...] [--truth-ref-names a,b,..] [--eval-overlap 0.1]
    [--eval-out FILE]` -> dict(query, truth=[...], ref_names=None or [...], overlap, out=None or FILE): the stand-alone mode
    that scores a mapper's BAM against truth BAMs (pbsim_truth_bam_eval).  --truth-bam repeats, so argv is walked and not
    zipped into a dict.  What pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    def overlap(got, v):
        try:
            got["overlap"] = float(v)
        except ValueError:
            got["overlap"] = -1.0
        if not 0.0 < got["overlap"] <= 1.0:
            raise ValueError("(eval-overlap: %s): the least intersection / union of a correct mapping, in (0, 1]." % v)
    rows = (("--eval-bam", TEXT, "query"),
            ("--truth-bam", TEXTS, "truth"),
            ("--truth-ref-names", NAMES, "ref_names"),
            ("--eval-overlap", HOOK, None, overlap),
            ("--eval-out", TEXT, "out"))
    got = _walk(argv, rows, dict(query=None, truth=[], ref_names=None, overlap=0.1, out=None))
    if not got["query"]:
        raise ValueError("--eval-bam MAPPED.bam: name the mapper's BAM file.")
    if not got["truth"]:
        raise ValueError("--eval-bam needs the truth: --truth-bam FILE [--truth-bam FILE ...] (the .aln.bam files of --truth-format bam).")
    _need_file_names("truth-ref-names", got["ref_names"], "--truth-bam", len(got["truth"]))
    _refuse_empty_name("truth-ref-names", got["ref_names"])
    return got


def depth_bam(argv):
    """`pbsim --depth-bam FILE --depth-out FILE [--depth-format bedgraph|window] [--depth-window N] [--depth-min-mapq Q]
    [--depth-exclude-flags F] [--depth-no-deletions]` -> dict(bam, out, format, window, min_mapq, exclude_flags, deletions): the
    stand-alone mode that writes the depth of coverage of a BAM (pbsim_bam_depth).  F is decimal or 0x hexadecimal.  What
    pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    rows = (("--depth-bam", TEXT, "bam"),
            ("--depth-out", TEXT, "out"),
            ("--depth-format", CHOICE, "format", "bedgraph", "window", "bedgraph or window."),
            ("--depth-window", WHOLE, "window", 1, 2 ** 63 - 1, "a whole number of at least 1."),
            ("--depth-min-mapq", WHOLE, "min_mapq", 0, 255, _MAPQ),
            ("--depth-exclude-flags", FLAGS, "exclude_flags", 0, 65535, _FLAG_WORDS),
            ("--depth-no-deletions", SWITCH, "deletions", False))
    got = _walk(argv, rows, dict(bam=None, out=None, format="bedgraph", window=0, min_mapq=0, exclude_flags=0x704, deletions=True))
    have_window = got["window"] != 0            # (a window that was given is 1 or more)
    if not got["bam"]:
        raise ValueError("--depth-bam FILE: name the BAM file.")
    if not got["out"]:
        raise ValueError("--depth-bam needs --depth-out FILE: the bedGraph or window text goes there (the report goes to the standard output).")
    if got["format"] == "window" and not have_window:
        raise ValueError("--depth-format window needs --depth-window N.")
    if got["format"] != "window" and have_window:
        raise ValueError("--depth-window N goes with --depth-format window.")
    return got


def stats_bam(argv):
    """`pbsim --stats-bam FILE [--stats-bam FILE ...] [--stats-out FILE] [--stats-min-mapq Q] [--stats-exclude-flags F]` ->
    dict(bams, out, min_mapq, exclude_flags): the stand-alone mode that summarises the reads of BAM files (pbsim_bam_stats).  F
    is decimal or 0x hexadecimal.  What pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    rows = (("--stats-bam", TEXTS, "bams"),
            ("--stats-out", TEXT, "out"),
            ("--stats-min-mapq", WHOLE, "min_mapq", 0, 255, _MAPQ),
            ("--stats-exclude-flags", FLAGS, "exclude_flags", 0, 65535, _FLAG_WORDS))
    got = _walk(argv, rows, dict(bams=[], out=None, min_mapq=0, exclude_flags=0x900))
    if not got["bams"]:
        raise ValueError("--stats-bam FILE: name the BAM file.")
    return got


def _pile_checks(mode, got, needs_out=None):
    """what the four modes that read aligned BAM files against their genome need and check alike; needs_out: what the mode says
    when it must have --<mode>-out and has none"""
    if not got["bams"]:
        raise ValueError("--%s-bam FILE: name the BAM file." % mode)
    if not got["genome"]:
        raise ValueError("--%s-bam needs --%s-genome FASTA: the genome the reads were aligned to." % (mode, mode))
    if needs_out and not got["out"]:
        raise ValueError(needs_out)
    _need_file_names(mode + "-ref-names", got["ref_names"], "--%s-bam" % mode, len(got["bams"]))
    _refuse_empty_name(mode + "-ref-names", got["ref_names"])
    return got


def errors_bam(argv):
    """`pbsim --errors-bam FILE [--errors-bam FILE ...] --errors-genome FASTA [--errors-ref-names a,b,..] [--errors-out FILE]
    [--errors-min-mapq Q] [--errors-exclude-flags F]` -> dict(bams, genome, ref_names, out, min_mapq, exclude_flags): the stand-alone
    mode that profiles the errors of aligned reads against their genome (pbsim_bam_errors).  F is decimal or 0x hexadecimal.  What
    pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    rows = (("--errors-bam", TEXTS, "bams"),
            ("--errors-genome", TEXT, "genome"),
            ("--errors-ref-names", NAMES, "ref_names"),
            ("--errors-out", TEXT, "out"),
            ("--errors-min-mapq", WHOLE, "min_mapq", 0, 255, _MAPQ),
            ("--errors-exclude-flags", FLAGS, "exclude_flags", 0, 65535, _FLAG_WORDS))
    return _pile_checks("errors", _walk(argv, rows, dict(bams=[], genome=None, ref_names=None, out=None, min_mapq=0, exclude_flags=0x900)))


def pileup_bam(argv):
    """`pbsim --pileup-bam FILE [--pileup-bam FILE ...] --pileup-genome FASTA [--pileup-ref-names a,b,..] [--pileup-out FILE]
    [--pileup-format sites|all] [--pileup-min-mapq N] [--pileup-min-baseq N] [--pileup-min-depth N]` -> dict(bams, genome, ref_names,
    out, fmt, min_mapq, min_baseq, min_depth): the stand-alone mode that piles the aligned reads up against their genome
    (pbsim_bam_pileup).  What pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    rows = (("--pileup-bam", TEXTS, "bams"),
            ("--pileup-genome", TEXT, "genome"),
            ("--pileup-ref-names", NAMES, "ref_names"),
            ("--pileup-out", TEXT, "out"),
            ("--pileup-format", CHOICE, "fmt", "sites", "all", "sites or all."),
            ("--pileup-min-mapq", WHOLE, "min_mapq", 0, 255, _MAPQ),
            ("--pileup-min-baseq", WHOLE, "min_baseq", 0, 255, _MAPQ),
            ("--pileup-min-depth", WHOLE, "min_depth", 0, 1000000000000, _DEPTH_WORDS))
    return _pile_checks("pileup", _walk(argv, rows, dict(bams=[], genome=None, ref_names=None, out=None, fmt="sites", min_mapq=0, min_baseq=0, min_depth=1)))


def consensus_bam(argv):
    """`pbsim --consensus-bam FILE [--consensus-bam FILE ...] --consensus-genome FASTA --consensus-out FILE [--consensus-ref-names a,b,..]
    [--consensus-min-mapq N] [--consensus-min-baseq N] [--consensus-min-depth N] [--consensus-exclude-flags F] [--consensus-fill n|ref]
    [--consensus-max-ins N] [--consensus-line-width N]` -> dict(bams, genome, ref_names, out, min_mapq, min_baseq, min_depth,
    exclude_flags, fill, max_ins, line_width): the stand-alone mode that writes the consensus FASTA of the aligned reads
    (pbsim_bam_consensus).  What pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    rows = (("--consensus-bam", TEXTS, "bams"),
            ("--consensus-genome", TEXT, "genome"),
            ("--consensus-out", TEXT, "out"),
            ("--consensus-ref-names", NAMES, "ref_names"),
            ("--consensus-min-mapq", WHOLE, "min_mapq", 0, 255, _MAPQ),
            ("--consensus-min-baseq", WHOLE, "min_baseq", 0, 255, _MAPQ),
            ("--consensus-min-depth", WHOLE, "min_depth", 0, 1000000000000, _DEPTH_WORDS),
            ("--consensus-exclude-flags", FLAGS, "exclude_flags", 0, 65535, _FLAG_WORDS),
            ("--consensus-fill", CHOICE, "fill", "n", "ref", "n or ref."),
            ("--consensus-max-ins", WHOLE, "max_ins", 1, 65535, _MAX_INS),
            ("--consensus-line-width", WHOLE, "line_width", 0, 1048576, _LINE_WIDTH))
    got = _walk(argv, rows, dict(bams=[], genome=None, ref_names=None, out=None, min_mapq=0, min_baseq=0, min_depth=1, exclude_flags=0x900, fill="n",
                                 max_ins=1024, line_width=60))
    return _pile_checks("consensus", got, "--consensus-bam needs --consensus-out FILE: where the consensus FASTA goes.")


def call_bam(argv):
    """`pbsim --call-bam FILE [--call-bam FILE ...] --call-genome FASTA --call-out FILE [--call-ref-names a,b,..] [--call-min-mapq N]
    [--call-min-baseq N] [--call-min-depth N] [--call-exclude-flags F] [--call-max-ins N]` -> dict(bams, genome, ref_names, out,
    min_mapq, min_baseq, min_depth, exclude_flags, max_ins): the stand-alone mode that writes the variants the aligned reads support
    as VCF (pbsim_bam_call).  What pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    rows = (("--call-bam", TEXTS, "bams"),
            ("--call-genome", TEXT, "genome"),
            ("--call-out", TEXT, "out"),
            ("--call-ref-names", NAMES, "ref_names"),
            ("--call-min-mapq", WHOLE, "min_mapq", 0, 255, _MAPQ),
            ("--call-min-baseq", WHOLE, "min_baseq", 0, 255, _MAPQ),
            ("--call-min-depth", WHOLE, "min_depth", 0, 1000000000000, _DEPTH_WORDS),
            ("--call-exclude-flags", FLAGS, "exclude_flags", 0, 65535, _FLAG_WORDS),
            ("--call-max-ins", WHOLE, "max_ins", 1, 65535, _MAX_INS))
    got = _walk(argv, rows, dict(bams=[], genome=None, ref_names=None, out=None, min_mapq=0, min_baseq=0, min_depth=1, exclude_flags=0x900, max_ins=1024))
    return _pile_checks("call", got, "--call-bam needs --call-out FILE: where the VCF goes.")


def mutate_genome(argv):
    """`pbsim --mutate-genome FASTA --mutate-out FASTA --mutate-vcf FILE [--mutate-seed N] [--mutate-snv-ppm N] [--mutate-ins-ppm N]
    [--mutate-del-ppm N] [--mutate-ext-ppm N] [--mutate-max-indel N] [--mutate-line-width N]` -> dict(genome, out, vcf, seed, snv_ppm,
    ins_ppm, del_ppm, ext_ppm, max_indel, line_width): the stand-alone mode that draws a variant genome and its truth VCF
    (pbsim_genome_mutate).  What pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    rows = (("--mutate-genome", TEXT, "genome"),
            ("--mutate-out", TEXT, "out"),
            ("--mutate-vcf", TEXT, "vcf"),
            ("--mutate-seed", WHOLE, "seed", 0, 4294967295, "a whole number, 0 .. 4294967295."),
            ("--mutate-snv-ppm", WHOLE, "snv_ppm", 0, 1000000, _PPM),
            ("--mutate-ins-ppm", WHOLE, "ins_ppm", 0, 1000000, _PPM),
            ("--mutate-del-ppm", WHOLE, "del_ppm", 0, 1000000, _PPM),
            ("--mutate-ext-ppm", WHOLE, "ext_ppm", 0, 999999, "a whole number, 0 .. 999999."),
            ("--mutate-max-indel", WHOLE, "max_indel", 1, 65535, _MAX_INS),
            ("--mutate-line-width", WHOLE, "line_width", 0, 1048576, _LINE_WIDTH))
    got = _walk(argv, rows, dict(genome=None, out=None, vcf=None, seed=1, snv_ppm=1000, ins_ppm=100, del_ppm=100, ext_ppm=500000, max_indel=50, line_width=60))
    if not got["genome"]:
        raise ValueError("--mutate-genome FASTA: name the genome.")
    if not got["out"]:
        raise ValueError("--mutate-genome needs --mutate-out FASTA: where the variant genome goes.")
    if not got["vcf"]:
        raise ValueError("--mutate-genome needs --mutate-vcf FILE: where the truth variants go.")
    if got["snv_ppm"] + got["ins_ppm"] + got["del_ppm"] > 1000000:
        raise ValueError("(mutate-snv-ppm + mutate-ins-ppm + mutate-del-ppm): the three rates sum to more than 1000000.")
    return got


def compare_vcf(argv):
    """`pbsim --compare-vcf CALLS --compare-truth TRUTH --compare-genome FASTA [--compare-out FILE] [--compare-lines discordant|all]
    [--compare-min-ms N] [--compare-ref-names a,b,..]` -> dict(calls, truth, genome, out, lines, min_ms, ref_names): the stand-alone
    mode that scores a call set against the truth variants (pbsim_vcf_compare).  What pbsim_cli_main refuses from the command line
    alone raises ValueError with its message."""
    rows = (("--compare-vcf", TEXT, "calls"),
            ("--compare-truth", TEXT, "truth"),
            ("--compare-genome", TEXT, "genome"),
            ("--compare-out", TEXT, "out"),
            ("--compare-lines", CHOICE, "lines", "discordant", "all", "discordant or all."),
            ("--compare-min-ms", WHOLE, "min_ms", 0, 2147483647, "a whole number, 0 .. 2147483647."),
            ("--compare-ref-names", NAMES, "ref_names"))
    got = _walk(argv, rows, dict(calls=None, truth=None, genome=None, out=None, lines="discordant", min_ms=0, ref_names=None))
    if not got["calls"]:
        raise ValueError("--compare-vcf CALLS: name the call set.")
    if not got["truth"]:
        raise ValueError("--compare-vcf needs --compare-truth VCF: the truth variants.")
    if not got["genome"]:
        raise ValueError("--compare-vcf needs --compare-genome FASTA: the genome both files speak of.")
    _refuse_empty_name("compare-ref-names", got["ref_names"])
    return got


def apply_vcf(argv):
    """`pbsim --apply-vcf VCF --apply-genome FASTA --apply-out FASTA [--apply-ref-names a,b,..] [--apply-haplotype 0|1|2] [--apply-sample
    N|NAME] [--apply-report FILE] [--apply-lines discordant|all] [--apply-line-width N] [--apply-origin FILE]` -> dict(vcf, genome, out,
    ref_names, haplotype, sample, report, lines, line_width, origin): the stand-alone mode that applies the lines of a VCF to a genome
    (pbsim_vcf_apply); sample is a column (int) or a name (str).  What pbsim_cli_main refuses from the command line alone raises
    ValueError with its message."""
    def sample(got, v):
        if not v:
            raise ValueError("(apply-sample): a 0-based sample column or a sample's name.")
        n = _whole(v)
        got["sample"] = v if n is None or n > 2147483647 else n
    rows = (("--apply-vcf", TEXT, "vcf"),
            ("--apply-genome", TEXT, "genome"),
            ("--apply-out", TEXT, "out"),
            ("--apply-ref-names", NAMES, "ref_names"),
            ("--apply-haplotype", WHOLE, "haplotype", 0, 2, "0 (the first ALT of every line), 1 or 2."),
            ("--apply-sample", HOOK, None, sample),
            ("--apply-report", TEXT, "report"),
            ("--apply-lines", CHOICE, "lines", "discordant", "all", "discordant or all."),
            ("--apply-line-width", WHOLE, "line_width", 0, 1048576, _LINE_WIDTH),
            ("--apply-origin", TEXT, "origin"))
    got = _walk(argv, rows, dict(vcf=None, genome=None, out=None, ref_names=None, haplotype=0, sample=0, report=None, lines="discordant", line_width=60,
                                 origin=None))
    if not got["vcf"]:
        raise ValueError("--apply-vcf VCF: name the variants.")
    if not got["genome"]:
        raise ValueError("--apply-vcf needs --apply-genome FASTA: the genome the file speaks of.")
    if not got["out"]:
        raise ValueError("--apply-vcf needs --apply-out FASTA: where the spliced genome goes.")
    _refuse_empty_name("apply-ref-names", got["ref_names"])
    return got


def lift_bam(argv):
    """`pbsim --lift-bam IN --lift-out OUT --lift-genome FASTA --lift-vcf VCF [--lift-haplotype 0|1|2] [--lift-sample N|NAME]
    [--lift-ref-names a,b,..] [--lift-ref-name NAME]` -> dict(bam, out, genome, vcf, haplotype, sample, ref_names, ref_name): the
    stand-alone mode that places a truth BAM of a variant genome on the original one (pbsim_vcf_apply for the origin maps, then
    pbsim_bam_lift); sample is a column (int) or a name (str).  What pbsim_cli_main refuses from the command line alone raises
    ValueError with its message."""
    def sample(got, v):
        if not v:
            raise ValueError("(lift-sample): a 0-based sample column or a sample's name.")
        n = _whole(v)
        got["sample"] = v if n is None or n > 2147483647 else n
    rows = (("--lift-bam", TEXT, "bam"),
            ("--lift-out", TEXT, "out"),
            ("--lift-genome", TEXT, "genome"),
            ("--lift-vcf", TEXT, "vcf"),
            ("--lift-haplotype", WHOLE, "haplotype", 0, 2, "0 (the first ALT of every line), 1 or 2."),
            ("--lift-sample", HOOK, None, sample),
            ("--lift-ref-names", NAMES, "ref_names"),
            ("--lift-ref-name", TEXT, "ref_name"))
    got = _walk(argv, rows, dict(bam=None, out=None, genome=None, vcf=None, haplotype=0, sample=0, ref_names=None, ref_name=None))
    if not got["bam"]:
        raise ValueError("--lift-bam IN: name the BAM file whose records lie on the variant genome.")
    if not got["out"]:
        raise ValueError("--lift-bam needs --lift-out FILE: where the lifted BAM goes.")
    if not got["genome"]:
        raise ValueError("--lift-bam needs --lift-genome FASTA: the original genome.")
    if not got["vcf"]:
        raise ValueError("--lift-bam needs --lift-vcf VCF: the variants the variant genome was made with (--mutate-vcf's file, or the file given to --apply-vcf).")
    _refuse_empty_name("lift-ref-names", got["ref_names"])
    return got
