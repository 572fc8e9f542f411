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


def eval_bam(argv):
    """`pbsim --eval-bam MAPPED.bam --truth-bam FILE [--truth-bam FILE ...] [--truth-ref-names a,b,..] [--eval-overlap 0.1]
    [--eval-out FILE]` -> dict(query, truth=[...], ref_names=None or [...], overlap, out=None or FILE): the stand-alone mode
    that scores a mapper's BAM against truth BAMs (pbsim_truth_bam_eval).  --truth-bam repeats, so argv is walked and not
    zipped into a dict.  What pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    takes = ("--eval-bam", "--truth-bam", "--truth-ref-names", "--eval-overlap", "--eval-out", "--device")
    ranks = ("--devices", "--processes", "--rank", "--world", "--rendezvous", "--comm", "--comm-selftest")
    got = dict(query=None, truth=[], ref_names=None, overlap=0.1, out=None)
    if any(a.split("=")[0] in ranks for a in argv):
        raise ValueError("--eval-bam runs on one GPU (--device N): no --devices / --processes / --rank / --world / --rendezvous / --comm beside it.")
    i = 0
    while i < len(argv):
        a = argv[i]
        if a not in takes:
            raise ValueError("(%s): --eval-bam takes --truth-bam, --truth-ref-names, --eval-overlap, --eval-out and --device, and no other option." % a)
        if i + 1 >= len(argv):
            raise ValueError("(%s): the option needs a value." % a)
        v = argv[i + 1]
        i += 2
        if a == "--eval-bam":
            got["query"] = v
        elif a == "--truth-bam":
            got["truth"].append(v)
        elif a == "--truth-ref-names":
            got["ref_names"] = v.split(",")
        elif a == "--eval-out":
            got["out"] = v
        elif a == "--eval-overlap":
            try:
                got["overlap"] = float(v)
            except ValueError:
                got["overlap"] = -1.0
            if not 0.0 < got["overlap"] <= 1.0:
                raise ValueError("(eval-overlap: %s): the least intersection / union of a correct mapping, in (0, 1]." % v)
    if not got["query"]:
        raise ValueError("--eval-bam MAPPED.bam: name the mapper's BAM file.")
    if not got["truth"]:
        raise ValueError("--eval-bam needs the truth: --truth-bam FILE [--truth-bam FILE ...] (the .aln.bam files of --truth-format bam).")
    if got["ref_names"] is not None:
        if len(got["ref_names"]) != len(got["truth"]):
            raise ValueError("(truth-ref-names): %d names for %d --truth-bam files: the k-th name goes to the k-th file."
                             % (len(got["ref_names"]), len(got["truth"])))
        if "" in got["ref_names"]:
            raise ValueError("(truth-ref-names): an empty name.")
    return got


def _whole(v, base=10):
    """a whole number written with digits only (what the command line takes), or None"""
    body = v[2:] if base == 16 else v
    digits = "0123456789abcdefABCDEF" if base == 16 else "0123456789"
    if not body or any(ch not in digits for ch in body):
        return None
    return int(body, base)


def depth_bam(argv):
    """`pbsim --depth-bam FILE --depth-out FILE [--depth-format bedgraph|window] [--depth-window N] [--depth-min-mapq Q]
    [--depth-exclude-flags F] [--depth-no-deletions]` -> dict(bam, out, format, window, min_mapq, exclude_flags, deletions): the
    stand-alone mode that writes the depth of coverage of a BAM (pbsim_bam_depth).  F is decimal or 0x hexadecimal.  What
    pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    takes = ("--depth-bam", "--depth-out", "--depth-format", "--depth-window", "--depth-min-mapq", "--depth-exclude-flags", "--device")
    ranks = ("--devices", "--processes", "--rank", "--world", "--rendezvous", "--comm", "--comm-selftest")
    got = dict(bam=None, out=None, format="bedgraph", window=0, min_mapq=0, exclude_flags=0x704, deletions=True)
    if any(a.split("=")[0] in ranks for a in argv):
        raise ValueError("--depth-bam runs on one GPU (--device N): no --devices / --processes / --rank / --world / --rendezvous / --comm beside it.")
    have_window = False
    i = 0
    while i < len(argv):
        a = argv[i]
        if a == "--depth-no-deletions":
            got["deletions"] = False
            i += 1
            continue
        if a not in takes:
            raise ValueError("(%s): --depth-bam takes --depth-out, --depth-format, --depth-window, --depth-min-mapq, --depth-exclude-flags, "
                             "--depth-no-deletions and --device, and no other option." % a)
        if i + 1 >= len(argv):
            raise ValueError("(%s): the option needs a value." % a)
        v = argv[i + 1]
        i += 2
        if a == "--depth-bam":
            got["bam"] = v
        elif a == "--depth-out":
            got["out"] = v
        elif a == "--depth-format":
            if v not in ("bedgraph", "window"):
                raise ValueError("(depth-format: %s): bedgraph or window." % v)
            got["format"] = v
        elif a == "--depth-window":
            have_window = True
            n = _whole(v)
            if n is None or not 1 <= n < 2 ** 63:
                raise ValueError("(depth-window: %s): a whole number of at least 1." % v)
            got["window"] = n
        elif a == "--depth-min-mapq":
            n = _whole(v)
            if n is None or n > 255:
                raise ValueError("(depth-min-mapq: %s): a whole number, 0 .. 255." % v)
            got["min_mapq"] = n
        elif a == "--depth-exclude-flags":
            n = _whole(v, 16 if v[:2] in ("0x", "0X") else 10)
            if n is None or n > 65535:
                raise ValueError("(depth-exclude-flags: %s): decimal or 0x hexadecimal, 0 .. 65535." % v)
            got["exclude_flags"] = n
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
    takes = ("--stats-bam", "--stats-out", "--stats-min-mapq", "--stats-exclude-flags", "--device")
    ranks = ("--devices", "--processes", "--rank", "--world", "--rendezvous", "--comm", "--comm-selftest")
    got = dict(bams=[], out=None, min_mapq=0, exclude_flags=0x900)
    if any(a.split("=")[0] in ranks for a in argv):
        raise ValueError("--stats-bam runs on one GPU (--device N): no --devices / --processes / --rank / --world / --rendezvous / --comm beside it.")
    i = 0
    while i < len(argv):
        a = argv[i]
        if a not in takes:
            raise ValueError("(%s): --stats-bam takes --stats-out, --stats-min-mapq, --stats-exclude-flags and --device, and no other option." % a)
        if i + 1 >= len(argv):
            raise ValueError("(%s): the option needs a value." % a)
        v = argv[i + 1]
        i += 2
        if a == "--stats-bam":
            got["bams"].append(v)
        elif a == "--stats-out":
            got["out"] = v
        elif a == "--stats-min-mapq":
            n = _whole(v)
            if n is None or n > 255:
                raise ValueError("(stats-min-mapq: %s): a whole number, 0 .. 255." % v)
            got["min_mapq"] = n
        elif a == "--stats-exclude-flags":
            n = _whole(v, 16 if v[:2] in ("0x", "0X") else 10)
            if n is None or n > 65535:
                raise ValueError("(stats-exclude-flags: %s): decimal or 0x hexadecimal, 0 .. 65535." % v)
            got["exclude_flags"] = n
    if not got["bams"]:
        raise ValueError("--stats-bam FILE: name the BAM file.")
    return got


def errors_bam(argv):
    """`pbsim --errors-bam FILE [--errors-bam FILE ...] --errors-genome FASTA [--errors-ref-names a,b,..] [--errors-out FILE]
    [--errors-min-mapq Q] [--errors-exclude-flags F]` -> dict(bams, genome, ref_names, out, min_mapq, exclude_flags): the stand-alone
    mode that profiles the errors of aligned reads against their genome (pbsim_bam_errors).  F is decimal or 0x hexadecimal.  What
    pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    takes = ("--errors-bam", "--errors-genome", "--errors-ref-names", "--errors-out", "--errors-min-mapq", "--errors-exclude-flags", "--device")
    ranks = ("--devices", "--processes", "--rank", "--world", "--rendezvous", "--comm", "--comm-selftest")
    got = dict(bams=[], genome=None, ref_names=None, out=None, min_mapq=0, exclude_flags=0x900)
    if any(a.split("=")[0] in ranks for a in argv):
        raise ValueError("--errors-bam runs on one GPU (--device N): no --devices / --processes / --rank / --world / --rendezvous / --comm beside it.")
    i = 0
    while i < len(argv):
        a = argv[i]
        if a not in takes:
            raise ValueError("(%s): --errors-bam takes --errors-genome, --errors-ref-names, --errors-out, --errors-min-mapq, --errors-exclude-flags "
                             "and --device, and no other option." % a)
        if i + 1 >= len(argv):
            raise ValueError("(%s): the option needs a value." % a)
        v = argv[i + 1]
        i += 2
        if a == "--errors-bam":
            got["bams"].append(v)
        elif a == "--errors-genome":
            got["genome"] = v
        elif a == "--errors-ref-names":
            got["ref_names"] = v.split(",")
        elif a == "--errors-out":
            got["out"] = v
        elif a == "--errors-min-mapq":
            n = _whole(v)
            if n is None or n > 255:
                raise ValueError("(errors-min-mapq: %s): a whole number, 0 .. 255." % v)
            got["min_mapq"] = n
        elif a == "--errors-exclude-flags":
            n = _whole(v, 16 if v[:2] in ("0x", "0X") else 10)
            if n is None or n > 65535:
                raise ValueError("(errors-exclude-flags: %s): decimal or 0x hexadecimal, 0 .. 65535." % v)
            got["exclude_flags"] = n
    if not got["bams"]:
        raise ValueError("--errors-bam FILE: name the BAM file.")
    if not got["genome"]:
        raise ValueError("--errors-bam needs --errors-genome FASTA: the genome the reads were aligned to.")
    if got["ref_names"] is not None:
        if len(got["ref_names"]) != len(got["bams"]):
            raise ValueError("(errors-ref-names): %d names for %d --errors-bam files: the k-th name goes to the k-th file."
                             % (len(got["ref_names"]), len(got["bams"])))
        if "" in got["ref_names"]:
            raise ValueError("(errors-ref-names): an empty name.")
    return got


def pileup_bam(argv):
    """`pbsim --pileup-bam FILE [--pileup-bam FILE ...] --pileup-genome FASTA [--pileup-ref-names a,b,..] [--pileup-out FILE]
    [--pileup-format sites|all] [--pileup-min-mapq N] [--pileup-min-baseq N] [--pileup-min-depth N]` -> dict(bams, genome, ref_names,
    out, fmt, min_mapq, min_baseq, min_depth): the stand-alone mode that piles the aligned reads up against their genome
    (pbsim_bam_pileup).  What pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    takes = ("--pileup-bam", "--pileup-genome", "--pileup-ref-names", "--pileup-out", "--pileup-format", "--pileup-min-mapq", "--pileup-min-baseq",
             "--pileup-min-depth", "--device")
    ranks = ("--devices", "--processes", "--rank", "--world", "--rendezvous", "--comm", "--comm-selftest")
    got = dict(bams=[], genome=None, ref_names=None, out=None, fmt="sites", min_mapq=0, min_baseq=0, min_depth=1)
    if any(a.split("=")[0] in ranks for a in argv):
        raise ValueError("--pileup-bam runs on one GPU (--device N): no --devices / --processes / --rank / --world / --rendezvous / --comm beside it.")
    i = 0
    while i < len(argv):
        a = argv[i]
        if a not in takes:
            raise ValueError("(%s): --pileup-bam takes --pileup-genome, --pileup-ref-names, --pileup-out, --pileup-format, --pileup-min-mapq, "
                             "--pileup-min-baseq, --pileup-min-depth and --device, and no other option." % a)
        if i + 1 >= len(argv):
            raise ValueError("(%s): the option needs a value." % a)
        v = argv[i + 1]
        i += 2
        if a == "--pileup-bam":
            got["bams"].append(v)
        elif a == "--pileup-genome":
            got["genome"] = v
        elif a == "--pileup-ref-names":
            got["ref_names"] = v.split(",")
        elif a == "--pileup-out":
            got["out"] = v
        elif a == "--pileup-format":
            if v not in ("sites", "all"):
                raise ValueError("(pileup-format: %s): sites or all." % v)
            got["fmt"] = v
        elif a in ("--pileup-min-mapq", "--pileup-min-baseq"):
            n = _whole(v)
            if n is None or n > 255:
                raise ValueError("(%s: %s): a whole number, 0 .. 255." % (a[2:], v))
            got[a[9:].replace("-", "_")] = n
        elif a == "--pileup-min-depth":
            n = _whole(v)
            if n is None or n > 1000000000000:
                raise ValueError("(pileup-min-depth: %s): a whole number, 0 .. 1000000000000." % v)
            got["min_depth"] = n
    if not got["bams"]:
        raise ValueError("--pileup-bam FILE: name the BAM file.")
    if not got["genome"]:
        raise ValueError("--pileup-bam needs --pileup-genome FASTA: the genome the reads were aligned to.")
    if got["ref_names"] is not None:
        if len(got["ref_names"]) != len(got["bams"]):
            raise ValueError("(pileup-ref-names): %d names for %d --pileup-bam files: the k-th name goes to the k-th file."
                             % (len(got["ref_names"]), len(got["bams"])))
        if "" in got["ref_names"]:
            raise ValueError("(pileup-ref-names): an empty name.")
    return got


def consensus_bam(argv):
    """`pbsim --consensus-bam FILE [--consensus-bam FILE ...] --consensus-genome FASTA --consensus-out FILE [--consensus-ref-names a,b,..]
    [--consensus-min-mapq N] [--consensus-min-baseq N] [--consensus-min-depth N] [--consensus-exclude-flags F] [--consensus-fill n|ref]
    [--consensus-max-ins N] [--consensus-line-width N]` -> dict(bams, genome, ref_names, out, min_mapq, min_baseq, min_depth,
    exclude_flags, fill, max_ins, line_width): the stand-alone mode that writes the consensus FASTA of the aligned reads
    (pbsim_bam_consensus).  What pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    takes = ("--consensus-bam", "--consensus-genome", "--consensus-ref-names", "--consensus-out", "--consensus-min-mapq", "--consensus-min-baseq",
             "--consensus-min-depth", "--consensus-exclude-flags", "--consensus-fill", "--consensus-max-ins", "--consensus-line-width", "--device")
    ranks = ("--devices", "--processes", "--rank", "--world", "--rendezvous", "--comm", "--comm-selftest")
    got = dict(bams=[], genome=None, ref_names=None, out=None, min_mapq=0, min_baseq=0, min_depth=1, exclude_flags=0x900, fill="n", max_ins=1024,
               line_width=60)
    if any(a.split("=")[0] in ranks for a in argv):
        raise ValueError("--consensus-bam runs on one GPU (--device N): no --devices / --processes / --rank / --world / --rendezvous / --comm beside it.")
    i = 0
    while i < len(argv):
        a = argv[i]
        if a not in takes:
            raise ValueError("(%s): --consensus-bam takes --consensus-genome, --consensus-out, --consensus-ref-names, --consensus-min-mapq, "
                             "--consensus-min-baseq, --consensus-min-depth, --consensus-exclude-flags, --consensus-fill, --consensus-max-ins, "
                             "--consensus-line-width and --device, and no other option." % a)
        if i + 1 >= len(argv):
            raise ValueError("(%s): the option needs a value." % a)
        v = argv[i + 1]
        i += 2
        if a == "--consensus-bam":
            got["bams"].append(v)
        elif a == "--consensus-genome":
            got["genome"] = v
        elif a == "--consensus-ref-names":
            got["ref_names"] = v.split(",")
        elif a == "--consensus-out":
            got["out"] = v
        elif a == "--consensus-fill":
            if v not in ("n", "ref"):
                raise ValueError("(consensus-fill: %s): n or ref." % v)
            got["fill"] = v
        elif a == "--consensus-exclude-flags":
            n = _whole(v, 16 if v[:2] in ("0x", "0X") else 10)
            if n is None or n > 65535:
                raise ValueError("(consensus-exclude-flags: %s): decimal or 0x hexadecimal, 0 .. 65535." % v)
            got["exclude_flags"] = n
        elif a in ("--consensus-min-mapq", "--consensus-min-baseq"):
            n = _whole(v)
            if n is None or n > 255:
                raise ValueError("(%s: %s): a whole number, 0 .. 255." % (a[2:], v))
            got[a[12:].replace("-", "_")] = n
        elif a == "--consensus-min-depth":
            n = _whole(v)
            if n is None or n > 1000000000000:
                raise ValueError("(consensus-min-depth: %s): a whole number, 0 .. 1000000000000." % v)
            got["min_depth"] = n
        elif a == "--consensus-max-ins":
            n = _whole(v)
            if n is None or not 1 <= n <= 65535:
                raise ValueError("(consensus-max-ins: %s): a whole number, 1 .. 65535." % v)
            got["max_ins"] = n
        elif a == "--consensus-line-width":
            n = _whole(v)
            if n is None or n > 1048576:
                raise ValueError("(consensus-line-width: %s): a whole number, 0 .. 1048576 (0: one line per record)." % v)
            got["line_width"] = n
    if not got["bams"]:
        raise ValueError("--consensus-bam FILE: name the BAM file.")
    if not got["genome"]:
        raise ValueError("--consensus-bam needs --consensus-genome FASTA: the genome the reads were aligned to.")
    if not got["out"]:
        raise ValueError("--consensus-bam needs --consensus-out FILE: where the consensus FASTA goes.")
    if got["ref_names"] is not None:
        if len(got["ref_names"]) != len(got["bams"]):
            raise ValueError("(consensus-ref-names): %d names for %d --consensus-bam files: the k-th name goes to the k-th file."
                             % (len(got["ref_names"]), len(got["bams"])))
        if "" in got["ref_names"]:
            raise ValueError("(consensus-ref-names): an empty name.")
    return got


def call_bam(argv):
    """`pbsim --call-bam FILE [--call-bam FILE ...] --call-genome FASTA --call-out FILE [--call-ref-names a,b,..] [--call-min-mapq N]
    [--call-min-baseq N] [--call-min-depth N] [--call-exclude-flags F] [--call-max-ins N]` -> dict(bams, genome, ref_names, out,
    min_mapq, min_baseq, min_depth, exclude_flags, max_ins): the stand-alone mode that writes the variants the aligned reads support
    as VCF (pbsim_bam_call).  What pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    takes = ("--call-bam", "--call-genome", "--call-ref-names", "--call-out", "--call-min-mapq", "--call-min-baseq", "--call-min-depth",
             "--call-exclude-flags", "--call-max-ins", "--device")
    ranks = ("--devices", "--processes", "--rank", "--world", "--rendezvous", "--comm", "--comm-selftest")
    got = dict(bams=[], genome=None, ref_names=None, out=None, min_mapq=0, min_baseq=0, min_depth=1, exclude_flags=0x900, max_ins=1024)
    if any(a.split("=")[0] in ranks for a in argv):
        raise ValueError("--call-bam runs on one GPU (--device N): no --devices / --processes / --rank / --world / --rendezvous / --comm beside it.")
    i = 0
    while i < len(argv):
        a = argv[i]
        if a not in takes:
            raise ValueError("(%s): --call-bam takes --call-genome, --call-out, --call-ref-names, --call-min-mapq, --call-min-baseq, --call-min-depth, "
                             "--call-exclude-flags, --call-max-ins and --device, and no other option." % a)
        if i + 1 >= len(argv):
            raise ValueError("(%s): the option needs a value." % a)
        v = argv[i + 1]
        i += 2
        if a == "--call-bam":
            got["bams"].append(v)
        elif a == "--call-genome":
            got["genome"] = v
        elif a == "--call-ref-names":
            got["ref_names"] = v.split(",")
        elif a == "--call-out":
            got["out"] = v
        elif a == "--call-exclude-flags":
            n = _whole(v, 16 if v[:2] in ("0x", "0X") else 10)
            if n is None or n > 65535:
                raise ValueError("(call-exclude-flags: %s): decimal or 0x hexadecimal, 0 .. 65535." % v)
            got["exclude_flags"] = n
        elif a in ("--call-min-mapq", "--call-min-baseq"):
            n = _whole(v)
            if n is None or n > 255:
                raise ValueError("(%s: %s): a whole number, 0 .. 255." % (a[2:], v))
            got[a[7:].replace("-", "_")] = n
        elif a == "--call-min-depth":
            n = _whole(v)
            if n is None or n > 1000000000000:
                raise ValueError("(call-min-depth: %s): a whole number, 0 .. 1000000000000." % v)
            got["min_depth"] = n
        elif a == "--call-max-ins":
            n = _whole(v)
            if n is None or not 1 <= n <= 65535:
                raise ValueError("(call-max-ins: %s): a whole number, 1 .. 65535." % v)
            got["max_ins"] = n
    if not got["bams"]:
        raise ValueError("--call-bam FILE: name the BAM file.")
    if not got["genome"]:
        raise ValueError("--call-bam needs --call-genome FASTA: the genome the reads were aligned to.")
    if not got["out"]:
        raise ValueError("--call-bam needs --call-out FILE: where the VCF goes.")
    if got["ref_names"] is not None:
        if len(got["ref_names"]) != len(got["bams"]):
            raise ValueError("(call-ref-names): %d names for %d --call-bam files: the k-th name goes to the k-th file."
                             % (len(got["ref_names"]), len(got["bams"])))
        if "" in got["ref_names"]:
            raise ValueError("(call-ref-names): an empty name.")
    return got


def mutate_genome(argv):
    """`pbsim --mutate-genome FASTA --mutate-out FASTA --mutate-vcf FILE [--mutate-seed N] [--mutate-snv-ppm N] [--mutate-ins-ppm N]
    [--mutate-del-ppm N] [--mutate-ext-ppm N] [--mutate-max-indel N] [--mutate-line-width N]` -> dict(genome, out, vcf, seed, snv_ppm,
    ins_ppm, del_ppm, ext_ppm, max_indel, line_width): the stand-alone mode that draws a variant genome and its truth VCF
    (pbsim_genome_mutate).  What pbsim_cli_main refuses from the command line alone raises ValueError with its message."""
    takes = ("--mutate-genome", "--mutate-out", "--mutate-vcf", "--mutate-seed", "--mutate-snv-ppm", "--mutate-ins-ppm", "--mutate-del-ppm",
             "--mutate-ext-ppm", "--mutate-max-indel", "--mutate-line-width", "--device")
    ranks = ("--devices", "--processes", "--rank", "--world", "--rendezvous", "--comm", "--comm-selftest")
    got = dict(genome=None, out=None, vcf=None, seed=1, snv_ppm=1000, ins_ppm=100, del_ppm=100, ext_ppm=500000, max_indel=50, line_width=60)
    if any(a.split("=")[0] in ranks for a in argv):
        raise ValueError("--mutate-genome runs on one GPU (--device N): no --devices / --processes / --rank / --world / --rendezvous / --comm beside it.")
    i = 0
    while i < len(argv):
        a = argv[i]
        if a not in takes:
            raise ValueError("(%s): --mutate-genome takes --mutate-out, --mutate-vcf, --mutate-seed, --mutate-snv-ppm, --mutate-ins-ppm, "
                             "--mutate-del-ppm, --mutate-ext-ppm, --mutate-max-indel, --mutate-line-width and --device, and no other option." % a)
        if i + 1 >= len(argv):
            raise ValueError("(%s): the option needs a value." % a)
        v = argv[i + 1]
        i += 2
        if a in ("--mutate-genome", "--mutate-out", "--mutate-vcf"):
            got[a[9:]] = v
        elif a == "--mutate-seed":
            n = _whole(v)
            if n is None or n > 4294967295:
                raise ValueError("(mutate-seed: %s): a whole number, 0 .. 4294967295." % v)
            got["seed"] = n
        elif a in ("--mutate-snv-ppm", "--mutate-ins-ppm", "--mutate-del-ppm"):
            n = _whole(v)
            if n is None or n > 1000000:
                raise ValueError("(%s: %s): a whole number, 0 .. 1000000." % (a[2:], v))
            got[a[9:].replace("-", "_")] = n
        elif a == "--mutate-ext-ppm":
            n = _whole(v)
            if n is None or n > 999999:
                raise ValueError("(mutate-ext-ppm: %s): a whole number, 0 .. 999999." % v)
            got["ext_ppm"] = n
        elif a == "--mutate-max-indel":
            n = _whole(v)
            if n is None or not 1 <= n <= 65535:
                raise ValueError("(mutate-max-indel: %s): a whole number, 1 .. 65535." % v)
            got["max_indel"] = n
        elif a == "--mutate-line-width":
            n = _whole(v)
            if n is None or n > 1048576:
                raise ValueError("(mutate-line-width: %s): a whole number, 0 .. 1048576 (0: one line per record)." % v)
            got["line_width"] = n
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
    takes = ("--compare-vcf", "--compare-truth", "--compare-genome", "--compare-out", "--compare-lines", "--compare-min-ms", "--compare-ref-names",
             "--device")
    ranks = ("--devices", "--processes", "--rank", "--world", "--rendezvous", "--comm", "--comm-selftest")
    got = dict(calls=None, truth=None, genome=None, out=None, lines="discordant", min_ms=0, ref_names=None)
    if any(a.split("=")[0] in ranks for a in argv):
        raise ValueError("--compare-vcf runs on one GPU (--device N): no --devices / --processes / --rank / --world / --rendezvous / --comm beside it.")
    i = 0
    while i < len(argv):
        a = argv[i]
        if a not in takes:
            raise ValueError("(%s): --compare-vcf takes --compare-truth, --compare-genome, --compare-out, --compare-lines, --compare-min-ms, "
                             "--compare-ref-names and --device, and no other option." % a)
        if i + 1 >= len(argv):
            raise ValueError("(%s): the option needs a value." % a)
        v = argv[i + 1]
        i += 2
        if a == "--compare-vcf":
            got["calls"] = v
        elif a in ("--compare-truth", "--compare-genome", "--compare-out"):
            got[a[10:]] = v
        elif a == "--compare-ref-names":
            got["ref_names"] = v.split(",")
        elif a == "--compare-lines":
            if v not in ("discordant", "all"):
                raise ValueError("(compare-lines: %s): discordant or all." % v)
            got["lines"] = v
        elif a == "--compare-min-ms":
            n = _whole(v)
            if n is None or n > 2147483647:
                raise ValueError("(compare-min-ms: %s): a whole number, 0 .. 2147483647." % v)
            got["min_ms"] = n
    if not got["calls"]:
        raise ValueError("--compare-vcf CALLS: name the call set.")
    if not got["truth"]:
        raise ValueError("--compare-vcf needs --compare-truth VCF: the truth variants.")
    if not got["genome"]:
        raise ValueError("--compare-vcf needs --compare-genome FASTA: the genome both files speak of.")
    if got["ref_names"] is not None and "" in got["ref_names"]:
        raise ValueError("(compare-ref-names): an empty name.")
    return got


def apply_vcf(argv):
    """`pbsim --apply-vcf VCF --apply-genome FASTA --apply-out FASTA [--apply-ref-names a,b,..] [--apply-haplotype 0|1|2] [--apply-sample
    N|NAME] [--apply-report FILE] [--apply-lines discordant|all] [--apply-line-width N] [--apply-origin FILE]` -> dict(vcf, genome, out,
    ref_names, haplotype, sample, report, lines, line_width, origin): the stand-alone mode that applies the lines of a VCF to a genome
    (pbsim_vcf_apply); sample is a column (int) or a name (str).  What pbsim_cli_main refuses from the command line alone raises
    ValueError with its message."""
    takes = ("--apply-vcf", "--apply-genome", "--apply-out", "--apply-ref-names", "--apply-haplotype", "--apply-sample", "--apply-report",
             "--apply-lines", "--apply-line-width", "--apply-origin", "--device")
    ranks = ("--devices", "--processes", "--rank", "--world", "--rendezvous", "--comm", "--comm-selftest")
    got = dict(vcf=None, genome=None, out=None, ref_names=None, haplotype=0, sample=0, report=None, lines="discordant", line_width=60, origin=None)
    if any(a.split("=")[0] in ranks for a in argv):
        raise ValueError("--apply-vcf runs on one GPU (--device N): no --devices / --processes / --rank / --world / --rendezvous / --comm beside it.")
    i = 0
    while i < len(argv):
        a = argv[i]
        if a not in takes:
            raise ValueError("(%s): --apply-vcf takes --apply-genome, --apply-out, --apply-ref-names, --apply-haplotype, --apply-sample, "
                             "--apply-report, --apply-lines, --apply-line-width, --apply-origin and --device, and no other option." % a)
        if i + 1 >= len(argv):
            raise ValueError("(%s): the option needs a value." % a)
        v = argv[i + 1]
        i += 2
        if a in ("--apply-vcf", "--apply-genome", "--apply-out", "--apply-report", "--apply-origin"):
            got[a[8:]] = v
        elif a == "--apply-ref-names":
            got["ref_names"] = v.split(",")
        elif a == "--apply-haplotype":
            n = _whole(v)
            if n is None or n > 2:
                raise ValueError("(apply-haplotype: %s): 0 (the first ALT of every line), 1 or 2." % v)
            got["haplotype"] = n
        elif a == "--apply-sample":
            if not v:
                raise ValueError("(apply-sample): a 0-based sample column or a sample's name.")
            n = _whole(v)
            got["sample"] = v if n is None or n > 2147483647 else n
        elif a == "--apply-lines":
            if v not in ("discordant", "all"):
                raise ValueError("(apply-lines: %s): discordant or all." % v)
            got["lines"] = v
        elif a == "--apply-line-width":
            n = _whole(v)
            if n is None or n > 1048576:
                raise ValueError("(apply-line-width: %s): a whole number, 0 .. 1048576 (0: one line per record)." % v)
            got["line_width"] = n
    if not got["vcf"]:
        raise ValueError("--apply-vcf VCF: name the variants.")
    if not got["genome"]:
        raise ValueError("--apply-vcf needs --apply-genome FASTA: the genome the file speaks of.")
    if not got["out"]:
        raise ValueError("--apply-vcf needs --apply-out FASTA: where the spliced genome goes.")
    if got["ref_names"] is not None and "" in got["ref_names"]:
        raise ValueError("(apply-ref-names): an empty name.")
    return got
