// cli_stages.cpp -- the stand-alone modes of the `pbsim` binary: no simulation, one stage of the C ABI of include/pbsim3_amd.h on
// one GPU (--eval-bam, --depth-bam, --stats-bam, --errors-bam, --pileup-bam, --consensus-bam, --call-bam, --mutate-genome,
// --compare-vcf, --apply-vcf, --lift-bam; cli_stages.h names them).  Every mode has the same frame, and each step of it is written once here:
// the options as a table of rows that one parser walks, the names list, the input files, the genome, the VCF bytes, the one-GPU
// context, the output files with their ending, the report.  A mode's main is then its table, its "needs" refusals, its options
// struct, its call and its report.  What can be refused from the command line alone is refused before a GPU is touched;
// pbsim3_amd/args.py mirrors those refusals, table by table.
#include <ctype.h>
#include <errno.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdlib.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "cli_common.h"
#include "cli_stages.h"
#include "input_file.h"
#include "unit_io.h"

namespace pbsim {
namespace cli {
namespace {

// ---------------------------------------------------------------- the option table and its parser
enum Kind {
  kText,    // a value: std::string
  kTexts,   // a value, and the option repeats: std::vector<std::string>
  kNames,   // a comma-separated list of names: std::vector<std::string> (never empty once the option was given)
  kWhole,   // a whole number of lo .. hi: long long
  kFlags,   // the same, decimal or 0x hexadecimal: long long
  kChoice,  // one of two words: long long, 0 for `zero` and 1 for `one`
  kSwitch,  // no value: bool, set
  kHook     // a value the mode reads itself
};

// One option of a mode.  Row 0 of a mode's table is the option that selects it; the rows behind it stand in the order of the
// "takes" sentence, which is made from them.  --device belongs to every mode and has no row.
struct Opt {
  const char *name;
  Kind kind;
  size_t at;               // where the value goes in the mode's arguments
  long long lo, hi;        // kWhole, kFlags
  const char *words;       // what a refused value is told behind "(name: value): "
  const char *zero, *one;  // kChoice
  void (*hook)(const char *v, void *args);
};

bool whole_number(const char *v, int base, long long lo, long long hi, long long *out) {
  char *e = NULL;
  errno = 0;
  const long long x = strtoll(v, &e, base);
  if (e == v || *e || errno || x < lo || x > hi || !(isdigit((unsigned char)v[0]))) return false;
  *out = x;
  return true;
}

std::vector<std::string> split_names(const std::string &list) {
  std::vector<std::string> names;
  for (size_t at = 0;;) {
    const size_t comma = list.find(',', at);
    names.push_back(list.substr(at, comma == std::string::npos ? std::string::npos : comma - at));
    if (comma == std::string::npos) return names;
    at = comma + 1;
  }
}

// argv in order: the first unknown option or bad value ends the run
void parse_stage(int argc, char **argv, const pbsim_comm *comm, const Opt *opts, size_t n_opts, void *args, int *device) {
  const char *mode = opts[0].name;
  if (comm && comm->world > 1) die(": %s runs on one GPU.", mode);
  for (int i = 1; i < argc; i++) {
    const Opt *o = nullptr;
    for (size_t k = 0; k < n_opts && !o; k++)
      if (!strcmp(argv[i], opts[k].name)) o = &opts[k];
    const bool is_device = !o && !strcmp(argv[i], "--device");
    if (!o && !is_device) {
      std::string takes = std::string(mode) + " takes ";
      for (size_t k = 1; k < n_opts; k++) takes += std::string(k > 1 ? ", " : "") + opts[k].name;
      die(" (%s): %s and --device, and no other option.", argv[i], takes.c_str());
    }
    char *to = (char *)args + (o ? o->at : 0);
    if (o && o->kind == kSwitch) {
      *(bool *)to = true;
      continue;
    }
    if (i + 1 >= argc) die(" (%s): the option needs a value.", argv[i]);
    const char *v = argv[++i];
    if (is_device) {
      *device = *device >= 0 ? *device : atoi(v);
      continue;
    }
    const std::string refused = std::string(" (%s: %s): ") + (o->words ? o->words : "");
    const bool hex = o->kind == kFlags && v[0] == '0' && (v[1] == 'x' || v[1] == 'X');
    switch (o->kind) {
      case kText: *(std::string *)to = v; break;
      case kTexts: ((std::vector<std::string> *)to)->push_back(v); break;
      case kNames: *(std::vector<std::string> *)to = split_names(v); break;
      case kWhole:
      case kFlags:
        if (!whole_number(v, hex ? 16 : 10, o->lo, o->hi, (long long *)to)) die(refused.c_str(), o->name + 2, v);
        break;
      case kChoice:
        if (strcmp(v, o->zero) && strcmp(v, o->one)) die(refused.c_str(), o->name + 2, v);
        *(long long *)to = !strcmp(v, o->one);
        break;
      case kHook: o->hook(v, args); break;
      case kSwitch: break;
    }
  }
}
#define PARSE_STAGE(opts, args) parse_stage(argc, argv, comm, opts, sizeof(opts) / sizeof(opts[0]), &(args), &device)

// ---------------------------------------------------------------- the names list
// `option` without its dashes, as the refusals name it
void need_name_count(const char *option, size_t names, size_t want, const char *of_what, const char *each) {
  if (names == want) return;
  const std::string what = std::to_string(names) + " names for " + std::to_string(want) + " " + of_what + ": the k-th name goes to the k-th " + each + ".";
  die(" (%s): %s", option, what.c_str());
}
void need_file_names(const char *option, const std::vector<std::string> &names, const char *file_option, size_t n_files) {
  if (!names.empty()) need_name_count(option, names.size(), n_files, (std::string(file_option) + " files").c_str(), "file");
}
void need_record_names(const char *option, const std::vector<std::string> &names, size_t n_records) {
  if (!names.empty()) need_name_count(option, names.size(), n_records, "genome records", "record");
}
// with_list: the refusal shows the list as it was given (--truth-ref-names alone does)
void refuse_empty_name(const char *option, const std::vector<std::string> &names, bool with_list = false) {
  std::string list;
  for (size_t k = 0; k < names.size(); k++) list += (k ? "," : "") + names[k];
  for (const std::string &n : names) {
    if (!n.empty()) continue;
    if (with_list) die(" (%s: %s): an empty name.", option, list.c_str());
    die(" (%s): an empty name.", option);
  }
}
const char *name_or_null(const std::vector<std::string> &names, size_t k) { return names.empty() ? NULL : names[k].c_str(); }

// ---------------------------------------------------------------- the inputs
void open_inputs(const std::vector<std::string> &names, std::vector<MappedFile> *files) {
  *files = std::vector<MappedFile>(names.size());
  for (size_t f = 0; f < names.size(); f++)
    if (!(*files)[f].open_file(names[f])) die(": Cannot open file: %s", names[f].c_str());
}
void need_readable(std::initializer_list<const std::string *> names) {
  for (const std::string *name : names)
    if (access(name->c_str(), R_OK) != 0) die(": Cannot open file: %s", name->c_str());
}
std::vector<pbsim_errors_file> errors_files(const std::vector<MappedFile> &files, const std::vector<std::string> &names) {
  std::vector<pbsim_errors_file> in(files.size());
  for (size_t f = 0; f < files.size(); f++) in[f] = pbsim_errors_file{files[f].map, (int64_t)files[f].n, name_or_null(names, f)};
  return in;
}

// The genome: each record's sequence lines as they lie in the file, its name the id up to the first white space.  A BGZF file
// is inflated on a device: a mode that takes one makes its context first and hands it in (`inflate_on`), the others map the
// genome before a GPU is touched.
struct GenomeRefs {
  FastaMap fm;
  std::vector<std::string> names;
  std::vector<pbsim_errors_ref> refs;
};
void map_genome_refs(const char *option, const std::string &file, pbsim_ctx *inflate_on, GenomeRefs *g) {
  GenomeInfo gm;
  bool fallback = false;
  std::string err;
  pbsim_ctx *before = inflate_on ? set_input_context(inflate_on) : nullptr;
  const bool mapped = map_genome(file.c_str(), &g->fm, &gm, false, &fallback, &err);
  if (inflate_on) set_input_context(before);
  if (!mapped) {
    if (fallback) err = "not a FASTA file that can be mapped (a regular file that begins with '>' and holds no NUL byte)";
    die((std::string(": ") + option + " %s: %s").c_str(), file.c_str(), err.c_str());
  }
  for (const FastaRecord &r : g->fm.recs) g->names.push_back(r.id.substr(0, r.id.find_first_of(" \t\r\n\v\f")));
  for (size_t r = 0; r < g->fm.recs.size(); r++) g->refs.push_back(pbsim_errors_ref{g->names[r].c_str(), g->fm.recs[r].lines, g->fm.recs[r].bytes});
}

// a VCF: the inflated bytes of a gzip file (on the context's device), else the file as it is (an empty one has no lines)
struct VcfBytes {
  InputBytes gz;
  MappedFile plain;
  const void *bytes = NULL;
  int64_t n = 0;
};
void load_vcf(const std::string &name, pbsim_ctx *inflate_on, VcfBytes *v) {
  std::string err;
  pbsim_ctx *before = set_input_context(inflate_on);
  const int g = open_input(name.c_str(), &v->gz, &err);
  set_input_context(before);
  if (g < 0) die(": %s", err.c_str());
  struct stat sb;
  if (g > 0) {
    v->bytes = v->gz.map, v->n = (int64_t)v->gz.size;
  } else if (!(stat(name.c_str(), &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size == 0)) {
    if (!v->plain.open_file(name)) die(": Cannot open file: %s", name.c_str());
    v->bytes = v->plain.map, v->n = (int64_t)v->plain.n;
  }
}

pbsim_ctx *one_gpu_context(int device) {
  pbsim_params p;
  pbsim_params_default(&p);
  p.strategy = PBSIM_STRATEGY_WGS;
  p.method = PBSIM_METHOD_ERR;
  pbsim_ctx *ctx = pbsim_create(&p, device >= 0 ? device : 0);
  if (!ctx) check(0);
  return ctx;
}

// ---------------------------------------------------------------- the outputs
// A mode's output files, one to three in an array: the sink's user pointer is the array, text_to_0 and text_to_1 its callbacks.
// A file without a name is not wanted: it stays closed, and the mode gives the stage no callback for it.
struct OutFile {
  std::string name;
  FILE *fp = NULL;
  bool write_failed = false;
};
int put(OutFile *x, const void *z, size_t bytes) {
  if (fwrite(z, 1, bytes, x->fp) != bytes) x->write_failed = true;
  return x->write_failed ? 0 : 1;
}
int text_to_0(void *u, const char *z, int64_t k, int64_t) { return put((OutFile *)u, z, (size_t)k); }
int text_to_1(void *u, const char *z, int64_t k, int64_t) { return put((OutFile *)u + 1, z, (size_t)k); }

void open_outputs(OutFile *outs, int n) {
  for (int k = 0; k < n; k++) {
    if (outs[k].name.empty()) continue;
    outs[k].fp = fopen(outs[k].name.c_str(), "wb");
    if (outs[k].fp) continue;
    for (int j = 0; j < k; j++)
      if (outs[j].fp) fclose(outs[j].fp), unlink(outs[j].name.c_str());
    die(": Cannot open output file: %s", outs[k].name.c_str());
  }
}
// The files closed; where the stage failed or a write did, the reason (the first output that failed to be written, else the
// stage's), the input files named where there are several, every output removed, and the reference's exit(-1).
void finish_outputs(OutFile *outs, int n, bool ok, const std::vector<std::string> *inputs = nullptr) {
  const OutFile *failed = NULL;
  for (int k = 0; k < n; k++) {
    if (outs[k].fp && fclose(outs[k].fp) != 0) outs[k].write_failed = true;
    if (outs[k].write_failed && !failed) failed = &outs[k];
  }
  if (ok && !failed) return;
  fprintf(stderr, "ERROR: %s\n", failed ? ("write error on " + failed->name).c_str() : pbsim_last_error());
  if (inputs && inputs->size() > 1)
    for (size_t f = 0; f < inputs->size(); f++) fprintf(stderr, "ERROR: file %zu is %s\n", f, (*inputs)[f].c_str());
  for (int k = 0; k < n; k++)
    if (!outs[k].name.empty()) unlink(outs[k].name.c_str());
  quit(-1);
}

// ---------------------------------------------------------------- the report and the end
// report(to, cap): a *_report of the ABI with its numbers bound; called for the size, then for the text
template <class Report>
std::string report_text(Report report) {
  std::string text((size_t)report((char *)NULL, (int64_t)0), '\0');
  report(&text[0], (int64_t)text.size());
  return text;
}
template <class Report>
void print_report(Report report) {
  const std::string text = report_text(report);
  const bool wrote = fwrite(text.data(), 1, text.size(), stdout) == text.size();
  if (fflush(stdout) != 0 || !wrote) die(": write error on the standard output");
}
// PBSIM_CLI_LEAVE_CONTEXT=1 (main.cpp): the process ends behind this, the context's pools go back to the driver with it
int leave(pbsim_ctx *ctx) {
  const char *keep = getenv("PBSIM_CLI_LEAVE_CONTEXT");
  if (!(keep && *keep == '1')) pbsim_destroy(ctx);
  return 0;
}

// ---------------------------------------------------------------- the modes
const char kMapq[] = "a whole number, 0 .. 255.", kFlagWords[] = "decimal or 0x hexadecimal, 0 .. 65535.", kDepthWords[] = "a whole number, 0 .. 1000000000000.",
           kMaxIns[] = "a whole number, 1 .. 65535.", kLineWidth[] = "a whole number, 0 .. 1048576 (0: one line per record).", kPpm[] = "a whole number, 0 .. 1000000.";

// `pbsim --eval-bam MAPPED.bam --truth-bam FILE ...`: a mapper's BAM scored against finished truth BAMs (pbsim_truth_bam_eval),
// the report to stdout or --eval-out.  The odd one at its end: it has no sink, and names its truth files when the stage fails.
struct EvalArgs {
  std::string query, out;
  std::vector<std::string> truth, names;
  double overlap = 0.1;
};
void eval_overlap(const char *v, void *args) {
  char *e = NULL;
  const double overlap = ((EvalArgs *)args)->overlap = strtod(v, &e);
  if (e == v || *e || !(overlap > 0.0 && overlap <= 1.0)) die(" (eval-overlap: %s): the least intersection / union of a correct mapping, in (0, 1].", v);
}
const Opt kEvalOpts[] = {{"--eval-bam", kText, offsetof(EvalArgs, query)},
                         {"--truth-bam", kTexts, offsetof(EvalArgs, truth)},
                         {"--truth-ref-names", kNames, offsetof(EvalArgs, names)},
                         {"--eval-overlap", kHook, 0, 0, 0, nullptr, nullptr, nullptr, eval_overlap},
                         {"--eval-out", kText, offsetof(EvalArgs, out)}};

int eval_bam_main(int argc, char **argv, const pbsim_comm *comm, int device) {
  EvalArgs a;
  PARSE_STAGE(kEvalOpts, a);
  if (a.query.empty()) die(": --eval-bam MAPPED.bam: name the mapper's BAM file.");
  if (a.truth.empty()) die(": --eval-bam needs the truth: --truth-bam FILE [--truth-bam FILE ...] (the .aln.bam files of --truth-format bam).");
  need_file_names("truth-ref-names", a.names, "--truth-bam", a.truth.size());
  refuse_empty_name("truth-ref-names", a.names, true);
  std::vector<std::string> in_names = a.truth;
  in_names.push_back(a.query);
  std::vector<MappedFile> files;
  open_inputs(in_names, &files);
  pbsim_ctx *ctx = one_gpu_context(device);
  std::vector<pbsim_eval_truth> tr(a.truth.size());
  for (size_t f = 0; f < tr.size(); f++) tr[f] = pbsim_eval_truth{files[f].map, (int64_t)files[f].n, name_or_null(a.names, f)};
  pbsim_eval_opts opts = {(int32_t)std::min(1000L, std::max(1L, lround(a.overlap * 1000))), 0};
  int64_t counts[12], hist[512];
  if (!pbsim_truth_bam_eval(ctx, tr.data(), (int)tr.size(), files.back().map, (int64_t)files.back().n, &opts, NULL, counts, hist)) {
    fprintf(stderr, "ERROR: %s\n", pbsim_last_error());
    for (size_t f = 0; f < a.truth.size(); f++) fprintf(stderr, "ERROR: truth file %zu is %s\n", f, a.truth[f].c_str());
    quit(-1);
  }
  const std::string text = report_text([&](char *to, int64_t cap) { return pbsim_eval_report(counts, hist, to, cap); });
  FILE *fp = a.out.empty() ? stdout : fopen(a.out.c_str(), "wb");
  if (!fp) die(": Cannot open output file: %s", a.out.c_str());
  const bool wrote = fwrite(text.data(), 1, text.size(), fp) == text.size();
  if ((fp == stdout ? fflush(fp) : fclose(fp)) != 0 || !wrote) die(": write error on %s", a.out.empty() ? "the standard output" : a.out.c_str());
  return leave(ctx);
}

// `pbsim --depth-bam FILE --depth-out FILE ...`: the depth of coverage of a BAM (pbsim_bam_depth), the text to --depth-out, the
// report to stdout.
struct DepthArgs {
  std::string in, out;
  long long format = 0, window = 0, min_mapq = 0, exclude = 0x704;
  bool no_deletions = false;
};
const Opt kDepthOpts[] = {{"--depth-bam", kText, offsetof(DepthArgs, in)},
                          {"--depth-out", kText, offsetof(DepthArgs, out)},
                          {"--depth-format", kChoice, offsetof(DepthArgs, format), 0, 0, "bedgraph or window.", "bedgraph", "window"},
                          {"--depth-window", kWhole, offsetof(DepthArgs, window), 1, LLONG_MAX, "a whole number of at least 1."},
                          {"--depth-min-mapq", kWhole, offsetof(DepthArgs, min_mapq), 0, 255, kMapq},
                          {"--depth-exclude-flags", kFlags, offsetof(DepthArgs, exclude), 0, 65535, kFlagWords},
                          {"--depth-no-deletions", kSwitch, offsetof(DepthArgs, no_deletions)}};

int depth_bam_main(int argc, char **argv, const pbsim_comm *comm, int device) {
  DepthArgs a;
  PARSE_STAGE(kDepthOpts, a);
  const bool have_window = a.window != 0;  // (a window that was given is 1 or more)
  if (a.in.empty()) die(": --depth-bam FILE: name the BAM file.");
  if (a.out.empty()) die(": --depth-bam needs --depth-out FILE: the bedGraph or window text goes there (the report goes to the standard output).");
  if (a.format == 1 && !have_window) die(": --depth-format window needs --depth-window N.");
  if (a.format != 1 && have_window) die(": --depth-window N goes with --depth-format window.");
  std::vector<MappedFile> files;
  open_inputs({a.in}, &files);
  pbsim_ctx *ctx = one_gpu_context(device);
  struct Result {
    OutFile out;  // (first: the sink's user pointer is the output array's too)
    std::vector<std::string> names;
    std::vector<int64_t> rows;
  } res;
  res.out.name = a.out;
  open_outputs(&res.out, 1);
  pbsim_depth_opts opts = {(int32_t)a.exclude, (int32_t)a.min_mapq, a.no_deletions ? 0 : 1, (int32_t)a.format, (int64_t)a.window, 0};
  pbsim_depth_sink sink = {&res, text_to_0,
                           [](void *u, int32_t n_ref, const char *const *names, const int64_t *rows) {
                             Result *x = (Result *)u;
                             x->names.assign(names, names + n_ref);
                             x->rows.assign(rows, rows + 4 * (size_t)n_ref);
                             return 1;
                           },
                           NULL};
  int64_t counts[6], hist[256];
  const bool ok = pbsim_bam_depth(ctx, files[0].map, (int64_t)files[0].n, &opts, &sink, counts, hist) != 0;
  finish_outputs(&res.out, 1, ok);
  std::vector<const char *> name_ptr;
  for (const std::string &nm : res.names) name_ptr.push_back(nm.c_str());
  const int32_t n_ref = (int32_t)name_ptr.size();
  print_report([&](char *to, int64_t cap) { return pbsim_depth_report(counts, n_ref, name_ptr.data(), res.rows.data(), hist, to, cap); });
  return leave(ctx);
}

// `pbsim --stats-bam FILE [--stats-bam FILE ...] ...`: a summary of the reads of BAM files (pbsim_bam_stats), the report to
// stdout, the per-read text to --stats-out.
struct StatsArgs {
  std::vector<std::string> in;
  OutFile out;
  long long min_mapq = 0, exclude = 0x900;
};
const Opt kStatsOpts[] = {{"--stats-bam", kTexts, offsetof(StatsArgs, in)},
                          {"--stats-out", kText, offsetof(StatsArgs, out.name)},
                          {"--stats-min-mapq", kWhole, offsetof(StatsArgs, min_mapq), 0, 255, kMapq},
                          {"--stats-exclude-flags", kFlags, offsetof(StatsArgs, exclude), 0, 65535, kFlagWords}};

int stats_bam_main(int argc, char **argv, const pbsim_comm *comm, int device) {
  StatsArgs a;
  PARSE_STAGE(kStatsOpts, a);
  if (a.in.empty()) die(": --stats-bam FILE: name the BAM file.");
  std::vector<MappedFile> files;
  open_inputs(a.in, &files);
  pbsim_ctx *ctx = one_gpu_context(device);
  open_outputs(&a.out, 1);
  std::vector<pbsim_stats_file> in(files.size());
  for (size_t f = 0; f < files.size(); f++) in[f] = pbsim_stats_file{files[f].map, (int64_t)files[f].n};
  pbsim_stats_opts opts = {(int32_t)a.exclude, (int32_t)a.min_mapq, 0};
  pbsim_stats_sink sink = {&a.out, a.out.fp ? text_to_0 : NULL};
  int64_t counts[10], len_row[16], totals[12], hist_q[128], hist_identity[1001], hist_qacc[1001];
  const bool ok = pbsim_bam_stats(ctx, in.data(), (int)in.size(), &opts, &sink, counts, len_row, totals, hist_q, hist_identity, hist_qacc) != 0;
  finish_outputs(&a.out, 1, ok, &a.in);
  print_report([&](char *to, int64_t cap) { return pbsim_stats_report(counts, len_row, totals, hist_q, hist_identity, hist_qacc, to, cap); });
  return leave(ctx);
}

// The four modes that read aligned BAM files against their genome share their first options and their inputs: the files, the
// genome (mapped before a GPU is touched), a name per file, one output.
struct PileArgs {
  std::vector<std::string> in, names;
  std::string genome;
  OutFile out;
  long long min_mapq = 0, min_baseq = 0, min_depth = 1, exclude = 0x900, max_ins = 1024, format = 0, fill = 0, line_width = 60;
};
struct PileInputs {
  std::vector<MappedFile> files;
  GenomeRefs g;
  std::vector<pbsim_errors_file> in;
  pbsim_ctx *ctx = nullptr;
};
// mode: "errors", "pileup", ..; needs_out: what the mode says when it must have --<mode>-out and has none
void open_pile_inputs(const std::string &mode, PileArgs &a, const char *needs_out, int device, PileInputs *p) {
  const std::string bam = "--" + mode + "-bam", genome = "--" + mode + "-genome", names = mode + "-ref-names";
  if (a.in.empty()) die(": %s FILE: name the BAM file.", bam.c_str());
  if (a.genome.empty()) die(": %s needs %s FASTA: the genome the reads were aligned to.", bam.c_str(), genome.c_str());
  if (needs_out && a.out.name.empty()) die(needs_out);
  need_file_names(names.c_str(), a.names, bam.c_str(), a.in.size());
  refuse_empty_name(names.c_str(), a.names);
  open_inputs(a.in, &p->files);
  map_genome_refs(genome.c_str(), a.genome, nullptr, &p->g);
  p->ctx = one_gpu_context(device);
  open_outputs(&a.out, 1);
  p->in = errors_files(p->files, a.names);
}

// `pbsim --errors-bam FILE [--errors-bam FILE ...] --errors-genome FASTA ...`: the error profile of aligned reads against their
// genome (pbsim_bam_errors), the report to stdout, the per-read text to --errors-out.
const Opt kErrorsOpts[] = {{"--errors-bam", kTexts, offsetof(PileArgs, in)},
                           {"--errors-genome", kText, offsetof(PileArgs, genome)},
                           {"--errors-ref-names", kNames, offsetof(PileArgs, names)},
                           {"--errors-out", kText, offsetof(PileArgs, out.name)},
                           {"--errors-min-mapq", kWhole, offsetof(PileArgs, min_mapq), 0, 255, kMapq},
                           {"--errors-exclude-flags", kFlags, offsetof(PileArgs, exclude), 0, 65535, kFlagWords}};

int errors_bam_main(int argc, char **argv, const pbsim_comm *comm, int device) {
  PileArgs a;
  PileInputs p;
  PARSE_STAGE(kErrorsOpts, a);
  open_pile_inputs("errors", a, nullptr, device, &p);
  pbsim_errors_opts opts = {(int32_t)a.exclude, (int32_t)a.min_mapq, 0};
  pbsim_errors_sink sink = {&a.out, a.out.fp ? text_to_0 : NULL};
  std::vector<pbsim_errors_result> result(1);
  const bool ok = pbsim_bam_errors(p.ctx, p.g.refs.data(), (int)p.g.refs.size(), p.in.data(), (int)p.in.size(), &opts, &sink, result.data()) != 0;
  finish_outputs(&a.out, 1, ok, &a.in);
  print_report([&](char *to, int64_t cap) { return pbsim_errors_report(result.data(), to, cap); });
  return leave(p.ctx);
}

// `pbsim --pileup-bam FILE [--pileup-bam FILE ...] --pileup-genome FASTA ...`: the pileup of aligned reads against their genome
// (pbsim_bam_pileup), the report to stdout, the sites' text to --pileup-out.
const Opt kPileupOpts[] = {{"--pileup-bam", kTexts, offsetof(PileArgs, in)},
                           {"--pileup-genome", kText, offsetof(PileArgs, genome)},
                           {"--pileup-ref-names", kNames, offsetof(PileArgs, names)},
                           {"--pileup-out", kText, offsetof(PileArgs, out.name)},
                           {"--pileup-format", kChoice, offsetof(PileArgs, format), 0, 0, "sites or all.", "sites", "all"},
                           {"--pileup-min-mapq", kWhole, offsetof(PileArgs, min_mapq), 0, 255, kMapq},
                           {"--pileup-min-baseq", kWhole, offsetof(PileArgs, min_baseq), 0, 255, kMapq},
                           {"--pileup-min-depth", kWhole, offsetof(PileArgs, min_depth), 0, 1000000000000LL, kDepthWords}};

int pileup_bam_main(int argc, char **argv, const pbsim_comm *comm, int device) {
  PileArgs a;
  PileInputs p;
  PARSE_STAGE(kPileupOpts, a);
  open_pile_inputs("pileup", a, nullptr, device, &p);
  pbsim_pileup_opts opts = {0x900, (int32_t)a.min_mapq, (int32_t)a.min_baseq, (int32_t)a.format, (int64_t)a.min_depth, 0};
  pbsim_pileup_sink sink = {&a.out, a.out.fp ? text_to_0 : NULL, NULL};
  pbsim_pileup_result result;
  const bool ok = pbsim_bam_pileup(p.ctx, p.g.refs.data(), (int)p.g.refs.size(), p.in.data(), (int)p.in.size(), &opts, &sink, &result) != 0;
  finish_outputs(&a.out, 1, ok, &a.in);
  print_report([&](char *to, int64_t cap) { return pbsim_pileup_report(&result, to, cap); });
  return leave(p.ctx);
}

// `pbsim --consensus-bam FILE [--consensus-bam FILE ...] --consensus-genome FASTA --consensus-out FILE ...`: the consensus of the
// aligned reads against their genome (pbsim_bam_consensus), the report to stdout, the FASTA to --consensus-out.
const Opt kConsensusOpts[] = {{"--consensus-bam", kTexts, offsetof(PileArgs, in)},
                              {"--consensus-genome", kText, offsetof(PileArgs, genome)},
                              {"--consensus-out", kText, offsetof(PileArgs, out.name)},
                              {"--consensus-ref-names", kNames, offsetof(PileArgs, names)},
                              {"--consensus-min-mapq", kWhole, offsetof(PileArgs, min_mapq), 0, 255, kMapq},
                              {"--consensus-min-baseq", kWhole, offsetof(PileArgs, min_baseq), 0, 255, kMapq},
                              {"--consensus-min-depth", kWhole, offsetof(PileArgs, min_depth), 0, 1000000000000LL, kDepthWords},
                              {"--consensus-exclude-flags", kFlags, offsetof(PileArgs, exclude), 0, 65535, kFlagWords},
                              {"--consensus-fill", kChoice, offsetof(PileArgs, fill), 0, 0, "n or ref.", "n", "ref"},
                              {"--consensus-max-ins", kWhole, offsetof(PileArgs, max_ins), 1, 65535, kMaxIns},
                              {"--consensus-line-width", kWhole, offsetof(PileArgs, line_width), 0, 1048576, kLineWidth}};

int consensus_bam_main(int argc, char **argv, const pbsim_comm *comm, int device) {
  PileArgs a;
  PileInputs p;
  PARSE_STAGE(kConsensusOpts, a);
  open_pile_inputs("consensus", a, ": --consensus-bam needs --consensus-out FILE: where the consensus FASTA goes.", device, &p);
  pbsim_consensus_opts opts = {(int32_t)a.exclude, (int32_t)a.min_mapq, (int32_t)a.min_baseq, (int32_t)a.fill, (int64_t)a.min_depth, (int32_t)a.max_ins, (int32_t)a.line_width, 0};
  pbsim_consensus_sink sink = {&a.out, text_to_0, NULL};
  pbsim_consensus_result result;
  const bool ok = pbsim_bam_consensus(p.ctx, p.g.refs.data(), (int)p.g.refs.size(), p.in.data(), (int)p.in.size(), &opts, &sink, &result) != 0;
  finish_outputs(&a.out, 1, ok, &a.in);
  print_report([&](char *to, int64_t cap) { return pbsim_consensus_report(&result, to, cap); });
  return leave(p.ctx);
}

// `pbsim --call-bam FILE [--call-bam FILE ...] --call-genome FASTA --call-out FILE ...`: the variants the aligned reads support
// against their genome (pbsim_bam_call), the report to stdout, the VCF to --call-out.
const Opt kCallOpts[] = {{"--call-bam", kTexts, offsetof(PileArgs, in)},
                         {"--call-genome", kText, offsetof(PileArgs, genome)},
                         {"--call-out", kText, offsetof(PileArgs, out.name)},
                         {"--call-ref-names", kNames, offsetof(PileArgs, names)},
                         {"--call-min-mapq", kWhole, offsetof(PileArgs, min_mapq), 0, 255, kMapq},
                         {"--call-min-baseq", kWhole, offsetof(PileArgs, min_baseq), 0, 255, kMapq},
                         {"--call-min-depth", kWhole, offsetof(PileArgs, min_depth), 0, 1000000000000LL, kDepthWords},
                         {"--call-exclude-flags", kFlags, offsetof(PileArgs, exclude), 0, 65535, kFlagWords},
                         {"--call-max-ins", kWhole, offsetof(PileArgs, max_ins), 1, 65535, kMaxIns}};

int call_bam_main(int argc, char **argv, const pbsim_comm *comm, int device) {
  PileArgs a;
  PileInputs p;
  PARSE_STAGE(kCallOpts, a);
  open_pile_inputs("call", a, ": --call-bam needs --call-out FILE: where the VCF goes.", device, &p);
  pbsim_call_opts opts = {(int32_t)a.exclude, (int32_t)a.min_mapq, (int32_t)a.min_baseq, (int32_t)a.max_ins, (int64_t)a.min_depth, 0};
  pbsim_call_sink sink = {&a.out, text_to_0, NULL};
  pbsim_call_result result;
  const bool ok = pbsim_bam_call(p.ctx, p.g.refs.data(), (int)p.g.refs.size(), p.in.data(), (int)p.in.size(), &opts, &sink, &result) != 0;
  finish_outputs(&a.out, 1, ok, &a.in);
  print_report([&](char *to, int64_t cap) { return pbsim_call_report(&result, to, cap); });
  return leave(p.ctx);
}

// `pbsim --mutate-genome FASTA --mutate-out FASTA --mutate-vcf FILE ...`: a variant genome and its truth variants drawn from the
// genome and a seed (pbsim_genome_mutate), the report to stdout, the variant genome to --mutate-out, the VCF to --mutate-vcf.
// The context is there before the genome is mapped: a BGZF file is inflated on its device.
struct MutateArgs {
  std::string genome;
  OutFile outs[2];  // the variant genome, the VCF
  long long seed = 1, snv = 1000, ins = 100, del = 100, ext = 500000, max_indel = 50, line_width = 60;
};
const Opt kMutateOpts[] = {{"--mutate-genome", kText, offsetof(MutateArgs, genome)},
                           {"--mutate-out", kText, offsetof(MutateArgs, outs[0].name)},
                           {"--mutate-vcf", kText, offsetof(MutateArgs, outs[1].name)},
                           {"--mutate-seed", kWhole, offsetof(MutateArgs, seed), 0, 4294967295LL, "a whole number, 0 .. 4294967295."},
                           {"--mutate-snv-ppm", kWhole, offsetof(MutateArgs, snv), 0, 1000000, kPpm},
                           {"--mutate-ins-ppm", kWhole, offsetof(MutateArgs, ins), 0, 1000000, kPpm},
                           {"--mutate-del-ppm", kWhole, offsetof(MutateArgs, del), 0, 1000000, kPpm},
                           {"--mutate-ext-ppm", kWhole, offsetof(MutateArgs, ext), 0, 999999, "a whole number, 0 .. 999999."},
                           {"--mutate-max-indel", kWhole, offsetof(MutateArgs, max_indel), 1, 65535, kMaxIns},
                           {"--mutate-line-width", kWhole, offsetof(MutateArgs, line_width), 0, 1048576, kLineWidth}};

int mutate_genome_main(int argc, char **argv, const pbsim_comm *comm, int device) {
  MutateArgs a;
  PARSE_STAGE(kMutateOpts, a);
  if (a.genome.empty()) die(": --mutate-genome FASTA: name the genome.");
  if (a.outs[0].name.empty()) die(": --mutate-genome needs --mutate-out FASTA: where the variant genome goes.");
  if (a.outs[1].name.empty()) die(": --mutate-genome needs --mutate-vcf FILE: where the truth variants go.");
  if (a.snv + a.ins + a.del > 1000000) die(" (mutate-snv-ppm + mutate-ins-ppm + mutate-del-ppm): the three rates sum to more than 1000000.");
  if (access(a.genome.c_str(), R_OK) != 0) die(": --mutate-genome %s: Cannot open file: %s", a.genome.c_str(), a.genome.c_str());
  pbsim_ctx *ctx = one_gpu_context(device);
  GenomeRefs g;
  map_genome_refs("--mutate-genome", a.genome, ctx, &g);
  open_outputs(a.outs, 2);
  pbsim_mutate_opts opts = {(uint32_t)a.seed, (int32_t)a.snv, (int32_t)a.ins, (int32_t)a.del, (int32_t)a.ext, (int32_t)a.max_indel, (int32_t)a.line_width, 0};
  pbsim_mutate_sink sink = {a.outs, text_to_0, text_to_1, NULL, NULL};
  pbsim_mutate_result result;
  const bool ok = pbsim_genome_mutate(ctx, g.refs.data(), (int)g.refs.size(), &opts, &sink, &result) != 0;
  finish_outputs(a.outs, 2, ok);
  print_report([&](char *to, int64_t cap) { return pbsim_mutate_report(&result, to, cap); });
  return leave(ctx);
}

// `pbsim --compare-vcf CALLS --compare-truth TRUTH --compare-genome FASTA ...`: a call set scored against the truth variants
// (pbsim_vcf_compare), the report to stdout, the annotated lines to --compare-out.  The context is made before the files are
// read: a BGZF file is inflated on its device.
struct CompareArgs {
  std::string calls, truth, genome;
  OutFile out;
  std::vector<std::string> names;
  long long lines = 0, min_ms = 0;
};
const Opt kCompareOpts[] = {{"--compare-vcf", kText, offsetof(CompareArgs, calls)},
                            {"--compare-truth", kText, offsetof(CompareArgs, truth)},
                            {"--compare-genome", kText, offsetof(CompareArgs, genome)},
                            {"--compare-out", kText, offsetof(CompareArgs, out.name)},
                            {"--compare-lines", kChoice, offsetof(CompareArgs, lines), 0, 0, "discordant or all.", "discordant", "all"},
                            {"--compare-min-ms", kWhole, offsetof(CompareArgs, min_ms), 0, 2147483647LL, "a whole number, 0 .. 2147483647."},
                            {"--compare-ref-names", kNames, offsetof(CompareArgs, names)}};

// the names a VCF mode hands its stage in place of the genome's own: NULL without the option
std::vector<const char *> used_names(const std::vector<std::string> &names) {
  std::vector<const char *> used;
  for (const std::string &n : names) used.push_back(n.c_str());
  return used;
}

int compare_vcf_main(int argc, char **argv, const pbsim_comm *comm, int device) {
  CompareArgs a;
  PARSE_STAGE(kCompareOpts, a);
  if (a.calls.empty()) die(": --compare-vcf CALLS: name the call set.");
  if (a.truth.empty()) die(": --compare-vcf needs --compare-truth VCF: the truth variants.");
  if (a.genome.empty()) die(": --compare-vcf needs --compare-genome FASTA: the genome both files speak of.");
  refuse_empty_name("compare-ref-names", a.names);
  need_readable({&a.calls, &a.truth, &a.genome});
  pbsim_ctx *ctx = one_gpu_context(device);
  VcfBytes truth, calls;
  load_vcf(a.truth, ctx, &truth);
  load_vcf(a.calls, ctx, &calls);
  GenomeRefs g;
  map_genome_refs("--compare-genome", a.genome, ctx, &g);
  need_record_names("compare-ref-names", a.names, g.refs.size());
  const std::vector<const char *> used = used_names(a.names);
  open_outputs(&a.out, 1);
  pbsim_compare_opts opts = {(int32_t)a.lines, (int32_t)a.min_ms, 0};
  pbsim_compare_sink sink = {&a.out, a.out.fp ? text_to_0 : NULL};
  pbsim_compare_result result;
  const bool ok = pbsim_vcf_compare(ctx, g.refs.data(), (int)g.refs.size(), used.empty() ? NULL : used.data(), truth.bytes, truth.n, calls.bytes, calls.n, &opts,
                                    &sink, &result) != 0;
  finish_outputs(&a.out, 1, ok);
  print_report([&](char *to, int64_t cap) { return pbsim_compare_report(&result, to, cap); });
  return leave(ctx);
}

// `pbsim --apply-vcf VCF --apply-genome FASTA --apply-out FASTA ...`: the lines of a VCF applied to the genome (pbsim_vcf_apply),
// the summary to stdout, the spliced genome to --apply-out, the annotated lines to --apply-report, the origin map to
// --apply-origin.  The context is made before the files are read: a BGZF file is inflated on its device.
struct ApplyArgs {
  std::string vcf, genome, sample_name;
  OutFile outs[3];  // the spliced genome, the annotated lines, the origin map
  std::vector<std::string> names;
  long long haplotype = 0, sample = 0, lines = 0, line_width = 60;
};
// a 0-based column, else a sample's name, looked up in the file's #CHROM line once the file is read
void apply_sample(const char *v, void *args) {
  ApplyArgs *a = (ApplyArgs *)args;
  if (!*v) die(" (apply-sample): a 0-based sample column or a sample's name.");
  a->sample_name.clear();
  if (!whole_number(v, 10, 0, 2147483647LL, &a->sample)) a->sample_name = v, a->sample = 0;
}
const Opt kApplyOpts[] = {{"--apply-vcf", kText, offsetof(ApplyArgs, vcf)},
                          {"--apply-genome", kText, offsetof(ApplyArgs, genome)},
                          {"--apply-out", kText, offsetof(ApplyArgs, outs[0].name)},
                          {"--apply-ref-names", kNames, offsetof(ApplyArgs, names)},
                          {"--apply-haplotype", kWhole, offsetof(ApplyArgs, haplotype), 0, 2, "0 (the first ALT of every line), 1 or 2."},
                          {"--apply-sample", kHook, 0, 0, 0, nullptr, nullptr, nullptr, apply_sample},
                          {"--apply-report", kText, offsetof(ApplyArgs, outs[1].name)},
                          {"--apply-lines", kChoice, offsetof(ApplyArgs, lines), 0, 0, "discordant or all.", "discordant", "all"},
                          {"--apply-line-width", kWhole, offsetof(ApplyArgs, line_width), 0, 1048576, kLineWidth},
                          {"--apply-origin", kText, offsetof(ApplyArgs, outs[2].name)}};

int apply_vcf_main(int argc, char **argv, const pbsim_comm *comm, int device) {
  ApplyArgs a;
  PARSE_STAGE(kApplyOpts, a);
  if (a.vcf.empty()) die(": --apply-vcf VCF: name the variants.");
  if (a.genome.empty()) die(": --apply-vcf needs --apply-genome FASTA: the genome the file speaks of.");
  if (a.outs[0].name.empty()) die(": --apply-vcf needs --apply-out FASTA: where the spliced genome goes.");
  refuse_empty_name("apply-ref-names", a.names);
  need_readable({&a.vcf, &a.genome});
  pbsim_ctx *ctx = one_gpu_context(device);
  VcfBytes vcf;
  load_vcf(a.vcf, ctx, &vcf);
  GenomeRefs g;
  map_genome_refs("--apply-genome", a.genome, ctx, &g);
  if (!a.sample_name.empty()) {
    const int32_t column = pbsim_apply_sample(vcf.bytes, vcf.n, a.sample_name.c_str());
    if (column < 0) die(" (apply-sample: %s): the #CHROM line of %s names no such sample.", a.sample_name.c_str(), a.vcf.c_str());
    a.sample = column;
  }
  need_record_names("apply-ref-names", a.names, g.refs.size());
  const std::vector<const char *> used = used_names(a.names);
  open_outputs(a.outs, 3);
  pbsim_apply_opts opts = {(int32_t)a.haplotype, (int32_t)a.sample, (int32_t)a.lines, (int32_t)a.line_width, 0};
  pbsim_apply_sink sink = {a.outs, text_to_0, a.outs[1].fp ? text_to_1 : NULL, NULL,
                           [](void *u, int32_t, const int32_t *z, int64_t k) { return put((OutFile *)u + 2, z, 4 * (size_t)k); }};
  if (!a.outs[2].fp) sink.on_origin = NULL;
  pbsim_apply_result result;
  const bool ok = pbsim_vcf_apply(ctx, g.refs.data(), (int)g.refs.size(), used.empty() ? NULL : used.data(), vcf.bytes, vcf.n, &opts, &sink, &result) != 0;
  finish_outputs(a.outs, 3, ok);
  print_report([&](char *to, int64_t cap) { return pbsim_apply_report(&result, to, cap); });
  return leave(ctx);
}

// `pbsim --lift-bam IN --lift-out OUT --lift-genome FASTA --lift-vcf VCF ...`: a truth BAM whose records lie on the variant genome
// that VCF makes of FASTA, placed on FASTA itself (pbsim_bam_lift), the summary to stdout.  The VCF is the chain: pbsim_vcf_apply
// runs with on_origin alone -- no FASTA, no text --, and its origin maps go to the lift; no origin file and no variant FASTA is read.
struct LiftArgs {
  std::string bam, genome, vcf, ref_name, sample_name;
  OutFile out;
  std::vector<std::string> names;
  long long haplotype = 0, sample = 0;
};
void lift_sample(const char *v, void *args) {
  LiftArgs *a = (LiftArgs *)args;
  if (!*v) die(" (lift-sample): a 0-based sample column or a sample's name.");
  a->sample_name.clear();
  if (!whole_number(v, 10, 0, 2147483647LL, &a->sample)) a->sample_name = v, a->sample = 0;
}
const Opt kLiftOpts[] = {{"--lift-bam", kText, offsetof(LiftArgs, bam)},
                         {"--lift-out", kText, offsetof(LiftArgs, out.name)},
                         {"--lift-genome", kText, offsetof(LiftArgs, genome)},
                         {"--lift-vcf", kText, offsetof(LiftArgs, vcf)},
                         {"--lift-haplotype", kWhole, offsetof(LiftArgs, haplotype), 0, 2, "0 (the first ALT of every line), 1 or 2."},
                         {"--lift-sample", kHook, 0, 0, 0, nullptr, nullptr, nullptr, lift_sample},
                         {"--lift-ref-names", kNames, offsetof(LiftArgs, names)},
                         {"--lift-ref-name", kText, offsetof(LiftArgs, ref_name)}};

int lift_bam_main(int argc, char **argv, const pbsim_comm *comm, int device) {
  LiftArgs a;
  PARSE_STAGE(kLiftOpts, a);
  if (a.bam.empty()) die(": --lift-bam IN: name the BAM file whose records lie on the variant genome.");
  if (a.out.name.empty()) die(": --lift-bam needs --lift-out FILE: where the lifted BAM goes.");
  if (a.genome.empty()) die(": --lift-bam needs --lift-genome FASTA: the original genome.");
  if (a.vcf.empty()) die(": --lift-bam needs --lift-vcf VCF: the variants the variant genome was made with (--mutate-vcf's file, or the file given to --apply-vcf).");
  refuse_empty_name("lift-ref-names", a.names);
  need_readable({&a.bam, &a.genome, &a.vcf});
  pbsim_ctx *ctx = one_gpu_context(device);
  VcfBytes vcf;
  load_vcf(a.vcf, ctx, &vcf);
  GenomeRefs g;
  map_genome_refs("--lift-genome", a.genome, ctx, &g);
  if (!a.sample_name.empty()) {
    const int32_t column = pbsim_apply_sample(vcf.bytes, vcf.n, a.sample_name.c_str());
    if (column < 0) die(" (lift-sample: %s): the #CHROM line of %s names no such sample.", a.sample_name.c_str(), a.vcf.c_str());
    a.sample = column;
  }
  need_record_names("lift-ref-names", a.names, g.refs.size());
  const std::vector<const char *> used = used_names(a.names);
  std::vector<MappedFile> bam;
  open_inputs({a.bam}, &bam);
  // the chain: the origin map of every genome record
  std::vector<std::vector<int32_t>> maps(g.refs.size());
  pbsim_apply_opts opts = {(int32_t)a.haplotype, (int32_t)a.sample, 0, 60, 0};
  pbsim_apply_sink chain = {&maps, NULL, NULL, NULL, [](void *u, int32_t ref, const int32_t *z, int64_t k) {
                              (*(std::vector<std::vector<int32_t>> *)u)[(size_t)ref].assign(z, z + k);
                              return 1;
                            }};
  pbsim_apply_result applied;
  if (!pbsim_vcf_apply(ctx, g.refs.data(), (int)g.refs.size(), used.empty() ? NULL : used.data(), vcf.bytes, vcf.n, &opts, &chain, &applied)) check(0);
  std::vector<pbsim_lift_origin> origins(maps.size());
  for (size_t r = 0; r < maps.size(); r++) origins[r] = pbsim_lift_origin{maps[r].data(), (int64_t)maps[r].size()};
  open_outputs(&a.out, 1);
  const pbsim_errors_file file = {bam[0].map, (int64_t)bam[0].n, a.ref_name.empty() ? NULL : a.ref_name.c_str()};
  pbsim_lift_sink sink = {&a.out, text_to_0};
  pbsim_lift_result result;
  const bool ok = pbsim_bam_lift(ctx, g.refs.data(), (int)g.refs.size(), origins.data(), &file, &sink, &result) != 0;
  finish_outputs(&a.out, 1, ok);
  print_report([&](char *to, int64_t cap) { return pbsim_lift_report(&result, to, cap); });
  return leave(ctx);
}

#define PBSIM_STAGE_ROW(option, run) {option, run},
const StageMode kStageModes[] = {PBSIM_STAGE_MODES(PBSIM_STAGE_ROW){nullptr, nullptr}};

}  // namespace

const StageMode *stage_modes() { return kStageModes; }

}  // namespace cli
}  // namespace pbsim
