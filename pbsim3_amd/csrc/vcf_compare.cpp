// vcf_compare.cpp -- pbsim_vcf_compare: a call set scored against the truth variants, both VCF texts over one genome (the rule:
// include/pbsim3_amd.h, tests/compare_model.py).  The host's part: the genome into HBM as the BAM stages hold it (load_genome,
// bam_genome.h); the contig names' sorted hash table; both texts into one buffer; the line table's sizes, the tiles' scan and the
// fill; the parse; the sort of (site, line) (bs_sort_pairs); the match; the tally with the annotated text's sizes, the scan again,
// the header -- written here -- and the lines behind it; the text to the sink (deliver_text).  The kernels are vcf_compare.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "bam_errors.h"
#include "bam_genome.h"
#include "bam_sort.h"
#include "kernels.h"
#include "vcf_compare.h"

namespace pbsim {

namespace {

const char kWho[] = "pbsim_vcf_compare: ";
const BamStage kStage = {kWho, "the stage holds the genome at 2 bytes per base, both VCF texts, 104 bytes per data line, the sort's scratch and the annotated text in HBM at once, and does not chunk"};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

int compare_vcf(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const std::vector<std::string> &used, const void *truth, int64_t n_truth,
                const void *calls, int64_t n_calls, const pbsim_compare_opts &o, const pbsim_compare_sink *sink, pbsim_compare_result *result) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "compare");
  const bool want_text = sink && sink->on_text;
  Genome genome;
  if (!load_genome(c, kStage, refs, n_refs, &genome)) return PBSIM_FAILED;
  ph.mark("genome");
  // ---- the names' table and the texts
  std::vector<uint64_t> hash;
  std::vector<int32_t> record;
  compare_name_table(used, &hash, &record);
  std::string names;
  std::vector<int64_t> name_at;
  for (int r = 0; r < n_refs; r++) {
    name_at.push_back((int64_t)names.size());
    names += used[(size_t)r];
  }
  name_at.push_back((int64_t)names.size());
  const int64_t tiles0 = (n_truth + kCmpTile - 1) / kCmpTile, tiles = tiles0 + (n_calls + kCmpTile - 1) / kCmpTile;
  DevBuf d_at, d_len, d_hash, d_record, d_name_at, d_names, d_bytes, d_tile, d_scan_tmp, d_cells;
  if (!alloc(d_at, n_refs * 8, "the genome records' places") || !alloc(d_len, n_refs * 8, "the genome records' lengths") ||
      !alloc(d_hash, n_refs * 8, "the names' hashes") || !alloc(d_record, n_refs * 4, "the names' records") ||
      !alloc(d_name_at, (n_refs + 1) * 8, "the genome records' names") || !alloc(d_names, (int64_t)names.size() + 1, "the genome records' names") ||
      !alloc(d_bytes, tiles * kCmpTile + 64, "the VCF texts") || !alloc(d_tile, (tiles + 1) * 8, "the tiles") ||
      !alloc(d_scan_tmp, (tiles / 1024 + 8) * 8, "the scan's scratch") || !alloc(d_cells, kCmpCells * 8, "the counts"))
    return PBSIM_FAILED;
  HIP_OK(hipMemcpyAsync(d_at.p, genome.at.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_len.p, genome.len.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_hash.p, hash.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_record.p, record.data(), (size_t)n_refs * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_name_at.p, name_at.data(), name_at.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(d_bytes.p, 0, (size_t)(tiles * kCmpTile + 64), st));
  if (n_truth > 0) HIP_OK(hipMemcpyAsync(d_bytes.p, truth, (size_t)n_truth, hipMemcpyHostToDevice, st));
  if (n_calls > 0) HIP_OK(hipMemcpyAsync(d_bytes.as<char>() + tiles0 * kCmpTile, calls, (size_t)n_calls, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(d_cells.p, 0, kCmpCells * 8, st));
  const CmpText text = {d_bytes.as<uint8_t>(), {n_truth, n_calls}, tiles0, tiles};
  const CmpGenome g = {n_refs, d_at.as<int64_t>(), d_len.as<int64_t>(), genome.seq.as<uint8_t>(), d_hash.as<uint64_t>(), d_record.as<int32_t>(),
                       d_name_at.as<int64_t>(), d_names.as<char>()};
  unsigned long long *cells = d_cells.as<unsigned long long>();
  int64_t *tile = d_tile.as<int64_t>();
  HIP_OK(hipStreamSynchronize(st));  // (the caller's texts have been read)
  ph.mark("upload");
  // ---- the line table
  launch_compare_line_sizes(text, tile, st);
  HIP_OK(hipGetLastError());
  launch_exclusive_scan_i64(tile, tile, tiles, d_scan_tmp.as<int64_t>(), tile + tiles, st);
  HIP_OK(hipGetLastError());
  int64_t n_lines = 0, n0 = 0;
  HIP_OK(hipMemcpyAsync(&n_lines, tile + tiles, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(&n0, tile + tiles0, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (n_lines >= kCmpMaxLines)
    return fail(std::string(kWho) + "the two files have " + std::to_string(n_lines) + " data lines: together they must have fewer than " +
                std::to_string(kCmpMaxLines));
  const int64_t text_tiles = (n_lines + kCmpTextTile - 1) / kCmpTextTile;
  DevBuf d_line, d_key, d_val, d_key2, d_val2, d_sort_tmp, d_text_tile, d_text_tmp;
  if (!alloc(d_line, n_lines * (int64_t)sizeof(CmpLine), "the lines") || !alloc(d_key, n_lines * 8, "the lines' sites") ||
      !alloc(d_val, n_lines * 4, "the lines' numbers") || !alloc(d_key2, n_lines * 8, "the sorted sites") ||
      !alloc(d_val2, n_lines * 4, "the sorted lines") || !alloc(d_text_tile, (text_tiles + 1) * 8, "the text's tiles") ||
      !alloc(d_text_tmp, (text_tiles / 1024 + 8) * 8, "the scan's scratch"))
    return PBSIM_FAILED;
  CmpLine *line = d_line.as<CmpLine>();
  launch_compare_line_fill(text, tile, line, st);
  HIP_OK(hipGetLastError());
  ph.mark("lines");
  // ---- parse, sort, match
  launch_compare_parse(text, g, line, n_lines, n0, o.min_ms, d_key.as<uint64_t>(), d_val.as<uint32_t>(), cells, st);
  HIP_OK(hipGetLastError());
  ph.mark("parse");
  if (n_lines > 0) {
    int end_bit = 32;  // the keys go up to n_refs << 32
    while (end_bit < 64 && ((uint64_t)n_refs >> (end_bit - 32)) != 0) end_bit++;
    size_t tb = 0;
    HIP_OK(bs_sort_pairs(nullptr, &tb, d_key.as<uint64_t>(), d_key2.as<uint64_t>(), d_val.as<uint32_t>(), d_val2.as<uint32_t>(), n_lines, end_bit, st));
    if (!alloc(d_sort_tmp, (int64_t)tb, "the sort's scratch")) return PBSIM_FAILED;
    HIP_OK(bs_sort_pairs(d_sort_tmp.p, &tb, d_key.as<uint64_t>(), d_key2.as<uint64_t>(), d_val.as<uint32_t>(), d_val2.as<uint32_t>(), n_lines, end_bit, st));
  }
  ph.mark("sort");
  launch_compare_match(text, line, n_lines, n0, d_key2.as<uint64_t>(), d_val2.as<uint32_t>(), n_refs, st);
  HIP_OK(hipGetLastError());
  ph.mark("match");
  // ---- the tally and the annotated text
  int64_t *text_tile = d_text_tile.as<int64_t>();
  launch_compare_text_sizes(text, line, n_lines, n0, o.lines, text_tile, cells, st);
  HIP_OK(hipGetLastError());
  launch_exclusive_scan_i64(text_tile, text_tile, text_tiles, d_text_tmp.as<int64_t>(), text_tile + text_tiles, st);
  HIP_OK(hipGetLastError());
  int64_t n_body = 0;
  std::vector<uint64_t> h_cells(kCmpCells);
  HIP_OK(hipMemcpyAsync(&n_body, text_tile + text_tiles, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_cells.data(), d_cells.p, kCmpCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("tally");
  if (h_cells[kCmpCellTooLong] != 0)
    return fail(std::string(kWho) + std::to_string(h_cells[kCmpCellTooLong]) + " data lines are longer than " + std::to_string(kCmpMaxSpan) + " bytes");
  const int64_t n_head = (int64_t)strlen(kCmpTextHeader), n_text = n_head + n_body;
  std::deque<FileText> texts;
  if (want_text) {
    texts.emplace_back();
    FileText &t = texts.back();
    t.n = n_text;
    if (!alloc(t.d, t.n, "the annotated text")) return PBSIM_FAILED;
    HIP_OK(hipMemcpyAsync(t.d.p, kCmpTextHeader, (size_t)n_head, hipMemcpyHostToDevice, st));
    launch_compare_text_fill(text, line, n_lines, n0, o.lines, text_tile, t.d.as<char>() + n_head, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("text");
    if (!deliver_text(st, kStage, texts, n_text, o.piece_bytes, sink->on_text, sink->user)) return PBSIM_FAILED;
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("deliver");
  }
  // ---- what the caller is told
  for (int w = 0; w < 2; w++)
    for (int k = 0; k < kCmpFileCells; k++) result->files[w][k] = (int64_t)h_cells[(size_t)(kCmpCellFiles + w * kCmpFileCells + k)];
  for (int t = 0; t < kCmpTypes; t++)
    for (int k = 0; k < kCmpTypeCells; k++) result->types[t][k] = (int64_t)h_cells[(size_t)(kCmpCellTypes + t * kCmpTypeCells + k)];
  for (int w = 0; w < 2; w++)
    for (int b = 0; b < kCmpBins; b++)
      for (int k = 0; k < kCmpLengthCells; k++)
        result->lengths[w][b][k] = (int64_t)h_cells[(size_t)(kCmpCellLengths + (w * kCmpBins + b) * kCmpLengthCells + k)];
  for (int m = 0; m < kCmpMsBins; m++)
    for (int k = 0; k < 2; k++) result->ms[m][k] = (int64_t)h_cells[(size_t)(kCmpCellMs + 2 * m + k)];
  result->text_bytes = n_text;
  if (result->files[0][kCfLines] != n0 || result->files[0][kCfLines] + result->files[1][kCfLines] != n_lines)
    return fail(std::string(kWho) + "the tally counted " + std::to_string(result->files[0][kCfLines]) + " and " +
                std::to_string(result->files[1][kCfLines]) + " data lines where the line table has " + std::to_string(n0) + " of " + std::to_string(n_lines));
  {
    char sum[400];
    snprintf(sum, sizeof sum, "%d genome records, %.3f + %.3f MB of VCF in %lld tiles, %lld + %lld data lines in %lld tiles, %.3f MB of text", n_refs,
             n_truth / 1e6, n_calls / 1e6, (long long)tiles, (long long)n0, (long long)(n_lines - n0), (long long)text_tiles, n_text / 1e6);
    ph.print(sum);
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_vcf_compare(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const char *const *ref_names, const void *truth, int64_t n_truth,
                                 const void *calls, int64_t n_calls, const pbsim_compare_opts *opts, const pbsim_compare_sink *sink,
                                 pbsim_compare_result *result) {
  using pbsim::fail;
  if (!c || !refs || n_refs < 1 || !result || n_truth < 0 || n_calls < 0 || (n_truth > 0 && !truth) || (n_calls > 0 && !calls))
    return fail("pbsim_vcf_compare: bad argument");
  pbsim_compare_opts o;
  std::string err;
  std::vector<std::string> used;
  if (!pbsim::compare_check_opts(opts, &o, &err) || !pbsim::errors_check_genome(refs, n_refs, &err)) return fail("pbsim_vcf_compare: " + err);
  std::vector<const char *> own((size_t)n_refs);
  for (int r = 0; r < n_refs; r++) own[(size_t)r] = refs[r].name;
  if (!pbsim::compare_check_names(own.data(), ref_names, n_refs, &used, &err)) return fail("pbsim_vcf_compare: " + err);
  memset(result, 0, sizeof *result);
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::compare_vcf(c, refs, n_refs, used, truth, n_truth, calls, n_calls, o, sink, result);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
    memset(result, 0, sizeof *result);
  }
  return ok;
}
