// bam_call.cpp -- pbsim_bam_call: the differences between the genome and what the pile of aligned reads of BAM files spells, as
// VCF (the rule: include/pbsim3_amd.h, tests/call_model.py).  The host's part is pbsim_bam_consensus's up to the base pass's first
// half (consensus_front, bam_consensus_front.h), which leaves the class bytes, the cells and the slots with their emitted lengths
// in HBM; then the line pass over the groups (bam_call.hip) sizes the lines, the tiles are scanned, the header -- written here --
// goes into the front of the text's buffer, the line pass writes the lines behind it, and the text goes to the sink.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <deque>
#include <string>
#include <vector>

#include "bam_call.h"
#include "bam_consensus_front.h"
#include "bam_genome.h"
#include "kernels.h"

namespace pbsim {

namespace {

const char kWho[] = "pbsim_bam_call: ";
const BamStage kStage = {kWho, "the stage holds the genome at 2 bytes per base, the cells at 32 bytes per position, a class byte per position, one file's inflated stream and 69 bytes per record, 8 bytes per inserted base of every file, 20 bytes per base of the insertions at the ins_sites in HBM at once, and the text, and does not chunk"};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

int call_bam(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files, const pbsim_call_opts &o,
             const pbsim_call_sink *sink, pbsim_call_result *result) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "call");
  const bool want_text = sink && sink->on_text;
  ConsFront fr;
  if (!consensus_front(c, kStage, ph, refs, n_refs, files, n_files, o.exclude_flags, o.min_mapq, o.min_baseq, o.min_depth, o.max_ins, &fr)) return PBSIM_FAILED;
  ph.mark("bases");
  const uint32_t *table = fr.d_table.as<uint32_t>();
  const uint8_t *cls = fr.d_cls.as<uint8_t>();
  // ---- the lines' sizes: the consensus's tiles are free again
  DevBuf d_call, d_rec_n;
  if (!alloc(d_call, kCallCells * 8, "the variant counts") || !alloc(d_rec_n, (int64_t)n_refs * 8, "the genome records' variants")) return PBSIM_FAILED;
  HIP_OK(hipMemsetAsync(d_call.p, 0, kCallCells * 8, st));
  HIP_OK(hipMemsetAsync(d_rec_n.p, 0, (size_t)n_refs * 8, st));
  int64_t *tile = fr.d_tile.as<int64_t>();
  int64_t n_lines = 0;
  launch_call_line_sizes(fr.pg, table, cls, fr.slots, tile, d_call.as<unsigned long long>(), d_rec_n.as<unsigned long long>(), st);
  HIP_OK(hipGetLastError());
  launch_exclusive_scan_i64(tile, tile, fr.tiles, fr.d_scan_tmp.as<int64_t>(), tile + fr.tiles, st);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(&n_lines, tile + fr.tiles, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("lines");
  std::vector<const char *> names((size_t)n_refs);
  for (int r = 0; r < n_refs; r++) names[(size_t)r] = refs[r].name;
  const std::string header = call_header_text(names.data(), fr.genome.len.data(), n_refs);
  const int64_t n_text = (int64_t)header.size() + n_lines;
  // ---- the text
  std::deque<FileText> texts;
  if (want_text) {
    texts.emplace_back();
    FileText &t = texts.back();
    t.n = n_text;
    if (!alloc(t.d, t.n, "the text")) return PBSIM_FAILED;
    HIP_OK(hipMemcpyAsync(t.d.p, header.data(), header.size(), hipMemcpyHostToDevice, st));
    launch_call_line_fill(fr.pg, table, cls, fr.slots, tile, t.d.as<char>() + header.size(), st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("text");
  }
  std::vector<uint64_t> h_cells(kErrCells), h_pile(kPileCells), h_call(kCallCells), h_rec_n((size_t)n_refs);
  HIP_OK(hipMemcpyAsync(h_cells.data(), fr.d_cells.p, kErrCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_pile.data(), fr.d_pile.p, kPileCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_call.data(), d_call.p, kCallCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_rec_n.data(), d_rec_n.p, (size_t)n_refs * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (want_text && !deliver_text(st, kStage, texts, n_text, o.piece_bytes, sink->on_text, sink->user)) return PBSIM_FAILED;
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("deliver");
  if (sink && sink->on_record)
    for (int r = 0; r < n_refs; r++)
      if (!sink->on_record(sink->user, r, fr.genome.len[(size_t)r], (int64_t)h_rec_n[(size_t)r])) return fail("sink aborted (records)");
  // ---- what the caller is told
  for (int k = 0; k < kPileCounts; k++) result->counts[k] = (int64_t)h_cells[(size_t)kErrCellCounts + (size_t)k];
  for (int k = 0; k < kPileSites; k++) result->sites[k] = (int64_t)h_pile[(size_t)kPileCellSites + (size_t)k];
  result->ins_unanchored = (int64_t)h_pile[kPileCellUnanchored];
  result->max_depth = (int64_t)h_pile[kPileCellMaxDepth];
  result->variants = (int64_t)h_call[kCallCellVariants];
  for (int k = 0; k < kCallTypes; k++) result->types[k] = (int64_t)h_call[(size_t)kCallCellTypes + (size_t)k];
  result->ref_bases = (int64_t)h_call[kCallCellRefBases], result->alt_bases = (int64_t)h_call[kCallCellAltBases];
  result->longest_ref = (int64_t)h_call[kCallCellLongestRef], result->longest_alt = (int64_t)h_call[kCallCellLongestAlt];
  result->unplaced_records = (int64_t)h_call[kCallCellUnplacedRecords], result->unplaced_sites = (int64_t)h_call[kCallCellUnplacedSites];
  result->header_bytes = (int64_t)header.size();
  result->text_bytes = n_text;
  {
    char sum[400];
    snprintf(sum, sizeof sum,
             "%d genome records, %lld positions, %d files, %.1f MB inflated, %lld records, %lld segments, %lld log entries (%.1f MB), %lld ins_sites, "
             "%lld insertion cells, %lld variants, %.3f MB of text",
             n_refs, (long long)result->sites[kPsSites], n_files, fr.inflated / 1e6, (long long)fr.n_all, (long long)fr.segments, (long long)fr.logged,
             fr.logged * 8 / 1e6, (long long)fr.slots.n, (long long)fr.n_cells, (long long)result->variants, n_text / 1e6);
    ph.print(sum);
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_bam_call(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files,
                              const pbsim_call_opts *opts, const pbsim_call_sink *sink, pbsim_call_result *result) {
  using pbsim::fail;
  if (!c || !refs || n_refs < 1 || !files || n_files < 1 || !result) return fail("pbsim_bam_call: bad argument");
  for (int f = 0; f < n_files; f++)
    if (files[f].n < 0 || (files[f].n > 0 && !files[f].bam)) return fail("pbsim_bam_call: bad argument");
  pbsim_call_opts o;
  std::string err;
  if (!pbsim::call_check_opts(opts, &o, &err) || !pbsim::errors_check_genome(refs, n_refs, &err)) return fail("pbsim_bam_call: " + err);
  memset(result, 0, sizeof *result);
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::call_bam(c, refs, n_refs, files, n_files, o, sink, result);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
    memset(result, 0, sizeof *result);
  }
  return ok;
}
