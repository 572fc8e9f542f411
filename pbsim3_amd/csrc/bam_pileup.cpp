// bam_pileup.cpp -- pbsim_bam_pileup: the pileup of the aligned reads of BAM files against their genome (the rule:
// include/pbsim3_amd.h, tests/pileup_model.py).  The host's part has the flow of pbsim_bam_errors (bam_errors.cpp): the genome into
// HBM (bam_genome.cpp), the table zeroed, then per file the front half the three stages share (bam_file_front.h: its stream and
// records, the references by name, the record pass and the segments) and the column pass; then once the site pass, the text and
// its way to the sink; the kernels are inflate.hip's, bam_scan.hip's, bam_errors.hip's and bam_pileup.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "bam_genome.h"
#include "bam_pileup.h"
#include "bam_file_front.h"
#include "bam_scan.h"
#include "bam_stream.h"
#include "ctx.h"
#include "kernels.h"

namespace pbsim {

namespace {

const char kWho[] = "pbsim_bam_pileup: ";
const BamStage kStage = {kWho, "the stage holds the genome at 2 bytes per base, the cells at 32 bytes per position, a class byte per position, one file's inflated stream and 69 bytes per record in HBM at once, and the text, and does not chunk"};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

int pileup_bam(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files, const pbsim_pileup_opts &o,
               const pbsim_pileup_sink *sink, pbsim_pileup_result *result) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "pileup");
  const bool want_text = sink && sink->on_text, want_cells = sink && sink->on_cells;
  Genome genome;
  if (!load_genome(c, kStage, refs, n_refs, &genome)) return PBSIM_FAILED;
  ph.mark("genome");
  const ErrGenome g = {genome.seq.as<uint8_t>(), genome.hp.as<uint8_t>()};
  const int64_t total = genome.total;
  // the table shares the genome's offsets: 64 positions and more of padding lie behind every record
  DevBuf d_table, d_cls, d_cells, d_pile;
  if (!alloc(d_table, total * kPileWidth * 4, "the cells of every position") || !alloc(d_cls, total, "the sites' classes") ||
      !alloc(d_cells, kErrCells * 8, "the record counts") || !alloc(d_pile, kPileCells * 8, "the counts"))
    return PBSIM_FAILED;
  uint32_t *table = d_table.as<uint32_t>();
  unsigned long long *cells = d_cells.as<unsigned long long>(), *pile = d_pile.as<unsigned long long>();
  HIP_OK(hipMemsetAsync(d_table.p, 0, (size_t)total * kPileWidth * 4, st));
  HIP_OK(hipMemsetAsync(d_cells.p, 0, kErrCells * 8, st));
  HIP_OK(hipMemsetAsync(cells + kErrCellFault, 0xff, 8, st));
  HIP_OK(hipMemsetAsync(d_pile.p, 0, kPileCells * 8, st));
  ph.mark("zero");
  int64_t n_all = 0, inflated = 0, segments = 0;
  for (int f = 0; f < n_files; f++) {
    BamFileFront pf;
    if (!bam_file_front(c, kStage, ph, refs, n_refs, genome, files, f, n_files, o.exclude_flags, o.min_mapq, cells, false, &pf)) return PBSIM_FAILED;
    inflated += pf.s.N, n_all += pf.n_rec, segments += pf.n_seg;
    if (pf.n_seg > 0) {
      launch_pileup_columns(pf.recs, pf.er, g, pf.d_seg.as<ErrSegment>(), pf.n_seg, (uint32_t)o.min_baseq, table, pile, st);
      HIP_OK(hipGetLastError());
      ph.mark("columns");
    }
    HIP_OK(hipStreamSynchronize(st));  // the stream and the per-record arrays go with this frame
  }
  // ---- 5. the sites, once
  std::string names;
  std::vector<int64_t> name_at;
  for (int r = 0; r < n_refs; r++) {
    name_at.push_back((int64_t)names.size());
    names += refs[r].name;
  }
  name_at.push_back((int64_t)names.size());
  DevBuf d_at, d_len, d_name_at, d_names;
  if (!alloc(d_at, n_refs * 8, "the genome records' places") || !alloc(d_len, n_refs * 8, "the genome records' lengths") ||
      !alloc(d_name_at, (n_refs + 1) * 8, "the genome records' names") || !alloc(d_names, (int64_t)names.size() + 1, "the genome records' names"))
    return PBSIM_FAILED;
  HIP_OK(hipMemcpyAsync(d_at.p, genome.at.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_len.p, genome.len.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_name_at.p, name_at.data(), name_at.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, st));
  const PileGenome pg = {n_refs, total, d_at.as<int64_t>(), d_len.as<int64_t>(), d_name_at.as<int64_t>(), d_names.as<char>(), g.seq, g.hp};
  launch_pileup_sites(pg, table, o.min_depth, d_cls.as<uint8_t>(), pile, st);
  HIP_OK(hipGetLastError());
  ph.mark("sites");
  // ---- 6. the text
  std::deque<FileText> texts;
  int64_t n_text = 0;
  if (want_text) {
    const int64_t tiles = (total + kPileTile - 1) / kPileTile;
    DevBuf d_tile, d_scan_tmp;
    texts.emplace_back();
    FileText &t = texts.back();
    if (!alloc(d_tile, (tiles + 1) * 8, "the text's tiles") || !alloc(d_scan_tmp, (tiles / 1024 + 8) * 8, "the scan's scratch")) return PBSIM_FAILED;
    int64_t *tile = d_tile.as<int64_t>();
    launch_pileup_text_sizes(pg, table, d_cls.as<uint8_t>(), o.format, tile, st);
    HIP_OK(hipGetLastError());
    launch_exclusive_scan_i64(tile, tile, tiles, d_scan_tmp.as<int64_t>(), tile + tiles, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&t.n, tile + tiles, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (t.n > 0) {
      if (!alloc(t.d, t.n, "the text")) return PBSIM_FAILED;
      launch_pileup_text_fill(pg, table, d_cls.as<uint8_t>(), o.format, tile, t.d.as<char>(), st);
      HIP_OK(hipGetLastError());
    }
    n_text = t.n;
    HIP_OK(hipStreamSynchronize(st));  // (the tiles go with this frame)
    ph.mark("text");
  }
  std::vector<uint64_t> h_cells(kErrCells), h_pile(kPileCells);
  HIP_OK(hipMemcpyAsync(h_cells.data(), d_cells.p, kErrCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_pile.data(), d_pile.p, kPileCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (want_text && n_text > 0 && !deliver_text(st, kStage, texts, n_text, o.piece_bytes, sink->on_text, sink->user)) return PBSIM_FAILED;
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("deliver");
  if (want_cells) {
    std::vector<uint32_t> host;
    for (int r = 0; r < n_refs; r++) {
      const int64_t n = genome.len[(size_t)r] * kPileWidth;
      host.resize((size_t)std::max<int64_t>(n, 1));
      if (n > 0) HIP_OK(hipMemcpy(host.data(), table + genome.at[(size_t)r] * kPileWidth, (size_t)n * 4, hipMemcpyDeviceToHost));
      if (!sink->on_cells(sink->user, r, host.data(), genome.len[(size_t)r])) return fail("sink aborted (cells)");
    }
    ph.mark("cells");
  }
  // ---- what the caller is told
  const struct {
    int64_t *to;
    int from, n;
  } parts[] = {{result->sites, kPileCellSites, kPileSites},        {result->cell_sums, kPileCellSums, kPileWidth},
               {&result->ins_unanchored, kPileCellUnanchored, 1},  {&result->max_depth, kPileCellMaxDepth, 1},
               {result->hp_called, kPileCellHpCalled, kPileHp},    {result->hp_sub, kPileCellHpSub, kPileHp},
               {result->hp_del, kPileCellHpDel, kPileHp},          {result->hp_ins, kPileCellHpIns, kPileHp}};
  for (int k = 0; k < kPileCounts; k++) result->counts[k] = (int64_t)h_cells[(size_t)kErrCellCounts + (size_t)k];
  for (const auto &p : parts)
    for (int k = 0; k < p.n; k++) p.to[k] = (int64_t)h_pile[(size_t)p.from + (size_t)k];
  {
    char sum[300];
    snprintf(sum, sizeof sum, "%d genome records, %lld positions, %d files, %.1f MB inflated, %lld records, %lld segments, %lld columns, %.1f MB of text",
             n_refs, (long long)result->sites[kPsSites], n_files, inflated / 1e6, (long long)n_all, (long long)segments,
             (long long)(result->cell_sums[0] + result->cell_sums[1] + result->cell_sums[2] + result->cell_sums[3] + result->cell_sums[kPcOther] +
                         result->cell_sums[kPcDel] + result->cell_sums[kPcMasked]),
             n_text / 1e6);
    ph.print(sum);
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_bam_pileup(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files,
                                const pbsim_pileup_opts *opts, const pbsim_pileup_sink *sink, pbsim_pileup_result *result) {
  using pbsim::fail;
  if (!c || !refs || n_refs < 1 || !files || n_files < 1 || !result) return fail("pbsim_bam_pileup: bad argument");
  for (int f = 0; f < n_files; f++)
    if (files[f].n < 0 || (files[f].n > 0 && !files[f].bam)) return fail("pbsim_bam_pileup: bad argument");
  pbsim_pileup_opts o;
  std::string err;
  if (!pbsim::pileup_check_opts(opts, &o, &err) || !pbsim::errors_check_genome(refs, n_refs, &err)) return fail("pbsim_bam_pileup: " + err);
  memset(result, 0, sizeof *result);
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::pileup_bam(c, refs, n_refs, files, n_files, o, sink, result);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
    memset(result, 0, sizeof *result);
  }
  return ok;
}
