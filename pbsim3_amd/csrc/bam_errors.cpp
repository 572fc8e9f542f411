// bam_errors.cpp -- pbsim_bam_errors: the error profile of the aligned reads of BAM files against their genome (the rule:
// include/pbsim3_amd.h, tests/errors_model.py).  The host's part: the genome into HBM (bam_genome.cpp), per file the front half
// it shares with the pileup and the consensus stages (bam_file_front.h: the stream, its records, the references by name, the
// record pass, the segments), here with the records' column counts, then the column pass, the reads and the text's way to the sink
// (bam_genome.cpp); the kernels are inflate.hip's, bam_scan.hip's and bam_errors.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "bam_errors.h"
#include "bam_file_front.h"
#include "bam_genome.h"
#include "bam_scan.h"
#include "bam_stream.h"
#include "ctx.h"
#include "kernels.h"

namespace pbsim {

namespace {

const char kWho[] = "pbsim_bam_errors: ";
const BamStage kStage = {kWho, "the stage holds the genome at 2 bytes per base, one file's inflated stream and 93 bytes per record in HBM at once, 101 with the text, and does not chunk"};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

int errors_bam(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files, const pbsim_errors_opts &o,
               const pbsim_errors_sink *sink, pbsim_errors_result *result) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "errors");
  const bool want_text = sink && sink->on_text;
  Genome genome;
  if (!load_genome(c, kStage, refs, n_refs, &genome)) return PBSIM_FAILED;
  ph.mark("genome");
  const ErrGenome g = {genome.seq.as<uint8_t>(), genome.hp.as<uint8_t>()};
  DevBuf d_cells;
  if (!alloc(d_cells, kErrCells * 8, "the counts")) return PBSIM_FAILED;
  unsigned long long *cells = d_cells.as<unsigned long long>();
  HIP_OK(hipMemsetAsync(d_cells.p, 0, kErrCells * 8, st));
  HIP_OK(hipMemsetAsync(cells + kErrCellFault, 0xff, 8, st));
  std::deque<FileText> texts;
  int64_t n_all = 0, inflated = 0, n_text = 0, segments = 0;
  for (int f = 0; f < n_files; f++) {
    // ---- 1. - 4. the stream, its records, its references by name, the record pass and the segments
    BamFileFront ff;
    if (!bam_file_front(c, kStage, ph, refs, n_refs, genome, files, f, n_files, o.exclude_flags, o.min_mapq, cells, true, &ff)) return PBSIM_FAILED;
    const int64_t n_rec = ff.n_rec;
    const ErrRecs &recs = ff.recs;
    inflated += ff.s.N, n_all += n_rec, segments += ff.n_seg;
    texts.emplace_back();
    if (n_rec == 0) continue;
    // ---- the segments' columns, into the records' column counts
    if (ff.n_seg > 0) {
      launch_errors_columns(recs, ff.er, g, ff.d_seg.as<ErrSegment>(), ff.n_seg, cells, st);
      HIP_OK(hipGetLastError());
      ph.mark("columns");
    }
    launch_errors_reads(recs, cells, st);
    HIP_OK(hipGetLastError());
    ph.mark("reads");
    // ---- 5. the text, while the names are here
    if (want_text) {
      DevBuf d_len;
      FileText &t = texts.back();
      if (!alloc(d_len, (n_rec + 1) * 8, "the lines' lengths")) return PBSIM_FAILED;
      int64_t *len = d_len.as<int64_t>();
      launch_errors_line_sizes(recs, len, st);
      HIP_OK(hipGetLastError());
      launch_exclusive_scan_i64(len, len, n_rec, ff.d_scan_tmp.as<int64_t>(), len + n_rec, st);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(&t.n, len + n_rec, 8, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      if (t.n > 0) {
        if (!alloc(t.d, t.n, "the text")) return PBSIM_FAILED;
        launch_errors_line_fill(recs, len, t.d.as<char>(), st);
        HIP_OK(hipGetLastError());
      }
      n_text += t.n;
      HIP_OK(hipStreamSynchronize(st));  // (d_len goes with this frame)
      ph.mark("text");
    }
    HIP_OK(hipStreamSynchronize(st));  // the stream and the per-record arrays go with this frame
  }
  std::vector<uint64_t> h_cells(kErrCells);
  HIP_OK(hipMemcpyAsync(h_cells.data(), d_cells.p, kErrCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (want_text && n_text > 0 && !deliver_text(st, kStage, texts, n_text, o.piece_bytes, sink->on_text, sink->user)) return PBSIM_FAILED;
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("deliver");
  // ---- what the caller is told
  const struct {
    int64_t *to;
    int from, n;
  } parts[] = {{result->counts, kErrCellCounts, kErrCounts},   {result->totals, kErrCellTotals, kErrTotals},
               {result->pair, kErrCellPair, kErrPair},         {result->hp_cols, kErrCellHpCols, kErrHp},
               {result->hp_sub, kErrCellHpSub, kErrHp},        {result->hp_del, kErrCellHpDel, kErrHp},
               {result->ins_len, kErrCellInsLen, kErrLenBins}, {result->del_len, kErrCellDelLen, kErrLenBins},
               {result->ins_base, kErrCellInsBase, kErrBases}, {result->del_base, kErrCellDelBase, kErrBases},
               {&result->qcal[0][0], kErrCellQcal, 3 * kErrQBins}, {result->hist_identity, kErrCellHistIdentity, kErrPpmBins}};
  for (const auto &p : parts)
    for (int k = 0; k < p.n; k++) p.to[k] = (int64_t)h_cells[(size_t)p.from + (size_t)k];
  errors_fit(result);
  {
    char sum[260];
    snprintf(sum, sizeof sum, "%d genome records, %d files, %.1f MB inflated, %lld records, %lld segments, %lld columns, %.1f MB of text", n_refs, n_files,
             inflated / 1e6, (long long)n_all, (long long)segments, (long long)result->totals[kErrCols], n_text / 1e6);
    ph.print(sum);
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_bam_errors(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files,
                                const pbsim_errors_opts *opts, const pbsim_errors_sink *sink, pbsim_errors_result *result) {
  using pbsim::fail;
  if (!c || !refs || n_refs < 1 || !files || n_files < 1 || !result) return fail("pbsim_bam_errors: bad argument");
  for (int f = 0; f < n_files; f++)
    if (files[f].n < 0 || (files[f].n > 0 && !files[f].bam)) return fail("pbsim_bam_errors: bad argument");
  pbsim_errors_opts o;
  std::string err;
  if (!pbsim::errors_check_opts(opts, &o, &err) || !pbsim::errors_check_genome(refs, n_refs, &err)) return fail("pbsim_bam_errors: " + err);
  memset(result, 0, sizeof *result);
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::errors_bam(c, refs, n_refs, files, n_files, o, sink, result);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
    memset(result, 0, sizeof *result);
  }
  return ok;
}
