// bam_stats.cpp -- pbsim_bam_stats: a summary of the reads of one or more BAM files (the rule: include/pbsim3_amd.h,
// tests/stats_model.py).  The host's part: each file's stream into HBM and its records (bam_stream.cpp), the buffers, the
// lengths kept from file to file, and the text's way to the sink; the kernels are inflate.hip's, bam_scan.hip's, rocPRIM's sort
// and scan and bam_stats.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "bam_scan.h"
#include "bam_stats.h"
#include "bam_stream.h"
#include "ctx.h"
#include "kernels.h"

namespace pbsim {

namespace {

const char kWho[] = "pbsim_bam_stats: ";
const BamStage kStage = {kWho, "the stage holds one file's inflated stream and 45 bytes per record in HBM at once, 93 with the text, and does not chunk"};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

struct FileText {
  DevBuf d;
  int64_t n = 0;
};

int stats_bam(pbsim_ctx *c, const pbsim_stats_file *files, int n_files, const pbsim_stats_opts &o, const pbsim_stats_sink *sink,
              int64_t counts[kStatsCounts], int64_t len_row[kStatsLenRow], int64_t totals[kStatsTotals], int64_t hist_q[kStatsQBins],
              int64_t hist_identity[kStatsPpmBins], int64_t hist_qacc[kStatsPpmBins]) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "stats");
  const bool want_text = sink && sink->on_text;
  DevBuf d_cells, d_e;
  if (!alloc(d_cells, kStatsCells * 8, "the counts") || !alloc(d_e, kStatsQBins * 8, "the table of error probabilities")) return PBSIM_FAILED;
  unsigned long long *cells = d_cells.as<unsigned long long>();
  HIP_OK(hipMemsetAsync(d_cells.p, 0, kStatsCells * 8, st));
  HIP_OK(hipMemsetAsync(cells + kStatsCellFault, 0xff, 8, st));
  HIP_OK(hipMemsetAsync(cells + kStatsCellLenMin, 0xff, 8, st));
  HIP_OK(hipMemcpyAsync(d_e.p, kStatsE, kStatsQBins * 8, hipMemcpyHostToDevice, st));
  std::deque<DevBuf> lengths;  // per file: l_seq of the records that take part in the lengths, 0 for the others
  std::vector<int64_t> file_recs;
  std::deque<FileText> texts;
  int64_t n_all = 0, inflated = 0, n_text = 0, quality_bytes = 0;
  for (int f = 0; f < n_files; f++) {
    // ---- 1. the stream into HBM, and its records
    BamStream s;
    s.a_what = "a file";
    if (n_files > 1) s.what = "file " + std::to_string(f);
    if (!bam_inflate_stream(c, kStage, (const uint8_t *)files[f].bam, files[f].n, &s)) return PBSIM_FAILED;
    ph.mark("inflate");
    {
      BamScan scan;
      if (!bam_locate(c, kStage, &s, &scan, kBamScanAny, kBamSamplePacking)) return PBSIM_FAILED;
    }
    ph.mark("locate");
    const int64_t n_rec = (int64_t)s.rec.size();
    inflated += s.N;
    n_all += n_rec;
    if (n_all >= (int64_t)1 << 31)
      return fail(std::string(kWho) + std::to_string(n_all) + " records: 2^31 records or more in total are not taken (the sums of the lengths' squares are two 64-bit cells)");
    lengths.emplace_back();
    file_recs.push_back(n_rec);
    texts.emplace_back();
    if (n_rec == 0) continue;
    // ---- 2. the records
    DevBuf d_rec, d_st, d_qoff, d_qlen, d_qsum, d_cig, d_nm, d_scan_tmp;
    if (!alloc(d_rec, n_rec * 8, "the record list") || !alloc(d_st, n_rec, "the records' classes") ||
        !alloc(d_qoff, n_rec * 8, "the quality fields' offsets") || !alloc(d_qlen, (n_rec + 1) * 8, "the quality fields' lengths") ||
        !alloc(d_qsum, n_rec * 16, "the reads' quality sums") || !alloc(lengths.back(), n_rec * 4, "the reads' lengths") ||
        !alloc(d_scan_tmp, (n_rec / 1024 + 8) * 8, "the scan's scratch") ||
        (want_text && (!alloc(d_cig, n_rec * 32, "the records' CIGAR sums") || !alloc(d_nm, n_rec * 8, "the records' NM values"))))
      return PBSIM_FAILED;
    HIP_OK(hipMemcpyAsync(d_rec.p, s.rec.data(), (size_t)n_rec * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_qsum.p, 0, (size_t)n_rec * 16, st));
    if (want_text) {
      HIP_OK(hipMemsetAsync(d_cig.p, 0, (size_t)n_rec * 32, st));
      HIP_OK(hipMemsetAsync(d_nm.p, 0, (size_t)n_rec * 8, st));
    }
    const StatsRecs recs = {s.bytes(),
                            d_rec.as<uint64_t>(),
                            n_rec,
                            d_st.as<uint8_t>(),
                            d_qoff.as<int64_t>(),
                            d_qlen.as<int64_t>(),
                            d_qsum.as<unsigned long long>(),
                            lengths.back().as<uint32_t>(),
                            want_text ? d_cig.as<int64_t>() : nullptr,
                            want_text ? d_nm.as<int64_t>() : nullptr};
    launch_stats_records(recs, o.exclude_flags, o.min_mapq, cells, st);
    HIP_OK(hipGetLastError());
    uint64_t fault = 0;
    HIP_OK(hipMemcpyAsync(&fault, cells + kStatsCellFault, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("records");
    if (fault != ~(uint64_t)0)
      return fail(kStage.who + s.what + (s.what.empty() ? "" : ": ") + "the record at inflated byte offset " + std::to_string(fault) +
                  " is malformed: a CIGAR op code above 8, or an aux field that runs past the record or has an unknown type");
    // ---- 3. the quality bytes
    int64_t n_bytes = 0;
    launch_exclusive_scan_i64(recs.qlen, recs.qlen, n_rec, d_scan_tmp.as<int64_t>(), recs.qlen + n_rec, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&n_bytes, recs.qlen + n_rec, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    launch_stats_quals(recs, n_bytes, d_e.as<unsigned long long>(), cells, st);
    HIP_OK(hipGetLastError());
    quality_bytes += n_bytes;
    ph.mark("quals");
    launch_stats_reads(recs, cells, st);
    HIP_OK(hipGetLastError());
    ph.mark("reads");
    // ---- 4. the text, while the names are here
    if (want_text) {
      DevBuf d_len;
      FileText &t = texts.back();
      if (!alloc(d_len, (n_rec + 1) * 8, "the lines' lengths")) return PBSIM_FAILED;
      int64_t *len = d_len.as<int64_t>();
      launch_stats_line_sizes(recs, len, st);
      HIP_OK(hipGetLastError());
      launch_exclusive_scan_i64(len, len, n_rec, d_scan_tmp.as<int64_t>(), len + n_rec, st);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(&t.n, len + n_rec, 8, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      if (t.n > 0) {
        if (!alloc(t.d, t.n, "the text")) return PBSIM_FAILED;
        launch_stats_line_fill(recs, len, t.d.as<char>(), st);
        HIP_OK(hipGetLastError());
      }
      n_text += t.n;
      HIP_OK(hipStreamSynchronize(st));  // (d_len goes with this frame)
      ph.mark("text");
    }
    HIP_OK(hipStreamSynchronize(st));  // the stream and the per-record arrays go with this frame
  }
  // ---- 5. the lengths of all files: sorted, their running sums, the median and the Nx
  std::vector<uint64_t> h_cells(kStatsCells);
  HIP_OK(hipMemcpyAsync(h_cells.data(), d_cells.p, kStatsCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  const int64_t n = (int64_t)h_cells[kStatsCellLenN];
  const uint64_t bases = h_cells[kStatsCellLenBases];
  int64_t nx[10] = {0};
  if (n > 0) {
    DevBuf d_in, d_sorted, d_sums, d_tmp, d_nx;
    if (!alloc(d_in, n_all * 4, "the lengths") || !alloc(d_sorted, n_all * 4, "the sorted lengths") || !alloc(d_sums, n_all * 8, "the lengths' running sums") ||
        !alloc(d_nx, 80, "the median and the Nx"))
      return PBSIM_FAILED;
    int64_t at = 0;
    for (size_t f = 0; f < file_recs.size(); at += file_recs[f], f++)
      if (file_recs[f]) HIP_OK(hipMemcpyAsync(d_in.as<uint32_t>() + at, lengths[f].p, (size_t)file_recs[f] * 4, hipMemcpyDeviceToDevice, st));
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_OK(stats_sort_lengths(nullptr, &sort_bytes, d_in.as<uint32_t>(), d_sorted.as<uint32_t>(), n_all, st));
    HIP_OK(stats_scan_lengths(nullptr, &scan_bytes, d_sorted.as<uint32_t>(), d_sums.as<unsigned long long>(), n_all, st));
    if (!alloc(d_tmp, (int64_t)std::max(sort_bytes, scan_bytes), "the sort's scratch")) return PBSIM_FAILED;
    HIP_OK(stats_sort_lengths(d_tmp.p, &sort_bytes, d_in.as<uint32_t>(), d_sorted.as<uint32_t>(), n_all, st));
    HIP_OK(stats_scan_lengths(d_tmp.p, &scan_bytes, d_sorted.as<uint32_t>(), d_sums.as<unsigned long long>(), n_all, st));
    launch_stats_nx(d_sorted.as<uint32_t>(), d_sums.as<unsigned long long>(), n_all, n, bases, d_nx.as<int64_t>(), st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(nx, d_nx.p, 80, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  }
  lengths.clear();
  ph.mark("lengths");
  // ---- what the caller is told
  for (int k = 0; k < kStatsCounts; k++) counts[k] = (int64_t)h_cells[(size_t)kStatsCellCounts + (size_t)k];
  for (int k = 0; k < kStatsTotals; k++) totals[k] = (int64_t)h_cells[(size_t)kStatsCellTotals + (size_t)k];
  for (int k = 0; k < kStatsQBins; k++) hist_q[k] = (int64_t)h_cells[(size_t)kStatsCellHistQ + (size_t)k];
  for (int k = 0; k < kStatsPpmBins; k++) hist_identity[k] = (int64_t)h_cells[(size_t)kStatsCellHistIdentity + (size_t)k];
  for (int k = 0; k < kStatsPpmBins; k++) hist_qacc[k] = (int64_t)h_cells[(size_t)kStatsCellHistQacc + (size_t)k];
  if (n > 0) {
    len_row[kStatsLenN] = n;
    len_row[kStatsLenBases] = (int64_t)bases;
    len_row[kStatsLenMin] = (int64_t)h_cells[kStatsCellLenMin];
    len_row[kStatsLenMax] = (int64_t)h_cells[kStatsCellLenMax];
    len_row[kStatsLenMean] = stats_muldiv(bases, 1000, (uint64_t)n);
    len_row[kStatsLenSd] = stats_length_sd((uint64_t)n, bases, h_cells[kStatsCellSqLo], h_cells[kStatsCellSqHi]);
    len_row[kStatsLenMedian] = nx[0];
    for (int k = 1; k <= 9; k++) len_row[kStatsLenN10 + k - 1] = nx[k];
  }
  if (want_text && n_text > 0) {
    // two pinned pieces: one on its way to the host while the sink has the other.  A piece does not cross from one file's text
    // into the next one's buffer, so it may be shorter than piece_bytes there.
    const int64_t piece = std::min(o.piece_bytes, n_text);
    HostBuf pinned[2];
    hipEvent_t done[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; k++) {
      if (pinned[k].ensure((size_t)piece) != hipSuccess) {
        (void)hipGetLastError();
        return fail(std::string(kWho) + "no pinned host memory for a piece of " + std::to_string(piece) + " bytes of text");
      }
    }
    struct Events {
      hipEvent_t *e;
      ~Events() {
        for (int k = 0; k < 2; k++)
          if (e[k]) (void)hipEventDestroy(e[k]);
      }
    } guard = {done};
    for (int k = 0; k < 2; k++) HIP_OK(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
    // the pieces: (file, offset in its text, bytes)
    struct Piece {
      size_t f;
      int64_t at, n;
    };
    std::vector<Piece> pieces;
    for (size_t f = 0; f < texts.size(); f++)
      for (int64_t at = 0; at < texts[f].n; at += piece) pieces.push_back({f, at, std::min(piece, texts[f].n - at)});
    auto start_copy = [&](const Piece &p, int which) {
      hipError_t e = hipMemcpyAsync(pinned[which].p, texts[p.f].d.as<char>() + p.at, (size_t)p.n, hipMemcpyDeviceToHost, st);
      return e != hipSuccess ? e : hipEventRecord(done[which], st);
    };
    HIP_OK(start_copy(pieces[0], 0));
    int64_t offset = 0;
    for (size_t k = 0; k < pieces.size(); k++) {
      const int which = (int)(k & 1);
      if (k + 1 < pieces.size()) HIP_OK(start_copy(pieces[k + 1], which ^ 1));
      HIP_OK(hipEventSynchronize(done[which]));
      if (!sink->on_text(sink->user, (const char *)pinned[which].p, pieces[k].n, offset)) return fail("sink aborted (text)");
      offset += pieces[k].n;
    }
  }
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("deliver");
  {
    char sum[240];
    snprintf(sum, sizeof sum, "%d files, %.1f MB inflated, %lld records, %lld quality bytes, %.1f MB of text", n_files, inflated / 1e6, (long long)n_all,
             (long long)quality_bytes, n_text / 1e6);
    ph.print(sum);
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_bam_stats(pbsim_ctx *c, const pbsim_stats_file *files, int n_files, const pbsim_stats_opts *opts,
                               const pbsim_stats_sink *sink, int64_t counts[10], int64_t len_row[16], int64_t totals[12], int64_t hist_q[128],
                               int64_t hist_identity[1001], int64_t hist_qacc[1001]) {
  using pbsim::fail;
  if (!c || !files || n_files < 1 || !counts || !len_row || !totals || !hist_q || !hist_identity || !hist_qacc)
    return fail("pbsim_bam_stats: bad argument");
  for (int f = 0; f < n_files; f++)
    if (files[f].n < 0 || (files[f].n > 0 && !files[f].bam)) return fail("pbsim_bam_stats: bad argument");
  pbsim_stats_opts o;
  std::string err;
  if (!pbsim::stats_check_opts(opts, &o, &err)) return fail("pbsim_bam_stats: " + err);
  memset(counts, 0, 10 * sizeof(int64_t));
  memset(len_row, 0, 16 * sizeof(int64_t));
  memset(totals, 0, 12 * sizeof(int64_t));
  memset(hist_q, 0, 128 * sizeof(int64_t));
  memset(hist_identity, 0, 1001 * sizeof(int64_t));
  memset(hist_qacc, 0, 1001 * sizeof(int64_t));
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::stats_bam(c, files, n_files, o, sink, counts, len_row, totals, hist_q, hist_identity, hist_qacc);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
  }
  return ok;
}
