// bam_errors.cpp -- pbsim_bam_errors: the error profile of the aligned reads of BAM files against their genome (the rule:
// include/pbsim3_amd.h, tests/errors_model.py).  The host's part: the genome into HBM (bam_genome.cpp), each file's stream and
// its records (bam_stream.cpp), the references by name (bam_errors_rule.cpp), the buffers, and the text's way to the sink
// (bam_genome.cpp); the kernels are inflate.hip's, bam_scan.hip's and bam_errors.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "bam_errors.h"
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
    // ---- 1. the stream into HBM, and its records
    BamStream s;
    s.a_what = "a file";
    if (n_files > 1) s.what = "file " + std::to_string(f);
    const std::string where = kStage.who + s.what + (s.what.empty() ? "" : ": ");
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
    if (n_rec >= ((int64_t)1 << 32) - 1) return fail(where + std::to_string(n_rec) + " records: a file of 2^32 - 1 records or more is not taken (a segment names its record in 32 bits)");
    // ---- 2. its references, by name
    std::vector<int32_t> map;
    {
      std::string err;
      if (!errors_ref_map(refs, n_refs, s.ref_names, files[f].ref_name, "file " + std::to_string(f), &map, &err)) return fail(kWho + err);
    }
    std::vector<int64_t> ref_at(std::max<size_t>(map.size(), 1), -1), ref_len(std::max<size_t>(map.size(), 1), 0);
    for (size_t r = 0; r < map.size(); r++) {
      if (map[r] < 0) continue;
      const int64_t have = genome.len[(size_t)map[r]];
      if (s.hd.ref_len[r] != have)
        return fail(where + "the reference \"" + (files[f].ref_name ? std::string(files[f].ref_name) : s.ref_names[r]) + "\" has l_ref " +
                    std::to_string(s.hd.ref_len[r]) + " in the file's header, and the genome's record of that name has " + std::to_string(have) +
                    " bases: this is not the genome the reads were aligned to");
      ref_at[r] = genome.at[(size_t)map[r]];
      ref_len[r] = have;
    }
    texts.emplace_back();
    if (n_rec == 0) continue;
    DevBuf d_ref_at, d_ref_len, d_rec, d_st, d_cig_at, d_n_ops, d_sums, d_nm, d_n_seg, d_col, d_scan_tmp, d_seg;
    if (!alloc(d_ref_at, (int64_t)ref_at.size() * 8, "the references' places") || !alloc(d_ref_len, (int64_t)ref_len.size() * 8, "the references' lengths") ||
        !alloc(d_rec, n_rec * 8, "the record list") || !alloc(d_st, n_rec, "the records' classes") || !alloc(d_cig_at, n_rec * 8, "the records' CIGARs") ||
        !alloc(d_n_ops, n_rec * 4, "the records' op counts") || !alloc(d_sums, n_rec * 32, "the records' CIGAR sums") ||
        !alloc(d_nm, n_rec * 8, "the records' NM values") || !alloc(d_n_seg, (n_rec + 1) * 8, "the records' segment counts") ||
        !alloc(d_col, n_rec * 24, "the records' column counts") || !alloc(d_scan_tmp, (n_rec / 1024 + 8) * 8, "the scan's scratch"))
      return PBSIM_FAILED;
    HIP_OK(hipMemcpyAsync(d_ref_at.p, ref_at.data(), ref_at.size() * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_ref_len.p, ref_len.data(), ref_len.size() * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_rec.p, s.rec.data(), (size_t)n_rec * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_col.p, 0, (size_t)n_rec * 24, st));
    HIP_OK(hipMemsetAsync(d_sums.p, 0, (size_t)n_rec * 32, st));
    HIP_OK(hipMemsetAsync(d_nm.p, 0, (size_t)n_rec * 8, st));
    const ErrRefs er = {(int32_t)map.size(), d_ref_at.as<int64_t>(), d_ref_len.as<int64_t>()};
    const ErrRecs recs = {s.bytes(),
                          d_rec.as<uint64_t>(),
                          n_rec,
                          d_st.as<uint8_t>(),
                          d_cig_at.as<int64_t>(),
                          d_n_ops.as<uint32_t>(),
                          d_sums.as<int64_t>(),
                          d_nm.as<int64_t>(),
                          d_n_seg.as<int64_t>(),
                          d_col.as<unsigned long long>()};
    // ---- 3. the records
    launch_errors_records(recs, er, o.exclude_flags, o.min_mapq, nullptr, cells, st);
    HIP_OK(hipGetLastError());
    uint64_t fault = 0;
    HIP_OK(hipMemcpyAsync(&fault, cells + kErrCellFault, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("records");
    if (fault != ~(uint64_t)0)
      return fail(where + "the record at inflated byte offset " + std::to_string(fault) +
                  " is malformed: a CIGAR op code above 8, or an aux field that runs past the record or has an unknown type");
    // ---- 4. the segments and their columns
    int64_t n_seg = 0;
    launch_exclusive_scan_i64(recs.n_seg, recs.n_seg, n_rec, d_scan_tmp.as<int64_t>(), recs.n_seg + n_rec, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&n_seg, recs.n_seg + n_rec, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    segments += n_seg;
    if (n_seg > 0) {
      if (!alloc(d_seg, n_seg * (int64_t)sizeof(ErrSegment), "the segments")) return PBSIM_FAILED;
      launch_errors_records(recs, er, o.exclude_flags, o.min_mapq, d_seg.as<ErrSegment>(), cells, st);
      HIP_OK(hipGetLastError());
      ph.mark("segments");
      launch_errors_columns(recs, er, g, d_seg.as<ErrSegment>(), n_seg, cells, st);
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
      launch_exclusive_scan_i64(len, len, n_rec, d_scan_tmp.as<int64_t>(), len + n_rec, st);
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
