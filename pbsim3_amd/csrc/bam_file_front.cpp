// bam_file_front.cpp -- bam_file_front (bam_file_front.h): the per-file first half that pbsim_bam_errors, pbsim_bam_pileup and
// pbsim_bam_consensus share.  The kernels are inflate.hip's, bam_scan.hip's and bam_errors.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bam_file_front.h"
#include "bam_scan.h"
#include "kernels.h"

namespace pbsim {

int bam_file_front(pbsim_ctx *c, const BamStage &stage, BamPhases &ph, const pbsim_errors_ref *refs, int n_refs, const Genome &genome,
                   const pbsim_errors_file *files, int f, int n_files, int32_t exclude_flags, int32_t min_mapq, unsigned long long *cells,
                   bool col_counts, BamFileFront *ff) {
  hipStream_t st = c->stream;
  auto alloc = [&](DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(stage, b, n, what); };
  // ---- 1. the stream into HBM, and its records
  BamStream &s = ff->s;
  s.a_what = "a file";
  if (n_files > 1) s.what = "file " + std::to_string(f);
  const std::string where = stage.who + s.what + (s.what.empty() ? "" : ": ");
  if (!bam_inflate_stream(c, stage, (const uint8_t *)files[f].bam, files[f].n, &s)) return PBSIM_FAILED;
  ph.mark("inflate");
  {
    BamScan scan;
    if (!bam_locate(c, stage, &s, &scan, kBamScanAny, kBamSamplePacking)) return PBSIM_FAILED;
  }
  ph.mark("locate");
  const int64_t n_rec = ff->n_rec = (int64_t)s.rec.size();
  if (n_rec >= ((int64_t)1 << 32) - 1) return fail(where + std::to_string(n_rec) + " records: a file of 2^32 - 1 records or more is not taken (a segment names its record in 32 bits)");
  // ---- 2. its references, by name
  std::vector<int32_t> map;
  {
    std::string err;
    if (!errors_ref_map(refs, n_refs, s.ref_names, files[f].ref_name, "file " + std::to_string(f), &map, &err)) return fail(stage.who + err);
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
  if (n_rec == 0) return PBSIM_SUCCEEDED;
  DevBuf &d_ref_at = ff->d_ref_at, &d_ref_len = ff->d_ref_len, &d_rec = ff->d_rec, &d_st = ff->d_st, &d_cig_at = ff->d_cig_at, &d_n_ops = ff->d_n_ops,
         &d_sums = ff->d_sums, &d_nm = ff->d_nm, &d_n_seg = ff->d_n_seg, &d_col = ff->d_col, &d_scan_tmp = ff->d_scan_tmp, &d_seg = ff->d_seg;
  if (!alloc(d_ref_at, (int64_t)ref_at.size() * 8, "the references' places") || !alloc(d_ref_len, (int64_t)ref_len.size() * 8, "the references' lengths") ||
      !alloc(d_rec, n_rec * 8, "the record list") || !alloc(d_st, n_rec, "the records' classes") || !alloc(d_cig_at, n_rec * 8, "the records' CIGARs") ||
      !alloc(d_n_ops, n_rec * 4, "the records' op counts") || !alloc(d_sums, n_rec * 32, "the records' CIGAR sums") ||
      !alloc(d_nm, n_rec * 8, "the records' NM values") || !alloc(d_n_seg, (n_rec + 1) * 8, "the records' segment counts") ||
      (col_counts && !alloc(d_col, n_rec * 24, "the records' column counts")) || !alloc(d_scan_tmp, (n_rec / 1024 + 8) * 8, "the scan's scratch"))
    return PBSIM_FAILED;
  HIP_OK(hipMemcpyAsync(d_ref_at.p, ref_at.data(), ref_at.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_ref_len.p, ref_len.data(), ref_len.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_rec.p, s.rec.data(), (size_t)n_rec * 8, hipMemcpyHostToDevice, st));
  if (col_counts) HIP_OK(hipMemsetAsync(d_col.p, 0, (size_t)n_rec * 24, st));
  HIP_OK(hipMemsetAsync(d_sums.p, 0, (size_t)n_rec * 32, st));
  HIP_OK(hipMemsetAsync(d_nm.p, 0, (size_t)n_rec * 8, st));
  const ErrRefs er = ff->er = {(int32_t)map.size(), d_ref_at.as<int64_t>(), d_ref_len.as<int64_t>()};
  const ErrRecs recs = ff->recs = {s.bytes(),
                                   d_rec.as<uint64_t>(),
                                   n_rec,
                                   d_st.as<uint8_t>(),
                                   d_cig_at.as<int64_t>(),
                                   d_n_ops.as<uint32_t>(),
                                   d_sums.as<int64_t>(),
                                   d_nm.as<int64_t>(),
                                   d_n_seg.as<int64_t>(),
                                   col_counts ? d_col.as<unsigned long long>() : nullptr};
  // ---- 3. the records
  launch_errors_records(recs, er, exclude_flags, min_mapq, nullptr, cells, st);
  HIP_OK(hipGetLastError());
  uint64_t fault = 0;
  HIP_OK(hipMemcpyAsync(&fault, cells + kErrCellFault, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("records");
  if (fault != ~(uint64_t)0)
    return fail(where + "the record at inflated byte offset " + std::to_string(fault) +
                " is malformed: a CIGAR op code above 8, or an aux field that runs past the record or has an unknown type");
  // ---- 4. the segments
  int64_t &n_seg = ff->n_seg;
  launch_exclusive_scan_i64(recs.n_seg, recs.n_seg, n_rec, d_scan_tmp.as<int64_t>(), recs.n_seg + n_rec, st);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(&n_seg, recs.n_seg + n_rec, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (n_seg > 0) {
    if (!alloc(d_seg, n_seg * (int64_t)sizeof(ErrSegment), "the segments")) return PBSIM_FAILED;
    launch_errors_records(recs, er, exclude_flags, min_mapq, d_seg.as<ErrSegment>(), cells, st);
    HIP_OK(hipGetLastError());
    ph.mark("segments");
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace pbsim
