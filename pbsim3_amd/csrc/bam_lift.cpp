// bam_lift.cpp -- pbsim_bam_lift: the aligned records of a BAM that lie on a variant genome, placed on the original genome (the
// rule: include/pbsim3_amd.h, tests/lift_model.py).  The host's part: the original genome into HBM (bam_genome.cpp); the stream
// and its records (bam_stream.cpp); the references by name (bam_errors_rule.cpp) with the l_ref check against the origin maps --
// which is why this stage does not go through bam_file_front: that checks l_ref against the genome's records, and makes segments
// this stage has no use for --; the origin maps beside the genome, their max-scan and rule 2; the record pass of bam_errors.hip
// for the resolved CIGARs; the span, the runs counted, the scan of the op counts, the runs written; the sizes, their scan, the
// records written; the header rewritten here, and the lifted stream through the sort stage's deflate lanes to the sink.  The
// kernels are inflate.hip's, bam_scan.hip's, bam_errors.hip's, bam_lift.hip's and deflate.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bam_errors.h"
#include "bam_genome.h"
#include "bam_lift.h"
#include "bam_scan.h"
#include "bam_stream.h"
#include "ctx.h"
#include "engine_internal.h"
#include "inflate_host.h"
#include "kernels.h"

namespace pbsim {

namespace {

const char kWho[] = "pbsim_bam_lift: ";
const BamStage kStage = {kWho, "the stage holds the inflated stream, the lifted stream, their compressed pieces, the genome at 2 bytes per base, 8 bytes per variant base, 4 bytes per lifted op and 181 bytes per record in HBM at once, and does not chunk"};
const unsigned char kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

int lift_bam(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_lift_origin *origins, const pbsim_errors_file *file,
             const pbsim_lift_sink *sink, pbsim_lift_result *result) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "lift");
  Genome genome;
  if (!load_genome(c, kStage, refs, n_refs, &genome)) return PBSIM_FAILED;
  ph.mark("genome");
  // ---- 1. the stream into HBM, its records, its references by name
  BamStream s;
  s.a_what = "a file";
  if (!bam_inflate_stream(c, kStage, (const uint8_t *)file->bam, file->n, &s)) return PBSIM_FAILED;
  ph.mark("inflate");
  {
    BamScan scan;
    if (!bam_locate(c, kStage, &s, &scan, kBamScanAny, kBamSamplePacking)) return PBSIM_FAILED;
  }
  ph.mark("locate");
  const int64_t n_rec = (int64_t)s.rec.size(), n_file_refs = (int64_t)s.ref_names.size();
  std::vector<int32_t> map;
  {
    std::string err;
    if (!errors_ref_map(refs, n_refs, s.ref_names, file->ref_name, "the file", &map, &err)) return fail(kWho + err);
  }
  std::vector<int64_t> new_len((size_t)n_file_refs);
  for (size_t r = 0; r < map.size(); r++) {
    const std::string name = file->ref_name ? std::string(file->ref_name) : s.ref_names[r];
    if (map[r] < 0) return fail(kWho + ("the genome has no record named \"" + name + "\""));
    const int64_t have = origins[map[r]].n;
    if (s.hd.ref_len[r] != have)
      return fail(kWho + ("the reference \"" + name + "\" has l_ref " + std::to_string(s.hd.ref_len[r]) +
                          " in the file's header, and the origin map of the genome's record of that name has " + std::to_string(have) +
                          " bases: this is not the genome these reads came from"));
    new_len[r] = genome.len[(size_t)map[r]];
  }
  DevBuf d_cells, d_err_cells;
  if (!alloc(d_cells, kLiftCells * 8, "the counts") || !alloc(d_err_cells, kErrCells * 8, "the record pass's counts")) return PBSIM_FAILED;
  unsigned long long *cells = d_cells.as<unsigned long long>(), *err_cells = d_err_cells.as<unsigned long long>();
  HIP_OK(hipMemsetAsync(d_cells.p, 0, kLiftCells * 8, st));
  HIP_OK(hipMemsetAsync(cells + kLiftCellFault, 0xff, 16, st));  // the fault cell and the origin cell
  HIP_OK(hipMemsetAsync(d_err_cells.p, 0, kErrCells * 8, st));
  HIP_OK(hipMemsetAsync(err_cells + kErrCellFault, 0xff, 8, st));
  // ---- 2. the origin maps of the genome records the file names, beside the genome; the max-scan of the kept values; rule 2
  std::vector<int64_t> origin_at((size_t)n_refs, -1);  // in int32 units
  int64_t origin_total = 0, longest = 0;
  for (int32_t g : map)
    if (origin_at[(size_t)g] < 0) {
      origin_at[(size_t)g] = origin_total;
      origin_total += (origins[g].n + 63) / 64 * 64;
      longest = std::max(longest, origins[g].n);
    }
  DevBuf d_origin, d_kept_max, d_kept, d_scan_tmp;
  if (!alloc(d_origin, origin_total * 4, "the origin maps") || !alloc(d_kept_max, origin_total * 4, "the origin maps' kept values scanned") ||
      !alloc(d_kept, longest * 4, "the origin maps' kept values"))
    return PBSIM_FAILED;
  for (int g = 0; g < n_refs; g++) {
    const int64_t n = origins[g].n;
    if (origin_at[(size_t)g] < 0 || n == 0) continue;
    int32_t *o = d_origin.as<int32_t>() + origin_at[(size_t)g], *km = d_kept_max.as<int32_t>() + origin_at[(size_t)g];
    HIP_OK(hipMemcpyAsync(o, origins[g].origin, (size_t)n * 4, hipMemcpyHostToDevice, st));
    launch_lift_kept(o, n, d_kept.as<int32_t>(), st);
    HIP_OK(hipGetLastError());
    size_t tb = 0;
    HIP_OK(lift_max_scan(nullptr, &tb, d_kept.as<int32_t>(), km, n, st));
    if (!alloc(d_scan_tmp, (int64_t)tb, "the scan's scratch")) return PBSIM_FAILED;
    HIP_OK(lift_max_scan(d_scan_tmp.p, &tb, d_kept.as<int32_t>(), km, n, st));
    launch_lift_check(o, km, n, genome.len[(size_t)g], cells, st);
    HIP_OK(hipGetLastError());
    uint64_t bad = 0;
    HIP_OK(hipMemcpyAsync(&bad, cells + kLiftCellOrigin, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));  // (d_scan_tmp is sized anew for the next map)
    if (bad != ~(uint64_t)0)
      return fail(kWho + ("the origin map of \"" + std::string(refs[g].name) + "\" is not one: variant position " + std::to_string(bad >> 2) + ": " +
                          lift_origin_fault((int)(bad & 3))));
  }
  d_kept.release();
  ph.mark("origin");
  // ---- the header, rewritten
  std::vector<uint8_t> hbytes((size_t)s.H);
  if (s.H) HIP_OK(hipMemcpy(hbytes.data(), s.d.p, (size_t)s.H, hipMemcpyDeviceToHost));
  const std::string head = lift_header(hbytes.data(), s.H, s.hd.l_text, s.ref_names, new_len);
  // ---- 3. the records: classes and resolved CIGARs (bam_errors.hip), then the span, the runs, the sizes and the records
  DevBuf d_out;
  int64_t total = 0, n_ops_total = 0;
  if (n_rec > 0) {
    if (n_rec >= ((int64_t)1 << 32) - 1) return fail(kWho + (std::to_string(n_rec) + " records: a file of 2^32 - 1 records or more is not taken"));
    std::vector<int64_t> zero_at((size_t)std::max<int64_t>(n_file_refs, 1), 0), var_len((size_t)std::max<int64_t>(n_file_refs, 1), 0);
    std::vector<LiftRef> lrefs((size_t)std::max<int64_t>(n_file_refs, 1));
    for (size_t r = 0; r < map.size(); r++) {
      const int32_t g = map[r];
      var_len[r] = origins[g].n;
      lrefs[r] = LiftRef{d_origin.as<int32_t>() + origin_at[(size_t)g], d_kept_max.as<int32_t>() + origin_at[(size_t)g], origins[g].n,
                         genome.len[(size_t)g], genome.at[(size_t)g]};
    }
    DevBuf d_ref_at, d_ref_len, d_lrefs, d_rec, d_st, d_cig_at, d_n_ops, d_sums, d_nm, d_n_seg, d_lr, d_n_out, d_cig, d_size;
    if (!alloc(d_ref_at, (int64_t)zero_at.size() * 8, "the references' places") || !alloc(d_ref_len, (int64_t)var_len.size() * 8, "the references' lengths") ||
        !alloc(d_lrefs, (int64_t)(lrefs.size() * sizeof(LiftRef)), "the references' maps") || !alloc(d_rec, n_rec * 8, "the record list") ||
        !alloc(d_st, n_rec, "the records' classes") || !alloc(d_cig_at, n_rec * 8, "the records' CIGARs") ||
        !alloc(d_n_ops, n_rec * 4, "the records' op counts") || !alloc(d_sums, n_rec * 32, "the records' CIGAR sums") ||
        !alloc(d_nm, n_rec * 8, "the records' NM values") || !alloc(d_n_seg, (n_rec + 1) * 8, "the records' segment counts") ||
        !alloc(d_lr, n_rec * (int64_t)sizeof(LiftRec), "the records' lifted places") || !alloc(d_n_out, (n_rec + 1) * 8, "the lifted op counts") ||
        !alloc(d_size, (n_rec + 1) * 8, "the lifted sizes") || !alloc(d_scan_tmp, (n_rec / 1024 + 8) * 8, "the scan's scratch"))
      return PBSIM_FAILED;
    HIP_OK(hipMemcpyAsync(d_ref_at.p, zero_at.data(), zero_at.size() * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_ref_len.p, var_len.data(), var_len.size() * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_lrefs.p, lrefs.data(), lrefs.size() * sizeof(LiftRef), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_rec.p, s.rec.data(), (size_t)n_rec * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_sums.p, 0, (size_t)n_rec * 32, st));
    HIP_OK(hipMemsetAsync(d_nm.p, 0, (size_t)n_rec * 8, st));
    const ErrRefs er = {(int32_t)n_file_refs, d_ref_at.as<int64_t>(), d_ref_len.as<int64_t>()};
    const ErrRecs recs = {s.bytes(), d_rec.as<uint64_t>(), n_rec, d_st.as<uint8_t>(), d_cig_at.as<int64_t>(), d_n_ops.as<uint32_t>(),
                          d_sums.as<int64_t>(), d_nm.as<int64_t>(), d_n_seg.as<int64_t>(), nullptr};
    const ErrGenome g = {genome.seq.as<uint8_t>(), genome.hp.as<uint8_t>()};
    const LiftRef *d_refs = d_lrefs.as<LiftRef>();
    LiftRec *lr = d_lr.as<LiftRec>();
    uint64_t fault = 0;
    auto malformed = [&](uint64_t at, const char *why) {
      return fail(kWho + ("the record at inflated byte offset " + std::to_string(at) + " is malformed: " + why));
    };
    launch_errors_records(recs, er, 0, 0, nullptr, err_cells, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&fault, err_cells + kErrCellFault, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("records");
    if (fault != ~(uint64_t)0) return malformed(fault, "a CIGAR op code above 8, or an aux field that runs past the record or has an unknown type");
    launch_lift_span(recs, d_refs, lr, cells, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&fault, cells + kLiftCellFault, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("span");
    if (fault != ~(uint64_t)0) return malformed(fault, "its CIGAR runs past its reference, or its query length is not l_seq");
    int64_t *n_out = d_n_out.as<int64_t>(), *size = d_size.as<int64_t>();
    launch_lift_runs(recs, d_refs, g, lr, n_out, nullptr, nullptr, cells, st);
    HIP_OK(hipGetLastError());
    launch_exclusive_scan_i64(n_out, n_out, n_rec, d_scan_tmp.as<int64_t>(), n_out + n_rec, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&n_ops_total, n_out + n_rec, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("runs counted");
    if (!alloc(d_cig, n_ops_total * 4 + 64, "the lifted CIGARs")) return PBSIM_FAILED;
    HIP_OK(hipMemsetAsync(d_cig.p, 0, (size_t)(n_ops_total * 4 + 64), st));
    launch_lift_runs(recs, d_refs, g, lr, n_out, n_out, d_cig.as<uint32_t>(), cells, st);
    HIP_OK(hipGetLastError());
    ph.mark("runs written");
    launch_lift_sizes(recs, lr, size, cells, st);
    HIP_OK(hipGetLastError());
    launch_exclusive_scan_i64(size, size, n_rec, d_scan_tmp.as<int64_t>(), size + n_rec, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&total, size + n_rec, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(&fault, cells + kLiftCellFault, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("sizes");
    if (fault != ~(uint64_t)0) return malformed(fault, "an aux field that runs past the record or has an unknown type");
    if (!alloc(d_out, total + 64, "the lifted stream")) return PBSIM_FAILED;
    launch_lift_write(recs, lr, n_out, d_cig.as<uint32_t>(), size, d_out.as<uint8_t>(), cells, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));  // the per-record arrays go with this frame
    ph.mark("write");
  }
  s.d.release();  // the input stream has been read for the last time
  std::vector<uint64_t> h_cells(kLiftCells);
  HIP_OK(hipMemcpy(h_cells.data(), d_cells.p, kLiftCells * 8, hipMemcpyDeviceToHost));
  // ---- 5. the header in members of its own, the lifted records through the deflate lanes, the EOF block
  std::vector<char> hz((size_t)pbsim_deflate_bound((int64_t)head.size()) + 64);
  int64_t hz_bytes = 0, at = 0;
  if (!pbsim_deflate_buffer(c, head.data(), (int64_t)head.size(), hz.data(), (int64_t)hz.size(), &hz_bytes)) return PBSIM_FAILED;
  auto send = [&](const char *z, int64_t k) -> int {
    if (k > 0 && sink->on_bam && !sink->on_bam(sink->user, z, k, at)) return fail("sink aborted (lifted BAM)");
    at += k;
    return PBSIM_SUCCEEDED;
  };
  if (!send(hz.data(), hz_bytes)) return PBSIM_FAILED;
  if (total > 0 && !deflate_pieces(c, c->slots[0].df[0], d_out.as<uint8_t>(), total, [&](const char *z, int64_t k) -> int { return send(z, k); }))
    return PBSIM_FAILED;
  if (!send((const char *)kEof, sizeof kEof)) return PBSIM_FAILED;
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("deflate and deliver");
  for (int k = 0; k < kLiftCounts; k++) result->counts[k] = (int64_t)h_cells[(size_t)(kLiftCellCounts + k)];
  for (int k = 0; k < kLiftTotals; k++) result->totals[k] = (int64_t)h_cells[(size_t)(kLiftCellTotals + k)];
  result->counts[kLiftRecords] = n_rec;
  {
    char sum[260];
    snprintf(sum, sizeof sum, "%d genome records, %.1f MB inflated, %lld records, %lld lifted, %lld columns, %lld ops, %.1f MB lifted", n_refs, s.N / 1e6,
             (long long)n_rec, (long long)result->counts[kLiftLifted], (long long)result->totals[kLiftColsIn], (long long)n_ops_total, total / 1e6);
    ph.print(sum);
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_bam_lift(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_lift_origin *origins, const pbsim_errors_file *file,
                              const pbsim_lift_sink *sink, pbsim_lift_result *result) {
  using pbsim::fail;
  if (!c || !refs || !result) return fail("pbsim_bam_lift: bad argument");
  std::string err;
  if (!pbsim::lift_check_args(origins, n_refs, file, sink, &err) || !pbsim::errors_check_genome(refs, n_refs, &err)) return fail("pbsim_bam_lift: " + err);
  memset(result, 0, sizeof *result);
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::lift_bam(c, refs, n_refs, origins, file, sink, result);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
    memset(result, 0, sizeof *result);
  }
  return ok;
}
