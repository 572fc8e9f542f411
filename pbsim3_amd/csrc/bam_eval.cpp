// bam_eval.cpp -- pbsim_truth_bam_eval: a mapper's BAM scored against the truth BAMs (the rule: include/pbsim3_amd.h,
// tests/mapeval_model.py).  The host's part: the streams into HBM and their records (bam_stream.cpp), the references by name
// (bam_eval_rule.cpp) and the counts; the kernels are inflate.hip's, bam_scan.hip's, bam_sort.hip's sort and bam_eval.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bam_eval.h"
#include "bam_fields.h"
#include "bam_scan.h"
#include "bam_sort.h"
#include "bam_stream.h"
#include "ctx.h"

namespace pbsim {

namespace {

const char kWho[] = "pbsim_truth_bam_eval: ";

const BamStage kStage = {kWho, "the stage holds every inflated stream and its records' keys in HBM at once and does not chunk"};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

typedef BamStream Stream;

// the read name of the record at `offset` of a stream
int name_at(const Stream &s, int64_t offset, std::string *name) {
  uint8_t b[kBamFixed + 256];
  memset(b, 0, sizeof b);
  HIP_OK(hipMemcpy(b, s.bytes() + offset, (size_t)std::min<int64_t>((int64_t)sizeof b, s.N - offset), hipMemcpyDeviceToHost));
  const size_t l = b[12];
  name->assign((const char *)b + kBamFixed, l ? l - 1 : 0);
  return PBSIM_SUCCEEDED;
}

int eval_bam(pbsim_ctx *c, const pbsim_eval_truth *truth, int n_truth_files, const uint8_t *query, int64_t n_query_bytes, int32_t permille,
             int hash_bits, const pbsim_eval_sink *sink, int64_t counts[kEvalCounts], int64_t hist[512]) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "eval");
  // ---- 1. every stream into HBM
  std::vector<Stream> tr((size_t)n_truth_files);
  Stream qu;
  qu.what = "the query";
  for (int f = 0; f < n_truth_files; f++) {
    tr[(size_t)f].what = "truth file " + std::to_string(f);
    if (!bam_inflate_stream(c, kStage, (const uint8_t *)truth[f].bytes, truth[f].n, &tr[(size_t)f])) return PBSIM_FAILED;
  }
  if (!bam_inflate_stream(c, kStage, query, n_query_bytes, &qu)) return PBSIM_FAILED;
  ph.mark("inflate");
  // ---- 2. the records of each
  int64_t inflated = qu.N;
  {
    BamScan scan;
    for (Stream &s : tr) {
      if (!bam_locate(c, kStage, &s, &scan, kBamScanPlaced, kBamSortPacking)) return PBSIM_FAILED;
      inflated += s.N;
      ph.mark("scan + chain, " + s.what);
    }
    if (!bam_locate(c, kStage, &qu, &scan, kBamScanAny, kBamSamplePacking)) return PBSIM_FAILED;
    ph.mark("scan + chain, " + qu.what);
  }
  std::vector<int64_t> first_record;  // of each truth file, among all truth records
  int64_t n_t = 0;
  for (const Stream &s : tr) {
    first_record.push_back(n_t);
    n_t += (int64_t)s.rec.size();
  }
  const int64_t n_q = (int64_t)qu.rec.size();
  if (n_t >= (int64_t)kEvalNoRecord || n_q >= (int64_t)kEvalNoRecord) return fail(std::string(kWho) + "more than 2^32 - 2 records");
  // ---- the references, by name
  EvalRefTables tab;
  {
    std::vector<std::vector<std::string>> names;
    std::vector<const char *> over;
    for (int f = 0; f < n_truth_files; f++) {
      names.push_back(tr[(size_t)f].ref_names);
      over.push_back(truth[f].ref_name);
    }
    std::string err;
    if (!eval_ref_tables(names, over, qu.ref_names, &tab, &err)) return fail(kWho + err);
  }
  std::vector<int32_t> maps;  // the truth files' tables one behind the other, then the query's
  std::vector<int64_t> map_at;
  for (const std::vector<int32_t> &m : tab.truth_map) {
    map_at.push_back((int64_t)maps.size());
    maps.insert(maps.end(), m.begin(), m.end());
  }
  const int64_t query_map_at = (int64_t)maps.size();
  maps.insert(maps.end(), tab.query_map.begin(), tab.query_map.end());
  // ---- 3. keys, and the truth's sorted by hash
  enum { kDup = 0, kCls = 1, kRes = 6, kHist = 10, kSmall = 10 + 512 };
  DevBuf d_maps, d_small, d_tptr, d_thash, d_tend, d_tgref, d_tidx, d_key, d_perm, d_qptr, d_qhash, d_qend, d_first, d_verdict, d_tmp;
  if (!alloc(d_maps, (int64_t)maps.size() * 4, "the reference tables") || !alloc(d_small, kSmall * 8, "the counts") ||
      !alloc(d_tptr, n_t * 8, "the truth records' addresses") || !alloc(d_thash, n_t * 8, "the truth records' hashes") ||
      !alloc(d_tend, n_t * 8, "the truth records' ends") || !alloc(d_tgref, n_t * 4, "the truth records' references") ||
      !alloc(d_tidx, n_t * 4, "the truth records' numbers") || !alloc(d_key, n_t * 8, "the sorted hashes") ||
      !alloc(d_perm, n_t * 4, "the sorted numbers") || !alloc(d_qptr, n_q * 8, "the query records' addresses") ||
      !alloc(d_qhash, n_q * 8, "the query records' hashes") || !alloc(d_qend, n_q * 8, "the query records' ends") ||
      !alloc(d_first, n_t * 4, "the truth records' slots") || !alloc(d_verdict, n_t, "the verdicts"))
    return PBSIM_FAILED;
  if (!maps.empty()) HIP_OK(hipMemcpyAsync(d_maps.p, maps.data(), maps.size() * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(d_small.p, 0, kSmall * 8, st));
  HIP_OK(hipMemsetAsync(d_small.p, 0xff, 8, st));  // kDup
  HIP_OK(hipMemsetAsync(d_first.p, 0xff, (size_t)std::max<int64_t>(n_t * 4, 4), st));
  const uint64_t hash_mask = hash_bits <= 0 || hash_bits >= 64 ? ~(uint64_t)0 : ((uint64_t)1 << hash_bits) - 1;
  {
    std::vector<DevBuf> d_rec((size_t)n_truth_files + 1);
    for (int f = 0; f <= n_truth_files; f++) {
      const Stream &s = f < n_truth_files ? tr[(size_t)f] : qu;
      const int64_t n = (int64_t)s.rec.size();
      if (n == 0) continue;
      if (!alloc(d_rec[(size_t)f], n * 8, "a record list")) return PBSIM_FAILED;
      HIP_OK(hipMemcpyAsync(d_rec[(size_t)f].p, s.rec.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
      if (f < n_truth_files)
        launch_eval_keys(s.bytes(), d_rec[(size_t)f].as<uint64_t>(), n, kBamSortPacking, hash_mask, d_maps.as<int32_t>() + map_at[(size_t)f],
                         first_record[(size_t)f], d_tptr.as<uint64_t>(), d_thash.as<uint64_t>(), d_tend.as<int64_t>(), d_tgref.as<int32_t>(),
                         d_tidx.as<uint32_t>(), st);
      else
        launch_eval_keys(s.bytes(), d_rec[(size_t)f].as<uint64_t>(), n, kBamSamplePacking, hash_mask, nullptr, 0, d_qptr.as<uint64_t>(),
                         d_qhash.as<uint64_t>(), d_qend.as<int64_t>(), nullptr, nullptr, st);
      HIP_OK(hipGetLastError());
    }
    HIP_OK(hipStreamSynchronize(st));  // (the record lists go with this frame)
  }
  unsigned long long *small = d_small.as<unsigned long long>();
  if (n_t > 0) {
    const int end_bit = hash_bits <= 0 || hash_bits >= 64 ? 64 : hash_bits;
    size_t tb = 0;
    HIP_OK(bs_sort_pairs(nullptr, &tb, d_thash.as<uint64_t>(), d_key.as<uint64_t>(), d_tidx.as<uint32_t>(), d_perm.as<uint32_t>(), n_t, end_bit, st));
    if (!alloc(d_tmp, (int64_t)tb, "the sort's scratch")) return PBSIM_FAILED;
    HIP_OK(bs_sort_pairs(d_tmp.p, &tb, d_thash.as<uint64_t>(), d_key.as<uint64_t>(), d_tidx.as<uint32_t>(), d_perm.as<uint32_t>(), n_t, end_bit, st));
    launch_eval_duplicates(d_key.as<uint64_t>(), d_perm.as<uint32_t>(), d_tptr.as<uint64_t>(), n_t, small + kDup, st);
    HIP_OK(hipGetLastError());
  }
  uint64_t dup = 0;
  HIP_OK(hipMemcpyAsync(&dup, small + kDup, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("keys + sort");
  if (dup != ~(uint64_t)0) {
    const int64_t later = (int64_t)(dup >> 32), earlier = (int64_t)(dup & 0xffffffffu);
    const int f1 = eval_file_of(first_record, earlier), f2 = eval_file_of(first_record, later);
    const int64_t r1 = earlier - first_record[(size_t)f1], r2 = later - first_record[(size_t)f2];
    std::string name;
    if (!name_at(tr[(size_t)f2], kBamSortPacking.offset(tr[(size_t)f2].rec[(size_t)r2]), &name)) return PBSIM_FAILED;
    return fail(std::string(kWho) + "the read name \"" + name + "\" occurs twice in the truth: record " + std::to_string(r1) + " of truth file " +
                std::to_string(f1) + " and record " + std::to_string(r2) + " of truth file " + std::to_string(f2) +
                " (reads are matched by name: a name may be in the truth once)");
  }
  // ---- 4. the join and the verdicts
  launch_eval_join(d_qptr.as<uint64_t>(), d_qhash.as<uint64_t>(), n_q, d_key.as<uint64_t>(), d_perm.as<uint32_t>(), d_tptr.as<uint64_t>(), n_t,
                   d_first.as<uint32_t>(), small + kCls, st);
  HIP_OK(hipGetLastError());
  launch_eval_verdict(d_tptr.as<uint64_t>(), d_tend.as<int64_t>(), d_tgref.as<int32_t>(), d_first.as<uint32_t>(), n_t, d_qptr.as<uint64_t>(),
                      d_qend.as<int64_t>(), d_maps.as<int32_t>() + query_map_at, (int32_t)tab.query_map.size(), permille, d_verdict.as<uint8_t>(),
                      small + kRes, small + kHist, st);
  HIP_OK(hipGetLastError());
  std::vector<uint64_t> h_small(kSmall);
  std::vector<uint8_t> verdicts;
  HIP_OK(hipMemcpyAsync(h_small.data(), d_small.p, kSmall * 8, hipMemcpyDeviceToHost, st));
  if (sink && sink->on_verdicts && n_t > 0) {
    verdicts.resize((size_t)n_t);
    HIP_OK(hipMemcpyAsync(verdicts.data(), d_verdict.p, (size_t)n_t, hipMemcpyDeviceToHost, st));
  }
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("join + verdict");
  {
    char sum[160];
    snprintf(sum, sizeof sum, "%.1f MB inflated, %lld truth records, %lld query records", inflated / 1e6, (long long)n_t, (long long)n_q);
    ph.print(sum);
  }
  const uint64_t *cls = h_small.data() + kCls, *res = h_small.data() + kRes;  // cls: primary, secondary, supplementary, unknown, known
  counts[kEvalTruth] = n_t;
  counts[kEvalQuery] = n_q;
  counts[kEvalPrimary] = (int64_t)cls[0];
  counts[kEvalSecondary] = (int64_t)cls[1];
  counts[kEvalSupplementary] = (int64_t)cls[2];
  counts[kEvalUnknown] = (int64_t)cls[3];
  counts[kEvalMissing] = (int64_t)res[0];
  counts[kEvalDuplicate] = (int64_t)cls[4] - (n_t - (int64_t)res[0]);  // the known primaries that are not the first of their name
  counts[kEvalUnmapped] = (int64_t)res[1];
  counts[kEvalCorrect] = (int64_t)res[2];
  counts[kEvalWrong] = (int64_t)res[3];
  counts[kEvalScored] = counts[kEvalCorrect] + counts[kEvalWrong];
  for (int k = 0; k < 512; k++) hist[k] = (int64_t)h_small[(size_t)kHist + (size_t)k];
  if (sink && sink->on_verdicts && !sink->on_verdicts(sink->user, verdicts.data(), n_t)) return fail("sink aborted (verdicts)");
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_truth_bam_eval(pbsim_ctx *c, const pbsim_eval_truth *truth, int n_truth, const void *query, int64_t n,
                                    const pbsim_eval_opts *opts, const pbsim_eval_sink *sink, int64_t counts[12], int64_t hist[512]) {
  using pbsim::fail;
  if (!c || !truth || n_truth < 1 || n < 0 || (n > 0 && !query) || !counts || !hist) return fail("pbsim_truth_bam_eval: bad argument");
  for (int f = 0; f < n_truth; f++)
    if (truth[f].n < 0 || (truth[f].n > 0 && !truth[f].bytes)) return fail("pbsim_truth_bam_eval: bad argument");
  int32_t permille = opts ? opts->overlap_permille : 0;
  const int32_t hash_bits = opts ? opts->hash_bits : 0;
  if (permille == 0) permille = 100;
  if (permille < 1 || permille > 1000) return fail("pbsim_truth_bam_eval: overlap_permille must be 1 .. 1000 (0: the default, 100)");
  if (hash_bits < 0 || hash_bits > 64) return fail("pbsim_truth_bam_eval: hash_bits must be 0 .. 64");
  memset(counts, 0, 12 * sizeof(int64_t));
  memset(hist, 0, 512 * sizeof(int64_t));
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::eval_bam(c, truth, n_truth, (const uint8_t *)query, n, permille, hash_bits, sink, counts, hist);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
  }
  return ok;
}
