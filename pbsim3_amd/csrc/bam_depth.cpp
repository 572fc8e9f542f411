// bam_depth.cpp -- pbsim_bam_depth: the depth of coverage of a BAM (the rule: include/pbsim3_amd.h, tests/depth_model.py).  The
// host's part: the stream into HBM and its records (bam_stream.cpp), the references' tables (bam_depth_rule.cpp), the buffers,
// and the text's way to the sink; the kernels are inflate.hip's, bam_scan.hip's, rocPRIM's scan and bam_depth.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bam_depth.h"
#include "bam_scan.h"
#include "bam_stream.h"
#include "ctx.h"
#include "kernels.h"

namespace pbsim {

namespace {

const char kWho[] = "pbsim_bam_depth: ";
const BamStage kStage = {kWho, "the stage holds the inflated stream and the depth array, 4 bytes per reference position, in HBM at once and does not chunk"};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

template <class T>
int upload(DevBuf &b, const std::vector<T> &v, const char *what, hipStream_t st) {
  if (!alloc(b, (int64_t)(v.size() * sizeof(T)), what)) return PBSIM_FAILED;
  if (!v.empty()) HIP_OK(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
  return PBSIM_SUCCEEDED;
}

int depth_bam(pbsim_ctx *c, const uint8_t *src, int64_t n_src, const pbsim_depth_opts &o, const pbsim_depth_sink *sink,
              int64_t counts[kDepthCounts], int64_t hist[256]) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "depth");
  // ---- 1. the stream into HBM, and its records
  BamStream s;
  s.a_what = "a file";
  if (!bam_inflate_stream(c, kStage, src, n_src, &s)) return PBSIM_FAILED;
  ph.mark("inflate");
  {
    BamScan scan;
    if (!bam_locate(c, kStage, &s, &scan, kBamScanAny, kBamSamplePacking)) return PBSIM_FAILED;
  }
  ph.mark("locate");
  const int64_t n_rec = (int64_t)s.rec.size(), inflated = s.N;
  if (n_rec >= (int64_t)1 << 31) return fail(std::string(kWho) + std::to_string(n_rec) + " records: a file of 2^31 records or more is not taken (a depth is an int32)");
  const int32_t n_ref = (int32_t)s.hd.n_ref;
  std::vector<int64_t> off, win;
  {
    std::string err;
    if (!depth_ref_offsets(s.hd.ref_len, o.window, &off, &win, &err)) return fail(kWho + err);
  }
  const int64_t n_slots = off.back(), n_win = o.window ? win.back() : 0;
  const int64_t n_tiles = (n_slots + kDepthTile - 1) / kDepthTile;
  std::vector<int64_t> name_at(1, 0);
  std::string names, names_z;  // one behind the other for the device; NUL-terminated for the sink
  std::vector<size_t> z_at;
  for (const std::string &nm : s.ref_names) {
    names += nm;
    name_at.push_back((int64_t)names.size());
    z_at.push_back(names_z.size());
    names_z += nm;
    names_z.push_back('\0');
  }
  std::vector<const char *> name_ptr;
  for (size_t at : z_at) name_ptr.push_back(names_z.data() + at);
  // ---- 2. the events
  DevBuf d_off, d_win, d_name_at, d_names, d_cells, d_stat, d_diff, d_rec;
  {
    const std::vector<char> nb(names.begin(), names.end());
    if (!upload(d_off, off, "the references' offsets", st) || !upload(d_name_at, name_at, "the references' names", st) ||
        !upload(d_names, nb, "the references' names", st) || (o.window && !upload(d_win, win, "the references' windows", st)))
      return PBSIM_FAILED;
  }
  if (!alloc(d_cells, kDepthCells * 8, "the counts") || !alloc(d_stat, (int64_t)n_ref * 24, "the references' sums") ||
      !alloc(d_diff, (n_tiles + 1) * kDepthTile * 4, "the depth array") || !upload(d_rec, s.rec, "the record list", st))
    return PBSIM_FAILED;
  unsigned long long *cells = d_cells.as<unsigned long long>();
  HIP_OK(hipMemsetAsync(d_cells.p, 0, kDepthCells * 8, st));
  HIP_OK(hipMemsetAsync(cells + kDepthCellFault, 0xff, 8, st));
  HIP_OK(hipMemsetAsync(d_stat.p, 0, (size_t)std::max<int64_t>((int64_t)n_ref * 24, 8), st));
  HIP_OK(hipMemsetAsync(d_diff.p, 0, (size_t)(n_tiles + 1) * kDepthTile * 4, st));
  const DepthRefs refs = {n_ref, d_off.as<int64_t>(), d_win.as<int64_t>(), d_name_at.as<int64_t>(), d_names.as<char>()};
  launch_depth_events(s.bytes(), d_rec.as<uint64_t>(), n_rec, kBamSamplePacking, refs, o.exclude_flags, o.min_mapq, o.count_deletions,
                      d_diff.as<int32_t>(), cells, st);
  HIP_OK(hipGetLastError());
  uint64_t fault = 0;
  HIP_OK(hipMemcpyAsync(&fault, cells + kDepthCellFault, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("events");
  if (fault != ~(uint64_t)0)
    return fail(std::string(kWho) + "the record at inflated byte offset " + std::to_string(fault) +
                " is malformed: a CIGAR op code above 8, or an aux field that runs past the record or has an unknown type");
  d_rec.release();  // the stream and its records have been read for the last time
  s.d.release();
  // ---- 3. the depths
  DevBuf d_tmp;
  if (n_slots > 0) {
    size_t tb = 0;
    HIP_OK(depth_scan(nullptr, &tb, d_diff.as<int32_t>(), n_slots, st));
    if (!alloc(d_tmp, (int64_t)tb, "the scan's scratch")) return PBSIM_FAILED;
    HIP_OK(depth_scan(d_tmp.p, &tb, d_diff.as<int32_t>(), n_slots, st));
  }
  ph.mark("scan");
  // ---- 4. the statistics, and the runs or the windows' sums
  DevBuf d_tiles, d_scan_tmp, d_win_sum, d_run_ref, d_run_start, d_run_depth;
  int64_t n_runs = 0;
  if (o.window) {
    if (!alloc(d_win_sum, n_win * 8, "the windows' sums")) return PBSIM_FAILED;
    HIP_OK(hipMemsetAsync(d_win_sum.p, 0, (size_t)std::max<int64_t>(n_win * 8, 8), st));
  } else if (!alloc(d_tiles, (n_tiles + 1) * 8, "the tiles' run counts") || !alloc(d_scan_tmp, (n_tiles / 1024 + 8) * 8, "the scan's scratch")) {
    return PBSIM_FAILED;
  }
  launch_depth_runs(d_diff.as<int32_t>(), n_slots, refs, o.window, cells, d_stat.as<unsigned long long>(), d_tiles.as<int64_t>(),
                    d_win_sum.as<unsigned long long>(), false, nullptr, nullptr, nullptr, st);
  HIP_OK(hipGetLastError());
  if (!o.window) {
    launch_exclusive_scan_i64(d_tiles.as<int64_t>(), d_tiles.as<int64_t>(), n_tiles, d_scan_tmp.as<int64_t>(), d_tiles.as<int64_t>() + n_tiles, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&n_runs, d_tiles.as<int64_t>() + n_tiles, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (!alloc(d_run_ref, n_runs * 4, "the runs' references") || !alloc(d_run_start, n_runs * 4, "the runs' starts") ||
        !alloc(d_run_depth, n_runs * 4, "the runs' depths"))
      return PBSIM_FAILED;
    launch_depth_runs(d_diff.as<int32_t>(), n_slots, refs, 0, cells, d_stat.as<unsigned long long>(), d_tiles.as<int64_t>(), nullptr, true,
                      d_run_ref.as<int32_t>(), d_run_start.as<int32_t>(), d_run_depth.as<int32_t>(), st);
    HIP_OK(hipGetLastError());
  }
  std::vector<uint64_t> h_cells(kDepthCells), h_stat((size_t)n_ref * 3);
  HIP_OK(hipMemcpyAsync(h_cells.data(), d_cells.p, kDepthCells * 8, hipMemcpyDeviceToHost, st));
  if (n_ref) HIP_OK(hipMemcpyAsync(h_stat.data(), d_stat.p, h_stat.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("runs");
  // ---- 5. the text
  const int64_t n_lines = o.window ? n_win : n_runs;
  DevBuf d_len, d_text;
  int64_t n_text = 0;
  if (n_lines > 0) {
    if (!alloc(d_len, (n_lines + 1) * 8, "the lines' lengths") || !alloc(d_scan_tmp, (n_lines / 1024 + 8) * 8, "the scan's scratch")) return PBSIM_FAILED;
    int64_t *len = d_len.as<int64_t>();
    launch_depth_line_sizes(n_lines, refs, o.window, d_run_ref.as<int32_t>(), d_run_start.as<int32_t>(), d_run_depth.as<int32_t>(),
                            d_win_sum.as<unsigned long long>(), len, st);
    HIP_OK(hipGetLastError());
    launch_exclusive_scan_i64(len, len, n_lines, d_scan_tmp.as<int64_t>(), len + n_lines, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&n_text, len + n_lines, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (!alloc(d_text, n_text, "the text")) return PBSIM_FAILED;
    launch_depth_line_fill(n_lines, refs, o.window, d_run_ref.as<int32_t>(), d_run_start.as<int32_t>(), d_run_depth.as<int32_t>(),
                           d_win_sum.as<unsigned long long>(), len, d_text.as<char>(), st);
    HIP_OK(hipGetLastError());
  }
  // ---- what the sink is told
  for (int k = 0; k < kDepthCounts; k++) counts[k] = (int64_t)h_cells[(size_t)kDepthCellCounts + (size_t)k];
  counts[kDepthRecords] = n_rec;
  for (int k = 0; k < 256; k++) hist[k] = (int64_t)h_cells[(size_t)kDepthCellHist + (size_t)k];
  std::vector<int64_t> rows((size_t)n_ref * 4);
  for (int32_t r = 0; r < n_ref; r++) {
    rows[4 * (size_t)r] = s.hd.ref_len[(size_t)r];
    for (int k = 0; k < 3; k++) rows[4 * (size_t)r + 1 + (size_t)k] = (int64_t)h_stat[3 * (size_t)r + (size_t)k];
  }
  if (sink && sink->on_refs && !sink->on_refs(sink->user, n_ref, name_ptr.data(), rows.data())) return fail("sink aborted (references)");
  if (sink && sink->on_text && n_text > 0) {
    // two pinned pieces: one on its way to the host while the sink has the other
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
    auto start_copy = [&](int64_t at, int which) {
      const int64_t take = std::min(piece, n_text - at);
      hipError_t e = hipMemcpyAsync(pinned[which].p, d_text.as<char>() + at, (size_t)take, hipMemcpyDeviceToHost, st);
      return e != hipSuccess ? e : hipEventRecord(done[which], st);
    };
    HIP_OK(start_copy(0, 0));
    int which = 0;
    for (int64_t at = 0; at < n_text; at += piece, which ^= 1) {
      if (at + piece < n_text) HIP_OK(start_copy(at + piece, which ^ 1));
      HIP_OK(hipEventSynchronize(done[which]));
      if (!sink->on_text(sink->user, (const char *)pinned[which].p, std::min(piece, n_text - at), at)) return fail("sink aborted (text)");
    }
  }
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("text");
  {
    char sum[200];
    snprintf(sum, sizeof sum, "%.1f MB inflated, %lld records, %lld reference positions, %lld lines, %.1f MB of text", inflated / 1e6, (long long)n_rec,
             (long long)(n_slots - n_ref), (long long)n_lines, n_text / 1e6);
    ph.print(sum);
  }
  if (sink && sink->on_depth) {
    std::vector<int32_t> host;
    for (int32_t r = 0; r < n_ref; r++) {
      const int64_t l = s.hd.ref_len[(size_t)r];
      host.resize((size_t)std::max<int64_t>(l, 1));
      if (l > 0) HIP_OK(hipMemcpy(host.data(), d_diff.as<int32_t>() + off[(size_t)r], (size_t)l * 4, hipMemcpyDeviceToHost));
      if (!sink->on_depth(sink->user, r, host.data(), l)) return fail("sink aborted (depth)");
    }
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_bam_depth(pbsim_ctx *c, const void *bam, int64_t n, const pbsim_depth_opts *opts, const pbsim_depth_sink *sink,
                               int64_t counts[6], int64_t hist[256]) {
  using pbsim::fail;
  if (!c || n < 0 || (n > 0 && !bam) || !counts || !hist) return fail("pbsim_bam_depth: bad argument");
  pbsim_depth_opts o;
  std::string err;
  if (!pbsim::depth_check_opts(opts, &o, &err)) return fail("pbsim_bam_depth: " + err);
  memset(counts, 0, 6 * sizeof(int64_t));
  memset(hist, 0, 256 * sizeof(int64_t));
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::depth_bam(c, (const uint8_t *)bam, n, o, sink, counts, hist);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
  }
  return ok;
}
