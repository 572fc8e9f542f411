// sample_profile.cpp -- get_sample_inf (pbsim.cpp:1155-1330) on the GPU: the host side of sample_profile.hip.  The FASTQ's
// bytes go through HBM in windows (pinned staging, the upload of window k + 1 beside the kernels of window k; bytes that are
// in HBM already are copied there); the line-feed phase and an unfinished quality line are carried from window to window;
// per record only its length and its accuracy come back, and the statistics are the host's arithmetic over them in file
// order (unit_io.cpp), so every number and every error text is the stdio parser's.  The kept strings never leave the GPU:
// they are packed into the pool pbsim_set_sample_profile would have uploaded.
//
// A BAM (unaligned or aligned; pbsim_load_sample, pbsim_sample_profile_from_bam_*) gives the profile of the FASTQ that
// `samtools fastq` would write from it, through sample_bam.hip: the stream behind the header passes through HBM in the same
// windows, the bytes of an unfinished record in front of the next one; the scan's candidates come back, the chain walk over
// them (bam_chain.cpp) says which are records, and from there on the pass is the FASTQ's.
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <limits.h>
#include <math.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "bam_scan.h"
#include "ctx.h"
#include "engine_internal.h"
#include "inflate_host.h"
#include "input_file.h"
#include "unit_io.h"

namespace pbsim {
namespace {

constexpr int64_t kCarryRoom = 1 << 20;     // in front of a window: the unfinished quality line (at most 1 000 000 bytes, else the reference's error)
constexpr int64_t kWindowSlack = kSpTile + 64;
constexpr int64_t kDefaultChunk = (int64_t)64 << 20;
constexpr int64_t kMaxChunk = (int64_t)1 << 30;  // window offsets are 32 bits
constexpr int64_t kMaxQual = 1000000, kMaxNum = 100000000;
const char *const kTooLong = "fastq is too long. Max acceptable length is 1000000.";
const char *const kTooMany = "fastq is too many. Max acceptable number is 100000000.";

struct Source {  // the FASTQ's bytes: on the host, in an open plain file, or in the memory of the context's GPU
  const uint8_t *host = nullptr, *dev = nullptr;
  int fd = -1;
  const char *path = nullptr;  // of fd
  int64_t n = 0;
};

struct Meta {  // device -> host per window
  int64_t n_lf, kept_bytes;
  int32_t nul, pad;
};

// A window's bytes into pinned staging on up to 16 threads -- the host's share of the pass, and the slowest stage of it: from
// host memory by memcpy, from a file by pread (no mapping whose pages would fault in one by one).  false: a read failed.
bool fill_staging(void *dst, const Source &src, int64_t at, size_t n) {
  const size_t nt = std::max<size_t>(1, std::min<size_t>(16, n / ((size_t)4 << 20)));
  std::vector<char> ok(nt, 1);
  auto part = [&](size_t t) {
    const size_t a = n * t / nt, e = n * (t + 1) / nt;
    if (src.host) {
      memcpy((char *)dst + a, src.host + at + a, e - a);
      return;
    }
    for (size_t o = a; o < e;) {
      const ssize_t k = pread(src.fd, (char *)dst + o, e - o, (off_t)(at + (int64_t)o));
      if (k <= 0) {
        ok[t] = 0;
        return;
      }
      o += (size_t)k;
    }
  };
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; t++) th.emplace_back(part, t);
  part(0);
  for (auto &x : th) x.join();
  return std::find(ok.begin(), ok.end(), 0) == ok.end();
}

void to_abi(const SampleProfile &s, pbsim_sample_stats *o) {
  o->num = s.num;
  o->len_min = s.len_min;
  o->len_max = s.len_max;
  o->len_total = s.len_total;
  o->num_filtered = s.num_filtered;
  o->len_min_filtered = s.len_min_filtered;
  o->len_max_filtered = s.len_max_filtered;
  o->len_total_filtered = s.len_total_filtered;
  o->len_mean_filtered = s.len_mean_filtered;
  o->len_sd_filtered = s.len_sd_filtered;
  o->accuracy_mean_filtered = s.accuracy_mean_filtered;
  o->accuracy_sd_filtered = s.accuracy_sd_filtered;
}

// the whole profile from a parse on the host (a FASTQ with NUL bytes, a pipe): uploaded as pbsim_set_sample_profile does
int commit_host_profile(pbsim_ctx *c, const SampleProfile &prof, pbsim_sample_stats *out) {
  std::vector<const uint8_t *> qp;
  std::vector<int64_t> ql;
  qp.reserve(prof.quals.size());
  ql.reserve(prof.quals.size());
  for (const std::string &q : prof.quals) {
    qp.push_back((const uint8_t *)q.data());
    ql.push_back((int64_t)q.size());
  }
  if (!pbsim_set_sample_profile(c, (int64_t)qp.size(), qp.data(), ql.data())) return PBSIM_FAILED;
  to_abi(prof, out);
  return PBSIM_SUCCEEDED;
}

struct Builder {
  pbsim_ctx *c;
  hipStream_t s_work = nullptr, s_copy = nullptr;
  hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
  bool up_used[2] = {false, false}, done_used[2] = {false, false};
  DevBuf d_buf[2], d_tiles, d_scan_tmp, d_meta, d_qprob, d_start, d_end, d_len, d_acc, d_padded, d_off, d_pool;
  HostBuf h_stage[2], h_meta, h_len, h_acc;
  ~Builder() {  // whatever happens: nothing in flight when the buffers go
    for (hipStream_t s : {s_work, s_copy})
      if (s) {
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
      }
    for (hipEvent_t e : {ev_up[0], ev_up[1], ev_done[0], ev_done[1]})
      if (e) (void)hipEventDestroy(e);
  }

  // PBSIM_SUCCEEDED with *nul = true: the bytes hold a NUL (fgets + strlen semantics, the caller's stdio pass)
  int run(const Source &src, double acc_min, double acc_max, pbsim_sample_stats *out, bool *nul) {
    *nul = false;
    const int64_t chunk = std::min(c->sp_chunk_bytes > 0 ? c->sp_chunk_bytes : kDefaultChunk, kMaxChunk);
    const int64_t n_chunks = (src.n + chunk - 1) / chunk;
    const int64_t room = std::min(chunk, src.n);
    const long len_min = (long)c->p.len_min, len_max = (long)c->p.len_max;
    const bool trace = getenv("PBSIM_TRACE") != nullptr;
    HIP_OK(hipStreamCreateWithFlags(&s_work, hipStreamNonBlocking));
    HIP_OK(hipStreamCreateWithFlags(&s_copy, hipStreamNonBlocking));
    for (int b = 0; b < 2; b++) {
      HIP_OK(hipEventCreateWithFlags(&ev_up[b], hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&ev_done[b], hipEventDisableTiming));
    }
    for (int b = 0; b < (n_chunks > 1 ? 2 : 1); b++) {
      HIP_OK(d_buf[b].ensure((size_t)(kCarryRoom + room + kWindowSlack), true));
      if (!src.dev) HIP_OK(h_stage[b].ensure((size_t)room));
    }
    HIP_OK(d_tiles.ensure((size_t)(sp_tiles(0, kCarryRoom + room) + 2) * 8));
    HIP_OK(d_scan_tmp.ensure((size_t)((kCarryRoom + room) / kSpTile / 1024 + 8) * 8));
    HIP_OK(d_meta.ensure(sizeof(Meta)));
    HIP_OK(h_meta.ensure(sizeof(Meta) + 8));
    HIP_OK(hipMemsetAsync(d_meta.p, 0, sizeof(Meta), s_work));
    {
      double qprob[94];
      for (int q = 0; q < 94; q++) qprob[q] = pow(10, (double)q / -10);  // pbsim.cpp:546-549
      HIP_OK(d_qprob.ensure(sizeof qprob));
      HIP_OK(hipMemcpyAsync(d_qprob.p, qprob, sizeof qprob, hipMemcpyHostToDevice, s_work));
      HIP_OK(hipStreamSynchronize(s_work));
    }
    // the pool: most FASTQ files are half quality lines; it grows when this one is not
    int64_t pool_fill = 0;
    HIP_OK(d_pool.ensure((size_t)(src.n / 2 + (64 << 10)), true));

    auto stage = [&](int64_t k) -> int {  // window k's bytes on their way into buffer k & 1, behind its carry room
      const int b = (int)(k & 1);
      const int64_t at = k * chunk, n = std::min(chunk, src.n - at);
      uint8_t *to = d_buf[b].as<uint8_t>() + kCarryRoom;
      if (done_used[b]) HIP_OK(hipStreamWaitEvent(s_copy, ev_done[b], 0));  // the kernels of window k - 2 read this buffer
      if (!src.dev) {
        if (up_used[b]) HIP_OK(hipEventSynchronize(ev_up[b]));
        if (!fill_staging(h_stage[b].p, src, at, (size_t)n)) return fail(std::string("Cannot read file: ") + src.path);
        HIP_OK(hipMemcpyAsync(to, h_stage[b].p, (size_t)n, hipMemcpyHostToDevice, s_copy));
      } else {
        HIP_OK(hipMemcpyAsync(to, src.dev + at, (size_t)n, hipMemcpyDeviceToDevice, s_copy));
      }
      HIP_OK(hipEventRecord(ev_up[b], s_copy));
      up_used[b] = true;
      return PBSIM_SUCCEEDED;
    };

    SampleProfile prof;
    prof.len_min = LONG_MAX;
    std::vector<int32_t> in_len;  // the records whose length is in range, in file order
    std::vector<double> in_acc;
    std::vector<int32_t> sq_len;
    std::vector<int64_t> sq_off;
    int phase = 0;          // line feeds into the current record
    int64_t carry_len = 0;  // bytes of an unfinished quality line in front of the next window
    if (n_chunks > 0 && !stage(0)) return PBSIM_FAILED;
    for (int64_t k = 0; k < n_chunks; k++) {
      const int b = (int)(k & 1);
      const uint8_t *buf = d_buf[b].as<uint8_t>();
      const int64_t b0 = kCarryRoom - carry_len, b1 = kCarryRoom + std::min(chunk, src.n - k * chunk);
      Meta *dm = d_meta.as<Meta>(), *hm = (Meta *)h_meta.p;
      HIP_OK(hipStreamWaitEvent(s_work, ev_up[b], 0));
      launch_sp_count(buf, b0, b1, d_tiles.as<int64_t>(), &dm->nul, s_work);
      launch_exclusive_scan_i64(d_tiles.as<int64_t>(), d_tiles.as<int64_t>(), sp_tiles(b0, b1), d_scan_tmp.as<int64_t>(), &dm->n_lf, s_work);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(hm, dm, sizeof(Meta), hipMemcpyDeviceToHost, s_work));
      if (k + 1 < n_chunks && !stage(k + 1)) return PBSIM_FAILED;  // (the host's copy into staging: beside the count)
      HIP_OK(hipStreamSynchronize(s_work));
      if (hm->nul) {
        *nul = true;
        return PBSIM_SUCCEEDED;
      }
      const int64_t n_lf = hm->n_lf, n_rec = (phase + n_lf) / 4;
      const int next_phase = (int)((phase + n_lf) % 4);
      uint32_t *h_tail = (uint32_t *)((char *)h_meta.p + sizeof(Meta));  // where the unfinished quality line starts
      if (n_rec > 0 || next_phase == 3) {
        HIP_OK(d_start.ensure((size_t)(n_rec + 1) * 4));
        HIP_OK(d_end.ensure((size_t)(n_rec + 1) * 4));
        launch_sp_lines(buf, b0, b1, phase, d_tiles.as<int64_t>(), d_start.as<uint32_t>(), d_end.as<uint32_t>(), s_work);
        if (next_phase == 3) HIP_OK(hipMemcpyAsync(h_tail, d_start.as<uint32_t>() + n_rec, 4, hipMemcpyDeviceToHost, s_work));
      }
      int64_t kept_bytes = 0;
      if (n_rec > 0) {
        HIP_OK(d_len.ensure((size_t)n_rec * 4));
        HIP_OK(d_acc.ensure((size_t)n_rec * 8));
        HIP_OK(d_padded.ensure((size_t)n_rec * 8));
        HIP_OK(d_off.ensure((size_t)n_rec * 8));
        HIP_OK(d_scan_tmp.ensure((size_t)(n_rec / 1024 + 8) * 8));
        HIP_OK(h_len.ensure((size_t)n_rec * 4));
        HIP_OK(h_acc.ensure((size_t)n_rec * 8));
        launch_sp_sums(buf, d_start.as<uint32_t>(), d_end.as<uint32_t>(), n_rec, (int32_t)std::min<long>(std::max<long>(len_min, 0), kMaxQual + 1),
                       (int32_t)std::min<long>(len_max, kMaxQual), acc_min, acc_max, d_qprob.as<double>(), d_len.as<int32_t>(),
                       d_acc.as<double>(), d_padded.as<int64_t>(), s_work);
        launch_exclusive_scan_i64(d_padded.as<int64_t>(), d_off.as<int64_t>(), n_rec, d_scan_tmp.as<int64_t>(), &dm->kept_bytes, s_work);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(h_len.p, d_len.p, (size_t)n_rec * 4, hipMemcpyDeviceToHost, s_work));
        HIP_OK(hipMemcpyAsync(h_acc.p, d_acc.p, (size_t)n_rec * 8, hipMemcpyDeviceToHost, s_work));
        HIP_OK(hipMemcpyAsync(hm, dm, sizeof(Meta), hipMemcpyDeviceToHost, s_work));
      }
      HIP_OK(hipStreamSynchronize(s_work));
      // ---- the window's records in file order: the all-reads numbers, the reference's limits, what the filter keeps
      const int32_t *hl = (const int32_t *)h_len.p;
      const double *ha = (const double *)h_acc.p;
      for (int64_t r = 0; r < n_rec; r++) {
        const long len = hl[r];
        if (len > kMaxQual) return fail(kTooLong);
        prof.num++;
        prof.len_total += len;
        if (prof.num > kMaxNum) return fail(kTooMany);
        prof.len_max = std::max(prof.len_max, len);
        prof.len_min = std::min(prof.len_min, len);
        if (len < len_min || len > len_max) continue;
        in_len.push_back((int32_t)len);
        in_acc.push_back(ha[r]);
        if (ha[r] >= acc_min && ha[r] <= acc_max) {
          sq_len.push_back((int32_t)len);
          sq_off.push_back(pool_fill + kept_bytes);
          kept_bytes += (len + 7) & ~7L;
        }
      }
      if (n_rec > 0 && kept_bytes != hm->kept_bytes) return fail("internal: the GPU's sample filter disagrees with the host's");
      if (kept_bytes > 0) {
        if ((size_t)(pool_fill + kept_bytes + 8) > d_pool.bytes) {  // grow, keeping what is there
          DevBuf bigger;
          HIP_OK(bigger.ensure((size_t)(pool_fill + kept_bytes + 8) + (size_t)(pool_fill + kept_bytes) / 2, true));
          HIP_OK(hipMemcpyAsync(bigger.p, d_pool.p, (size_t)pool_fill, hipMemcpyDeviceToDevice, s_work));
          HIP_OK(hipStreamSynchronize(s_work));
          std::swap(bigger.p, d_pool.p);
          std::swap(bigger.bytes, d_pool.bytes);
        }
        launch_sp_pool(buf, d_start.as<uint32_t>(), d_len.as<int32_t>(), d_padded.as<int64_t>(), d_off.as<int64_t>(), n_rec,
                       d_pool.as<uint8_t>() + pool_fill, s_work);
        HIP_OK(hipGetLastError());
        pool_fill += kept_bytes;
      }
      // ---- what the next window inherits
      carry_len = 0;
      if (next_phase == 3) {
        const int64_t from = (int64_t)*h_tail;
        carry_len = b1 - from;
        if (carry_len > kMaxQual) return fail(kTooLong);  // (the chunks of an unterminated 4th line trip the same test in the stdio path)
        if (k + 1 < n_chunks && carry_len > 0)
          HIP_OK(hipMemcpyAsync(d_buf[1 - b].as<uint8_t>() + kCarryRoom - carry_len, buf + from, (size_t)carry_len, hipMemcpyDeviceToDevice, s_work));
      }
      phase = next_phase;
      HIP_OK(hipEventRecord(ev_done[b], s_work));
      done_used[b] = true;
      if (trace)
        fprintf(stderr, "[pbsim sample profile] window %lld: %lld bytes, %lld records, %lld pool bytes, carry %lld\n", (long long)k,
                (long long)(b1 - b0), (long long)n_rec, (long long)kept_bytes, (long long)carry_len);
    }
    {
      std::string e;
      if (!sample_stats_from_records(in_len.data(), in_acc.data(), in_len.size(), len_max, acc_min, acc_max, &prof, &e)) return fail(e);
    }
    if (sq_len.size() > 0x7fffffffULL) return fail("too many sample reads");
    HIP_OK(hipMemsetAsync(d_pool.as<uint8_t>() + pool_fill, 0, 8, s_work));  // the 8 spare bytes of pbsim_set_sample_profile's pool
    HIP_OK(hipStreamSynchronize(s_work));
    // ---- the context's profile, replaced only now
    std::swap(c->d_sq.p, d_pool.p);
    std::swap(c->d_sq.bytes, d_pool.bytes);
    c->sq_len.swap(sq_len);
    c->sq_off.swap(sq_off);
    c->sq_total = prof.len_total_filtered;
    to_abi(prof, out);
    return PBSIM_SUCCEEDED;
  }
};

int check_args(pbsim_ctx *c, const char *who, bool have_input, int64_t n, double acc_min, double acc_max, pbsim_sample_stats *out) {
  if (!c || !out || n < 0 || !have_input) return fail(std::string(who) + ": bad argument");
  if (!(acc_min <= acc_max)) return fail(std::string(who) + ": accuracy_min exceeds accuracy_max");
  NEED_DEVICE(c);
  if (c->p.method != PBSIM_METHOD_SAMPLE) return fail(std::string(who) + ": method is not sample");
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipStreamSynchronize(c->stream));
  return PBSIM_SUCCEEDED;
}

int build(pbsim_ctx *c, const Source &src, double acc_min, double acc_max, pbsim_sample_stats *out) {
  bool nul = false;
  {
    Builder b;
    b.c = c;
    if (!b.run(src, acc_min, acc_max, out, &nul)) return PBSIM_FAILED;
  }
  if (!nul) return PBSIM_SUCCEEDED;
  // NUL bytes: strlen() ends an fgets chunk there, which only the stdio pass reproduces
  SampleProfile prof;
  std::string e;
  if (src.fd >= 0) {
    if (!read_sample_fastq_stdio(src.path, (long)c->p.len_min, (long)c->p.len_max, acc_min, acc_max, &prof, &e)) return fail(e);
    return commit_host_profile(c, prof, out);
  }
  std::vector<uint8_t> down;
  const uint8_t *bytes = src.host;
  if (!bytes) {
    down.resize((size_t)src.n);
    HIP_OK(hipMemcpy(down.data(), src.dev, (size_t)src.n, hipMemcpyDeviceToHost));
    bytes = down.data();
  }
  if (!read_sample_fastq_mem(bytes, (size_t)src.n, (long)c->p.len_min, (long)c->p.len_max, acc_min, acc_max, &prof, &e)) return fail(e);
  return commit_host_profile(c, prof, out);
}

// ---- BAM

struct BamMeta {  // device -> host per window
  int64_t kept_bytes;
};

struct BamBuilder {
  pbsim_ctx *c;
  hipStream_t st = nullptr;
  DevBuf d_buf[2], d_scan_tmp, d_meta, d_qprob, d_rec, d_qual, d_len, d_status, d_acc, d_padded, d_off, d_pool;
  HostBuf h_meta;
  BamScan scan;
  ~BamBuilder() {  // whatever happens: nothing in flight when the buffers go
    if (st) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
    }
  }

  // `label`: what the error texts call the input (the path)
  int run(const Source &src, const std::string &label, double acc_min, double acc_max, pbsim_sample_stats *out) {
    const int64_t chunk = std::min(c->sp_chunk_bytes > 0 ? c->sp_chunk_bytes : kDefaultChunk, kMaxChunk);
    const long len_min = (long)c->p.len_min, len_max = (long)c->p.len_max;
    const bool trace = getenv("PBSIM_TRACE") != nullptr;
    // ---- the header: only as far as the first record
    BamHeader hd;
    {
      std::vector<uint8_t> down;
      for (int64_t have = src.host ? src.n : std::min<int64_t>(src.n, 64 << 10);; have = std::min<int64_t>(src.n, have * 4)) {
        const uint8_t *h = src.host;
        if (!h) {
          down.resize((size_t)have);
          if (have) HIP_OK(hipMemcpy(down.data(), src.dev, (size_t)have, hipMemcpyDeviceToHost));
          h = down.data();
        }
        const int ok = bam_parse_header(h, have, src.n, false, &hd);
        if (ok == -2) return fail(label + ": not a BAM stream (no BAM\\1 magic)");
        if (ok < 0 || (ok == 0 && have >= src.n)) return fail(label + ": truncated BAM header");
        if (ok > 0) break;
      }
    }
    HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP_OK(d_meta.ensure(sizeof(BamMeta)));
    HIP_OK(h_meta.ensure(sizeof(BamMeta)));
    HIP_OK(hipMemsetAsync(d_meta.p, 0, sizeof(BamMeta), st));
    {
      double qprob[94];
      for (int q = 0; q < 94; q++) qprob[q] = pow(10, (double)q / -10);  // pbsim.cpp:546-549
      HIP_OK(d_qprob.ensure(sizeof qprob));
      HIP_OK(hipMemcpyAsync(d_qprob.p, qprob, sizeof qprob, hipMemcpyHostToDevice, st));
      HIP_OK(hipStreamSynchronize(st));
    }
    int64_t pool_fill = 0;
    HIP_OK(d_pool.ensure((size_t)(src.n / 2 + (64 << 10)), true));

    SampleProfile prof;
    prof.len_min = LONG_MAX;
    std::vector<int32_t> in_len;  // the counted records whose length is in range, in file order
    std::vector<double> in_acc;
    std::vector<int32_t> sq_len;
    std::vector<int64_t> sq_off;
    std::vector<uint64_t> hits, rec;
    std::vector<int32_t> hl, hs;
    std::vector<double> ha;
    BamMeta *dm = d_meta.as<BamMeta>(), *hm = (BamMeta *)h_meta.p;
    int64_t at = hd.first_record;  // stream offset of the window buffer's first byte: where the next record starts
    int64_t upto = hd.first_record;  // stream bytes that have been in a window
    int64_t carry_from = 0, carry_len = 0;  // the unfinished record in the previous window's buffer
    int64_t index = 0;       // records so far, skipped ones included
    for (int64_t k = 0; upto < src.n; k++) {
      const int b = (int)(k & 1);
      const int64_t fresh = std::min(chunk, src.n - upto), size = carry_len + fresh;
      const bool last = upto + fresh == src.n;
      HIP_OK(d_buf[b].ensure((size_t)(size + kBamSlack)));
      uint8_t *buf = d_buf[b].as<uint8_t>();
      if (carry_len > 0)
        HIP_OK(hipMemcpyAsync(buf, d_buf[1 - b].as<uint8_t>() + carry_from, (size_t)carry_len, hipMemcpyDeviceToDevice, st));
      if (src.dev) HIP_OK(hipMemcpyAsync(buf + carry_len, src.dev + upto, (size_t)fresh, hipMemcpyDeviceToDevice, st));
      else HIP_OK(hipMemcpyAsync(buf + carry_len, src.host + upto, (size_t)fresh, hipMemcpyHostToDevice, st));
      HIP_OK(hipMemsetAsync(buf + size, 0, (size_t)kBamSlack, st));
      upto += fresh;
      // ---- candidates, ascending
      HIP_OK(scan.run(kBamScanAny, buf, 0, size, (int32_t)hd.n_ref, st, &hits));
      // ---- the chain: the records that lie whole in this window
      rec.clear();
      int64_t stop = 0;
      const BamChainEnd end = bam_walk_chain(kBamSamplePacking, hits.data(), hits.size(), 0, size, last, &rec, &stop);
      const int64_t n_rec = (int64_t)rec.size();
      int64_t kept_bytes = 0;
      if (n_rec > 0) {
        HIP_OK(d_rec.ensure((size_t)n_rec * 8));
        HIP_OK(d_qual.ensure((size_t)n_rec * 4));
        HIP_OK(d_len.ensure((size_t)n_rec * 4));
        HIP_OK(d_status.ensure((size_t)n_rec * 4));
        HIP_OK(d_acc.ensure((size_t)n_rec * 8));
        HIP_OK(d_padded.ensure((size_t)n_rec * 8));
        HIP_OK(d_off.ensure((size_t)n_rec * 8));
        HIP_OK(d_scan_tmp.ensure((size_t)(n_rec / 1024 + 8) * 8));
        hl.resize((size_t)n_rec);
        hs.resize((size_t)n_rec);
        ha.resize((size_t)n_rec);
        HIP_OK(hipMemcpyAsync(d_rec.p, rec.data(), (size_t)n_rec * 8, hipMemcpyHostToDevice, st));
        launch_sb_sums(buf, d_rec.as<uint64_t>(), n_rec, (int32_t)std::min<long>(std::max<long>(len_min, 0), kMaxQual + 1),
                       (int32_t)std::min<long>(len_max, kMaxQual), acc_min, acc_max, d_qprob.as<double>(), d_qual.as<uint32_t>(),
                       d_len.as<int32_t>(), d_status.as<int32_t>(), d_acc.as<double>(), d_padded.as<int64_t>(), st);
        launch_exclusive_scan_i64(d_padded.as<int64_t>(), d_off.as<int64_t>(), n_rec, d_scan_tmp.as<int64_t>(), &dm->kept_bytes, st);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(hl.data(), d_len.p, (size_t)n_rec * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hs.data(), d_status.p, (size_t)n_rec * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(ha.data(), d_acc.p, (size_t)n_rec * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(hm, dm, sizeof(BamMeta), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
      }
      // ---- the window's records in file order, as the FASTQ's: the all-reads numbers, the reference's limits, the filter
      for (int64_t r = 0; r < n_rec; r++) {
        index++;
        if (hs[(size_t)r] == kSbSkipped) continue;  // secondary, supplementary: not a read of `samtools fastq`
        if (hs[(size_t)r] == kSbNoQual) {
          uint8_t head[36 + 256];
          const size_t n = (size_t)std::min<int64_t>((int64_t)sizeof head, 4 + kBamSamplePacking.size(rec[(size_t)r]));
          HIP_OK(hipMemcpy(head, buf + kBamSamplePacking.offset(rec[(size_t)r]), n, hipMemcpyDeviceToHost));
          const size_t l_name = std::min<size_t>(head[12], n - 36);
          return fail(label + ": BAM record " + std::to_string(index) + " (" +
                      std::string((const char *)head + 36, strnlen((const char *)head + 36, l_name)) + ") has no qualities");
        }
        const long len = hl[(size_t)r];
        if (len > kMaxQual) return fail(kTooLong);
        prof.num++;
        prof.len_total += len;
        if (prof.num > kMaxNum) return fail(kTooMany);
        prof.len_max = std::max(prof.len_max, len);
        prof.len_min = std::min(prof.len_min, len);
        if (len < len_min || len > len_max) continue;
        in_len.push_back((int32_t)len);
        in_acc.push_back(ha[(size_t)r]);
        if (ha[(size_t)r] >= acc_min && ha[(size_t)r] <= acc_max) {
          sq_len.push_back((int32_t)len);
          sq_off.push_back(pool_fill + kept_bytes);
          kept_bytes += (len + 7) & ~7L;
        }
      }
      if (n_rec > 0 && kept_bytes != hm->kept_bytes) return fail("internal: the GPU's sample filter disagrees with the host's");
      if (end == kBamChainMalformed)
        return fail(label + ": malformed or truncated BAM record at inflated offset " + std::to_string(at + stop));
      if (kept_bytes > 0) {
        if ((size_t)(pool_fill + kept_bytes + 8) > d_pool.bytes) {  // grow, keeping what is there
          DevBuf bigger;
          HIP_OK(bigger.ensure((size_t)(pool_fill + kept_bytes + 8) + (size_t)(pool_fill + kept_bytes) / 2, true));
          HIP_OK(hipMemcpyAsync(bigger.p, d_pool.p, (size_t)pool_fill, hipMemcpyDeviceToDevice, st));
          HIP_OK(hipStreamSynchronize(st));
          std::swap(bigger.p, d_pool.p);
          std::swap(bigger.bytes, d_pool.bytes);
        }
        launch_sb_pool(buf, d_rec.as<uint64_t>(), d_qual.as<uint32_t>(), d_len.as<int32_t>(), d_padded.as<int64_t>(), d_off.as<int64_t>(),
                       n_rec, d_pool.as<uint8_t>() + pool_fill, st);
        HIP_OK(hipGetLastError());
        pool_fill += kept_bytes;
      }
      // ---- what the next window inherits: the bytes of the record that this one does not complete
      carry_from = stop;
      carry_len = size - stop;
      at += stop;
      if (trace)
        fprintf(stderr, "[pbsim sample profile] BAM window %lld: %lld bytes, %lld candidates, %lld records, %lld pool bytes, carry %lld\n",
                (long long)k, (long long)size, (long long)hits.size(), (long long)n_rec, (long long)kept_bytes, (long long)carry_len);
    }
    {
      std::string e;
      if (!sample_stats_from_records(in_len.data(), in_acc.data(), in_len.size(), len_max, acc_min, acc_max, &prof, &e)) return fail(e);
    }
    if (sq_len.size() > 0x7fffffffULL) return fail("too many sample reads");
    HIP_OK(hipMemsetAsync(d_pool.as<uint8_t>() + pool_fill, 0, 8, st));  // the 8 spare bytes of pbsim_set_sample_profile's pool
    HIP_OK(hipStreamSynchronize(st));
    // ---- the context's profile, replaced only now
    std::swap(c->d_sq.p, d_pool.p);
    std::swap(c->d_sq.bytes, d_pool.bytes);
    c->sq_len.swap(sq_len);
    c->sq_off.swap(sq_off);
    c->sq_total = prof.len_total_filtered;
    to_abi(prof, out);
    return PBSIM_SUCCEEDED;
  }
};

int build_bam(pbsim_ctx *c, const Source &src, const std::string &label, double acc_min, double acc_max, pbsim_sample_stats *out) {
  BamBuilder b;
  b.c = c;
  return b.run(src, label, acc_min, acc_max, out);
}

bool is_bam(const uint8_t *four) { return memcmp(four, "BAM\1", 4) == 0; }

}  // namespace
}  // namespace pbsim

namespace pbsim {
namespace {
// a --sample file on the context's GPU; `bam_ok`: a stream that begins with BAM\1 is read as a BAM, else as the FASTQ it is not
int load_file(pbsim_ctx *c, const char *path, double accuracy_min, double accuracy_max, pbsim_sample_stats *out, bool bam_ok) {
  const long len_min = (long)c->p.len_min, len_max = (long)c->p.len_max;
  struct stat sb;
  int fd = -1;
  if (stat(path, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) {  // (a FIFO is opened once, by the stdio parse)
    fd = open(path, O_RDONLY);
    if (fd < 0) return fail(std::string("Cannot open file: ") + path);
  }
  if (fd < 0) {  // a pipe, an empty file, a file that is not there: the stdio parse (and its message), uploaded as ever
    SampleProfile prof;
    std::string e;
    if (!read_sample_fastq_stdio(path, len_min, len_max, accuracy_min, accuracy_max, &prof, &e)) return fail(e);
    return commit_host_profile(c, prof, out);
  }
  struct Close {
    int fd;
    ~Close() { close(fd); }
  } closer{fd};
  Source src;
  src.fd = fd;
  src.path = path;
  src.n = (int64_t)sb.st_size;
  unsigned char magic[4] = {0, 0, 0, 0};
  const ssize_t got = pread(fd, magic, 4, 0);
  if (bam_ok && got == 4 && is_bam(magic)) {  // an uncompressed BAM: the mapped file is the stream
    void *map = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (map == MAP_FAILED) return fail(std::string(path) + ": cannot map the BAM file");
    struct Unmap {
      void *p;
      size_t n;
      ~Unmap() { munmap(p, n); }
    } unmap{map, (size_t)sb.st_size};
    (void)madvise(map, (size_t)sb.st_size, MADV_SEQUENTIAL);
    src.fd = -1;
    src.host = (const uint8_t *)map;
    return build_bam(c, src, path, accuracy_min, accuracy_max, out);
  }
  if (got < 2 || magic[0] != 0x1f || magic[1] != 0x8b) return build(c, src, accuracy_min, accuracy_max, out);
  // ---- gzip: BGZF is inflated by this GPU, and the bytes stay in its memory when they fit there; else as any gzip input
  src.fd = -1;
  const size_t size = (size_t)sb.st_size;
  void *map = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
  if (map == MAP_FAILED) return fail(std::string(path) + ": cannot map the gzip file");
  struct Unmap {
    void *p;
    size_t n;
    ~Unmap() { munmap(p, n); }
  } unmap{map, size};
  (void)madvise(map, size, MADV_SEQUENTIAL);
  const uint8_t *bytes = (const uint8_t *)map;
  DevBuf d_inflated;
  InputBytes gz;
  std::vector<BgzfMember> mem;
  const bool bgzf = bgzf_index(bytes, (int64_t)size, &mem);
  const int64_t total = bgzf ? bgzf_inflated_size(mem) : 0;
  if (bgzf && total > 0 && d_inflated.ensure((size_t)total + 16, true) == hipSuccess) {
    if (!inflate_members(c, bytes, mem, d_inflated.as<uint8_t>(), true)) return fail(std::string(path) + ": " + g_err);
    src.dev = d_inflated.as<uint8_t>();
    src.n = total;
    if (bam_ok && total >= 4) {
      uint8_t four[4];
      HIP_OK(hipMemcpy(four, src.dev, 4, hipMemcpyDeviceToHost));
      if (is_bam(four)) return build_bam(c, src, path, accuracy_min, accuracy_max, out);
    }
  } else {
    (void)hipGetLastError();
    pbsim_ctx *was = set_input_context(c);
    std::string e;
    const int g = open_input(path, &gz, &e);
    set_input_context(was);
    if (g <= 0) return fail(g < 0 ? e : std::string("Cannot open file: ") + path);
    src.host = (const uint8_t *)(gz.map ? gz.map : (const void *)"");
    src.n = (int64_t)gz.size;
    if (bam_ok && src.n >= 4 && is_bam(src.host)) return build_bam(c, src, path, accuracy_min, accuracy_max, out);
  }
  return build(c, src, accuracy_min, accuracy_max, out);
}
}  // namespace
}  // namespace pbsim

extern "C" {

int pbsim_set_sample_chunk_bytes(pbsim_ctx *c, int64_t bytes) {
  if (!c || bytes < 0) return fail("pbsim_set_sample_chunk_bytes: bad argument");
  c->sp_chunk_bytes = bytes == 0 ? 0 : std::min<int64_t>(std::max<int64_t>(bytes, 16), kMaxChunk);
  return PBSIM_SUCCEEDED;
}

int pbsim_sample_profile_from_bytes(pbsim_ctx *c, const void *fastq, int64_t n, double accuracy_min, double accuracy_max,
                                    pbsim_sample_stats *out) {
  if (!check_args(c, "pbsim_sample_profile_from_bytes", fastq || n == 0, n, accuracy_min, accuracy_max, out)) return PBSIM_FAILED;
  Source src;
  src.host = (const uint8_t *)(fastq ? fastq : (const void *)"");
  src.n = n;
  return build(c, src, accuracy_min, accuracy_max, out);
}

int pbsim_sample_profile_from_device(pbsim_ctx *c, const void *d_fastq, int64_t n, double accuracy_min, double accuracy_max,
                                     pbsim_sample_stats *out) {
  if (!check_args(c, "pbsim_sample_profile_from_device", d_fastq || n == 0, n, accuracy_min, accuracy_max, out)) return PBSIM_FAILED;
  if (n == 0) return pbsim_sample_profile_from_bytes(c, "", 0, accuracy_min, accuracy_max, out);
  Source src;
  src.dev = (const uint8_t *)d_fastq;
  src.n = n;
  return build(c, src, accuracy_min, accuracy_max, out);
}

int pbsim_load_sample_fastq(pbsim_ctx *c, const char *path, double accuracy_min, double accuracy_max, pbsim_sample_stats *out) {
  if (!check_args(c, "pbsim_load_sample_fastq", path != nullptr, 0, accuracy_min, accuracy_max, out)) return PBSIM_FAILED;
  return load_file(c, path, accuracy_min, accuracy_max, out, false);
}

int pbsim_load_sample(pbsim_ctx *c, const char *path, double accuracy_min, double accuracy_max, pbsim_sample_stats *out) {
  if (!check_args(c, "pbsim_load_sample", path != nullptr, 0, accuracy_min, accuracy_max, out)) return PBSIM_FAILED;
  return load_file(c, path, accuracy_min, accuracy_max, out, true);
}

int pbsim_sample_profile_from_bam_bytes(pbsim_ctx *c, const void *bam, int64_t n, double accuracy_min, double accuracy_max,
                                        pbsim_sample_stats *out) {
  if (!check_args(c, "pbsim_sample_profile_from_bam_bytes", bam || n == 0, n, accuracy_min, accuracy_max, out)) return PBSIM_FAILED;
  Source src;
  src.host = (const uint8_t *)(bam ? bam : (const void *)"");
  src.n = n;
  return build_bam(c, src, "BAM bytes", accuracy_min, accuracy_max, out);
}

int pbsim_sample_profile_from_bam_device(pbsim_ctx *c, const void *d_bam, int64_t n, double accuracy_min, double accuracy_max,
                                         pbsim_sample_stats *out) {
  if (!check_args(c, "pbsim_sample_profile_from_bam_device", d_bam || n == 0, n, accuracy_min, accuracy_max, out)) return PBSIM_FAILED;
  Source src;
  if (n == 0) src.host = (const uint8_t *)"";
  else src.dev = (const uint8_t *)d_bam;
  src.n = n;
  return build_bam(c, src, "BAM bytes", accuracy_min, accuracy_max, out);
}

int pbsim_sample_profile_text(pbsim_ctx *c, char *dst, int64_t cap, int64_t *bytes) {
  if (!c || !bytes || cap < 0) return fail("pbsim_sample_profile_text: bad argument");
  NEED_DEVICE(c);
  if (c->sq_len.empty()) return fail("no sample profile set (pbsim_set_sample_profile)");
  const size_t n = c->sq_len.size();
  *bytes = c->sq_total + (int64_t)n;
  if (!dst) return PBSIM_SUCCEEDED;
  if (cap < *bytes) return fail("pbsim_sample_profile_text: output buffer too small");
  HIP_OK(hipSetDevice(c->device));
  // the pool comes down in pieces through pinned staging, and its strings are squeezed into lines on the way
  const int64_t pool_bytes = c->sq_off[n - 1] + (((int64_t)c->sq_len[n - 1] + 7) & ~7LL);
  const int64_t piece = std::min<int64_t>(pool_bytes, (int64_t)64 << 20);
  HostBuf h;
  HIP_OK(h.ensure((size_t)std::max<int64_t>(piece, (kMaxQual + 7) & ~7LL)));
  size_t r = 0;
  char *to = dst;
  for (int64_t at = 0; r < n;) {
    // whole strings only: up to `piece` bytes from the pool offset of string r
    size_t e = r;
    int64_t end = at;
    while (e < n && c->sq_off[e] + (((int64_t)c->sq_len[e] + 7) & ~7LL) - at <= (int64_t)h.bytes) {
      end = c->sq_off[e] + (((int64_t)c->sq_len[e] + 7) & ~7LL);
      e++;
    }
    HIP_OK(hipMemcpy(h.p, c->d_sq.as<uint8_t>() + at, (size_t)(end - at), hipMemcpyDeviceToHost));
    for (; r < e; r++) {
      memcpy(to, (const char *)h.p + (c->sq_off[r] - at), (size_t)c->sq_len[r]);
      to += c->sq_len[r];
      *to++ = '\n';
    }
    at = end;
  }
  return PBSIM_SUCCEEDED;
}

}  // extern "C"
