// inflate_host.cpp -- the host side of inflate.hip: the BGZF member index (headers only, no decoding), the piece pipeline
// (pinned staging -> HBM -> kernel -> HBM -> pinned staging, two streams, two buffer sets) and the ABI entries
// pbsim_inflate_bound / pbsim_inflate_buffer.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "ctx.h"
#include "engine_internal.h"
#include "inflate_host.h"

namespace pbsim {

namespace {
inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const uint8_t *p) { return le16(p) | le16(p + 2) << 16; }

// output bytes per piece (and compressed bytes: a piece ends at whichever bound it reaches first).  PBSIM_INFLATE_PIECE_KB is
// a test hook: small pieces put the pipeline's seams inside small files.
int64_t piece_bytes() {
  static const int64_t v = [] {
    const char *e = getenv("PBSIM_INFLATE_PIECE_KB");
    const int64_t kb = e && atoll(e) > 0 ? atoll(e) : (int64_t)256 << 10;
    return std::max<int64_t>(64, kb) << 10;
  }();
  return v;
}
// f(a, e) over [0, n) in up to eight ranges on as many threads: the copies into and out of pinned staging are
// the host's share of an inflate (a piece's output is 256 MiB, and the destination's pages are touched for the first time)
template <class F>
void parallel_ranges(size_t n, size_t min_per_thread, F &&f) {
  const size_t nt = std::max<size_t>(1, std::min<size_t>(8, n / std::max<size_t>(1, min_per_thread)));
  if (nt <= 1) {
    f((size_t)0, n);
    return;
  }
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; t++) th.emplace_back([&, t]() { f(n * t / nt, n * (t + 1) / nt); });
  f((size_t)0, n / nt);
  for (auto &x : th) x.join();
}
}  // namespace

bool bgzf_index(const uint8_t *p, int64_t n, std::vector<BgzfMember> *out) {
  out->clear();
  int64_t o = 0, out_off = 0;
  while (o < n) {
    if (n - o < 18) return false;                                   // header (12) + the BC subfield (6)
    const uint8_t *h = p + o;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) return false;    // magic, CM = deflate
    const uint8_t flg = h[3];
    if (!(flg & 4) || (flg & 0xe0)) return false;                  // FEXTRA, no reserved bits
    const int64_t xlen = le16(h + 10);
    if (12 + xlen > n - o) return false;
    int64_t bsize = -1;
    for (int64_t x = 12; x + 4 <= 12 + xlen;) {                     // subfields: SI1 SI2 SLEN data
      const int64_t slen = le16(h + x + 2);
      if (x + 4 + slen > 12 + xlen) return false;
      if (h[x] == 'B' && h[x + 1] == 'C' && slen == 2 && bsize < 0) bsize = le16(h + x + 4);
      x += 4 + slen;
    }
    if (bsize < 0) return false;
    const int64_t end = o + bsize + 1;                              // BSIZE = member bytes - 1
    if (end > n) return false;
    int64_t data = o + 12 + xlen;
    if (flg & 8)                                                    // FNAME, FCOMMENT: zero-terminated
      while (data < end && p[data++]) {}
    if (flg & 16)
      while (data < end && p[data++]) {}
    if (flg & 2) data += 2;                                         // FHCRC
    if (data > end - 8) return false;
    const uint32_t isize = le32(p + end - 4);
    if (isize > 65536) return false;
    BgzfMember m;
    m.offset = o;
    m.data = data;
    m.data_len = (int32_t)(end - 8 - data);
    m.isize = (int32_t)isize;
    m.crc = le32(p + end - 8);
    m.out_off = out_off;
    out->push_back(m);
    out_off += isize;
    o = end;
  }
  return true;
}

int64_t bgzf_inflated_size(const std::vector<BgzfMember> &mem) {
  return mem.empty() ? 0 : mem.back().out_off + mem.back().isize;
}

// the members of src (indexed by bgzf_index) -> dst[0 .. inflated size), on the GPU, piece by piece: the host fills the
// pinned input staging of piece k while the GPU decodes piece k - 1 and piece k - 2's output travels back (two buffer sets)
// dst_on_device: dst is memory of the context's GPU -- a piece's output goes there GPU to GPU and only its status words travel
int inflate_members(pbsim_ctx *c, const uint8_t *src, const std::vector<BgzfMember> &mem, uint8_t *dst, bool dst_on_device) {
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  if (mem.empty()) return PBSIM_SUCCEEDED;
  // ---- the pieces: [first member, end member)
  const int64_t cap = piece_bytes();
  std::vector<size_t> cut{0};
  {
    int64_t in = 0, out = 0;
    for (size_t i = 0; i < mem.size(); i++) {
      const int64_t mi = mem[i].data_len, mo = mem[i].isize;
      if (i > cut.back() && (in + mi > cap || out + mo > cap)) {
        cut.push_back(i);
        in = out = 0;
      }
      in += mi;
      out += mo;
    }
    cut.push_back(mem.size());
  }
  const size_t n_pieces = cut.size() - 1;
  // ---- tables, buffers, streams, events
  if (!ensure_crc_tables(c)) return PBSIM_FAILED;  // (deflate.hip's CRC-32 and pow128 tables: one copy for both directions)
  const uint32_t *tab = c->d_df_tables.as<uint32_t>();
  struct Set {
    HostBuf h_in, h_out;   // pinned: [member descriptors | compressed bytes], [output | status words]
    DevBuf d_in, d_out;
    hipEvent_t up = nullptr, k0 = nullptr, k1 = nullptr, down = nullptr;
    int64_t n_mem = 0, out_bytes = 0, status_off = 0;
    size_t first = 0;
    bool busy = false;
  } sets[2];
  hipStream_t s_work = nullptr, s_copy = nullptr;
  struct Cleanup {  // whatever happens: nothing in flight when the buffers go
    Set *s;
    hipStream_t *a, *b;
    ~Cleanup() {
      for (hipStream_t *st : {a, b})
        if (*st) {
          (void)hipStreamSynchronize(*st);
          (void)hipStreamDestroy(*st);
        }
      for (int i = 0; i < 2; i++)
        for (hipEvent_t e : {s[i].up, s[i].k0, s[i].k1, s[i].down})
          if (e) (void)hipEventDestroy(e);
    }
  } cleanup{sets, &s_work, &s_copy};
  HIP_OK(hipStreamCreateWithFlags(&s_work, hipStreamNonBlocking));
  HIP_OK(hipStreamCreateWithFlags(&s_copy, hipStreamNonBlocking));
  for (Set &s : sets) {
    HIP_OK(hipEventCreateWithFlags(&s.up, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&s.down, hipEventDisableTiming));
    HIP_OK(hipEventCreate(&s.k0));
    HIP_OK(hipEventCreate(&s.k1));
  }
  const bool trace = getenv("PBSIM_INFLATE_TRACE") != nullptr;
  const auto now = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_begin = now();
  double kernel_ms = 0;
  int64_t in_total = 0, out_total = 0;
  // piece k's output (its download done) -> dst, and its status words checked: the first failing member fails the call
  auto finish = [&](Set &s) -> int {
    HIP_OK(hipEventSynchronize(s.down));
    s.busy = false;
    float ms = 0;
    if (hipEventElapsedTime(&ms, s.k0, s.k1) == hipSuccess) kernel_ms += ms;
    const int32_t *st = reinterpret_cast<const int32_t *>((const uint8_t *)s.h_out.p + s.status_off);
    for (int64_t i = 0; i < s.n_mem; i++)
      if (st[i] != kInfOk) {
        char m[160];
        snprintf(m, sizeof m, "gzip member at byte offset %lld: %s", (long long)mem[s.first + (size_t)i].offset, inflate_reason(st[i]));
        return fail(m);
      }
    if (dst_on_device) return PBSIM_SUCCEEDED;
    uint8_t *to = dst + mem[s.first].out_off;
    const uint8_t *from = (const uint8_t *)s.h_out.p;
    parallel_ranges((size_t)s.out_bytes, (size_t)16 << 20, [&](size_t a, size_t e) { memcpy(to + a, from + a, e - a); });
    return PBSIM_SUCCEEDED;
  };
  auto download = [&](Set &s) -> int {
    HIP_OK(hipStreamWaitEvent(s_copy, s.k1, 0));
    if (dst_on_device) {
      HIP_OK(hipMemcpyAsync(dst + mem[s.first].out_off, s.d_out.p, (size_t)s.out_bytes, hipMemcpyDeviceToDevice, s_copy));
      HIP_OK(hipMemcpyAsync((uint8_t *)s.h_out.p + s.status_off, s.d_out.as<uint8_t>() + s.status_off, (size_t)(s.n_mem * 4),
                            hipMemcpyDeviceToHost, s_copy));
    } else {
      HIP_OK(hipMemcpyAsync(s.h_out.p, s.d_out.p, (size_t)(s.status_off + s.n_mem * 4), hipMemcpyDeviceToHost, s_copy));
    }
    HIP_OK(hipEventRecord(s.down, s_copy));
    return PBSIM_SUCCEEDED;
  };
  for (size_t k = 0; k < n_pieces; k++) {
    Set &s = sets[k & 1];
    if (s.busy && !finish(s)) return PBSIM_FAILED;  // piece k - 2: its buffers are free from here on
    const size_t a = cut[k], e = cut[k + 1];
    const int64_t nm = (int64_t)(e - a);
    const int64_t desc_bytes = (nm * (int64_t)sizeof(InflateMember) + 15) & ~(int64_t)15;
    int64_t in_bytes = 0;
    for (size_t i = a; i < e; i++) in_bytes += mem[i].data_len;
    const int64_t out_bytes = mem[e - 1].out_off + mem[e - 1].isize - mem[a].out_off;
    const int64_t status_off = (out_bytes + 15) & ~(int64_t)15;
    HIP_OK(s.h_in.ensure((size_t)(desc_bytes + in_bytes + 16)));
    HIP_OK(s.d_in.ensure((size_t)(desc_bytes + in_bytes + 16)));
    HIP_OK(s.h_out.ensure((size_t)(status_off + nm * 4)));
    HIP_OK(s.d_out.ensure((size_t)(status_off + nm * 4)));
    // the piece's deflate data packed back to back (headers and trailers stay on the host), its descriptors in front
    InflateMember *d = reinterpret_cast<InflateMember *>(s.h_in.p);
    uint8_t *z = (uint8_t *)s.h_in.p + desc_bytes;
    int64_t zo = 0;
    for (size_t i = a; i < e; i++) {
      const BgzfMember &m = mem[i];
      d[i - a] = InflateMember{zo, m.out_off - mem[a].out_off, m.data_len, m.isize, m.crc, 0};
      zo += m.data_len;
    }
    parallel_ranges((size_t)nm, 256, [&](size_t x, size_t y) {
      for (size_t i = x; i < y; i++) memcpy(z + d[i].in_off, src + mem[a + i].data, (size_t)d[i].in_len);
    });
    memset(z + zo, 0, 16);
    // one copy stream, in the order up(k), down(k - 1): the upload of piece k runs beside the kernel of piece k - 1, and the
    // download of piece k - 1 beside the kernel of piece k
    HIP_OK(hipMemcpyAsync(s.d_in.p, s.h_in.p, (size_t)(desc_bytes + in_bytes + 16), hipMemcpyHostToDevice, s_copy));
    HIP_OK(hipEventRecord(s.up, s_copy));
    HIP_OK(hipStreamWaitEvent(s_work, s.up, 0));
    HIP_OK(hipEventRecord(s.k0, s_work));
    uint8_t *dout = s.d_out.as<uint8_t>();
    launch_inflate(s.d_in.as<uint8_t>() + desc_bytes, s.d_in.as<InflateMember>(), nm, dout,
                   reinterpret_cast<int32_t *>(dout + status_off), tab, tab + 1024, s_work);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(s.k1, s_work));
    s.n_mem = nm;
    s.out_bytes = out_bytes;
    s.status_off = status_off;
    s.first = a;
    s.busy = true;
    in_total += in_bytes;
    out_total += out_bytes;
    if (k > 0 && !download(sets[(k - 1) & 1])) return PBSIM_FAILED;
  }
  if (!download(sets[(n_pieces - 1) & 1])) return PBSIM_FAILED;
  for (size_t k = n_pieces; k < n_pieces + 2; k++) {  // the last two pieces, in order
    Set &s = sets[k & 1];
    if (s.busy && !finish(s)) return PBSIM_FAILED;
  }
  if (trace)
    fprintf(stderr, "[inflate] %zu members, %zu pieces: %.1f MB -> %.1f MB in %.1f ms, kernels %.1f ms (%.2f GB/s of output)\n",
            mem.size(), n_pieces, in_total / 1e6, out_total / 1e6, now() - t_begin, kernel_ms,
            kernel_ms > 0 ? out_total / kernel_ms / 1e6 : 0.0);
  return PBSIM_SUCCEEDED;
}

}  // namespace pbsim

extern "C" {

int64_t pbsim_inflate_bound(const void *src, int64_t n) {
  if (n < 0 || (n > 0 && !src)) return -1;
  std::vector<pbsim::BgzfMember> mem;
  if (!pbsim::bgzf_index((const uint8_t *)src, n, &mem)) return -1;
  return pbsim::bgzf_inflated_size(mem);
}

int pbsim_inflate_buffer(pbsim_ctx *c, const void *src, int64_t n, void *dst, int64_t cap, int64_t *out_bytes) {
  if (!c || !out_bytes || n < 0 || (n > 0 && !src)) return fail("pbsim_inflate_buffer: bad argument");
  *out_bytes = 0;
  std::vector<pbsim::BgzfMember> mem;
  if (!pbsim::bgzf_index((const uint8_t *)src, n, &mem))
    return fail("pbsim_inflate_buffer: not BGZF (every member a gzip member with a 'BC' extra field, SAMv1 4.1)");
  const int64_t total = pbsim::bgzf_inflated_size(mem);
  if (total > cap || (total > 0 && !dst)) return fail("pbsim_inflate_buffer: output buffer too small");
  NEED_DEVICE(c);
  if (!pbsim::inflate_members(c, (const uint8_t *)src, mem, (uint8_t *)dst)) return PBSIM_FAILED;
  *out_bytes = total;
  return PBSIM_SUCCEEDED;
}

}  // extern "C"
