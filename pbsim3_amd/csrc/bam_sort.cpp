// bam_sort.cpp -- pbsim_truth_bam_sort: a finished truth BAM (pbsim_set_truth_bam's records behind a header, BGZF) -> the same
// records in coordinate order, BGZF again, and the CSI index of that file.  The host's part: the member index, the index, and
// what to say when bam_chain.cpp's header parse or chain walk refuses the stream; the kernels are bam_scan.hip's,
// bam_sort.hip's, inflate.hip's and deflate.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "bam_scan.h"
#include "bam_sort.h"
#include "ctx.h"
#include "engine_internal.h"
#include "inflate_host.h"
#include "kernels.h"

namespace pbsim {

namespace {

const unsigned char kEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
constexpr int kMinShift = 14;

inline void put32(std::string *o, uint32_t v) {
  for (int k = 0; k < 4; k++) o->push_back((char)(v >> (8 * k)));
}
inline void put64(std::string *o, uint64_t v) {
  for (int k = 0; k < 8; k++) o->push_back((char)(v >> (8 * k)));
}

// device memory of this call alone: the stage's buffers are as large as the file, nothing of them is kept
int out_of_memory(const char *what, size_t want) {
  return fail(std::string("pbsim_truth_bam_sort: out of device memory: ") + what + " needs " + std::to_string(want) +
              " bytes (the stage holds the inflated stream, the sorted stream and their compressed pieces in HBM at once and does not chunk)");
}
int alloc(DevBuf &b, int64_t n, const char *what) {
  b.release();
  const size_t want = (size_t)std::max<int64_t>(n, 256);
  if (b.ensure(want, /*exact=*/true) != hipSuccess) {
    (void)hipGetLastError();
    return out_of_memory(what, want);
  }
  return PBSIM_SUCCEEDED;
}

const char *const kHeaderFault[] = {"",
                                    "shorter than a BAM header",
                                    "no BAM\\1 magic",
                                    "l_text runs past the end",
                                    "n_ref is negative",
                                    "the reference list runs past the end"};

// "SO:coordinate" into the @HD line of the header text (SAMv1 1.3: @HD is the first line where there is one)
std::string sorted_text(const std::string &t) {
  if (t.compare(0, 3, "@HD") != 0 || (t.size() > 3 && t[3] != '\t' && t[3] != '\n')) return "@HD\tVN:1.6\tSO:coordinate\n" + t;
  size_t eol = t.find('\n');
  if (eol == std::string::npos) eol = t.find('\0');
  if (eol == std::string::npos) eol = t.size();
  const size_t so = t.find("\tSO:", 3);
  if (so == std::string::npos || so >= eol) return t.substr(0, eol) + "\tSO:coordinate" + t.substr(eol);
  size_t fin = t.find('\t', so + 4);
  if (fin == std::string::npos || fin > eol) fin = eol;
  return t.substr(0, so + 4) + "coordinate" + t.substr(fin);
}

// CSIv1's reg2bin: the smallest bin of [beg, end) that holds it whole; bins of level l start at (8^l - 1) / 7
inline uint32_t reg2bin(int64_t beg, int64_t end, int depth) {
  end--;
  int s = kMinShift;
  int64_t t = (((int64_t)1 << (3 * depth)) - 1) / 7;
  for (int l = depth; l > 0; l--) {
    if (beg >> s == end >> s) return (uint32_t)(t + (beg >> s));
    s += 3;
    t -= (int64_t)1 << (3 * (l - 1));
  }
  return 0;
}
// the first coordinate a bin covers
inline int64_t bin_start(uint32_t bin, int depth) {
  int l = 0;
  int64_t t = 0;  // first bin of level l
  while (l < depth && (int64_t)bin >= t + ((int64_t)1 << (3 * l))) {
    t += (int64_t)1 << (3 * l);
    l++;
  }
  return ((int64_t)bin - t) << (kMinShift + 3 * (depth - l));
}

struct Clock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
  bool on = getenv("PBSIM_TRACE") != nullptr;
  void phase(const char *what, int64_t bytes = 0) {
    if (!on) return;
    const auto t = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t - last).count();
    fprintf(stderr, "[pbsim sort] %9.1f ms  %-22s", ms, what);
    if (bytes > 0 && ms > 0) fprintf(stderr, "  %8.1f MB  %7.2f GB/s", bytes / 1e6, bytes / ms / 1e6);
    fprintf(stderr, "\n");
    last = t;
  }
  void total() {
    if (on) fprintf(stderr, "[pbsim sort] %9.1f ms  total\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};

int sort_bam(pbsim_ctx *c, const uint8_t *src, int64_t n_src, const pbsim_sorted_bam_sink *sink, int64_t stats[4]) {
  Clock clk;
  hipStream_t st = c->stream;
  // ---- 1. inflate the whole file into HBM
  std::vector<BgzfMember> mem;
  if (!bgzf_index(src, n_src, &mem))
    return fail("pbsim_truth_bam_sort: not BGZF (every member a gzip member with a 'BC' extra field, SAMv1 4.1)");
  const int64_t N = bgzf_inflated_size(mem);
  DevBuf d_in;
  if (!alloc(d_in, N + kBamSlack, "the inflated stream")) return PBSIM_FAILED;
  HIP_OK(hipMemsetAsync(d_in.as<uint8_t>() + N, 0, (size_t)kBamSlack, st));
  if (!inflate_members(c, src, mem, d_in.as<uint8_t>(), true)) return PBSIM_FAILED;
  HIP_OK(hipStreamSynchronize(st));
  clk.phase("inflate", N);
  // the header: only its bytes travel back
  BamHeader hd;
  std::vector<uint8_t> hbytes;
  for (int64_t have = std::min<int64_t>(N, 64 << 10);; have = std::min<int64_t>(N, have * 4)) {
    hbytes.resize((size_t)have);
    if (have) HIP_OK(hipMemcpy(hbytes.data(), d_in.p, (size_t)have, hipMemcpyDeviceToHost));
    const int ok = bam_parse_header(hbytes.data(), have, N, true, &hd);
    if (ok > 0 && hd.empty_name) hd.fault = kBamHeaderRefs;
    if (ok < 0 || hd.fault) return fail(std::string("pbsim_truth_bam_sort: not a BAM file: ") + kHeaderFault[hd.fault]);
    if (ok > 0) break;
    if (have >= N) return fail("pbsim_truth_bam_sort: not a BAM file: the header runs past the end");
  }
  const int64_t H = hd.first_record;
  const uint8_t *stream = d_in.as<uint8_t>();
  // ---- 2. candidates: every byte position against the fixed fields, compacted in order; then the chain, from the first record:
  // a step must land on a candidate, the last one on the end of the stream
  std::vector<uint64_t> rec;  // the true records, packed as kBamSortPacking
  {
    std::vector<uint64_t> cand;
    {
      BamScan scan;
      const hipError_t e = scan.run(kBamScanPlaced, stream, H, N, (int32_t)hd.n_ref, st, &cand);
      if (e == hipErrorOutOfMemory && scan.oom_what) return out_of_memory(scan.oom_what, scan.oom_bytes);
      HIP_OK(e);
    }
    clk.phase("scan", N - H);
    int64_t stop = 0;
    if (bam_walk_chain(kBamSortPacking, cand.data(), cand.size(), H, N, true, &rec, &stop) != kBamChainDone) {
      char m[512];
      int k = snprintf(m, sizeof m,
                       "pbsim_truth_bam_sort: the record at inflated byte offset %lld does not fit (a placed single-end record: "
                       "0 <= refID < n_ref, pos >= 0, next_refID = next_pos = -1, tlen = 0, a block_size that covers its fields and "
                       "ends inside the stream of %lld bytes)",
                       (long long)stop, (long long)N);
      if (!rec.empty())
        snprintf(m + k, sizeof m - (size_t)k, "; the block_size %u of the record before it, at offset %lld, leads there",
                 (uint32_t)kBamSortPacking.size(rec.back()), (long long)kBamSortPacking.offset(rec.back()));
      return fail(m);
    }
    clk.phase("chain");
  }
  const int64_t n_rec = (int64_t)rec.size(), total = N - H;
  if (n_rec >= ((int64_t)1 << 32)) return fail("pbsim_truth_bam_sort: more than 2^32 - 1 records");
  // ---- 3, 4. keys and the stable sort; 5. the scan of the sorted sizes and the gather
  std::vector<uint64_t> key((size_t)n_rec);
  std::vector<int64_t> rend((size_t)n_rec), dst_off((size_t)n_rec + 1, 0);
  DevBuf d_out;
  if (!alloc(d_out, total + 64, "the sorted stream")) return PBSIM_FAILED;
  if (n_rec > 0) {
    DevBuf d_rec, d_key, d_key2, d_idx, d_perm, d_end, d_tmp;
    if (!alloc(d_rec, n_rec * 8, "the record list") || !alloc(d_key, n_rec * 8, "the keys") || !alloc(d_key2, n_rec * 8, "the sorted keys") ||
        !alloc(d_idx, n_rec * 4, "the record indices") || !alloc(d_perm, n_rec * 4, "the sorted indices") ||
        !alloc(d_end, n_rec * 8, "the end coordinates"))
      return PBSIM_FAILED;
    HIP_OK(hipMemcpyAsync(d_rec.p, rec.data(), (size_t)n_rec * 8, hipMemcpyHostToDevice, st));
    launch_bs_keys(stream, d_rec.as<uint64_t>(), n_rec, d_key.as<uint64_t>(), d_idx.as<uint32_t>(), d_end.as<int64_t>(), st);
    HIP_OK(hipGetLastError());
    int ref_bits = 1;
    while (ref_bits < 31 && ((int64_t)1 << ref_bits) < hd.n_ref) ref_bits++;
    size_t tb = 0;
    HIP_OK(bs_sort_pairs(nullptr, &tb, d_key.as<uint64_t>(), d_key2.as<uint64_t>(), d_idx.as<uint32_t>(), d_perm.as<uint32_t>(), n_rec,
                         32 + ref_bits, st));
    if (!alloc(d_tmp, (int64_t)tb, "the sort's scratch")) return PBSIM_FAILED;
    HIP_OK(bs_sort_pairs(d_tmp.p, &tb, d_key.as<uint64_t>(), d_key2.as<uint64_t>(), d_idx.as<uint32_t>(), d_perm.as<uint32_t>(), n_rec,
                         32 + ref_bits, st));
    HIP_OK(hipStreamSynchronize(st));
    clk.phase("keys and sort");
    // (d_key and d_idx have done their part: the sorted sizes and offsets take their places)
    DevBuf d_src, d_size, d_dst, d_ends;
    d_idx.release();
    if (!alloc(d_src, n_rec * 8, "the source offsets") || !alloc(d_size, n_rec * 8, "the sorted sizes") ||
        !alloc(d_dst, (n_rec + 1) * 8, "the destination offsets") || !alloc(d_ends, n_rec * 8, "the sorted end coordinates"))
      return PBSIM_FAILED;
    launch_bs_permute(d_rec.as<uint64_t>(), d_perm.as<uint32_t>(), d_end.as<int64_t>(), n_rec, d_src.as<int64_t>(), d_size.as<int64_t>(),
                      d_ends.as<int64_t>(), st);
    HIP_OK(hipGetLastError());
    if (!alloc(d_tmp, (n_rec / 1024 + 8) * 8, "the scan's scratch")) return PBSIM_FAILED;
    launch_exclusive_scan_i64(d_size.as<int64_t>(), d_dst.as<int64_t>(), n_rec, d_tmp.as<int64_t>(), d_dst.as<int64_t>() + n_rec, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(dst_off.data(), d_dst.p, (size_t)(n_rec + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(key.data(), d_key2.p, (size_t)n_rec * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(rend.data(), d_ends.p, (size_t)n_rec * 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (dst_off[(size_t)n_rec] != total) return fail("pbsim_truth_bam_sort: internal error: the sorted sizes do not add up to the stream");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    HIP_OK(hipEventRecord(e0, st));
    launch_bs_gather(stream, d_out.as<uint8_t>(), d_src.as<int64_t>(), d_dst.as<int64_t>(), n_rec, total, st);
    const hipError_t le = hipGetLastError();
    HIP_OK(hipEventRecord(e1, st));
    const hipError_t se = hipStreamSynchronize(st);
    float gather_ms = 0;
    (void)hipEventElapsedTime(&gather_ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIP_OK(le);
    HIP_OK(se);
    clk.phase("gather", total);
    if (clk.on && gather_ms > 0)
      fprintf(stderr, "[pbsim sort]   gather kernel alone: %.2f ms, %.1f GB/s of records moved (read + write: twice that)\n", gather_ms,
              total / gather_ms / 1e6);
  }
  d_in.release();  // the unsorted stream has been read for the last time
  // ---- 6. the header: SO:coordinate, members of its own
  std::string head("BAM\1", 4);
  {
    const std::string text = sorted_text(std::string((const char *)hbytes.data() + 8, (size_t)hd.l_text));
    put32(&head, (uint32_t)text.size());
    head += text;
    head.append((const char *)hbytes.data() + 8 + hd.l_text, (size_t)(H - 8 - hd.l_text));
  }
  std::vector<char> hz((size_t)pbsim_deflate_bound((int64_t)head.size()) + 64);
  int64_t hz_bytes = 0;
  if (!pbsim_deflate_buffer(c, head.data(), (int64_t)head.size(), hz.data(), (int64_t)hz.size(), &hz_bytes)) return PBSIM_FAILED;
  int64_t at = 0;  // bytes of the sorted file delivered
  auto send = [&](const char *z, int64_t k) -> int {
    if (k > 0 && sink->on_bam && !sink->on_bam(sink->user, z, k, at)) return fail("sink aborted (sorted BAM)");
    at += k;
    return PBSIM_SUCCEEDED;
  };
  if (!send(hz.data(), hz_bytes)) return PBSIM_FAILED;
  // ---- 7. the sorted records through the deflate lanes; the members' sizes are what the index's virtual offsets are made of
  std::vector<int64_t> m_c, m_u;  // per member of the record stream: compressed offset in the file, offset of its text in the stream
  std::vector<int32_t> m_len;
  {
    int64_t text_at = 0;
    std::vector<BgzfMember> pm;
    const int ok = deflate_pieces(c, c->slots[0].df[0], d_out.as<uint8_t>(), total, [&](const char *z, int64_t k) -> int {
      if (!bgzf_index((const uint8_t *)z, k, &pm)) return fail("pbsim_truth_bam_sort: internal error: a compressed piece is not whole members");
      for (const BgzfMember &m : pm) {
        if (m.isize > 0) {
          m_c.push_back(at + m.offset);
          m_u.push_back(text_at);
          m_len.push_back(m.isize);
        }
        text_at += m.isize;
      }
      return send(z, k);
    });
    if (!ok) return PBSIM_FAILED;
    if (text_at != total) return fail("pbsim_truth_bam_sort: internal error: the members do not add up to the sorted stream");
  }
  const int64_t eof_at = at;
  if (!send((const char *)kEof, sizeof kEof)) return PBSIM_FAILED;
  d_out.release();
  clk.phase("deflate and deliver", total);
  // ---- the CSI index (CSIv1): bins, chunks and loffsets from the sorted records' arrays
  auto voff = [&](int64_t o) -> uint64_t {  // of the record that starts at byte o of the sorted stream
    if (o >= total) return (uint64_t)eof_at << 16;
    const size_t m = (size_t)(std::upper_bound(m_u.begin(), m_u.end(), o) - m_u.begin()) - 1;
    return (uint64_t)m_c[m] << 16 | (uint64_t)(o - m_u[m]);
  };
  int64_t longest = 0;
  for (int64_t l : hd.ref_len) longest = std::max(longest, l);
  int depth = 5;
  while (((int64_t)1 << (kMinShift + 3 * depth)) < longest) depth++;
  std::string csi("CSI\1", 4);
  put32(&csi, kMinShift);
  put32(&csi, (uint32_t)depth);
  put32(&csi, 0);  // l_aux
  put32(&csi, (uint32_t)hd.n_ref);
  int64_t n_bins = 0, refs_with = 0;
  {
    struct Chunk {
      uint32_t bin;
      uint64_t beg, end;
    };
    std::vector<Chunk> chunks;
    std::vector<int64_t> pmax;
    int64_t i = 0;
    for (int64_t r = 0; r < hd.n_ref; r++) {
      const int64_t a = i;
      while (i < n_rec && (int64_t)(key[(size_t)i] >> 32) == r) i++;
      if (i == a) {
        put32(&csi, 0);
        continue;
      }
      refs_with++;
      chunks.clear();
      pmax.resize((size_t)(i - a));
      int64_t mx = 0;
      for (int64_t k = a; k < i;) {
        const uint32_t bin = reg2bin((int64_t)(uint32_t)key[(size_t)k], rend[(size_t)k], depth);
        int64_t e = k;
        while (e < i && reg2bin((int64_t)(uint32_t)key[(size_t)e], rend[(size_t)e], depth) == bin) {
          mx = std::max(mx, rend[(size_t)e]);
          pmax[(size_t)(e - a)] = mx;
          e++;
        }
        chunks.push_back(Chunk{bin, voff(dst_off[(size_t)k]), voff(dst_off[(size_t)e])});
        k = e;
      }
      std::stable_sort(chunks.begin(), chunks.end(), [](const Chunk &x, const Chunk &y) { return x.bin < y.bin; });
      int64_t nb = 0;
      for (size_t k = 0; k < chunks.size(); k++) nb += k == 0 || chunks[k].bin != chunks[k - 1].bin;
      n_bins += nb;
      put32(&csi, (uint32_t)(nb + 1));
      for (size_t k = 0; k < chunks.size();) {
        size_t e = k;
        while (e < chunks.size() && chunks[e].bin == chunks[k].bin) e++;
        // loffset: the first record of the reference, in file order, that ends behind the bin's first coordinate
        const int64_t s = bin_start(chunks[k].bin, depth);
        const int64_t first = std::upper_bound(pmax.begin(), pmax.end(), s) - pmax.begin();
        put32(&csi, chunks[k].bin);
        put64(&csi, voff(dst_off[(size_t)(a + first)]));
        put32(&csi, (uint32_t)(e - k));
        for (size_t q = k; q < e; q++) {
          put64(&csi, chunks[q].beg);
          put64(&csi, chunks[q].end);
        }
        k = e;
      }
      put32(&csi, (uint32_t)((((int64_t)1 << (3 * (depth + 1))) - 1) / 7 + 1));  // the metadata pseudo-bin
      put64(&csi, 0);
      put32(&csi, 2);
      put64(&csi, voff(dst_off[(size_t)a]));
      put64(&csi, voff(dst_off[(size_t)i]));
      put64(&csi, (uint64_t)(i - a));  // n_mapped
      put64(&csi, 0);                  // n_unmapped
    }
    if (i != n_rec) return fail("pbsim_truth_bam_sort: internal error: the sorted keys do not end with the last reference");
  }
  put64(&csi, 0);  // n_no_coor
  std::vector<char> cz((size_t)pbsim_deflate_bound((int64_t)csi.size()) + 64 + sizeof kEof);
  int64_t cz_bytes = 0;
  if (!pbsim_deflate_buffer(c, csi.data(), (int64_t)csi.size(), cz.data(), (int64_t)cz.size() - (int64_t)sizeof kEof, &cz_bytes)) return PBSIM_FAILED;
  memcpy(cz.data() + cz_bytes, kEof, sizeof kEof);
  cz_bytes += sizeof kEof;
  clk.phase("index");
  clk.total();
  if (stats) {
    stats[0] = n_rec;
    stats[1] = refs_with;
    stats[2] = total;
    stats[3] = n_bins;
  }
  if (sink->on_index && !sink->on_index(sink->user, cz.data(), cz_bytes)) return fail("sink aborted (index)");
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_truth_bam_sort(pbsim_ctx *c, const void *bam, int64_t n, const pbsim_sorted_bam_sink *sink, int64_t stats[4]) {
  if (!c || !sink || n < 0 || (n > 0 && !bam)) return fail("pbsim_truth_bam_sort: bad argument");
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::sort_bam(c, (const uint8_t *)bam, n, sink, stats);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
  }
  return ok;
}
