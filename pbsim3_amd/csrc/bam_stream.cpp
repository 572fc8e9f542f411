// bam_stream.cpp -- a BAM file into HBM and its records located (bam_stream.h): the containers, the header, and what to say
// when bam_chain.cpp's header parse or chain walk refuses a stream.  The kernels are inflate.hip's and bam_scan.hip's.
#include "bam_stream.h"

#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>

#include "bam_eval.h"
#include "inflate_host.h"

namespace pbsim {

namespace {

const char *const kHeaderFault[] = {"",
                                    "shorter than a BAM header",
                                    "no BAM\\1 magic",
                                    "l_text runs past the end",
                                    "n_ref is negative",
                                    "the reference list runs past the end"};

// one gzip stream (concatenated members are one stream) through zlib
bool gunzip(const uint8_t *src, int64_t n, std::vector<uint8_t> *out, std::string *err) {
  z_stream z;
  memset(&z, 0, sizeof z);
  if (inflateInit2(&z, 16 + MAX_WBITS) != Z_OK) {
    *err = "zlib: inflateInit2 failed";
    return false;
  }
  out->clear();
  std::vector<uint8_t> piece((size_t)4 << 20);
  int64_t at = 0;
  for (;;) {
    const int64_t take = std::min<int64_t>(n - at, (int64_t)1 << 30);
    z.next_in = const_cast<Bytef *>(src + at);
    z.avail_in = (uInt)take;
    z.next_out = piece.data();
    z.avail_out = (uInt)piece.size();
    const int rc = inflate(&z, Z_NO_FLUSH);
    at += take - (int64_t)z.avail_in;
    out->insert(out->end(), piece.data(), piece.data() + (piece.size() - z.avail_out));
    if (rc == Z_STREAM_END) {
      if (at >= n) break;
      if (inflateReset(&z) == Z_OK) continue;  // the next member
    } else if (rc == Z_OK && (at < n || z.avail_out == 0)) {
      continue;  // more input to give, or more output to take
    }
    // no progress is possible: the data is damaged, or it breaks off
    *err = std::string("gzip data does not inflate: ") + (z.msg ? z.msg : "it breaks off");
    inflateEnd(&z);
    return false;
  }
  inflateEnd(&z);
  return true;
}

std::string prefix(const BamStage &g, const BamStream &s) { return s.what.empty() ? g.who : g.who + s.what + ": "; }

}  // namespace

int bam_stage_oom(const BamStage &g, const char *what, size_t want) {
  return fail(g.who + "out of device memory: " + what + " needs " + std::to_string(want) + " bytes (" + g.holds + ")");
}

int bam_stage_alloc(const BamStage &g, DevBuf &b, int64_t n, const char *what) {
  b.release();
  const size_t want = (size_t)std::max<int64_t>(n, 256);
  if (b.ensure(want, /*exact=*/true) != hipSuccess) {
    (void)hipGetLastError();
    return bam_stage_oom(g, what, want);
  }
  return PBSIM_SUCCEEDED;
}

// the container: BGZF is inflated on the GPU, one plain gzip stream by zlib on the host, "BAM\1" is the stream itself
int bam_inflate_stream(pbsim_ctx *c, const BamStage &g, const uint8_t *src, int64_t n, BamStream *s) {
  hipStream_t st = c->stream;
  const std::string who = prefix(g, *s);
  std::vector<BgzfMember> mem;
  std::vector<uint8_t> host;
  const uint8_t *plain = nullptr;
  if (n >= 4 && memcmp(src, "BAM\1", 4) == 0) {
    plain = src;
    s->N = n;
  } else if (n >= 2 && src[0] == 0x1f && src[1] == 0x8b) {
    if (bgzf_index(src, n, &mem)) {
      s->N = bgzf_inflated_size(mem);
    } else {
      std::string err;
      if (!gunzip(src, n, &host, &err)) return fail(who + err);
      plain = host.data();
      s->N = (int64_t)host.size();
    }
  } else {
    return fail(who + "neither BGZF, gzip nor an uncompressed BAM stream");
  }
  if (!bam_stage_alloc(g, s->d, s->N + kBamSlack, "an inflated stream")) return PBSIM_FAILED;
  uint8_t *d = s->d.as<uint8_t>();
  HIP_OK(hipMemsetAsync(d + s->N, 0, (size_t)kBamSlack, st));
  if (plain) {
    if (s->N > 0) HIP_OK(hipMemcpyAsync(d, plain, (size_t)s->N, hipMemcpyHostToDevice, st));
  } else if (!inflate_members(c, src, mem, d, true)) {
    return fail(who + g_err);
  }
  HIP_OK(hipStreamSynchronize(st));  // (`host` goes with this frame)
  return PBSIM_SUCCEEDED;
}

// the header, then the records: the scan's candidates and the chain over them
int bam_locate(pbsim_ctx *c, const BamStage &g, BamStream *s, BamScan *scan, BamScanPolicy policy, BamPacking pk) {
  hipStream_t st = c->stream;
  const std::string who = prefix(g, *s);
  const int64_t N = s->N;
  if (pk.size_bits > 24 && N >= ((int64_t)1 << (64 - pk.size_bits)))
    return fail(who + std::to_string(N) + " inflated bytes: " + s->a_what +
                " of 2^36 bytes or more is not taken (its records are packed as offset << 28 | block_size)");
  std::vector<uint8_t> hbytes;
  for (int64_t have = std::min<int64_t>(N, 64 << 10);; have = std::min<int64_t>(N, have * 4)) {
    hbytes.resize((size_t)have);
    if (have) HIP_OK(hipMemcpy(hbytes.data(), s->d.p, (size_t)have, hipMemcpyDeviceToHost));
    const int ok = bam_parse_header(hbytes.data(), have, N, true, &s->hd);
    if (ok < 0 || s->hd.fault) return fail(who + "not a BAM file: " + kHeaderFault[s->hd.fault]);
    if (ok > 0) break;
    if (have >= N) return fail(who + "not a BAM file: the header runs past the end");
  }
  bam_ref_names(hbytes.data(), s->hd, &s->ref_names);
  s->H = s->hd.first_record;
  std::vector<uint64_t> cand;
  const hipError_t e = scan->run(policy, s->bytes(), s->H, N, (int32_t)s->hd.n_ref, st, &cand);
  if (e == hipErrorOutOfMemory && scan->oom_what) return bam_stage_oom(g, scan->oom_what, scan->oom_bytes);
  HIP_OK(e);
  int64_t stop = 0;
  s->rec.clear();
  if (bam_walk_chain(pk, cand.data(), cand.size(), s->H, N, true, &s->rec, &stop) != kBamChainDone) {
    char m[640];
    int k = snprintf(m, sizeof m, "the record at inflated byte offset %lld does not fit (%s, l_seq >= 0, a block_size that covers its fields and ends "
                                  "inside the stream of %lld bytes)",
                     (long long)stop,
                     policy == kBamScanPlaced ? "a placed single-end record of a truth BAM: 0 <= refID < n_ref, pos >= 0, next_refID = next_pos = -1, tlen = 0"
                                              : "refID and next_refID in [-1, n_ref), pos and next_pos >= -1, a read name that ends with a NUL",
                     (long long)N);
    if (!s->rec.empty())
      snprintf(m + k, sizeof m - (size_t)k, "; the block_size %u of the record before it, at offset %lld, leads there", (uint32_t)pk.size(s->rec.back()),
               (long long)pk.offset(s->rec.back()));
    return fail(who + m);
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace pbsim
