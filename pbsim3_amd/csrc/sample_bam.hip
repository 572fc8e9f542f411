// sample_bam.hip -- the sampling method's profile from BAM bytes in HBM (unaligned or aligned): where the records start, every
// counted record's ordered sum of error probabilities, and the quality strings that pass the filter packed into the pool
// k_walk_sample reads -- the profile sample_profile.hip makes from the FASTQ `samtools fastq` would write.  The host side
// (header, windows, the chain walk that decides, statistics, errors) is sample_profile.cpp and bam_chain.cpp.
//
//   scan   : bam_scan.hip, with the policy "any record"; the host walks the chain over its candidates.
//   sums   : one LANE per record of the chain (k_sp_sums's shape): flag 0x900 -> skipped; a first quality byte 0xFF -> no
//            qualities; else the host's additions in READ order -- backward through memory for flag 0x10 -- of a table in LDS
//            indexed by the byte (qprob[min(q, 93)]), sixteen-byte loads between the unaligned ends of the string.
//   pool   : one wave per kept string, 8 bytes per lane and step, the source realigned (and for 0x10 byte-swapped) in
//            registers, min(q, 93) + 33 on the eight bytes at once, pad bytes 0: k_sp_pool's layout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bam_chain.h"
#include "bam_fields.h"
#include "kernels.h"

namespace pbsim {

namespace {

constexpr BamPacking kPk = kBamSamplePacking;

#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void k_sb_sums(const uint8_t *buf, const uint64_t *rec, int64_t n_rec, int32_t len_min, int32_t len_max,
                                                 double acc_min, double acc_max, const double *qprob, uint32_t *qual_at, int32_t *rec_len,
                                                 int32_t *status, double *accuracy, int64_t *padded) {
  // indexed by the quality byte itself: qprob[min(q, 93)] -- no test per base
  __shared__ double s_qp[256];
  {
    const int i = threadIdx.x;
    s_qp[i] = qprob[i > 93 ? 93 : i];
  }
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rec) return;
  const int64_t at = kPk.offset(rec[r]);
  const uint8_t *h = buf + at;
  const uint32_t l_read_name = h[kBamLReadName], n_cigar_op = ld16(h + kBamNCigarOp), flag = ld16(h + kBamFlag);
  const int32_t len = (int32_t)ld32(h + kBamLSeq);
  // (the chain walk took this record from the scan: its block_size covers the qualities)
  const int64_t start = at + kBamFixed + (int64_t)l_read_name + 4 * (int64_t)n_cigar_op + ((int64_t)len + 1) / 2;
  int32_t st = kSbCounted;
  if (flag & 0x900u) st = kSbSkipped;
  else if (len > 0 && buf[start] == 0xffu) st = kSbNoQual;
  double acc = 0.0;
  int64_t pad = 0;
  if (st == kSbCounted && len >= len_min && len <= len_max) {
    const uint8_t *p = buf + start;
    const bool rev = (flag & 0x10u) != 0;
    double prob = 0.0;
    int32_t head = (int32_t)((16u - ((uint32_t)start & 15u)) & 15u);  // bytes in front of the first 16-byte boundary
    head = head < len ? head : len;
    const int32_t n_q = (len - head) >> 4, tail = head + (n_q << 4);
    const uint4 *p4 = reinterpret_cast<const uint4 *>(p + head);
    if (!rev) {
      for (int32_t i = 0; i < head; i++) prob += s_qp[p[i]];
      // 64 qualities per turn as four 16-byte loads (a lane's loads are its own record's: few, wide loads)
      for (int32_t g0 = 0; g0 < n_q; g0 += 4) {
        uint4 v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = (g0 + i < n_q) ? p4[g0 + i] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          if (g0 + i < n_q) {
            const uint32_t w4[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
            double qp[16];
#pragma unroll
            for (int d = 0; d < 4; d++)
#pragma unroll
              for (int j = 0; j < 4; j++) qp[d * 4 + j] = s_qp[(w4[d] >> (8 * j)) & 0xffu];
#pragma unroll
            for (int k = 0; k < 16; k++) prob += qp[k];  // in read order
          }
        }
      }
      for (int32_t i = tail; i < len; i++) prob += s_qp[p[i]];
    } else {  // the read's first base is the record's last quality byte
      for (int32_t i = len - 1; i >= tail; i--) prob += s_qp[p[i]];
      for (int32_t g0 = n_q - 1; g0 >= 0; g0 -= 4) {
        uint4 v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = (g0 - i >= 0) ? p4[g0 - i] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          if (g0 - i >= 0) {
            const uint32_t w4[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
            double qp[16];
#pragma unroll
            for (int d = 0; d < 4; d++)
#pragma unroll
              for (int j = 0; j < 4; j++) qp[d * 4 + j] = s_qp[(w4[d] >> (8 * j)) & 0xffu];
#pragma unroll
            for (int k = 15; k >= 0; k--) prob += qp[k];  // in read order
          }
        }
      }
      for (int32_t i = head - 1; i >= 0; i--) prob += s_qp[p[i]];
    }
    acc = 1.0 - (prob / (double)len);
    if (acc >= acc_min && acc <= acc_max) pad = ((int64_t)len + 7) & ~(int64_t)7;
  }
  qual_at[r] = (uint32_t)start;
  rec_len[r] = st == kSbSkipped ? 0 : len;
  status[r] = st;
  accuracy[r] = acc;
  padded[r] = pad;
}

// min(q, 93) + 33 on eight bytes: 0x80 where a byte is 94 or more (no carry crosses a byte: 127 + 34 < 256)
__device__ __forceinline__ uint64_t fastq_chars(uint64_t v) {
  const uint64_t big = (((v & 0x7f7f7f7f7f7f7f7full) + 0x2222222222222222ull) | v) & 0x8080808080808080ull;
  const uint64_t m = (big >> 7) * 0xffull;
  return ((v & ~m) | (0x5d5d5d5d5d5d5d5dull & m)) + 0x2121212121212121ull;
}

__global__ __launch_bounds__(256) void k_sb_pool(const uint8_t *buf, const uint64_t *rec, const uint32_t *qual_at, const int32_t *rec_len,
                                                 const int64_t *padded, const int64_t *off, int64_t n_rec, uint8_t *pool) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * 4;
  for (int64_t r = wave; r < n_rec; r += n_waves) {
    const int64_t words = padded[r] >> 3;
    if (words == 0) continue;
    const int64_t start = qual_at[r], len = rec_len[r];
    const bool rev = (ld16(buf + kPk.offset(rec[r]) + kBamFlag) & 0x10u) != 0;
    uint64_t *dst = reinterpret_cast<uint64_t *>(pool + off[r]);
    for (int64_t w = lane; w < words; w += 64) {
      // the eight source bytes of this word begin at s: behind the string's start by up to 7 bytes for the last word of a
      // reversed string (the record's own bytes), and up to 15 bytes behind its end (the buffer's slack)
      const int64_t s = rev ? start + len - 8 - w * 8 : start + w * 8;
      const int sh = (int)(s & 7) * 8;
      const uint64_t *src = reinterpret_cast<const uint64_t *>(buf + (s - (s & 7)));
      uint64_t v = src[0];
      if (sh) v = (v >> sh) | (src[1] << (64 - sh));
      if (rev) v = __builtin_bswap64(v);
      v = fastq_chars(v);
      const int64_t rem = len - w * 8;
      if (rem < 8) v &= (1ull << (8 * rem)) - 1ull;  // the pad bytes are 0
      dst[w] = v;
    }
  }
}

}  // namespace

void launch_sb_sums(const uint8_t *buf, const uint64_t *rec, int64_t n_rec, int32_t len_min, int32_t len_max, double acc_min, double acc_max,
                    const double *qprob, uint32_t *qual_at, int32_t *rec_len, int32_t *status, double *accuracy, int64_t *padded,
                    hipStream_t s) {
  if (n_rec <= 0) return;
  hipLaunchKernelGGL(k_sb_sums, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s, buf, rec, n_rec, len_min, len_max, acc_min, acc_max,
                     qprob, qual_at, rec_len, status, accuracy, padded);
}

void launch_sb_pool(const uint8_t *buf, const uint64_t *rec, const uint32_t *qual_at, const int32_t *rec_len, const int64_t *padded,
                    const int64_t *off, int64_t n_rec, uint8_t *pool, hipStream_t s) {
  if (n_rec <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>((n_rec + 3) / 4, 1), kSpBlocksMax);
  hipLaunchKernelGGL(k_sb_pool, dim3(grid), dim3(256), 0, s, buf, rec, qual_at, rec_len, padded, off, n_rec, pool);
}

}  // namespace pbsim
