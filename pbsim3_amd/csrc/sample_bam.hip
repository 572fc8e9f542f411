// sample_bam.hip -- the sampling method's profile from BAM bytes in HBM (unaligned or aligned): where the records start, every
// counted record's ordered sum of error probabilities, and the quality strings that pass the filter packed into the pool
// k_walk_sample reads -- the profile sample_profile.hip makes from the FASTQ `samtools fastq` would write.  The host side
// (header, windows, the chain walk that decides, statistics, errors) is sample_profile.cpp and bam_chain.cpp.
//
//   scan   : BAM records are chained by block_size, and a chain is serial.  Every BYTE position is tested instead, in
//            parallel (k_bs_scan's shape: a 4 KiB tile plus a halo staged in LDS, a count pass and a write pass behind an
//            exclusive scan so the hits come out ascending).  A general record has no constant bytes, so the test is on
//            its fields: refID, next_refID in [-1, n_ref), pos, next_pos >= -1, l_read_name >= 1 with a NUL as the name's last
//            byte, l_seq >= 0, block_size >= 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq and <= kBamMaxBlock, the
//            record inside the bytes.  A lane holds the 64 bytes around its sixteen positions in registers and takes the
//            unaligned fields out of them with v_alignbyte; only the name's last byte is read from HBM, for the few positions
//            that come so far.  The hits are a SUPERSET of the record starts (a B array that holds a record image passes).
//   sums   : one LANE per record of the chain (k_sp_sums's shape): flag 0x900 -> skipped; a first quality byte 0xFF -> no
//            qualities; else the host's additions in READ order -- backward through memory for flag 0x10 -- of a table in LDS
//            indexed by the byte (qprob[min(q, 93)]), sixteen-byte loads between the unaligned ends of the string.
//   pool   : one wave per kept string, 8 bytes per lane and step, the source realigned (and for 0x10 byte-swapped) in
//            registers, min(q, 93) + 33 on the eight bytes at once, pad bytes 0: k_sp_pool's layout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bam_chain.h"
#include "kernels.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;
static_assert(kSbTile == kThreads * 16, "a lane tests sixteen positions");

__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return ld16(p) | ld16(p + 2) << 16; }

// the 32-bit field at byte K of the lane's 64 bytes
template <int K>
__device__ __forceinline__ uint32_t field(const uint32_t (&w)[16]) {
  static_assert(K + 4 <= 64, "inside the lane's bytes");
  if constexpr ((K & 3) == 0) return w[K >> 2];
  else return __builtin_amdgcn_alignbyte(w[(K >> 2) + 1], w[K >> 2], (uint32_t)(K & 3));
}

// position p = the lane's byte J: the record's block_size, or 0
template <int J>
__device__ __forceinline__ uint32_t sb_fits(const uint32_t (&w)[16], const uint8_t *buf, int64_t p, int64_t lo, int64_t n, int32_t n_ref) {
  const int32_t ref_id = (int32_t)field<J + 4>(w), next_ref_id = (int32_t)field<J + 24>(w);
  if (ref_id < -1 || ref_id >= n_ref || next_ref_id < -1 || next_ref_id >= n_ref) return 0;
  const int32_t pos = (int32_t)field<J + 8>(w), next_pos = (int32_t)field<J + 28>(w), l_seq = (int32_t)field<J + 20>(w);
  if (pos < -1 || next_pos < -1 || l_seq < 0) return 0;
  const uint32_t block_size = field<J>(w), x = field<J + 12>(w), y = field<J + 16>(w);
  const uint32_t l_read_name = x & 0xffu, n_cigar_op = y & 0xffffu;
  if (l_read_name == 0) return 0;
  const int64_t need = 32 + (int64_t)l_read_name + 4 * (int64_t)n_cigar_op + ((int64_t)l_seq + 1) / 2 + l_seq;
  if ((int64_t)block_size < need || (int64_t)block_size > kBamMaxBlock) return 0;
  if (p < lo || p + 4 + (int64_t)block_size > n) return 0;
  if (buf[p + 35 + l_read_name] != 0) return 0;  // (inside the record: need <= block_size)
  return block_size;
}

template <int J>
__device__ __forceinline__ void sb_fits_all(const uint32_t (&w)[16], const uint8_t *buf, int64_t p0, int64_t lo, int64_t n, int32_t n_ref,
                                            uint32_t (&size)[16], int &mine) {
  if constexpr (J < 16) {
    size[J] = sb_fits<J>(w, buf, p0 + J, lo, n, n_ref);
    mine += size[J] != 0;
    sb_fits_all<J + 1>(w, buf, p0, lo, n, n_ref, size, mine);
  }
}

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void k_sb_scan(const uint8_t *buf, int64_t lo, int64_t n, int32_t n_ref, int64_t *tile_count,
                                                     const int64_t *tile_base, uint64_t *out) {
  __shared__ uint4 sh[kThreads + 4];
  __shared__ int cnt[kThreads];
  const int i = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kSbTile;
  const uint4 *g = reinterpret_cast<const uint4 *>(buf + base);  // (the buffer is aligned, and readable kSbSlack bytes past n)
  sh[i] = g[i];
  if (i < 4) sh[kThreads + i] = g[kThreads + i];
  __syncthreads();
  uint32_t w[16];
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const uint4 x = sh[i + v];
    w[4 * v] = x.x;
    w[4 * v + 1] = x.y;
    w[4 * v + 2] = x.z;
    w[4 * v + 3] = x.w;
  }
  uint32_t size[16];
#pragma unroll
  for (int j = 0; j < 16; j++) size[j] = 0;
  int mine = 0;
  const int64_t p0 = base + 16 * i;
  if (p0 < n) sb_fits_all<0>(w, buf, p0, lo, n, n_ref, size, mine);  // (the fields of position 15 end at the lane's byte 46)
  const int total = __syncthreads_count(mine != 0);  // lanes with a hit
  if (!kWrite) {
    if (total == 0) {
      if (i == 0) tile_count[blockIdx.x] = 0;
      return;
    }
    cnt[i] = mine;
    __syncthreads();
    if (i == 0) {
      int64_t sum = 0;
      for (int k = 0; k < kThreads; k++) sum += cnt[k];
      tile_count[blockIdx.x] = sum;
    }
    return;
  }
  if (total == 0) return;
  cnt[i] = mine;
  __syncthreads();
  if (!mine) return;
  int64_t at = tile_base[blockIdx.x];
  for (int k = 0; k < i; k++) at += cnt[k];
#pragma unroll
  for (int j = 0; j < 16; j++)
    if (size[j]) out[at++] = (uint64_t)(p0 + j) << kSbSizeBits | size[j];
}

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
  const int64_t at = (int64_t)(rec[r] >> kSbSizeBits);
  const uint8_t *h = buf + at;
  const uint32_t l_read_name = h[12], n_cigar_op = ld16(h + 16), flag = ld16(h + 18);
  const int32_t len = (int32_t)ld32(h + 20);
  // (the chain walk took this record from the scan: its block_size covers the qualities)
  const int64_t start = at + 36 + (int64_t)l_read_name + 4 * (int64_t)n_cigar_op + ((int64_t)len + 1) / 2;
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
    const bool rev = (ld16(buf + (rec[r] >> kSbSizeBits) + 18) & 0x10u) != 0;
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

void launch_sb_scan(const uint8_t *buf, int64_t lo, int64_t n, int32_t n_ref, int64_t *tile_count, const int64_t *tile_base, uint64_t *out,
                    hipStream_t s) {
  const int64_t n_tiles = sb_tiles(n);
  if (n_tiles <= 0) return;
  if (out) hipLaunchKernelGGL(k_sb_scan<true>, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, buf, lo, n, n_ref, tile_count, tile_base, out);
  else hipLaunchKernelGGL(k_sb_scan<false>, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, buf, lo, n, n_ref, tile_count, tile_base, out);
}

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
  const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>((n_rec + 3) / 4, 1), 4096);
  hipLaunchKernelGGL(k_sb_pool, dim3(grid), dim3(256), 0, s, buf, rec, qual_at, rec_len, padded, off, n_rec, pool);
}

}  // namespace pbsim
