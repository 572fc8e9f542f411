// bam_sort.hip -- the kernels of pbsim_truth_bam_sort: a finished truth BAM, inflated into HBM, becomes the same records in
// coordinate order.
//
//   scan    : BAM records are chained by block_size, and a chain is serial.  Every BYTE position is tested instead, in
//             parallel, against the fields that are constant in a placed single-end record (twelve bytes: next_refID,
//             next_pos, tlen) and against what its sizes must satisfy.  A workgroup stages a 4 KiB tile plus a 64-byte halo in
//             LDS; a lane reduces the 48 bytes behind its sixteen positions to two bit masks (byte == 0xFF, byte == 0) and
//             finds the positions whose twelve constant bytes match with a handful of shifts -- the full test, on unaligned
//             fields, runs for those few only.  Two passes (count, then write behind an exclusive scan of the counts) keep
//             the hits in ascending order.  The hits are a SUPERSET of the record starts (a SEQ of 'N's in front of zero
//             qualities passes): the host walks the chain over them, and that walk alone decides (bam_sort.cpp).
//   keys    : one wave per record: refID, pos, and the reference span of its CIGAR, the ops across the lanes.
//   sort    : rocPRIM's radix sort of (refID << 32 | pos, record index): stable, so ties keep their input order.
//   gather  : destination-driven.  A wave owns 4 KiB of the sorted stream and a lane one 16-byte vector of it at a time: the
//             lane finds the record its vector lies in (a 64-ary search by the wave for the span's first record, then at
//             most seven steps per lane, none where one record covers the span) and stores the vector from the source's
//             aligned dwords shifted into place (v_alignbyte, as k_bam_finish does).  A 1.5 MB record is thus spread over
//             ~370 waves, and a 4 KiB span of 50-byte records is one wave's work; only a vector that straddles a record
//             boundary is put together byte by byte.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "bam_sort.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return ld16(p) | ld16(p + 2) << 16; }

// bit k = byte k of w is zero (exact: no carry runs from one byte into the next)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t w) {
  const uint32_t m = ~(((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w | 0x7F7F7F7Fu);  // 0x80 in every zero byte
  const uint32_t x = m >> 7;
  return (x | x >> 7 | x >> 14 | x >> 21) & 15u;
}

// the whole test of position p (the caller has seen the twelve constant bytes); the record's block_size, or 0
__device__ __forceinline__ uint32_t bs_fits(const uint8_t *stream, int64_t p, int64_t lo, int64_t n, int32_t n_ref) {
  if (p < lo || p + 36 > n) return 0;
  const uint8_t *r = stream + p;
  const uint32_t block_size = ld32(r);
  const int32_t ref_id = (int32_t)ld32(r + 4), pos = (int32_t)ld32(r + 8), l_seq = (int32_t)ld32(r + 20);
  const uint32_t l_read_name = r[12], n_cigar_op = ld16(r + 16);
  if (ref_id < 0 || ref_id >= n_ref || pos < 0 || l_seq < 0) return 0;
  if (ld32(r + 24) != 0xffffffffu || ld32(r + 28) != 0xffffffffu || ld32(r + 32) != 0u) return 0;
  const int64_t need = 32 + (int64_t)l_read_name + 4 * (int64_t)n_cigar_op + ((int64_t)l_seq + 1) / 2 + l_seq;
  if ((int64_t)block_size < need || block_size > kBsSizeMask) return 0;
  if (p + 4 + (int64_t)block_size > n) return 0;
  return block_size;
}

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void k_bs_scan(const uint8_t *stream, int64_t lo, int64_t n, int32_t n_ref, int64_t first_tile,
                                                     int64_t *tile_count, const int64_t *tile_base, uint64_t *out) {
  __shared__ uint4 sh[kThreads + 4];
  __shared__ int cnt[kThreads];
  const int i = threadIdx.x;
  const int64_t base = (first_tile + blockIdx.x) * kBsTile;
  const uint4 *g = reinterpret_cast<const uint4 *>(stream + base);  // (the stream's buffer is aligned, and readable kBsSlack bytes past n)
  sh[i] = g[i];
  if (i < 4) sh[kThreads + i] = g[kThreads + i];
  __syncthreads();
  // bytes 16 i + 16 .. 16 i + 63 of the tile: position j = 16 i + j' wants 0xFF in bytes j + 24 .. j + 31, 0 in j + 32 .. j + 35
  uint64_t ff = 0, zz = 0;
#pragma unroll
  for (int v = 0; v < 3; v++) {
    const uint4 x = sh[i + 1 + v];
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      ff |= (uint64_t)zero_bytes(~w[k]) << (16 * v + 4 * k);
      zz |= (uint64_t)zero_bytes(w[k]) << (16 * v + 4 * k);
    }
  }
  ff &= ff >> 1;
  ff &= ff >> 2;
  ff &= ff >> 4;  // bit k: bytes k .. k + 7 are 0xFF
  zz &= zz >> 1;
  zz &= zz >> 2;  // bit k: bytes k .. k + 3 are 0
  uint32_t hits = (uint32_t)((ff >> 8) & (zz >> 16)) & 0xffffu;
  uint32_t size[16];
#pragma unroll
  for (int j = 0; j < 16; j++) size[j] = 0;
  int mine = 0;
  if (hits) {  // rare: the unaligned fields, from HBM
#pragma unroll
    for (int j = 0; j < 16; j++) {
      if (hits >> j & 1) size[j] = bs_fits(stream, base + 16 * i + j, lo, n, n_ref);
      mine += size[j] != 0;
    }
  }
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
    if (size[j]) out[at++] = (uint64_t)(base + 16 * i + j) << kBsSizeBits | size[j];
}

__global__ __launch_bounds__(kThreads) void k_bs_keys(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, uint64_t *key, uint32_t *idx,
                                                     int64_t *end) {
  const int64_t r = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n_rec) return;
  const uint8_t *p = stream + (rec[r] >> kBsSizeBits);
  const uint32_t ref_id = ld32(p + 4), pos = ld32(p + 8), l_read_name = p[12], n_cigar_op = ld16(p + 16);
  const uint8_t *cig = p + 36 + l_read_name;
  int64_t span = 0;
  for (uint32_t k = lane; k < n_cigar_op; k += 64) {
    const uint32_t v = ld32(cig + 4 * (int64_t)k);
    const uint32_t op = v & 15u;  // MIDNSHP=X: M 0, D 2, N 3, = 7, X 8 consume the reference
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += v >> 4;
  }
  for (int d = 32; d > 0; d >>= 1) span += __shfl_xor(span, d, 64);
  if (lane == 0) {
    key[r] = (uint64_t)ref_id << 32 | pos;
    idx[r] = (uint32_t)r;
    end[r] = (int64_t)pos + (span > 0 ? span : 1);
  }
}

__global__ __launch_bounds__(kThreads) void k_bs_permute(const uint64_t *rec, const uint32_t *perm, const int64_t *end, int64_t n_rec,
                                                        int64_t *src_off, int64_t *size, int64_t *end_sorted) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i > n_rec) return;
  if (i == n_rec) {
    size[i] = 0;
    return;
  }
  const uint32_t r = perm[i];
  const uint64_t x = rec[r];
  src_off[i] = (int64_t)(x >> kBsSizeBits);
  size[i] = 4 + (int64_t)(x & kBsSizeMask);
  end_sorted[i] = end[r];
}

__global__ __launch_bounds__(kThreads) void k_bs_gather(const uint8_t *stream, uint8_t *out, const int64_t *src_off, const int64_t *dst_off,
                                                       int64_t n_rec, int64_t total) {
  const int lane = threadIdx.x & 63;
  const int64_t span0 = ((int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * kBsSpan;
  if (span0 >= total) return;  // (the whole wave)
  const int64_t span1 = min(span0 + kBsSpan, total);
  // ---- the record that holds byte span0: the largest r with dst_off[r] <= span0, 64 probes per step
  int64_t lo = 0, hi = n_rec;  // dst_off[lo] <= span0; hi == n_rec or dst_off[hi] > span0
  while (hi - lo > 1) {
    const int64_t step = (hi - lo + 63) / 64;
    const int64_t at = lo + (lane + 1) * step;
    const bool le = at < hi && dst_off[at] <= span0;
    const int k = __popcll(__ballot(le));  // (dst_off ascends: the lanes that say yes are the first k)
    const int64_t nhi = min(hi, lo + (k + 1) * step);
    lo += k * step;
    hi = nhi;
  }
  const int64_t r0 = lo;
  // a record is 36 bytes at least: the span holds the tail of r0 and at most 114 record starts
  const int64_t r_max = min(n_rec - 1, r0 + (kBsSpan + 35) / 36);
  const bool one = dst_off[r0 + 1] >= span1;  // (wave-uniform: one record covers the span)
#pragma unroll 1
  for (int round = 0; round < kBsSpan / (64 * 16); round++) {
    const int64_t d = span0 + (int64_t)(round * 64 + lane) * 16;
    if (d >= span1) continue;
    int64_t r = r0;
    if (!one) {
      int64_t a = r0, b = r_max;
      while (a < b) {
        const int64_t mid = (a + b + 1) >> 1;
        if (dst_off[mid] <= d) a = mid;
        else b = mid - 1;
      }
      r = a;
    }
    const int64_t r_begin = dst_off[r], r_end = dst_off[r + 1];
    uint4 o;
    if (d + 16 <= r_end) {  // the whole vector out of one record: aligned dwords of the source, shifted
      const int64_t s = src_off[r] + (d - r_begin);
      const uint32_t sh = (uint32_t)(s & 3);
      const uint32_t *p = reinterpret_cast<const uint32_t *>(stream + (s - sh));
      uint32_t w[5];
#pragma unroll
      for (int k = 0; k < 5; k++) w[k] = p[k];  // (k == 4 counts for sh != 0 only; the stream's buffer has slack)
      o.x = __builtin_amdgcn_alignbyte(w[1], w[0], sh);
      o.y = __builtin_amdgcn_alignbyte(w[2], w[1], sh);
      o.z = __builtin_amdgcn_alignbyte(w[3], w[2], sh);
      o.w = __builtin_amdgcn_alignbyte(w[4], w[3], sh);
    } else {  // a record ends inside the vector (or the stream does): byte by byte
      uint32_t w[4] = {0, 0, 0, 0};
      int64_t rr = r, beg = r_begin, fin = r_end, src = src_off[r];
      for (int b = 0; b < 16; b++) {
        const int64_t x = d + b;
        if (x >= total) break;
        while (x >= fin) {
          rr++;
          beg = fin;
          fin = dst_off[rr + 1];
          src = src_off[rr];
        }
        w[b >> 2] |= (uint32_t)stream[src + (x - beg)] << (8 * (b & 3));
      }
      o = make_uint4(w[0], w[1], w[2], w[3]);
    }
    *reinterpret_cast<uint4 *>(out + d) = o;
  }
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_bs_scan(const uint8_t *stream, int64_t lo, int64_t n, int32_t n_ref, int64_t first_tile, int64_t n_tiles, int64_t *tile_count,
                    const int64_t *tile_base, uint64_t *out, hipStream_t s) {
  if (n_tiles <= 0) return;
  if (out) hipLaunchKernelGGL(k_bs_scan<true>, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, stream, lo, n, n_ref, first_tile, tile_count, tile_base, out);
  else hipLaunchKernelGGL(k_bs_scan<false>, dim3((unsigned)n_tiles), dim3(kThreads), 0, s, stream, lo, n, n_ref, first_tile, tile_count, tile_base, out);
}

void launch_bs_keys(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, uint64_t *key, uint32_t *idx, int64_t *end, hipStream_t s) {
  if (n_rec <= 0) return;
  hipLaunchKernelGGL(k_bs_keys, dim3(blocks_of(n_rec, kThreads / 64)), dim3(kThreads), 0, s, stream, rec, n_rec, key, idx, end);
}

void launch_bs_permute(const uint64_t *rec, const uint32_t *perm, const int64_t *end, int64_t n_rec, int64_t *src_off, int64_t *size,
                       int64_t *end_sorted, hipStream_t s) {
  hipLaunchKernelGGL(k_bs_permute, dim3(blocks_of(n_rec + 1, kThreads)), dim3(kThreads), 0, s, rec, perm, end, n_rec, src_off, size, end_sorted);
}

void launch_bs_gather(const uint8_t *stream, uint8_t *out, const int64_t *src_off, const int64_t *dst_off, int64_t n_rec, int64_t total,
                      hipStream_t s) {
  if (n_rec <= 0 || total <= 0) return;
  hipLaunchKernelGGL(k_bs_gather, dim3(blocks_of(total, kBsSpan * (kThreads / 64))), dim3(kThreads), 0, s, stream, out, src_off, dst_off, n_rec,
                     total);
}

hipError_t bs_exclusive_scan(void *temp, size_t *temp_bytes, const int64_t *in, int64_t *out, int64_t n, hipStream_t s) {
  return rocprim::exclusive_scan(temp, *temp_bytes, in, out, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), s);
}

hipError_t bs_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *key_in, uint64_t *key_out, const uint32_t *val_in, uint32_t *val_out,
                         int64_t n, int end_bit, hipStream_t s) {
  return rocprim::radix_sort_pairs(temp, *temp_bytes, key_in, key_out, val_in, val_out, (size_t)n, 0u, (unsigned)end_bit, s);
}

}  // namespace pbsim
