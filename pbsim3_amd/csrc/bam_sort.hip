// bam_sort.hip -- the kernels of pbsim_truth_bam_sort: a finished truth BAM, inflated into HBM, becomes the same records in
// coordinate order.
//
//   scan    : bam_scan.hip, with the policy "placed single-end record"; the host walks the chain over its candidates.
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

#include "bam_chain.h"
#include "bam_fields.h"
#include "bam_sort.h"
#include "device_util.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;

constexpr BamPacking kPk = kBamSortPacking;

__global__ __launch_bounds__(kThreads) void k_bs_keys(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, uint64_t *key, uint32_t *idx,
                                                     int64_t *end) {
  const int64_t r = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= n_rec) return;
  const uint8_t *p = stream + kPk.offset(rec[r]);
  const uint32_t ref_id = ld32(p + kBamRefId), pos = ld32(p + kBamPos), l_read_name = p[kBamLReadName], n_cigar_op = ld16(p + kBamNCigarOp);
  const uint8_t *cig = p + kBamFixed + l_read_name;
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
  if (i >= n_rec) return;
  const uint32_t r = perm[i];
  const uint64_t x = rec[r];
  src_off[i] = kPk.offset(x);
  size[i] = 4 + kPk.size(x);
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

}  // namespace

void launch_bs_keys(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, uint64_t *key, uint32_t *idx, int64_t *end, hipStream_t s) {
  if (n_rec <= 0) return;
  hipLaunchKernelGGL(k_bs_keys, dim3(blocks_of(n_rec, kThreads / 64)), dim3(kThreads), 0, s, stream, rec, n_rec, key, idx, end);
}

void launch_bs_permute(const uint64_t *rec, const uint32_t *perm, const int64_t *end, int64_t n_rec, int64_t *src_off, int64_t *size,
                       int64_t *end_sorted, hipStream_t s) {
  if (n_rec <= 0) return;
  hipLaunchKernelGGL(k_bs_permute, dim3(blocks_of(n_rec, kThreads)), dim3(kThreads), 0, s, rec, perm, end, n_rec, src_off, size, end_sorted);
}

void launch_bs_gather(const uint8_t *stream, uint8_t *out, const int64_t *src_off, const int64_t *dst_off, int64_t n_rec, int64_t total,
                      hipStream_t s) {
  if (n_rec <= 0 || total <= 0) return;
  hipLaunchKernelGGL(k_bs_gather, dim3(blocks_of(total, kBsSpan * (kThreads / 64))), dim3(kThreads), 0, s, stream, out, src_off, dst_off, n_rec,
                     total);
}

hipError_t bs_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *key_in, uint64_t *key_out, const uint32_t *val_in, uint32_t *val_out,
                         int64_t n, int end_bit, hipStream_t s) {
  return rocprim::radix_sort_pairs(temp, *temp_bytes, key_in, key_out, val_in, val_out, (size_t)n, 0u, (unsigned)end_bit, s);
}

}  // namespace pbsim
