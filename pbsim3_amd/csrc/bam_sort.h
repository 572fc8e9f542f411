// bam_sort.h -- the device side of pbsim_truth_bam_sort (bam_sort.hip), as bam_sort.cpp drives it.  Internal: nothing here is
// part of include/pbsim3_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbsim {

// destination bytes per wave of the gather (64 lanes x 16 bytes x 4 rounds)
constexpr int kBsSpan = 4096;

// per record r (packed as kBamSortPacking, bam_chain.h): key[r] = refID << 32 | pos, idx[r] = r, end[r] = pos + the reference
// span of its CIGAR (M, D, N, =, X), pos + 1 where that is 0.  One wave per record.
void launch_bs_keys(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, uint64_t *key, uint32_t *idx, int64_t *end, hipStream_t s);
// per place i of the sorted order: src_off[i], size[i] (4 + block_size) and end_sorted[i] of record perm[i]
void launch_bs_permute(const uint64_t *rec, const uint32_t *perm, const int64_t *end, int64_t n_rec, int64_t *src_off, int64_t *size,
                       int64_t *end_sorted, hipStream_t s);
// out[dst_off[i] .. dst_off[i + 1]) = stream[src_off[i] ..) for every i; dst_off[n_rec] = total.  out is 16-byte aligned with
// 16 bytes of slack (whole vectors are stored: the bytes behind `total` up to the next multiple of 16 become zero).
void launch_bs_gather(const uint8_t *stream, uint8_t *out, const int64_t *src_off, const int64_t *dst_off, int64_t n_rec, int64_t total,
                      hipStream_t s);
// rocPRIM's radix sort behind two-phase calls (temp == nullptr: *temp_bytes receives the scratch size): stable, by the low
// `end_bit` bits of the keys
hipError_t bs_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *key_in, uint64_t *key_out, const uint32_t *val_in, uint32_t *val_out,
                         int64_t n, int end_bit, hipStream_t s);

}  // namespace pbsim
