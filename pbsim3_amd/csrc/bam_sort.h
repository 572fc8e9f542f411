// bam_sort.h -- the device side of pbsim_truth_bam_sort (bam_sort.hip), as bam_sort.cpp drives it.  Internal: nothing here is
// part of include/pbsim3_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbsim {

// bytes of the inflated stream one workgroup of the record scan tests (256 lanes x 16 byte positions)
constexpr int kBsTile = 4096;
// what the stream's buffer holds behind its last byte, zeroed: the scan loads whole tiles plus a 64-byte halo, the gather
// reads the aligned dwords around a record's last bytes
constexpr int64_t kBsSlack = kBsTile + 128;
// a candidate / a record: (inflated byte offset << 24) | block_size.  A record of 2^24 bytes or more is refused (a
// 1 000 000-base read with a run per column stays below 7 MB); 2^40 bytes of stream are more than any HBM holds
constexpr int kBsSizeBits = 24;
constexpr uint64_t kBsSizeMask = ((uint64_t)1 << kBsSizeBits) - 1;
// destination bytes per wave of the gather (64 lanes x 16 bytes x 4 rounds)
constexpr int kBsSpan = 4096;

// Every byte position p in [lo, n) of stream[0..n) against the fixed fields of a placed single-end record (next_refID =
// next_pos = -1, tlen = 0, 0 <= refID < n_ref, pos >= 0, l_seq >= 0, block_size >= 32 + l_read_name + 4 n_cigar_op +
// (l_seq + 1) / 2 + l_seq and < 2^24, p + 4 + block_size <= n).  Tile t = bytes [t kBsTile, (t + 1) kBsTile); the stream is
// readable and zero for kBsSlack bytes behind n.  out == nullptr: tile_count[t - first_tile] = the tile's hits (int64, so that
// the exclusive scan over them needs no conversion); else the hits, packed, in ascending order at out[tile_base[t - first_tile]..).
void launch_bs_scan(const uint8_t *stream, int64_t lo, int64_t n, int32_t n_ref, int64_t first_tile, int64_t n_tiles,
                    int64_t *tile_count, const int64_t *tile_base, uint64_t *out, hipStream_t s);
// per record r (packed as above): key[r] = refID << 32 | pos, idx[r] = r, end[r] = pos + the reference span of its CIGAR
// (M, D, N, =, X), pos + 1 where that is 0.  One wave per record.
void launch_bs_keys(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, uint64_t *key, uint32_t *idx, int64_t *end, hipStream_t s);
// per place i of the sorted order: src_off[i], size[i] (4 + block_size) and end_sorted[i] of record perm[i]; size[n_rec] = 0
void launch_bs_permute(const uint64_t *rec, const uint32_t *perm, const int64_t *end, int64_t n_rec, int64_t *src_off, int64_t *size,
                       int64_t *end_sorted, hipStream_t s);
// out[dst_off[i] .. dst_off[i + 1]) = stream[src_off[i] ..) for every i; dst_off[n_rec] = total.  out is 16-byte aligned with
// 16 bytes of slack (whole vectors are stored: the bytes behind `total` up to the next multiple of 16 become zero).
void launch_bs_gather(const uint8_t *stream, uint8_t *out, const int64_t *src_off, const int64_t *dst_off, int64_t n_rec, int64_t total,
                      hipStream_t s);
// rocPRIM behind two-phase calls (temp == nullptr: *temp_bytes receives the scratch size)
hipError_t bs_exclusive_scan(void *temp, size_t *temp_bytes, const int64_t *in, int64_t *out, int64_t n, hipStream_t s);
// stable, by the low `end_bit` bits of the keys
hipError_t bs_sort_pairs(void *temp, size_t *temp_bytes, const uint64_t *key_in, uint64_t *key_out, const uint32_t *val_in, uint32_t *val_out,
                         int64_t n, int end_bit, hipStream_t s);

}  // namespace pbsim
