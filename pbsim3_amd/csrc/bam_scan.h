// bam_scan.h -- where the records of a BAM stream in HBM may start (bam_scan.hip): the parallel scan whose candidates
// bam_walk_chain (bam_chain.h) walks.  Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "bam_chain.h"
#include "ctx.h"

namespace pbsim {

// bytes of the stream one workgroup tests (256 lanes x 16 byte positions)
constexpr int kBamTile = 4096;
// what the stream's buffer holds behind its last byte, zeroed: the scan loads whole tiles plus a 64-byte halo (and the sort's
// gather reads the aligned dwords around a record's last bytes, the sampling pool 15 bytes past a quality string)
constexpr int64_t kBamSlack = kBamTile + 128;

// What a position must look like; each policy packs its candidates its own way (bam_chain.h).  Both give a SUPERSET of the
// record starts -- the chain walk decides.
enum BamScanPolicy {
  // the sort's: a placed single-end record.  0 <= refID < n_ref, pos >= 0, l_seq >= 0, next_refID = next_pos = -1, tlen = 0,
  // block_size >= 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq and < 2^24, the record inside the bytes.
  // kBamSortPacking.  (A SEQ of 'N's in front of zero qualities passes.)
  kBamScanPlaced,
  // the sampling input's: any record.  refID, next_refID in [-1, n_ref), pos, next_pos >= -1, l_read_name >= 1 with a NUL as
  // the name's last byte, l_seq >= 0, block_size as above but <= 64 MiB, the record inside the bytes.  kBamSamplePacking.
  // (A B array that holds a record image passes.)
  kBamScanAny
};

// The scan and its buffers, kept from call to call.
struct BamScan {
  // The candidates among the byte positions [lo, n) of buf[0, n), ascending, into *hits.  buf is 16-byte aligned and readable
  // (zero) for kBamSlack bytes behind n.  Ends with the stream synchronised.  hipErrorOutOfMemory from a buffer of its own:
  // oom_what needed oom_bytes.
  hipError_t run(BamScanPolicy policy, const uint8_t *buf, int64_t lo, int64_t n, int32_t n_ref, hipStream_t s, std::vector<uint64_t> *hits);
  const char *oom_what = nullptr;
  size_t oom_bytes = 0;

 private:
  hipError_t need(DevBuf &b, size_t bytes, const char *what);
  DevBuf d_tiles, d_scan_tmp, d_hits;  // per tile: its hits, then where they go; launch_exclusive_scan_i64's scratch; the hits
};

}  // namespace pbsim
