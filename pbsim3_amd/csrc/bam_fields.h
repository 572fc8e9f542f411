// bam_fields.h -- the fixed fields of a BAM record (SAMv1 4.2) as device code reads them: little-endian loads from unaligned
// bytes, and where each field lies behind the record's first byte (its block_size).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbsim {

__device__ __forceinline__ uint32_t ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t ld32(const uint8_t *p) { return ld16(p) | ld16(p + 2) << 16; }

enum : int {
  kBamRefId = 4,
  kBamPos = 8,
  kBamLReadName = 12,  // one byte; mapq and bin follow it
  kBamNCigarOp = 16,   // two bytes
  kBamFlag = 18,       // two bytes
  kBamLSeq = 20,
  kBamNextRefId = 24,
  kBamNextPos = 28,
  kBamTlen = 32,
  kBamFixed = 36  // read_name, cigar, seq, qual and the tags from here
};

}  // namespace pbsim
