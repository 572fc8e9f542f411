// bam_tags.h -- what the truth BAM writer (kernels.hip) and the lift stage (bam_lift.hip) write alike into an aligned record
// (SAMv1 4.2): an integer tag of the smallest type that holds the value, as htslib's SAM parser chooses it; the bin of a placed
// record; and the op count above which a CIGAR moves into a CG:B,I tag behind NM and leaves <l_seq>S<span>N in its place
// (SAMv1 4.2.2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbsim {

__device__ __forceinline__ int bam_int_size(int64_t v) {
  if (v < 0) return v >= -128 ? 1 : v >= -32768 ? 2 : 4;
  return v < 256 ? 1 : v < 65536 ? 2 : 4;
}
__device__ __forceinline__ char *bam_put_int_tag(char *o, char t0, char t1, int64_t v) {
  *o++ = t0;
  *o++ = t1;
  const int n = bam_int_size(v);
  *o++ = (v < 0) ? (n == 1 ? 'c' : n == 2 ? 's' : 'i') : (n == 1 ? 'C' : n == 2 ? 'S' : 'I');
  for (int i = 0; i < n; i++) *o++ = (char)((uint64_t)v >> (8 * i));
  return o;
}
constexpr int kCigarMaxOps = 65535;
// SAMv1 5.3, reg2bin(beg, end) as the specification writes it
__device__ __forceinline__ int aln_reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}

}  // namespace pbsim
