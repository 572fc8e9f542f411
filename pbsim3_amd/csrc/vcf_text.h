// vcf_text.h -- what the kernels that read VCF text in HBM and write text back share (vcf_compare.hip, vcf_apply.hip): where a data
// line begins, the bytes' classes and the writer of a column's span.  The sums and the writers of numbers are device_util.h's.
// Device code only; internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_util.h"

namespace pbsim {
namespace vcftext {

__device__ __forceinline__ uint32_t upper(uint32_t c) { return c >= 'a' && c <= 'z' ? c - 32u : c; }
__device__ __forceinline__ bool base_or_n(uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; }

// The four bytes at i0 (a multiple of 4) of a text that lies at [lo, hi) of an aligned buffer with at least one byte behind i0 + 3:
// begins[k] says whether a data line begins at i0 + k -- at the text's first byte or behind a line feed, where the line is neither
// empty (a lone \r in front of the \n counted) nor begins with #.  One 32-bit load with the byte in front and the byte behind.
// Returns how many begin.
__device__ __forceinline__ u64 line_begins(const uint8_t *bytes, int64_t i0, int64_t lo, int64_t hi, bool begins[4]) {
  const uint32_t word = *(const uint32_t *)(bytes + i0);
  const uint32_t six[6] = {i0 > 0 ? bytes[i0 - 1] : (uint32_t)'\n', word & 255u, (word >> 8) & 255u, (word >> 16) & 255u, word >> 24, bytes[i0 + 4]};
  u64 n = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int64_t i = i0 + k;
    const uint32_t prev = six[k], c = six[k + 1], next = six[k + 2];
    begins[k] = i >= lo && i < hi && (i == lo || prev == '\n') && c != '#' && c != '\n' && !(c == '\r' && i + 1 < hi && next == '\n');
    n += begins[k];
  }
  return n;
}

// a column as the file has it, `.` for one the line lacks or that is empty
__device__ __forceinline__ char *put_span(char *o, const uint8_t *p, uint32_t n) {
  if (n == 0) *o++ = '.';
  for (uint32_t k = 0; k < n; k++) *o++ = (char)p[k];
  return o;
}
__device__ __forceinline__ int length_of(const char *s) {
  int n = 0;
  while (s[n]) n++;
  return n;
}

}  // namespace vcftext
}  // namespace pbsim
