// vcf_text.h -- what the kernels that read VCF text in HBM and write text back share (vcf_compare.hip, vcf_apply.hip): where a data
// line begins, the workgroup's prefix sum, the bytes' classes and the small writers of numbers and spans.  Device code only;
// internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bam_pileup_walk.h"

namespace pbsim {
namespace vcftext {

using pilewalk::kWaves;
using pilewalk::u64;
using pilewalk::wave_scan;

// the exclusive prefix sum of v over the workgroup and *all, the workgroup's sum; every lane of the workgroup calls it
__device__ __forceinline__ u64 block_scan(u64 v, u64 *sh_wave, int wave, int lane, u64 *all) {
  const u64 incl = wave_scan(v, lane);
  __syncthreads();  // (the values of the call before have been read)
  if (lane == 63) sh_wave[wave] = incl;
  __syncthreads();
  u64 before = 0, sum = 0;
  for (int w = 0; w < kWaves; w++) {
    if (w < wave) before += sh_wave[w];
    sum += sh_wave[w];
  }
  *all = sum;
  return before + incl - v;
}

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

__device__ __forceinline__ int digits(u64 x) {
  int n = 1;
  while (x >= 10) x /= 10, n++;
  return n;
}
__device__ __forceinline__ char *put(char *o, u64 x) {
  const int n = digits(x);
  for (int k = n - 1; k >= 0; k--, x /= 10) o[k] = (char)('0' + x % 10);
  return o + n;
}
__device__ __forceinline__ char *put(char *o, const char *s) {
  while (*s) *o++ = *s++;
  return o;
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
