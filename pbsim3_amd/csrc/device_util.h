// device_util.h -- the small device helpers every stage's kernels share: the wave's and the workgroup's sums, a rate in parts per
// million, a search in an ascending table, the writers of decimal numbers and of a line's tab-separated fields, and the host's
// grid size.  Device code: included by .hip files only.  Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbsim {

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_sum(u64 x) {
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

__device__ __forceinline__ u64 wave_max(u64 x) {
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 y = __shfl_xor(x, d, 64);
    x = y > x ? y : x;
  }
  return x;
}

__device__ __forceinline__ u64 wave_scan(u64 x, int lane) {  // inclusive
  for (int d = 1; d < 64; d <<= 1) {
    const u64 y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// the exclusive prefix sum of v over the workgroup and *all, the workgroup's sum; every lane of the workgroup calls it, with one
// cell of LDS per wave
template <int kWaves>
__device__ __forceinline__ u64 block_scan(u64 v, u64 (&sh_wave)[kWaves], int wave, int lane, u64 *all) {
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

// floor(x * 1000000 / c) for x <= c < 2^62, inside 64 bits: Horner over the bits of 1000000, quotient and remainder kept apart
__device__ __forceinline__ u64 ppm_of(u64 x, u64 c) {
  u64 q = 0, r = 0;
  for (int b = 19; b >= 0; b--) {
    q <<= 1;
    r <<= 1;
    if ((1000000u >> b) & 1u) r += x;  // r < 3 c
    if (r >= c) r -= c, q++;
    if (r >= c) r -= c, q++;
  }
  return q;
}

// the last r in [0, n) with table[r] <= x (table ascending, table[0] <= x)
template <class Index>
__device__ __forceinline__ Index last_at_most(const int64_t *table, Index n, int64_t x) {
  Index lo = 0, hi = n;  // table[lo] <= x, table[hi] > x (or hi == n)
  while (hi - lo > 1) {
    const Index mid = lo + ((hi - lo) >> 1);
    if (table[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
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

// A line's n numbers f[], each behind a tab, `*` for one the line lacks (bit j of has: f[j] is there): the bytes they take, and
// the bytes themselves.  The two passes of a stage's text share them: the sizes first, the fill after their exclusive scan.
__device__ __forceinline__ int64_t fields_len(uint32_t has, const u64 *f, int n) {
  int64_t l = 0;
  for (int j = 0; j < n; j++) l += 1 + ((has >> j) & 1u ? digits(f[j]) : 1);
  return l;
}
__device__ __forceinline__ char *put_fields(char *o, uint32_t has, const u64 *f, int n) {
  for (int j = 0; j < n; j++) {
    *o++ = '\t';
    if ((has >> j) & 1u) o = put(o, f[j]);
    else *o++ = '*';
  }
  return o;
}

// the workgroups that take n items, `per` each (256: every stage's workgroup is four waves)
inline unsigned blocks_of(int64_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

}  // namespace pbsim
