// sample_profile.hip -- the profile of the sampling method (get_sample_inf, pbsim.cpp:1155-1330) from FASTQ bytes in HBM:
// which bytes are quality lines, every quality line's ordered sum of error probabilities, and the strings that pass the
// filter packed into the pool k_walk_sample reads.  The host side (windows, carries across them, statistics, errors) is
// sample_profile.cpp.
//
//   lines  : a record ends with its 4th line feed (pbsim.cpp:1216-1283) -- nothing else in the bytes matters.  Line feeds are
//            counted per 1 KiB tile (one 16-byte load per lane of a wave), the counts are scanned, and a second pass over the
//            same tiles gives every line feed its index: index mod 4 = 2 starts a quality line behind it, = 3 ends one.
//   sums   : one LANE per record, the host's additions in the host's order (an f64 sum cannot be split), table in LDS
//            indexed by the byte, 64 bytes of the string per turn with the next 64 on their way -- k_sample_qsum's shape.
//            Additions and one division only: nothing here is a multiply-add the compiler could contract.
//   pool   : one wave per kept string, 8 bytes per lane and step, the source realigned in registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"

namespace pbsim {

namespace {

constexpr uint32_t kLf4 = 0x0a0a0a0au;

// 0x80 in every byte of w that equals the pattern's byte, 0 elsewhere (exact: no carry crosses a byte)
__device__ inline uint32_t eq_bytes(uint32_t w, uint32_t pattern) {
  const uint32_t x = w ^ pattern;
  const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
  return ~(t | x | 0x7f7f7f7fu);
}

// the 16 bytes at buf + o (o a multiple of 16); bytes outside [b0, b1) read as 0x01: neither a line feed nor NUL
__device__ inline uint4 load_window(const uint8_t *buf, int64_t o, int64_t b0, int64_t b1) {
  if (o >= b1 || o + 16 <= b0) return make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
  const uint4 v = *reinterpret_cast<const uint4 *>(buf + o);
  if (o >= b0 && o + 16 <= b1) return v;
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int d = 0; d < 4; d++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t p = o + d * 4 + j;
      if (p < b0 || p >= b1) w[d] = (w[d] & ~(0xffu << (8 * j))) | (0x01u << (8 * j));
    }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ inline uint32_t count_lf(const uint4 &v) {
  return __popc(eq_bytes(v.x, kLf4)) + __popc(eq_bytes(v.y, kLf4)) + __popc(eq_bytes(v.z, kLf4)) + __popc(eq_bytes(v.w, kLf4));
}

constexpr int kCountUnroll = 4;  // tiles a wave has in flight

__global__ __launch_bounds__(256) void k_sp_count(const uint8_t *buf, int64_t b0, int64_t b1, int64_t n_tiles, int64_t *tile_count,
                                                  int32_t *nul) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * 4;
  const int64_t tile0 = b0 & ~(int64_t)(kSpTile - 1);
  uint32_t zero = 0;
  for (int64_t t0 = wave * kCountUnroll; t0 < n_tiles; t0 += n_waves * kCountUnroll) {
    uint4 v[kCountUnroll];
#pragma unroll
    for (int k = 0; k < kCountUnroll; k++) {
      // (a tile behind the last one lies behind b1: nothing is loaded for it)
      v[k] = load_window(buf, tile0 + (t0 + k) * kSpTile + lane * 16, b0, b1);
    }
#pragma unroll
    for (int k = 0; k < kCountUnroll; k++) {
      zero |= eq_bytes(v[k].x, 0u) | eq_bytes(v[k].y, 0u) | eq_bytes(v[k].z, 0u) | eq_bytes(v[k].w, 0u);
      uint32_t c = count_lf(v[k]);
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
      if (lane == 0 && t0 + k < n_tiles) tile_count[t0 + k] = (int64_t)c;
    }
  }
  if (__any(zero != 0) && lane == 0) atomicOr(nul, 1);
}

__global__ __launch_bounds__(256) void k_sp_lines(const uint8_t *buf, int64_t b0, int64_t b1, int phase, int64_t n_tiles,
                                                  const int64_t *tile_base, uint32_t *rec_start, uint32_t *rec_end) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * 4;
  const int64_t tile0 = b0 & ~(int64_t)(kSpTile - 1);
  if (phase == 3 && wave == 0 && lane == 0) rec_start[0] = (uint32_t)b0;  // the window begins with a quality line
  for (int64_t t = wave; t < n_tiles; t += n_waves) {
    const int64_t o = tile0 + t * kSpTile + lane * 16;
    const uint4 v = load_window(buf, o, b0, b1);
    const uint32_t c = count_lf(v);
    uint32_t inc = c;  // inclusive scan over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(inc, d);
      if (lane >= d) inc += y;
    }
    if (c == 0) continue;
    int64_t idx = (int64_t)phase + tile_base[t] + (int64_t)(inc - c);  // line feeds in front of this lane's first one, in the record grid
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int d = 0; d < 4; d++) {
      uint32_t m = eq_bytes(w[d], kLf4);
      while (m) {
        const int j = (__ffs(m) - 1) >> 3;
        m &= m - 1;
        const uint32_t pos = (uint32_t)(o + d * 4 + j);
        const int ph = (int)(idx & 3);
        if (ph == 2) rec_start[idx >> 2] = pos + 1;
        else if (ph == 3) rec_end[idx >> 2] = pos;
        idx++;
      }
    }
  }
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void k_sp_sums(const uint8_t *buf, const uint32_t *rec_start, const uint32_t *rec_end, int64_t n_rec,
                                                 int32_t len_min, int32_t len_max, double acc_min, double acc_max,
                                                 const double *qprob, int32_t *rec_len, double *accuracy, int64_t *padded) {
  // indexed by the byte itself: qprob[clamp(byte - 33, 0, 93)] -- no test per character
  __shared__ double s_qp[256];
  {
    const int i = threadIdx.x;
    s_qp[i] = qprob[i < 33 ? 0 : i > 126 ? 93 : i - 33];
  }
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rec) return;
  const uint32_t start = rec_start[r];
  const int32_t len = (int32_t)(rec_end[r] - start);
  rec_len[r] = len;
  double acc = 0.0;
  int64_t pad = 0;
  if (len >= len_min && len <= len_max) {
    const uint8_t *p = buf + start;
    double prob = 0.0;
    int32_t n = len;
    int32_t head = (int32_t)((16u - (start & 15u)) & 15u);  // bytes in front of the first 16-byte boundary
    head = head < n ? head : n;
    for (int32_t i = 0; i < head; i++) prob += s_qp[p[i]];
    p += head;
    n -= head;
    const uint4 *p4 = reinterpret_cast<const uint4 *>(p);
    const int32_t n_q = n >> 4;
    // 64 characters per turn as four 16-byte loads, the next 64 on their way while these are added (a lane's loads are its
    // own string's: 64 different lines per load instruction of the wave, so few, wide loads)
    uint4 cur[4], nxt[4];
#pragma unroll
    for (int i = 0; i < 4; i++) cur[i] = (i < n_q) ? p4[i] : make_uint4(0u, 0u, 0u, 0u);
    for (int32_t g0 = 0; g0 < n_q; g0 += 4) {
#pragma unroll
      for (int i = 0; i < 4; i++) nxt[i] = (g0 + 4 + i < n_q) ? p4[g0 + 4 + i] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (g0 + i < n_q) {
          const uint32_t w4[4] = {cur[i].x, cur[i].y, cur[i].z, cur[i].w};
          double qp[16];
#pragma unroll
          for (int d = 0; d < 4; d++)
#pragma unroll
            for (int j = 0; j < 4; j++) qp[d * 4 + j] = s_qp[(w4[d] >> (8 * j)) & 0xffu];
#pragma unroll
          for (int k = 0; k < 16; k++) prob += qp[k];  // in string order
        }
      }
#pragma unroll
      for (int i = 0; i < 4; i++) cur[i] = nxt[i];
    }
    for (int32_t i = n_q << 4; i < n; i++) prob += s_qp[p[i]];
    acc = 1.0 - (prob / (double)len);
    if (acc >= acc_min && acc <= acc_max) pad = ((int64_t)len + 7) & ~(int64_t)7;
  }
  accuracy[r] = acc;
  padded[r] = pad;
}

__global__ __launch_bounds__(256) void k_sp_pool(const uint8_t *buf, const uint32_t *rec_start, const int32_t *rec_len, const int64_t *padded,
                                                 const int64_t *off, int64_t n_rec, uint8_t *pool) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, n_waves = (int64_t)gridDim.x * 4;
  for (int64_t r = wave; r < n_rec; r += n_waves) {
    const int64_t words = padded[r] >> 3;
    if (words == 0) continue;
    const uint32_t start = rec_start[r];
    const int64_t len = rec_len[r];
    const int sh = (int)(start & 7u) * 8;
    const uint64_t *src = reinterpret_cast<const uint64_t *>(buf + (start & ~7u));
    uint64_t *dst = reinterpret_cast<uint64_t *>(pool + off[r]);
    for (int64_t w = lane; w < words; w += 64) {
      uint64_t v = src[w];
      if (sh) v = (v >> sh) | (src[w + 1] << (64 - sh));  // (at most 15 bytes behind the string: inside the window's slack)
      const int64_t rem = len - w * 8;
      if (rem < 8) v &= (1ull << (8 * rem)) - 1ull;  // the pad bytes are 0
      dst[w] = v;
    }
  }
}

unsigned grid_for_waves(int64_t n_waves) { return (unsigned)std::min<int64_t>(std::max<int64_t>((n_waves + 3) / 4, 1), kSpBlocksMax); }

}  // namespace

void launch_sp_count(const uint8_t *buf, int64_t b0, int64_t b1, int64_t *tile_count, int32_t *nul, hipStream_t s) {
  const int64_t n_tiles = sp_tiles(b0, b1);
  if (n_tiles <= 0) return;
  hipLaunchKernelGGL(k_sp_count, dim3(grid_for_waves((n_tiles + kCountUnroll - 1) / kCountUnroll)), dim3(256), 0, s, buf, b0, b1, n_tiles,
                     tile_count, nul);
}

void launch_sp_lines(const uint8_t *buf, int64_t b0, int64_t b1, int phase, const int64_t *tile_base, uint32_t *rec_start,
                     uint32_t *rec_end, hipStream_t s) {
  const int64_t n_tiles = sp_tiles(b0, b1);
  hipLaunchKernelGGL(k_sp_lines, dim3(grid_for_waves(n_tiles)), dim3(256), 0, s, buf, b0, b1, phase, n_tiles, tile_base, rec_start,
                     rec_end);
}

void launch_sp_sums(const uint8_t *buf, const uint32_t *rec_start, const uint32_t *rec_end, int64_t n_rec, int32_t len_min,
                    int32_t len_max, double acc_min, double acc_max, const double *qprob, int32_t *rec_len, double *accuracy,
                    int64_t *padded, hipStream_t s) {
  if (n_rec <= 0) return;
  hipLaunchKernelGGL(k_sp_sums, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, s, buf, rec_start, rec_end, n_rec, len_min, len_max,
                     acc_min, acc_max, qprob, rec_len, accuracy, padded);
}

void launch_sp_pool(const uint8_t *buf, const uint32_t *rec_start, const int32_t *rec_len, const int64_t *padded, const int64_t *off,
                    int64_t n_rec, uint8_t *pool, hipStream_t s) {
  if (n_rec <= 0) return;
  hipLaunchKernelGGL(k_sp_pool, dim3(grid_for_waves(n_rec)), dim3(256), 0, s, buf, rec_start, rec_len, padded, off, n_rec, pool);
}

}  // namespace pbsim
