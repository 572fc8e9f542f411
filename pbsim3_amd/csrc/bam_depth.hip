// bam_depth.hip -- the kernels of pbsim_bam_depth: the depth of coverage of a BAM whose inflated stream lies in HBM with its
// records located (bam_scan.hip, bam_chain.cpp).  The rule: include/pbsim3_amd.h.
//
//   events : one lane per record: its skip class, its CIGAR (the CG tag's array where the field is the <l_seq>S<span>N
//            placeholder: bam_cigar.h's resolve_cigar, which walks the aux fields of no other record here), and for each
//            maximal covered interval +1 at its start and -1 at its end into a difference array of int32 over the
//            concatenated references -- l_ref + 1 slots each, so that an end at l_ref has a place.  Adjacent covering ops
//            merge, so a record without N (and, where deletions do not count, without D) is two atomics.  A record of more
//            than 64 ops is taken by its whole wave (bam_cigar.h's each_long_cigar), op k by lane k mod 64: a wave prefix sum
//            of the reference advances gives each op its position, two ballots tell each lane whether an interval is open in
//            front of it, and position and open interval are carried from one round of 64 to the next.  Clipping is
//            min(position, l_ref): what lies wholly past the end puts its +1 and its -1 into the extra slot, where they
//            cancel.
//   scan   : rocPRIM's inclusive scan in place.  Every reference's slots sum to zero, so nothing is segmented.
//   runs   : one pass over the depths in tiles of kDepthTile slots, 16 consecutive slots per lane; the reference of a lane's
//            first slot comes from a binary search in the offset table, the later ones by stepping.  The histogram and the
//            references' covered / sum / max are added up per lane over runs of equal destination, then per workgroup in LDS
//            (the first kLdsRefs references of a tile; a tile that spans more puts the rest straight into global memory), and
//            flushed with one vector atomic per cell that is not 0.  bedgraph: run starts (the depth changes, or a reference
//            begins) are counted per tile, and after the exclusive scan of the tiles a second pass writes each run's
//            reference, start and depth.  window: the pass adds each window's depths into its 64-bit sum.
//   text   : one lane per line: the decimal length, then (after the exclusive scan of the lengths) the bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>

#include "bam_cigar.h"
#include "bam_depth.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = kDepthTile / kThreads;
constexpr int kLdsRefs = 128;
static_assert(kPerLane == 16, "a lane loads its slots as four int4");

// MIDNSHP=X.  0: neither advances nor covers (I S H P, and any op of length 0); 1: covers; 2: advances only
__device__ __forceinline__ int op_class(uint32_t v, bool deletions) {
  if ((v >> 4) == 0) return 0;
  const uint32_t op = v & 15u;
  if (op == 0 || op == 7 || op == 8) return 1;
  if (op == 2) return deletions ? 1 : 2;
  return op == 3 ? 2 : 0;
}

__global__ __launch_bounds__(kThreads) void k_depth_events(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, int size_bits, DepthRefs refs,
                                                          uint32_t exclude_flags, int32_t min_mapq, int32_t count_deletions, int32_t *diff,
                                                          u64 *cells) {
  __shared__ unsigned int sh[kDepthCounts];
  if (threadIdx.x < kDepthCounts) sh[threadIdx.x] = 0;
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool deletions = count_deletions != 0;
  bool counted = false, bad = false, clipped = false;  // (no early return: the wave path below needs every lane)
  const uint8_t *p = stream, *cig = stream;
  uint32_t n_ops = 0;
  int64_t pos = 0, base = 0, l_ref = 0;
  if (r < n_rec) {
    const uint64_t w = rec[r];
    p = stream + (int64_t)(w >> size_bits);
    const uint8_t *end = p + 4 + (int64_t)(w & (((uint64_t)1 << size_bits) - 1));
    const uint32_t flag = ld16(p + kBamFlag);
    const int32_t ref = (int32_t)ld32(p + kBamRefId);
    pos = (int32_t)ld32(p + kBamPos);
    atomicAdd(&sh[kDepthRecords], 1u);
    if (flag & exclude_flags) {
      atomicAdd(&sh[kDepthSkippedFlag], 1u);
    } else if (ref < 0 || pos < 0) {
      atomicAdd(&sh[kDepthSkippedUnplaced], 1u);
    } else if ((int32_t)p[kBamLReadName + 1] < min_mapq) {
      atomicAdd(&sh[kDepthSkippedMapq], 1u);
    } else if (ref >= refs.n_ref) {  // (the locator has refused it already)
      bad = true;
    } else {
      counted = true;
      atomicAdd(&sh[kDepthCounted], 1u);
      base = refs.off[ref];
      l_ref = refs.off[ref + 1] - base - 1;
      // (CG alone: the aux fields are walked only where the field is the placeholder)
      const ResolvedCigar rc = resolve_cigar(p, end, ld32(p + kBamLSeq), kAuxCg);
      cig = rc.ops, n_ops = rc.n_ops, bad = rc.bad;
    }
  }
  const bool mine = counted && !bad;
  if (mine && n_ops <= 64) {
    int64_t cur = pos, start = 0;
    bool open = false;
    for (uint32_t k = 0; k < n_ops; k++) {
      const uint32_t v = ld32(cig + 4 * k);
      if ((v & 15u) > 8) {
        bad = true;
        break;
      }
      const int c = op_class(v, deletions);
      if (c == 0) continue;
      if (c == 1 && !open) {
        open = true;
        start = cur;
      }
      if (c == 2 && open) {
        open = false;
        if (start < l_ref) {
          atomicAdd(&diff[base + start], 1);
          atomicAdd(&diff[base + min(cur, l_ref)], -1);
        }
      }
      cur += (int64_t)(v >> 4);
      if (c == 1 && cur > l_ref) clipped = true;
    }
    if (open && start < l_ref) {
      atomicAdd(&diff[base + start], 1);
      atomicAdd(&diff[base + min(cur, l_ref)], -1);
    }
  }
  each_long_cigar(mine, cig, n_ops, [&](int src, const uint8_t *c_ops, int64_t n) {
    const int64_t r_base = __shfl(base, src, 64), r_len = __shfl(l_ref, src, 64);
    int64_t carry = __shfl(pos, src, 64);
    bool carry_open = false, any_bad = false, any_clip = false;
    for (int64_t k0 = 0; k0 < n; k0 += 64) {
      const int64_t k = k0 + lane;
      const uint32_t v = k < n ? ld32(c_ops + 4 * k) : 0u;
      if ((v & 15u) > 8) any_bad = true;
      const int c = op_class(v, deletions);
      const int64_t adv = c ? (int64_t)(v >> 4) : 0;
      const int64_t incl = (int64_t)wave_scan((u64)adv, lane);
      const int64_t at = carry + incl - adv;
      const uint64_t cover = __ballot(c == 1), sig = cover | __ballot(c == 2);
      const uint64_t below = sig & (((uint64_t)1 << lane) - 1);
      const bool open = below ? (cover >> (63 - __clzll((long long)below))) & 1 : carry_open;
      if (c == 1 && !open) atomicAdd(&diff[r_base + min(at, r_len)], 1);
      if (c == 2 && open) atomicAdd(&diff[r_base + min(at, r_len)], -1);
      if (c == 1 && at + adv > r_len) any_clip = true;
      carry += __shfl(incl, 63, 64);
      if (sig) carry_open = (cover >> (63 - __clzll((long long)sig))) & 1;
    }
    if (carry_open && lane == 0) atomicAdd(&diff[r_base + min(carry, r_len)], -1);
    const bool w_bad = __ballot(any_bad) != 0, w_clip = __ballot(any_clip) != 0;
    if (lane == src) {
      bad = w_bad;
      clipped = w_clip;
    }
  });
  if (clipped) atomicAdd(&sh[kDepthClipped], 1u);
  if (bad) atomicMin(&cells[kDepthCellFault], (u64)(p - stream));
  __syncthreads();
  if (threadIdx.x < kDepthCounts && sh[threadIdx.x]) atomicAdd(&cells[kDepthCellCounts + threadIdx.x], (u64)sh[threadIdx.x]);
}

// what a lane has added up for one reference, into the workgroup's cells or, past them, into global memory
__device__ __forceinline__ void flush_ref(int32_t r, int32_t r_first, uint32_t covered, u64 sum, uint32_t top, unsigned int *sh_cov, u64 *sh_sum,
                                          unsigned int *sh_max, u64 *ref_stat) {
  if (covered == 0) return;
  const int32_t k = r - r_first;
  if (k < kLdsRefs) {
    atomicAdd(&sh_cov[k], covered);
    atomicAdd(&sh_sum[k], sum);
    atomicMax(&sh_max[k], top);
  } else {
    atomicAdd(&ref_stat[3 * (int64_t)r], (u64)covered);
    atomicAdd(&ref_stat[3 * (int64_t)r + 1], sum);
    atomicMax(&ref_stat[3 * (int64_t)r + 2], (u64)top);
  }
}

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void k_depth_runs(const int32_t *depth, int64_t n_slots, DepthRefs refs, int64_t window, u64 *cells,
                                                        u64 *ref_stat, int64_t *tile_runs, u64 *win_sum, int32_t *run_ref, int32_t *run_start,
                                                        int32_t *run_depth) {
  __shared__ unsigned int sh_hist[256], sh_cov[kLdsRefs], sh_max[kLdsRefs], sh_runs, sh_wave[kThreads / 64];
  __shared__ u64 sh_sum[kLdsRefs];
  __shared__ int32_t sh_first;
  const int tid = threadIdx.x;
  if (!kWrite) {
    sh_hist[tid] = 0;
    if (tid < kLdsRefs) sh_cov[tid] = 0, sh_max[tid] = 0, sh_sum[tid] = 0;
    if (tid == 0) sh_runs = 0;
  }
  const int64_t i0 = (int64_t)blockIdx.x * kDepthTile + (int64_t)tid * kPerLane;
  int32_t d[kPerLane];
  int32_t prev = 0;
  int32_t r = 0;
  if (i0 < n_slots) {  // (the array is padded to whole tiles: a lane's int4 loads stay inside it)
    const int4 *q = (const int4 *)(depth + i0);
    for (int j = 0; j < kPerLane / 4; j++) {
      const int4 x = q[j];
      d[4 * j] = x.x, d[4 * j + 1] = x.y, d[4 * j + 2] = x.z, d[4 * j + 3] = x.w;
    }
    if (i0 > 0) prev = depth[i0 - 1];
    r = last_at_most(refs.off, refs.n_ref, i0);
  }
  if (tid == 0) sh_first = r;
  __syncthreads();
  const int32_t r_first = sh_first;
  // pass 1: the statistics and the number of run starts; pass 2: the runs
  uint32_t starts = 0;
  if (!kWrite && i0 < n_slots) {
    int64_t from = refs.off[r], next = refs.off[r + 1];
    uint32_t covered = 0, top = 0, bin = 0, bin_n = 0;
    u64 sum = 0, w_sum = 0;
    int64_t w_id = -1, w_end = 0;
    for (int j = 0; j < kPerLane && i0 + j < n_slots; j++) {
      const int64_t i = i0 + j;
      if (i >= next) {
        flush_ref(r, r_first, covered, sum, top, sh_cov, sh_sum, sh_max, ref_stat);
        covered = 0, top = 0, sum = 0;
        do {
          r++;
          from = next;
          next = refs.off[r + 1];
        } while (i >= next);
        if (w_sum) atomicAdd(&win_sum[w_id], w_sum);
        w_sum = 0, w_id = -1;
      }
      if (i == next - 1) continue;  // the slot behind the reference's last position
      const int32_t x = d[j];
      const int64_t at = i - from;
      const uint32_t b = (uint32_t)min(x, 255);
      if (b != bin) {
        if (bin_n) atomicAdd(&sh_hist[bin], bin_n);
        bin = b, bin_n = 0;
      }
      bin_n++;
      if (x > 0) {
        covered++;
        sum += (u64)x;
        top = max(top, (uint32_t)x);
      }
      if (window > 0) {
        if (w_id < 0 || at >= w_end) {
          if (w_sum) atomicAdd(&win_sum[w_id], w_sum);
          w_sum = 0;
          const int64_t kw = w_id < 0 ? at / window : w_id - refs.win[r] + 1;
          w_id = refs.win[r] + kw;
          w_end = (kw + 1) * window;
        }
        w_sum += (u64)x;
      } else if (at == 0 || x != (j ? d[j - 1] : prev)) {
        starts++;
      }
    }
    flush_ref(r, r_first, covered, sum, top, sh_cov, sh_sum, sh_max, ref_stat);
    if (bin_n) atomicAdd(&sh_hist[bin], bin_n);
    if (w_sum) atomicAdd(&win_sum[w_id], w_sum);
    if (starts) atomicAdd(&sh_runs, starts);
  }
  if (kWrite) {
    int64_t from = 0, next = 0;
    if (i0 < n_slots) {
      from = refs.off[r], next = refs.off[r + 1];
      int32_t rr = r;
      int64_t f = from, nx = next;
      for (int j = 0; j < kPerLane && i0 + j < n_slots; j++) {
        const int64_t i = i0 + j;
        while (i >= nx) rr++, f = nx, nx = refs.off[rr + 1];
        if (i == nx - 1) continue;
        if (i == f || d[j] != (j ? d[j - 1] : prev)) starts++;
      }
    }
    // where this lane's runs go: the tile's first run, the waves in front, the lanes in front
    uint32_t incl = starts;
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t t = __shfl_up(incl, s, 64);
      if ((tid & 63) >= s) incl += t;
    }
    if ((tid & 63) == 63) sh_wave[tid >> 6] = incl;
    __syncthreads();
    int64_t k = tile_runs[blockIdx.x] + (incl - starts);
    for (int w = 0; w < (tid >> 6); w++) k += sh_wave[w];
    if (i0 < n_slots) {
      for (int j = 0; j < kPerLane && i0 + j < n_slots; j++) {
        const int64_t i = i0 + j;
        while (i >= next) r++, from = next, next = refs.off[r + 1];
        if (i == next - 1) continue;
        if (i == from || d[j] != (j ? d[j - 1] : prev)) {
          run_ref[k] = r;
          run_start[k] = (int32_t)(i - from);
          run_depth[k] = d[j];
          k++;
        }
      }
    }
    return;
  }
  __syncthreads();
  if (sh_hist[tid]) atomicAdd(&cells[kDepthCellHist + tid], (u64)sh_hist[tid]);
  if (tid < kLdsRefs && sh_cov[tid]) {
    const int64_t at = 3 * ((int64_t)r_first + tid);
    atomicAdd(&ref_stat[at], (u64)sh_cov[tid]);
    atomicAdd(&ref_stat[at + 1], sh_sum[tid]);
    atomicMax(&ref_stat[at + 2], (u64)sh_max[tid]);
  }
  if (tid == 0 && window == 0) tile_runs[blockIdx.x] = (int64_t)sh_runs;
}

// line k: its reference and the numbers behind the name (three for bedgraph, four for window)
__device__ __forceinline__ int line_fields(int64_t k, int64_t n_lines, const DepthRefs &refs, int64_t window, const int32_t *run_ref,
                                           const int32_t *run_start, const int32_t *run_depth, const u64 *win_sum, int32_t *ref, u64 f[4]) {
  if (window == 0) {
    const int32_t r = run_ref[k];
    *ref = r;
    f[0] = (u64)run_start[k];
    f[1] = k + 1 < n_lines && run_ref[k + 1] == r ? (u64)run_start[k + 1] : (u64)(refs.off[r + 1] - refs.off[r] - 1);
    f[2] = (u64)run_depth[k];
    return 3;
  }
  const int32_t r = last_at_most(refs.win, refs.n_ref, k);  // (the last of equal entries: references without windows lie in front)
  const int64_t l_ref = refs.off[r + 1] - refs.off[r] - 1, start = (k - refs.win[r]) * window, end = min(start + window, l_ref);
  const u64 sum = win_sum[k], len = (u64)(end - start);
  *ref = r;
  f[0] = (u64)start;
  f[1] = (u64)end;
  f[2] = sum;
  f[3] = sum / len * 1000 + sum % len * 1000 / len;  // sum * 1000 / len inside 64 bits
  return 4;
}

__global__ __launch_bounds__(kThreads) void k_depth_line_sizes(int64_t n_lines, DepthRefs refs, int64_t window, const int32_t *run_ref,
                                                              const int32_t *run_start, const int32_t *run_depth, const u64 *win_sum,
                                                              int64_t *len) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= n_lines) return;
  int32_t r;
  u64 f[4];
  const int n = line_fields(k, n_lines, refs, window, run_ref, run_start, run_depth, win_sum, &r, f);
  len[k] = refs.name_at[r + 1] - refs.name_at[r] + fields_len(~0u, f, n) + 1;  // the name, a tab in front of each number, the line feed
}

__global__ __launch_bounds__(kThreads) void k_depth_line_fill(int64_t n_lines, DepthRefs refs, int64_t window, const int32_t *run_ref,
                                                             const int32_t *run_start, const int32_t *run_depth, const u64 *win_sum,
                                                             const int64_t *off, char *text) {
  const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= n_lines) return;
  int32_t r;
  u64 f[4];
  const int n = line_fields(k, n_lines, refs, window, run_ref, run_start, run_depth, win_sum, &r, f);
  char *o = text + off[k];
  const char *name = refs.names + refs.name_at[r];
  const int64_t l_name = refs.name_at[r + 1] - refs.name_at[r];
  for (int64_t j = 0; j < l_name; j++) *o++ = name[j];
  *put_fields(o, ~0u, f, n) = '\n';
}

}  // namespace

void launch_depth_events(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, BamPacking pk, DepthRefs refs, int32_t exclude_flags,
                         int32_t min_mapq, int32_t count_deletions, int32_t *diff, unsigned long long *cells, hipStream_t s) {
  if (n_rec <= 0) return;
  hipLaunchKernelGGL(k_depth_events, dim3(blocks_of(n_rec)), dim3(kThreads), 0, s, stream, rec, n_rec, pk.size_bits, refs, (uint32_t)exclude_flags,
                     min_mapq, count_deletions, diff, cells);
}

hipError_t depth_scan(void *tmp, size_t *tmp_bytes, int32_t *diff, int64_t n, hipStream_t s) {
  return rocprim::inclusive_scan(tmp, *tmp_bytes, diff, diff, (size_t)n, rocprim::plus<int32_t>(), s);
}

void launch_depth_runs(const int32_t *depth, int64_t n_slots, DepthRefs refs, int64_t window, unsigned long long *cells,
                       unsigned long long *ref_stat, int64_t *tile_runs, unsigned long long *win_sum, bool runs, int32_t *run_ref,
                       int32_t *run_start, int32_t *run_depth, hipStream_t s) {
  if (n_slots <= 0) return;
  const dim3 grid(blocks_of(n_slots, kDepthTile)), block(kThreads);
  if (runs) hipLaunchKernelGGL(k_depth_runs<true>, grid, block, 0, s, depth, n_slots, refs, window, cells, ref_stat, tile_runs, win_sum, run_ref,
                               run_start, run_depth);
  else hipLaunchKernelGGL(k_depth_runs<false>, grid, block, 0, s, depth, n_slots, refs, window, cells, ref_stat, tile_runs, win_sum, run_ref,
                          run_start, run_depth);
}

void launch_depth_line_sizes(int64_t n_lines, DepthRefs refs, int64_t window, const int32_t *run_ref, const int32_t *run_start,
                             const int32_t *run_depth, const unsigned long long *win_sum, int64_t *len, hipStream_t s) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_depth_line_sizes, dim3(blocks_of(n_lines)), dim3(kThreads), 0, s, n_lines, refs, window, run_ref, run_start, run_depth,
                     win_sum, len);
}

void launch_depth_line_fill(int64_t n_lines, DepthRefs refs, int64_t window, const int32_t *run_ref, const int32_t *run_start,
                            const int32_t *run_depth, const unsigned long long *win_sum, const int64_t *off, char *text, hipStream_t s) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_depth_line_fill, dim3(blocks_of(n_lines)), dim3(kThreads), 0, s, n_lines, refs, window, run_ref, run_start, run_depth,
                     win_sum, off, text);
}

}  // namespace pbsim
