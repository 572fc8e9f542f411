// bam_stats.hip -- the kernels of pbsim_bam_stats: a summary of the reads of a BAM whose inflated stream lies in HBM with its
// records located (bam_scan.hip, bam_chain.cpp).  The rule: include/pbsim3_amd.h.
//
//   records : one lane per record: its class, its quality field's place, its length, and for an aligned record the CIGAR sums
//             (the CG tag's array where the field is the <l_seq>S<span>N placeholder) and NM (bam_cigar.h's resolve_cigar).  A
//             record of more than 64 ops is taken by its whole wave, op k by lane k mod 64, the sums reduced across the wave
//             (bam_cigar.h's each_long_cigar and wave_cigar_sums).  The counts, the length cells and the totals over scored
//             records are added up per workgroup in LDS and flushed with one vector atomic per cell that is not 0; the identity
//             histogram takes one atomic per scored record.
//   quals   : the quality fields of the records that have qualities, laid end to end, in tiles of kStatsTile bytes: 64
//             consecutive bytes of that axis per lane.  A lane finds its first record by a binary search in the scanned lengths
//             and steps to the later ones, so a long read spreads over many workgroups and short reads share one.  Each piece
//             (the part of one record in a lane's 64 bytes) is read as the aligned sixteen-byte words that hold it, the bytes in
//             front of the piece and behind it masked off.  A lane adds runs of equal q', not bases: the ERRHMM truth files'
//             all-zero qualities are one add per piece.  Per read, esum and the sum of q' go into the record's two cells: by one
//             lane for the whole wave where the wave lies inside one record, else per piece.
//             The 128-bin histogram is privatised per WAVE (four copies of 512 bytes in LDS): LDS atomics of one wave on one
//             address are serialised whatever the layout, and quality values cluster on a few dozen bins, so what a second
//             level of copies could remove is the waves' contention with each other -- that is what the per-wave copy removes,
//             while per-lane copies (128 bins x 256 lanes) would not fit beside eight resident workgroups.  Copy w of bin q
//             lies in bank (128 w + q) mod 64 = q mod 64: lanes on different bins below 64 never conflict.
//   reads   : one lane per record with qualities: acc_ppm, its histogram, the quality totals (per workgroup in LDS first).
//   lengths : rocPRIM's radix sort of the lengths (0 where a record takes no part: they sort in front), rocPRIM's exclusive
//             scan of the sorted lengths into 64-bit running sums, and ten lanes that find the median and N10 .. N90.
//   text    : one lane per record: the line's length, then (after the exclusive scan of the lengths) the bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "bam_cigar.h"
#include "bam_stats.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = kStatsTile / kThreads;
static_assert(kChunk == 64, "a lane takes 64 bytes of the quality axis");

// 1000000 - floor(esum * 1000000 / (l_seq << 32)) for esum <= l_seq << 32 < 2^63: the division by 2^32 first, which the
// nested floors allow
__device__ __forceinline__ u64 acc_ppm_of(u64 esum, u64 l_seq) {
  const u64 t = (esum >> 32) * 1000000ull + (((esum & 0xffffffffull) * 1000000ull) >> 32);
  return 1000000ull - t / l_seq;
}

// the workgroup's cells of the record pass, and where each goes in the call's cells
enum : int { kShN = kStatsCounts, kShBases, kShSqLo, kShSqHi, kShTotals, kShCells = kShTotals + 9 };
__device__ __forceinline__ int cell_of(int k) {
  if (k < kStatsCounts) return kStatsCellCounts + k;
  if (k == kShN) return kStatsCellLenN;
  if (k == kShBases) return kStatsCellLenBases;
  if (k == kShSqLo) return kStatsCellSqLo;
  if (k == kShSqHi) return kStatsCellSqHi;
  return kStatsCellTotals + (k - kShTotals);
}

__global__ __launch_bounds__(kThreads) void k_stats_records(StatsRecs a, int size_bits, uint32_t exclude_flags, int32_t min_mapq, u64 *cells) {
  __shared__ u64 sh[kShCells];
  __shared__ unsigned int sh_min, sh_max;
  if (threadIdx.x < kShCells) sh[threadIdx.x] = 0;
  if (threadIdx.x == 0) sh_min = ~0u, sh_max = 0;
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool aligned = false, bad = false, has_nm = false;  // (no early return: the wave path below needs every lane)
  const uint8_t *p = a.stream, *cig = a.stream;
  uint32_t n_ops = 0;
  int64_t nm = 0;
  uint32_t st = 0;
  if (r < a.n_rec) {
    const uint64_t w = a.rec[r];
    p = a.stream + (int64_t)(w >> size_bits);
    const uint8_t *end = p + 4 + (int64_t)(w & (((uint64_t)1 << size_bits) - 1));
    const uint32_t flag = ld16(p + kBamFlag), n_cigar = ld16(p + kBamNCigarOp), l_seq = ld32(p + kBamLSeq);
    const int32_t ref = (int32_t)ld32(p + kBamRefId), pos = (int32_t)ld32(p + kBamPos);
    int64_t qoff = 0, qlen = 0;
    uint32_t length = 0;
    atomicAdd(&sh[kStatsRecords], 1ull);
    const bool unaligned = (flag & 4u) || ref < 0 || pos < 0 || n_cigar == 0;
    if (flag & exclude_flags) {
      atomicAdd(&sh[kStatsSkippedFlag], 1ull);
    } else if (!unaligned && (int32_t)p[kBamLReadName + 1] < min_mapq) {
      atomicAdd(&sh[kStatsSkippedMapq], 1ull);
    } else {
      st = kStCounted;
      aligned = !unaligned;
      if (aligned) st |= kStAligned;
      atomicAdd(&sh[aligned ? kStatsAligned : kStatsUnaligned], 1ull);
      const uint8_t *field = p + kBamFixed + p[kBamLReadName];
      const uint8_t *q = field + 4 * (int64_t)n_cigar + ((int64_t)l_seq + 1) / 2;  // (the locator: the fields lie inside the record)
      if (l_seq == 0) {
        atomicAdd(&sh[kStatsNoSeq], 1ull);
      } else {
        length = l_seq;
        const u64 sq = (u64)l_seq * l_seq;
        atomicAdd(&sh[kShN], 1ull);
        atomicAdd(&sh[kShBases], (u64)l_seq);
        atomicAdd(&sh[kShSqLo], sq & 0xffffffffull);
        atomicAdd(&sh[kShSqHi], sq >> 32);
        atomicMin(&sh_min, l_seq);
        atomicMax(&sh_max, l_seq);
        qoff = q - a.stream;
        if (*q == 0xffu) {
          atomicAdd(&sh[kStatsNoQual], 1ull);
        } else {
          st |= kStQual;
          qlen = l_seq;
        }
      }
      if (aligned) {
        const ResolvedCigar rc = resolve_cigar(p, end, l_seq, kAuxCg | kAuxNm);
        cig = rc.ops, n_ops = rc.n_ops, bad = rc.bad, has_nm = rc.has_nm, nm = rc.nm;
      }
    }
    a.qoff[r] = qoff;
    a.qlen[r] = qlen;
    a.length[r] = length;
  }
  const bool mine = aligned && !bad;
  CigarSums c;
  if (mine && n_ops <= 64)
    for (uint32_t k = 0; k < n_ops; k++) add_op(ld32(cig + 4 * k), c);
  each_long_cigar(mine, cig, n_ops, [&](int src, const uint8_t *c_ops, int64_t n) {
    const CigarSums whole = wave_cigar_sums(c_ops, n, lane);
    if (lane == src) c = whole;
  });
  if (mine && c.bad) bad = true;
  if (mine && !bad) {
    const u64 indel = c.ins + c.del, cols = c.m + indel;
    if (a.cig) {
      a.cig[4 * r] = (int64_t)cols, a.cig[4 * r + 1] = (int64_t)c.ins, a.cig[4 * r + 2] = (int64_t)c.del, a.cig[4 * r + 3] = (int64_t)c.soft;
      a.nm[r] = nm;
    }
    if (!has_nm || nm < 0) {
      atomicAdd(&sh[kStatsNoNm], 1ull);
    } else {
      st |= kStNm;
      if ((u64)nm < indel || (u64)nm - indel > c.m || cols == 0) {
        atomicAdd(&sh[kStatsNmBad], 1ull);
      } else {
        st |= kStScored;
        const u64 identity = ppm_of(cols - (u64)nm, cols);
        atomicAdd(&sh[kStatsScored], 1ull);
        atomicAdd(&sh[kShTotals + kStatsCols], cols);
        atomicAdd(&sh[kShTotals + kStatsSub], (u64)nm - indel);
        atomicAdd(&sh[kShTotals + kStatsIns], c.ins);
        atomicAdd(&sh[kShTotals + kStatsDel], c.del);
        atomicAdd(&sh[kShTotals + kStatsInsEvents], c.ins_events);
        atomicAdd(&sh[kShTotals + kStatsDelEvents], c.del_events);
        atomicAdd(&sh[kShTotals + kStatsSoft], c.soft);
        atomicAdd(&sh[kShTotals + kStatsHard], c.hard);
        atomicAdd(&sh[kShTotals + kStatsIdentitySum], identity);
        atomicAdd(&cells[kStatsCellHistIdentity + identity / 1000], 1ull);
      }
    }
  }
  if (r < a.n_rec) a.st[r] = (uint8_t)st;
  if (bad) atomicMin(&cells[kStatsCellFault], (u64)(p - a.stream));
  __syncthreads();
  if (threadIdx.x < kShCells && sh[threadIdx.x]) atomicAdd(&cells[cell_of(threadIdx.x)], sh[threadIdx.x]);
  if (threadIdx.x == 0 && sh_min != ~0u) {
    atomicMin(&cells[kStatsCellLenMin], (u64)sh_min);
    atomicMax(&cells[kStatsCellLenMax], (u64)sh_max);
  }
}

__global__ __launch_bounds__(kThreads) void k_stats_quals(StatsRecs a, int64_t n_bytes, const u64 *e_table, u64 *cells) {
  __shared__ unsigned int sh_hist[kThreads / 64][kStatsQBins];
  __shared__ u64 sh_e[kStatsQBins];
  const int tid = threadIdx.x;
  for (int i = tid; i < (kThreads / 64) * kStatsQBins; i += kThreads) (&sh_hist[0][0])[i] = 0;
  if (tid < kStatsQBins) sh_e[tid] = e_table[tid];
  __syncthreads();
  unsigned int *hist = sh_hist[tid >> 6];
  const int64_t *start = a.qlen;  // scanned: where each record's quality bytes begin on the axis; start[n_rec] == n_bytes
  const int64_t v0 = (int64_t)blockIdx.x * kStatsTile + (int64_t)tid * kChunk;
  const bool active = v0 < n_bytes;
  const int64_t v1 = min(v0 + kChunk, n_bytes);
  int64_t r = 0;
  bool single = false;
  if (active) {
    r = last_at_most(start, a.n_rec, v0);  // (of equal entries the last: the one that has bytes)
    single = start[r + 1] >= v1;
  }
  // a wave inside one record adds its sums once
  const int64_t r0 = __shfl(r, 0, 64);
  const bool uniform = __shfl((int)active, 0, 64) != 0 && __all(!active || (single && r == r0));
  u64 e_wave = 0, q_wave = 0;
  if (active) {
    int64_t v = v0;
    while (v < v1) {
      int64_t next = start[r + 1];
      while (next <= v) next = start[++r + 1];  // (records without quality bytes in between; v < n_bytes = start[n_rec] ends it)
      const int64_t seg_end = min(next, v1);
      const int64_t from = a.qoff[r] + (v - start[r]), to = from + (seg_end - v);  // inside the record's quality field
      u64 e = 0, q = 0;
      uint32_t bin = 0, bin_n = 0;
      for (int64_t blk = from & ~(int64_t)15; blk < to; blk += 16) {  // (the stream is 16-byte aligned and readable kBamSlack bytes past its end)
        const uint4 x = *reinterpret_cast<const uint4 *>(a.stream + blk);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
        const int lo = (int)(max(from, blk) - blk), hi = (int)(min(to, blk + 16) - blk);
#pragma unroll
        for (int j = 0; j < 16; j++) {
          if (j >= lo && j < hi) {
            const uint32_t b = min((w[j >> 2] >> (8 * (j & 3))) & 0xffu, 127u);
            if (b != bin) {
              if (bin_n) {
                atomicAdd(&hist[bin], bin_n);
                e += (u64)bin_n * sh_e[bin];
                q += (u64)bin_n * bin;
              }
              bin = b, bin_n = 0;
            }
            bin_n++;
          }
        }
      }
      if (bin_n) {
        atomicAdd(&hist[bin], bin_n);
        e += (u64)bin_n * sh_e[bin];
        q += (u64)bin_n * bin;
      }
      if (uniform) {
        e_wave += e, q_wave += q;
      } else {
        atomicAdd(&a.qsum[2 * r], e);
        atomicAdd(&a.qsum[2 * r + 1], q);
      }
      v = seg_end;
    }
  }
  if (uniform) {
    e_wave = wave_sum(e_wave), q_wave = wave_sum(q_wave);
    if ((tid & 63) == 0) {
      atomicAdd(&a.qsum[2 * r0], e_wave);
      atomicAdd(&a.qsum[2 * r0 + 1], q_wave);
    }
  }
  __syncthreads();
  if (tid < kStatsQBins) {
    u64 sum = 0;
    for (int w = 0; w < kThreads / 64; w++) sum += sh_hist[w][tid];
    if (sum) atomicAdd(&cells[kStatsCellHistQ + tid], sum);
  }
}

__global__ __launch_bounds__(kThreads) void k_stats_reads(StatsRecs a, u64 *cells) {
  __shared__ u64 sh[3];
  if (threadIdx.x < 3) sh[threadIdx.x] = 0;
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r < a.n_rec && (a.st[r] & kStQual)) {
    const u64 acc = acc_ppm_of(a.qsum[2 * r], (u64)a.length[r]);
    atomicAdd(&cells[kStatsCellHistQacc + acc / 1000], 1ull);
    atomicAdd(&sh[0], acc);
    atomicAdd(&sh[1], 1ull);
    atomicAdd(&sh[2], a.qsum[2 * r + 1]);
  }
  __syncthreads();
  if (threadIdx.x < 3 && sh[threadIdx.x]) atomicAdd(&cells[kStatsCellTotals + kStatsAccSum + threadIdx.x], sh[threadIdx.x]);
}
static_assert(kStatsAccReads == kStatsAccSum + 1 && kStatsQSum == kStatsAccSum + 2, "k_stats_reads flushes the three in this order");

struct Widen {
  __host__ __device__ u64 operator()(uint32_t v) const { return (u64)v; }
};

// lane 0: the median; lane k = 1 .. 9: N(10 k).  sorted[0, n_all) ascending, the n records that take part behind the zeros;
// sums: the exclusive running sums.  Descending from the top, the running sum at element i is bases - sums[i]: it grows as i
// falls, so the first record at which it suffices is the largest i where it does.
__global__ void k_stats_nx(const uint32_t *sorted, const u64 *sums, int64_t n_all, int64_t n, u64 bases, int64_t *out) {
  const int k = threadIdx.x;
  if (k > 9) return;
  const int64_t first = n_all - n;
  if (k == 0) {
    out[0] = sorted[first + (n - 1) / 2];
    return;
  }
  const u64 x = 10ull * k, want_hi = __umul64hi(x, bases), want_lo = x * bases;
  int64_t lo = first, hi = n_all;  // suffices at lo (there the sum is all bases), not at hi (or hi == n_all)
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const u64 run = bases - sums[mid], got_hi = __umul64hi(run, 100ull), got_lo = run * 100ull;
    if (got_hi > want_hi || (got_hi == want_hi && got_lo >= want_lo)) lo = mid;
    else hi = mid;
  }
  out[k] = sorted[lo];
}

// the nine numbers behind a counted record's name and class, and which of them the record defines (bit j: f[j])
__device__ __forceinline__ uint32_t line_fields(const StatsRecs &a, int64_t r, uint32_t st, u64 f[9]) {
  uint32_t has = 1;
  f[0] = ld32(a.stream + (int64_t)(a.rec[r] >> kBamSamplePacking.size_bits) + kBamLSeq);
  if (st & kStAligned) {
    has |= 2u | 8u | 16u | 32u;
    f[1] = (u64)a.cig[4 * r], f[3] = (u64)a.cig[4 * r + 1], f[4] = (u64)a.cig[4 * r + 2], f[5] = (u64)a.cig[4 * r + 3];
    if (st & kStNm) has |= 4u, f[2] = (u64)a.nm[r];
    if (st & kStScored) has |= 64u, f[6] = ppm_of(f[1] - f[2], f[1]);
  }
  if (st & kStQual) {
    has |= 128u | 256u;
    f[7] = a.qsum[2 * r + 1] * 1000ull / f[0];
    f[8] = acc_ppm_of(a.qsum[2 * r], f[0]);
  }
  return has;
}

__global__ __launch_bounds__(kThreads) void k_stats_line_sizes(StatsRecs a, int64_t *len) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.n_rec) return;
  const uint32_t st = a.st[r];
  int64_t l = 0;
  if (st & kStCounted) {
    u64 f[9];
    const uint32_t has = line_fields(a, r, st, f);
    const uint8_t *name = a.stream + (int64_t)(a.rec[r] >> kBamSamplePacking.size_bits) + kBamFixed;
    while (name[l]) l++;  // (the locator: the name ends with a NUL inside the record)
    l += 3 + fields_len(has, f, 9);  // the tab and the class, the line feed
  }
  len[r] = l;
}

__global__ __launch_bounds__(kThreads) void k_stats_line_fill(StatsRecs a, const int64_t *off, char *text) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.n_rec) return;
  const uint32_t st = a.st[r];
  if (!(st & kStCounted)) return;
  u64 f[9];
  const uint32_t has = line_fields(a, r, st, f);
  char *o = text + off[r];
  for (const uint8_t *name = a.stream + (int64_t)(a.rec[r] >> kBamSamplePacking.size_bits) + kBamFixed; *name; name++) *o++ = (char)*name;
  *o++ = '\t';
  *o++ = st & kStAligned ? 'A' : 'U';
  *put_fields(o, has, f, 9) = '\n';
}

}  // namespace

void launch_stats_records(StatsRecs r, int32_t exclude_flags, int32_t min_mapq, unsigned long long *cells, hipStream_t s) {
  if (r.n_rec <= 0) return;
  hipLaunchKernelGGL(k_stats_records, dim3(blocks_of(r.n_rec)), dim3(kThreads), 0, s, r, kBamSamplePacking.size_bits, (uint32_t)exclude_flags,
                     min_mapq, cells);
}

void launch_stats_quals(StatsRecs r, int64_t n_bytes, const unsigned long long *e_table, unsigned long long *cells, hipStream_t s) {
  if (r.n_rec <= 0 || n_bytes <= 0) return;
  hipLaunchKernelGGL(k_stats_quals, dim3(blocks_of(n_bytes, kStatsTile)), dim3(kThreads), 0, s, r, n_bytes, e_table, cells);
}

void launch_stats_reads(StatsRecs r, unsigned long long *cells, hipStream_t s) {
  if (r.n_rec <= 0) return;
  hipLaunchKernelGGL(k_stats_reads, dim3(blocks_of(r.n_rec)), dim3(kThreads), 0, s, r, cells);
}

void launch_stats_line_sizes(StatsRecs r, int64_t *len, hipStream_t s) {
  if (r.n_rec <= 0) return;
  hipLaunchKernelGGL(k_stats_line_sizes, dim3(blocks_of(r.n_rec)), dim3(kThreads), 0, s, r, len);
}

void launch_stats_line_fill(StatsRecs r, const int64_t *off, char *text, hipStream_t s) {
  if (r.n_rec <= 0) return;
  hipLaunchKernelGGL(k_stats_line_fill, dim3(blocks_of(r.n_rec)), dim3(kThreads), 0, s, r, off, text);
}

hipError_t stats_sort_lengths(void *tmp, size_t *tmp_bytes, const uint32_t *in, uint32_t *out, int64_t n, hipStream_t s) {
  return rocprim::radix_sort_keys(tmp, *tmp_bytes, in, out, (size_t)n, 0u, 32u, s);
}

hipError_t stats_scan_lengths(void *tmp, size_t *tmp_bytes, const uint32_t *sorted, unsigned long long *sums, int64_t n, hipStream_t s) {
  return rocprim::exclusive_scan(tmp, *tmp_bytes, rocprim::make_transform_iterator(sorted, Widen()), sums, 0ull, (size_t)n, rocprim::plus<u64>(), s);
}

void launch_stats_nx(const uint32_t *sorted, const unsigned long long *sums, int64_t n_all, int64_t n, unsigned long long bases, int64_t *out,
                     hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_stats_nx, dim3(1), dim3(64), 0, s, sorted, sums, n_all, n, bases, out);
}

}  // namespace pbsim
