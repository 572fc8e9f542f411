// bam_pileup_walk.h -- what is about the pile: the column pass of pbsim_bam_pileup as a template over bam_cigar.h's walk, for
// bam_pileup.hip (kLog false: without a slot beside the op in LDS, and nothing of the log is compiled in) and bam_consensus.hip
// (kLog true: besides, every inserted base of an anchored I op is appended to a log); the genome's record of a position and a
// site's cells.  Device code: included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bam_cigar.h"
#include "bam_pileup.h"

namespace pbsim {
namespace pilewalk {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSegBlocksMax = 2048;  // workgroups of the column pass, as bam_errors.hip's: one input takes both past their caps

// The log of inserted bases: one entry per column of an anchored I op with an offset j below max_ins inside the op,
// (position << 24) | (j << 8) | class: the anchor's position as in the genome's buffers (below 2^40), j below 2^16, the class
// 0 .. 4.  *count is the entries asked for; only those below cap are written.  A wave takes the slots of a round's 64 ops with
// one atomic: every lane knows how many entries its op leaves inside the segment, a wave scan gives each op its first slot, and
// the lanes that walk the columns find it in LDS beside the op -- no atomic and no vote in the divergent part of the walk.
struct InsLog {
  u64 *entry;
  u64 *count;
  u64 cap;
  uint32_t max_ins;
};
struct NoLog {};
constexpr int kInsLogPosShift = 24, kInsLogOffShift = 8;

template <bool kLog>
__global__ __launch_bounds__(kThreads) void k_pile_columns(ErrRecs a, ErrRefs refs, const uint8_t *genome, const ErrSegment *seg, int64_t n_seg,
                                                           uint32_t min_baseq, uint32_t *table, u64 *cells,
                                                           typename std::conditional<kLog, InsLog, NoLog>::type log) {
  typedef typename std::conditional<kLog, WaveLdsSlot, WaveLds>::type Lds;  // kLog: the slot of offset 0 of each op of the round
  __shared__ unsigned int sh_unanchored[kWaves];
  __shared__ Lds sh_walk[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < kWaves) sh_unanchored[tid] = 0;
  __syncthreads();
  for (int64_t s = (int64_t)blockIdx.x * kWaves + wave; s < n_seg; s += (int64_t)gridDim.x * kWaves) {
    const ErrSegment sg = seg[s];
    const RecView rv = view_of(a, sg.rec);
    const u64 pos = (u64)rv.pos;  // (a scored record: pos >= 0)
    const bool has_qual = (a.st[sg.rec] & kEsQual) != 0;
    const u64 l_ref = (u64)refs.l_ref[rv.ref_id];
    const uint8_t *g_seq = genome + refs.at[rv.ref_id];
    uint32_t *tab = table + refs.at[rv.ref_id] * kPileWidth;  // positions [0, l_ref) of this reference: the record pass held pos + span to it
    const ColumnRange range = range_of(rv, sg);
    walk_columns(
        range, lane, &sh_walk[wave],
        [&](uint32_t v, u64 col, u64 my_col, u64 my_ref) {
          if (col == 0 || (v & 15u) != kOpI) v = 0;  // (only an I op with columns does anything here)
          // an I op adds where its first column lies: to the position in front of it, or, with none consumed yet, to the call's cell
          if (v && my_col >= range.x_lo && my_col < range.x_hi) {
            if (my_ref > pos) {
              if (my_ref - 1 < l_ref) atomicAdd(&tab[(my_ref - 1) * kPileWidth + kPcIns], 1u);  // (always: pos + span <= l_ref)
            } else {
              atomicAdd(&sh_unanchored[wave], 1u);
            }
          }
          u64 my_slot = 0;
          if constexpr (kLog) {
            // the entries this op leaves: its offsets inside the segment, below max_ins, where it is an anchored I op
            u64 j_lo = 0, n_mine = 0;
            if (v && my_ref > pos && my_ref - 1 < l_ref && my_col < range.x_hi && my_col + col > range.x_lo) {
              j_lo = my_col < range.x_lo ? range.x_lo - my_col : 0;
              const u64 j_hi = min(min(my_col + col, range.x_hi) - my_col, (u64)log.max_ins);
              n_mine = j_hi > j_lo ? j_hi - j_lo : 0;
            }
            const u64 in_n = wave_scan(n_mine, lane), all_n = __shfl(in_n, 63, 64);
            u64 base = 0;
            if (all_n != 0) {  // (the same for every lane)
              if (lane == 0) base = atomicAdd(log.count, all_n);
              base = __shfl(base, 0, 64);
            }
            my_slot = base + (in_n - n_mine) - j_lo;  // (offset j lies at my_slot + j, modulo 2^64 where j_lo is not reached)
          }
          return my_slot;
        },
        [&](const Column &c) {
          if (!c.valid) return;
          if (c.op == kOpI) {
            if constexpr (kLog) {
              // an inserted base: offset j of its op, which is anchored where some of the reference lies in front of it
              const u64 j = c.off, anchor = c.rp - c.off, slot = c.slot + j;
              if (anchor > pos && anchor - 1 < l_ref && j < log.max_ins && slot < log.cap) {
                u64 entry = ~(u64)0;  // (never: the query length is l_seq; an entry no later pass takes)
                if (c.qp < rv.l_seq)
                  entry = ((u64)(refs.at[rv.ref_id] + (int64_t)anchor - 1) << kInsLogPosShift) | (j << kInsLogOffShift) | code_class(base_code(rv.bases, c.qp));
                log.entry[slot] = entry;
              }
            }
            return;
          }
          if (c.rp >= l_ref) return;  // (never: pos + span <= l_ref)
          uint32_t cell = kPcDel;
          if (c.op != kOpD) {
            if (c.qp >= rv.l_seq) return;  // (never: the query length is l_seq)
            const uint32_t nib = base_code(rv.bases, c.qp);
            cell = nib == 0 ? ref_class(g_seq[c.rp]) : code_class(nib);
            if (has_qual && (uint32_t)rv.qual[c.qp] < min_baseq) cell = kPcMasked;
          }
          atomicAdd(&tab[c.rp * kPileWidth + cell], 1u);
        });
  }
  __syncthreads();
  if (tid == 0) {
    u64 sum = 0;
    for (int w = 0; w < kWaves; w++) sum += sh_unanchored[w];
    if (sum) atomicAdd(&cells[kPileCellUnanchored], sum);
  }
}

// the genome's record that holds index i of its buffers (bases or the padding behind them)
__device__ __forceinline__ int record_of(const PileGenome &g, int64_t i) {
  int lo = 0, hi = g.n - 1;  // at[lo] <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (g.at[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct Site {
  uint32_t c[kPileWidth];
  u64 depth;
};

__device__ __forceinline__ Site load_site(const uint32_t *table, int64_t i) {
  const uint4 *t = (const uint4 *)(table + i * kPileWidth);
  const uint4 x = t[0], y = t[1];
  Site s;
  s.c[0] = x.x, s.c[1] = x.y, s.c[2] = x.z, s.c[3] = x.w, s.c[4] = y.x, s.c[5] = y.y, s.c[6] = y.z, s.c[7] = y.w;
  s.depth = (u64)x.x + x.y + x.z + x.w + y.x + y.y;
  return s;
}

}  // namespace pilewalk
}  // namespace pbsim
