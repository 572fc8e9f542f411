// bam_pileup_walk.h -- the column pass of pbsim_bam_pileup as a template, for bam_pileup.hip (kLog false: the pass as it always
// was, and the same machine code) and bam_consensus.hip (kLog true: besides, every inserted base of an anchored I op is appended
// to a log).  Device code: included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bam_fields.h"
#include "bam_pileup.h"

namespace pbsim {
namespace pilewalk {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

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

// what one op advances: the columns of the alignment (M = X I D), the reference (M = X D N), the query (M = X I S)
__device__ __forceinline__ void advances(uint32_t v, u64 *col, u64 *ref, u64 *query) {
  const uint32_t op = v & 15u;
  const u64 n = v >> 4;
  const bool m = op == 0 || op == 7 || op == 8;
  *col = m || op == 1 || op == 2 ? n : 0;
  *ref = m || op == 2 || op == 3 ? n : 0;
  *query = m || op == 1 || op == 4 ? n : 0;
}

__device__ __forceinline__ uint32_t ref_class(uint32_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }
__device__ __forceinline__ uint32_t code_class(uint32_t nib) { return nib == 1 ? 0u : nib == 2 ? 1u : nib == 4 ? 2u : nib == 8 ? 3u : 4u; }

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
template <bool kLog>
struct LogOf {
  typedef NoLog type;
};
template <>
struct LogOf<true> {
  typedef InsLog type;
};
constexpr int kInsLogPosShift = 24, kInsLogOffShift = 8;

template <bool kLog>
__global__ __launch_bounds__(kThreads) void k_pile_columns(ErrRecs a, ErrRefs refs, const uint8_t *genome, int size_bits, const ErrSegment *seg,
                                                           int64_t n_seg, uint32_t min_baseq, uint32_t *table, u64 *cells,
                                                           typename LogOf<kLog>::type log) {
  __shared__ unsigned int sh_unanchored[kWaves];
  __shared__ u64 sh_col[kWaves][64], sh_ref[kWaves][64], sh_query[kWaves][64];  // where each op of the round begins
  __shared__ uint32_t sh_op[kWaves][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < kWaves) sh_unanchored[tid] = 0;
  __syncthreads();
  u64 *w_col = sh_col[wave], *w_ref = sh_ref[wave], *w_query = sh_query[wave];
  uint32_t *w_op = sh_op[wave];
  u64 *w_slot = nullptr;  // kLog: the slot of offset 0 of each op of the round
  if constexpr (kLog) {
    __shared__ u64 sh_slot[kWaves][64];
    w_slot = sh_slot[wave];
  }
  for (int64_t s = (int64_t)blockIdx.x * kWaves + wave; s < n_seg; s += (int64_t)gridDim.x * kWaves) {
    const ErrSegment sg = seg[s];
    const uint8_t *p = a.stream + (int64_t)(a.rec[sg.rec] >> size_bits);
    const u64 l_seq = ld32(p + kBamLSeq);
    const int32_t ref_id = (int32_t)ld32(p + kBamRefId);
    const u64 pos = (u64)(int64_t)(int32_t)ld32(p + kBamPos);  // (a scored record: pos >= 0)
    const uint8_t *bases = p + kBamFixed + p[kBamLReadName] + 4 * (int64_t)ld16(p + kBamNCigarOp);
    const uint8_t *qual = bases + (l_seq + 1) / 2;
    const bool has_qual = (a.st[sg.rec] & kEsQual) != 0;
    const uint8_t *ops = a.stream + a.cig_at[sg.rec];
    const int64_t op_end = min((int64_t)sg.op0 + kErrSegOps, (int64_t)a.n_ops[sg.rec]);
    const u64 l_ref = (u64)refs.l_ref[ref_id];
    const uint8_t *g_seq = genome + refs.at[ref_id];
    uint32_t *tab = table + refs.at[ref_id] * kPileWidth;  // positions [0, l_ref) of this reference: the record pass held pos + span to it
    const u64 col_lo = (u64)sg.col0, col_hi = col_lo + kErrSegCols;
    u64 run_col = 0, run_ref = (u64)sg.ref_pos, run_query = (u64)sg.query_pos;
    for (int64_t k0 = sg.op0; k0 < op_end && run_col < col_hi; k0 += 64) {
      const uint32_t v = k0 + lane < op_end ? ld32(ops + 4 * (k0 + lane)) : 0u;
      u64 col, ref, query;
      advances(v, &col, &ref, &query);
      const u64 in_col = wave_scan(col, lane), in_ref = wave_scan(ref, lane), in_query = wave_scan(query, lane);
      const u64 my_col = run_col + in_col - col, my_ref = run_ref + in_ref - ref;
      u64 my_slot = 0;
      if constexpr (kLog) {
        // the entries this op leaves: its offsets inside the segment, below max_ins, where it is an anchored I op
        u64 j_lo = 0, n_mine = 0;
        if (col != 0 && (v & 15u) == 1 && my_ref > pos && my_ref - 1 < l_ref && my_col < col_hi && my_col + col > col_lo) {
          j_lo = my_col < col_lo ? col_lo - my_col : 0;
          const u64 j_hi = min(min(my_col + col, col_hi) - my_col, (u64)log.max_ins);
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
      __builtin_amdgcn_wave_barrier();  // (the lanes' searches of the round before are over)
      w_col[lane] = my_col, w_ref[lane] = my_ref, w_query[lane] = run_query + in_query - query;
      w_op[lane] = v;
      if constexpr (kLog) w_slot[lane] = my_slot;
      __builtin_amdgcn_wave_barrier();
      const u64 round_cols = __shfl(in_col, 63, 64);
      // an I op adds where its first column lies: to the position in front of it, or, with none consumed yet, to the call's cell
      if (col != 0 && (v & 15u) == 1 && my_col >= col_lo && my_col < col_hi) {
        if (my_ref > pos) {
          if (my_ref - 1 < l_ref) atomicAdd(&tab[(my_ref - 1) * kPileWidth + kPcIns], 1u);  // (always: pos + span <= l_ref)
        } else {
          atomicAdd(&sh_unanchored[wave], 1u);
        }
      }
      const u64 lo = max(col_lo, run_col), hi = min(col_hi, run_col + round_cols);
      for (u64 x0 = lo; x0 < hi; x0 += 64) {
        const u64 x = x0 + lane;
        if (x >= hi) continue;
        int i = 0;  // the last op of the round that begins at or before x: the one that holds it
        for (int d = 32; d >= 1; d >>= 1)
          if (w_col[i + d] <= x) i += d;
        const uint32_t op = w_op[i] & 15u;
        if (op == 1) {
          if constexpr (kLog) {
            // an inserted base: offset j of its op, which is anchored where some of the reference lies in front of it
            const u64 j = x - w_col[i], anchor = w_ref[i], qp = w_query[i] + j, slot = w_slot[i] + j;
            if (anchor > pos && anchor - 1 < l_ref && j < log.max_ins && slot < log.cap) {
              u64 entry = ~(u64)0;  // (never: the query length is l_seq; an entry no later pass takes)
              if (qp < l_seq) {
                const uint32_t nib = (bases[qp >> 1] >> (qp & 1 ? 0 : 4)) & 15u;
                entry = ((u64)(refs.at[ref_id] + (int64_t)anchor - 1) << kInsLogPosShift) | (j << kInsLogOffShift) | code_class(nib);
              }
              log.entry[slot] = entry;
            }
          }
          continue;
        }
        const u64 off = x - w_col[i], rp = w_ref[i] + off, qp = w_query[i] + off;
        if (rp >= l_ref) continue;  // (never: pos + span <= l_ref)
        uint32_t cell = kPcDel;
        if (op != 2) {
          if (qp >= l_seq) continue;  // (never: the query length is l_seq)
          const uint32_t nib = (bases[qp >> 1] >> (qp & 1 ? 0 : 4)) & 15u;
          cell = nib == 0 ? ref_class(g_seq[rp]) : code_class(nib);
          if (has_qual && (uint32_t)qual[qp] < min_baseq) cell = kPcMasked;
        }
        atomicAdd(&tab[rp * kPileWidth + cell], 1u);
      }
      run_col += round_cols, run_ref += __shfl(in_ref, 63, 64), run_query += __shfl(in_query, 63, 64);
    }
  }
  __syncthreads();
  if (tid == 0) {
    u64 sum = 0;
    for (int w = 0; w < kWaves; w++) sum += sh_unanchored[w];
    if (sum) atomicAdd(&cells[kPileCellUnanchored], sum);
  }
}

// the workgroups of the column pass over n_seg segments: its waves stride over them
inline int64_t column_blocks(int64_t n_seg) {
  constexpr int kSegBlocksMax = 2048;
  // a wave's cell is 32 bits wide: its segments hold fewer than 2^32 I ops as long as it takes fewer than 2^20 of them
  const int64_t least = (n_seg + ((int64_t)kWaves << 19) - 1) / ((int64_t)kWaves << 19);
  return std::max<int64_t>(std::min<int64_t>((n_seg + kWaves - 1) / kWaves, kSegBlocksMax), least);
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
