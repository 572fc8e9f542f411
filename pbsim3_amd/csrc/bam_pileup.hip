// bam_pileup.hip -- the kernels of pbsim_bam_pileup: what the aligned reads of a BAM say at every position of the genome that lies
// prepared in HBM beside them.  The record pass and the segments are bam_errors.hip's (launch_errors_records).  The rule:
// include/pbsim3_amd.h.
//
//   columns : one wave per segment, the waves striding over the segments, walking a segment as k_err_columns does: a round loads 64
//             ops of the block, forms the wave's prefix sums of their column, reference and query advances and leaves them in the
//             wave's part of LDS; then the round's columns inside the segment are taken 64 at a time, each lane finding its op by
//             a binary search among the 64 prefix values.  Every M = X or D column issues one atomic add on a 32-bit cell of the
//             table in global memory, laid out [position][8]: a wave's 64 consecutive columns fall into one span of 2 KB.  An I op
//             adds to the ins cell of the position before it, by the lane that holds the op, in the segment that holds its first
//             column; where nothing of the reference is consumed yet it counts in the wave's LDS cell, flushed once per workgroup.
//   sites   : one lane per position (the workgroups striding over the table): the eight cells with two 16-byte loads, depth, the
//             call and the class, one class byte written; the totals are kept in registers and reduced once per wave at the end,
//             the homopolymer classes in cells in LDS private to the wave; one global add per workgroup and cell.
//   text    : one lane per position, a workgroup per tile of kPileTile positions: the line's length, scanned across the workgroup;
//             the first pass leaves the tile's bytes, and after their exclusive scan the second writes the lines.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bam_fields.h"
#include "bam_pileup.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSegBlocksMax = 2048;   // workgroups of the column pass: its waves stride over the segments
constexpr int kSiteBlocksMax = 2048;  // workgroups of the site pass
static_assert(kPileTile == kThreads, "a tile of the text is one workgroup's positions");

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

__global__ __launch_bounds__(kThreads) void k_pile_columns(ErrRecs a, ErrRefs refs, const uint8_t *genome, int size_bits, const ErrSegment *seg,
                                                           int64_t n_seg, uint32_t min_baseq, uint32_t *table, u64 *cells) {
  __shared__ unsigned int sh_unanchored[kWaves];
  __shared__ u64 sh_col[kWaves][64], sh_ref[kWaves][64], sh_query[kWaves][64];  // where each op of the round begins
  __shared__ uint32_t sh_op[kWaves][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid < kWaves) sh_unanchored[tid] = 0;
  __syncthreads();
  u64 *w_col = sh_col[wave], *w_ref = sh_ref[wave], *w_query = sh_query[wave];
  uint32_t *w_op = sh_op[wave];
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
      __builtin_amdgcn_wave_barrier();  // (the lanes' searches of the round before are over)
      w_col[lane] = my_col, w_ref[lane] = my_ref, w_query[lane] = run_query + in_query - query;
      w_op[lane] = v;
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
        if (op == 1) continue;
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

__global__ __launch_bounds__(kThreads) void k_pile_sites(PileGenome g, const uint32_t *table, u64 min_depth, uint8_t *cls, u64 *cells) {
  __shared__ u64 sh[kWaves][kPileCells];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < kWaves * kPileCells; i += kThreads) (&sh[0][0])[i] = 0;
  __syncthreads();
  u64 *cell = sh[wave];
  const int64_t total = g.total;
  u64 n_site[kPileSites] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, sums[kPileWidth] = {0, 0, 0, 0, 0, 0, 0, 0}, deepest = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + tid; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int r = record_of(g, i);
    if (i - g.at[r] >= g.len[r]) {
      cls[i] = (uint8_t)kPileNoSite;
      continue;
    }
    const Site s = load_site(table, i);
#pragma unroll
    for (int k = 0; k < kPileWidth; k++) sums[k] += s.c[k];
    deepest = s.depth > deepest ? s.depth : deepest;
    const uint32_t rc = ref_class(g.seq[i]), hv = min((uint32_t)g.hp[i], (uint32_t)kPileHp - 1);
    n_site[kPsSites]++;
    uint32_t out;
    if (rc == 4) {
      n_site[kPsRefN]++;
      out = kPileRefN | (kPileNoCall << 4);
    } else if (s.depth < min_depth) {
      n_site[kPsLow]++;
      out = kPileLow | (kPileNoCall << 4);
    } else {
      // the largest of A C G T del; among equals the genome's own, else the first
      const uint32_t cand[5] = {s.c[0], s.c[1], s.c[2], s.c[3], s.c[kPcDel]};
      uint32_t best = cand[0], call = 0;
#pragma unroll
      for (uint32_t k = 1; k < 5; k++)
        if (cand[k] > best) best = cand[k], call = k;
      const uint32_t own = rc == 0 ? cand[0] : rc == 1 ? cand[1] : rc == 2 ? cand[2] : cand[3];
      if (own == best) call = rc;
      const bool ins = 2 * (u64)s.c[kPcIns] > s.depth;
      const uint32_t kind = call == rc ? kPileMatch : call == 4 ? kPileDel : kPileSub;
      n_site[kPsCalled]++;
      atomicAdd(&cell[kPileCellHpCalled + hv], 1ull);
      if (kind == kPileMatch) n_site[kPsConcordant]++;
      if (kind == kPileSub) n_site[kPsSub]++, atomicAdd(&cell[kPileCellHpSub + hv], 1ull);
      if (kind == kPileDel) n_site[kPsDel]++, atomicAdd(&cell[kPileCellHpDel + hv], 1ull);
      if (ins) n_site[kPsIns]++, atomicAdd(&cell[kPileCellHpIns + hv], 1ull);
      if (ins || kind != kPileMatch) n_site[kPsDiscordant]++;
      out = kind | (ins ? kPileInsBit : 0) | (call << 4);
    }
    cls[i] = (uint8_t)out;
  }
#pragma unroll
  for (int k = 0; k < kPileSites; k++) {
    const u64 v = wave_sum(n_site[k]);
    if (lane == 0) cell[kPileCellSites + k] = v;
  }
#pragma unroll
  for (int k = 0; k < kPileWidth; k++) {
    const u64 v = wave_sum(sums[k]);
    if (lane == 0) cell[kPileCellSums + k] = v;
  }
  deepest = wave_max(deepest);
  if (lane == 0) cell[kPileCellMaxDepth] = deepest;
  __syncthreads();
  for (int i = tid; i < kPileCells; i += kThreads) {
    if (i == kPileCellUnanchored) continue;  // (the column pass's)
    if (i == kPileCellMaxDepth) {
      u64 m = 0;
      for (int w = 0; w < kWaves; w++) m = sh[w][i] > m ? sh[w][i] : m;
      if (m) atomicMax(&cells[i], m);
      continue;
    }
    u64 sum = 0;
    for (int w = 0; w < kWaves; w++) sum += sh[w][i];
    if (sum) atomicAdd(&cells[i], sum);
  }
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

__device__ __forceinline__ bool listed(uint32_t c, int format) {
  if (c == (uint32_t)kPileNoSite) return false;
  const uint32_t kind = c & 7u;
  return format == 1 || kind == kPileSub || kind == kPileDel || (c & kPileInsBit) != 0;
}

// the line of position i (a site that is listed): its length, and with o the bytes
__device__ __forceinline__ u64 site_line(const PileGenome &g, const uint32_t *table, int64_t i, uint32_t c, char *o) {
  const int r = record_of(g, i);
  const Site s = load_site(table, i);
  const int64_t name_n = g.name_at[r + 1] - g.name_at[r];
  const u64 pos1 = (u64)(i - g.at[r]) + 1;
  const uint32_t kind = c & 7u, call = (c >> 4) & 7u;
  const bool ins = (c & kPileInsBit) != 0;
  if (!o) {
    u64 l = (u64)name_n + 13 + 1 + digits(pos1) + 1 + digits(s.depth) + 1;  // the tabs, the line feed, pos1, ref, depth, call
    for (int k = 0; k < kPileWidth; k++) l += digits(s.c[k]);
    return l + (kind == kPileRefN || kind == kPileMatch ? 5 : 3) + (ins ? 4 : 0);
  }
  const char *name = g.names + g.name_at[r];
  for (int64_t k = 0; k < name_n; k++) *o++ = name[k];
  *o++ = '\t';
  o = put(o, pos1);
  *o++ = '\t';
  *o++ = (char)g.seq[i];
  *o++ = '\t';
  o = put(o, s.depth);
  for (int k = 0; k < kPileWidth; k++) {
    *o++ = '\t';
    o = put(o, (u64)s.c[k]);
  }
  *o++ = '\t';
  *o++ = call == (uint32_t)kPileNoCall ? '.' : call == 4 ? '*' : "ACGT"[call];
  *o++ = '\t';
  o = put(o, kind == kPileRefN ? "ref_n" : kind == kPileLow ? "low" : kind == kPileMatch ? "match" : kind == kPileSub ? "sub" : "del");
  if (ins) o = put(o, "+ins");
  *o = '\n';
  return 0;
}

template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_pile_text(PileGenome g, const uint32_t *table, const uint8_t *cls, int format, const int64_t *tile_off,
                                                        int64_t *tile_len, char *text) {
  __shared__ u64 sh_wave[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t i = (int64_t)blockIdx.x * kThreads + tid;
  const uint32_t c = i < g.total ? cls[i] : (uint32_t)kPileNoSite;
  const bool mine = listed(c, format);
  const u64 l = mine ? site_line(g, table, i, c, nullptr) : 0;
  const u64 incl = wave_scan(l, lane);
  if (lane == 63) sh_wave[wave] = incl;
  __syncthreads();
  u64 before = 0, all = 0;
  for (int w = 0; w < kWaves; w++) {
    if (w < wave) before += sh_wave[w];
    all += sh_wave[w];
  }
  if (!kFill) {
    if (tid == 0) tile_len[blockIdx.x] = (int64_t)all;
  } else if (mine) {
    site_line(g, table, i, c, text + tile_off[blockIdx.x] + (int64_t)(before + incl - l));
  }
}

inline int64_t tiles_of(const PileGenome &g) { return (g.total + kPileTile - 1) / kPileTile; }

}  // namespace

void launch_pileup_columns(ErrRecs r, ErrRefs refs, ErrGenome g, const ErrSegment *seg, int64_t n_seg, uint32_t min_baseq, uint32_t *table,
                           unsigned long long *cells, hipStream_t s) {
  if (n_seg <= 0) return;
  // a wave's cell is 32 bits wide: its segments hold fewer than 2^32 I ops as long as it takes fewer than 2^20 of them
  const int64_t least = (n_seg + ((int64_t)kWaves << 19) - 1) / ((int64_t)kWaves << 19);
  const int64_t blocks = std::max<int64_t>(std::min<int64_t>((n_seg + kWaves - 1) / kWaves, kSegBlocksMax), least);
  hipLaunchKernelGGL(k_pile_columns, dim3((unsigned)blocks), dim3(kThreads), 0, s, r, refs, g.seq, kBamSamplePacking.size_bits, seg, n_seg, min_baseq,
                     table, cells);
}

void launch_pileup_sites(PileGenome g, const uint32_t *table, int64_t min_depth, uint8_t *cls, unsigned long long *cells, hipStream_t s) {
  if (g.total <= 0) return;
  const int64_t blocks = std::min<int64_t>(tiles_of(g), kSiteBlocksMax);
  hipLaunchKernelGGL(k_pile_sites, dim3((unsigned)blocks), dim3(kThreads), 0, s, g, table, (u64)min_depth, cls, cells);
}

void launch_pileup_text_sizes(PileGenome g, const uint32_t *table, const uint8_t *cls, int format, int64_t *tile_len, hipStream_t s) {
  if (g.total <= 0) return;
  hipLaunchKernelGGL(k_pile_text<false>, dim3((unsigned)tiles_of(g)), dim3(kThreads), 0, s, g, table, cls, format, (const int64_t *)nullptr, tile_len,
                     (char *)nullptr);
}

void launch_pileup_text_fill(PileGenome g, const uint32_t *table, const uint8_t *cls, int format, const int64_t *tile_off, char *text,
                             hipStream_t s) {
  if (g.total <= 0) return;
  hipLaunchKernelGGL(k_pile_text<true>, dim3((unsigned)tiles_of(g)), dim3(kThreads), 0, s, g, table, cls, format, tile_off, (int64_t *)nullptr, text);
}

}  // namespace pbsim
