// bam_pileup.hip -- the kernels of pbsim_bam_pileup: what the aligned reads of a BAM say at every position of the genome that lies
// prepared in HBM beside them.  The record pass and the segments are bam_errors.hip's (launch_errors_records).  The rule:
// include/pbsim3_amd.h.
//
//   columns : (k_pile_columns<false> of bam_pileup_walk.h, which pbsim_bam_consensus runs with its log switched on)
//             one wave per segment, the waves striding over the segments, walking a segment with bam_cigar.h's walk_columns as
//             k_err_columns does.  Every M = X or D column issues one atomic add on a 32-bit cell of the
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

#include "bam_pileup.h"
#include "bam_pileup_walk.h"

namespace pbsim {

namespace {

using namespace pilewalk;  // the column pass and a site's cells (bam_pileup_walk.h)

constexpr int kSiteBlocksMax = 2048;  // workgroups of the site pass
static_assert(kPileTile == kThreads, "a tile of the text is one workgroup's positions");

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
  hipLaunchKernelGGL(k_pile_columns<false>, dim3((unsigned)column_blocks(n_seg, kWaves, kSegBlocksMax)), dim3(kThreads), 0, s, r, refs, g.seq, seg, n_seg,
                     min_baseq, table, cells, NoLog());
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
