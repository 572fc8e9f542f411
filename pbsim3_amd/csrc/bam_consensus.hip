// bam_consensus.hip -- the kernels of pbsim_bam_consensus: the sequence the pile of reads spells, written as FASTA on the device.
// The record pass and the segments are bam_errors.hip's, the site pass is bam_pileup.hip's, the column pass is the pileup's with
// its log switched on (bam_pileup_walk.h).  The rule: include/pbsim3_amd.h.
//
//   columns : k_pile_columns<true>: as the pileup's, and every inserted base of an anchored I op (offset j < max_ins) leaves an
//             8-byte entry (position, j, class) in the file's log; a wave takes the slots of a round's 64 ops with one atomic on
//             the log's counter.  The order of the entries means nothing: all that follows are integer tallies.
//   slots   : after the site pass, one lane per position, a workgroup per tile: the ins_sites counted, and after the tiles'
//             exclusive scan their places written in ascending order: slot k is the k-th ins_site.
//   lengths : one lane per log entry: entries whose anchor is no ins_site are dropped by the class byte; the slot is found by a
//             binary search among the places; one 64-bit atomic max of j + 1 per entry (skipped where the slot holds as much).
//   tally   : after the lengths' exclusive scan, one lane per log entry again: one 32-bit atomic add into [off[k] + j][5].
//             The cells are as many as the longest insertions of the ins_sites together, never positions x max_ins.
//   bases   : one lane per position, workgroups striding over the tiles: 0 or 1 bases for the site and, at an ins_site, the
//             length of the insertion from a walk over its slot's cells; scanned across the workgroup.  The first pass leaves a
//             tile's bases, the emitted lengths, the counts (registers, one reduction per wave at the end, one global add per
//             workgroup and cell) and what lies in front of every record inside its first tile; after the tiles' scan the second
//             writes the headers, the bases at header + i + i / line_width, the line feeds and the last one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bam_consensus.h"
#include "bam_pileup_walk.h"

namespace pbsim {

namespace {

using namespace pilewalk;

constexpr int kLogBlocksMax = 4096;   // workgroups over a log: their lanes stride over the entries
constexpr int kBaseBlocksMax = 2048;  // workgroups of the base pass: they stride over the tiles
constexpr int kLogSizeBlocksMax = 1024;  // workgroups of the log-size pass: their lanes stride over the records
static_assert(kConsTile == kThreads, "a tile is one workgroup's positions");

__device__ __forceinline__ bool ins_site(uint32_t c) { return c != (uint32_t)kPileNoSite && (c & kPileInsBit) != 0; }

// the inserted bases of a file's scored records, from the record pass's CIGAR sums: as many entries as the log can get at most
__global__ __launch_bounds__(kThreads) void k_cons_log_size(ErrRecs a, u64 *out) {
  u64 sum = 0;
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < a.n_rec; r += (int64_t)gridDim.x * kThreads)
    if (a.st[r] & kEsScored) sum += (u64)a.sums[4 * r + 1];
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(out, sum);
}

template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_cons_slots(PileGenome g, const uint8_t *cls, const int64_t *tile_off, int64_t *tile_n, int64_t *pos) {
  __shared__ u64 sh_wave[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t i = (int64_t)blockIdx.x * kThreads + tid;
  const bool mine = i < g.total && ins_site(cls[i]);
  u64 all;
  const u64 before = block_scan(mine ? 1 : 0, sh_wave, wave, lane, &all);
  if (!kFill) {
    if (tid == 0) tile_n[blockIdx.x] = (int64_t)all;
  } else if (mine) {
    pos[tile_off[blockIdx.x] + (int64_t)before] = i;
  }
}

template <bool kTally>
__global__ __launch_bounds__(kThreads) void k_cons_log(const u64 *entry, int64_t n, int64_t total, const uint8_t *cls, ConsSlots slots) {
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
    const u64 v = entry[e];
    const int64_t at = (int64_t)(v >> kInsLogPosShift);
    const int64_t j = (int64_t)((v >> kInsLogOffShift) & 0xffffu);
    const uint32_t b = (uint32_t)(v & 7u);
    if (at >= total || b > 4 || !ins_site(cls[at])) continue;
    const int64_t k = slot_of(slots, at);
    if (k < 0) continue;  // (never: every ins_site has its slot)
    if (!kTally) {
      if (slots.len[k] < j + 1) atomicMax((u64 *)&slots.len[k], (u64)(j + 1));  // (the length only grows: a stale value costs an atomic)
    } else if (j < slots.len[k]) {  // (always)
      atomicAdd(&slots.cell[(slots.off[k] + j) * 5 + b], 1u);
    }
  }
}

__global__ void k_cons_record_bases(int32_t n, const int64_t *at, const int64_t *part, const int64_t *tile_off, int64_t tiles, int64_t *base_at) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += gridDim.x * blockDim.x)
    base_at[r] = r < n ? tile_off[at[r] / kConsTile] + part[r] : tile_off[tiles];
}

// base idx of a record whose bases begin at o: its byte, and the line feed behind it where it ends a line or the record
__device__ __forceinline__ void put_base(char *o, int64_t idx, int64_t n_bases, int64_t line_width, char ch) {
  const int64_t at = idx + (line_width ? idx / line_width : 0);
  o[at] = ch;
  if (idx == n_bases - 1 || (line_width && (idx + 1) % line_width == 0)) o[at + 1] = '\n';
}

template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_cons_bases(PileGenome g, const uint32_t *table, const uint8_t *cls, ConsSlots slots, uint32_t max_ins,
                                                         int fill, int64_t line_width, ConsRecords rec, const int64_t *tile_off, int64_t *tile_n,
                                                         char *text, u64 *cells) {
  __shared__ u64 sh_wave[kWaves];
  __shared__ u64 sh[kWaves][kConsCells];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (!kFill) {
    for (int i = tid; i < kWaves * kConsCells; i += kThreads) (&sh[0][0])[i] = 0;
    __syncthreads();
  }
  u64 *cell = sh[wave];
  u64 n_base[kConsBases] = {0, 0, 0, 0, 0, 0}, n_ins_sites = 0, n_capped = 0, longest = 0;
  const int64_t tiles = (g.total + kConsTile - 1) / kConsTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kThreads + tid;
    const uint32_t c = i < g.total ? cls[i] : (uint32_t)kPileNoSite;
    const uint32_t kind = c & 7u, call = (c >> 4) & 7u;
    const bool site = c != (uint32_t)kPileNoSite, filled = site && (kind == kPileRefN || kind == kPileLow);
    const bool own = site && (filled || call < 4);  // the site's own base is there
    int64_t k = -1;
    u64 l_ins = 0;
    if (ins_site(c)) k = slot_of(slots, i);
    if (k >= 0) {  // (every ins_site)
      if (!kFill) {
        const u64 depth = load_site(table, i).depth, logged = min((u64)slots.len[k], (u64)max_ins);
        const uint32_t *q = slots.cell + slots.off[k] * 5;
        while (l_ins < logged && 2 * ((u64)q[0] + q[1] + q[2] + q[3] + q[4]) > depth) l_ins++, q += 5;
        slots.len[k] = (int64_t)l_ins;  // from here on the length that is emitted
        n_ins_sites++;
        n_base[kCbIns] += l_ins;
        n_capped += l_ins == max_ins;
        longest = l_ins > longest ? l_ins : longest;
        atomicAdd(&cell[kConsCellInsLen + (int)min(l_ins, (u64)kConsLenBins - 1)], 1ull);
      } else {
        l_ins = (u64)slots.len[k];
      }
    }
    const u64 emits = (own ? 1 : 0) + l_ins;
    u64 all;
    const u64 before = block_scan(emits, sh_wave, wave, lane, &all);
    if (!kFill) {
      if (site) {
        n_base[kCbOut] += emits;
        if (filled) n_base[kCbFill]++;
        else if (call >= 4) n_base[kCbDel]++;
        else if (kind == kPileMatch) n_base[kCbKept]++;
        else n_base[kCbSub]++;
      }
      if (tid == 0) tile_n[tile] = (int64_t)all;
      if (i < g.total && (i & 63) == 0) {  // (a record begins at a multiple of 64)
        const int r = record_of(g, i);
        if (g.at[r] == i) rec.part[r] = (int64_t)before;
      }
    } else if (i < g.total) {
      const int r = record_of(g, i);
      const int64_t name_n = g.name_at[r + 1] - g.name_at[r];
      char *o = text + rec.byte_at[r];
      if (g.at[r] == i) {  // the record's first position, or with no bases its padding: the header line
        const char *name = g.names + g.name_at[r];
        o[0] = '>';
        for (int64_t x = 0; x < name_n; x++) o[1 + x] = name[x];
        o[1 + name_n] = '\n';
      }
      if (emits) {
        o += name_n + 2;
        const int64_t n_bases = rec.base_at[r + 1] - rec.base_at[r];
        int64_t idx = tile_off[tile] + (int64_t)before - rec.base_at[r];
        if (own) put_base(o, idx++, n_bases, line_width, filled ? (fill ? (char)g.seq[i] : 'N') : "ACGT"[call]);
        const uint32_t *q = k >= 0 ? slots.cell + slots.off[k] * 5 : nullptr;
        for (u64 j = 0; j < l_ins; j++, q += 5) put_base(o, idx++, n_bases, line_width, ins_base(q));
      }
    }
  }
  if (kFill) return;
#pragma unroll
  for (int x = 0; x < kConsBases; x++) {
    const u64 v = wave_sum(n_base[x]);
    if (lane == 0) cell[kConsCellBases + x] = v;
  }
  n_ins_sites = wave_sum(n_ins_sites), n_capped = wave_sum(n_capped), longest = wave_max(longest);
  if (lane == 0) cell[kConsCellInsSites] = n_ins_sites, cell[kConsCellCapped] = n_capped, cell[kConsCellLongest] = longest;
  __syncthreads();
  for (int i = tid; i < kConsCells; i += kThreads) {
    if (i == kConsCellLongest) {
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

inline int64_t tiles_of(const PileGenome &g) { return (g.total + kConsTile - 1) / kConsTile; }

}  // namespace

void launch_consensus_log_size(ErrRecs r, unsigned long long *out, hipStream_t s) {
  if (r.n_rec <= 0) return;
  const int64_t blocks = std::min<int64_t>((r.n_rec + kThreads - 1) / kThreads, kLogSizeBlocksMax);
  hipLaunchKernelGGL(k_cons_log_size, dim3((unsigned)blocks), dim3(kThreads), 0, s, r, out);
}

void launch_consensus_columns(ErrRecs r, ErrRefs refs, ErrGenome g, const ErrSegment *seg, int64_t n_seg, uint32_t min_baseq, uint32_t *table,
                              unsigned long long *cells, ConsLog log, uint32_t max_ins, hipStream_t s) {
  if (n_seg <= 0) return;
  const InsLog to = {log.entry, log.count, (u64)log.cap, max_ins};
  hipLaunchKernelGGL(k_pile_columns<true>, dim3((unsigned)column_blocks(n_seg, kWaves, kSegBlocksMax)), dim3(kThreads), 0, s, r, refs, g.seq, seg, n_seg,
                     min_baseq, table, cells, to);
}

void launch_consensus_slot_sizes(PileGenome g, const uint8_t *cls, int64_t *tile_n, hipStream_t s) {
  if (g.total <= 0) return;
  hipLaunchKernelGGL(k_cons_slots<false>, dim3((unsigned)tiles_of(g)), dim3(kThreads), 0, s, g, cls, (const int64_t *)nullptr, tile_n, (int64_t *)nullptr);
}

void launch_consensus_slot_fill(PileGenome g, const uint8_t *cls, const int64_t *tile_off, int64_t *pos, hipStream_t s) {
  if (g.total <= 0) return;
  hipLaunchKernelGGL(k_cons_slots<true>, dim3((unsigned)tiles_of(g)), dim3(kThreads), 0, s, g, cls, tile_off, (int64_t *)nullptr, pos);
}

void launch_consensus_lengths(ConsLog log, int64_t n, int64_t total, const uint8_t *cls, ConsSlots slots, hipStream_t s) {
  if (n <= 0 || slots.n <= 0) return;
  const int64_t blocks = std::min<int64_t>((n + kThreads - 1) / kThreads, kLogBlocksMax);
  hipLaunchKernelGGL(k_cons_log<false>, dim3((unsigned)blocks), dim3(kThreads), 0, s, log.entry, n, total, cls, slots);
}

void launch_consensus_tally(ConsLog log, int64_t n, int64_t total, const uint8_t *cls, ConsSlots slots, hipStream_t s) {
  if (n <= 0 || slots.n <= 0) return;
  const int64_t blocks = std::min<int64_t>((n + kThreads - 1) / kThreads, kLogBlocksMax);
  hipLaunchKernelGGL(k_cons_log<true>, dim3((unsigned)blocks), dim3(kThreads), 0, s, log.entry, n, total, cls, slots);
}

void launch_consensus_base_sizes(PileGenome g, const uint32_t *table, const uint8_t *cls, ConsSlots slots, uint32_t max_ins, ConsRecords rec,
                                 int64_t *tile_n, unsigned long long *cells, hipStream_t s) {
  if (g.total <= 0) return;
  const int64_t blocks = std::min<int64_t>(tiles_of(g), kBaseBlocksMax);
  hipLaunchKernelGGL(k_cons_bases<false>, dim3((unsigned)blocks), dim3(kThreads), 0, s, g, table, cls, slots, max_ins, 0, (int64_t)0, rec,
                     (const int64_t *)nullptr, tile_n, (char *)nullptr, cells);
}

void launch_consensus_record_bases(PileGenome g, const int64_t *part, const int64_t *tile_off, int64_t *base_at, hipStream_t s) {
  if (g.total <= 0) return;
  hipLaunchKernelGGL(k_cons_record_bases, dim3((unsigned)((g.n + 1 + 255) / 256)), dim3(256), 0, s, g.n, g.at, part, tile_off, tiles_of(g), base_at);
}

void launch_consensus_base_fill(PileGenome g, const uint8_t *cls, ConsSlots slots, int fill, int64_t line_width, ConsRecords rec,
                                const int64_t *tile_off, char *text, hipStream_t s) {
  if (g.total <= 0) return;
  const int64_t blocks = std::min<int64_t>(tiles_of(g), kBaseBlocksMax);
  hipLaunchKernelGGL(k_cons_bases<true>, dim3((unsigned)blocks), dim3(kThreads), 0, s, g, (const uint32_t *)nullptr, cls, slots, 0u, fill, line_width, rec,
                     tile_off, (int64_t *)nullptr, text, (unsigned long long *)nullptr);
}

}  // namespace pbsim
