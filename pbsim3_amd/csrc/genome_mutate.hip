// genome_mutate.hip -- the kernels of pbsim_genome_mutate: SNVs, insertions and deletions drawn per position of a genome with the
// keyed Philox stream, the variant genome written as FASTA and the variants as VCF lines on the device.  The rule:
// include/pbsim3_amd.h.  The genome lies in HBM as the BAM stages hold it (bam_genome.h): every record at a multiple of 64, 64 zero
// bytes behind it.  A tile is kMutTile positions of that buffer, one workgroup's; workgroups stride over the tiles.
//
//   events : one lane per position, one Philox block: the kind.  Only a lane with an indel loops over the length draws, and a del
//            lane walks its run for the cut.  It leaves the kind byte, the length and, for a del, the buffer index behind its run
//            (else 0), and per tile the largest of those ends.
//   scan   : the deleted set is an inclusive max-scan of the ends: position i is deleted where an end in front of it lies above
//            i.  Runs never leave their record, so one scan over the whole buffer serves.  One workgroup scans the tiles' largest
//            ends (exclusive, in place); the scan inside a tile is made where it is needed, by the base pass.  No atomics.
//   bases  : the first pass finishes the scan, sets kMutDeleted in the kind bytes, and sums what every position emits (0, 1, or
//            1 + the insertion) across the workgroup: a tile's bases, what lies in front of every record inside its first tile,
//            the counts.  After the tiles' scan the second writes the headers, the bases at header + i + i / line_width with the
//            line feeds, and the origin map; an insertion is written by its one lane, across line breaks and tile edges.
//   lines  : an anchor that carries an event writes a line; the lane of a del walks the deleted run behind it (kind bytes only).
//            Sizes, the tiles' scan, then the fill, as bam_call.hip's line pass.
//
// The counts are kept in registers, reduced once per wave at the end and added with one atomic per workgroup and cell: integer
// sums and maxima, so their order means nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bam_pileup_walk.h"
#include "genome_mutate.h"
#include "philox.h"

namespace pbsim {

namespace {

using namespace pilewalk;

constexpr int kEventBlocksMax = 2048;  // workgroups of the event pass: they stride over the tiles
constexpr int kBaseBlocksMax = 2048;   // of the base pass
constexpr int kLineBlocksMax = 2048;   // of the line pass
constexpr int kScanPerLane = 4;        // the tiles one lane of the scan's one workgroup takes per trip
static_assert(kMutTile == kThreads, "a tile is one workgroup's positions");

enum : uint32_t { kNone = 0, kSnv, kIns, kDel };

// D(r, p, sub, 4 * block + k), k = 0 .. 3
__device__ __forceinline__ U4 mut_block(uint32_t seed, uint32_t r, uint32_t p, uint32_t sub, uint32_t block) {
  U4 v = philox4x32_10(block, sub, p, r, seed, kStreamMutate);
  v.x >>= 1, v.y >>= 1, v.z >>= 1, v.w >>= 1;
  return v;
}
__device__ __forceinline__ uint32_t word_of(const U4 &v, uint32_t k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

__device__ __forceinline__ u64 wave_scan_max(u64 x, int lane) {  // inclusive
  for (int d = 1; d < 64; d <<= 1) {
    const u64 y = __shfl_up(x, d, 64);
    if (lane >= d && y > x) x = y;
  }
  return x;
}

// block_scan (device_util.h) with the maximum: the largest v of the lanes in front (0: none), *all the workgroup's largest
template <int kWaves>
__device__ __forceinline__ u64 block_scan_max(u64 v, u64 (&sh_wave)[kWaves], int wave, int lane, u64 *all) {
  const u64 incl = wave_scan_max(v, lane);
  u64 prev = __shfl_up(incl, 1, 64);
  if (lane == 0) prev = 0;
  __syncthreads();
  if (lane == 63) sh_wave[wave] = incl;
  __syncthreads();
  u64 before = 0, most = 0;
  for (int w = 0; w < kWaves; w++) {
    if (w < wave && sh_wave[w] > before) before = sh_wave[w];
    if (sh_wave[w] > most) most = sh_wave[w];
  }
  *all = most;
  return before > prev ? before : prev;
}

__device__ __forceinline__ bool longest_cell(int x) { return x == kMutCellLongestRef || x == kMutCellLongestAlt; }

// a workgroup's counts into the cells: one reduction per wave, one global atomic per cell that is not 0
__device__ __forceinline__ void add_cells(const u64 *n_cell, u64 (*sh)[kMutCells], u64 *cells, int tid, int wave, int lane) {
#pragma unroll
  for (int x = 0; x < kMutCells; x++) {
    const u64 v = longest_cell(x) ? wave_max(n_cell[x]) : wave_sum(n_cell[x]);
    if (lane == 0) sh[wave][x] = v;
  }
  __syncthreads();
  for (int x = tid; x < kMutCells; x += kThreads) {
    u64 v = 0;
    for (int w = 0; w < kWaves; w++) v = longest_cell(x) ? (sh[w][x] > v ? sh[w][x] : v) : v + sh[w][x];
    if (!v) continue;
    if (longest_cell(x)) atomicMax(&cells[x], v);
    else atomicAdd(&cells[x], v);
  }
}

__global__ __launch_bounds__(kThreads) void k_mut_events(PileGenome g, pbsim_mutate_opts o, MutSites s, u64 *cells) {
  __shared__ u64 sh_wave[kWaves];
  __shared__ u64 sh[kWaves][kMutCells];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  u64 n_cell[kMutCells];
#pragma unroll
  for (int x = 0; x < kMutCells; x++) n_cell[x] = 0;
  const uint32_t snv = (uint32_t)o.snv_ppm, ins = snv + (uint32_t)o.ins_ppm, del = ins + (uint32_t)o.del_ppm;
  const uint32_t ext = (uint32_t)o.ext_ppm, max_indel = (uint32_t)o.max_indel;
  const int64_t tiles = (g.total + kMutTile - 1) / kMutTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kThreads + tid;
    uint32_t kind = kMutNoSite, len = 0;
    u64 end = 0;
    if (i < g.total) {
      const int r = record_of(g, i);
      const int64_t p = i - g.at[r], n = g.len[r];
      if (p < n) {
        kind = kNone;
        if (ref_class(g.seq[i]) < 4) {
          n_cell[kMutCellEligible]++;
          const uint32_t e = mut_block(o.seed, (uint32_t)r, (uint32_t)p, 0, 0).x % 1000000u;
          kind = e < snv ? kSnv : e < ins ? kIns : e < del ? kDel : kNone;
          if (kind >= kIns) {
            len = 1;
            for (uint32_t block = 0; len < max_indel; block++) {
              const U4 d = mut_block(o.seed, (uint32_t)r, (uint32_t)p, 1, block);
              uint32_t k = 0;
              while (k < 4 && len < max_indel && word_of(d, k) % 1000000u < ext) k++, len++;
              if (k < 4) break;
            }
          }
          if (kind == kDel) {  // the cut: the record's end, the first byte that is not A C G T
            const int64_t most = (int64_t)len < n - 1 - p ? (int64_t)len : n - 1 - p;
            int64_t run = 0;
            while (run < most && ref_class(g.seq[i + run + 1]) < 4) run++;
            len = (uint32_t)run;
            if (run == 0) kind = kNone, n_cell[kMutCellVoidDel]++;
            else end = (u64)(i + run + 1);
          }
          n_cell[kMutCellDrawn + kMtSnv] += kind == kSnv, n_cell[kMutCellDrawn + kMtIns] += kind == kIns, n_cell[kMutCellDrawn + kMtDel] += kind == kDel;
        }
      }
      s.kind[i] = (uint8_t)kind, s.len[i] = (uint16_t)(kind >= kIns ? len : 0), s.end[i] = end;
    }
    const u64 most = wave_max(end);
    if (lane == 0) sh_wave[wave] = most;
    __syncthreads();
    if (tid == 0) {
      u64 m = 0;
      for (int w = 0; w < kWaves; w++) m = sh_wave[w] > m ? sh_wave[w] : m;
      s.tile[tile] = m;
    }
    __syncthreads();
  }
  add_cells(n_cell, sh, cells, tid, wave, lane);
}

// one workgroup: tile[t] becomes the largest of tile[0 .. t - 1], kThreads * kScanPerLane tiles per trip
__global__ __launch_bounds__(kThreads) void k_mut_tile_scan(u64 *tile, int64_t tiles) {
  __shared__ u64 sh_wave[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  u64 carry = 0;
  for (int64_t base = 0; base < tiles; base += (int64_t)kThreads * kScanPerLane) {
    const int64_t at = base + (int64_t)tid * kScanPerLane;
    u64 v[kScanPerLane], mine = 0;
#pragma unroll
    for (int k = 0; k < kScanPerLane; k++) {
      v[k] = at + k < tiles ? tile[at + k] : 0;
      mine = v[k] > mine ? v[k] : mine;
    }
    u64 all;
    const u64 before = block_scan_max(mine, sh_wave, wave, lane, &all);
    u64 run = before > carry ? before : carry;
#pragma unroll
    for (int k = 0; k < kScanPerLane; k++) {
      if (at + k < tiles) tile[at + k] = run;
      run = v[k] > run ? v[k] : run;
    }
    carry = all > carry ? all : carry;
  }
}

__global__ void k_mut_record_bases(int32_t n, const int64_t *at, const int64_t *part, const int64_t *tile_off, int64_t tiles, int64_t *base_at) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += gridDim.x * blockDim.x)
    base_at[r] = r < n ? tile_off[at[r] / kMutTile] + part[r] : tile_off[tiles];
}

// base idx of a record whose bases begin at o: its byte, and the line feed behind it where it ends a line or the record
__device__ __forceinline__ void put_base(char *o, int64_t idx, int64_t n_bases, int64_t line_width, char ch) {
  const int64_t at = idx + (line_width ? idx / line_width : 0);
  o[at] = ch;
  if (idx == n_bases - 1 || (line_width && (idx + 1) % line_width == 0)) o[at + 1] = '\n';
}

template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_mut_bases(PileGenome g, pbsim_mutate_opts o, MutSites s, int64_t *part, const int64_t *base_at,
                                                        const int64_t *byte_at, const int64_t *tile_off, int64_t *tile_n, char *text, int32_t *origin,
                                                        u64 *cells) {
  __shared__ u64 sh_wave[kWaves];
  __shared__ u64 sh[kWaves][kMutCells];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  u64 n_cell[kMutCells];
#pragma unroll
  for (int x = 0; x < kMutCells; x++) n_cell[x] = 0;
  const int64_t tiles = (g.total + kMutTile - 1) / kMutTile, line_width = o.line_width;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kThreads + tid;
    uint32_t c = i < g.total ? s.kind[i] : (uint32_t)kMutNoSite;
    const bool site = !(c & kMutNoSite);
    const uint32_t kind = c & kMutKindBits;
    u64 all;
    if (!kFill) {  // the scan's last level: an end in front of i that lies above i
      const u64 in_tile = block_scan_max(i < g.total ? s.end[i] : 0, sh_wave, wave, lane, &all), in_front = s.tile[tile];
      if (site && (in_tile > in_front ? in_tile : in_front) > (u64)i) {
        c |= kMutDeleted;
        s.kind[i] = (uint8_t)c;
        n_cell[kMutCellDeleted]++;
        n_cell[kMutCellDropped] += kind == kSnv || kind == kIns, n_cell[kMutCellMerged] += kind == kDel;
      }
    }
    const bool kept = site && !(c & kMutDeleted);
    const u64 l_ins = kept && kind == kIns ? s.len[i] : 0, emits = (kept ? 1 : 0) + l_ins;
    const u64 before = block_scan(emits, sh_wave, wave, lane, &all);
    if (!kFill) {
      n_cell[kMutCellBasesOut] += emits, n_cell[kMutCellInserted] += l_ins, n_cell[kMutCellSubstituted] += kept && kind == kSnv;
      if (tid == 0) tile_n[tile] = (int64_t)all;
      if (i < g.total && (i & 63) == 0) {  // (a record begins at a multiple of 64)
        const int r = record_of(g, i);
        if (g.at[r] == i) part[r] = (int64_t)before;
      }
    } else if (i < g.total && (emits || (i & 63) == 0)) {
      const int r = record_of(g, i);
      const int64_t name_n = g.name_at[r + 1] - g.name_at[r];
      char *t = text ? text + byte_at[r] : nullptr;
      if (t && g.at[r] == i) {  // the record's first position, or with no bases its padding: the header line
        const char *name = g.names + g.name_at[r];
        t[0] = '>';
        for (int64_t x = 0; x < name_n; x++) t[1 + x] = name[x];
        t[1 + name_n] = '\n';
      }
      if (emits) {
        if (t) t += name_n + 2;
        const uint32_t p = (uint32_t)(i - g.at[r]);
        const int64_t n_bases = base_at[r + 1] - base_at[r];
        int64_t idx = tile_off[tile] + (int64_t)before - base_at[r];
        int32_t *to = origin ? origin + base_at[r] : nullptr;
        char own = (char)g.seq[i];
        if (kind == kSnv) own = "ACGT"[(ref_class((uint32_t)own) + 1 + mut_block(o.seed, (uint32_t)r, p, 0, 0).y % 3u) & 3u];
        if (t) put_base(t, idx, n_bases, line_width, own);
        if (to) to[idx] = (int32_t)p;
        idx++;
        U4 d = {0, 0, 0, 0};
        for (uint32_t j = 0; j < (uint32_t)l_ins; j++, idx++) {
          if ((j & 3u) == 0) d = mut_block(o.seed, (uint32_t)r, p, 2, j >> 2);
          if (t) put_base(t, idx, n_bases, line_width, "ACGT"[word_of(d, j & 3u) & 3u]);
          if (to) to[idx] = -1 - (int32_t)p;
        }
      }
    }
  }
  if (!kFill) add_cells(n_cell, sh, cells, tid, wave, lane);
}

template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_mut_lines(PileGenome g, pbsim_mutate_opts o, MutSites s, const int64_t *tile_off, int64_t *tile_n,
                                                        char *text, u64 *cells, u64 *rec_n) {
  __shared__ u64 sh_wave[kWaves];
  __shared__ u64 sh[kWaves][kMutCells];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  u64 n_cell[kMutCells];
#pragma unroll
  for (int x = 0; x < kMutCells; x++) n_cell[x] = 0;
  const int64_t total = g.total, tiles = (total + kMutTile - 1) / kMutTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kThreads + tid;
    const uint32_t c = i < total ? s.kind[i] : (uint32_t)kMutNoSite, kind = c & kMutKindBits;
    const bool written = !(c & (kMutNoSite | kMutDeleted)) && kind != kNone;  // an anchor with its event: REF and ALT differ
    u64 l = 0, ref_len = 1, alt_len = 1;
    int r = 0;
    int64_t name_n = 0;
    if (written) {
      r = record_of(g, i);
      name_n = g.name_at[r + 1] - g.name_at[r];
      if (kind == kIns) alt_len += s.len[i];
      if (kind == kDel) {  // the deleted run behind the anchor: its own run and what merged runs add (the padding is not deleted)
        int64_t hi = i;
        while (hi + 1 < total && (s.kind[hi + 1] & kMutDeleted)) hi++;
        ref_len = (u64)(hi - i + 1);
      }
      // name, POS, ".", REF, ALT, ".", ".", TYPE= with their tabs, the type's three letters and the line feed
      l = (u64)name_n + 1 + digits((u64)(i - g.at[r]) + 1) + 3 + ref_len + 1 + alt_len + 10 + 3 + 1;
    }
    u64 all;
    const u64 before = block_scan(l, sh_wave, wave, lane, &all);
    if (!kFill) {
      if (tid == 0) tile_n[tile] = (int64_t)all;
      if (written) {
        n_cell[kMutCellVariants]++;
        n_cell[kMutCellTypes + kMtSnv] += kind == kSnv, n_cell[kMutCellTypes + kMtIns] += kind == kIns, n_cell[kMutCellTypes + kMtDel] += kind == kDel;
        n_cell[kMutCellRefBases] += ref_len, n_cell[kMutCellAltBases] += alt_len;
        n_cell[kMutCellLongestRef] = max(n_cell[kMutCellLongestRef], ref_len);
        n_cell[kMutCellLongestAlt] = max(n_cell[kMutCellLongestAlt], alt_len);
        atomicAdd(&rec_n[r], 1ull);
      }
    } else if (written) {
      char *t = text + tile_off[tile] + (int64_t)before;
      const char *name = g.names + g.name_at[r];
      const uint32_t p = (uint32_t)(i - g.at[r]);
      for (int64_t x = 0; x < name_n; x++) *t++ = name[x];
      *t++ = '\t';
      t = put(t, (u64)p + 1);
      t = put(t, "\t.\t");
      for (u64 x = 0; x < ref_len; x++) *t++ = (char)g.seq[i + (int64_t)x];
      *t++ = '\t';
      char own = (char)g.seq[i];
      if (kind == kSnv) own = "ACGT"[(ref_class((uint32_t)own) + 1 + mut_block(o.seed, (uint32_t)r, p, 0, 0).y % 3u) & 3u];
      *t++ = own;
      U4 d = {0, 0, 0, 0};
      for (uint32_t j = 0; j + 1 < (uint32_t)alt_len; j++) {
        if ((j & 3u) == 0) d = mut_block(o.seed, (uint32_t)r, p, 2, j >> 2);
        *t++ = "ACGT"[word_of(d, j & 3u) & 3u];
      }
      t = put(t, "\t.\t.\tTYPE=");
      t = put(t, kind == kSnv ? "snv" : kind == kIns ? "ins" : "del");
      *t = '\n';
    }
  }
  if (!kFill) add_cells(n_cell, sh, cells, tid, wave, lane);
}

inline int64_t tiles_of(const PileGenome &g) { return (g.total + kMutTile - 1) / kMutTile; }

}  // namespace

void launch_mutate_events(PileGenome g, pbsim_mutate_opts o, MutSites s, unsigned long long *cells, hipStream_t st) {
  if (g.total <= 0) return;
  const int64_t blocks = std::min<int64_t>(tiles_of(g), kEventBlocksMax);
  hipLaunchKernelGGL(k_mut_events, dim3((unsigned)blocks), dim3(kThreads), 0, st, g, o, s, cells);
}

void launch_mutate_tile_scan(MutSites s, int64_t tiles, hipStream_t st) {
  if (tiles <= 0) return;
  hipLaunchKernelGGL(k_mut_tile_scan, dim3(1), dim3(kThreads), 0, st, s.tile, tiles);
}

void launch_mutate_base_sizes(PileGenome g, MutSites s, int64_t *part, int64_t *tile_n, unsigned long long *cells, hipStream_t st) {
  if (g.total <= 0) return;
  const int64_t blocks = std::min<int64_t>(tiles_of(g), kBaseBlocksMax);
  const pbsim_mutate_opts none = {};
  hipLaunchKernelGGL(k_mut_bases<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, g, none, s, part, (const int64_t *)nullptr,
                     (const int64_t *)nullptr, (const int64_t *)nullptr, tile_n, (char *)nullptr, (int32_t *)nullptr, cells);
}

void launch_mutate_record_bases(PileGenome g, const int64_t *part, const int64_t *tile_off, int64_t *base_at, hipStream_t st) {
  if (g.total <= 0) return;
  hipLaunchKernelGGL(k_mut_record_bases, dim3((unsigned)((g.n + 1 + 255) / 256)), dim3(256), 0, st, g.n, g.at, part, tile_off, tiles_of(g), base_at);
}

void launch_mutate_base_fill(PileGenome g, pbsim_mutate_opts o, MutSites s, const int64_t *base_at, const int64_t *byte_at, const int64_t *tile_off,
                             char *text, int32_t *origin, hipStream_t st) {
  if (g.total <= 0 || (!text && !origin)) return;
  const int64_t blocks = std::min<int64_t>(tiles_of(g), kBaseBlocksMax);
  hipLaunchKernelGGL(k_mut_bases<true>, dim3((unsigned)blocks), dim3(kThreads), 0, st, g, o, s, (int64_t *)nullptr, base_at, byte_at, tile_off,
                     (int64_t *)nullptr, text, origin, (unsigned long long *)nullptr);
}

void launch_mutate_line_sizes(PileGenome g, MutSites s, int64_t *tile_n, unsigned long long *cells, unsigned long long *rec_n, hipStream_t st) {
  if (g.total <= 0) return;
  const int64_t blocks = std::min<int64_t>(tiles_of(g), kLineBlocksMax);
  const pbsim_mutate_opts none = {};
  hipLaunchKernelGGL(k_mut_lines<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, g, none, s, (const int64_t *)nullptr, tile_n, (char *)nullptr,
                     cells, rec_n);
}

void launch_mutate_line_fill(PileGenome g, pbsim_mutate_opts o, MutSites s, const int64_t *tile_off, char *text, hipStream_t st) {
  if (g.total <= 0) return;
  const int64_t blocks = std::min<int64_t>(tiles_of(g), kLineBlocksMax);
  hipLaunchKernelGGL(k_mut_lines<true>, dim3((unsigned)blocks), dim3(kThreads), 0, st, g, o, s, tile_off, (int64_t *)nullptr, text,
                     (unsigned long long *)nullptr, (unsigned long long *)nullptr);
}

}  // namespace pbsim
