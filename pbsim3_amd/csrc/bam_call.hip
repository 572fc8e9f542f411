// bam_call.hip -- the kernels of pbsim_bam_call: the differences between the genome and what the pile of reads spells, joined
// into events and written as VCF lines on the device.  Everything in front of them is pbsim_bam_consensus's (bam_consensus.hip,
// through launch_consensus_base_sizes): the class byte of every position, the eight cells, the ins_sites' slots with their emitted
// lengths and tallied cells.  The rule: include/pbsim3_amd.h.
//
//   lines : one lane per position, workgroups striding over the tiles of kCallTile positions.  A lane whose position is an anchor
//           (a site that is no del_site) reads the class bytes of its two neighbours; where it is no sub_site and no ins_site and
//           neither neighbour is a del_site its group is the position alone and spells the genome: 0 bytes, from three class
//           bytes that share their cache line with the neighbouring lanes'.  Nearly every lane takes this path.  Otherwise the
//           lane walks its group, serially: back over the del_sites in front of it to learn whether the run reaches the record's
//           first position (then the group takes it), forward over the del_sites behind it, then once over the group's positions
//           for the ALT string's length, its first byte, whether it equals REF, and the smallest support; an ins_site's slot
//           comes from a binary search among the slots' places.  The line's length is scanned across the workgroup.  The first
//           pass leaves a tile's bytes (8 bytes per tile), the counts (registers, one reduction per wave at the end, one global
//           add per workgroup and cell, an atomic max for the two longest values) and one add per written record into its genome
//           record's counter; the lane at a record's first position, where that is a del_site, walks the run to learn whether
//           the record has an anchor at all.  After the tiles' exclusive scan the second pass walks the same way and writes the
//           line at the tile's offset plus the lane's: one lane writes a whole REF and ALT.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bam_call.h"
#include "bam_pileup_walk.h"

namespace pbsim {

namespace {

using namespace pilewalk;

constexpr int kLineBlocksMax = 2048;  // workgroups of the line pass: they stride over the tiles
static_assert(kCallTile == kThreads, "a tile is one workgroup's positions");

// (a byte of the padding has 7 in its class bits: no del_site)
__device__ __forceinline__ bool del_site(uint32_t c) { return (c & 7u) == (uint32_t)kPileDel; }

// What the positions lo .. hi spell, in order: byte(ch) per byte of E(lo) .. E(hi), and with kSupport support(n) per count
// that stands behind a byte that is not the genome's or behind a deleted one.
template <bool kSupport, class Byte, class Support>
__device__ __forceinline__ void spell(const PileGenome &g, const uint32_t *table, const uint8_t *cls, const ConsSlots &slots, int64_t lo, int64_t hi,
                                      Byte byte, Support support) {
  for (int64_t p = lo; p <= hi; p++) {
    const uint32_t c = cls[p], kind = c & 7u, call = (c >> 4) & 7u;
    if (kind == kPileRefN || kind == kPileLow) {
      byte((char)g.seq[p]);
    } else if (call < 4) {
      byte("ACGT"[call]);
      if (kSupport && kind == kPileSub) support((u64)table[p * kPileWidth + call]);
    } else if (kSupport) {
      support((u64)table[p * kPileWidth + kPcDel]);
    }
    if (!(c & kPileInsBit)) continue;
    const int64_t k = slot_of(slots, p);
    if (k < 0) continue;  // (never: every ins_site has its slot)
    const int64_t l = slots.len[k];
    const uint32_t *q = slots.cell + slots.off[k] * 5;
    for (int64_t j = 0; j < l; j++, q += 5) {
      byte(ins_base(q));
      if (kSupport) support((u64)q[0] + q[1] + q[2] + q[3] + q[4]);
    }
  }
}

struct Group {
  int64_t lo, hi;
  u64 ref_len, alt_len, dp, ms;
  int type;
  bool written;
};

// the group of the anchor at i over lo .. hi: its strings' lengths, whether they differ, DP, MS and the type
__device__ __forceinline__ Group measure(const PileGenome &g, const uint32_t *table, const uint8_t *cls, const ConsSlots &slots, int64_t i, int64_t lo,
                                         int64_t hi) {
  Group m;
  m.lo = lo, m.hi = hi, m.ref_len = (u64)(hi - lo + 1);
  u64 alt_len = 0, ms = ~0ull;
  bool same = true;
  char first = 0;
  const uint8_t *ref = g.seq + lo;
  const u64 ref_len = m.ref_len;
  spell<true>(
      g, table, cls, slots, lo, hi,
      [&](char ch) {
        if (alt_len == 0) first = ch;
        if (alt_len >= ref_len || (char)ref[alt_len] != ch) same = false;
        alt_len++;
      },
      [&](u64 n) { ms = n < ms ? n : ms; });
  m.alt_len = alt_len, m.ms = ms;
  m.written = !(same && alt_len == ref_len);
  m.dp = load_site(table, i).depth;
  const bool begins = alt_len > 0 && first == (char)ref[0];
  m.type = ref_len == 1 && alt_len == 1 ? kCtSnv : ref_len == 1 && begins ? kCtIns : alt_len == 1 && begins ? kCtDel : kCtComplex;
  return m;
}

__device__ __forceinline__ const char *type_name(int t) { return t == kCtSnv ? "snv" : t == kCtIns ? "ins" : t == kCtDel ? "del" : "complex"; }

template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_call_lines(PileGenome g, const uint32_t *table, const uint8_t *cls, ConsSlots slots, const int64_t *tile_off,
                                                         int64_t *tile_n, char *text, u64 *cells, u64 *rec_n) {
  __shared__ u64 sh_wave[kWaves];
  __shared__ u64 sh[kWaves][kCallCells];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  u64 n_cell[kCallCells];
#pragma unroll
  for (int x = 0; x < kCallCells; x++) n_cell[x] = 0;
  const int64_t total = g.total, tiles = (total + kCallTile - 1) / kCallTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kThreads + tid;
    const uint32_t c = i < total ? cls[i] : (uint32_t)kPileNoSite;
    Group m = {};  // (written: false)
    int r = 0;
    if (c != (uint32_t)kPileNoSite && !del_site(c)) {  // an anchor
      const uint32_t prev = i > 0 ? cls[i - 1] : (uint32_t)kPileNoSite, next = i + 1 < total ? cls[i + 1] : (uint32_t)kPileNoSite;
      const bool own = (c & 7u) == kPileSub || (c & kPileInsBit) != 0;
      if (own || del_site(prev) || del_site(next)) {
        int64_t lo = i, hi = i;
        if (del_site(prev)) {  // the run in front is this group's where it reaches the record's first position
          int64_t j = i - 1;
          while (j >= 0 && del_site(cls[j])) j--;
          if (j < 0 || cls[j] == kPileNoSite) lo = j + 1;
        }
        while (hi + 1 < total && del_site(cls[hi + 1])) hi++;
        if (own || lo != i || hi != i) {
          m = measure(g, table, cls, slots, i, lo, hi);
          if (m.written) r = record_of(g, lo);
        }
      }
    } else if (!kFill && del_site(c) && (i & 63) == 0) {  // (a record begins at a multiple of 64)
      const int r0 = record_of(g, i);
      if (g.at[r0] == i) {  // the record's first position: has the record an anchor?
        int64_t j = i + 1;
        while (j < total && del_site(cls[j])) j++;
        if (j >= total || cls[j] == kPileNoSite) n_cell[kCallCellUnplacedRecords]++, n_cell[kCallCellUnplacedSites] += (u64)g.len[r0];
      }
    }
    u64 l = 0;
    int64_t name_n = 0;
    if (m.written) {
      name_n = g.name_at[r + 1] - g.name_at[r];
      const u64 pos1 = (u64)(m.lo - g.at[r]) + 1;
      // name, POS, ".", REF, ALT, ".", ".", DP=;MS=;TYPE= with their tabs and the line feed
      l = (u64)name_n + 1 + digits(pos1) + 3 + m.ref_len + 1 + m.alt_len + 8 + digits(m.dp) + 4 + digits(m.ms) + 6 + (m.type == kCtComplex ? 7 : 3) + 1;
    }
    u64 all;
    const u64 before = block_scan(l, sh_wave, wave, lane, &all);
    if (!kFill) {
      if (tid == 0) tile_n[tile] = (int64_t)all;
      if (m.written) {
        n_cell[kCallCellVariants]++;
#pragma unroll
        for (int t = 0; t < kCallTypes; t++) n_cell[kCallCellTypes + t] += m.type == t;  // (no indexed register)
        n_cell[kCallCellRefBases] += m.ref_len, n_cell[kCallCellAltBases] += m.alt_len;
        n_cell[kCallCellLongestRef] = max(n_cell[kCallCellLongestRef], m.ref_len);
        n_cell[kCallCellLongestAlt] = max(n_cell[kCallCellLongestAlt], m.alt_len);
        atomicAdd(&rec_n[r], 1ull);
      }
    } else if (m.written) {
      char *o = text + tile_off[tile] + (int64_t)before;
      const char *name = g.names + g.name_at[r];
      for (int64_t x = 0; x < name_n; x++) *o++ = name[x];
      *o++ = '\t';
      o = put(o, (u64)(m.lo - g.at[r]) + 1);
      o = put(o, "\t.\t");
      for (int64_t p = m.lo; p <= m.hi; p++) *o++ = (char)g.seq[p];
      *o++ = '\t';
      spell<false>(g, table, cls, slots, m.lo, m.hi, [&](char ch) { *o++ = ch; }, [](u64) {});
      o = put(o, "\t.\t.\tDP=");
      o = put(o, m.dp);
      o = put(o, ";MS=");
      o = put(o, m.ms);
      o = put(o, ";TYPE=");
      o = put(o, type_name(m.type));
      *o = '\n';
    }
  }
  if (kFill) return;
  u64 *cell = sh[wave];
#pragma unroll
  for (int x = 0; x < kCallCells; x++) {
    const bool longest = x == kCallCellLongestRef || x == kCallCellLongestAlt;
    const u64 v = longest ? wave_max(n_cell[x]) : wave_sum(n_cell[x]);
    if (lane == 0) cell[x] = v;
  }
  __syncthreads();
  for (int x = tid; x < kCallCells; x += kThreads) {
    if (x == kCallCellLongestRef || x == kCallCellLongestAlt) {
      u64 v = 0;
      for (int w = 0; w < kWaves; w++) v = sh[w][x] > v ? sh[w][x] : v;
      if (v) atomicMax(&cells[x], v);
      continue;
    }
    u64 sum = 0;
    for (int w = 0; w < kWaves; w++) sum += sh[w][x];
    if (sum) atomicAdd(&cells[x], sum);
  }
}

inline int64_t tiles_of(const PileGenome &g) { return (g.total + kCallTile - 1) / kCallTile; }

}  // namespace

void launch_call_line_sizes(PileGenome g, const uint32_t *table, const uint8_t *cls, ConsSlots slots, int64_t *tile_n, unsigned long long *cells,
                            unsigned long long *rec_n, hipStream_t s) {
  if (g.total <= 0) return;
  const int64_t blocks = std::min<int64_t>(tiles_of(g), kLineBlocksMax);
  hipLaunchKernelGGL(k_call_lines<false>, dim3((unsigned)blocks), dim3(kThreads), 0, s, g, table, cls, slots, (const int64_t *)nullptr, tile_n,
                     (char *)nullptr, cells, rec_n);
}

void launch_call_line_fill(PileGenome g, const uint32_t *table, const uint8_t *cls, ConsSlots slots, const int64_t *tile_off, char *text, hipStream_t s) {
  if (g.total <= 0) return;
  const int64_t blocks = std::min<int64_t>(tiles_of(g), kLineBlocksMax);
  hipLaunchKernelGGL(k_call_lines<true>, dim3((unsigned)blocks), dim3(kThreads), 0, s, g, table, cls, slots, tile_off, (int64_t *)nullptr, text,
                     (unsigned long long *)nullptr, (unsigned long long *)nullptr);
}

}  // namespace pbsim
