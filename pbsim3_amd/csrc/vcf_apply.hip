// vcf_apply.hip -- the kernels of pbsim_vcf_apply: a VCF text in HBM parsed, every line's allele chosen and brought into its form
// against the genome, the lines sorted by site, the collisions decided, the applied lines marked at their positions, and the
// spliced genome written as FASTA with its origin map and the annotated text on the device.  The rule: include/pbsim3_amd.h.  The
// genome lies in HBM as the BAM stages hold it (bam_genome.h): every record at a multiple of 64, at least 64 bytes behind its last
// base that belong to no other record.
//
//   lines   : vcf_compare.hip's line table over one text (vcf_text.h has what the two share): a tile is kApTile bytes, four per
//             lane; sizes, the tiles' scan, the fill.
//   parse   : one lane per data line: the spans of the columns, POS, FILTER, the genotype's field and the allele's bytes in ALT, the
//             contig by binary search in the host-sorted table of the names' hashes and then by the name's bytes, REF against the
//             genome, the two trims.  X is never copied: it stays a span of the line's ALT bytes.  One lane walks a whole line, and
//             its byte loads are uncoalesced by nature: the pass is bound by latency, not by HBM.
//   sort    : bam_sort.hip's bs_sort_pairs (stable) over (r << 33 | s << 1 | d > 0, line): by site, insertions before spans, then by
//             line; a line a class took out has the key n_refs << 33 and lies behind all others.
//   reach   : (r << 32 | s + d) per sorted place and its largest per tile of kApLineTile places; one workgroup scans the tiles'
//             largest (exclusive, in place), as genome_mutate.hip does for the deletion runs' ends.
//   cluster : the scan's last level inside the tile: a place begins a cluster where its (r << 32 | s) is not below the largest reach
//             in front of it, unless it is an insertion just behind an insertion of its (r, s).  Such a line is applied whatever
//             came before: every applied span in front ends at or before it, and no insertion in front shares its site.
//   walk    : one lane per cluster walks it with the sequential rule: a cluster of n lines costs n steps of one lane.
//   marks   : one lane per applied line: its index + 1 at its start in ins_at or span_at, a span's buffer end in end[] and, with
//             one atomic maximum, in its tile's cell.  The rule leaves at most one insertion and one span per position: no race.
//   bases   : genome_mutate.hip's pair: the first pass finds the covered positions from the ends (tile scan, then the max-scan
//             inside the tile) and sums what every position emits; after the tiles' scan the second writes headers, bases, line
//             feeds and the origin map.  One lane writes a whole X, across line breaks and tile edges.
//   text    : a tile is kApLineTile lines.  The first pass tallies -- into a workgroup's cells in LDS, then one global atomic per
//             workgroup and cell that is not 0, and the records' applied lines with one atomic per wave and record: integer sums,
//             so their order means nothing -- and sums the annotated lines' bytes per tile; after the tiles' scan the second
//             writes them.
//
// Every pass strides over its tiles or lines with a capped grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bam_pileup_walk.h"
#include "vcf_apply.h"
#include "vcf_text.h"

namespace pbsim {

namespace {

using pilewalk::kThreads;
using pilewalk::kWaves;
using pilewalk::record_of;
using vcftext::base_or_n;
using vcftext::length_of;
using vcftext::line_begins;
using vcftext::put_span;
using vcftext::upper;

constexpr int kTileBlocksMax = 2048;  // workgroups of the line table's passes: they stride over the tiles of bytes
constexpr int kLaneBlocksMax = 1024;  // of the parse, the walk and the marks: they stride over the lines
constexpr int kLineBlocksMax = 1024;  // of the reach, the cluster and the text's passes: they stride over the tiles of lines
constexpr int kBaseBlocksMax = 2048;  // of the base passes: they stride over the tiles of positions
constexpr int kScanPerLane = 4;       // the tiles one lane of the scan's one workgroup takes per trip
static_assert(kApTile == 4 * kThreads, "a lane takes four bytes of a tile");
static_assert(kApLineTile == kThreads && kApPosTile == kThreads, "a tile of lines or positions is one workgroup's");
static_assert(sizeof(ApLine) == 72, "the host sizes the table by it");

__device__ __forceinline__ u64 wave_scan_max(u64 x, int lane) {  // inclusive
  for (int d = 1; d < 64; d <<= 1) {
    const u64 y = __shfl_up(x, d, 64);
    if (lane >= d && y > x) x = y;
  }
  return x;
}

// the same with the maximum: the largest v of the lanes in front (0: none), *all the workgroup's largest
__device__ __forceinline__ u64 block_scan_max(u64 v, u64 *sh_wave, int wave, int lane, u64 *all) {
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

// what a sorted key holds
__device__ __forceinline__ u64 record_of_key(u64 k) { return k >> 33; }
__device__ __forceinline__ u64 start_of_key(u64 k) { return (k >> 1) & 0xffffffffull; }
__device__ __forceinline__ u64 site_of_key(u64 k) { return (record_of_key(k) << 32) | start_of_key(k); }

// ---------------------------------------------------------------- the line table
template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_ap_lines(ApText t, const int64_t *tile_off, int64_t *tile_n, ApLine *line) {
  __shared__ u64 sh_wave[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int64_t tile = blockIdx.x; tile < t.tiles; tile += gridDim.x) {
    const int64_t i0 = tile * kApTile + (int64_t)tid * 4;
    bool begins[4];
    const u64 n = line_begins(t.bytes, i0, 0, t.n, begins);  // (the buffer is aligned, and 64 bytes longer than its tiles)
    u64 all;
    const u64 before = block_scan(n, sh_wave, wave, lane, &all);
    if (!kFill) {
      if (tid == 0) tile_n[tile] = (int64_t)all;
    } else {
      int64_t at = tile_off[tile] + (int64_t)before;
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (begins[k]) line[at++].start = i0 + k;
    }
  }
}

// ---------------------------------------------------------------- parse: columns, allele, class, form
__global__ __launch_bounds__(kThreads) void k_ap_parse(ApText t, CmpGenome g, ApLine *line, int64_t n_lines, int32_t haplotype, int32_t sample, uint64_t *key,
                                                      uint32_t *val, u64 *cells) {
  const int64_t sample_col = 9 + (int64_t)sample;
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n_lines; idx += (int64_t)gridDim.x * kThreads) {
    const int64_t start = line[idx].start;
    const uint8_t *p = t.bytes + start;
    const int64_t room = t.n - start;  // (> 0: a line begins inside the text)
    // the columns: CHROM 0, POS 1, REF 3, ALT 4, FILTER 6, FORMAT 8, the sample 9 + sample
    int64_t chrom_n = 0, pos_off = 0, pos_n = 0, ref_off = 0, ref_n = 0, alt_off = 0, alt_n = 0, fil_off = 0, fil_n = 0, fmt_off = 0, fmt_n = 0, smp_off = 0,
            smp_n = 0;
    int64_t n_cols = 0, begin = 0, e = 0;
    for (;; e++) {
      const bool over = e >= room;
      const uint32_t c = over ? (uint32_t)'\n' : p[e];
      if (c != '\n' && c != '\t') continue;
      int64_t len = e - begin;
      if (c == '\n' && !over && len > 0 && p[e - 1] == '\r') len--;
      if (n_cols == 0) chrom_n = len;
      else if (n_cols == 1) pos_off = begin, pos_n = len;
      else if (n_cols == 3) ref_off = begin, ref_n = len;
      else if (n_cols == 4) alt_off = begin, alt_n = len;
      else if (n_cols == 6) fil_off = begin, fil_n = len;
      else if (n_cols == 8) fmt_off = begin, fmt_n = len;
      if (n_cols == sample_col) smp_off = begin, smp_n = len;
      n_cols++;
      begin = e + 1;
      if (c == '\n') break;
    }
    if (n_cols > sample_col) atomicAdd(&cells[kApCellHasSample], 1ull);
    ApLine out = {};
    out.start = start;
    uint32_t cls = 0;
    if (e > kApMaxSpan) {  // (the host refuses the call)
      atomicAdd(&cells[kApCellTooLong], 1ull);
      cls = kApMalformed;
      chrom_n = pos_n = ref_n = alt_n = 0;
    }
    out.chrom_n = (uint32_t)chrom_n, out.pos_off = (uint32_t)pos_off, out.pos_n = (uint32_t)pos_n, out.ref_off = (uint32_t)ref_off;
    out.ref_n = (uint32_t)ref_n, out.alt_off = (uint32_t)alt_off, out.alt_n = (uint32_t)alt_n;
    // POS: one or more digits, 1 .. 2^31 - 1
    u64 pos = 0;
    bool pos_ok = pos_n > 0;
    for (int64_t k = 0; k < pos_n; k++) {
      const uint32_t c = p[pos_off + k];
      if (c < '0' || c > '9') pos_ok = false;
      else pos = pos * 10 + (c - '0');
      if (pos > (u64)kApMaxSpan) pos = (u64)kApMaxSpan + 1;
    }
    pos_ok = pos_ok && pos >= 1 && pos <= (u64)kApMaxSpan;
    if (!cls && (n_cols < 5 || chrom_n == 0 || ref_n == 0 || alt_n == 0 || !pos_ok)) cls = kApMalformed;
    // the alleles of ALT: k of them, none empty
    u64 n_alleles = 1;
    if (!cls) {
      bool empty = p[alt_off] == ',' || p[alt_off + alt_n - 1] == ',';
      for (int64_t k = 0; k < alt_n; k++) {
        if (p[alt_off + k] != ',') continue;
        n_alleles++;
        empty = empty || (k + 1 < alt_n && p[alt_off + k + 1] == ',');
      }
      if (empty) cls = kApMalformed;
    }
    // the allele's number: 1, or the genotype's field of the haplotype
    u64 number = 1;
    bool no_call = false;
    if (!cls && haplotype != 0) {
      const uint8_t *f = p + fmt_off, *q = p + smp_off;
      bool ok = n_cols > sample_col && fmt_n >= 2 && f[0] == 'G' && f[1] == 'T' && (fmt_n == 2 || f[2] == ':');
      int64_t gn = 0;
      while (ok && gn < smp_n && q[gn] != ':') gn++;
      u64 value0 = 0, value1 = 0;  // (no arrays: a lane's index into one would send it to scratch)
      bool dot0 = false, dot1 = false;
      int n_fields = 0;
      for (int64_t k = 0; ok;) {
        if (n_fields == 2) {  // a third field
          ok = false;
          break;
        }
        if (k < gn && q[k] == '.') {
          if (n_fields == 0) dot0 = true;
          else dot1 = true;
          k++;
        } else if (k < gn && q[k] >= '0' && q[k] <= '9') {
          u64 v = 0;
          for (; k < gn && q[k] >= '0' && q[k] <= '9'; k++) {
            v = v * 10 + (q[k] - '0');
            if (v > (u64)kApMaxSpan) v = (u64)kApMaxSpan;
          }
          if (n_fields == 0) value0 = v;
          else value1 = v;
        } else {
          ok = false;
          break;
        }
        n_fields++;
        if (k == gn) break;
        if (q[k] != '/' && q[k] != '|') ok = false;
        k++;
      }
      if (ok) {
        const bool second = n_fields == 2 && haplotype == 2;
        no_call = second ? dot1 : dot0, number = second ? value1 : value0;
        ok = no_call || number <= n_alleles;
      }
      if (!ok) cls = kApMalformed;
    }
    if (!cls && !no_call) out.has_allele = 1, out.allele = (uint32_t)number;
    int r = -1;
    if (!cls) {  // the contig: the first place of its hash, then the names with that hash, byte by byte
      u64 h = 0xcbf29ce484222325ull;
      for (int64_t k = 0; k < chrom_n; k++) h = (h ^ p[k]) * 0x100000001b3ull;
      int a = 0, b = g.n;  // hash[a - 1] < h <= hash[b]
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (g.hash[mid] < h) a = mid + 1;
        else b = mid;
      }
      for (; a < g.n && g.hash[a] == h && r < 0; a++) {
        const int cand = g.record[a];
        const int64_t at = g.name_at[cand];
        if (g.name_at[cand + 1] - at != chrom_n) continue;
        int64_t k = 0;
        while (k < chrom_n && (uint8_t)g.names[at + k] == p[k]) k++;
        if (k == chrom_n) r = cand;
      }
      if (r < 0) cls = kApUnknownContig;
    }
    if (!cls && no_call) cls = kApNoCall;
    if (!cls && number == 0) cls = kApRefAllele;
    // the allele's bytes: behind the (number - 1)-th comma of ALT
    int64_t ao = alt_off, an = 0;
    if (!cls) {
      u64 commas = 0;
      int64_t k = 0;
      for (; k < alt_n && commas + 1 < number; k++) commas += p[alt_off + k] == ',';
      ao = alt_off + k;
      while (k + an < alt_n && p[alt_off + k + an] != ',') an++;
    }
    if (!cls) {
      bool ok = true;
      for (int64_t k = 0; k < ref_n; k++) ok = ok && base_or_n(upper(p[ref_off + k]));
      for (int64_t k = 0; k < an; k++) ok = ok && base_or_n(upper(p[ao + k]));
      if (!ok) cls = kApUnsupported;
    }
    const uint8_t *seq = r >= 0 ? g.seq + g.at[r] : g.seq;
    int64_t s = (int64_t)pos - 1;
    if (!cls) {
      bool same = s + ref_n <= g.len[r];
      for (int64_t k = 0; same && k < ref_n; k++) same = seq[s + k] == upper(p[ref_off + k]);
      if (!same) cls = kApRefMismatch;
    }
    if (!cls && n_cols >= 7) {
      const uint8_t *q = p + fil_off;
      const bool pass = (fil_n == 1 && q[0] == '.') || (fil_n == 4 && q[0] == 'P' && q[1] == 'A' && q[2] == 'S' && q[3] == 'S');
      if (!pass) cls = kApFiltered;
    }
    if (!cls) {
      bool same = ref_n == an;
      for (int64_t k = 0; same && k < ref_n; k++) same = upper(p[ref_off + k]) == upper(p[ao + k]);
      if (same) cls = kApNoChange;
    }
    u64 my_key = (u64)(uint32_t)g.n << 33;
    if (!cls) {  // the prefix first, then the suffix
      int64_t ro = ref_off, rn = ref_n;
      while (rn > 0 && an > 0 && upper(p[ro]) == upper(p[ao])) ro++, ao++, rn--, an--, s++;
      while (rn > 0 && an > 0 && upper(p[ro + rn - 1]) == upper(p[ao + an - 1])) rn--, an--;
      out.r = r, out.s = (uint32_t)s, out.d = (uint32_t)rn;
      out.x_off = (uint32_t)ao, out.x_n = (uint32_t)an;
      out.type = (uint8_t)(rn == 1 && an == 1 ? kAtSnv : rn == 0 ? kAtIns : an == 0 ? kAtDel : kAtComplex);
      my_key = ((u64)(uint32_t)r << 33) | ((u64)(uint32_t)s << 1) | (rn > 0 ? 1ull : 0ull);
    }
    out.cls = (uint8_t)cls;
    line[idx] = out;
    key[idx] = my_key, val[idx] = (uint32_t)idx;
  }
}

// ---------------------------------------------------------------- the collisions
__global__ __launch_bounds__(kThreads) void k_ap_reach(const ApLine *line, int64_t n_lines, const uint64_t *key, const uint32_t *val, int32_t n_refs, u64 *reach,
                                                      u64 *tile_max) {
  __shared__ u64 sh_wave[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t tiles = (n_lines + kApLineTile - 1) / kApLineTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kApLineTile + tid;
    u64 v = 0;
    if (i < n_lines) {
      const u64 k = key[i];
      if (record_of_key(k) != (u64)(uint32_t)n_refs) v = site_of_key(k) + line[val[i]].d;  // (s + d stays below 2^31)
      reach[i] = v;
    }
    const u64 most = wave_max(v);
    if (lane == 0) sh_wave[wave] = most;
    __syncthreads();
    if (tid == 0) {
      u64 m = 0;
      for (int w = 0; w < kWaves; w++) m = sh_wave[w] > m ? sh_wave[w] : m;
      tile_max[tile] = m;
    }
    __syncthreads();
  }
}

// one workgroup: tile[t] becomes the largest of tile[0 .. t - 1], kThreads * kScanPerLane tiles per trip
__global__ __launch_bounds__(kThreads) void k_ap_tile_scan(u64 *tile, int64_t tiles) {
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

__global__ __launch_bounds__(kThreads) void k_ap_cluster(int64_t n_lines, const uint64_t *key, int32_t n_refs, const u64 *reach, const u64 *tile_max,
                                                        uint8_t *start) {
  __shared__ u64 sh_wave[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t tiles = (n_lines + kApLineTile - 1) / kApLineTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kApLineTile + tid;
    u64 all;
    const u64 in_tile = block_scan_max(i < n_lines ? reach[i] : 0, sh_wave, wave, lane, &all), in_front = tile_max[tile];
    if (i < n_lines) {
      const u64 k = key[i], front = in_tile > in_front ? in_tile : in_front;
      const bool left = record_of_key(k) != (u64)(uint32_t)n_refs;
      const bool chained = (k & 1) == 0 && i > 0 && key[i - 1] == k;  // an insertion just behind an insertion of its (r, s)
      start[i] = (uint8_t)(!left || (site_of_key(k) >= front && !chained));
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_ap_walk(ApLine *line, int64_t n_lines, const uint64_t *key, const uint32_t *val, int32_t n_refs,
                                                     const uint8_t *start, u64 *cells) {
  u64 longest = 0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_lines; i += (int64_t)gridDim.x * kThreads) {
    if (!start[i] || record_of_key(key[i]) == (u64)(uint32_t)n_refs) continue;
    // the rule, from a line that is applied whatever came before; a cluster stays inside its record
    u64 end = 0, ins_s = ~0ull, n = 0;
    uint32_t owner = 0, ins_line = 0;
    for (int64_t j = i; j < n_lines && (j == i || !start[j]); j++, n++) {
      const uint32_t me = val[j];
      const u64 s = start_of_key(key[j]), d = line[me].d;
      if (s < end) {
        line[me].cls = (uint8_t)kApOverlap, line[me].by = owner;
      } else if (d == 0 && ins_s == s) {
        line[me].cls = (uint8_t)kApOverlap, line[me].by = ins_line;
      } else if (d == 0) {
        ins_s = s, ins_line = me + 1;
      } else {
        end = s + d, owner = me + 1;
      }
    }
    longest = n > longest ? n : longest;
  }
  longest = wave_max(longest);
  if ((threadIdx.x & 63) == 0 && longest) atomicMax(&cells[kApCellLongestCluster], longest);
}

__global__ __launch_bounds__(kThreads) void k_ap_marks(const ApLine *line, int64_t n_lines, const int64_t *at, ApMarks m) {
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n_lines; idx += (int64_t)gridDim.x * kThreads) {
    const ApLine &a = line[idx];
    if (a.cls != kApApplied) continue;
    const int64_t i = at[a.r] + a.s;  // (s <= l_ref: inside the record's own part of the buffers)
    if (a.d == 0) {
      m.ins_at[i] = (uint32_t)idx + 1;
    } else {
      m.span_at[i] = (uint32_t)idx + 1;
      m.end[i] = (u64)i + a.d;
      atomicMax(&m.tile[i / kApPosTile], (u64)i + a.d);
    }
  }
}

// ---------------------------------------------------------------- the bases
// base idx of a record whose bases begin at o: its byte, and the line feed behind it where it ends a line or the record
__device__ __forceinline__ void put_base(char *o, int64_t idx, int64_t n_bases, int64_t line_width, char ch) {
  const int64_t at = idx + (line_width ? idx / line_width : 0);
  o[at] = ch;
  if (idx == n_bases - 1 || (line_width && (idx + 1) % line_width == 0)) o[at + 1] = '\n';
}

template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_ap_bases(PileGenome g, ApText t, const ApLine *line, ApMarks m, int32_t width, int64_t *part,
                                                      const int64_t *base_at, const int64_t *byte_at, const int64_t *tile_off, int64_t *tile_n, char *text,
                                                      int32_t *origin, u64 *cells) {
  __shared__ u64 sh_wave[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t tiles = (g.total + kApPosTile - 1) / kApPosTile, line_width = width;
  u64 n_out = 0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t i = tile * kThreads + tid;
    const bool in = i < g.total;
    const uint32_t ins = in ? m.ins_at[i] : 0, span = in ? m.span_at[i] : 0;
    u64 all;
    // the scan's last level: an end in front of i that lies above i
    const u64 in_tile = block_scan_max(in ? m.end[i] : 0, sh_wave, wave, lane, &all), in_front = m.tile[tile];
    const bool covered = (in_tile > in_front ? in_tile : in_front) > (u64)i;
    int r = 0;
    int64_t p = 0;
    bool site = false;
    if (in) {
      r = record_of(g, i);
      p = i - g.at[r];
      site = p < g.len[r];
    }
    const u64 l_ins = ins ? line[ins - 1].x_n : 0, l_span = span ? line[span - 1].x_n : 0;
    const u64 emits = l_ins + (!site ? 0 : span ? l_span : covered ? 0 : 1);
    const u64 before = block_scan(emits, sh_wave, wave, lane, &all);
    if (!kFill) {
      if (tid == 0) tile_n[tile] = (int64_t)all, n_out += all;
      if (in && g.at[r] == i) part[r] = (int64_t)before;
    } else if (in && (emits || g.at[r] == i)) {
      const int64_t name_n = g.name_at[r + 1] - g.name_at[r];
      char *o = text ? text + byte_at[r] : nullptr;
      if (o && g.at[r] == i) {  // the record's first position, or with no bases its padding: the header line
        const char *name = g.names + g.name_at[r];
        o[0] = '>';
        for (int64_t x = 0; x < name_n; x++) o[1 + x] = name[x];
        o[1 + name_n] = '\n';
      }
      if (emits) {
        if (o) o += name_n + 2;
        const int64_t n_bases = base_at[r + 1] - base_at[r];
        int64_t idx = tile_off[tile] + (int64_t)before - base_at[r];
        int32_t *to = origin ? origin + base_at[r] : nullptr;
        if (ins) {  // behind p - 1; in front of the record's first base it has no base to stand behind
          const ApLine &a = line[ins - 1];
          const uint8_t *x = t.bytes + a.start + a.x_off;
          const int32_t from = p ? (int32_t)-p : (int32_t)(-2147483647 - 1);
          for (u64 j = 0; j < l_ins; j++, idx++) {
            if (o) put_base(o, idx, n_bases, line_width, (char)upper(x[j]));
            if (to) to[idx] = from;
          }
        }
        if (site && span) {
          const ApLine &a = line[span - 1];
          const uint8_t *x = t.bytes + a.start + a.x_off;
          for (u64 j = 0; j < l_span; j++, idx++) {
            if (o) put_base(o, idx, n_bases, line_width, (char)upper(x[j]));
            if (to) to[idx] = j < a.d ? (int32_t)(p + (int64_t)j) : (int32_t)-(p + (int64_t)a.d);
          }
        } else if (site && !covered) {
          if (o) put_base(o, idx, n_bases, line_width, (char)g.seq[i]);
          if (to) to[idx] = (int32_t)p;
        }
      }
    }
  }
  if (!kFill && tid == 0 && n_out) atomicAdd(&cells[kApCellBasesOut], n_out);
}

// ---------------------------------------------------------------- tally and text
__device__ __forceinline__ const char *type_name(int x) { return x == kAtSnv ? "snv" : x == kAtIns ? "ins" : x == kAtDel ? "del" : "complex"; }
__device__ __forceinline__ const char *word_of(int cls) {
  switch (cls) {
    case kApMalformed: return "malformed";
    case kApUnknownContig: return "unknown_contig";
    case kApNoCall: return "no_call";
    case kApRefAllele: return "ref_allele";
    case kApUnsupported: return "unsupported";
    case kApRefMismatch: return "ref_mismatch";
    case kApFiltered: return "filtered";
    case kApNoChange: return "no_change";
    case kApOverlap: return "overlap";
    default: break;
  }
  return "applied";
}

template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_ap_text(ApText t, const ApLine *line, int64_t n_lines, int32_t all_lines, const int64_t *tile_off,
                                                     int64_t *tile_n, char *text, u64 *cells, u64 *rec_n) {
  __shared__ u64 sh_wave[kWaves];
  __shared__ u64 sh_cells[kApCells];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (!kFill) {
    for (int x = tid; x < kApCells; x += kThreads) sh_cells[x] = 0;
    __syncthreads();
  }
  const int64_t tiles = (n_lines + kApLineTile - 1) / kApLineTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t idx = tile * kApLineTile + tid;
    u64 l = 0;
    ApLine a = {};
    bool formed = false;
    if (idx < n_lines) {
      a = line[idx];
      formed = a.cls == kApApplied || a.cls == kApOverlap;
      if (all_lines || a.cls != kApApplied) {
        // the number, four columns of the file, the allele, the form's four, the word, `by`: eleven tabs and the line feed
        l = digits((u64)idx + 1) + (a.chrom_n ? a.chrom_n : 1) + (a.pos_n ? a.pos_n : 1) + (a.ref_n ? a.ref_n : 1) + (a.alt_n ? a.alt_n : 1) +
            (a.has_allele ? digits(a.allele) : 1) + (u64)length_of(word_of(a.cls)) + digits(a.by) + 12;
        l += formed ? (u64)length_of(type_name(a.type)) + digits((u64)a.s + 1) + digits(a.d) + (a.x_n ? a.x_n : 1) : 4;
      }
      if (!kFill) {
        atomicAdd(&sh_cells[kApCellLines], 1ull);
        atomicAdd(&sh_cells[kApCellClass + a.cls], 1ull);
        if (a.cls == kApApplied) {
          const u64 both = a.d < a.x_n ? a.d : a.x_n;
          atomicAdd(&sh_cells[kApCellTypes + a.type], 1ull);
          if (a.x_n > both) atomicAdd(&sh_cells[kApCellInserted], a.x_n - both);
          if (a.d > both) atomicAdd(&sh_cells[kApCellDeleted], a.d - both);
          if (both) atomicAdd(&sh_cells[kApCellSubstituted], both);
        }
      }
    }
    if (!kFill) {  // the records' applied lines: one atomic per wave and record among its lines -- a file in order has one or two
      bool pending = idx < n_lines && a.cls == kApApplied;
      for (u64 left = __ballot(pending); left != 0; left = __ballot(pending)) {
        const int leader = __ffsll((long long)left) - 1;
        const int32_t r = __shfl(a.r, leader, 64);
        const u64 same = __ballot(pending && a.r == r);
        if (lane == leader) atomicAdd(&rec_n[r], (u64)__popcll(same));
        if (a.r == r) pending = false;
      }
    }
    u64 all;
    const u64 before = block_scan(l, sh_wave, wave, lane, &all);
    if (!kFill) {
      if (tid == 0) tile_n[tile] = (int64_t)all;
    } else if (l) {
      char *o = text + tile_off[tile] + (int64_t)before;
      const uint8_t *p = t.bytes + a.start;
      o = put(o, (u64)idx + 1);
      *o++ = '\t';
      o = put_span(o, p, a.chrom_n);
      *o++ = '\t';
      o = put_span(o, p + a.pos_off, a.pos_n);
      *o++ = '\t';
      o = put_span(o, p + a.ref_off, a.ref_n);
      *o++ = '\t';
      o = put_span(o, p + a.alt_off, a.alt_n);
      *o++ = '\t';
      if (a.has_allele) o = put(o, (u64)a.allele);
      else *o++ = '.';
      *o++ = '\t';
      if (formed) {
        o = put(o, type_name(a.type));
        *o++ = '\t';
        o = put(o, (u64)a.s + 1);
        *o++ = '\t';
        o = put(o, (u64)a.d);
        *o++ = '\t';
        if (a.x_n == 0) *o++ = '.';
        for (uint32_t k = 0; k < a.x_n; k++) *o++ = (char)upper(p[a.x_off + k]);
      } else {
        o = put(o, ".\t.\t.\t.");
      }
      *o++ = '\t';
      o = put(o, word_of(a.cls));
      *o++ = '\t';
      o = put(o, (u64)a.by);
      *o = '\n';
    }
  }
  if (!kFill) {
    __syncthreads();
    for (int x = tid; x < kApCells; x += kThreads)
      if (sh_cells[x]) atomicAdd(&cells[x], sh_cells[x]);
  }
}

inline unsigned lane_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + kThreads - 1) / kThreads, kLaneBlocksMax); }
inline unsigned line_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + kApLineTile - 1) / kApLineTile, kLineBlocksMax); }
inline unsigned base_blocks(const PileGenome &g) { return (unsigned)std::min<int64_t>((g.total + kApPosTile - 1) / kApPosTile, kBaseBlocksMax); }

}  // namespace

void launch_apply_line_sizes(ApText t, int64_t *tile_n, hipStream_t st) {
  if (t.tiles <= 0) return;
  hipLaunchKernelGGL(k_ap_lines<false>, dim3((unsigned)std::min<int64_t>(t.tiles, kTileBlocksMax)), dim3(kThreads), 0, st, t, (const int64_t *)nullptr, tile_n,
                     (ApLine *)nullptr);
}

void launch_apply_line_fill(ApText t, const int64_t *tile_off, ApLine *line, hipStream_t st) {
  if (t.tiles <= 0) return;
  hipLaunchKernelGGL(k_ap_lines<true>, dim3((unsigned)std::min<int64_t>(t.tiles, kTileBlocksMax)), dim3(kThreads), 0, st, t, tile_off, (int64_t *)nullptr,
                     line);
}

void launch_apply_parse(ApText t, CmpGenome g, ApLine *line, int64_t n_lines, int32_t haplotype, int32_t sample, uint64_t *key, uint32_t *val,
                        unsigned long long *cells, hipStream_t st) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_ap_parse, dim3(lane_blocks(n_lines)), dim3(kThreads), 0, st, t, g, line, n_lines, haplotype, sample, key, val, cells);
}

void launch_apply_reach(const ApLine *line, int64_t n_lines, const uint64_t *key, const uint32_t *val, int32_t n_refs, unsigned long long *reach,
                        unsigned long long *tile_max, hipStream_t st) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_ap_reach, dim3(line_blocks(n_lines)), dim3(kThreads), 0, st, line, n_lines, key, val, n_refs, reach, tile_max);
}

void launch_apply_tile_scan(unsigned long long *tile, int64_t tiles, hipStream_t st) {
  if (tiles <= 0) return;
  hipLaunchKernelGGL(k_ap_tile_scan, dim3(1), dim3(kThreads), 0, st, tile, tiles);
}

void launch_apply_cluster(int64_t n_lines, const uint64_t *key, int32_t n_refs, const unsigned long long *reach, const unsigned long long *tile_max,
                          uint8_t *start, hipStream_t st) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_ap_cluster, dim3(line_blocks(n_lines)), dim3(kThreads), 0, st, n_lines, key, n_refs, reach, tile_max, start);
}

void launch_apply_walk(ApLine *line, int64_t n_lines, const uint64_t *key, const uint32_t *val, int32_t n_refs, const uint8_t *start,
                       unsigned long long *cells, hipStream_t st) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_ap_walk, dim3(lane_blocks(n_lines)), dim3(kThreads), 0, st, line, n_lines, key, val, n_refs, start, cells);
}

void launch_apply_marks(const ApLine *line, int64_t n_lines, const int64_t *at, ApMarks m, hipStream_t st) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_ap_marks, dim3(lane_blocks(n_lines)), dim3(kThreads), 0, st, line, n_lines, at, m);
}

void launch_apply_base_sizes(PileGenome g, ApText t, const ApLine *line, ApMarks m, int64_t *part, int64_t *tile_n, unsigned long long *cells,
                             hipStream_t st) {
  if (g.total <= 0) return;
  hipLaunchKernelGGL(k_ap_bases<false>, dim3(base_blocks(g)), dim3(kThreads), 0, st, g, t, line, m, 0, part, (const int64_t *)nullptr,
                     (const int64_t *)nullptr, (const int64_t *)nullptr, tile_n, (char *)nullptr, (int32_t *)nullptr, cells);
}

void launch_apply_base_fill(PileGenome g, ApText t, const ApLine *line, ApMarks m, int32_t line_width, const int64_t *base_at, const int64_t *byte_at,
                            const int64_t *tile_off, char *text, int32_t *origin, hipStream_t st) {
  if (g.total <= 0 || (!text && !origin)) return;
  hipLaunchKernelGGL(k_ap_bases<true>, dim3(base_blocks(g)), dim3(kThreads), 0, st, g, t, line, m, line_width, (int64_t *)nullptr, base_at, byte_at, tile_off,
                     (int64_t *)nullptr, text, origin, (unsigned long long *)nullptr);
}

void launch_apply_text_sizes(ApText t, const ApLine *line, int64_t n_lines, int32_t all_lines, int64_t *tile_n, unsigned long long *cells,
                             unsigned long long *rec_n, hipStream_t st) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_ap_text<false>, dim3(line_blocks(n_lines)), dim3(kThreads), 0, st, t, line, n_lines, all_lines, (const int64_t *)nullptr, tile_n,
                     (char *)nullptr, cells, rec_n);
}

void launch_apply_text_fill(ApText t, const ApLine *line, int64_t n_lines, int32_t all_lines, const int64_t *tile_off, char *text, hipStream_t st) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_ap_text<true>, dim3(line_blocks(n_lines)), dim3(kThreads), 0, st, t, line, n_lines, all_lines, tile_off, (int64_t *)nullptr, text,
                     (unsigned long long *)nullptr, (unsigned long long *)nullptr);
}

}  // namespace pbsim
