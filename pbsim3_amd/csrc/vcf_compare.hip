// vcf_compare.hip -- the kernels of pbsim_vcf_compare: two VCF texts in HBM parsed, every line brought into its canonical form
// against the genome, both files' lines sorted by site, matched, tallied, and the annotated text written on the device.  The rule:
// include/pbsim3_amd.h.  The genome lies in HBM as the BAM stages hold it (bam_genome.h).  Both texts lie in one buffer, the calls
// at the first multiple of kCmpTile behind the truth, zero bytes between and 64 behind them, so that no tile holds bytes of both.
//
//   lines : a tile is kCmpTile bytes, one workgroup's, four per lane in one 32-bit load with the byte in front and the byte behind.
//           A data line begins at a file's first byte or behind a line feed, where the line is neither empty nor begins with #.
//           Sizes, the tiles' scan (launch_exclusive_scan_i64), then the fill writes every data line's start into its place of the
//           one table both files share, the truth's lines first.  A line's end is found by the lane that parses it, which reads
//           every byte of it anyway.
//   parse : one lane per data line: the spans of the columns, POS, FILTER, MS, the contig by binary search in the host-sorted table
//           of the names' hashes (FNV-1a) and then, always, by the name's bytes; REF against the genome; the trims and the left
//           move.  X is never copied: it stays a span of the line's ALT bytes and a rotation.  One lane walks a whole line and a
//           whole left move: a REF of n bases and a tandem repeat of n bases cost n steps of one lane, and its byte loads are
//           uncoalesced by nature: the pass is bound by latency, not by HBM.  A line's bytes are consecutive, so a lane's loads fall
//           into few cache lines, one after the other.
//   sort  : bam_sort.hip's bs_sort_pairs (stable) over (r << 32 | s, line); a line a class took out has the key n_refs << 32 and
//           lies behind all others.
//   match : one lane per sorted place walks its run of equal keys: an equal form earlier in its own file makes it dup; the first
//           equal form of the other file is its mate; any line of the truth in the run makes a call without mate fp_site.  Bytes
//           are compared through the rotation.  The walk is quadratic in the run's length -- lines at one (r, s) --, as
//           bam_eval.hip's k_eval_duplicates is in the reads of one name.
//   text  : a tile is kCmpTextTile lines.  The first pass tallies -- every count into a workgroup's cells in LDS, then one global
//           atomic per workgroup and cell that is not 0: integer sums and one maximum, so their order means nothing -- and sums
//           the annotated lines' bytes per tile; after the tiles' scan the second writes them.
//
// Every per-line pass strides over the lines with a capped grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "vcf_compare.h"
#include "vcf_text.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
using vcftext::base_or_n;
using vcftext::length_of;
using vcftext::line_begins;
using vcftext::put_span;
using vcftext::upper;

constexpr int kTileBlocksMax = 2048;  // workgroups of the line table's passes: they stride over the tiles of bytes
constexpr int kLaneBlocksMax = 1024;  // of the parse, the match and the text's passes: they stride over the lines
static_assert(kCmpTile == 4 * kThreads, "a lane takes four bytes of a tile");
static_assert(kCmpTextTile == kThreads, "a tile of the text is one workgroup's lines");
static_assert(sizeof(CmpLine) == 80, "the host sizes the table by it");

// ---------------------------------------------------------------- the line table
template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_cmp_lines(CmpText t, const int64_t *tile_off, int64_t *tile_n, CmpLine *line) {
  __shared__ u64 sh_wave[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int64_t tile = blockIdx.x; tile < t.tiles; tile += gridDim.x) {
    const int w = tile >= t.tiles0;
    const int64_t lo = w ? t.tiles0 * kCmpTile : 0, hi = lo + t.n[w];
    const int64_t i0 = tile * kCmpTile + (int64_t)tid * 4;
    bool begins[4];
    const u64 n = line_begins(t.bytes, i0, lo, hi, begins);  // (the buffer is aligned, and 64 bytes longer than its tiles)
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

// ---------------------------------------------------------------- parse and normalise
__global__ __launch_bounds__(kThreads) void k_cmp_parse(CmpText t, CmpGenome g, CmpLine *line, int64_t n_lines, int64_t n0, int32_t min_ms, uint64_t *key,
                                                       uint32_t *val, u64 *cells) {
  for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < n_lines; idx += (int64_t)gridDim.x * kThreads) {
    const bool calls = idx >= n0;
    const int64_t lo = calls ? t.tiles0 * kCmpTile : 0, hi = lo + t.n[calls ? 1 : 0];
    const int64_t start = line[idx].start;
    const uint8_t *p = t.bytes + start;
    const int64_t room = hi - start;  // (> 0: a line begins inside its file)
    // the columns: CHROM 0, POS 1, REF 3, ALT 4, FILTER 6, INFO 7
    int64_t chrom_n = 0, pos_off = 0, pos_n = 0, ref_off = 0, ref_n = 0, alt_off = 0, alt_n = 0, fil_off = 0, fil_n = 0, info_off = 0, info_n = 0;
    int n_cols = 0;
    int64_t begin = 0, e = 0;
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
      else if (n_cols == 7) info_off = begin, info_n = len;
      n_cols++;
      begin = e + 1;
      if (c == '\n') break;
    }
    CmpLine out = {};
    out.start = start;
    uint32_t cls = 0;
    if (e > kCmpMaxSpan) {  // (the host refuses the call)
      atomicAdd(&cells[kCmpCellTooLong], 1ull);
      cls = kCfMalformed;
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
      if (pos > (u64)kCmpMaxSpan) pos = (u64)kCmpMaxSpan + 1;
    }
    pos_ok = pos_ok && pos >= 1 && pos <= (u64)kCmpMaxSpan;
    if (!cls && (n_cols < 5 || chrom_n == 0 || ref_n == 0 || alt_n == 0 || !pos_ok)) cls = kCfMalformed;
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
      if (r < 0) cls = kCfUnknownContig;
    }
    if (!cls) {
      bool ok = true;
      for (int64_t k = 0; k < ref_n; k++) ok = ok && base_or_n(upper(p[ref_off + k]));
      for (int64_t k = 0; k < alt_n; k++) ok = ok && base_or_n(upper(p[alt_off + k]));
      if (!ok) cls = kCfUnsupported;
    }
    const uint8_t *seq = r >= 0 ? g.seq + g.at[r] : g.seq;
    int64_t s = (int64_t)pos - 1;
    if (!cls) {
      bool same = s + ref_n <= g.len[r];
      for (int64_t k = 0; same && k < ref_n; k++) same = seq[s + k] == upper(p[ref_off + k]);
      if (!same) cls = kCfRefMismatch;
    }
    if (!cls) {
      u64 ms = 0;
      if (n_cols >= 8) {  // the first MS= that begins INFO or follows a `;`
        const uint8_t *q = p + info_off;
        int64_t k = 0;
        while (k < info_n) {
          if (k + 3 <= info_n && q[k] == 'M' && q[k + 1] == 'S' && q[k + 2] == '=') {
            for (k += 3; k < info_n && q[k] >= '0' && q[k] <= '9'; k++) {
              ms = ms * 10 + (q[k] - '0');
              if (ms > (u64)kCmpMaxSpan) ms = (u64)kCmpMaxSpan;
            }
            break;
          }
          while (k < info_n && q[k] != ';') k++;
          k++;
        }
      }
      out.ms = (uint32_t)ms;
      bool filtered = calls && ms < (u64)min_ms;
      if (n_cols >= 7) {
        const uint8_t *q = p + fil_off;
        const bool pass = (fil_n == 1 && q[0] == '.') || (fil_n == 4 && q[0] == 'P' && q[1] == 'A' && q[2] == 'S' && q[3] == 'S');
        filtered = filtered || !pass;
      }
      if (filtered) cls = kCfFiltered;
    }
    if (!cls) {
      bool same = ref_n == alt_n;
      for (int64_t k = 0; same && k < ref_n; k++) same = upper(p[ref_off + k]) == upper(p[alt_off + k]);
      if (same) cls = kCfNoChange;
    }
    u64 my_key = (u64)(uint32_t)g.n << 32;
    if (!cls) {
      int64_t ro = ref_off, rn = ref_n, ao = alt_off, an = alt_n;
      while (rn > 0 && an > 0 && upper(p[ro + rn - 1]) == upper(p[ao + an - 1])) rn--, an--;
      while (rn > 0 && an > 0 && upper(p[ro]) == upper(p[ao])) ro++, ao++, rn--, an--, s++;
      int64_t shift = 0, rot = 0;
      if (an == 0) {  // a deletion: Y is the genome's own bytes s .. s + rn - 1
        while (s > 0 && seq[s - 1] == seq[s + rn - 1]) s--, shift++;
      } else if (rn == 0) {  // an insertion: k is where the rotated Y's last byte lies in the ALT bytes that are left
        int64_t k = an - 1;
        while (s > 0 && seq[s - 1] == upper(p[ao + k])) s--, shift++, k = k == 0 ? an - 1 : k - 1;
        rot = k + 1 == an ? 0 : k + 1;
      }
      out.r = r, out.s = (uint32_t)s, out.d = (uint32_t)rn;
      out.x_off = (uint32_t)ao, out.x_n = (uint32_t)an, out.x_rot = (uint32_t)rot, out.shift = (uint32_t)shift;
      out.type = (uint8_t)(rn == 1 && an == 1 ? kCtSnv : rn == 0 ? kCtIns : an == 0 ? kCtDel : kCtComplex);
      my_key = ((u64)(uint32_t)r << 32) | (u64)(uint32_t)s;
    }
    out.cls = (uint8_t)cls;
    line[idx] = out;
    key[idx] = my_key, val[idx] = (uint32_t)idx;
  }
}

// ---------------------------------------------------------------- match
// byte i of a line's X walks as p[x_off + j] with j from x_rot, wrapping at x_n
__device__ __forceinline__ bool same_form(const uint8_t *bytes, const CmpLine &a, const CmpLine &b) {
  if (a.d != b.d || a.x_n != b.x_n) return false;  // (r and s are equal: one run)
  const uint8_t *pa = bytes + a.start + a.x_off, *pb = bytes + b.start + b.x_off;
  uint32_t ja = a.x_rot, jb = b.x_rot;
  for (uint32_t k = 0; k < a.x_n; k++) {
    if (upper(pa[ja]) != upper(pb[jb])) return false;
    ja = ja + 1 == a.x_n ? 0 : ja + 1, jb = jb + 1 == b.x_n ? 0 : jb + 1;
  }
  return true;
}

__global__ __launch_bounds__(kThreads) void k_cmp_match(CmpText t, CmpLine *line, int64_t n_lines, int64_t n0, const uint64_t *key, const uint32_t *val,
                                                       int32_t n_refs) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_lines; i += (int64_t)gridDim.x * kThreads) {
    const u64 k = key[i];
    if ((k >> 32) == (u64)(uint32_t)n_refs) continue;  // a class took it out
    const int64_t me = val[i];
    const bool mine_calls = me >= n0;
    const CmpLine a = line[me];
    int64_t first = i;
    while (first > 0 && key[first - 1] == k) first--;
    bool dup = false, site = false;
    uint32_t mate = 0;
    for (int64_t j = first; j < n_lines && key[j] == k; j++) {
      if (j == i) continue;
      const int64_t other = val[j];
      const bool other_calls = other >= n0;
      if (other_calls == mine_calls) {  // (the sort is stable: a place in front is an earlier line of the file)
        if (j < i && !dup && same_form(t.bytes, a, line[other])) dup = true;
      } else {
        site = site || !other_calls;
        if (!mate && same_form(t.bytes, a, line[other])) mate = (uint32_t)(other - (other_calls ? n0 : 0) + 1);
      }
    }
    if (dup) {
      line[me].cls = (uint8_t)kCmpDup;
    } else {
      line[me].mate = mate;
      line[me].verdict = (uint8_t)(!mine_calls ? (mate ? kCvFound : kCvMissed) : mate ? kCvTp : site ? kCvFpSite : kCvFp);
    }
  }
}

// ---------------------------------------------------------------- tally and text
__device__ __forceinline__ const char *type_name(int x) { return x == kCtSnv ? "snv" : x == kCtIns ? "ins" : x == kCtDel ? "del" : "complex"; }
// the verdict of a compared line, else the class
__device__ __forceinline__ const char *word_of(const CmpLine &l) {
  switch (l.cls) {
    case kCfMalformed: return "malformed";
    case kCfUnknownContig: return "unknown_contig";
    case kCfUnsupported: return "unsupported";
    case kCfRefMismatch: return "ref_mismatch";
    case kCfFiltered: return "filtered";
    case kCfNoChange: return "no_change";
    case kCmpDup: return "dup";
    default: break;
  }
  return l.verdict == kCvFound ? "found" : l.verdict == kCvMissed ? "missed" : l.verdict == kCvTp ? "tp" : l.verdict == kCvFpSite ? "fp_site" : "fp";
}

template <bool kFill>
__global__ __launch_bounds__(kThreads) void k_cmp_text(CmpText t, const CmpLine *line, int64_t n_lines, int64_t n0, int32_t all_lines,
                                                      const int64_t *tile_off, int64_t *tile_n, char *text, u64 *cells) {
  __shared__ u64 sh_wave[kWaves];
  __shared__ unsigned int sh_cells[kCmpCells];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (!kFill) {
    for (int x = tid; x < kCmpCells; x += kThreads) sh_cells[x] = 0;
    __syncthreads();
  }
  const int64_t tiles = (n_lines + kCmpTextTile - 1) / kCmpTextTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t idx = tile * kCmpTextTile + tid;
    u64 l = 0;
    CmpLine a = {};
    int w = 0;
    bool formed = false;
    if (idx < n_lines) {
      a = line[idx];
      w = idx >= n0;
      formed = a.cls == 0 || a.cls == kCmpDup;
      const u64 number = (u64)(idx - (w ? n0 : 0) + 1);
      if (all_lines || !(a.cls == 0 && (a.verdict == kCvFound || a.verdict == kCvTp))) {
        // T or C, the number, four columns of the file, the form's four, the word, MATE: eleven tabs and the line feed
        l = 1 + digits(number) + (a.chrom_n ? a.chrom_n : 1) + (a.pos_n ? a.pos_n : 1) + (a.ref_n ? a.ref_n : 1) + (a.alt_n ? a.alt_n : 1) +
            (u64)length_of(word_of(a)) + digits(a.mate) + 12;
        l += formed ? (u64)length_of(type_name(a.type)) + digits((u64)a.s + 1) + digits(a.d) + (a.x_n ? a.x_n : 1) : 4;
      }
      if (!kFill) {
        unsigned int *f = sh_cells + kCmpCellFiles + w * kCmpFileCells;
        atomicAdd(&f[kCfLines], 1u);
        if (a.cls) atomicAdd(&f[a.cls], 1u);  // (the classes and dup: the class byte is the cell)
        else atomicAdd(&f[kCfCompared], 1u);
        if (formed && a.shift) {
          atomicAdd(&f[kCfShifted], 1u);
          atomicMax(&f[kCfLongestShift], a.shift);
        }
        if (a.cls == 0) {
          const bool hit = a.mate != 0;
          unsigned int *ty = sh_cells + kCmpCellTypes + a.type * kCmpTypeCells;
          atomicAdd(&ty[w ? kCnCalls : kCnTruth], 1u);
          if (hit) atomicAdd(&ty[w ? kCnTp : kCnFound], 1u);
          if (w && !hit) atomicAdd(&ty[kCnFp], 1u);
          if (w && a.verdict == kCvFpSite) atomicAdd(&ty[kCnFpSite], 1u);
          if (a.type == kCtIns || a.type == kCtDel) {
            const int bin = compare_bin(a.type == kCtIns ? (int64_t)a.x_n : (int64_t)a.d);
            unsigned int *ln = sh_cells + kCmpCellLengths + ((a.type == kCtIns ? 0 : 1) * kCmpBins + bin) * kCmpLengthCells;
            atomicAdd(&ln[w ? 2 : 0], 1u);
            if (hit) atomicAdd(&ln[w ? 3 : 1], 1u);
          }
          if (w) atomicAdd(&sh_cells[kCmpCellMs + 2 * (int)(a.ms < (uint32_t)(kCmpMsBins - 1) ? a.ms : (uint32_t)(kCmpMsBins - 1)) + (hit ? 0 : 1)], 1u);
        }
      }
    }
    u64 all;
    const u64 before = block_scan(l, sh_wave, wave, lane, &all);
    if (!kFill) {
      if (tid == 0) tile_n[tile] = (int64_t)all;
    } else if (l) {
      char *o = text + tile_off[tile] + (int64_t)before;
      const uint8_t *p = t.bytes + a.start;
      *o++ = w ? 'C' : 'T';
      *o++ = '\t';
      o = put(o, (u64)(idx - (w ? n0 : 0) + 1));
      *o++ = '\t';
      o = put_span(o, p, a.chrom_n);
      *o++ = '\t';
      o = put_span(o, p + a.pos_off, a.pos_n);
      *o++ = '\t';
      o = put_span(o, p + a.ref_off, a.ref_n);
      *o++ = '\t';
      o = put_span(o, p + a.alt_off, a.alt_n);
      *o++ = '\t';
      if (formed) {
        o = put(o, type_name(a.type));
        *o++ = '\t';
        o = put(o, (u64)a.s + 1);
        *o++ = '\t';
        o = put(o, (u64)a.d);
        *o++ = '\t';
        if (a.x_n == 0) *o++ = '.';
        uint32_t j = a.x_rot;
        for (uint32_t k = 0; k < a.x_n; k++) {
          *o++ = (char)upper(p[a.x_off + j]);
          j = j + 1 == a.x_n ? 0 : j + 1;
        }
      } else {
        o = put(o, ".\t.\t.\t.");
      }
      *o++ = '\t';
      o = put(o, word_of(a));
      *o++ = '\t';
      o = put(o, (u64)a.mate);
      *o = '\n';
    }
  }
  if (!kFill) {
    __syncthreads();
    for (int x = tid; x < kCmpCells; x += kThreads) {
      const unsigned int v = sh_cells[x];
      if (!v) continue;
      if (x == kCmpCellFiles + kCfLongestShift || x == kCmpCellFiles + kCmpFileCells + kCfLongestShift) atomicMax(&cells[x], (u64)v);
      else atomicAdd(&cells[x], (u64)v);
    }
  }
}

inline unsigned lane_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + kThreads - 1) / kThreads, kLaneBlocksMax); }

}  // namespace

void launch_compare_line_sizes(CmpText t, int64_t *tile_n, hipStream_t st) {
  if (t.tiles <= 0) return;
  hipLaunchKernelGGL(k_cmp_lines<false>, dim3((unsigned)std::min<int64_t>(t.tiles, kTileBlocksMax)), dim3(kThreads), 0, st, t, (const int64_t *)nullptr,
                     tile_n, (CmpLine *)nullptr);
}

void launch_compare_line_fill(CmpText t, const int64_t *tile_off, CmpLine *line, hipStream_t st) {
  if (t.tiles <= 0) return;
  hipLaunchKernelGGL(k_cmp_lines<true>, dim3((unsigned)std::min<int64_t>(t.tiles, kTileBlocksMax)), dim3(kThreads), 0, st, t, tile_off, (int64_t *)nullptr,
                     line);
}

void launch_compare_parse(CmpText t, CmpGenome g, CmpLine *line, int64_t n_lines, int64_t n0, int32_t min_ms, uint64_t *key, uint32_t *val,
                          unsigned long long *cells, hipStream_t st) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_cmp_parse, dim3(lane_blocks(n_lines)), dim3(kThreads), 0, st, t, g, line, n_lines, n0, min_ms, key, val, cells);
}

void launch_compare_match(CmpText t, CmpLine *line, int64_t n_lines, int64_t n0, const uint64_t *key, const uint32_t *val, int32_t n_refs, hipStream_t st) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_cmp_match, dim3(lane_blocks(n_lines)), dim3(kThreads), 0, st, t, line, n_lines, n0, key, val, n_refs);
}

void launch_compare_text_sizes(CmpText t, const CmpLine *line, int64_t n_lines, int64_t n0, int32_t all_lines, int64_t *tile_n, unsigned long long *cells,
                               hipStream_t st) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_cmp_text<false>, dim3(lane_blocks(n_lines)), dim3(kThreads), 0, st, t, line, n_lines, n0, all_lines, (const int64_t *)nullptr, tile_n,
                     (char *)nullptr, cells);
}

void launch_compare_text_fill(CmpText t, const CmpLine *line, int64_t n_lines, int64_t n0, int32_t all_lines, const int64_t *tile_off, char *text,
                              hipStream_t st) {
  if (n_lines <= 0) return;
  hipLaunchKernelGGL(k_cmp_text<true>, dim3(lane_blocks(n_lines)), dim3(kThreads), 0, st, t, line, n_lines, n0, all_lines, tile_off, (int64_t *)nullptr, text,
                     (unsigned long long *)nullptr);
}

}  // namespace pbsim
