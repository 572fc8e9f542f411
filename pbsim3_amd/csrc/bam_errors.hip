// bam_errors.hip -- the kernels of pbsim_bam_errors: the error profile of the aligned reads of a BAM, whose inflated stream lies in
// HBM with its records located (bam_scan.hip, bam_chain.cpp), against the prepared genome beside it.  The rule:
// include/pbsim3_amd.h.
//
//   records  : one lane per record: its class, and for an aligned record the resolved CIGAR (the CG tag's array where the field is
//              the <l_seq>S<span>N placeholder) and NM (bam_cigar.h's resolve_cigar) and the CIGAR's sums, from which no_seq /
//              misfit / scored follow.  A record of more than 64 ops is taken by its whole wave, 64 ops a round (bam_cigar.h's
//              each_long_cigar).  What the sums alone decide is counted here, per workgroup in LDS first.  A scored record also
//              learns how many segments it has.
//   segments : after the exclusive scan of those counts, the same walk over the scored records alone writes one ErrSegment per
//              segment.  A block is kErrSegOps consecutive ops; a segment is at most kErrSegCols consecutive columns of one
//              block, so neither a read of a million ops nor an op of a million columns stays with one wave.
//   columns  : one wave per segment, the waves striding over the segments, each segment walked by bam_cigar.h's walk_columns:
//              64 ops a round, their prefix sums in the wave's part of LDS, the round's columns inside the segment 64 at a time,
//              each lane finding its op by a binary search.  An M = X column reads a reference byte, its class byte, a 4-bit
//              base and a quality byte; an I column the last two; a D column the first two.  An I or D op is counted (events,
//              length bin) by the segment that holds its first column.  All tallies go to cells in LDS, private to the wave (a wave adds into few bins at a time:
//              what a private copy removes is the waves' contention with each other, as in k_stats_quals), and are flushed at the
//              end with one vector atomic per cell that is not 0.  Match, sub and ambiguous are reduced across the wave per
//              segment and added to the record's three cells with one atomic each.
//   reads    : one lane per scored record: cols, identity and its histogram, the NM classes, the totals of the columns.
//   text     : one lane per record: the line's length, then (after the exclusive scan of the lengths) the bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bam_cigar.h"
#include "bam_errors.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSegBlocksMax = 2048;  // workgroups of the column pass: its waves stride over the segments

__device__ __forceinline__ u64 segments_of(u64 cols) { return (cols + kErrSegCols - 1) / kErrSegCols; }

// The n ops at `ops`, by the whole wave, 64 a round; every lane gets the same values.  sums (where not null): the CIGAR's sums.
// Returns the segments of the record; with seg they are written, seg[0] the record's first.
__device__ __forceinline__ u64 wave_walk(const uint8_t *ops, int64_t n, int lane, uint32_t rec, int64_t pos, CigarSums *sums, ErrSegment *seg) {
  CigarSums part;
  u64 n_seg = 0, blk_cols = 0, blk_ref = 0, blk_query = 0, run_ref = 0, run_query = 0;
  for (int64_t k0 = 0; k0 < n + 64; k0 += 64) {  // (one more round closes the last block)
    if (k0 >= n || (k0 > 0 && k0 % kErrSegOps == 0)) {
      const u64 ns = segments_of(blk_cols);
      if (seg) {
        const int64_t op0 = (k0 - 1) / kErrSegOps * kErrSegOps;
        for (u64 c = (u64)lane; c < ns; c += 64) seg[n_seg + c] = ErrSegment{rec, (uint32_t)op0, pos + (int64_t)blk_ref, (int64_t)blk_query, (int64_t)(c * kErrSegCols)};
      }
      n_seg += ns;
      blk_cols = 0, blk_ref = run_ref, blk_query = run_query;
      if (k0 >= n) break;
    }
    u64 col = 0, ref = 0, query = 0;
    if (k0 + lane < n) {
      const uint32_t v = ld32(ops + 4 * (k0 + lane));
      if (sums) add_op(v, part);
      advances(v, &col, &ref, &query);
    }
    blk_cols += wave_sum(col), run_ref += wave_sum(ref), run_query += wave_sum(query);
  }
  if (sums) *sums = wave_total(part);
  return n_seg;
}

// the workgroup's cells of the record pass and of the read pass: the counts, then the totals
constexpr int kShCells = kErrCounts + kErrTotals;
__device__ __forceinline__ int cell_of(int k) { return k < kErrCounts ? kErrCellCounts + k : kErrCellTotals + (k - kErrCounts); }

__global__ __launch_bounds__(kThreads) void k_err_records(ErrRecs a, ErrRefs refs, int size_bits, uint32_t exclude_flags, int32_t min_mapq, u64 *cells) {
  __shared__ u64 sh[kShCells];
  if (threadIdx.x < kShCells) sh[threadIdx.x] = 0;
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool aligned = false, bad = false, has_nm = false;  // (no early return: the wave path below needs every lane)
  const uint8_t *p = a.stream, *cig = a.stream, *qual = a.stream;
  uint32_t n_ops = 0, l_seq = 0, st = 0;
  int64_t nm = 0, pos = 0, l_ref = 0;
  if (r < a.n_rec) {
    const uint64_t w = a.rec[r];
    p = a.stream + (int64_t)(w >> size_bits);
    const uint8_t *end = p + 4 + (int64_t)(w & (((uint64_t)1 << size_bits) - 1));
    const uint32_t flag = ld16(p + kBamFlag), n_cigar = ld16(p + kBamNCigarOp);
    const int32_t ref = (int32_t)ld32(p + kBamRefId);
    l_seq = ld32(p + kBamLSeq);
    pos = (int32_t)ld32(p + kBamPos);
    atomicAdd(&sh[kErrRecords], 1ull);
    if (flag & exclude_flags) {
      atomicAdd(&sh[kErrSkippedFlag], 1ull);
    } else if ((flag & 4u) || ref < 0 || ref >= refs.n_ref || pos < 0 || n_cigar == 0) {
      atomicAdd(&sh[kErrUnaligned], 1ull);
    } else if ((int32_t)p[kBamLReadName + 1] < min_mapq) {
      atomicAdd(&sh[kErrSkippedMapq], 1ull);
    } else if (refs.at[ref] < 0) {
      atomicAdd(&sh[kErrSkippedRef], 1ull);
    } else {
      aligned = true;
      st = kEsAligned;
      l_ref = refs.l_ref[ref];
      atomicAdd(&sh[kErrAligned], 1ull);
      // (the locator: the fields lie inside the record)
      qual = p + kBamFixed + p[kBamLReadName] + 4 * (int64_t)n_cigar + ((int64_t)l_seq + 1) / 2;
      const ResolvedCigar rc = resolve_cigar(p, end, l_seq, kAuxCg | kAuxNm);
      cig = rc.ops, n_ops = rc.n_ops, bad = rc.bad, has_nm = rc.has_nm, nm = rc.nm;
    }
  }
  const bool mine = aligned && !bad;
  CigarSums c;
  u64 n_seg = 0;
  if (mine && n_ops <= 64) {
    for (uint32_t k = 0; k < n_ops; k++) add_op(ld32(cig + 4 * k), c);
    n_seg = segments_of(c.m + c.ins + c.del);  // one block
  }
  each_long_cigar(mine, cig, n_ops, [&](int src, const uint8_t *c_ops, int64_t n) {
    CigarSums whole;
    const u64 ns = wave_walk(c_ops, n, lane, 0, 0, &whole, nullptr);
    if (lane == src) c = whole, n_seg = ns;
  });
  if (mine && c.bad) bad = true;
  if (mine && !bad) {
    a.cig_at[r] = cig - a.stream;
    a.n_ops[r] = n_ops;
    a.sums[4 * r] = (int64_t)c.m, a.sums[4 * r + 1] = (int64_t)c.ins, a.sums[4 * r + 2] = (int64_t)c.del, a.sums[4 * r + 3] = (int64_t)c.soft;
    a.nm[r] = nm;
    if (has_nm && nm >= 0) st |= kEsNm;
    if (l_seq == 0) {
      st |= kEsNoSeq;
      atomicAdd(&sh[kErrNoSeq], 1ull);
    } else if (c.m + c.ins + c.soft != (u64)l_seq || (u64)pos + c.m + c.del + c.skip > (u64)l_ref) {
      atomicAdd(&sh[kErrMisfit], 1ull);
    } else {
      st |= kEsScored;
      atomicAdd(&sh[kErrScored], 1ull);
      if (*qual != 0xffu) {
        st |= kEsQual;
        atomicAdd(&sh[kErrWithQual], 1ull);
      }
      atomicAdd(&sh[kErrCounts + kErrIns], c.ins);
      atomicAdd(&sh[kErrCounts + kErrDel], c.del);
      atomicAdd(&sh[kErrCounts + kErrInsEvents], c.ins_events);
      atomicAdd(&sh[kErrCounts + kErrDelEvents], c.del_events);
      atomicAdd(&sh[kErrCounts + kErrSoft], c.soft);
      atomicAdd(&sh[kErrCounts + kErrHard], c.hard);
    }
  }
  if (r < a.n_rec) {
    a.st[r] = (uint8_t)st;
    a.n_seg[r] = st & kEsScored ? (int64_t)n_seg : 0;
  }
  if (bad) atomicMin(&cells[kErrCellFault], (u64)(p - a.stream));
  __syncthreads();
  if (threadIdx.x < kShCells && sh[threadIdx.x]) atomicAdd(&cells[cell_of(threadIdx.x)], sh[threadIdx.x]);
}

// the scored records' segments, each record's from seg[n_seg[r]] on (n_seg scanned)
__global__ __launch_bounds__(kThreads) void k_err_segments(ErrRecs a, int size_bits, ErrSegment *seg) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool mine = r < a.n_rec && (a.st[r] & kEsScored);
  const uint8_t *cig = a.stream;
  uint32_t n_ops = 0;
  int64_t pos = 0, first = 0;
  if (mine) {
    cig = a.stream + a.cig_at[r];
    n_ops = a.n_ops[r];
    pos = (int32_t)ld32(a.stream + (int64_t)(a.rec[r] >> size_bits) + kBamPos);
    first = a.n_seg[r];
  }
  if (mine && n_ops <= 64) {
    const u64 ns = segments_of((u64)(a.sums[4 * r] + a.sums[4 * r + 1] + a.sums[4 * r + 2]));
    for (u64 c = 0; c < ns; c++) seg[first + (int64_t)c] = ErrSegment{(uint32_t)r, 0u, pos, 0, (int64_t)(c * kErrSegCols)};
  }
  each_long_cigar(mine, cig, n_ops, [&](int src, const uint8_t *c_ops, int64_t n) {
    wave_walk(c_ops, n, lane, (uint32_t)__shfl(r, src, 64), __shfl(pos, src, 64), nullptr, seg + __shfl(first, src, 64));
  });
}

// the wave's cells of the column pass, in the order of the call's cells from kErrCellPair on
enum : int {
  kWcPair = 0,
  kWcHpCols = kWcPair + kErrPair,
  kWcHpSub = kWcHpCols + kErrHp,
  kWcHpDel = kWcHpSub + kErrHp,
  kWcInsLen = kWcHpDel + kErrHp,
  kWcDelLen = kWcInsLen + kErrLenBins,
  kWcInsBase = kWcDelLen + kErrLenBins,
  kWcDelBase = kWcInsBase + kErrBases,
  kWcQcal = kWcDelBase + kErrBases,
  kWcCells = kWcQcal + 3 * kErrQBins
};
static_assert(kErrCellQcal - kErrCellPair == kWcQcal && kErrCellHistIdentity - kErrCellPair == kWcCells, "the wave's cells lie as the call's do");

__global__ __launch_bounds__(kThreads) void k_err_columns(ErrRecs a, ErrRefs refs, ErrGenome g, const ErrSegment *seg, int64_t n_seg, u64 *cells) {
  __shared__ unsigned int sh_cell[kWaves][kWcCells];
  __shared__ WaveLds sh_walk[kWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < kWaves * kWcCells; i += kThreads) (&sh_cell[0][0])[i] = 0;
  __syncthreads();
  unsigned int *cell = sh_cell[wave];
  for (int64_t s = (int64_t)blockIdx.x * kWaves + wave; s < n_seg; s += (int64_t)gridDim.x * kWaves) {
    const ErrSegment sg = seg[s];
    const RecView rv = view_of(a, sg.rec);
    const bool has_qual = (a.st[sg.rec] & kEsQual) != 0;
    const u64 l_ref = (u64)refs.l_ref[rv.ref_id];
    const uint8_t *g_seq = g.seq + refs.at[rv.ref_id], *g_hp = g.hp + refs.at[rv.ref_id];
    const ColumnRange range = range_of(rv, sg);
    u64 n_match = 0, n_sub = 0, n_amb = 0;
    walk_columns(
        range, lane, &sh_walk[wave],
        [&](uint32_t v, u64 col, u64 my_col, u64) {
          // an I or D op is counted where its first column lies
          if (col != 0 && my_col >= range.x_lo && my_col < range.x_hi) {
            const uint32_t op = v & 15u, bin = min(v >> 4, (uint32_t)kErrLenBins - 1);
            if (op == kOpI) atomicAdd(&cell[kWcInsLen + bin], 1u);
            else if (op == kOpD) atomicAdd(&cell[kWcDelLen + bin], 1u);
          }
          return (u64)0;
        },
        [&](const Column &c) {
          if (!c.valid) return;
          if (c.op == kOpD) {
            if (c.rp >= l_ref) return;  // (never: pos + span <= l_ref)
            const uint32_t rc = ref_class(g_seq[c.rp]), hv = min((uint32_t)g_hp[c.rp], (uint32_t)kErrHp - 1);
            atomicAdd(&cell[kWcDelBase + rc], 1u);
            atomicAdd(&cell[kWcHpCols + hv], 1u);
            atomicAdd(&cell[kWcHpDel + hv], 1u);
            return;
          }
          if (c.qp >= rv.l_seq) return;  // (never: the query length is l_seq)
          const uint32_t nib = base_code(rv.bases, c.qp);
          const uint32_t q = has_qual ? min((uint32_t)rv.qual[c.qp], (uint32_t)kErrQBins - 1) : 0u;
          if (c.op == kOpI) {
            atomicAdd(&cell[kWcInsBase + code_class(nib)], 1u);
            if (has_qual) atomicAdd(&cell[kWcQcal + 3 * q + 2], 1u);
            return;
          }
          if (c.rp >= l_ref) return;
          const uint32_t rc = ref_class(g_seq[c.rp]), hv = min((uint32_t)g_hp[c.rp], (uint32_t)kErrHp - 1);
          const uint32_t bc = nib == 0 ? rc : code_class(nib);
          atomicAdd(&cell[kWcPair + 5 * rc + bc], 1u);
          atomicAdd(&cell[kWcHpCols + hv], 1u);
          if (rc == 4 || bc == 4) {
            n_amb++;
          } else {
            if (has_qual) atomicAdd(&cell[kWcQcal + 3 * q], 1u);
            if (rc == bc) {
              n_match++;
            } else {
              n_sub++;
              atomicAdd(&cell[kWcHpSub + hv], 1u);
              if (has_qual) atomicAdd(&cell[kWcQcal + 3 * q + 1], 1u);
            }
          }
        });
    n_match = wave_sum(n_match), n_sub = wave_sum(n_sub), n_amb = wave_sum(n_amb);
    if (lane == 0) {
      if (n_match) atomicAdd(&a.col[3 * (int64_t)sg.rec], n_match);
      if (n_sub) atomicAdd(&a.col[3 * (int64_t)sg.rec + 1], n_sub);
      if (n_amb) atomicAdd(&a.col[3 * (int64_t)sg.rec + 2], n_amb);
    }
  }
  __syncthreads();
  for (int i = tid; i < kWcCells; i += kThreads) {
    u64 sum = 0;
    for (int w = 0; w < kWaves; w++) sum += sh_cell[w][i];
    if (sum) atomicAdd(&cells[kErrCellPair + i], sum);
  }
}

__global__ __launch_bounds__(kThreads) void k_err_reads(ErrRecs a, u64 *cells) {
  __shared__ u64 sh[kShCells];
  if (threadIdx.x < kShCells) sh[threadIdx.x] = 0;
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r < a.n_rec && (a.st[r] & kEsScored)) {
    const u64 match = a.col[3 * r], sub = a.col[3 * r + 1], amb = a.col[3 * r + 2];
    const u64 ins = (u64)a.sums[4 * r + 1], del = (u64)a.sums[4 * r + 2], cols = (u64)a.sums[4 * r] + ins + del;
    atomicAdd(&sh[kErrCounts + kErrCols], cols);
    atomicAdd(&sh[kErrCounts + kErrMatch], match);
    atomicAdd(&sh[kErrCounts + kErrSub], sub);
    atomicAdd(&sh[kErrCounts + kErrAmbiguous], amb);
    if (cols >= 1) {
      const u64 identity = ppm_of(match, cols);
      atomicAdd(&sh[kErrCounts + kErrIdentitySum], identity);
      atomicAdd(&cells[kErrCellHistIdentity + identity / 1000], 1ull);
    }
    const int cls = !(a.st[r] & kEsNm) ? kErrNoNm : amb > 0 ? kErrNmUnchecked : (u64)a.nm[r] == sub + ins + del ? kErrNmAgree : kErrNmDiffer;
    atomicAdd(&sh[cls], 1ull);
  }
  __syncthreads();
  if (threadIdx.x < kShCells && sh[threadIdx.x]) atomicAdd(&cells[cell_of(threadIdx.x)], sh[threadIdx.x]);
}

// the eleven numbers behind an aligned record's name and class, and which of them the record defines (bit j: f[j]): length, cols,
// match, sub, ambiguous, ins, del, soft, nm_tag, nm_derived, identity_ppm
constexpr int kLineFields = 11;
__device__ __forceinline__ uint32_t line_fields(const ErrRecs &a, int64_t r, uint32_t st, u64 f[kLineFields]) {
  uint32_t has = 1u | 2u | 32u | 64u | 128u;
  f[0] = ld32(a.stream + (int64_t)(a.rec[r] >> kBamSamplePacking.size_bits) + kBamLSeq);
  f[5] = (u64)a.sums[4 * r + 1], f[6] = (u64)a.sums[4 * r + 2], f[7] = (u64)a.sums[4 * r + 3];
  f[1] = (u64)a.sums[4 * r] + f[5] + f[6];
  if (st & kEsNm) has |= 256u, f[8] = (u64)a.nm[r];
  if (st & kEsScored) {
    has |= 4u | 8u | 16u | 512u;
    f[2] = a.col[3 * r], f[3] = a.col[3 * r + 1], f[4] = a.col[3 * r + 2];
    f[9] = f[3] + f[5] + f[6];
    if (f[1] >= 1) has |= 1024u, f[10] = ppm_of(f[2], f[1]);
  }
  return has;
}

__global__ __launch_bounds__(kThreads) void k_err_line_sizes(ErrRecs a, int64_t *len) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.n_rec) return;
  const uint32_t st = a.st[r];
  int64_t l = 0;
  if (st & kEsAligned) {
    u64 f[kLineFields];
    const uint32_t has = line_fields(a, r, st, f);
    const uint8_t *name = a.stream + (int64_t)(a.rec[r] >> kBamSamplePacking.size_bits) + kBamFixed;
    while (name[l]) l++;  // (the locator: the name ends with a NUL inside the record)
    l += 3 + fields_len(has, f, kLineFields);  // the tab and the class, the line feed
  }
  len[r] = l;
}

__global__ __launch_bounds__(kThreads) void k_err_line_fill(ErrRecs a, const int64_t *off, char *text) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.n_rec) return;
  const uint32_t st = a.st[r];
  if (!(st & kEsAligned)) return;
  u64 f[kLineFields];
  const uint32_t has = line_fields(a, r, st, f);
  char *o = text + off[r];
  for (const uint8_t *name = a.stream + (int64_t)(a.rec[r] >> kBamSamplePacking.size_bits) + kBamFixed; *name; name++) *o++ = (char)*name;
  *o++ = '\t';
  *o++ = st & kEsScored ? 'S' : st & kEsNoSeq ? 'N' : 'F';
  *put_fields(o, has, f, kLineFields) = '\n';
}

}  // namespace

void launch_errors_records(ErrRecs r, ErrRefs refs, int32_t exclude_flags, int32_t min_mapq, ErrSegment *seg, unsigned long long *cells,
                           hipStream_t s) {
  if (r.n_rec <= 0) return;
  if (seg) hipLaunchKernelGGL(k_err_segments, dim3(blocks_of(r.n_rec)), dim3(kThreads), 0, s, r, kBamSamplePacking.size_bits, seg);
  else
    hipLaunchKernelGGL(k_err_records, dim3(blocks_of(r.n_rec)), dim3(kThreads), 0, s, r, refs, kBamSamplePacking.size_bits, (uint32_t)exclude_flags,
                       min_mapq, cells);
}

void launch_errors_columns(ErrRecs r, ErrRefs refs, ErrGenome g, const ErrSegment *seg, int64_t n_seg, unsigned long long *cells, hipStream_t s) {
  if (n_seg <= 0) return;
  hipLaunchKernelGGL(k_err_columns, dim3((unsigned)column_blocks(n_seg, kWaves, kSegBlocksMax)), dim3(kThreads), 0, s, r, refs, g, seg, n_seg, cells);
}

void launch_errors_reads(ErrRecs r, unsigned long long *cells, hipStream_t s) {
  if (r.n_rec <= 0) return;
  hipLaunchKernelGGL(k_err_reads, dim3(blocks_of(r.n_rec)), dim3(kThreads), 0, s, r, cells);
}

void launch_errors_line_sizes(ErrRecs r, int64_t *len, hipStream_t s) {
  if (r.n_rec <= 0) return;
  hipLaunchKernelGGL(k_err_line_sizes, dim3(blocks_of(r.n_rec)), dim3(kThreads), 0, s, r, len);
}

void launch_errors_line_fill(ErrRecs r, const int64_t *off, char *text, hipStream_t s) {
  if (r.n_rec <= 0) return;
  hipLaunchKernelGGL(k_err_line_fill, dim3(blocks_of(r.n_rec)), dim3(kThreads), 0, s, r, off, text);
}

}  // namespace pbsim
