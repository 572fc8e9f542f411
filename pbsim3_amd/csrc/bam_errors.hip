// bam_errors.hip -- the kernels of pbsim_bam_errors: the error profile of the aligned reads of a BAM, whose inflated stream lies in
// HBM with its records located (bam_scan.hip, bam_chain.cpp), against the prepared genome beside it.  The rule:
// include/pbsim3_amd.h.
//
//   records  : one lane per record: its class, and for an aligned record the resolved CIGAR (the CG tag's array where the field is
//              the <l_seq>S<span>N placeholder), NM (bam_aux.h) and the CIGAR's sums, from which no_seq / misfit / scored follow.
//              A record of more than 64 ops is taken by its whole wave, 64 ops a round (k_stats_records' shape).  What the sums
//              alone decide is counted here, per workgroup in LDS first.  A scored record also learns how many segments it has.
//   segments : after the exclusive scan of those counts, the same walk over the scored records alone writes one ErrSegment per
//              segment.  A block is kErrSegOps consecutive ops; a segment is at most kErrSegCols consecutive columns of one
//              block, so neither a read of a million ops nor an op of a million columns stays with one wave.
//   columns  : one wave per segment, the waves striding over the segments.  A round loads 64 ops of the block, forms the wave's
//              prefix sums of their column, reference and query advances and leaves them in the wave's part of LDS; then the
//              round's columns inside the segment are taken 64 at a time, each lane finding its op by a binary search among the
//              64 prefix values.  An M = X column reads a reference byte, its class byte, a 4-bit base and a quality byte; an I
//              column the last two; a D column the first two.  An I or D op is counted (events, length bin) by the segment that
//              holds its first column.  All tallies go to cells in LDS, private to the wave (a wave adds into few bins at a time:
//              what a private copy removes is the waves' contention with each other, as in k_stats_quals), and are flushed at the
//              end with one vector atomic per cell that is not 0.  Match, sub and ambiguous are reduced across the wave per
//              segment and added to the record's three cells with one atomic each.
//   reads    : one lane per scored record: cols, identity and its histogram, the NM classes, the totals of the columns.
//   text     : one lane per record: the line's length, then (after the exclusive scan of the lengths) the bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bam_aux.h"
#include "bam_errors.h"
#include "bam_fields.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSegBlocksMax = 2048;  // workgroups of the column pass: its waves stride over the segments

typedef unsigned long long u64;

// floor(x * 1000000 / c) for x <= c < 2^62, inside 64 bits: Horner over the bits of 1000000, quotient and remainder kept apart
__device__ __forceinline__ u64 ppm_of(u64 x, u64 c) {
  u64 q = 0, r = 0;
  for (int b = 19; b >= 0; b--) {
    q <<= 1;
    r <<= 1;
    if ((1000000u >> b) & 1u) r += x;  // r < 3 c
    if (r >= c) r -= c, q++;
    if (r >= c) r -= c, q++;
  }
  return q;
}

__device__ __forceinline__ u64 wave_sum(u64 x) {
  for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
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

struct CigarSums {
  u64 m = 0, ins = 0, del = 0, soft = 0, hard = 0, skip = 0, ins_events = 0, del_events = 0;
  bool bad = false;
};

__device__ __forceinline__ void add_op(uint32_t v, CigarSums &c) {
  const uint32_t op = v & 15u;
  const u64 n = v >> 4;
  if (op > 8) c.bad = true;
  else if (op == 0 || op == 7 || op == 8) c.m += n;
  else if (op == 1) c.ins += n, c.ins_events += n != 0;
  else if (op == 2) c.del += n, c.del_events += n != 0;
  else if (op == 3) c.skip += n;
  else if (op == 4) c.soft += n;
  else if (op == 5) c.hard += n;
}

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
  if (sums) {
    sums->m = wave_sum(part.m), sums->ins = wave_sum(part.ins), sums->del = wave_sum(part.del), sums->soft = wave_sum(part.soft);
    sums->hard = wave_sum(part.hard), sums->skip = wave_sum(part.skip), sums->ins_events = wave_sum(part.ins_events);
    sums->del_events = wave_sum(part.del_events);
    sums->bad = __ballot(part.bad) != 0;
  }
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
      const uint8_t *field = p + kBamFixed + p[kBamLReadName];
      qual = field + 4 * (int64_t)n_cigar + ((int64_t)l_seq + 1) / 2;  // (the locator: the fields lie inside the record)
      cig = field;
      n_ops = n_cigar;
      int want = kAuxNm;
      if (n_ops == 2) {
        const uint32_t op0 = ld32(cig), op1 = ld32(cig + 4);
        if ((op0 & 15u) == 4 && (op0 >> 4) == l_seq && (op1 & 15u) == 3) want |= kAuxCg;
      }
      const uint8_t *aux = qual + (int64_t)l_seq;
      BamAux ax;
      const int got = aux > end ? -1 : bam_aux_walk(aux, end, want, &ax);
      if (got < 0) {
        bad = true;
      } else {
        if (got & kAuxCg) cig = ax.cg, n_ops = ax.n_cg;
        if (got & kAuxNm) has_nm = true, nm = ax.nm;
      }
    }
  }
  const bool mine = aligned && !bad;
  CigarSums c;
  u64 n_seg = 0;
  if (mine && n_ops <= 64) {
    for (uint32_t k = 0; k < n_ops; k++) add_op(ld32(cig + 4 * k), c);
    n_seg = segments_of(c.m + c.ins + c.del);  // one block
  }
  // the records of more than 64 ops, one after the other, each by the whole wave
  for (uint64_t big = __ballot(mine && n_ops > 64); big; big &= big - 1) {
    const int src = __ffsll((long long)big) - 1;
    const uint8_t *c_ops = (const uint8_t *)__shfl((int64_t)cig, src, 64);
    const int64_t n = (int64_t)__shfl(n_ops, src, 64);
    CigarSums whole;
    const u64 ns = wave_walk(c_ops, n, lane, 0, 0, &whole, nullptr);
    if (lane == src) c = whole, n_seg = ns;
  }
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
  for (uint64_t big = __ballot(mine && n_ops > 64); big; big &= big - 1) {
    const int src = __ffsll((long long)big) - 1;
    const uint8_t *c_ops = (const uint8_t *)__shfl((int64_t)cig, src, 64);
    wave_walk(c_ops, (int64_t)__shfl(n_ops, src, 64), lane, (uint32_t)__shfl(r, src, 64), __shfl(pos, src, 64), nullptr, seg + __shfl(first, src, 64));
  }
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

__device__ __forceinline__ uint32_t ref_class(uint32_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }
__device__ __forceinline__ uint32_t code_class(uint32_t nib) { return nib == 1 ? 0u : nib == 2 ? 1u : nib == 4 ? 2u : nib == 8 ? 3u : 4u; }

__global__ __launch_bounds__(kThreads) void k_err_columns(ErrRecs a, ErrRefs refs, ErrGenome g, int size_bits, const ErrSegment *seg, int64_t n_seg,
                                                          u64 *cells) {
  __shared__ unsigned int sh_cell[kWaves][kWcCells];
  __shared__ u64 sh_col[kWaves][64], sh_ref[kWaves][64], sh_query[kWaves][64];  // where each op of the round begins
  __shared__ uint32_t sh_op[kWaves][64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < kWaves * kWcCells; i += kThreads) (&sh_cell[0][0])[i] = 0;
  __syncthreads();
  unsigned int *cell = sh_cell[wave];
  u64 *w_col = sh_col[wave], *w_ref = sh_ref[wave], *w_query = sh_query[wave];
  uint32_t *w_op = sh_op[wave];
  for (int64_t s = (int64_t)blockIdx.x * kWaves + wave; s < n_seg; s += (int64_t)gridDim.x * kWaves) {
    const ErrSegment sg = seg[s];
    const uint8_t *p = a.stream + (int64_t)(a.rec[sg.rec] >> size_bits);
    const u64 l_seq = ld32(p + kBamLSeq);
    const int32_t ref_id = (int32_t)ld32(p + kBamRefId);
    const uint8_t *bases = p + kBamFixed + p[kBamLReadName] + 4 * (int64_t)ld16(p + kBamNCigarOp);
    const uint8_t *qual = bases + (l_seq + 1) / 2;
    const bool has_qual = (a.st[sg.rec] & kEsQual) != 0;
    const uint8_t *ops = a.stream + a.cig_at[sg.rec];
    const int64_t op_end = min((int64_t)sg.op0 + kErrSegOps, (int64_t)a.n_ops[sg.rec]);
    const u64 l_ref = (u64)refs.l_ref[ref_id];
    const uint8_t *g_seq = g.seq + refs.at[ref_id], *g_hp = g.hp + refs.at[ref_id];
    const u64 col_lo = (u64)sg.col0, col_hi = col_lo + kErrSegCols;
    u64 run_col = 0, run_ref = (u64)sg.ref_pos, run_query = (u64)sg.query_pos;
    u64 n_match = 0, n_sub = 0, n_amb = 0;
    for (int64_t k0 = sg.op0; k0 < op_end && run_col < col_hi; k0 += 64) {
      const uint32_t v = k0 + lane < op_end ? ld32(ops + 4 * (k0 + lane)) : 0u;
      u64 col, ref, query;
      advances(v, &col, &ref, &query);
      const u64 in_col = wave_scan(col, lane), in_ref = wave_scan(ref, lane), in_query = wave_scan(query, lane);
      const u64 my_col = run_col + in_col - col;
      __builtin_amdgcn_wave_barrier();  // (the lanes' searches of the round before are over)
      w_col[lane] = my_col, w_ref[lane] = run_ref + in_ref - ref, w_query[lane] = run_query + in_query - query;
      w_op[lane] = v;
      __builtin_amdgcn_wave_barrier();
      const u64 round_cols = __shfl(in_col, 63, 64);
      // an I or D op is counted where its first column lies
      if (col != 0 && my_col >= col_lo && my_col < col_hi) {
        const uint32_t op = v & 15u, bin = min(v >> 4, (uint32_t)kErrLenBins - 1);
        if (op == 1) atomicAdd(&cell[kWcInsLen + bin], 1u);
        else if (op == 2) atomicAdd(&cell[kWcDelLen + bin], 1u);
      }
      const u64 lo = max(col_lo, run_col), hi = min(col_hi, run_col + round_cols);
      for (u64 x0 = lo; x0 < hi; x0 += 64) {
        const u64 x = x0 + lane;
        if (x >= hi) continue;
        int i = 0;  // the last op of the round that begins at or before x: the one that holds it
        for (int d = 32; d >= 1; d >>= 1)
          if (w_col[i + d] <= x) i += d;
        const uint32_t op = w_op[i] & 15u;
        const u64 off = x - w_col[i], rp = w_ref[i] + off, qp = w_query[i] + off;
        if (op == 2) {
          if (rp >= l_ref) continue;  // (never: pos + span <= l_ref)
          const uint32_t rc = ref_class(g_seq[rp]), hv = min((uint32_t)g_hp[rp], (uint32_t)kErrHp - 1);
          atomicAdd(&cell[kWcDelBase + rc], 1u);
          atomicAdd(&cell[kWcHpCols + hv], 1u);
          atomicAdd(&cell[kWcHpDel + hv], 1u);
          continue;
        }
        if (qp >= l_seq) continue;  // (never: the query length is l_seq)
        const uint32_t nib = (bases[qp >> 1] >> (qp & 1 ? 0 : 4)) & 15u;
        const uint32_t q = has_qual ? min((uint32_t)qual[qp], (uint32_t)kErrQBins - 1) : 0u;
        if (op == 1) {
          atomicAdd(&cell[kWcInsBase + code_class(nib)], 1u);
          if (has_qual) atomicAdd(&cell[kWcQcal + 3 * q + 2], 1u);
          continue;
        }
        if (rp >= l_ref) continue;
        const uint32_t rc = ref_class(g_seq[rp]), hv = min((uint32_t)g_hp[rp], (uint32_t)kErrHp - 1);
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
      }
      run_col += round_cols, run_ref += __shfl(in_ref, 63, 64), run_query += __shfl(in_query, 63, 64);
    }
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
    l += 3;               // the tab and the class, the line feed
    for (int j = 0; j < kLineFields; j++) l += 1 + ((has >> j) & 1u ? digits(f[j]) : 1);
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
  for (int j = 0; j < kLineFields; j++) {
    *o++ = '\t';
    if ((has >> j) & 1u) o = put(o, f[j]);
    else *o++ = '*';
  }
  *o = '\n';
}

inline unsigned blocks_of(int64_t n, int per = kThreads) { return (unsigned)((n + per - 1) / per); }

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
  // a wave's cells are 32 bits wide: its segments hold fewer than 2^32 columns as long as it takes fewer than 2^20 of them
  const int64_t least = (n_seg + ((int64_t)kWaves << 19) - 1) / ((int64_t)kWaves << 19);
  const int64_t blocks = std::max<int64_t>(std::min<int64_t>((n_seg + kWaves - 1) / kWaves, kSegBlocksMax), least);
  hipLaunchKernelGGL(k_err_columns, dim3((unsigned)blocks), dim3(kThreads), 0, s, r, refs, g, kBamSamplePacking.size_bits, seg, n_seg, cells);
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
