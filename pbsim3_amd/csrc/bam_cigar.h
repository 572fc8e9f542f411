// bam_cigar.h -- what the BAM stages' kernels share about a record's CIGAR: the ops' algebra and the CIGAR's sums, the resolved
// CIGAR (the CG tag's array where the field is the <l_seq>S<span>N placeholder), the turn of the records of more than 64 ops by
// their whole wave, the record's fields a column pass needs, and the column walk itself, which bam_errors.hip, the pileup
// (bam_pileup_walk.h) and bam_lift.hip run with their own bodies.  Device code: included by .hip files only.  Internal: nothing
// here is part of include/pbsim3_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bam_aux.h"
#include "bam_errors.h"
#include "bam_fields.h"
#include "device_util.h"

namespace pbsim {

enum : uint32_t { kOpM = 0, kOpI = 1, kOpD = 2, kOpN = 3, kOpS = 4, kOpH = 5, kOpP = 6, kOpEq = 7, kOpX = 8, kOpNone = 15 };

// what one op advances: the columns of the alignment (M = X I D), the reference (M = X D N), the query (M = X I S)
__device__ __forceinline__ void advances(uint32_t v, u64 *col, u64 *ref, u64 *query) {
  const uint32_t op = v & 15u;
  const u64 n = v >> 4;
  const bool m = op == kOpM || op == kOpEq || op == kOpX;
  *col = m || op == kOpI || op == kOpD ? n : 0;
  *ref = m || op == kOpD || op == kOpN ? n : 0;
  *query = m || op == kOpI || op == kOpS ? n : 0;
}

struct CigarSums {
  u64 m = 0, ins = 0, del = 0, soft = 0, hard = 0, skip = 0, ins_events = 0, del_events = 0;
  bool bad = false;
};

__device__ __forceinline__ void add_op(uint32_t v, CigarSums &c) {
  const uint32_t op = v & 15u;
  const u64 n = v >> 4;
  if (op > kOpX) c.bad = true;
  else if (op == kOpM || op == kOpEq || op == kOpX) c.m += n;
  else if (op == kOpI) c.ins += n, c.ins_events += n != 0;
  else if (op == kOpD) c.del += n, c.del_events += n != 0;
  else if (op == kOpN) c.skip += n;
  else if (op == kOpS) c.soft += n;
  else if (op == kOpH) c.hard += n;
}

// the lanes' partial sums added up: every lane gets the wave's
__device__ __forceinline__ CigarSums wave_total(const CigarSums &part) {
  CigarSums c;
  c.m = wave_sum(part.m), c.ins = wave_sum(part.ins), c.del = wave_sum(part.del), c.soft = wave_sum(part.soft);
  c.hard = wave_sum(part.hard), c.skip = wave_sum(part.skip), c.ins_events = wave_sum(part.ins_events);
  c.del_events = wave_sum(part.del_events);
  c.bad = __ballot(part.bad) != 0;
  return c;
}

// the sums of the n ops at `ops`, by the whole wave: op k by lane k mod 64
__device__ __forceinline__ CigarSums wave_cigar_sums(const uint8_t *ops, int64_t n, int lane) {
  CigarSums part;
  for (int64_t k = lane; k < n; k += 64) add_op(ld32(ops + 4 * k), part);
  return wave_total(part);
}

__device__ __forceinline__ uint32_t ref_class(uint32_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }
__device__ __forceinline__ uint32_t code_class(uint32_t nib) { return nib == 1 ? 0u : nib == 2 ? 1u : nib == 4 ? 2u : nib == 8 ? 3u : 4u; }
// the 4-bit code of base qp of a record's SEQ field
__device__ __forceinline__ uint32_t base_code(const uint8_t *bases, u64 qp) { return (bases[qp >> 1] >> (qp & 1 ? 0 : 4)) & 15u; }

// A record's CIGAR as the stages take it: the field's ops, or the CG tag's where the field is the placeholder; NM where it was
// wanted and found.  bad: an aux field runs past the record or has an unknown type.
struct ResolvedCigar {
  const uint8_t *ops;
  uint32_t n_ops;
  bool bad, has_nm;
  int64_t nm;
};

// The record at p, which ends at `end` (the locator: its fields lie inside it); want: kAuxCg, kAuxNm or both (bam_aux.h).  The CG
// tag is looked for only where the field is the placeholder, so the aux fields are walked only where something wanted can be there.
__device__ __forceinline__ ResolvedCigar resolve_cigar(const uint8_t *p, const uint8_t *end, uint32_t l_seq, int want) {
  ResolvedCigar c = {p + kBamFixed + p[kBamLReadName], ld16(p + kBamNCigarOp), false, false, 0};
  const uint8_t *aux = c.ops + 4 * (int64_t)c.n_ops + ((int64_t)l_seq + 1) / 2 + (int64_t)l_seq;
  int look = want & kAuxNm;
  if (c.n_ops == 2) {
    const uint32_t op0 = ld32(c.ops), op1 = ld32(c.ops + 4);
    if ((op0 & 15u) == 4 && (op0 >> 4) == l_seq && (op1 & 15u) == 3) look |= want & kAuxCg;
  }
  if (!look) return c;
  BamAux ax;
  const int got = aux > end ? -1 : bam_aux_walk(aux, end, look, &ax);
  if (got < 0) {
    c.bad = true;
  } else {
    if (got & kAuxCg) c.ops = ax.cg, c.n_ops = ax.n_cg;
    if (got & kAuxNm) c.has_nm = true, c.nm = ax.nm;
  }
  return c;
}

// The record passes give a lane a record and let it take a CIGAR of up to 64 ops alone.  The records of more than 64 ops among
// those the lanes say are `mine` are taken one after the other, each by the whole wave: f(src, ops, n), the same for every lane,
// with the lane that holds the record, its ops and their number.  Every lane of the wave calls this.
template <class F>
__device__ __forceinline__ void each_long_cigar(bool mine, const uint8_t *ops, uint32_t n_ops, F f) {
  for (uint64_t big = __ballot(mine && n_ops > 64); big; big &= big - 1) {
    const int src = __ffsll((long long)big) - 1;
    f(src, (const uint8_t *)__shfl((int64_t)ops, src, 64), (int64_t)__shfl(n_ops, src, 64));
  }
}

// the fields of record r a column pass needs (the record pass of bam_errors.hip has resolved its CIGAR)
struct RecView {
  const uint8_t *p, *ops, *bases, *qual;
  int64_t n_ops, pos;
  u64 l_seq;
  int32_t ref_id;
};
__device__ __forceinline__ RecView view_of(const ErrRecs &a, int64_t r) {
  RecView v;
  v.p = a.stream + (int64_t)(a.rec[r] >> kBamSamplePacking.size_bits);
  v.ops = a.stream + a.cig_at[r];
  v.n_ops = a.n_ops[r];
  v.pos = (int32_t)ld32(v.p + kBamPos);
  v.l_seq = ld32(v.p + kBamLSeq);
  v.ref_id = (int32_t)ld32(v.p + kBamRefId);
  v.bases = v.p + kBamFixed + v.p[kBamLReadName] + 4 * (int64_t)ld16(v.p + kBamNCigarOp);
  v.qual = v.bases + (v.l_seq + 1) / 2;
  return v;
}

// What a walk covers: the ops [op0, op_end) of `ops`, the reference and query positions at op0, and the columns [x_lo, x_hi)
// counted from op0's first column.
struct ColumnRange {
  const uint8_t *ops;
  int64_t op0, op_end;
  u64 ref, query, x_lo, x_hi;
};
// a whole record's ops (the caller sets the columns)
__device__ __forceinline__ ColumnRange range_of(const RecView &rv) { return {rv.ops, 0, rv.n_ops, (u64)rv.pos, 0, 0, 0}; }
// a segment: at most kErrSegCols columns of one block of kErrSegOps ops
__device__ __forceinline__ ColumnRange range_of(const RecView &rv, const ErrSegment &sg) {
  return {rv.ops, (int64_t)sg.op0, min((int64_t)sg.op0 + kErrSegOps, rv.n_ops), (u64)sg.ref_pos, (u64)sg.query_pos, (u64)sg.col0,
          (u64)sg.col0 + kErrSegCols};
}

// the wave's part of LDS: where each op of the round begins, and the op; with a slot, one value per op from the caller's hook
struct WaveLds {
  static constexpr bool kHasSlot = false;
  u64 col[64], ref[64], query[64];
  uint32_t op[64];
};
struct WaveLdsSlot {
  static constexpr bool kHasSlot = true;
  u64 col[64], ref[64], query[64], slot[64];
  uint32_t op[64];
};

// one column of a walk: x counted as the range's columns are; op 0 (M = X), 1 or 2; off the column's offset inside its op; rp
// the reference position (of an I column: of the op's first, the position behind the anchor, plus off), qp the query index (of
// a D column: of the base behind it); slot what the hook left for the op.  Where valid is false the lane has no column and the
// rest is that of the last column of the 64.
struct Column {
  bool valid;
  uint32_t op;
  u64 x, off, rp, qp, slot;
};

struct NoOpHook {
  __device__ __forceinline__ u64 operator()(uint32_t, u64, u64, u64) const { return 0; }
};

// The columns of a range, by the whole wave.  A round loads 64 ops, forms the wave's prefix sums of their column, reference and
// query advances and leaves them in the wave's part of LDS.  hook(v, col, my_col, my_ref) is then called once by every lane
// with its op word (0 behind the last op), the columns it advances, and where it begins; what it returns is kept beside the op
// where W has a slot.  Then the round's columns inside the range are taken 64 at a time, each lane finding its op by a binary
// search among the 64 prefix values, and f(column) is called by all 64 lanes together, so that it may vote.
template <class W, class Hook, class F>
__device__ __forceinline__ void walk_columns(const ColumnRange &g, int lane, W *w, Hook hook, F f) {
  u64 run_col = 0, run_ref = g.ref, run_query = g.query;
  for (int64_t k0 = g.op0; k0 < g.op_end && run_col < g.x_hi; k0 += 64) {
    const uint32_t v = k0 + lane < g.op_end ? ld32(g.ops + 4 * (k0 + lane)) : 0u;
    u64 col, ref, query;
    advances(v, &col, &ref, &query);
    const u64 in_col = wave_scan(col, lane), in_ref = wave_scan(ref, lane), in_query = wave_scan(query, lane);
    const u64 my_col = run_col + in_col - col, my_ref = run_ref + in_ref - ref;
    __builtin_amdgcn_wave_barrier();  // (the lanes' searches of the round before are over)
    w->col[lane] = my_col, w->ref[lane] = my_ref, w->query[lane] = run_query + in_query - query;
    w->op[lane] = v;
    const u64 my_slot = hook(v, col, my_col, my_ref);
    if constexpr (W::kHasSlot) w->slot[lane] = my_slot;
    __builtin_amdgcn_wave_barrier();
    const u64 round_cols = __shfl(in_col, 63, 64);
    const u64 lo = max(g.x_lo, run_col), hi = min(g.x_hi, run_col + round_cols);
    for (u64 x0 = lo; x0 < hi; x0 += 64) {
      Column c;
      c.x = x0 + lane;
      c.valid = c.x < hi;
      const u64 xs = c.valid ? c.x : hi - 1;
      int i = 0;  // the last op of the round that begins at or before x: the one that holds it
      for (int d = 32; d >= 1; d >>= 1)
        if (w->col[i + d] <= xs) i += d;
      const uint32_t op = w->op[i] & 15u;
      c.op = op == kOpEq || op == kOpX ? (uint32_t)kOpM : op;
      c.off = xs - w->col[i];
      c.rp = w->ref[i] + c.off, c.qp = w->query[i] + c.off;
      c.slot = 0;
      if constexpr (W::kHasSlot) c.slot = w->slot[i];
      f(c);
    }
    run_col += round_cols, run_ref += __shfl(in_ref, 63, 64), run_query += __shfl(in_query, 63, 64);
  }
}

// the workgroups (of `waves` waves each, `most` of them unless more are needed) of a column pass over n_seg segments: its waves
// stride over them
inline int64_t column_blocks(int64_t n_seg, int waves, int most) {
  // a wave's cells in LDS are 32 bits wide: its segments hold fewer than 2^32 columns as long as it takes fewer than 2^20 of them
  const int64_t least = (n_seg + ((int64_t)waves << 19) - 1) / ((int64_t)waves << 19);
  return std::max<int64_t>(std::min<int64_t>((n_seg + waves - 1) / waves, most), least);
}

}  // namespace pbsim
