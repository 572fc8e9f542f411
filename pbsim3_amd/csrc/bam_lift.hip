// bam_lift.hip -- the kernels of pbsim_bam_lift: the aligned records of a BAM that lie on a variant genome, placed on the original
// genome through the variant genome's origin maps.  The inflated stream lies in HBM with its records located (bam_scan.hip,
// bam_chain.cpp) and their CIGARs resolved (the record pass of bam_errors.hip); the original genome's prepared bases and, per
// variant base, origin[] and kept_max[] (the inclusive max-scan of the kept values: what rule 8 needs as o_prev, made by rocPRIM, so
// that no lane walks back over an insertion) lie beside it.  The rule: include/pbsim3_amd.h, tests/lift_model.py.
//
//   kept, check : one lane per variant base: the scan's input; rule 2 against the scan's output.
//   span        : one wave per record, its columns walked by bam_cigar.h's walk_columns (the walk of k_err_columns and of the
//                 pileup, here over the whole record); each lane reads origin[] at its column's variant base.  It leaves the first and the
//                 last column that stays M, their query indices, the lifted pos, the clips and the verdict.
//   runs        : the same walk over the columns of the core alone, twice.  A lane's column gives up to two pieces of the lifted
//                 CIGAR: the D columns of the original bases the variant genome deleted in front of it, and its own M, I or D.
//                 A ballot and one cross-lane read give each lane the op of the last piece in front of it, so it knows where a
//                 run begins; the wave scan of those beginnings numbers the runs.  The first time the runs are counted, with M, I,
//                 D, sub (against the genome) and the gap columns; the second time, after the scan of the counts, each run's
//                 length is added up in an aligned buffer of 4 bytes per op: the lane that leads a stretch of lanes inside one run
//                 adds the stretch's length, and the op code where the run begins there, with one vector atomic.
//   sizes       : one lane per record: the new size = the old one less the old CIGAR, NM and CG fields plus the new ones.
//   write       : one wave per record: the fixed fields patched, then the name, the CIGAR, SEQ and QUAL and the aux fields that
//                 stay copied by the wave with 16-byte stores made of the source's aligned dwords shifted into place (as
//                 k_bs_gather does), byte by byte only up to the destination's first 16-byte boundary and behind its last.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>

#include "bam_cigar.h"
#include "bam_lift.h"
#include "bam_tags.h"

namespace pbsim {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRecBlocksMax = 4096;  // workgroups of the per-record wave passes: their waves stride over the records
constexpr int kSizeBits = kBamSamplePacking.size_bits;

__global__ __launch_bounds__(kThreads) void k_lift_kept(const int32_t *origin, int64_t n, int32_t *kept) {
  const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (v < n) kept[v] = origin[v] >= 0 ? origin[v] : -1;
}

__global__ __launch_bounds__(kThreads) void k_lift_check(const int32_t *origin, const int32_t *kept_max, int64_t n, int64_t l_orig, u64 *cells) {
  const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (v >= n) return;
  const int32_t o = origin[v], before = v ? kept_max[v - 1] : -1;  // the last kept value in front of v where all in front of v is good
  int kind = 0;
  if (o >= 0) kind = o >= l_orig ? kLiftBadRange : o <= before ? kLiftBadOrder : 0;
  else if (o != (before < 0 ? kLiftFront : -1 - before)) kind = kLiftBadAnchor;
  if (kind) atomicMin(&cells[kLiftCellOrigin], (u64)v << 2 | (u64)kind);
}

__global__ __launch_bounds__(kThreads) void k_lift_span(ErrRecs a, const LiftRef *refs, LiftRec *lr, u64 *cells) {
  __shared__ WaveLds sh[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  WaveLds *w = &sh[wave];
  for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < a.n_rec; r += (int64_t)gridDim.x * kWaves) {
    LiftRec out = {};
    out.verdict = kLvCopy;
    if (!(a.st[r] & kEsAligned)) {  // (wave-uniform)
      if (lane == 0) {
        lr[r] = out;
        atomicAdd(&cells[kLiftCellCounts + kLiftUnaligned], 1ull);
      }
      continue;
    }
    const RecView rv = view_of(a, r);
    const LiftRef ref = refs[rv.ref_id];
    // the clips, and whether an N or P op makes the record unsupported
    u64 col_sum = 0, ref_sum = 0, q_sum = 0, h_left = 0, h_right = 0;
    bool skip = false;
    for (int64_t k0 = 0; k0 < rv.n_ops; k0 += 64) {
      const uint32_t v = k0 + lane < rv.n_ops ? ld32(rv.ops + 4 * (k0 + lane)) : 0u;
      u64 col, rf, query;
      advances(v, &col, &rf, &query);
      const u64 before = col_sum + wave_scan(col, lane) - col;  // the columns in front of this op
      if ((v & 15u) == kOpH) (before == 0 ? h_left : h_right) += v >> 4;
      skip |= (v & 15u) == kOpN || (v & 15u) == kOpP;
      col_sum += wave_sum(col), ref_sum += wave_sum(rf), q_sum += wave_sum(query);
    }
    h_left = wave_sum(h_left), h_right = wave_sum(h_right);
    if (__ballot(skip)) {
      out.verdict = kLvUnsupported;
      if (lane == 0) {
        lr[r] = out;
        atomicAdd(&cells[kLiftCellCounts + kLiftUnsupported], 1ull);
      }
      continue;
    }
    if ((u64)rv.pos + ref_sum > (u64)ref.l_var || (rv.l_seq != 0 && q_sum != rv.l_seq)) {  // never a read outside origin[]
      if (lane == 0) {
        lr[r] = out;
        atomicMin(&cells[kLiftCellFault], (u64)(rv.p - a.stream));
      }
      continue;
    }
    bool found = false;
    u64 x_first = 0, x_last = 0, q_first = 0, q_last = 0, to_ins = 0, vanished = 0;
    int32_t pos_out = 0;
    ColumnRange range = range_of(rv);
    range.x_hi = col_sum;
    walk_columns(range, lane, w, NoOpHook(), [&](const Column &c) {
      const bool on_ref = c.valid && c.op != kOpI && c.rp < (u64)ref.l_var;
      const int32_t o = on_ref ? ref.origin[c.rp] : 0;
      const u64 kept = __ballot(on_ref && c.op == kOpM && o >= 0);
      to_ins += on_ref && c.op == kOpM && o < 0;
      vanished += on_ref && c.op == kOpD && o < 0;
      if (!kept) return;
      const int lo = __ffsll((long long)kept) - 1, hi = 63 - __clzll((long long)kept);
      if (!found) {
        found = true;
        x_first = __shfl(c.x, lo, 64), q_first = __shfl(c.qp, lo, 64), pos_out = __shfl(o, lo, 64);
      }
      x_last = __shfl(c.x, hi, 64), q_last = __shfl(c.qp, hi, 64);
    });
    to_ins = wave_sum(to_ins), vanished = wave_sum(vanished);
    out.verdict = found ? kLvLift : kLvUnplaced;
    out.x_first = (int64_t)x_first, out.x_last = (int64_t)x_last, out.q_first = (int64_t)q_first, out.q_last = (int64_t)q_last;
    out.q_total = (int64_t)q_sum, out.cols_in = (int64_t)col_sum;
    out.h_left = (uint32_t)h_left, out.h_right = (uint32_t)h_right, out.pos = pos_out;
    if (lane == 0) {
      lr[r] = out;
      if (!found) {
        atomicAdd(&cells[kLiftCellCounts + kLiftUnplaced], 1ull);
      } else {
        atomicAdd(&cells[kLiftCellCounts + kLiftLifted], 1ull);
        atomicAdd(&cells[kLiftCellTotals + kLiftColsIn], col_sum);
        atomicAdd(&cells[kLiftCellTotals + kLiftBasesToIns], to_ins);
        atomicAdd(&cells[kLiftCellTotals + kLiftDelsVanished], vanished);
        if (rv.l_seq == 0) atomicAdd(&cells[kLiftCellCounts + kLiftNoSeq], 1ull);
        if (rv.ops != rv.p + kBamFixed + rv.p[kBamLReadName]) atomicAdd(&cells[kLiftCellCounts + kLiftLongIn], 1ull);
      }
    }
  }
}

template <bool kWrite>
__global__ __launch_bounds__(kThreads) void k_lift_runs(ErrRecs a, const LiftRef *refs, ErrGenome g, LiftRec *lr, int64_t *n_ops_out,
                                                        const int64_t *cig_off, uint32_t *cig, u64 *cells) {
  __shared__ WaveLds sh[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  WaveLds *w = &sh[wave];
  for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < a.n_rec; r += (int64_t)gridDim.x * kWaves) {
    const LiftRec me = lr[r];
    if (me.verdict != kLvLift) {  // (wave-uniform)
      if (!kWrite && lane == 0) n_ops_out[r] = 0;
      continue;
    }
    const RecView rv = view_of(a, r);
    const LiftRef ref = refs[rv.ref_id];
    const uint8_t *g_seq = g.seq + ref.at;
    const u64 s_left = (u64)me.q_first, s_right = (u64)(me.q_total - 1 - me.q_last);
    const uint32_t lead = (me.h_left != 0) + (s_left != 0);  // the ops in front of the core's
    uint32_t *my_cig = kWrite ? cig + cig_off[r] : nullptr;
    u64 starts = 0;             // the runs begun so far (wave-uniform)
    uint32_t last_op = kOpNone;  // the op of the last piece so far (wave-uniform)
    u64 n_m = 0, n_i = 0, n_d = 0, n_gap = 0, n_sub = 0;
    ColumnRange range = range_of(rv);
    range.x_lo = (u64)me.x_first, range.x_hi = (u64)me.x_last + 1;
    walk_columns(range, lane, w, NoOpHook(), [&](const Column &c) {
      const bool valid = c.valid;
      const uint32_t op = c.op;
      const u64 x = c.x, rp = c.rp, qp = c.qp;
      const bool on_ref = valid && op != kOpI && rp < (u64)ref.l_var;
      const int32_t o = on_ref ? ref.origin[rp] : -1;
      // this column's own piece and the gap in front of it
      uint32_t t = kOpNone;
      if (valid) t = op == kOpI ? kOpI : op == kOpM ? (o >= 0 ? kOpM : kOpI) : (o >= 0 ? kOpD : kOpNone);
      u64 gap = 0;
      if (on_ref && o >= 0 && x > (u64)me.x_first) gap = (u64)((int64_t)o - 1 - (rp ? (int64_t)ref.kept_max[rp - 1] : -1));
      // the op of the last piece in front of this lane's
      const uint32_t mine_last = t != kOpNone ? t : gap ? kOpD : kOpNone;
      const u64 has = __ballot(mine_last != kOpNone);
      const u64 below = has & (((u64)1 << lane) - 1);
      const int src = below ? 63 - __clzll((long long)below) : 0;
      const uint32_t from_lane = __shfl(mine_last, src, 64);
      const uint32_t prev = below ? from_lane : last_op;
      const bool start_gap = gap != 0 && prev != kOpD;
      const uint32_t before_own = gap ? (uint32_t)kOpD : prev;
      const bool start_own = t != kOpNone && before_own != t;
      const u64 n_start = (u64)start_gap + (u64)start_own;
      const u64 in_start = wave_scan(n_start, lane);
      if (kWrite) {
        const u64 idx_gap = starts + in_start - n_start + (start_gap ? 1 : 0) - 1;  // (a piece in front of every run is a run's begin: never -1)
        const u64 idx_own = idx_gap + (start_own ? 1 : 0);
        if (gap) atomicAdd(&my_cig[lead + idx_gap], (uint32_t)gap << 4 | (start_gap ? (uint32_t)kOpD : 0u));
        // the lanes whose own pieces lie in one run without a gap between them: their first lane adds for all
        const u64 own = __ballot(t != kOpNone);
        const bool leads = t != kOpNone && (start_own || gap != 0 || !(own & (((u64)1 << lane) - 1)));
        const u64 leaders = __ballot(leads);
        if (leads) {
          const u64 above = lane == 63 ? 0 : leaders >> (lane + 1);
          const int next = above ? lane + __ffsll((long long)above) : 64;
          const u64 mask = (next == 64 ? ~(u64)0 : (((u64)1 << next) - 1)) & ~(((u64)1 << lane) - 1);
          atomicAdd(&my_cig[lead + idx_own], (uint32_t)__popcll(own & mask) << 4 | (start_own ? t : 0u));
        }
      } else {
        n_m += t == kOpM, n_i += t == kOpI, n_d += (t == kOpD) + gap, n_gap += gap;
        if (t == kOpM && rv.l_seq != 0 && qp < rv.l_seq && (u64)o < (u64)ref.l_orig) {
          const uint32_t nib = base_code(rv.bases, qp);
          const uint32_t rc = ref_class(g_seq[o]), bc = nib == 0 ? rc : code_class(nib);
          n_sub += rc != 4 && bc != 4 && rc != bc;
        }
      }
      starts += __shfl(in_start, 63, 64);
      if (has) last_op = __shfl(mine_last, 63 - __clzll((long long)has), 64);
    });
    if (!kWrite) {
      n_m = wave_sum(n_m), n_i = wave_sum(n_i), n_d = wave_sum(n_d), n_gap = wave_sum(n_gap), n_sub = wave_sum(n_sub);
      if (lane == 0) {
        const uint32_t n_out = lead + (uint32_t)starts + (s_right != 0) + (me.h_right != 0);
        LiftRec o = me;
        o.span = (int64_t)(n_m + n_d), o.nm = (int64_t)(n_sub + n_i + n_d), o.n_core = (uint32_t)starts, o.n_ops_out = n_out;
        lr[r] = o;
        n_ops_out[r] = n_out;
        atomicAdd(&cells[kLiftCellTotals + kLiftColsOut], n_m + n_i + n_d);
        atomicAdd(&cells[kLiftCellTotals + kLiftM], n_m);
        atomicAdd(&cells[kLiftCellTotals + kLiftIns], n_i);
        atomicAdd(&cells[kLiftCellTotals + kLiftDel], n_d);
        atomicAdd(&cells[kLiftCellTotals + kLiftSoft], s_left + s_right);
        atomicAdd(&cells[kLiftCellTotals + kLiftSub], n_sub);
        atomicAdd(&cells[kLiftCellTotals + kLiftGapDel], n_gap);
        if (n_out > (uint32_t)kCigarMaxOps) atomicAdd(&cells[kLiftCellCounts + kLiftLongOut], 1ull);
      }
    } else if (lane == 0) {  // the clips around the core
      uint32_t k = 0;
      if (me.h_left) my_cig[k++] = me.h_left << 4 | kOpH;
      if (s_left) my_cig[k++] = (uint32_t)s_left << 4 | kOpS;
      k += me.n_core;
      if (s_right) my_cig[k++] = (uint32_t)s_right << 4 | kOpS;
      if (me.h_right) my_cig[k++] = me.h_right << 4 | kOpH;
    }
  }
}

// One aux field at a, inside [a, end): its whole size, the tag and type included; -1: it runs past the end or has an unknown type.
__device__ __forceinline__ int64_t aux_field(const uint8_t *a, const uint8_t *end) {
  if (end - a < 3) return -1;
  const uint8_t t = a[2];
  int64_t size;
  if (t == 'A' || t == 'c' || t == 'C') {
    size = 1;
  } else if (t == 's' || t == 'S') {
    size = 2;
  } else if (t == 'i' || t == 'I' || t == 'f') {
    size = 4;
  } else if (t == 'Z' || t == 'H') {
    const uint8_t *z = a + 3;
    while (z < end && *z) z++;
    if (z >= end) return -1;
    size = z + 1 - (a + 3);
  } else if (t == 'B') {
    if (end - a < 8) return -1;
    const uint8_t sub = a[3];
    const int64_t each = sub == 'c' || sub == 'C' ? 1 : sub == 's' || sub == 'S' ? 2 : sub == 'i' || sub == 'I' || sub == 'f' ? 4 : 0;
    if (each == 0) return -1;
    size = 5 + (int64_t)ld32(a + 4) * each;
  } else {
    return -1;
  }
  return 3 + size > end - a ? -1 : 3 + size;
}
__device__ __forceinline__ bool aux_goes(const uint8_t *a) { return (a[0] == 'N' && a[1] == 'M') || (a[0] == 'C' && a[1] == 'G'); }

__device__ __forceinline__ int64_t tags_size(const LiftRec &me, uint32_t l_seq) {
  return (l_seq ? 3 + bam_int_size(me.nm) : 0) + (me.n_ops_out > (uint32_t)kCigarMaxOps ? 8 + 4 * (int64_t)me.n_ops_out : 0);
}

__global__ __launch_bounds__(kThreads) void k_lift_sizes(ErrRecs a, const LiftRec *lr, int64_t *size, u64 *cells) {
  const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (r >= a.n_rec) return;
  const uint64_t wd = a.rec[r];
  const uint8_t *p = a.stream + (int64_t)(wd >> kSizeBits);
  const int64_t old = 4 + (int64_t)(wd & (((uint64_t)1 << kSizeBits) - 1));
  const LiftRec me = lr[r];
  int64_t now = 0;
  if (me.verdict == kLvCopy) {
    now = old;
  } else if (me.verdict == kLvLift) {
    const uint32_t l_seq = ld32(p + kBamLSeq), n_cigar = ld16(p + kBamNCigarOp);
    const uint8_t *aux = p + kBamFixed + p[kBamLReadName] + 4 * (int64_t)n_cigar + ((int64_t)l_seq + 1) / 2 + l_seq, *end = p + old;
    int64_t gone = 0;
    while (aux < end) {
      const int64_t n = aux_field(aux, end);
      if (n < 0) {
        atomicMin(&cells[kLiftCellFault], (u64)(p - a.stream));
        break;
      }
      if (aux_goes(aux)) gone += n;
      aux += n;
    }
    const bool big = me.n_ops_out > (uint32_t)kCigarMaxOps;
    now = old - 4 * (int64_t)n_cigar - gone + 4 * (int64_t)(big ? 2 : me.n_ops_out) + tags_size(me, l_seq);
    atomicAdd(&cells[kLiftCellTotals + kLiftBytesIn], (u64)old);
    atomicAdd(&cells[kLiftCellTotals + kLiftBytesOut], (u64)now);
  }
  size[r] = now;
}

// n bytes from src to dst by the whole wave: 16-byte stores where dst allows, each made of the source's aligned dwords shifted
// into place.  The source's buffer is readable 4 bytes past src + n.
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, int64_t n, int lane) {
  const int64_t head = min(n, (int64_t)((16 - ((uintptr_t)dst & 15)) & 15));
  if (lane < head) dst[lane] = src[lane];
  const int64_t body = (n - head) / 16;
  for (int64_t k = lane; k < body; k += 64) {
    const uint8_t *s = src + head + 16 * k;
    const uint32_t sh = (uint32_t)((uintptr_t)s & 3);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(s - sh);
    const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = sh ? q[4] : 0u;
    uint4 o;
    o.x = __builtin_amdgcn_alignbyte(w1, w0, sh);
    o.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
    o.z = __builtin_amdgcn_alignbyte(w3, w2, sh);
    o.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
    *reinterpret_cast<uint4 *>(dst + head + 16 * k) = o;
  }
  const int64_t done = head + 16 * body;
  if (lane < n - done) dst[done + lane] = src[done + lane];
}

__global__ __launch_bounds__(kThreads) void k_lift_write(ErrRecs a, const LiftRec *lr, const int64_t *cig_off, const uint32_t *cig,
                                                         const int64_t *dst, uint8_t *out, u64 *cells) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < a.n_rec; r += (int64_t)gridDim.x * kWaves) {
    const LiftRec me = lr[r];
    if (me.verdict != kLvCopy && me.verdict != kLvLift) continue;  // (wave-uniform)
    const uint64_t wd = a.rec[r];
    const uint8_t *p = a.stream + (int64_t)(wd >> kSizeBits);
    const int64_t old = 4 + (int64_t)(wd & (((uint64_t)1 << kSizeBits) - 1));
    uint8_t *o = out + dst[r];
    if (me.verdict == kLvCopy) {
      wave_copy(o, p, old, lane);
      continue;
    }
    const int64_t now = dst[r + 1] - dst[r];
    const uint32_t l_seq = ld32(p + kBamLSeq), n_cigar = ld16(p + kBamNCigarOp), l_name = p[kBamLReadName];
    const bool big = me.n_ops_out > (uint32_t)kCigarMaxOps;
    const uint32_t n_field = big ? 2u : me.n_ops_out;
    const uint8_t *my_cig = (const uint8_t *)(cig + cig_off[r]);
    // moved: pos or the CIGAR differs from the record's resolved one
    bool differs = (int64_t)me.pos != (int32_t)ld32(p + kBamPos) || me.n_ops_out != a.n_ops[r];
    if (!differs)
      for (uint32_t k = lane; k < me.n_ops_out; k += 64) differs |= ld32(a.stream + a.cig_at[r] + 4 * (int64_t)k) != ld32(my_cig + 4 * (int64_t)k);
    if (__ballot(differs) && lane == 0) atomicAdd(&cells[kLiftCellCounts + kLiftMoved], 1ull);
    // the fixed fields: block_size, pos, bin and n_cigar_op are new
    if (lane < kBamFixed) {
      uint32_t b = p[lane];
      const uint32_t bin = (uint32_t)aln_reg2bin(me.pos, (int64_t)me.pos + me.span);
      if (lane < 4) b = (uint32_t)(now - 4) >> (8 * lane);
      else if (lane >= kBamPos && lane < kBamPos + 4) b = (uint32_t)me.pos >> (8 * (lane - kBamPos));
      else if (lane >= 14 && lane < 16) b = bin >> (8 * (lane - 14));
      else if (lane >= kBamNCigarOp && lane < kBamNCigarOp + 2) b = n_field >> (8 * (lane - kBamNCigarOp));
      o[lane] = (uint8_t)b;
    }
    o += kBamFixed;
    wave_copy(o, p + kBamFixed, l_name, lane);
    o += l_name;
    if (big) {
      if (lane < 8) o[lane] = (uint8_t)((lane < 4 ? l_seq << 4 | kOpS : (uint32_t)me.span << 4 | kOpN) >> (8 * (lane & 3)));
    } else {
      wave_copy(o, my_cig, 4 * (int64_t)n_field, lane);
    }
    o += 4 * (int64_t)n_field;
    const uint8_t *seq = p + kBamFixed + l_name + 4 * (int64_t)n_cigar;
    const int64_t n_seq = ((int64_t)l_seq + 1) / 2 + l_seq;
    wave_copy(o, seq, n_seq, lane);
    o += n_seq;
    if (l_seq) {
      if (lane == 0) bam_put_int_tag((char *)o, 'N', 'M', me.nm);
      o += 3 + bam_int_size(me.nm);
    }
    if (big) {
      if (lane < 8) o[lane] = lane < 4 ? (uint8_t)"CGBI"[lane] : (uint8_t)(me.n_ops_out >> (8 * (lane - 4)));
      o += 8;
      wave_copy(o, my_cig, 4 * (int64_t)me.n_ops_out, lane);
      o += 4 * (int64_t)me.n_ops_out;
    }
    // the aux fields that stay, each stretch of them between two that go in one copy (the sizes pass has seen them whole)
    const uint8_t *aux = seq + n_seq, *end = p + old, *from = aux;
    while (aux < end) {
      const int64_t n = aux_field(aux, end);
      if (n < 0) break;
      if (aux_goes(aux)) {
        wave_copy(o, from, aux - from, lane);
        o += aux - from;
        from = aux + n;
      }
      aux += n;
    }
    wave_copy(o, from, end - from, lane);
  }
}

inline unsigned wave_blocks(int64_t n_rec) { return (unsigned)std::min<int64_t>((n_rec + kWaves - 1) / kWaves, kRecBlocksMax); }

}  // namespace

void launch_lift_kept(const int32_t *origin, int64_t n, int32_t *kept, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_lift_kept, dim3(blocks_of(n)), dim3(kThreads), 0, s, origin, n, kept);
}

hipError_t lift_max_scan(void *temp, size_t *temp_bytes, const int32_t *kept, int32_t *kept_max, int64_t n, hipStream_t s) {
  return rocprim::inclusive_scan(temp, *temp_bytes, kept, kept_max, (size_t)n, rocprim::maximum<int32_t>(), s);
}

void launch_lift_check(const int32_t *origin, const int32_t *kept_max, int64_t n, int64_t l_orig, unsigned long long *cells, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_lift_check, dim3(blocks_of(n)), dim3(kThreads), 0, s, origin, kept_max, n, l_orig, cells);
}

void launch_lift_span(ErrRecs recs, const LiftRef *refs, LiftRec *lr, unsigned long long *cells, hipStream_t s) {
  if (recs.n_rec <= 0) return;
  hipLaunchKernelGGL(k_lift_span, dim3(wave_blocks(recs.n_rec)), dim3(kThreads), 0, s, recs, refs, lr, cells);
}

void launch_lift_runs(ErrRecs recs, const LiftRef *refs, ErrGenome g, LiftRec *lr, int64_t *n_ops, const int64_t *cig_off, uint32_t *cig,
                      unsigned long long *cells, hipStream_t s) {
  if (recs.n_rec <= 0) return;
  if (cig) hipLaunchKernelGGL(k_lift_runs<true>, dim3(wave_blocks(recs.n_rec)), dim3(kThreads), 0, s, recs, refs, g, lr, n_ops, cig_off, cig, cells);
  else hipLaunchKernelGGL(k_lift_runs<false>, dim3(wave_blocks(recs.n_rec)), dim3(kThreads), 0, s, recs, refs, g, lr, n_ops, cig_off, cig, cells);
}

void launch_lift_sizes(ErrRecs recs, const LiftRec *lr, int64_t *size, unsigned long long *cells, hipStream_t s) {
  if (recs.n_rec <= 0) return;
  hipLaunchKernelGGL(k_lift_sizes, dim3(blocks_of(recs.n_rec)), dim3(kThreads), 0, s, recs, lr, size, cells);
}

void launch_lift_write(ErrRecs recs, const LiftRec *lr, const int64_t *cig_off, const uint32_t *cig, const int64_t *dst, uint8_t *out,
                       unsigned long long *cells, hipStream_t s) {
  if (recs.n_rec <= 0) return;
  hipLaunchKernelGGL(k_lift_write, dim3(wave_blocks(recs.n_rec)), dim3(kThreads), 0, s, recs, lr, cig_off, cig, dst, out, cells);
}

}  // namespace pbsim
