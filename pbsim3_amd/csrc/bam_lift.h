// bam_lift.h -- pbsim_bam_lift (bam_lift.cpp) in its parts.  The first half is free of HIP (bam_lift_rule.cpp): the argument
// check, the header rewritten for the original genome, and the report text, so that it compiles alone; the second is the device
// side (bam_lift.hip), left out where PBSIM_LIFT_NO_HIP is defined.  Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

// counts[] of pbsim_lift_result
enum : int { kLiftRecords = 0, kLiftUnaligned, kLiftUnsupported, kLiftUnplaced, kLiftLifted, kLiftMoved, kLiftNoSeq, kLiftLongIn, kLiftLongOut, kLiftCounts };
// totals[], over the lifted records
enum : int {
  kLiftColsIn = 0,
  kLiftColsOut,
  kLiftM,
  kLiftIns,
  kLiftDel,
  kLiftSoft,
  kLiftSub,
  kLiftGapDel,
  kLiftBasesToIns,
  kLiftDelsVanished,
  kLiftBytesIn,
  kLiftBytesOut,
  kLiftTotals
};
static_assert(sizeof(pbsim_lift_result) == (kLiftCounts + kLiftTotals) * sizeof(int64_t), "the result is its counts and its totals");

constexpr int32_t kLiftFront = INT32_MIN;  // origin[]: a base inserted in front of position 0

// the arguments that need no device: the origin maps (one per genome record, none missing, none of 2^31 - 1 bases or more), the
// file, the sink.  false: *err
bool lift_check_args(const pbsim_lift_origin *origins, int n_refs, const pbsim_errors_file *file, const pbsim_lift_sink *sink, std::string *err);
// The header of the lifted file from the inflated header bytes h[0, n) of the input (magic .. the last l_ref; parsed before):
// in the text an SO: value of a leading @HD line becomes `unsorted` and the LN: of the @SQ line whose SN: is reference k's name
// becomes new_len[k]; every l_ref of the reference list becomes new_len[k]; nothing else changes.
std::string lift_header(const uint8_t *h, int64_t n, int64_t l_text, const std::vector<std::string> &names, const std::vector<int64_t> &new_len);
// what is wrong with the origin map at a faulty position (kind: kLiftBad* below), for the failure's words
const char *lift_origin_fault(int kind);
// the report text (pbsim_lift_report)
std::string lift_report_text(const pbsim_lift_result &r);

// what the validation pass says of a variant position
enum : int { kLiftBadRange = 1, kLiftBadOrder = 2, kLiftBadAnchor = 3 };

}  // namespace pbsim

#ifndef PBSIM_LIFT_NO_HIP
#include <hip/hip_runtime.h>

#include "bam_errors.h"

namespace pbsim {

// the cells the kernels add into, one buffer of unsigned long long
enum : int {
  kLiftCellCounts = 0,
  kLiftCellTotals = kLiftCounts,
  kLiftCellFault = kLiftCellTotals + kLiftTotals,  // min(the inflated offset of a record that does not fit or has bad aux fields); preset to all ones
  kLiftCellOrigin,                                 // min(variant position << 2 | kind) of a bad origin map; preset to all ones
  kLiftCells
};

// a record's verdict
enum : uint8_t { kLvCopy = 0, kLvLift = 1, kLvUnsupported = 2, kLvUnplaced = 3 };

// what the span pass leaves per record, and the run pass completes
struct LiftRec {
  int64_t x_first, x_last;  // the input columns of the first and the last M column that stays M
  int64_t q_first, q_last;  // their query indices
  int64_t q_total;          // the query bases of the CIGAR: m + ins + soft
  int64_t span;             // M + D columns of the lifted core
  int64_t nm;               // sub + ins + del of the lifted core
  int64_t cols_in;
  uint32_t h_left, h_right;  // the H clips
  uint32_t n_core;           // the runs of the lifted core
  int32_t pos;               // the lifted pos
  uint32_t n_ops_out;        // all ops of the lifted CIGAR
  uint8_t verdict;
};

// one reference of the file: its origin map and prev_kept (the inclusive max-scan of the kept values), the variant and original
// lengths, and where the original record's prepared bases begin in the genome's buffer
struct LiftRef {
  const int32_t *origin, *kept_max;
  int64_t l_var, l_orig, at;
};

// kept[v] = origin[v] where that is >= 0, else -1: what the max-scan runs over
void launch_lift_kept(const int32_t *origin, int64_t n, int32_t *kept, hipStream_t s);
// kept_max = the inclusive max-scan of kept (rocPRIM); temp as the first call (temp nullptr) sizes it
hipError_t lift_max_scan(void *temp, size_t *temp_bytes, const int32_t *kept, int32_t *kept_max, int64_t n, hipStream_t s);
// rule 2 on one reference's map: cells[kLiftCellOrigin] = min(v << 2 | kind) over the faulty positions
void launch_lift_check(const int32_t *origin, const int32_t *kept_max, int64_t n, int64_t l_orig, unsigned long long *cells, hipStream_t s);
// one wave per record: the verdict, the first and last M column, the clips (recs: the record pass's, bam_errors.hip)
void launch_lift_span(ErrRecs recs, const LiftRef *refs, LiftRec *lr, unsigned long long *cells, hipStream_t s);
// one wave per lifted record over the columns of its core: without cig the runs are counted, the totals and NM made (lr, n_ops[r]
// for the scan); with cig (zeroed, 4 bytes per op from cig_off[r] on) the lifted CIGAR is written and `moved` counted
void launch_lift_runs(ErrRecs recs, const LiftRef *refs, ErrGenome g, LiftRec *lr, int64_t *n_ops, const int64_t *cig_off, uint32_t *cig,
                      unsigned long long *cells, hipStream_t s);
// one lane per record: the lifted record's size into size[r] (0 for a dropped one, the record's own for a copied one)
void launch_lift_sizes(ErrRecs recs, const LiftRec *lr, int64_t *size, unsigned long long *cells, hipStream_t s);
// one wave per record: the lifted record at out + dst[r]
void launch_lift_write(ErrRecs recs, const LiftRec *lr, const int64_t *cig_off, const uint32_t *cig, const int64_t *dst, uint8_t *out,
                       unsigned long long *cells, hipStream_t s);

}  // namespace pbsim
#endif
