// bam_errors.h -- pbsim_bam_errors (bam_errors.cpp) in its parts.  The first half is free of HIP (bam_errors_rule.cpp): the option
// check, the genome's names, the references looked up by name, the fit of the homopolymer deletion bias at 128 bits and the
// report text, so that it compiles alone; the second is the device side (bam_errors.hip), left out where PBSIM_ERRORS_NO_HIP is
// defined.  Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

// counts[] of pbsim_errors_result
enum : int {
  kErrRecords = 0,
  kErrSkippedFlag,
  kErrUnaligned,
  kErrSkippedMapq,
  kErrSkippedRef,
  kErrAligned,
  kErrNoSeq,
  kErrMisfit,
  kErrScored,
  kErrNoNm,
  kErrNmUnchecked,
  kErrNmAgree,
  kErrNmDiffer,
  kErrWithQual,
  kErrCounts
};
// totals[]
enum : int {
  kErrCols = 0,
  kErrMatch,
  kErrSub,
  kErrAmbiguous,
  kErrIns,
  kErrDel,
  kErrInsEvents,
  kErrDelEvents,
  kErrSoft,
  kErrHard,
  kErrIdentitySum,
  kErrTotals
};
constexpr int kErrPair = 25, kErrHp = 12, kErrLenBins = 64, kErrBases = 5, kErrQBins = 128, kErrPpmBins = 1001;
constexpr int64_t kErrDefaultPiece = (int64_t)8 << 20;

// A scored record is cut into segments for the column pass: a segment lies inside one block of kErrSegOps consecutive ops and
// holds at most kErrSegCols of the block's columns (a long op is cut inside).
constexpr int kErrSegOps = 512;
constexpr int kErrSegCols = 4096;
static_assert(kErrSegOps % 64 == 0, "the column pass takes a block's ops 64 a round");

// opts (nullptr: the defaults) checked and completed: piece_bytes 0 becomes the default.  false: *err says which one is bad.
bool errors_check_opts(const pbsim_errors_opts *opts, pbsim_errors_opts *out, std::string *err);
// the genome's names: none missing, no two equal.  false: *err
bool errors_check_genome(const pbsim_errors_ref *refs, int n_refs, std::string *err);
// One file's references looked up in the genome by name (over: the name its only reference goes by, or nullptr): map[r] = the
// genome's record, or -1.  false: *err (a name given to a file that has not exactly one reference; what: "file 2")
bool errors_ref_map(const pbsim_errors_ref *refs, int n_refs, const std::vector<std::string> &file_names, const char *over,
                    const std::string &what, std::vector<int32_t> *map, std::string *err);
// fit_ok, fit_bias_milli, fit_suggest_milli from hp_cols and hp_del
void errors_fit(pbsim_errors_result *r);
// the report text (pbsim_errors_report)
std::string errors_report_text(const pbsim_errors_result &r);

}  // namespace pbsim

#ifndef PBSIM_ERRORS_NO_HIP
#include <hip/hip_runtime.h>

#include "bam_chain.h"

namespace pbsim {

// the small cells the kernels add into, one behind the other in one buffer of unsigned long long
enum : int {
  kErrCellCounts = 0,
  kErrCellFault = kErrCellCounts + kErrCounts,  // min(the inflated offset of a malformed record); preset to all ones
  kErrCellTotals,
  kErrCellPair = kErrCellTotals + kErrTotals,
  kErrCellHpCols = kErrCellPair + kErrPair,
  kErrCellHpSub = kErrCellHpCols + kErrHp,
  kErrCellHpDel = kErrCellHpSub + kErrHp,
  kErrCellInsLen = kErrCellHpDel + kErrHp,
  kErrCellDelLen = kErrCellInsLen + kErrLenBins,
  kErrCellInsBase = kErrCellDelLen + kErrLenBins,
  kErrCellDelBase = kErrCellInsBase + kErrBases,
  kErrCellQcal = kErrCellDelBase + kErrBases,
  kErrCellHistIdentity = kErrCellQcal + 3 * kErrQBins,
  kErrCells = kErrCellHistIdentity + kErrPpmBins
};

// what the record pass leaves per record in st[]
enum : int { kEsAligned = 1, kEsScored = 2, kEsNoSeq = 4, kEsNm = 8, kEsQual = 16 };

// the genome in HBM: every record's prepared bases and class bytes at the same offset of two buffers
struct ErrGenome {
  const uint8_t *seq, *hp;
};
// one file's references: where the genome's record of reference r begins (-1: the genome lacks it), and its l_ref
struct ErrRefs {
  int32_t n_ref;
  const int64_t *at;
  const int64_t *l_ref;
};

// where a segment of the column pass begins: the block of ops it lies in, the reference and query positions at the block's
// first op, and the first of its columns, counted from the block's first column
struct ErrSegment {
  uint32_t rec, op0;
  int64_t ref_pos, query_pos, col0;
};

// one file's per-record arrays (n_rec entries each unless said otherwise)
struct ErrRecs {
  const uint8_t *stream;
  const uint64_t *rec;  // packed as kBamSamplePacking
  int64_t n_rec;
  uint8_t *st;
  int64_t *cig_at;          // an aligned record's resolved CIGAR: where its ops begin in the stream
  uint32_t *n_ops;          //                                     and how many
  int64_t *sums;            // [4 n_rec]: m, ins, del, soft of an aligned record
  int64_t *nm;              // the NM value where st has kEsNm
  int64_t *n_seg;           // [n_rec + 1]: a scored record's segments; then their exclusive scan
  unsigned long long *col;  // [3 n_rec]: match, sub, ambiguous of a scored record, zeroed
};

// the record pass: classes, the resolved CIGAR and its sums, NM, the segments' count; with seg the segments themselves (n_seg
// scanned), and nothing is counted again
void launch_errors_records(ErrRecs r, ErrRefs refs, int32_t exclude_flags, int32_t min_mapq, ErrSegment *seg, unsigned long long *cells,
                           hipStream_t s);
// the column pass over the n_seg segments
void launch_errors_columns(ErrRecs r, ErrRefs refs, ErrGenome g, const ErrSegment *seg, int64_t n_seg, unsigned long long *cells, hipStream_t s);
// per scored record: identity, the NM classes, the totals of the columns
void launch_errors_reads(ErrRecs r, unsigned long long *cells, hipStream_t s);
// the lines' lengths into len[0, n_rec) (0 for a record that has no line), then (off: their exclusive scan) the lines
void launch_errors_line_sizes(ErrRecs r, int64_t *len, hipStream_t s);
void launch_errors_line_fill(ErrRecs r, const int64_t *off, char *text, hipStream_t s);

}  // namespace pbsim
#endif
