// bam_stats.h -- pbsim_bam_stats (bam_stats.cpp) in its parts.  The first half is free of HIP (bam_stats_rule.cpp): the option
// check, the table E of the fixed-point error probabilities, the arithmetic that needs more than 64 bits and the report text,
// so that it compiles alone; the second is the device side (bam_stats.hip), left out where PBSIM_STATS_NO_HIP is defined.
// Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

// counts[] of pbsim_bam_stats
enum : int {
  kStatsRecords = 0,
  kStatsSkippedFlag,
  kStatsUnaligned,
  kStatsSkippedMapq,
  kStatsAligned,
  kStatsNoSeq,
  kStatsNoQual,
  kStatsNoNm,
  kStatsNmBad,
  kStatsScored,
  kStatsCounts
};
// len_row[]: n, bases, min, max, mean_milli, sd, median, N10 .. N90
enum : int { kStatsLenN = 0, kStatsLenBases, kStatsLenMin, kStatsLenMax, kStatsLenMean, kStatsLenSd, kStatsLenMedian, kStatsLenN10, kStatsLenRow = 16 };
// totals[]
enum : int {
  kStatsCols = 0,
  kStatsSub,
  kStatsIns,
  kStatsDel,
  kStatsInsEvents,
  kStatsDelEvents,
  kStatsSoft,
  kStatsHard,
  kStatsIdentitySum,
  kStatsAccSum,
  kStatsAccReads,
  kStatsQSum,
  kStatsTotals
};
constexpr int kStatsQBins = 128, kStatsPpmBins = 1001;
constexpr int64_t kStatsDefaultPiece = (int64_t)8 << 20;

// E[q] = round(2^32 10^(-q/10)), q = 0 .. 127
extern const uint64_t kStatsE[kStatsQBins];

// opts (nullptr: the defaults) checked and completed: piece_bytes 0 becomes the default.  false: *err says which one is bad.
bool stats_check_opts(const pbsim_stats_opts *opts, pbsim_stats_opts *out, std::string *err);

// isqrt((n sumsq - bases^2) / n^2), sumsq = sq_lo + sq_hi 2^32 (the sums of the low and of the high 32 bits of every length's
// square), in 128-bit arithmetic; 0 where n == 0
int64_t stats_length_sd(uint64_t n, uint64_t bases, uint64_t sq_lo, uint64_t sq_hi);

// floor(a * m / b), b >= 1, in 128-bit arithmetic (the caller knows that the quotient fits)
int64_t stats_muldiv(uint64_t a, uint64_t m, uint64_t b);

// the report text (pbsim_stats_report)
std::string stats_report_text(const int64_t counts[kStatsCounts], const int64_t len_row[kStatsLenRow], const int64_t totals[kStatsTotals],
                              const int64_t hist_q[kStatsQBins], const int64_t hist_identity[kStatsPpmBins],
                              const int64_t hist_qacc[kStatsPpmBins]);

}  // namespace pbsim

#ifndef PBSIM_STATS_NO_HIP
#include <hip/hip_runtime.h>

#include "bam_chain.h"

namespace pbsim {

// bytes of quality one workgroup of the quality pass takes (256 lanes x 64 bytes), cut from the counted records' quality
// fields laid end to end
constexpr int kStatsTile = 16384;

// the small cells the kernels add into, one behind the other in one buffer of unsigned long long
enum : int {
  kStatsCellCounts = 0,
  kStatsCellFault = kStatsCellCounts + kStatsCounts,  // min(the inflated offset of a malformed record); preset to all ones
  kStatsCellLenN,
  kStatsCellLenBases,
  kStatsCellLenMin,  // preset to all ones
  kStatsCellLenMax,
  kStatsCellSqLo,  // the sum of the low 32 bits of l_seq^2
  kStatsCellSqHi,  // the sum of the high 32 bits
  kStatsCellTotals,
  kStatsCellHistQ = kStatsCellTotals + kStatsTotals,
  kStatsCellHistIdentity = kStatsCellHistQ + kStatsQBins,
  kStatsCellHistQacc = kStatsCellHistIdentity + kStatsPpmBins,
  kStatsCells = kStatsCellHistQacc + kStatsPpmBins
};

// what the record pass leaves per record in st[]
enum : int { kStCounted = 1, kStAligned = 2, kStQual = 4, kStNm = 8, kStScored = 16 };

// one file's per-record arrays (n_rec entries each unless said otherwise)
struct StatsRecs {
  const uint8_t *stream;
  const uint64_t *rec;  // packed as kBamSamplePacking
  int64_t n_rec;
  uint8_t *st;
  int64_t *qoff;             // where the record's quality field begins in the stream
  int64_t *qlen;             // [n_rec + 1]: its length where the record takes part in the quality pass, else 0; then their exclusive scan
  unsigned long long *qsum;  // [2 n_rec]: esum and the sum of q', zeroed
  uint32_t *length;          // l_seq of a counted record with l_seq >= 1, else 0
  int64_t *cig;              // [4 n_rec]: cols, ins, del, soft of an aligned record; nullptr without text
  int64_t *nm;               // the NM value of an aligned record that has one; nullptr without text
};

// the record pass: classes, CIGAR sums, NM, the counts, the length cells, the totals and the identity histogram
void launch_stats_records(StatsRecs r, int32_t exclude_flags, int32_t min_mapq, unsigned long long *cells, hipStream_t s);
// the quality pass over the n_bytes quality bytes (qlen scanned): hist_q, and per record esum and the sum of q'
void launch_stats_quals(StatsRecs r, int64_t n_bytes, const unsigned long long *e_table, unsigned long long *cells, hipStream_t s);
// per record with qualities: acc_ppm, its histogram and the three quality totals
void launch_stats_reads(StatsRecs r, unsigned long long *cells, hipStream_t s);
// the lines' lengths into len[0, n_rec) (0 for a record that is not counted), then (off: their exclusive scan) the lines
void launch_stats_line_sizes(StatsRecs r, int64_t *len, hipStream_t s);
void launch_stats_line_fill(StatsRecs r, const int64_t *off, char *text, hipStream_t s);
// the lengths: sorted ascending, their running sums, and median and N10 .. N90 into out[0, 10)
hipError_t stats_sort_lengths(void *tmp, size_t *tmp_bytes, const uint32_t *in, uint32_t *out, int64_t n, hipStream_t s);
hipError_t stats_scan_lengths(void *tmp, size_t *tmp_bytes, const uint32_t *sorted, unsigned long long *sums, int64_t n, hipStream_t s);
void launch_stats_nx(const uint32_t *sorted, const unsigned long long *sums, int64_t n_all, int64_t n, unsigned long long bases, int64_t *out,
                     hipStream_t s);

}  // namespace pbsim
#endif
