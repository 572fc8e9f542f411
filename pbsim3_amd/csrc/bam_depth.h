// bam_depth.h -- pbsim_bam_depth (bam_depth.cpp) in its parts.  The first half is free of HIP (bam_depth_rule.cpp): the option
// check, the offset table of the references and the report text, so that it compiles alone; the second is the device side
// (bam_depth.hip), left out where PBSIM_DEPTH_NO_HIP is defined.  Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

// counts[] of pbsim_bam_depth
enum : int { kDepthRecords = 0, kDepthCounted, kDepthSkippedFlag, kDepthSkippedUnplaced, kDepthSkippedMapq, kDepthClipped, kDepthCounts };
constexpr int64_t kDepthDefaultPiece = (int64_t)8 << 20;

// opts (nullptr: the defaults) checked and completed: piece_bytes 0 becomes the default.  false: *err says which one is bad.
bool depth_check_opts(const pbsim_depth_opts *opts, pbsim_depth_opts *out, std::string *err);

// Where each reference's slots begin in the difference array: l_ref + 1 slots each, so that an end at l_ref has a place;
// off[n_ref] is the number of slots.  With window >= 1, win[r] is the number of reference r's first window among all windows
// (win[n_ref]: how many there are); with window 0, win stays empty.  false: a negative l_ref (*err).
bool depth_ref_offsets(const std::vector<int64_t> &ref_len, int64_t window, std::vector<int64_t> *off, std::vector<int64_t> *win,
                       std::string *err);

// floor(sum * 1000 / len) without leaving 64 bits: sum may be 2^62
inline int64_t depth_mean_milli(int64_t sum, int64_t len) { return sum / len * 1000 + sum % len * 1000 / len; }

// the report text (pbsim_depth_report); rows: n_ref x 4 (l_ref, covered, sum, max)
std::string depth_report_text(const int64_t counts[kDepthCounts], int32_t n_ref, const char *const *names, const int64_t *rows,
                              const int64_t hist[256]);

}  // namespace pbsim

#ifndef PBSIM_DEPTH_NO_HIP
#include <hip/hip_runtime.h>

#include "bam_chain.h"

namespace pbsim {

// reference positions one workgroup of the runs pass takes (256 lanes x 16 slots)
constexpr int kDepthTile = 4096;

// the small cells the kernels add into, one behind the other in one buffer of unsigned long long
enum : int { kDepthCellCounts = 0, kDepthCellFault = 6, kDepthCellHist = 7, kDepthCells = 7 + 256 };

struct DepthRefs {
  int32_t n_ref;
  const int64_t *off;      // [n_ref + 1] (depth_ref_offsets)
  const int64_t *win;      // [n_ref + 1], window format only
  const int64_t *name_at;  // [n_ref + 1]: the names one behind the other in `names`
  const char *names;
};

// Per record of the stream (rec packed as pk): its skip class, its CIGAR (the CG tag's where the field is the placeholder),
// and +1 / -1 into diff at the ends of each maximal covered interval, clipped to the reference.  cells[0..6) += the counts;
// cells[kDepthCellFault] = min(the inflated offset of a malformed record) (preset to all ones).
void launch_depth_events(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, BamPacking pk, DepthRefs refs, int32_t exclude_flags,
                         int32_t min_mapq, int32_t count_deletions, int32_t *diff, unsigned long long *cells, hipStream_t s);
// diff[0, n) -> its inclusive prefix sums, in place: tmp == nullptr asks for *tmp_bytes
hipError_t depth_scan(void *tmp, size_t *tmp_bytes, int32_t *diff, int64_t n, hipStream_t s);
// One pass over the depths, in tiles of kDepthTile slots.  Without `runs`: cells[kDepthCellHist..) += the histogram, per
// reference covered / sum / max into ref_stat[3 r ..], tile_runs[tile] = the run starts in the tile (window == 0), or
// win_sum[window] += the depths (window >= 1).  With `runs` (window == 0, tile_runs scanned exclusively): run k's reference,
// start and depth into run_ref, run_start, run_depth.
void launch_depth_runs(const int32_t *depth, int64_t n_slots, DepthRefs refs, int64_t window, unsigned long long *cells,
                       unsigned long long *ref_stat, int64_t *tile_runs, unsigned long long *win_sum, bool runs, int32_t *run_ref,
                       int32_t *run_start, int32_t *run_depth, hipStream_t s);
// the lines' lengths into len[0, n_lines), then (off: their exclusive scan) the lines themselves into text.  bedgraph
// (window == 0): line k is run k; window: line k is window k.
void launch_depth_line_sizes(int64_t n_lines, DepthRefs refs, int64_t window, const int32_t *run_ref, const int32_t *run_start,
                             const int32_t *run_depth, const unsigned long long *win_sum, int64_t *len, hipStream_t s);
void launch_depth_line_fill(int64_t n_lines, DepthRefs refs, int64_t window, const int32_t *run_ref, const int32_t *run_start,
                            const int32_t *run_depth, const unsigned long long *win_sum, const int64_t *off, char *text, hipStream_t s);

}  // namespace pbsim
#endif
