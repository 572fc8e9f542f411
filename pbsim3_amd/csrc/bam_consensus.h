// bam_consensus.h -- pbsim_bam_consensus (bam_consensus.cpp) in its parts.  The first half is free of HIP
// (bam_consensus_rule.cpp): the option check and the report text, so that it compiles alone; the second is the device side
// (bam_consensus.hip), left out where PBSIM_CONSENSUS_NO_HIP is defined.  The front half of the stage is bam_pileup.h's and
// bam_errors.h's.  Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

// bases[] of pbsim_consensus_result
enum : int { kCbOut = 0, kCbKept, kCbSub, kCbIns, kCbFill, kCbDel, kConsBases };
constexpr int kConsLenBins = 64;
constexpr int32_t kConsMaxIns = 65535, kConsMaxWidth = 1 << 20;

// opts (nullptr: the defaults) checked and completed: piece_bytes 0 becomes the default.  false: *err says which one is bad.
bool consensus_check_opts(const pbsim_consensus_opts *opts, pbsim_consensus_opts *out, std::string *err);
// the report text (pbsim_consensus_report)
std::string consensus_report_text(const pbsim_consensus_result &r);

}  // namespace pbsim

#ifndef PBSIM_CONSENSUS_NO_HIP
#include <hip/hip_runtime.h>

#include "bam_pileup.h"

namespace pbsim {

// the small cells the base pass adds into, one behind the other in one buffer of unsigned long long
enum : int {
  kConsCellBases = 0,
  kConsCellInsSites = kConsCellBases + kConsBases,
  kConsCellLongest,
  kConsCellCapped,
  kConsCellInsLen,
  kConsCells = kConsCellInsLen + kConsLenBins
};

// The inserted bases of the anchored I ops, as the column pass logs them (bam_pileup_walk.h's InsLog): *count entries were asked
// for, those below cap are there.
struct ConsLog {
  unsigned long long *entry, *count;
  int64_t cap;
};
// The ins_sites in ascending order of their place in the genome's buffers, n of them: pos[k]; len[k] the longest insertion
// logged there (then, after the base pass, the length emitted); off[k] the exclusive scan of the logged lengths: slot k's cells
// are cell[(off[k] + j) * 5 + class].
struct ConsSlots {
  int64_t n;
  const int64_t *pos;
  int64_t *len;
  const int64_t *off;
  uint32_t *cell;
};
// what the base pass knows of the genome's records beside PileGenome: the first base of record r in the count over all
// positions (base_at[r], from part[r] and the tiles' scan) and the first byte of its text
struct ConsRecords {
  int64_t *part;           // [n]: the bases in front of the record's first position inside that position's tile
  const int64_t *base_at;  // [n + 1]
  const int64_t *byte_at;  // [n]
};

constexpr int kConsTile = kPileTile;

// the slot of the ins_site at place i, -1 where it is none
__device__ __forceinline__ int64_t slot_of(const ConsSlots &s, int64_t i) {
  int64_t lo = 0, hi = s.n;  // the first slot whose place is not below i
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (s.pos[mid] < i) lo = mid + 1;
    else hi = mid;
  }
  return lo < s.n && s.pos[lo] == i ? lo : -1;
}

// the base an insertion has at one offset: the largest of the A C G T cells, among equals the first; N where all four are 0
__device__ __forceinline__ char ins_base(const uint32_t *c) {
  uint32_t best = c[0], call = 0;
#pragma unroll
  for (uint32_t k = 1; k < 4; k++)
    if (c[k] > best) best = c[k], call = k;
  return best == 0 ? 'N' : "ACGT"[call];
}

// *out (zeroed) += the inserted bases of the file's scored records: the most entries its log can get
void launch_consensus_log_size(ErrRecs r, unsigned long long *out, hipStream_t s);
// the column pass with the log (the kernel is bam_pileup_walk.h's)
void launch_consensus_columns(ErrRecs r, ErrRefs refs, ErrGenome g, const ErrSegment *seg, int64_t n_seg, uint32_t min_baseq, uint32_t *table,
                              unsigned long long *cells, ConsLog log, uint32_t max_ins, hipStream_t s);
// the ins_sites of every tile of kConsTile positions into tile_n; then (tile_off: their exclusive scan) their places into pos
void launch_consensus_slot_sizes(PileGenome g, const uint8_t *cls, int64_t *tile_n, hipStream_t s);
void launch_consensus_slot_fill(PileGenome g, const uint8_t *cls, const int64_t *tile_off, int64_t *pos, hipStream_t s);
// over n entries of a log: the longest insertion at every slot (len zeroed before the first log); then the cells' tally
void launch_consensus_lengths(ConsLog log, int64_t n, int64_t total, const uint8_t *cls, ConsSlots slots, hipStream_t s);
void launch_consensus_tally(ConsLog log, int64_t n, int64_t total, const uint8_t *cls, ConsSlots slots, hipStream_t s);
// the base pass: what every position emits, the counts into cells, a tile's bases into tile_n, the emitted lengths into
// slots.len and the records' parts; then (tile_off: the scan) base_at[0 .. n] from the parts; then (rec complete) the FASTA
void launch_consensus_base_sizes(PileGenome g, const uint32_t *table, const uint8_t *cls, ConsSlots slots, uint32_t max_ins, ConsRecords rec,
                                 int64_t *tile_n, unsigned long long *cells, hipStream_t s);
void launch_consensus_record_bases(PileGenome g, const int64_t *part, const int64_t *tile_off, int64_t *base_at, hipStream_t s);
void launch_consensus_base_fill(PileGenome g, const uint8_t *cls, ConsSlots slots, int fill, int64_t line_width, ConsRecords rec,
                                const int64_t *tile_off, char *text, hipStream_t s);

}  // namespace pbsim
#endif
