// bam_call.h -- pbsim_bam_call (bam_call.cpp) in its parts.  The first half is free of HIP (bam_call_rule.cpp): the option
// check, the header text and the report text, so that it compiles alone; the second is the device side (bam_call.hip), left
// out where PBSIM_CALL_NO_HIP is defined.  The front half of the stage is bam_consensus.h's, bam_pileup.h's and bam_errors.h's.
// Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

// types[] of pbsim_call_result
enum : int { kCtSnv = 0, kCtIns, kCtDel, kCtComplex, kCallTypes };

// opts (nullptr: the defaults) checked and completed: piece_bytes 0 becomes the default.  false: *err says which one is bad.
bool call_check_opts(const pbsim_call_opts *opts, pbsim_call_opts *out, std::string *err);
// the VCF header over the genome's n records: names[r] (ending with NUL) and the bases of each
std::string call_header_text(const char *const *names, const int64_t *lengths, int n);
// the report text (pbsim_call_report)
std::string call_report_text(const pbsim_call_result &r);

}  // namespace pbsim

#ifndef PBSIM_CALL_NO_HIP
#include <hip/hip_runtime.h>

#include "bam_consensus.h"

namespace pbsim {

// the small cells the line pass adds into, one behind the other in one buffer of unsigned long long
enum : int {
  kCallCellVariants = 0,
  kCallCellTypes,
  kCallCellRefBases = kCallCellTypes + kCallTypes,
  kCallCellAltBases,
  kCallCellLongestRef,
  kCallCellLongestAlt,
  kCallCellUnplacedRecords,
  kCallCellUnplacedSites,
  kCallCells
};

constexpr int kCallTile = kConsTile;

// The line pass over the groups (the rule: include/pbsim3_amd.h), after launch_consensus_base_sizes has left the emitted lengths
// in slots.len.  sizes: every tile's bytes into tile_n, the counts into cells (zeroed), every written record counted in rec_n
// (one per genome record, zeroed).  fill (tile_off: the exclusive scan of tile_n): the lines into text.
void launch_call_line_sizes(PileGenome g, const uint32_t *table, const uint8_t *cls, ConsSlots slots, int64_t *tile_n, unsigned long long *cells,
                            unsigned long long *rec_n, hipStream_t s);
void launch_call_line_fill(PileGenome g, const uint32_t *table, const uint8_t *cls, ConsSlots slots, const int64_t *tile_off, char *text, hipStream_t s);

}  // namespace pbsim
#endif
