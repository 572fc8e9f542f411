// genome_mutate.h -- pbsim_genome_mutate (genome_mutate.cpp) in its parts.  The first half is free of HIP (genome_mutate_rule.cpp):
// the option check, the header text and the report text, so that it compiles alone; the second is the device side
// (genome_mutate.hip), left out where PBSIM_MUTATE_NO_HIP is defined.  Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

// drawn[] and types[] of pbsim_mutate_result
enum : int { kMtSnv = 0, kMtIns, kMtDel, kMutTypes };

constexpr int64_t kMutDefaultPiece = 8 << 20;       // piece_bytes 0
constexpr int64_t kMutMaxBases = 2147483647;        // a record has fewer bases: a position is a 32-bit counter word and an int32 of the origin map

// opts (nullptr: the defaults) checked and completed: piece_bytes 0 becomes the default.  false: *err says which one is bad.
bool mutate_check_opts(const pbsim_mutate_opts *opts, pbsim_mutate_opts *out, std::string *err);
// the VCF header over the genome's n records: names[r] (ending with NUL) and the bases of each
std::string mutate_header_text(const pbsim_mutate_opts &o, const char *const *names, const int64_t *lengths, int n);
// the report text (pbsim_mutate_report)
std::string mutate_report_text(const pbsim_mutate_result &r);

}  // namespace pbsim

#ifndef PBSIM_MUTATE_NO_HIP
#include <hip/hip_runtime.h>

#include "bam_pileup.h"

namespace pbsim {

// the small cells the passes add into, one behind the other in one buffer of unsigned long long
enum : int {
  kMutCellEligible = 0,
  kMutCellDrawn,
  kMutCellVoidDel = kMutCellDrawn + kMutTypes,
  kMutCellDropped,
  kMutCellMerged,
  kMutCellSubstituted,
  kMutCellInserted,
  kMutCellDeleted,
  kMutCellBasesOut,
  kMutCellVariants,
  kMutCellTypes,
  kMutCellRefBases = kMutCellTypes + kMutTypes,
  kMutCellAltBases,
  kMutCellLongestRef,
  kMutCellLongestAlt,
  kMutCells
};

constexpr int kMutTile = kPileTile;  // positions of a tile: one workgroup's

// what the event pass leaves of every position of the genome's buffers
struct MutSites {
  uint8_t *kind;             // bits 0 .. 1: none, snv, ins, del; kMutDeleted: in the deleted set; kMutNoSite: padding
  uint16_t *len;             // an ins: its bases; a del: the positions of its run after the cut
  unsigned long long *end;   // a del: the buffer index behind its run's last position; else 0
  unsigned long long *tile;  // [tiles]: the largest end of the tile; after launch_mutate_tile_scan the largest of the tiles in front
};
constexpr uint8_t kMutKindBits = 3, kMutDeleted = 8, kMutNoSite = 0x80;

// The passes over the genome's buffers (g.hp is not read); the rule: include/pbsim3_amd.h.
//   events    : the kind, length and end of every position, every tile's largest end, the counts of the draws into cells (zeroed)
//   tile_scan : the tiles' largest ends into their exclusive max-scan, in place
//   base_sizes: the deleted set from the ends (kMutDeleted into kind), what every position emits: a tile's bases into tile_n, the
//               records' parts (as the consensus has them), the counts
//   base_fill : (tile_off: the scan of tile_n; rec complete) the FASTA into text where that is asked for, the origin map into
//               origin (one int32 per base, at base_at[r] + the base's index) where that is
//   line_sizes: every tile's VCF bytes into tile_n, the counts, every written record counted in rec_n (one per genome record, zeroed)
//   line_fill : (tile_off: the scan) the lines into text
void launch_mutate_events(PileGenome g, pbsim_mutate_opts o, MutSites s, unsigned long long *cells, hipStream_t st);
void launch_mutate_tile_scan(MutSites s, int64_t tiles, hipStream_t st);
void launch_mutate_base_sizes(PileGenome g, MutSites s, int64_t *part, int64_t *tile_n, unsigned long long *cells, hipStream_t st);
void launch_mutate_record_bases(PileGenome g, const int64_t *part, const int64_t *tile_off, int64_t *base_at, hipStream_t st);
void launch_mutate_base_fill(PileGenome g, pbsim_mutate_opts o, MutSites s, const int64_t *base_at, const int64_t *byte_at, const int64_t *tile_off,
                             char *text, int32_t *origin, hipStream_t st);
void launch_mutate_line_sizes(PileGenome g, MutSites s, int64_t *tile_n, unsigned long long *cells, unsigned long long *rec_n, hipStream_t st);
void launch_mutate_line_fill(PileGenome g, pbsim_mutate_opts o, MutSites s, const int64_t *tile_off, char *text, hipStream_t st);

}  // namespace pbsim
#endif
