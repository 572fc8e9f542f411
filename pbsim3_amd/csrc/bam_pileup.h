// bam_pileup.h -- pbsim_bam_pileup (bam_pileup.cpp) in its parts.  The first half is free of HIP (bam_pileup_rule.cpp): the option
// check and the report text, so that it compiles alone; the second is the device side (bam_pileup.hip), left out where
// PBSIM_PILEUP_NO_HIP is defined.  The record classes, the references by name and the CIGAR resolution are bam_errors.h's.
// Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

// counts[] of pbsim_pileup_result: the first nine of pbsim_errors_result's
constexpr int kPileCounts = 9;
// sites[]
enum : int { kPsSites = 0, kPsRefN, kPsLow, kPsCalled, kPsConcordant, kPsSub, kPsDel, kPsIns, kPsDiscordant, kPileSites };
// the cells of a position
enum : int { kPcOther = 4, kPcDel = 5, kPcIns = 6, kPcMasked = 7, kPileWidth = 8 };
constexpr int kPileHp = 12;
constexpr int64_t kPileDefaultPiece = (int64_t)8 << 20;

// opts (nullptr: the defaults) checked and completed: piece_bytes 0 becomes the default.  false: *err says which one is bad.
bool pileup_check_opts(const pbsim_pileup_opts *opts, pbsim_pileup_opts *out, std::string *err);
// the report text (pbsim_pileup_report)
std::string pileup_report_text(const pbsim_pileup_result &r);

}  // namespace pbsim

#ifndef PBSIM_PILEUP_NO_HIP
#include <hip/hip_runtime.h>

#include "bam_errors.h"

namespace pbsim {

// the small cells the kernels add into, one behind the other in one buffer of unsigned long long
enum : int {
  kPileCellSites = 0,
  kPileCellSums = kPileCellSites + kPileSites,
  kPileCellUnanchored = kPileCellSums + kPileWidth,
  kPileCellMaxDepth,
  kPileCellHpCalled,
  kPileCellHpSub = kPileCellHpCalled + kPileHp,
  kPileCellHpDel = kPileCellHpSub + kPileHp,
  kPileCellHpIns = kPileCellHpDel + kPileHp,
  kPileCells = kPileCellHpIns + kPileHp
};

// a site's class byte: bits 0 .. 2 the class, bit 3 an ins_site, bits 4 .. 6 the call (A C G T del; kPileNoCall: none); a byte of
// the padding between genome records is kPileNoSite
enum : int { kPileRefN = 0, kPileLow, kPileMatch, kPileSub, kPileDel, kPileInsBit = 8, kPileNoCall = 7, kPileNoSite = 0xff };

// the genome's records as the site pass and the text see them: record r lies at [at[r], at[r] + len[r]) of the genome's two
// buffers, of the table (in positions) and of the class bytes; total is their size; its name is names[name_at[r], name_at[r + 1])
struct PileGenome {
  int32_t n;
  int64_t total;
  const int64_t *at, *len, *name_at;
  const char *names;
  const uint8_t *seq, *hp;
};

// the column pass over the n_seg segments: one atomic per column into table ([position][8], position as in the genome's buffers)
void launch_pileup_columns(ErrRecs r, ErrRefs refs, ErrGenome g, const ErrSegment *seg, int64_t n_seg, uint32_t min_baseq, uint32_t *table,
                           unsigned long long *cells, hipStream_t s);
// the site pass: every position's class byte, the totals into cells
void launch_pileup_sites(PileGenome g, const uint32_t *table, int64_t min_depth, uint8_t *cls, unsigned long long *cells, hipStream_t s);
// the text: the bytes of every tile of kPileTile positions into tile_len, then (tile_off: their exclusive scan) the lines
constexpr int kPileTile = 256;
void launch_pileup_text_sizes(PileGenome g, const uint32_t *table, const uint8_t *cls, int format, int64_t *tile_len, hipStream_t s);
void launch_pileup_text_fill(PileGenome g, const uint32_t *table, const uint8_t *cls, int format, const int64_t *tile_off, char *text, hipStream_t s);

}  // namespace pbsim
#endif
