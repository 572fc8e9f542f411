// bam_consensus_front.h -- the way of pbsim_bam_consensus from its arguments to the end of its base pass's first half, as
// pbsim_bam_call goes it too (bam_consensus.cpp): the genome into HBM, per file the pileup's front half and the column pass with
// its log, the site pass, the ins_sites' slots with their tallied cells, and launch_consensus_base_sizes, after which slots.len
// holds the emitted lengths.  What it leaves in HBM lives as long as the ConsFront.  Host code: the .hip files do not include this.
#pragma once
#include <string>
#include <vector>

#include "bam_consensus.h"
#include "bam_genome.h"
#include "bam_stream.h"
#include "ctx.h"

namespace pbsim {

struct ConsFront {
  Genome genome;
  DevBuf d_table, d_cls, d_cells, d_pile, d_cons;          // the cells, the class bytes, the record / site / base counts
  DevBuf d_at, d_len, d_name_at, d_names;                  // pg's arrays
  DevBuf d_tile, d_scan_tmp;                               // (tiles + 1) values: the base pass's bases per tile; a scan's scratch over them
  DevBuf d_pos, d_slot_len, d_slot_off, d_slot_cell;       // slots' arrays
  DevBuf d_part, d_base_at, d_byte_at;                     // rec's arrays
  std::string names;
  std::vector<int64_t> name_at;
  PileGenome pg = {};
  ConsSlots slots = {0, nullptr, nullptr, nullptr, nullptr};
  ConsRecords rec = {nullptr, nullptr, nullptr};
  int64_t tiles = 0, n_cells = 0;
  int64_t n_all = 0, inflated = 0, segments = 0, logged = 0;  // records, inflated bytes, segments and log entries over all files
};

// ph gets the marks genome, zero, per file the front's and columns, then sites, slots, lengths, tally.  The base sizes are
// launched and not yet marked; the stream is not synchronised behind them.  PBSIM_FAILED: the message is set.
int consensus_front(pbsim_ctx *c, const BamStage &stage, BamPhases &ph, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files,
                    int n_files, int32_t exclude_flags, int32_t min_mapq, int32_t min_baseq, int64_t min_depth, int32_t max_ins, ConsFront *out);

}  // namespace pbsim
