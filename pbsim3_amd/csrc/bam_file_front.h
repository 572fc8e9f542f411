// bam_file_front.h -- one file's way from its bytes to the segments of its scored records, as pbsim_bam_errors, pbsim_bam_pileup
// and pbsim_bam_consensus go it, and pbsim_bam_call through the consensus stage's pile (bam_file_front.cpp): the stream into HBM
// and its records (bam_stream.cpp), the references by name with the l_ref check (bam_errors_rule.cpp), the record pass and the
// segments (bam_errors.hip).  The caller runs its column pass over them and lets the frame go.  Host code: the .hip files do not
// include this.
#pragma once
#include "bam_errors.h"
#include "bam_genome.h"
#include "bam_stream.h"
#include "ctx.h"

namespace pbsim {

struct BamFileFront {
  BamStream s;
  DevBuf d_ref_at, d_ref_len, d_rec, d_st, d_cig_at, d_n_ops, d_sums, d_nm, d_n_seg, d_col, d_scan_tmp, d_seg;
  ErrRefs er = {0, nullptr, nullptr};
  ErrRecs recs = {};
  int64_t n_rec = 0, n_seg = 0;  // n_seg > 0: d_seg holds that many ErrSegment
};

// File f of n_files: its failures name it as "file f" where there are several.  cells: the record pass's (kErrCells, the fault
// cell preset); ph gets the marks inflate, locate, records, segments.  col_counts: the records' column counts (d_col, zeroed, as
// recs.col) for a column pass that fills them -- the errors stage's alone; recs.col is nullptr without.  A file without records
// succeeds with n_rec 0 and nothing allocated.  PBSIM_FAILED: the message is set.
int bam_file_front(pbsim_ctx *c, const BamStage &stage, BamPhases &ph, const pbsim_errors_ref *refs, int n_refs, const Genome &genome,
                   const pbsim_errors_file *files, int f, int n_files, int32_t exclude_flags, int32_t min_mapq, unsigned long long *cells,
                   bool col_counts, BamFileFront *ff);

}  // namespace pbsim
