// bam_genome.h -- what the stages that hold a genome in HBM beside a BAM's records share (pbsim_bam_errors, pbsim_bam_pileup): the
// genome squeezed and prepared record by record, and the way of text made on the device to a sink, through two pinned pieces
// (bam_genome.cpp).  Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <deque>
#include <vector>

#include "../../include/pbsim3_amd.h"
#include "bam_stream.h"
#include "ctx.h"

namespace pbsim {

struct Genome {
  DevBuf seq, hp;
  std::vector<int64_t> at, len;  // where each record begins in both buffers (a multiple of 64); its bases
  int64_t total = 0;             // the bytes of each buffer: every record's bases rounded up to 64, and 64 behind them
};

// every record's lines into HBM, squeezed to its bases and prepared on its own: 64 zero bytes lie behind each, which the
// preparation's sixteen-byte loads need and which keep a run from reaching the next record
int load_genome(pbsim_ctx *c, const BamStage &stage, const pbsim_errors_ref *refs, int n_refs, Genome *g);

struct FileText {
  DevBuf d;
  int64_t n = 0;
};

// the texts, one behind the other, through two pinned pieces: one on its way to the host while the sink has the other.  A piece
// does not cross from one text into the next one's buffer, so it may be shorter than piece_bytes there.
int deliver_text(hipStream_t st, const BamStage &stage, std::deque<FileText> &texts, int64_t n_text, int64_t piece_bytes,
                 int (*on_text)(void *user, const char *bytes, int64_t n, int64_t offset), void *user);

}  // namespace pbsim
