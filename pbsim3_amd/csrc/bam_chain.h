// bam_chain.h -- what the sampling method's BAM input (sample_bam.hip, sample_profile.cpp) decides on the host, free of HIP so
// that it compiles alone: the header up to the first record, and the walk along block_size over the candidates of the
// parallel scan -- the one place that says what a record is.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace pbsim {

// block_size of a record at most (HiFi kinetics tags make records of several megabytes; nothing real comes near this)
constexpr int64_t kBamMaxBlock = (int64_t)64 << 20;
// a candidate / a record: (byte offset in the window's buffer << kSbSizeBits) | block_size
constexpr int kSbSizeBits = 28;
constexpr uint64_t kSbSizeMask = ((uint64_t)1 << kSbSizeBits) - 1;
static_assert((uint64_t)kBamMaxBlock <= kSbSizeMask, "block_size fits its bits");

// The header of the n-byte stream h, of which `have` bytes are there: magic, l_text, text, n_ref, the references (l_name,
// name, l_ref).  1: parsed (*n_ref, *first_record = the offset behind the reference list); 0: `have` bytes are not enough
// (more of the stream exists); -1: the header overruns the stream (or a length in it is negative); -2: no BAM\1 magic
int bam_parse_header(const uint8_t *h, int64_t have, int64_t n, int64_t *n_ref, int64_t *first_record);

enum BamChainEnd {
  kBamChainDone = 0,       // the last record ends where the bytes end
  kBamChainCarry = 1,      // the bytes from *stop on are the beginning of a record that the next window completes
  kBamChainMalformed = -1  // no record can start at *stop
};
// The chain from offset `from` of a buffer of `end` bytes: a step must land on a candidate (ascending, packed as above), the
// next one lies 4 + block_size further.  Appends the records to *rec and stops where no candidate is (*stop).  A true record
// that lies inside the bytes always is a candidate, so behind the last window (`last`), or with 4 + kBamMaxBlock bytes
// behind *stop, a missing candidate is a malformed record -- never a reason to look for the next plausible one.
BamChainEnd bam_walk_chain(const uint64_t *hits, size_t n_hits, int64_t from, int64_t end, bool last, std::vector<uint64_t> *rec,
                           int64_t *stop);

}  // namespace pbsim
