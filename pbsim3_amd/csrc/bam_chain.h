// bam_chain.h -- what the host decides about a BAM stream in HBM, for the truth-BAM sort (bam_sort.cpp) and the sampling
// method's BAM input (sample_profile.cpp) alike, free of HIP so that it compiles alone: the header up to the first record, and
// the walk along block_size over the candidates of the parallel scan (bam_scan.hip) -- the one place that says what a record is.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace pbsim {

// A candidate / a record in one word: (byte offset << size_bits) | block_size, block_size <= max_block.
struct BamPacking {
  int size_bits;
  int64_t max_block;
  constexpr uint64_t mask() const { return ((uint64_t)1 << size_bits) - 1; }
  constexpr uint64_t pack(int64_t offset, uint32_t block_size) const { return (uint64_t)offset << size_bits | block_size; }
  constexpr int64_t offset(uint64_t x) const { return (int64_t)(x >> size_bits); }
  constexpr int64_t size(uint64_t x) const { return (int64_t)(x & mask()); }
};
// Two packings, deliberately.  The sort holds a whole file in HBM, and 288 GB of it are more than 2^36 bytes: it needs 40
// offset bits, so it has 24 for the size and refuses a record of 2^24 bytes or more (a 1 000 000-base read with a run per
// column stays below 7 MB).  The sampling input packs offsets into a window's buffer, reads other people's files (HiFi kinetics
// tags make records of several megabytes; nothing real comes near 64 MiB) and so takes 28 size bits.  Giving the sort the
// larger cap would change what it accepts.
constexpr BamPacking kBamSortPacking{24, ((int64_t)1 << 24) - 1};
constexpr BamPacking kBamSamplePacking{28, (int64_t)64 << 20};
static_assert((uint64_t)kBamSortPacking.max_block <= kBamSortPacking.mask(), "block_size fits its bits");
static_assert((uint64_t)kBamSamplePacking.max_block <= kBamSamplePacking.mask(), "block_size fits its bits");

// why a stream is no BAM header, in the order the checks come
enum BamHeaderFault {
  kBamHeaderGood = 0,
  kBamHeaderShort,  // fewer than 12 bytes
  kBamHeaderMagic,  // no BAM\1
  kBamHeaderText,   // l_text is negative or runs past the end
  kBamHeaderNRef,   // n_ref is negative
  kBamHeaderRefs    // the reference list runs past the end (or an l_name is negative)
};
struct BamHeader {
  int64_t l_text = 0, n_ref = 0, first_record = 0;  // first_record: the offset behind the reference list
  std::vector<int64_t> ref_len;                     // with `want_ref_len` only
  bool empty_name = false;                          // some l_name is 0 (not even the NUL): the sort refuses that, the sampling input does not
  BamHeaderFault fault = kBamHeaderGood;            // set with every negative return
};
// The header of the n-byte stream h, of which `have` bytes are there: magic, l_text, text, n_ref, the references (l_name,
// name, l_ref).  1: parsed (*out); 0: `have` bytes are not enough (more of the stream exists; *out untouched); -1: the header
// overruns the stream (or a length in it is negative); -2: no BAM\1 magic (both: only out->fault is written).  Without
// `want_ref_len` the last reference's l_name is the last byte looked at; with it every l_ref must be there too.
int bam_parse_header(const uint8_t *h, int64_t have, int64_t n, bool want_ref_len, BamHeader *out);

enum BamChainEnd {
  kBamChainDone = 0,       // the last record ends where the bytes end
  kBamChainCarry = 1,      // the bytes from *stop on are the beginning of a record that the next window completes
  kBamChainMalformed = -1  // no record can start at *stop
};
// The chain from offset `from` of a buffer of `end` bytes: a step must land on a candidate (ascending, packed as `pk` says), the
// next one lies 4 + block_size further.  Appends the records to *rec and stops where no candidate is (*stop; rec->back() is
// then the record whose block_size led there).  A true record that lies inside the bytes always is a candidate, so behind the
// last window (`last`), or with 4 + pk.max_block bytes behind *stop, a missing candidate is a malformed record -- never a
// reason to look for the next plausible one.
BamChainEnd bam_walk_chain(BamPacking pk, const uint64_t *hits, size_t n_hits, int64_t from, int64_t end, bool last,
                           std::vector<uint64_t> *rec, int64_t *stop);

}  // namespace pbsim
