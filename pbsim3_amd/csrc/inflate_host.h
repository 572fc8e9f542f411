// inflate_host.h -- BGZF input (inflate_host.cpp): the member index the host reads from the headers alone, and the GPU
// inflate of the indexed members (inflate.hip).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

struct BgzfMember {
  int64_t offset;    // of the member's first byte in the file
  int64_t data;      // of its deflate data
  int64_t out_off;   // of its bytes in the inflated file (exclusive prefix sum of ISIZE)
  int32_t data_len;  // deflate bytes (the member less header and trailer)
  int32_t isize;
  uint32_t crc;
};
// false: not BGZF -- a member without the 'BC' subfield, or framing that runs past the end or breaks off (SAMv1 4.1)
bool bgzf_index(const uint8_t *p, int64_t n, std::vector<BgzfMember> *out);
int64_t bgzf_inflated_size(const std::vector<BgzfMember> &mem);
// the indexed members of src -> dst (bgzf_inflated_size bytes), on the context's GPU; PBSIM_FAILED with
// "gzip member at byte offset N: <reason>" for the first member that is not good.  dst_on_device: dst is memory of that
// GPU and the inflated bytes never leave it (the sample FASTQ of sample_profile.cpp)
int inflate_members(pbsim_ctx *c, const uint8_t *src, const std::vector<BgzfMember> &mem, uint8_t *dst, bool dst_on_device = false);

}  // namespace pbsim
