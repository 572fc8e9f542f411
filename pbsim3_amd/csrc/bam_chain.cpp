// bam_chain.cpp -- see bam_chain.h
#include "bam_chain.h"

#include <string.h>

namespace pbsim {

namespace {
inline int64_t le32s(const uint8_t *p) {
  return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}
}  // namespace

int bam_parse_header(const uint8_t *h, int64_t have, int64_t n, int64_t *n_ref, int64_t *first_record) {
  if (have > n) have = n;
  if (n < 4) return have < n ? 0 : (n > 0 && memcmp(h, "BAM\1", (size_t)n) == 0 ? -1 : -2);
  if (have < 4) return 0;
  if (memcmp(h, "BAM\1", 4)) return -2;
  if (n < 12) return -1;
  if (have < 8) return 0;
  const int64_t l_text = le32s(h + 4);
  if (l_text < 0 || 12 + l_text > n) return -1;
  if (have < 12 + l_text) return 0;
  const int64_t refs = le32s(h + 8 + l_text);
  if (refs < 0) return -1;
  int64_t at = 12 + l_text;
  for (int64_t r = 0; r < refs; r++) {
    if (at + 4 > n) return -1;
    if (have < at + 4) return 0;
    const int64_t l_name = le32s(h + at);
    if (l_name < 0 || at + 8 + l_name > n) return -1;
    at += 8 + l_name;
  }
  *n_ref = refs;
  *first_record = at;
  return 1;
}

BamChainEnd bam_walk_chain(const uint64_t *hits, size_t n_hits, int64_t from, int64_t end, bool last, std::vector<uint64_t> *rec,
                           int64_t *stop) {
  size_t i = 0;
  int64_t cur = from;
  while (cur < end) {
    while (i < n_hits && (int64_t)(hits[i] >> kSbSizeBits) < cur) i++;  // (candidates inside a record: decoys)
    if (i == n_hits || (int64_t)(hits[i] >> kSbSizeBits) != cur) break;
    const int64_t size = (int64_t)(hits[i] & kSbSizeMask);
    if (size > kBamMaxBlock || cur + 4 + size > end) break;  // (the scan gives no such candidate)
    rec->push_back(hits[i]);
    cur += 4 + size;
  }
  *stop = cur;
  if (cur >= end) return kBamChainDone;
  if (last || end - cur >= 4 + kBamMaxBlock) return kBamChainMalformed;
  return kBamChainCarry;
}

}  // namespace pbsim
