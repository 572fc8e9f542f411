// bam_chain.cpp -- see bam_chain.h
#include "bam_chain.h"

#include <string.h>

#include <utility>

namespace pbsim {

namespace {
inline int64_t le32s(const uint8_t *p) {
  return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}
}  // namespace

int bam_parse_header(const uint8_t *h, int64_t have, int64_t n, bool want_ref_len, BamHeader *out) {
  auto bad = [&](BamHeaderFault f, int rc) {
    out->fault = n < 12 ? kBamHeaderShort : f;
    return rc;
  };
  if (have > n) have = n;
  if (n < 4) return have < n ? 0 : bad(kBamHeaderShort, n > 0 && memcmp(h, "BAM\1", (size_t)n) == 0 ? -1 : -2);
  if (have < 4) return 0;
  if (memcmp(h, "BAM\1", 4)) return bad(kBamHeaderMagic, -2);
  if (n < 12) return bad(kBamHeaderShort, -1);
  if (have < 8) return 0;
  BamHeader hd;
  hd.l_text = le32s(h + 4);
  if (hd.l_text < 0 || 12 + hd.l_text > n) return bad(kBamHeaderText, -1);
  if (have < 12 + hd.l_text) return 0;
  hd.n_ref = le32s(h + 8 + hd.l_text);
  if (hd.n_ref < 0) return bad(kBamHeaderNRef, -1);
  int64_t at = 12 + hd.l_text;
  for (int64_t r = 0; r < hd.n_ref; r++) {
    if (at + 4 > n) return bad(kBamHeaderRefs, -1);
    if (have < at + 4) return 0;
    const int64_t l_name = le32s(h + at);
    if (l_name < 0 || at + 8 + l_name > n) return bad(kBamHeaderRefs, -1);
    hd.empty_name |= l_name == 0;
    if (want_ref_len) {
      if (have < at + 8 + l_name) return 0;
      hd.ref_len.push_back(le32s(h + at + 4 + l_name));
    }
    at += 8 + l_name;
  }
  hd.first_record = at;
  *out = std::move(hd);
  return 1;
}

BamChainEnd bam_walk_chain(BamPacking pk, const uint64_t *hits, size_t n_hits, int64_t from, int64_t end, bool last,
                           std::vector<uint64_t> *rec, int64_t *stop) {
  size_t i = 0;
  int64_t cur = from;
  while (cur < end) {
    while (i < n_hits && pk.offset(hits[i]) < cur) i++;  // (candidates inside a record: decoys)
    if (i == n_hits || pk.offset(hits[i]) != cur) break;
    const int64_t size = pk.size(hits[i]);
    if (size > pk.max_block || cur + 4 + size > end) break;  // (the scan gives no such candidate)
    rec->push_back(hits[i]);
    cur += 4 + size;
  }
  *stop = cur;
  if (cur >= end) return kBamChainDone;
  if (last || end - cur >= 4 + pk.max_block) return kBamChainMalformed;
  return kBamChainCarry;
}

}  // namespace pbsim
