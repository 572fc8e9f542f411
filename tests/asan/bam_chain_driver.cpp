// The host's decisions about a BAM stream (pbsim3_amd/csrc/bam_chain.cpp: the header parse and the chain walk over the scan's
// candidates, for the sampling input and the truth-BAM sort alike) as a program of their own, for
// tests/test_sample_bam_cpu.py under ASan + UBSan.
//   bam_chain_driver header FILE N:HAVE ...        the first N bytes of FILE are the stream, of which the parser sees a heap
//                                                  copy of exactly HAVE bytes:  "header N:HAVE -> RC N_REF FIRST"
//   bam_chain_driver header+ FILE N:HAVE ...       the same with the reference lengths wanted:
//                                                  "header N:HAVE -> RC FAULT EMPTY_NAME L_TEXT N_REF FIRST [L_REF ...]"
//   bam_chain_driver chain BITS FROM END LAST [OFFSET:SIZE ...]   BITS = 24: the sort's packing, 28: the sampling input's
//                                                  "chain -> END_KIND STOP N_REC OFFSET:SIZE ..."
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "bam_chain.h"

int main(int argc, char **argv) {
  if (argc >= 3 && (!strcmp(argv[1], "header") || !strcmp(argv[1], "header+"))) {
    const bool full = argv[1][6] == '+';
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<unsigned char> all;
    for (int ch; (ch = fgetc(f)) != EOF;) all.push_back((unsigned char)ch);
    fclose(f);
    for (int i = 3; i < argc; i++) {
      long long n = 0, have = 0;
      if (sscanf(argv[i], "%lld:%lld", &n, &have) != 2 || n < 0 || (size_t)n > all.size() || have < 0 || have > n) return 2;
      unsigned char *h = (unsigned char *)malloc((size_t)have + (have == 0));  // exactly `have` bytes: a byte too far is a report
      memcpy(h, all.data(), (size_t)have);
      pbsim::BamHeader hd;
      hd.l_text = hd.n_ref = hd.first_record = -7;  // (a return other than 1 leaves them)
      const int rc = pbsim::bam_parse_header(h, have, n, full, &hd);
      if (full) {
        printf("header %lld:%lld -> %d %d %d %lld %lld %lld", n, have, rc, (int)hd.fault, (int)hd.empty_name, (long long)hd.l_text,
               (long long)hd.n_ref, (long long)hd.first_record);
        for (int64_t l : hd.ref_len) printf(" %lld", (long long)l);
        printf("\n");
      } else {
        printf("header %lld:%lld -> %d %lld %lld\n", n, have, rc, (long long)hd.n_ref, (long long)hd.first_record);
      }
      free(h);
    }
    return 0;
  }
  if (argc >= 6 && !strcmp(argv[1], "chain")) {
    const int bits = atoi(argv[2]);
    if (bits != 24 && bits != 28) return 2;
    const pbsim::BamPacking pk = bits == 24 ? pbsim::kBamSortPacking : pbsim::kBamSamplePacking;
    const long long from = atoll(argv[3]), end = atoll(argv[4]);
    const bool last = atoi(argv[5]) != 0;
    argv++, argc--;
    const size_t n_hits = (size_t)(argc - 5);
    uint64_t *hits = (uint64_t *)malloc(n_hits * 8 + (n_hits == 0));
    for (size_t i = 0; i < n_hits; i++) {
      long long off = 0, size = 0;
      if (sscanf(argv[5 + i], "%lld:%lld", &off, &size) != 2) return 2;
      hits[i] = (uint64_t)off << pk.size_bits | (uint64_t)size;
    }
    std::vector<uint64_t> rec;
    int64_t stop = -7;
    const pbsim::BamChainEnd e = pbsim::bam_walk_chain(pk, hits, n_hits, from, end, last, &rec, &stop);
    printf("chain -> %s %lld %zu", e == pbsim::kBamChainDone ? "done" : e == pbsim::kBamChainCarry ? "carry" : "malformed", (long long)stop,
           rec.size());
    for (uint64_t r : rec) printf(" %llu:%llu", (unsigned long long)pk.offset(r), (unsigned long long)pk.size(r));
    printf("\n");
    free(hits);
    return 0;
  }
  return 2;
}
