// The host's decisions of pbsim_bam_consensus that need no device (pbsim3_amd/csrc/bam_consensus_rule.cpp: the option check and the
// report text) as a program of its own, for tests/test_consensus_model.py under ASan + UBSan.
//   bam_consensus_rule_driver opts - | EXCLUDE MAPQ BASEQ FILL DEPTH MAX_INS WIDTH PIECE
//                                                         "opts e q b f d m w p" (completed) or "opts refused: <message>"
//   bam_consensus_rule_driver report COUNT x9 SITE x9 UNANCHORED MAX BASES x6 INS_SITES LONGEST CAPPED INS_LEN x64 TEXT_BYTES
//                                                         the report text, through pbsim_consensus_report into a buffer of its exact size
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#define PBSIM_CONSENSUS_NO_HIP
#include "bam_consensus.h"

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "opts")) {
    pbsim_consensus_opts in, out;
    const bool defaults = !strcmp(argv[2], "-");
    if (!defaults) {
      if (argc != 10) return 2;
      in = pbsim_consensus_opts{(int32_t)atoll(argv[2]), (int32_t)atoll(argv[3]), (int32_t)atoll(argv[4]), (int32_t)atoll(argv[5]), atoll(argv[6]),
                                (int32_t)atoll(argv[7]), (int32_t)atoll(argv[8]), atoll(argv[9])};
    }
    std::string err;
    if (!pbsim::consensus_check_opts(defaults ? nullptr : &in, &out, &err)) {
      printf("opts refused: %s\n", err.c_str());
      return 0;
    }
    printf("opts %d %d %d %d %lld %d %d %lld\n", out.exclude_flags, out.min_mapq, out.min_baseq, out.fill, (long long)out.min_depth, out.max_ins,
           out.line_width, (long long)out.piece_bytes);
    return 0;
  }
  if (argc == 2 + 9 + 9 + 2 + 6 + 3 + 64 + 1 && !strcmp(argv[1], "report")) {
    std::unique_ptr<pbsim_consensus_result> res(new pbsim_consensus_result());
    int i = 2;
    for (int k = 0; k < 9; k++) res->counts[k] = atoll(argv[i++]);
    for (int k = 0; k < 9; k++) res->sites[k] = atoll(argv[i++]);
    res->ins_unanchored = atoll(argv[i++]);
    res->max_depth = atoll(argv[i++]);
    for (int k = 0; k < 6; k++) res->bases[k] = atoll(argv[i++]);
    res->ins_sites = atoll(argv[i++]);
    res->ins_longest = atoll(argv[i++]);
    res->ins_capped = atoll(argv[i++]);
    for (int k = 0; k < 64; k++) res->ins_len[k] = atoll(argv[i++]);
    res->text_bytes = atoll(argv[i++]);
    const int64_t n = pbsim_consensus_report(res.get(), nullptr, 0);
    if (n < 0) return 3;
    std::vector<char> buf((size_t)n);
    if (pbsim_consensus_report(res.get(), buf.data(), n) != n) return 4;
    if (pbsim_consensus_report(res.get(), buf.data(), n - 1) != n) return 5;  // too small: untouched
    fwrite(buf.data(), 1, buf.size(), stdout);
    return 0;
  }
  return 2;
}
