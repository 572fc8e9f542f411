// The host's decisions of pbsim_bam_pileup that need no device (pbsim3_amd/csrc/bam_pileup_rule.cpp: the option check and the
// report text) as a program of its own, for tests/test_pileup_model.py under ASan + UBSan.
//   bam_pileup_rule_driver opts - | EXCLUDE MAPQ BASEQ FORMAT DEPTH PIECE   "opts e q b f d p" (completed) or "opts refused: <message>"
//   bam_pileup_rule_driver report COUNT x9 SITE x9 SUM x8 UNANCHORED MAX CALLED x12 SUB x12 DEL x12 INS x12
//                                                         the report text, through pbsim_pileup_report into a buffer of its exact size
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#define PBSIM_PILEUP_NO_HIP
#include "bam_pileup.h"

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "opts")) {
    pbsim_pileup_opts in, out;
    const bool defaults = !strcmp(argv[2], "-");
    if (!defaults) {
      if (argc != 8) return 2;
      in = pbsim_pileup_opts{(int32_t)atoll(argv[2]), (int32_t)atoll(argv[3]), (int32_t)atoll(argv[4]), (int32_t)atoll(argv[5]), atoll(argv[6]), atoll(argv[7])};
    }
    std::string err;
    if (!pbsim::pileup_check_opts(defaults ? nullptr : &in, &out, &err)) {
      printf("opts refused: %s\n", err.c_str());
      return 0;
    }
    printf("opts %d %d %d %d %lld %lld\n", out.exclude_flags, out.min_mapq, out.min_baseq, out.format, (long long)out.min_depth, (long long)out.piece_bytes);
    return 0;
  }
  if (argc == 2 + 9 + 9 + 8 + 2 + 48 && !strcmp(argv[1], "report")) {
    std::unique_ptr<pbsim_pileup_result> res(new pbsim_pileup_result());
    int i = 2;
    for (int k = 0; k < 9; k++) res->counts[k] = atoll(argv[i++]);
    for (int k = 0; k < 9; k++) res->sites[k] = atoll(argv[i++]);
    for (int k = 0; k < 8; k++) res->cell_sums[k] = atoll(argv[i++]);
    res->ins_unanchored = atoll(argv[i++]);
    res->max_depth = atoll(argv[i++]);
    for (int64_t *to : {res->hp_called, res->hp_sub, res->hp_del, res->hp_ins})
      for (int k = 0; k < 12; k++) to[k] = atoll(argv[i++]);
    const int64_t n = pbsim_pileup_report(res.get(), nullptr, 0);
    if (n < 0) return 3;
    std::vector<char> buf((size_t)n);
    if (pbsim_pileup_report(res.get(), buf.data(), n) != n) return 4;
    if (pbsim_pileup_report(res.get(), buf.data(), n - 1) != n) return 5;  // too small: untouched
    fwrite(buf.data(), 1, buf.size(), stdout);
    return 0;
  }
  return 2;
}
