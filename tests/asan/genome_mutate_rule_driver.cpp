// The host's decisions of pbsim_genome_mutate that need no device (pbsim3_amd/csrc/genome_mutate_rule.cpp: the option check, the
// VCF header and the report text) as a program of its own, for tests/test_mutate_model.py under ASan + UBSan.
//   genome_mutate_rule_driver opts - | SEED SNV INS DEL EXT MAX_INDEL LINE_WIDTH PIECE   "opts s a b c e m w p" (completed) or
//                                                                                         "opts refused: <message>"
//   genome_mutate_rule_driver header SEED SNV INS DEL EXT MAX_INDEL [NAME LENGTH] ...    the header text over those genome records
//   genome_mutate_rule_driver report VALUE x24                 the result's numbers in its order, the arrays spread: the report
//                                                              text, through pbsim_mutate_report into a buffer of its exact size
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#define PBSIM_MUTATE_NO_HIP
#include "genome_mutate.h"

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "opts")) {
    pbsim_mutate_opts in, out;
    const bool defaults = !strcmp(argv[2], "-");
    if (!defaults) {
      if (argc != 10) return 2;
      in = pbsim_mutate_opts{(uint32_t)atoll(argv[2]), (int32_t)atoll(argv[3]), (int32_t)atoll(argv[4]), (int32_t)atoll(argv[5]),
                             (int32_t)atoll(argv[6]), (int32_t)atoll(argv[7]), (int32_t)atoll(argv[8]), atoll(argv[9])};
    }
    std::string err;
    if (!pbsim::mutate_check_opts(defaults ? nullptr : &in, &out, &err)) {
      printf("opts refused: %s\n", err.c_str());
      return 0;
    }
    printf("opts %u %d %d %d %d %d %d %lld\n", (unsigned)out.seed, out.snv_ppm, out.ins_ppm, out.del_ppm, out.ext_ppm, out.max_indel, out.line_width,
           (long long)out.piece_bytes);
    return 0;
  }
  if (argc >= 8 && argc % 2 == 0 && !strcmp(argv[1], "header")) {
    const pbsim_mutate_opts o = {(uint32_t)atoll(argv[2]), (int32_t)atoll(argv[3]), (int32_t)atoll(argv[4]), (int32_t)atoll(argv[5]),
                                 (int32_t)atoll(argv[6]), (int32_t)atoll(argv[7]), 60, 0};
    std::vector<const char *> names;
    std::vector<int64_t> lengths;
    for (int i = 8; i < argc; i += 2) names.push_back(argv[i]), lengths.push_back(atoll(argv[i + 1]));
    const std::string text = pbsim::mutate_header_text(o, names.data(), lengths.data(), (int)names.size());
    fwrite(text.data(), 1, text.size(), stdout);
    return 0;
  }
  if (argc == 2 + 24 && !strcmp(argv[1], "report")) {
    std::unique_ptr<pbsim_mutate_result> res(new pbsim_mutate_result());
    static_assert(sizeof(pbsim_mutate_result) == 24 * sizeof(int64_t), "the result is 24 numbers");
    int64_t *to = &res->records;  // (the struct holds int64_t only, in the report's order)
    std::vector<int64_t> values;
    for (int i = 2; i < argc; i++) values.push_back(atoll(argv[i]));
    memcpy(to, values.data(), sizeof(pbsim_mutate_result));
    const int64_t n = pbsim_mutate_report(res.get(), nullptr, 0);
    if (n < 0) return 3;
    std::vector<char> buf((size_t)n);
    if (pbsim_mutate_report(res.get(), buf.data(), n) != n) return 4;
    if (pbsim_mutate_report(res.get(), buf.data(), n - 1) != n) return 5;  // too small: untouched
    fwrite(buf.data(), 1, buf.size(), stdout);
    return 0;
  }
  return 2;
}
