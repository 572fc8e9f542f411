// The host's decisions of pbsim_vcf_apply that need no device (pbsim3_amd/csrc/vcf_apply_rule.cpp: the option check, the sample's
// name looked up in the #CHROM line, and the report text) as a program of its own, for tests/test_apply_model.py under ASan + UBSan.
//   vcf_apply_rule_driver opts - | HAPLOTYPE SAMPLE LINES WIDTH PIECE   "opts h s l w p" (completed) or "opts refused: <message>"
//   vcf_apply_rule_driver sample FILE NAME                             "sample <column>": the text of FILE, copied into a buffer of
//                                                                      its exact size, through pbsim_apply_sample
//   vcf_apply_rule_driver report VALUE x23                             the result's numbers in its order: the report text, through
//                                                                      pbsim_apply_report into a buffer of its exact size
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#define PBSIM_APPLY_NO_HIP
#include "vcf_apply.h"

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "opts")) {
    pbsim_apply_opts in, out;
    const bool defaults = !strcmp(argv[2], "-");
    if (!defaults) {
      if (argc != 7) return 2;
      in = pbsim_apply_opts{(int32_t)atoll(argv[2]), (int32_t)atoll(argv[3]), (int32_t)atoll(argv[4]), (int32_t)atoll(argv[5]), atoll(argv[6])};
    }
    std::string err;
    if (!pbsim::apply_check_opts(defaults ? nullptr : &in, &out, &err)) {
      printf("opts refused: %s\n", err.c_str());
      return 0;
    }
    printf("opts %d %d %d %d %lld\n", out.haplotype, out.sample, out.lines, out.line_width, (long long)out.piece_bytes);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "sample")) {
    FILE *fp = fopen(argv[2], "rb");
    if (!fp) return 3;
    std::string text;
    char piece[4096];
    for (size_t n; (n = fread(piece, 1, sizeof piece, fp)) > 0;) text.append(piece, n);
    fclose(fp);
    std::unique_ptr<char[]> exact(new char[text.size() ? text.size() : 1]);  // (a read past the text's last byte is seen)
    memcpy(exact.get(), text.data(), text.size());
    printf("sample %d\n", (int)pbsim_apply_sample(exact.get(), (int64_t)text.size(), argv[3]));
    return 0;
  }
  if (argc == 2 + 23 && !strcmp(argv[1], "report")) {
    std::unique_ptr<pbsim_apply_result> res(new pbsim_apply_result());
    static_assert(sizeof(pbsim_apply_result) == 23 * sizeof(int64_t), "the result is 23 numbers");
    std::vector<int64_t> values;
    for (int i = 2; i < argc; i++) values.push_back(atoll(argv[i]));
    memcpy(res.get(), values.data(), sizeof(pbsim_apply_result));  // (the struct holds int64_t only, in the report's order)
    const int64_t n = pbsim_apply_report(res.get(), nullptr, 0);
    if (n < 0) return 3;
    std::vector<char> buf((size_t)n);
    if (pbsim_apply_report(res.get(), buf.data(), n) != n) return 4;
    if (pbsim_apply_report(res.get(), buf.data(), n - 1) != n) return 5;  // too small: untouched
    fwrite(buf.data(), 1, buf.size(), stdout);
    return 0;
  }
  return 2;
}
