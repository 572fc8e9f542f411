// The host's decisions of pbsim_bam_depth that need no device (pbsim3_amd/csrc/bam_depth_rule.cpp: the option check, the
// references' offset table, the report text) as a program of its own, for tests/test_depth_model.py under ASan + UBSan.
//   bam_depth_rule_driver opts - | EXCLUDE MAPQ DELETIONS FORMAT WINDOW PIECE
//                                                  "opts e q d f w p" (completed) or "opts refused: <message>"
//   bam_depth_rule_driver offsets WINDOW L_REF..    "offsets o0 o1 .. | w0 w1 .." or "offsets refused: <message>"
//   bam_depth_rule_driver report COUNT x6 [R NAME L_REF COVERED SUM MAX]... [H DEPTH POSITIONS]...
//                                                  the report text, through pbsim_depth_report into a buffer of its exact size
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#define PBSIM_DEPTH_NO_HIP
#include "bam_depth.h"

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "opts")) {
    pbsim_depth_opts in, out;
    const bool defaults = !strcmp(argv[2], "-");
    if (!defaults) {
      if (argc != 8) return 2;
      in = pbsim_depth_opts{(int32_t)atoll(argv[2]), (int32_t)atoll(argv[3]), (int32_t)atoll(argv[4]), (int32_t)atoll(argv[5]), atoll(argv[6]), atoll(argv[7])};
    }
    std::string err;
    if (!pbsim::depth_check_opts(defaults ? nullptr : &in, &out, &err)) {
      printf("opts refused: %s\n", err.c_str());
      return 0;
    }
    printf("opts %d %d %d %d %lld %lld\n", out.exclude_flags, out.min_mapq, out.count_deletions, out.format, (long long)out.window, (long long)out.piece_bytes);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "offsets")) {
    std::vector<int64_t> len, off, win;
    for (int i = 3; i < argc; i++) len.push_back(atoll(argv[i]));
    std::string err;
    if (!pbsim::depth_ref_offsets(len, atoll(argv[2]), &off, &win, &err)) {
      printf("offsets refused: %s\n", err.c_str());
      return 0;
    }
    printf("offsets");
    for (int64_t x : off) printf(" %lld", (long long)x);
    printf(" |");
    for (int64_t x : win) printf(" %lld", (long long)x);
    printf("\n");
    return 0;
  }
  if (argc >= 8 && !strcmp(argv[1], "report")) {
    int64_t counts[6], hist[256] = {0};
    for (int k = 0; k < 6; k++) counts[k] = atoll(argv[2 + k]);
    std::vector<std::string> names;
    std::vector<int64_t> rows;
    int i = 8;
    for (; i + 5 < argc && !strcmp(argv[i], "R"); i += 6) {
      names.push_back(argv[i + 1]);
      for (int k = 2; k < 6; k++) rows.push_back(atoll(argv[i + k]));
    }
    for (; i + 2 < argc && !strcmp(argv[i], "H"); i += 3) hist[atoi(argv[i + 1]) & 255] = atoll(argv[i + 2]);
    if (i != argc) return 2;
    std::vector<const char *> ptr;
    for (const std::string &n : names) ptr.push_back(n.c_str());
    const int64_t n = pbsim_depth_report(counts, (int32_t)ptr.size(), ptr.data(), rows.data(), hist, nullptr, 0);
    if (n < 0) return 3;
    std::vector<char> buf((size_t)n);
    if (pbsim_depth_report(counts, (int32_t)ptr.size(), ptr.data(), rows.data(), hist, buf.data(), n) != n) return 4;
    if (pbsim_depth_report(counts, (int32_t)ptr.size(), ptr.data(), rows.data(), hist, buf.data(), n - 1) != n) return 5;  // too small: untouched
    fwrite(buf.data(), 1, buf.size(), stdout);
    return 0;
  }
  return 2;
}
