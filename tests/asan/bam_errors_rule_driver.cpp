// The host's decisions of pbsim_bam_errors that need no device (pbsim3_amd/csrc/bam_errors_rule.cpp: the option check, the genome's
// names, the references by name, the fit at 128 bits, the report text) as a program of its own, for tests/test_errors_model.py
// under ASan + UBSan.
//   bam_errors_rule_driver opts - | EXCLUDE MAPQ PIECE    "opts e q p" (completed) or "opts refused: <message>"
//   bam_errors_rule_driver genome NAME...                 "genome ok" or "genome refused: <message>"
//   bam_errors_rule_driver refmap OVER|- G NAME x G F NAME x F   "refmap m0 m1 .." or "refmap refused: <message>"
//   bam_errors_rule_driver fit COLS x12 DEL x12           "fit ok bias suggest"
//   bam_errors_rule_driver report COUNT x14 TOTAL x11 [ARRAY INDEX VALUE]...
//                                                         the report text, through pbsim_errors_report into a buffer of its exact size
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#define PBSIM_ERRORS_NO_HIP
#include "bam_errors.h"

int main(int argc, char **argv) {
  if (argc >= 3 && !strcmp(argv[1], "opts")) {
    pbsim_errors_opts in, out;
    const bool defaults = !strcmp(argv[2], "-");
    if (!defaults) {
      if (argc != 5) return 2;
      in = pbsim_errors_opts{(int32_t)atoll(argv[2]), (int32_t)atoll(argv[3]), atoll(argv[4])};
    }
    std::string err;
    if (!pbsim::errors_check_opts(defaults ? nullptr : &in, &out, &err)) {
      printf("opts refused: %s\n", err.c_str());
      return 0;
    }
    printf("opts %d %d %lld\n", out.exclude_flags, out.min_mapq, (long long)out.piece_bytes);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "genome")) {
    std::vector<pbsim_errors_ref> refs;
    for (int i = 2; i < argc; i++) refs.push_back(pbsim_errors_ref{argv[i], "ACGT", 4});
    std::string err;
    if (!pbsim::errors_check_genome(refs.data(), (int)refs.size(), &err)) printf("genome refused: %s\n", err.c_str());
    else printf("genome ok\n");
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "refmap")) {
    const char *over = strcmp(argv[2], "-") ? argv[2] : nullptr;
    int i = 3;
    const int g = atoi(argv[i++]);
    if (g < 0 || i + g >= argc) return 2;
    std::vector<pbsim_errors_ref> refs;
    for (int k = 0; k < g; k++) refs.push_back(pbsim_errors_ref{argv[i++], "ACGT", 4});
    const int f = atoi(argv[i++]);
    if (f < 0 || i + f != argc) return 2;
    std::vector<std::string> names(argv + i, argv + i + f);
    std::vector<int32_t> map;
    std::string err;
    if (!pbsim::errors_ref_map(refs.data(), g, names, over, "file 3", &map, &err)) {
      printf("refmap refused: %s\n", err.c_str());
      return 0;
    }
    printf("refmap");
    for (int32_t m : map) printf(" %d", m);
    printf("\n");
    return 0;
  }
  std::unique_ptr<pbsim_errors_result> res(new pbsim_errors_result());
  if (argc == 26 && !strcmp(argv[1], "fit")) {
    for (int k = 0; k < 12; k++) res->hp_cols[k] = atoll(argv[2 + k]), res->hp_del[k] = atoll(argv[14 + k]);
    pbsim::errors_fit(res.get());
    printf("fit %lld %lld %lld\n", (long long)res->fit_ok, (long long)res->fit_bias_milli, (long long)res->fit_suggest_milli);
    return 0;
  }
  if (argc >= 27 && !strcmp(argv[1], "report")) {
    int i = 2;
    for (int k = 0; k < 14; k++) res->counts[k] = atoll(argv[i++]);
    for (int k = 0; k < 11; k++) res->totals[k] = atoll(argv[i++]);
    const struct {
      const char *name;
      int64_t *at;
      long n;
    } arrays[] = {{"pair", res->pair, 25},        {"hp_cols", res->hp_cols, 12},   {"hp_sub", res->hp_sub, 12},     {"hp_del", res->hp_del, 12},
                  {"ins_len", res->ins_len, 64},  {"del_len", res->del_len, 64},   {"ins_base", res->ins_base, 5},  {"del_base", res->del_base, 5},
                  {"qcal", &res->qcal[0][0], 384}, {"hist_identity", res->hist_identity, 1001}};
    for (; i + 2 < argc; i += 3) {
      const long at = atol(argv[i + 1]);
      bool found = false;
      for (const auto &a : arrays)
        if (!strcmp(argv[i], a.name)) {
          if (at < 0 || at >= a.n) return 2;
          a.at[at] = atoll(argv[i + 2]);
          found = true;
        }
      if (!found) return 2;
    }
    if (i != argc) return 2;
    res->fit_ok = res->fit_bias_milli = res->fit_suggest_milli = -7;  // (not read)
    const int64_t n = pbsim_errors_report(res.get(), nullptr, 0);
    if (n < 0) return 3;
    std::vector<char> buf((size_t)n);
    if (pbsim_errors_report(res.get(), buf.data(), n) != n) return 4;
    if (pbsim_errors_report(res.get(), buf.data(), n - 1) != n) return 5;  // too small: untouched
    fwrite(buf.data(), 1, buf.size(), stdout);
    return 0;
  }
  return 2;
}
