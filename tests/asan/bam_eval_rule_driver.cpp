// The host's decisions of pbsim_truth_bam_eval that need no device (pbsim3_amd/csrc/bam_eval_rule.cpp: the reference names of
// a parsed header, the tables that match references by name, the truth file of a record number, the report text) as a program
// of its own, for tests/test_mapeval_model.py under ASan + UBSan.
//   bam_eval_rule_driver names FILE                 FILE is an inflated BAM stream; the parser sees a heap copy of exactly the
//                                                  header's bytes:  "names N <name> ..." (each name in brackets)
//   bam_eval_rule_driver tables T OVER NAME.. [T OVER NAME..]... Q NAME..
//                                                  per truth file: T, its override or "-", its names; then Q and the query's
//                                                  names:  "tables [a b ..] .. | q .." or "tables refused: <message>"
//   bam_eval_rule_driver file_of INDEX FIRST..      "file_of F"
//   bam_eval_rule_driver report COUNT x12 [MAPQ:N:WRONG ...]     the report text, through pbsim_eval_report
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#define PBSIM_EVAL_NO_HIP
#include "bam_eval.h"
#include "pbsim3_amd.h"

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "names")) {
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<unsigned char> all;
    for (int ch; (ch = fgetc(f)) != EOF;) all.push_back((unsigned char)ch);
    fclose(f);
    pbsim::BamHeader hd;
    if (pbsim::bam_parse_header(all.data(), (int64_t)all.size(), (int64_t)all.size(), true, &hd) != 1) return 3;
    unsigned char *h = (unsigned char *)malloc((size_t)hd.first_record);  // exactly the header: a byte too far is a report
    memcpy(h, all.data(), (size_t)hd.first_record);
    std::vector<std::string> names;
    pbsim::bam_ref_names(h, hd, &names);
    printf("names %zu", names.size());
    for (const std::string &n : names) printf(" [%s]", n.c_str());
    printf("\n");
    free(h);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "tables")) {
    std::vector<std::vector<std::string>> truth;
    std::vector<const char *> over;
    std::vector<std::string> query;
    bool in_query = false;
    for (int i = 2; i < argc; i++) {
      if (!strcmp(argv[i], "T") && i + 1 < argc) {
        truth.emplace_back();
        over.push_back(strcmp(argv[i + 1], "-") ? argv[i + 1] : nullptr);
        i++;
      } else if (!strcmp(argv[i], "Q")) {
        in_query = true;
      } else if (in_query) {
        query.push_back(argv[i]);
      } else if (!truth.empty()) {
        truth.back().push_back(argv[i]);
      } else {
        return 2;
      }
    }
    pbsim::EvalRefTables tab;
    std::string err;
    if (!pbsim::eval_ref_tables(truth, over, query, &tab, &err)) {
      printf("tables refused: %s\n", err.c_str());
      return 0;
    }
    printf("tables");
    for (const std::vector<int32_t> &m : tab.truth_map) {
      printf(" [");
      for (size_t k = 0; k < m.size(); k++) printf(k ? " %d" : "%d", m[k]);
      printf("]");
    }
    printf(" |");
    for (int32_t v : tab.query_map) printf(" %d", v);
    printf("\n");
    return 0;
  }
  if (argc >= 4 && !strcmp(argv[1], "file_of")) {
    std::vector<int64_t> first;
    for (int i = 3; i < argc; i++) first.push_back(atoll(argv[i]));
    printf("file_of %d\n", pbsim::eval_file_of(first, atoll(argv[2])));
    return 0;
  }
  if (argc >= 14 && !strcmp(argv[1], "report")) {
    int64_t *counts = (int64_t *)malloc(12 * sizeof(int64_t)), *hist = (int64_t *)calloc(512, sizeof(int64_t));
    for (int k = 0; k < 12; k++) counts[k] = atoll(argv[2 + k]);
    for (int i = 14; i < argc; i++) {
      long long q = 0, n = 0, w = 0;
      if (sscanf(argv[i], "%lld:%lld:%lld", &q, &n, &w) != 3 || q < 0 || q > 255) return 2;
      hist[2 * q] = n;
      hist[2 * q + 1] = w;
    }
    const int64_t need = pbsim_eval_report(counts, hist, nullptr, 0);
    if (need < 0) return 3;
    char *buf = (char *)malloc((size_t)need + (need == 0));  // exactly the text
    if (pbsim_eval_report(counts, hist, buf, need - 1) != need) return 4;  // (a buffer one byte short is left alone)
    if (pbsim_eval_report(counts, hist, buf, need) != need) return 4;
    fwrite(buf, 1, (size_t)need, stdout);
    free(buf);
    free(counts);
    free(hist);
    return 0;
  }
  return 2;
}
