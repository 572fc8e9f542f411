// The host's decisions of pbsim_bam_lift that need no device (pbsim3_amd/csrc/bam_lift_rule.cpp: the argument check, the header
// rewritten for the original genome, the words for a bad origin map, and the report text) as a program of its own, for
// tests/test_lift_model.py under ASan + UBSan.
//   bam_lift_rule_driver report VALUE x21      the result's numbers in its order: the report text, through pbsim_lift_report into a
//                                              buffer of its exact size
//   bam_lift_rule_driver header FILE LEN ..    FILE holds an inflated BAM header (magic .. the last l_ref), copied into a buffer of its
//                                              exact size; one new length per reference: the rewritten header's bytes
//   bam_lift_rule_driver args CASE N           "args ok" or "args refused: <message>"; CASE 0 good maps of N bases, 1 the second map
//                                              missing, 2 a map of 2^31 - 1 bases, 3 no file
//   bam_lift_rule_driver fault KIND            the words for a bad origin map
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#define PBSIM_LIFT_NO_HIP
#include "bam_lift.h"

static uint32_t le32(const char *p) {
  uint32_t v = 0;
  for (int k = 0; k < 4; k++) v |= (uint32_t)(unsigned char)p[k] << (8 * k);
  return v;
}

int main(int argc, char **argv) {
  if (argc == 2 + 21 && !strcmp(argv[1], "report")) {
    std::unique_ptr<pbsim_lift_result> res(new pbsim_lift_result());
    std::vector<int64_t> values;
    for (int i = 2; i < argc; i++) values.push_back(atoll(argv[i]));
    memcpy(res.get(), values.data(), sizeof(pbsim_lift_result));  // (the struct holds int64_t only, in the report's order)
    const int64_t n = pbsim_lift_report(res.get(), nullptr, 0);
    if (n < 0) return 3;
    std::vector<char> buf((size_t)n);
    if (pbsim_lift_report(res.get(), buf.data(), n) != n) return 4;
    if (pbsim_lift_report(res.get(), buf.data(), n - 1) != n) return 5;  // too small: untouched
    fwrite(buf.data(), 1, buf.size(), stdout);
    return 0;
  }
  if (argc >= 3 && !strcmp(argv[1], "header")) {
    FILE *fp = fopen(argv[2], "rb");
    if (!fp) return 3;
    std::string bytes;
    char piece[4096];
    for (size_t n; (n = fread(piece, 1, sizeof piece, fp)) > 0;) bytes.append(piece, n);
    fclose(fp);
    std::unique_ptr<char[]> exact(new char[bytes.size() ? bytes.size() : 1]);  // (a read past the header's last byte is seen)
    memcpy(exact.get(), bytes.data(), bytes.size());
    const int64_t l_text = le32(exact.get() + 4);
    const int64_t n_ref = le32(exact.get() + 8 + l_text);
    if (argc != 3 + n_ref) return 2;
    std::vector<std::string> names;
    std::vector<int64_t> new_len;
    int64_t at = 12 + l_text;
    for (int64_t r = 0; r < n_ref; r++) {
      const int64_t l_name = le32(exact.get() + at);
      names.push_back(std::string(exact.get() + at + 4, (size_t)l_name - 1));
      new_len.push_back(atoll(argv[3 + r]));
      at += 8 + l_name;
    }
    const std::string out = pbsim::lift_header((const uint8_t *)exact.get(), (int64_t)bytes.size(), l_text, names, new_len);
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "args")) {
    const int which = atoi(argv[2]);
    const int64_t n = atoll(argv[3]);
    std::vector<int32_t> map((size_t)n, 0);
    pbsim_lift_origin origins[2] = {{map.data(), n}, {map.data(), n}};
    if (which == 1) origins[1].origin = nullptr;
    if (which == 2) origins[0].n = 2147483647;
    const char bam[4] = {'B', 'A', 'M', 1};
    pbsim_errors_file file = {bam, 4, nullptr};
    pbsim_lift_sink sink = {nullptr, nullptr};
    std::string err;
    if (pbsim::lift_check_args(origins, 2, which == 3 ? nullptr : &file, &sink, &err)) printf("args ok\n");
    else printf("args refused: %s\n", err.c_str());
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "fault")) {
    printf("%s\n", pbsim::lift_origin_fault(atoi(argv[2])));
    return 0;
  }
  return 2;
}
