// bam_eval_rule.cpp -- what pbsim_truth_bam_eval decides on the host, free of HIP (see bam_eval.h): the reference names of a
// parsed header, the tables that match references by name, and the report text (pbsim_eval_report).
#define PBSIM_EVAL_NO_HIP
#include "bam_eval.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

namespace {
inline int64_t le32s(const uint8_t *p) {
  return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}
const char *const kCountName[kEvalCounts] = {"truth_records", "query_records", "primary", "secondary", "supplementary", "unknown",
                                             "duplicate",     "unmapped",      "scored",  "correct",   "wrong",         "missing"};
}  // namespace

void bam_ref_names(const uint8_t *h, const BamHeader &hd, std::vector<std::string> *names) {
  names->clear();
  int64_t at = 12 + hd.l_text;
  for (int64_t r = 0; r < hd.n_ref; r++) {
    const int64_t l_name = le32s(h + at);
    const char *name = (const char *)h + at + 4;
    names->emplace_back(name, strnlen(name, (size_t)l_name));
    at += 8 + l_name;
  }
}

bool eval_ref_tables(const std::vector<std::vector<std::string>> &truth_names, const std::vector<const char *> &override_name,
                     const std::vector<std::string> &query_names, EvalRefTables *out, std::string *err) {
  std::unordered_map<std::string, int32_t> number;
  out->truth_map.assign(truth_names.size(), std::vector<int32_t>());
  for (size_t f = 0; f < truth_names.size(); f++) {
    const char *over = f < override_name.size() ? override_name[f] : nullptr;
    if (over && truth_names[f].size() != 1) {
      *err = "truth file " + std::to_string(f) + " has " + std::to_string(truth_names[f].size()) +
             " references: a reference name can be given only to a truth file with exactly one";
      return false;
    }
    for (const std::string &own : truth_names[f]) {
      const std::string name = over ? std::string(over) : own;
      const auto it = number.emplace(name, (int32_t)number.size()).first;
      out->truth_map[f].push_back(it->second);
    }
  }
  out->query_map.clear();
  for (const std::string &name : query_names) {
    const auto it = number.find(name);
    out->query_map.push_back(it == number.end() ? -1 : it->second);
  }
  return true;
}

int eval_file_of(const std::vector<int64_t> &first_record, int64_t index) {
  return (int)(std::upper_bound(first_record.begin(), first_record.end(), index) - first_record.begin()) - 1;
}

std::string eval_report_text(const int64_t counts[kEvalCounts], const int64_t hist[512]) {
  std::string out = "#";
  char line[256];
  for (int k = 0; k < kEvalCounts; k++) {
    snprintf(line, sizeof line, " %s=%lld", kCountName[k], (long long)counts[k]);
    out += line;
  }
  out += "\n";
  int64_t cum_n = 0, cum_w = 0;
  for (int q = 255; q >= 0; q--) {
    const int64_t n = hist[2 * q], w = hist[2 * q + 1];
    if (n <= 0) continue;
    cum_n += n;
    cum_w += w;
    const int64_t truth = counts[kEvalTruth] > 0 ? counts[kEvalTruth] : 1;  // (scored records without truth records: not from the stage)
    snprintf(line, sizeof line, "Q\t%d\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\n", q, (long long)n, (long long)w, (long long)cum_n, (long long)cum_w,
             (long long)(cum_w * 1000000 / cum_n), (long long)(cum_n * 1000000 / truth));
    out += line;
  }
  return out;
}

}  // namespace pbsim

extern "C" int64_t pbsim_eval_report(const int64_t counts[12], const int64_t hist[512], char *buf, int64_t cap) {
  if (!counts || !hist || cap < 0) return -1;
  const std::string text = pbsim::eval_report_text(counts, hist);
  if (buf && cap >= (int64_t)text.size()) memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}
