// vcf_compare_rule.cpp -- what pbsim_vcf_compare decides on the host, free of HIP (see vcf_compare.h): the option check, the contig
// names and their hash table, and the report text (pbsim_compare_report).
#define PBSIM_COMPARE_NO_HIP
#include "vcf_compare.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <utility>

namespace pbsim {

const char kCmpTextHeader[] = "#file\tline\tCHROM\tPOS\tREF\tALT\ttype\tstart\tref_len\talt\tverdict\tmate\n";

bool compare_check_opts(const pbsim_compare_opts *opts, pbsim_compare_opts *out, std::string *err) {
  const pbsim_compare_opts defaults = {0, 0, 0};
  *out = opts ? *opts : defaults;
  if (out->lines < 0 || out->lines > 1) {
    *err = "lines must be 0 (discordant) or 1 (all)";
    return false;
  }
  if (out->min_ms < 0) {
    *err = "min_ms must be 0 .. 2147483647";
    return false;
  }
  if (out->piece_bytes < 0) {
    *err = "piece_bytes must not be negative (0: the default)";
    return false;
  }
  if (out->piece_bytes == 0) out->piece_bytes = kCmpDefaultPiece;
  return true;
}

bool compare_check_names(const char *const *own, const char *const *ref_names, int n, std::vector<std::string> *used, std::string *err) {
  used->clear();
  for (int r = 0; r < n; r++) {
    const char *name = ref_names ? ref_names[r] : own[r];
    if (!name || !*name) {
      *err = std::string(ref_names ? "ref_names: " : "") + "genome record " + std::to_string(r) + " has no name";
      return false;
    }
    used->push_back(name);
  }
  std::vector<std::pair<std::string, int>> sorted;
  for (int r = 0; r < n; r++) sorted.push_back({(*used)[(size_t)r], r});
  std::sort(sorted.begin(), sorted.end());
  for (size_t k = 1; k < sorted.size(); k++)
    if (sorted[k].first == sorted[k - 1].first) {
      *err = std::string(ref_names ? "ref_names: " : "") + "two genome records are named \"" + sorted[k].first + "\" (records " +
             std::to_string(sorted[k - 1].second) + " and " + std::to_string(sorted[k].second) + ")";
      return false;
    }
  return true;
}

uint64_t compare_name_hash(const char *bytes, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t k = 0; k < n; k++) h = (h ^ (uint8_t)bytes[k]) * 0x100000001b3ull;
  return h;
}

void compare_name_table(const std::vector<std::string> &used, std::vector<uint64_t> *hash, std::vector<int32_t> *record) {
  std::vector<std::pair<uint64_t, int32_t>> pairs;
  for (size_t r = 0; r < used.size(); r++) pairs.push_back({compare_name_hash(used[r].data(), used[r].size()), (int32_t)r});
  std::sort(pairs.begin(), pairs.end());
  hash->clear(), record->clear();
  for (const auto &p : pairs) hash->push_back(p.first), record->push_back(p.second);
}

std::string compare_report_text(const pbsim_compare_result &r) {
  static const char *const kTypeNames[] = {"snv", "ins", "del", "complex", "all"};
  static const char *const kBinNames[] = {"1", "2-5", "6-15", "16-49", "50+"};
  std::string out =
      "#\tlines\tmalformed\tunknown_contig\tunsupported\tref_mismatch\tfiltered\tno_change\tdup\tcompared\tshifted\tlongest_shift\n";
  char item[40];
  auto add = [&](int64_t v) {
    snprintf(item, sizeof item, "\t%lld", (long long)v);
    out += item;
  };
  // (the quotient of two counts below 2^63: the product is taken in 128 bits)
  auto ppm = [](int64_t a, int64_t b) { return b > 0 && a >= 0 ? (int64_t)((unsigned __int128)a * 1000000u / (unsigned __int128)b) : 0; };
  for (int w = 0; w < 2; w++) {
    out += w ? "C" : "T";
    for (int k = 0; k < kCmpFileCells; k++) add(r.files[w][k]);
    out += "\n";
  }
  for (int t = 0; t <= kCmpTypes; t++) {
    int64_t v[kCmpTypeCells];
    for (int k = 0; k < kCmpTypeCells; k++) {
      // (the sum wraps as the model's unbounded one does not: counts of lines stay far below)
      uint64_t sum = 0;
      for (int u = 0; u < kCmpTypes; u++) sum += (uint64_t)r.types[u][k];
      v[k] = t < kCmpTypes ? r.types[t][k] : (int64_t)sum;
    }
    out += std::string("P\t") + kTypeNames[t];
    for (int k = 0; k < kCmpTypeCells; k++) add(v[k]);
    add(ppm(v[kCnFound], v[kCnTruth]));
    add(ppm(v[kCnTp], v[kCnCalls]));
    out += "\n";
  }
  for (int w = 0; w < 2; w++)
    for (int b = 0; b < kCmpBins; b++) {
      const int64_t *v = r.lengths[w][b];
      if (!v[0] && !v[1] && !v[2] && !v[3]) continue;
      out += std::string("L\t") + (w ? "del" : "ins") + "\t" + kBinNames[b];
      for (int k = 0; k < kCmpLengthCells; k++) add(v[k]);
      out += "\n";
    }
  uint64_t above_tp[kCmpMsBins + 1], above_fp[kCmpMsBins + 1];
  above_tp[kCmpMsBins] = above_fp[kCmpMsBins] = 0;
  for (int k = kCmpMsBins - 1; k >= 0; k--) above_tp[k] = above_tp[k + 1] + (uint64_t)r.ms[k][0], above_fp[k] = above_fp[k + 1] + (uint64_t)r.ms[k][1];
  for (int k = 0; k < kCmpMsBins; k++) {
    if (!r.ms[k][0] && !r.ms[k][1]) continue;
    snprintf(item, sizeof item, "Q\t%d", k);
    out += item;
    add(r.ms[k][0]), add(r.ms[k][1]), add((int64_t)above_tp[k]), add((int64_t)above_fp[k]);
    out += "\n";
  }
  return out;
}

}  // namespace pbsim

extern "C" int64_t pbsim_compare_report(const pbsim_compare_result *result, char *buf, int64_t cap) {
  if (!result || cap < 0) return -1;
  const std::string text = pbsim::compare_report_text(*result);
  if (buf && cap >= (int64_t)text.size()) memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}
