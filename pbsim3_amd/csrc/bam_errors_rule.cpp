// bam_errors_rule.cpp -- what pbsim_bam_errors decides on the host, free of HIP (see bam_errors.h): the option check, the genome's
// names, the references looked up by name, the fit of the homopolymer deletion bias at 128 bits, and the report text
// (pbsim_errors_report).
#define PBSIM_ERRORS_NO_HIP
#include "bam_errors.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <unordered_map>

namespace pbsim {

namespace {
const char *const kCountName[kErrCounts] = {"records", "skipped_flag", "unaligned",    "skipped_mapq", "skipped_ref", "aligned",   "no_seq",
                                            "misfit",  "scored",       "no_nm",        "nm_unchecked", "nm_agree",    "nm_differ", "with_qual"};
typedef __int128 i128;
typedef unsigned __int128 u128;
constexpr int64_t kFitLimit = (int64_t)1 << 62;
}  // namespace

bool errors_check_opts(const pbsim_errors_opts *opts, pbsim_errors_opts *out, std::string *err) {
  const pbsim_errors_opts defaults = {0x900, 0, 0};
  *out = opts ? *opts : defaults;
  if (out->exclude_flags < 0 || out->exclude_flags > 65535) {
    *err = "exclude_flags must be 0 .. 65535";
    return false;
  }
  if (out->min_mapq < 0 || out->min_mapq > 255) {
    *err = "min_mapq must be 0 .. 255";
    return false;
  }
  if (out->piece_bytes < 0) {
    *err = "piece_bytes must not be negative (0: the default)";
    return false;
  }
  if (out->piece_bytes == 0) out->piece_bytes = kErrDefaultPiece;
  return true;
}

bool errors_check_genome(const pbsim_errors_ref *refs, int n_refs, std::string *err) {
  std::unordered_map<std::string, int> seen;
  for (int r = 0; r < n_refs; r++) {
    if (!refs[r].name || refs[r].bytes < 0 || (refs[r].bytes > 0 && !refs[r].lines)) {
      *err = "bad argument (genome record " + std::to_string(r) + ")";
      return false;
    }
    const auto got = seen.emplace(refs[r].name, r);
    if (!got.second) {
      *err = "the genome holds two records named \"" + std::string(refs[r].name) + "\" (records " + std::to_string(got.first->second) + " and " +
             std::to_string(r) + "): references are looked up by name";
      return false;
    }
  }
  return true;
}

bool errors_ref_map(const pbsim_errors_ref *refs, int n_refs, const std::vector<std::string> &file_names, const char *over,
                    const std::string &what, std::vector<int32_t> *map, std::string *err) {
  if (over && file_names.size() != 1) {
    *err = what + " has " + std::to_string(file_names.size()) + " references: a reference name can be given only to a file with exactly one";
    return false;
  }
  std::unordered_map<std::string, int32_t> number;
  for (int r = 0; r < n_refs; r++) number.emplace(refs[r].name, (int32_t)r);
  map->clear();
  for (const std::string &own : file_names) {
    const auto it = number.find(over ? std::string(over) : own);
    map->push_back(it == number.end() ? -1 : it->second);
  }
  return true;
}

void errors_fit(pbsim_errors_result *r) {
  i128 w = 0, sx = 0, sxx = 0, sy = 0, sxy = 0;
  for (int v = 1; v <= 10; v++) {
    const i128 x = v - 1, c = r->hp_cols[v], d = r->hp_del[v];
    w += c, sx += c * x, sxx += c * x * x, sy += d, sxy += d * x;
  }
  const i128 num = w * sxy - sx * sy, den = sxx * sy - sx * sxy;
  r->fit_ok = r->fit_bias_milli = r->fit_suggest_milli = 0;
  if (!(sy > 0 && den > 0)) return;
  const i128 n9 = 9000 * num;
  i128 q = n9 / den;
  if (n9 % den != 0 && n9 < 0) q -= 1;  // the floor toward minus infinity (den > 0)
  q += 1000;
  if (q > kFitLimit) q = kFitLimit;
  if (q < -kFitLimit) q = -kFitLimit;
  r->fit_ok = 1;
  r->fit_bias_milli = (int64_t)q;
  r->fit_suggest_milli = q < 1000 ? 1000 : q > 10000 ? 10000 : (int64_t)q;
}

std::string errors_report_text(const pbsim_errors_result &r) {
  std::string out = "#";
  char line[200];
  for (int k = 0; k < kErrCounts; k++) {
    snprintf(line, sizeof line, " %s=%lld", kCountName[k], (long long)r.counts[k]);
    out += line;
  }
  out += "\nE";
  for (int k = 0; k < kErrIdentitySum; k++) {
    snprintf(line, sizeof line, "\t%lld", (long long)r.totals[k]);
    out += line;
  }
  const uint64_t cols = (uint64_t)r.totals[kErrCols];
  for (int k : {kErrSub, kErrIns, kErrDel}) {
    snprintf(line, sizeof line, "\t%lld", cols ? (long long)((u128)(uint64_t)r.totals[k] * 1000000 / cols) : 0LL);
    out += line;
  }
  i128 n_identity = 0;
  for (int k = 0; k < kErrPpmBins; k++) n_identity += r.hist_identity[k];
  snprintf(line, sizeof line, "\t%lld\n", n_identity > 0 ? (long long)((i128)r.totals[kErrIdentitySum] / n_identity) : 0LL);
  out += line;
  for (int a = 0; a < 5; a++) {
    out += "M\t";
    out += "ACGTN"[a];
    for (int b = 0; b < 5; b++) {
      snprintf(line, sizeof line, "\t%lld", (long long)r.pair[5 * a + b]);
      out += line;
    }
    out += "\n";
  }
  for (int v = 0; v < kErrHp; v++) {
    if (r.hp_cols[v] <= 0) continue;
    snprintf(line, sizeof line, "HP\t%d\t%lld\t%lld\t%lld\t%lld\n", v, (long long)r.hp_cols[v], (long long)r.hp_sub[v], (long long)r.hp_del[v],
             (long long)((u128)(uint64_t)r.hp_del[v] * 1000000 / (uint64_t)r.hp_cols[v]));
    out += line;
  }
  pbsim_errors_result f = r;
  errors_fit(&f);
  snprintf(line, sizeof line, "B\t%lld\t%lld\t%lld\n", (long long)f.fit_ok, (long long)f.fit_bias_milli, (long long)f.fit_suggest_milli);
  out += line;
  for (int pass = 0; pass < 2; pass++)
    for (int k = 0; k < kErrLenBins; k++) {
      const int64_t v = pass ? r.del_len[k] : r.ins_len[k];
      if (v <= 0) continue;
      snprintf(line, sizeof line, "%s\t%d\t%lld\n", pass ? "DL" : "IL", k, (long long)v);
      out += line;
    }
  for (int pass = 0; pass < 2; pass++) {
    out += pass ? "DB" : "IB";
    for (int k = 0; k < kErrBases; k++) {
      snprintf(line, sizeof line, "\t%lld", (long long)(pass ? r.del_base[k] : r.ins_base[k]));
      out += line;
    }
    out += "\n";
  }
  for (int q = 0; q < kErrQBins; q++) {
    const int64_t c = r.qcal[q][0], s = r.qcal[q][1], i = r.qcal[q][2];
    if (c <= 0 && s <= 0 && i <= 0) continue;
    snprintf(line, sizeof line, "QC\t%d\t%lld\t%lld\t%lld\t", q, (long long)c, (long long)s, (long long)i);
    out += line;
    if (c > 0 && s > 0) {
      snprintf(line, sizeof line, "%lld\n", (long long)floor(-10000.0 * log10((double)s / (double)c)));
      out += line;
    } else {
      out += "*\n";
    }
  }
  for (int k = 0; k < kErrPpmBins; k++) {
    if (r.hist_identity[k] <= 0) continue;
    snprintf(line, sizeof line, "HI\t%d\t%lld\n", k, (long long)r.hist_identity[k]);
    out += line;
  }
  return out;
}

}  // namespace pbsim

extern "C" int64_t pbsim_errors_report(const pbsim_errors_result *result, char *buf, int64_t cap) {
  if (!result || cap < 0) return -1;
  const std::string text = pbsim::errors_report_text(*result);
  if (buf && cap >= (int64_t)text.size()) memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}
