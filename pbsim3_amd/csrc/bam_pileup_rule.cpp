// bam_pileup_rule.cpp -- what pbsim_bam_pileup decides on the host, free of HIP (see bam_pileup.h): the option check and the report
// text (pbsim_pileup_report).  The genome's names and the references by name are bam_errors_rule.cpp's.
#define PBSIM_PILEUP_NO_HIP
#include "bam_pileup.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

namespace pbsim {

namespace {
const char *const kCountName[kPileCounts] = {"records", "skipped_flag", "unaligned", "skipped_mapq", "skipped_ref", "aligned", "no_seq", "misfit", "scored"};
typedef unsigned __int128 u128;
}  // namespace

bool pileup_check_opts(const pbsim_pileup_opts *opts, pbsim_pileup_opts *out, std::string *err) {
  const pbsim_pileup_opts defaults = {0x900, 0, 0, 0, 1, 0};
  *out = opts ? *opts : defaults;
  if (out->exclude_flags < 0 || out->exclude_flags > 65535) {
    *err = "exclude_flags must be 0 .. 65535";
    return false;
  }
  if (out->min_mapq < 0 || out->min_mapq > 255) {
    *err = "min_mapq must be 0 .. 255";
    return false;
  }
  if (out->min_baseq < 0 || out->min_baseq > 255) {
    *err = "min_baseq must be 0 .. 255";
    return false;
  }
  if (out->format != 0 && out->format != 1) {
    *err = "format must be 0 (sites) or 1 (all)";
    return false;
  }
  if (out->min_depth < 0) {
    *err = "min_depth must not be negative";
    return false;
  }
  if (out->piece_bytes < 0) {
    *err = "piece_bytes must not be negative (0: the default)";
    return false;
  }
  if (out->piece_bytes == 0) out->piece_bytes = kPileDefaultPiece;
  return true;
}

std::string pileup_report_text(const pbsim_pileup_result &r) {
  std::string out = "#";
  char line[200];
  for (int k = 0; k < kPileCounts; k++) {
    snprintf(line, sizeof line, " %s=%lld", kCountName[k], (long long)r.counts[k]);
    out += line;
  }
  out += "\nS";
  for (int k = 0; k < kPileSites; k++) {
    snprintf(line, sizeof line, "\t%lld", (long long)r.sites[k]);
    out += line;
  }
  const int64_t d = r.sites[kPsDiscordant], c = r.sites[kPsCalled];
  snprintf(line, sizeof line, "\t%lld\t", c ? (long long)((u128)(uint64_t)d * 1000000 / (uint64_t)c) : 0LL);
  out += line;
  if (d > 0 && c > 0) {
    snprintf(line, sizeof line, "%lld\n", (long long)floor(-10000.0 * log10((double)d / (double)c)));
    out += line;
  } else {
    out += "*\n";
  }
  out += "C";
  for (int k = 0; k < kPileWidth; k++) {
    snprintf(line, sizeof line, "\t%lld", (long long)r.cell_sums[k]);
    out += line;
  }
  snprintf(line, sizeof line, "\t%lld\t%lld\n", (long long)r.ins_unanchored, (long long)r.max_depth);
  out += line;
  for (int v = 0; v < kPileHp; v++) {
    if (!r.hp_called[v] && !r.hp_sub[v] && !r.hp_del[v] && !r.hp_ins[v]) continue;
    snprintf(line, sizeof line, "HP\t%d\t%lld\t%lld\t%lld\t%lld\n", v, (long long)r.hp_called[v], (long long)r.hp_sub[v], (long long)r.hp_del[v],
             (long long)r.hp_ins[v]);
    out += line;
  }
  return out;
}

}  // namespace pbsim

extern "C" int64_t pbsim_pileup_report(const pbsim_pileup_result *result, char *buf, int64_t cap) {
  if (!result || cap < 0) return -1;
  const std::string text = pbsim::pileup_report_text(*result);
  if (buf && cap >= (int64_t)text.size()) memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}
