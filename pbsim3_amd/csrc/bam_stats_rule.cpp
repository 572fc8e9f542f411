// bam_stats_rule.cpp -- what pbsim_bam_stats decides on the host, free of HIP (see bam_stats.h): the option check, the table of
// the fixed-point error probabilities, the length row's standard deviation at 128 bits, and the report text (pbsim_stats_report).
#define PBSIM_STATS_NO_HIP
#include "bam_stats.h"

#include <stdio.h>
#include <string.h>

namespace pbsim {

namespace {
const char *const kCountName[kStatsCounts] = {"records", "skipped_flag", "unaligned", "skipped_mapq", "aligned",
                                              "no_seq",  "no_qual",      "no_nm",     "nm_bad",       "scored"};
typedef unsigned __int128 u128;

uint64_t isqrt64(uint64_t x) {
  uint64_t r = 0;
  for (uint64_t bit = (uint64_t)1 << 62; bit; bit >>= 2) {
    if (x >= r + bit) {
      x -= r + bit;
      r = (r >> 1) + bit;
    } else {
      r >>= 1;
    }
  }
  return r;
}
}  // namespace

// round(2^32 10^(-q/10)): no entry lies within 0.003 of a rounding tie (tests/test_stats_model.py holds them to 80-digit decimals)
const uint64_t kStatsE[kStatsQBins] = {
    4294967296ull, 3411613790ull, 2709941160ull, 2152582778ull, 1709857278ull, 1358187913ull, 1078847007ull, 856958639ull,
    680706443ull, 540704347ull, 429496730ull, 341161379ull, 270994116ull, 215258278ull, 170985728ull, 135818791ull,
    107884701ull, 85695864ull, 68070644ull, 54070435ull, 42949673ull, 34116138ull, 27099412ull, 21525828ull,
    17098573ull, 13581879ull, 10788470ull, 8569586ull, 6807064ull, 5407043ull, 4294967ull, 3411614ull,
    2709941ull, 2152583ull, 1709857ull, 1358188ull, 1078847ull, 856959ull, 680706ull, 540704ull,
    429497ull, 341161ull, 270994ull, 215258ull, 170986ull, 135819ull, 107885ull, 85696ull,
    68071ull, 54070ull, 42950ull, 34116ull, 27099ull, 21526ull, 17099ull, 13582ull,
    10788ull, 8570ull, 6807ull, 5407ull, 4295ull, 3412ull, 2710ull, 2153ull,
    1710ull, 1358ull, 1079ull, 857ull, 681ull, 541ull, 429ull, 341ull,
    271ull, 215ull, 171ull, 136ull, 108ull, 86ull, 68ull, 54ull,
    43ull, 34ull, 27ull, 22ull, 17ull, 14ull, 11ull, 9ull,
    7ull, 5ull, 4ull, 3ull, 3ull, 2ull, 2ull, 1ull,
    1ull, 1ull, 1ull, 1ull, 0ull, 0ull, 0ull, 0ull,
    0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull,
    0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull,
    0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull,
};

bool stats_check_opts(const pbsim_stats_opts *opts, pbsim_stats_opts *out, std::string *err) {
  const pbsim_stats_opts defaults = {0x900, 0, 0};
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
  if (out->piece_bytes == 0) out->piece_bytes = kStatsDefaultPiece;
  return true;
}

int64_t stats_length_sd(uint64_t n, uint64_t bases, uint64_t sq_lo, uint64_t sq_hi) {
  if (n == 0) return 0;
  const u128 sumsq = (u128)sq_lo + ((u128)sq_hi << 32);
  const u128 num = (u128)n * sumsq - (u128)bases * bases;  // (Cauchy-Schwarz: not negative)
  return (int64_t)isqrt64((uint64_t)(num / ((u128)n * n)));
}

int64_t stats_muldiv(uint64_t a, uint64_t m, uint64_t b) { return (int64_t)((u128)a * m / b); }

std::string stats_report_text(const int64_t counts[kStatsCounts], const int64_t len_row[kStatsLenRow], const int64_t totals[kStatsTotals],
                              const int64_t hist_q[kStatsQBins], const int64_t hist_identity[kStatsPpmBins],
                              const int64_t hist_qacc[kStatsPpmBins]) {
  std::string out = "#";
  char line[160];
  for (int k = 0; k < kStatsCounts; k++) {
    snprintf(line, sizeof line, " %s=%lld", kCountName[k], (long long)counts[k]);
    out += line;
  }
  out += "\nL";
  for (int k = 0; k < kStatsLenRow; k++) {
    snprintf(line, sizeof line, "\t%lld", (long long)len_row[k]);
    out += line;
  }
  const uint64_t cols = (uint64_t)totals[kStatsCols], sub = (uint64_t)totals[kStatsSub], ins = (uint64_t)totals[kStatsIns],
                 del = (uint64_t)totals[kStatsDel];
  const u128 diff = (u128)sub + ins + del;
  snprintf(line, sizeof line, "\nE\t%llu\t%llu\t%llu\t%llu", (unsigned long long)sub, (unsigned long long)ins, (unsigned long long)del,
           (unsigned long long)cols);
  out += line;
  for (uint64_t x : {sub, ins, del}) {
    snprintf(line, sizeof line, "\t%lld", cols ? (long long)((u128)x * 1000000 / cols) : 0LL);
    out += line;
  }
  for (uint64_t x : {sub, ins, del}) {
    snprintf(line, sizeof line, "\t%lld", diff ? (long long)((u128)x * 1000 / diff) : 0LL);
    out += line;
  }
  int64_t q_bases = 0;
  for (int q = 0; q < kStatsQBins; q++) q_bases += hist_q[q];
  snprintf(line, sizeof line, "\t%lld\nQ\t%lld\t%lld\n", counts[kStatsScored] ? (long long)(totals[kStatsIdentitySum] / counts[kStatsScored]) : 0LL,
           totals[kStatsAccReads] ? (long long)(totals[kStatsAccSum] / totals[kStatsAccReads]) : 0LL,
           q_bases ? (long long)((u128)(uint64_t)totals[kStatsQSum] * 1000 / (uint64_t)q_bases) : 0LL);
  out += line;
  const struct {
    const char *tag;
    const int64_t *h;
    int n;
  } hists[3] = {{"HQ", hist_q, kStatsQBins}, {"HI", hist_identity, kStatsPpmBins}, {"HA", hist_qacc, kStatsPpmBins}};
  for (const auto &h : hists)
    for (int k = 0; k < h.n; k++) {
      if (h.h[k] <= 0) continue;
      snprintf(line, sizeof line, "%s\t%d\t%lld\n", h.tag, k, (long long)h.h[k]);
      out += line;
    }
  return out;
}

}  // namespace pbsim

extern "C" int64_t pbsim_stats_report(const int64_t counts[10], const int64_t len_row[16], const int64_t totals[12], const int64_t hist_q[128],
                                      const int64_t hist_identity[1001], const int64_t hist_qacc[1001], char *buf, int64_t cap) {
  if (!counts || !len_row || !totals || !hist_q || !hist_identity || !hist_qacc || cap < 0) return -1;
  const std::string text = pbsim::stats_report_text(counts, len_row, totals, hist_q, hist_identity, hist_qacc);
  if (buf && cap >= (int64_t)text.size()) memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}
