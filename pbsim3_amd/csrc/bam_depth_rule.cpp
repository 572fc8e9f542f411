// bam_depth_rule.cpp -- what pbsim_bam_depth decides on the host, free of HIP (see bam_depth.h): the option check, the offset
// table of the references, and the report text (pbsim_depth_report).
#define PBSIM_DEPTH_NO_HIP
#include "bam_depth.h"

#include <stdio.h>
#include <string.h>

namespace pbsim {

namespace {
const char *const kCountName[kDepthCounts] = {"records", "counted", "skipped_flag", "skipped_unplaced", "skipped_mapq", "clipped"};
}

bool depth_check_opts(const pbsim_depth_opts *opts, pbsim_depth_opts *out, std::string *err) {
  const pbsim_depth_opts defaults = {0x704, 0, 1, 0, 0, 0};
  *out = opts ? *opts : defaults;
  if (out->format != 0 && out->format != 1) {
    *err = "format must be 0 (bedgraph) or 1 (window)";
    return false;
  }
  if (out->format == 1 && out->window < 1) {
    *err = "window must be at least 1 with the window format";
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
  if (out->format == 0) out->window = 0;
  if (out->piece_bytes == 0) out->piece_bytes = kDepthDefaultPiece;
  return true;
}

bool depth_ref_offsets(const std::vector<int64_t> &ref_len, int64_t window, std::vector<int64_t> *off, std::vector<int64_t> *win,
                       std::string *err) {
  off->assign(1, 0);
  win->clear();
  if (window >= 1) win->push_back(0);
  for (size_t r = 0; r < ref_len.size(); r++) {
    const int64_t l = ref_len[r];
    if (l < 0) {
      *err = "reference " + std::to_string(r) + " has the negative length " + std::to_string(l);
      return false;
    }
    off->push_back(off->back() + l + 1);
    if (window >= 1) win->push_back(win->back() + (l + window - 1) / window);
  }
  return true;
}

std::string depth_report_text(const int64_t counts[kDepthCounts], int32_t n_ref, const char *const *names, const int64_t *rows,
                              const int64_t hist[256]) {
  std::string out = "#";
  char line[160];
  for (int k = 0; k < kDepthCounts; k++) {
    snprintf(line, sizeof line, " %s=%lld", kCountName[k], (long long)counts[k]);
    out += line;
  }
  out += "\n";
  for (int32_t r = 0; r < n_ref; r++) {
    const int64_t *row = rows + 4 * (int64_t)r;
    if (row[0] <= 0) continue;
    out += "R\t";
    out += names[r];
    snprintf(line, sizeof line, "\t%lld\t%lld\t%lld\t%lld\t%lld\n", (long long)row[0], (long long)row[1], (long long)row[2], (long long)row[3],
             (long long)depth_mean_milli(row[2], row[0]));
    out += line;
  }
  for (int d = 0; d < 256; d++) {
    if (hist[d] <= 0) continue;
    snprintf(line, sizeof line, "H\t%d\t%lld\n", d, (long long)hist[d]);
    out += line;
  }
  return out;
}

}  // namespace pbsim

extern "C" int64_t pbsim_depth_report(const int64_t counts[6], int32_t n_ref, const char *const *names, const int64_t *rows,
                                      const int64_t hist[256], char *buf, int64_t cap) {
  if (!counts || !hist || n_ref < 0 || cap < 0 || (n_ref > 0 && (!names || !rows))) return -1;
  for (int32_t r = 0; r < n_ref; r++)
    if (!names[r]) return -1;
  const std::string text = pbsim::depth_report_text(counts, n_ref, names, rows, hist);
  if (buf && cap >= (int64_t)text.size()) memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}
