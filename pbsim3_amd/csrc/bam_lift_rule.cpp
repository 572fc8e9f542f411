// bam_lift_rule.cpp -- what pbsim_bam_lift decides on the host, free of HIP (see bam_lift.h): the argument check, the header
// rewritten for the original genome, what is wrong with an origin map, and the report text (pbsim_lift_report).
#define PBSIM_LIFT_NO_HIP
#include "bam_lift.h"

#include <stdio.h>
#include <string.h>

namespace pbsim {

bool lift_check_args(const pbsim_lift_origin *origins, int n_refs, const pbsim_errors_file *file, const pbsim_lift_sink *sink, std::string *err) {
  if (!origins || n_refs < 1 || !file || !sink) {
    *err = "bad argument";
    return false;
  }
  if (file->n < 0 || (file->n > 0 && !file->bam)) {
    *err = "bad argument";
    return false;
  }
  for (int r = 0; r < n_refs; r++) {
    if (origins[r].n < 0 || (origins[r].n > 0 && !origins[r].origin)) {
      *err = "origin map " + std::to_string(r) + " is missing";
      return false;
    }
    if (origins[r].n >= 2147483647) {
      *err = "origin map " + std::to_string(r) + " has " + std::to_string(origins[r].n) + " bases: a variant record must have fewer than 2147483647";
      return false;
    }
  }
  return true;
}

namespace {

void put32(std::string *o, uint32_t v) {
  for (int k = 0; k < 4; k++) o->push_back((char)(v >> (8 * k)));
}

// the tab-separated fields of a line
std::vector<std::string> fields_of(const std::string &line) {
  std::vector<std::string> f;
  for (size_t at = 0;;) {
    const size_t tab = line.find('\t', at);
    f.push_back(line.substr(at, tab == std::string::npos ? std::string::npos : tab - at));
    if (tab == std::string::npos) return f;
    at = tab + 1;
  }
}

std::string lift_text(const std::string &text, const std::vector<std::string> &names, const std::vector<int64_t> &new_len) {
  std::string out;
  bool first = true;
  for (size_t at = 0;; first = false) {
    const size_t nl = text.find('\n', at);
    const std::string line = text.substr(at, nl == std::string::npos ? std::string::npos : nl - at);
    std::vector<std::string> f = fields_of(line);
    if (first && f[0] == "@HD") {
      for (std::string &x : f)
        if (x.compare(0, 3, "SO:") == 0) x = "SO:unsorted";
    } else if (f[0] == "@SQ") {
      const std::string *sn = nullptr;
      for (size_t k = 1; k < f.size() && !sn; k++)
        if (f[k].compare(0, 3, "SN:") == 0) sn = &f[k];
      if (sn) {
        for (size_t r = 0; r < names.size(); r++) {
          if (sn->compare(3, std::string::npos, names[r]) != 0) continue;
          for (size_t k = 1; k < f.size(); k++)
            if (f[k].compare(0, 3, "LN:") == 0) f[k] = "LN:" + std::to_string(new_len[r]);
          break;
        }
      }
    }
    for (size_t k = 0; k < f.size(); k++) out += (k ? "\t" : "") + f[k];
    if (nl == std::string::npos) return out;
    out += '\n';
    at = nl + 1;
  }
}

}  // namespace

std::string lift_header(const uint8_t *h, int64_t n, int64_t l_text, const std::vector<std::string> &names, const std::vector<int64_t> &new_len) {
  std::string out("BAM\1", 4);
  const std::string text = lift_text(std::string((const char *)h + 8, (size_t)l_text), names, new_len);
  put32(&out, (uint32_t)text.size());
  out += text;
  int64_t at = 8 + l_text;
  out.append((const char *)h + at, 4);  // n_ref
  at += 4;
  for (size_t r = 0; r < names.size() && at + 4 <= n; r++) {
    uint32_t l_name = 0;
    for (int k = 0; k < 4; k++) l_name |= (uint32_t)h[at + k] << (8 * k);
    if (at + 8 + (int64_t)l_name > n) break;  // (never: the header was parsed)
    out.append((const char *)h + at, 4 + (size_t)l_name);
    put32(&out, (uint32_t)new_len[r]);
    at += 8 + (int64_t)l_name;
  }
  return out;
}

const char *lift_origin_fault(int kind) {
  return kind == kLiftBadRange   ? "a kept base names a position outside the original record"
         : kind == kLiftBadOrder ? "the kept bases' positions do not rise strictly"
                                 : "an inserted base does not name the last kept base in front of it";
}

std::string lift_report_text(const pbsim_lift_result &r) {
  std::string out =
      "#\trecords\tunaligned\tunsupported\tunplaced\tlifted\tmoved\tno_seq\tlong_cigar_in\tlong_cigar_out\tcols_in\tcols_out\tm\tins\tdel\tsoft\tsub"
      "\tgap_del\tbases_to_ins\tdels_vanished\tbytes_in\tbytes_out\nL";
  char item[40];
  for (int k = 0; k < kLiftCounts; k++) {
    snprintf(item, sizeof item, "\t%lld", (long long)r.counts[k]);
    out += item;
  }
  for (int k = 0; k < kLiftTotals; k++) {
    snprintf(item, sizeof item, "\t%lld", (long long)r.totals[k]);
    out += item;
  }
  return out + "\n";
}

}  // namespace pbsim

extern "C" int64_t pbsim_lift_report(const pbsim_lift_result *result, char *buf, int64_t cap) {
  if (!result || cap < 0) return -1;
  const std::string text = pbsim::lift_report_text(*result);
  if (buf && cap >= (int64_t)text.size()) memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}
