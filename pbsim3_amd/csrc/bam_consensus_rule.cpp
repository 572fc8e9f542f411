// bam_consensus_rule.cpp -- what pbsim_bam_consensus decides on the host, free of HIP (see bam_consensus.h): the option check and
// the report text (pbsim_consensus_report).  The options it shares with pbsim_bam_pileup are checked by that stage's check, and
// the report's first two lines are written by that stage's report (bam_pileup_rule.cpp).
#define PBSIM_CONSENSUS_NO_HIP
#define PBSIM_PILEUP_NO_HIP
#include "bam_consensus.h"

#include <stdio.h>
#include <string.h>

#include "bam_pileup.h"

namespace pbsim {

bool consensus_check_opts(const pbsim_consensus_opts *opts, pbsim_consensus_opts *out, std::string *err) {
  const pbsim_consensus_opts defaults = {0x900, 0, 0, 0, 1, 1024, 60, 0};
  *out = opts ? *opts : defaults;
  if (out->fill != 0 && out->fill != 1) {
    *err = "fill must be 0 (N) or 1 (the genome's base)";
    return false;
  }
  if (out->max_ins < 1 || out->max_ins > kConsMaxIns) {
    *err = "max_ins must be 1 .. 65535";
    return false;
  }
  if (out->line_width < 0 || out->line_width > kConsMaxWidth) {
    *err = "line_width must be 0 .. 1048576 (0: one line)";
    return false;
  }
  const pbsim_pileup_opts shared = {out->exclude_flags, out->min_mapq, out->min_baseq, 0, out->min_depth, out->piece_bytes};
  pbsim_pileup_opts done;
  if (!pileup_check_opts(&shared, &done, err)) return false;
  out->piece_bytes = done.piece_bytes;
  return true;
}

std::string consensus_report_text(const pbsim_consensus_result &r) {
  pbsim_pileup_result p;
  memset(&p, 0, sizeof p);
  memcpy(p.counts, r.counts, sizeof p.counts);
  memcpy(p.sites, r.sites, sizeof p.sites);
  const std::string head = pileup_report_text(p);
  std::string out = head.substr(0, head.find('\n', head.find('\n') + 1) + 1);  // the "#" line and the "S" line
  char line[100];
  out += "K";
  for (int k = 0; k < kConsBases; k++) {
    snprintf(line, sizeof line, "\t%lld", (long long)r.bases[k]);
    out += line;
  }
  snprintf(line, sizeof line, "\t%lld\t%lld\t%lld\n", (long long)r.ins_sites, (long long)r.ins_longest, (long long)r.ins_capped);
  out += line;
  for (int v = 0; v < kConsLenBins; v++) {
    if (!r.ins_len[v]) continue;
    snprintf(line, sizeof line, "IL\t%d\t%lld\n", v, (long long)r.ins_len[v]);
    out += line;
  }
  return out;
}

}  // namespace pbsim

extern "C" int64_t pbsim_consensus_report(const pbsim_consensus_result *result, char *buf, int64_t cap) {
  if (!result || cap < 0) return -1;
  const std::string text = pbsim::consensus_report_text(*result);
  if (buf && cap >= (int64_t)text.size()) memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}
