// bam_call_rule.cpp -- what pbsim_bam_call decides on the host, free of HIP (see bam_call.h): the option check, the VCF header
// and the report text (pbsim_call_report).  The options it shares with pbsim_bam_consensus are checked by that stage's check, and
// the report's first two lines are written by the pileup's report (bam_pileup_rule.cpp).
#define PBSIM_CALL_NO_HIP
#define PBSIM_CONSENSUS_NO_HIP
#define PBSIM_PILEUP_NO_HIP
#include "bam_call.h"

#include <stdio.h>
#include <string.h>

#include "bam_consensus.h"
#include "bam_pileup.h"

namespace pbsim {

bool call_check_opts(const pbsim_call_opts *opts, pbsim_call_opts *out, std::string *err) {
  const pbsim_call_opts defaults = {0x900, 0, 0, 1024, 1, 0};
  *out = opts ? *opts : defaults;
  const pbsim_consensus_opts shared = {out->exclude_flags, out->min_mapq, out->min_baseq, 1, out->min_depth, out->max_ins, 0, out->piece_bytes};
  pbsim_consensus_opts done;
  if (!consensus_check_opts(&shared, &done, err)) return false;
  out->piece_bytes = done.piece_bytes;
  return true;
}

std::string call_header_text(const char *const *names, const int64_t *lengths, int n) {
  std::string out = "##fileformat=VCFv4.2\n##source=pbsim3_amd\n";
  for (int r = 0; r < n; r++) out += std::string("##contig=<ID=") + names[r] + ",length=" + std::to_string((long long)lengths[r]) + ">\n";
  out += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Depth of the pile at the record's anchor: A + C + G + T + other + del\">\n"
         "##INFO=<ID=MS,Number=1,Type=Integer,Description=\"Minimum support: the smallest count behind a substituted, deleted or inserted base of the "
         "record\">\n"
         "##INFO=<ID=TYPE,Number=1,Type=String,Description=\"snv, ins, del or complex\">\n"
         "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
  return out;
}

std::string call_report_text(const pbsim_call_result &r) {
  pbsim_pileup_result p;
  memset(&p, 0, sizeof p);
  memcpy(p.counts, r.counts, sizeof p.counts);
  memcpy(p.sites, r.sites, sizeof p.sites);
  const std::string head = pileup_report_text(p);
  std::string out = head.substr(0, head.find('\n', head.find('\n') + 1) + 1);  // the "#" line and the "S" line
  const int64_t values[] = {r.variants,  r.types[kCtSnv], r.types[kCtIns], r.types[kCtDel],    r.types[kCtComplex], r.ref_bases,
                            r.alt_bases, r.longest_ref,   r.longest_alt,   r.unplaced_records, r.unplaced_sites};
  char item[32];
  out += "V";
  for (int64_t v : values) {
    snprintf(item, sizeof item, "\t%lld", (long long)v);
    out += item;
  }
  out += "\n";
  return out;
}

}  // namespace pbsim

extern "C" int64_t pbsim_call_report(const pbsim_call_result *result, char *buf, int64_t cap) {
  if (!result || cap < 0) return -1;
  const std::string text = pbsim::call_report_text(*result);
  if (buf && cap >= (int64_t)text.size()) memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}
