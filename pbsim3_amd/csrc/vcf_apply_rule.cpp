// vcf_apply_rule.cpp -- what pbsim_vcf_apply decides on the host, free of HIP (see vcf_apply.h): the option check, the sample's name
// looked up in the #CHROM line, the report text (pbsim_apply_report) and the annotated text's header.  The contig names and their
// hash table are vcf_compare_rule.cpp's.
#define PBSIM_APPLY_NO_HIP
#include "vcf_apply.h"

#include <stdio.h>
#include <string.h>

namespace pbsim {

const char kApTextHeader[] = "#line\tCHROM\tPOS\tREF\tALT\tallele\ttype\tstart\tref_len\talt\tverdict\tby\n";

bool apply_check_opts(const pbsim_apply_opts *opts, pbsim_apply_opts *out, std::string *err) {
  const pbsim_apply_opts defaults = {0, 0, 0, 60, 0};
  *out = opts ? *opts : defaults;
  if (out->haplotype < 0 || out->haplotype > 2) {
    *err = "haplotype must be 0 (the first ALT), 1 or 2";
    return false;
  }
  if (out->sample < 0) {
    *err = "sample must be 0 .. 2147483647";
    return false;
  }
  if (out->lines < 0 || out->lines > 1) {
    *err = "lines must be 0 (discordant) or 1 (all)";
    return false;
  }
  if (out->line_width < 0 || out->line_width > 1048576) {
    *err = "line_width must be 0 .. 1048576";
    return false;
  }
  if (out->piece_bytes < 0) {
    *err = "piece_bytes must not be negative (0: the default)";
    return false;
  }
  if (out->piece_bytes == 0) out->piece_bytes = kApDefaultPiece;
  return true;
}

int32_t apply_sample_column(const char *vcf, int64_t n, const char *name) {
  const size_t name_n = strlen(name);
  for (int64_t at = 0; at < n;) {
    const char *nl = (const char *)memchr(vcf + at, '\n', (size_t)(n - at));
    int64_t end = nl ? nl - vcf : n;
    const int64_t next = end + 1;
    if (end - at >= 6 && !memcmp(vcf + at, "#CHROM", 6)) {
      if (vcf[end - 1] == '\r') end--;
      int64_t col = 0, begin = at;
      for (int64_t k = at; k <= end; k++) {
        if (k < end && vcf[k] != '\t') continue;
        if (col >= 9 && (size_t)(k - begin) == name_n && !memcmp(vcf + begin, name, name_n)) return (int32_t)(col - 9);
        if (col - 9 >= 2147483647) return -1;
        col++, begin = k + 1;
      }
      return -1;
    }
    at = next;
  }
  return -1;
}

std::string apply_report_text(const pbsim_apply_result &r) {
  std::string out =
      "#\tlines\tmalformed\tunknown_contig\tno_call\tref_allele\tunsupported\tref_mismatch\tfiltered\tno_change\toverlap\tapplied\tsnv\tins\tdel\tcomplex"
      "\tbases_in\tbases_out\tinserted\tdeleted\tsubstituted\tlongest_cluster\tfasta_bytes\ttext_bytes\nA";
  const int64_t v[] = {r.lines,    r.malformed, r.unknown_contig, r.no_call,  r.ref_allele, r.unsupported, r.ref_mismatch, r.filtered,
                       r.no_change, r.overlap,   r.applied,        r.types[0], r.types[1],   r.types[2],    r.types[3],     r.bases_in,
                       r.bases_out, r.inserted,  r.deleted,        r.substituted, r.longest_cluster, r.fasta_bytes, r.text_bytes};
  char item[40];
  for (int64_t x : v) {
    snprintf(item, sizeof item, "\t%lld", (long long)x);
    out += item;
  }
  return out + "\n";
}

}  // namespace pbsim

extern "C" int64_t pbsim_apply_report(const pbsim_apply_result *result, char *buf, int64_t cap) {
  if (!result || cap < 0) return -1;
  const std::string text = pbsim::apply_report_text(*result);
  if (buf && cap >= (int64_t)text.size()) memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}

extern "C" int32_t pbsim_apply_sample(const void *vcf, int64_t n_vcf, const char *name) {
  if (n_vcf < 0 || (n_vcf > 0 && !vcf) || !name) return -1;
  return pbsim::apply_sample_column((const char *)vcf, n_vcf, name);
}
