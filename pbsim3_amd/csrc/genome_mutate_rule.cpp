// genome_mutate_rule.cpp -- what pbsim_genome_mutate decides on the host, free of HIP (see genome_mutate.h): the option check, the
// VCF header and the report text (pbsim_mutate_report).
#define PBSIM_MUTATE_NO_HIP
#include "genome_mutate.h"

#include <stdio.h>
#include <string.h>

namespace pbsim {

bool mutate_check_opts(const pbsim_mutate_opts *opts, pbsim_mutate_opts *out, std::string *err) {
  const pbsim_mutate_opts defaults = {1, 1000, 100, 100, 500000, 50, 60, 0};
  *out = opts ? *opts : defaults;
  const struct {
    const char *name;
    int32_t v;
  } rates[] = {{"snv_ppm", out->snv_ppm}, {"ins_ppm", out->ins_ppm}, {"del_ppm", out->del_ppm}};
  for (const auto &r : rates)
    if (r.v < 0 || r.v > 1000000) {
      *err = std::string(r.name) + " must be 0 .. 1000000";
      return false;
    }
  if ((int64_t)out->snv_ppm + out->ins_ppm + out->del_ppm > 1000000) {
    *err = "snv_ppm + ins_ppm + del_ppm must not be above 1000000";
    return false;
  }
  if (out->ext_ppm < 0 || out->ext_ppm > 999999) {
    *err = "ext_ppm must be 0 .. 999999";
    return false;
  }
  if (out->max_indel < 1 || out->max_indel > 65535) {
    *err = "max_indel must be 1 .. 65535";
    return false;
  }
  if (out->line_width < 0 || out->line_width > 1048576) {
    *err = "line_width must be 0 .. 1048576 (0: one line per record)";
    return false;
  }
  if (out->piece_bytes < 0) {
    *err = "piece_bytes must not be negative (0: the default)";
    return false;
  }
  if (out->piece_bytes == 0) out->piece_bytes = kMutDefaultPiece;
  return true;
}

std::string mutate_header_text(const pbsim_mutate_opts &o, const char *const *names, const int64_t *lengths, int n) {
  char line[200];
  snprintf(line, sizeof line, "##pbsim_mutate=seed=%u;snv_ppm=%d;ins_ppm=%d;del_ppm=%d;ext_ppm=%d;max_indel=%d\n", (unsigned)o.seed, (int)o.snv_ppm,
           (int)o.ins_ppm, (int)o.del_ppm, (int)o.ext_ppm, (int)o.max_indel);
  std::string out = std::string("##fileformat=VCFv4.2\n##source=pbsim3_amd\n") + line;
  for (int r = 0; r < n; r++) out += std::string("##contig=<ID=") + names[r] + ",length=" + std::to_string((long long)lengths[r]) + ">\n";
  out += "##INFO=<ID=TYPE,Number=1,Type=String,Description=\"snv, ins, del or complex\">\n"
         "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
  return out;
}

std::string mutate_report_text(const pbsim_mutate_result &r) {
  const int64_t values[] = {r.records,   r.bases_in, r.eligible, r.bases_out,   r.drawn[kMtSnv], r.drawn[kMtIns], r.drawn[kMtDel], r.void_del,
                            r.dropped,   r.merged,   r.substituted, r.inserted, r.deleted,       r.variants,      r.types[kMtSnv], r.types[kMtIns],
                            r.types[kMtDel], r.ref_bases, r.alt_bases, r.longest_ref, r.longest_alt, r.header_bytes, r.vcf_bytes, r.fasta_bytes};
  std::string out =
      "#\trecords\tbases_in\teligible\tbases_out\tdrawn_snv\tdrawn_ins\tdrawn_del\tvoid_del\tdropped\tmerged\tsubstituted\tinserted\tdeleted\tvariants\tsnv\t"
      "ins\tdel\tref_bases\talt_bases\tlongest_ref\tlongest_alt\theader_bytes\tvcf_bytes\tfasta_bytes\nM";
  char item[32];
  for (int64_t v : values) {
    snprintf(item, sizeof item, "\t%lld", (long long)v);
    out += item;
  }
  out += "\n";
  return out;
}

}  // namespace pbsim

extern "C" int64_t pbsim_mutate_report(const pbsim_mutate_result *result, char *buf, int64_t cap) {
  if (!result || cap < 0) return -1;
  const std::string text = pbsim::mutate_report_text(*result);
  if (buf && cap >= (int64_t)text.size()) memcpy(buf, text.data(), text.size());
  return (int64_t)text.size();
}
