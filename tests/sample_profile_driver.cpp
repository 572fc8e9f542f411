// The host's stdio parse of a --sample FASTQ (read_sample_fastq_stdio, pbsim3_amd/csrc/unit_io.cpp: fgets chunks as the
// reference reads them), printed for tests/test_gpu_sample_profile.py: the eight integers, the four doubles as their bits,
// the kept strings one per line into a file of their own -- or the error text.
//   sample_profile_driver FILE LEN_MIN LEN_MAX ACC_MIN ACC_MAX KEPT_OUT     (accuracies as C hex floats)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "unit_io.h"

static unsigned long long bits(double d) {
  unsigned long long u;
  memcpy(&u, &d, sizeof u);
  return u;
}

int main(int argc, char **argv) {
  if (argc != 7) return 2;
  pbsim::SampleProfile p;
  std::string e;
  if (!pbsim::read_sample_fastq_stdio(argv[1], atol(argv[2]), atol(argv[3]), strtod(argv[4], nullptr), strtod(argv[5], nullptr), &p, &e)) {
    printf("error %s\n", e.c_str());
    return 0;
  }
  printf("ints %ld %ld %ld %lld %ld %ld %ld %lld\n", p.num, p.len_min, p.len_max, p.len_total, p.num_filtered, p.len_min_filtered,
         p.len_max_filtered, p.len_total_filtered);
  printf("bits %016llx %016llx %016llx %016llx\n", bits(p.len_mean_filtered), bits(p.len_sd_filtered), bits(p.accuracy_mean_filtered),
         bits(p.accuracy_sd_filtered));
  FILE *f = fopen(argv[6], "wb");
  if (!f) return 3;
  for (const std::string &q : p.quals) {
    fwrite(q.data(), 1, q.size(), f);
    fputc('\n', f);
  }
  return fclose(f) == 0 ? 0 : 3;
}
