// cli_stages.h -- the stand-alone modes of the `pbsim` binary (cli_stages.cpp), named once: the option that selects a mode and
// the function that runs it, in the order pbsim_cli_main looks for them (a line that names two of them goes to the earlier one).
// main.cpp takes the options' names from the same list; the macro alone links nothing.
#pragma once
#include "../../include/pbsim3_amd.h"

#define PBSIM_STAGE_MODES(X)              \
  X("--eval-bam", eval_bam_main)           \
  X("--depth-bam", depth_bam_main)         \
  X("--stats-bam", stats_bam_main)         \
  X("--errors-bam", errors_bam_main)       \
  X("--pileup-bam", pileup_bam_main)       \
  X("--consensus-bam", consensus_bam_main) \
  X("--call-bam", call_bam_main)           \
  X("--mutate-genome", mutate_genome_main) \
  X("--compare-vcf", compare_vcf_main)     \
  X("--apply-vcf", apply_vcf_main)         \
  X("--lift-bam", lift_bam_main)

namespace pbsim {
namespace cli {

struct StageMode {
  const char *option;
  int (*run)(int argc, char **argv, const pbsim_comm *comm, int device);
};
const StageMode *stage_modes();  // the list above; a row of nullptr ends it

}  // namespace cli
}  // namespace pbsim
