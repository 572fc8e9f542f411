// bam_eval.h -- pbsim_truth_bam_eval (bam_eval.cpp) in its parts.  The first half is free of HIP (bam_eval_rule.cpp): what the
// host decides by name and the report text, so that it compiles alone; the second is the device side (bam_eval.hip), left out
// where PBSIM_EVAL_NO_HIP is defined.  Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "bam_chain.h"

namespace pbsim {

// counts[] of pbsim_truth_bam_eval
enum : int {
  kEvalTruth = 0,
  kEvalQuery,
  kEvalPrimary,
  kEvalSecondary,
  kEvalSupplementary,
  kEvalUnknown,
  kEvalDuplicate,
  kEvalUnmapped,
  kEvalScored,
  kEvalCorrect,
  kEvalWrong,
  kEvalMissing,
  kEvalCounts
};

// The reference names of a header that bam_parse_header has accepted (h holds hd.first_record bytes at least): the bytes in
// front of the first NUL of each name.
void bam_ref_names(const uint8_t *h, const BamHeader &hd, std::vector<std::string> *names);

// References by name.  truth_names[f]: the names of truth file f; override_name[f]: nullptr or the name given to its only
// reference.  Every distinct truth name gets a number; truth_map[f][refID] and query_map[refID] are those numbers, -1 for a
// query reference that no truth file names.  false: *err says which file cannot take its override.
struct EvalRefTables {
  std::vector<std::vector<int32_t>> truth_map;
  std::vector<int32_t> query_map;
};
bool eval_ref_tables(const std::vector<std::vector<std::string>> &truth_names, const std::vector<const char *> &override_name,
                     const std::vector<std::string> &query_names, EvalRefTables *out, std::string *err);

// the truth file that holds truth record `index`: first_record[f] is the number of file f's first record (ascending, [0] = 0)
int eval_file_of(const std::vector<int64_t> &first_record, int64_t index);

// the report text (pbsim_eval_report)
std::string eval_report_text(const int64_t counts[kEvalCounts], const int64_t hist[512]);

}  // namespace pbsim

#ifndef PBSIM_EVAL_NO_HIP
#include <hip/hip_runtime.h>

namespace pbsim {

constexpr uint32_t kEvalNoRecord = 0xffffffffu;

// Per record r of one stream (rec[r] packed as pk, records at stream + offset): ptr[r] its address, hash[r] the hash of its
// read name (the l_read_name - 1 bytes in front of the NUL) under hash_mask, end[r] = pos + max(1, reference span of its
// CIGAR).  With ref_map (the truth): gref[r] = ref_map[refID] and idx[r] = first + r, where ptr, hash, end, gref and idx are
// the arrays of ALL truth records and `first` is the number of this stream's first record.
void launch_eval_keys(const uint8_t *stream, const uint64_t *rec, int64_t n_rec, BamPacking pk, uint64_t hash_mask, const int32_t *ref_map,
                      int64_t first, uint64_t *ptr, uint64_t *hash, int64_t *end, int32_t *gref, uint32_t *idx, hipStream_t s);
// sorted (hash, truth record) pairs: dup[0] = min over the pairs of equal names of (later record << 32 | earlier record),
// untouched (preset to all ones) where no name occurs twice
void launch_eval_duplicates(const uint64_t *key, const uint32_t *perm, const uint64_t *t_ptr, int64_t n_truth, unsigned long long *dup,
                            hipStream_t s);
// per query record: its class into cls[0..5) (primary, secondary, supplementary, unknown, known), and for a known primary
// atomicMin of its number into first[truth record] (preset to kEvalNoRecord)
void launch_eval_join(const uint64_t *q_ptr, const uint64_t *q_hash, int64_t n_query, const uint64_t *key, const uint32_t *perm,
                      const uint64_t *t_ptr, int64_t n_truth, uint32_t *first, unsigned long long *cls, hipStream_t s);
// per truth record: its verdict byte, res[0..4) += (missing, unmapped, correct, wrong), hist[2 mapq] += scored, [2 mapq + 1] += wrong
void launch_eval_verdict(const uint64_t *t_ptr, const int64_t *t_end, const int32_t *t_gref, const uint32_t *first, int64_t n_truth,
                         const uint64_t *q_ptr, const int64_t *q_end, const int32_t *query_map, int32_t n_query_ref, int32_t permille,
                         uint8_t *verdict, unsigned long long *res, unsigned long long *hist, hipStream_t s);

}  // namespace pbsim
#endif
