// bam_stream.h -- a whole BAM file brought into HBM and its records located, for the stages that read other people's files
// (bam_eval.cpp, bam_depth.cpp): the container (BGZF inflated on the GPU, one plain gzip stream by zlib on the host, or the
// uncompressed stream itself), the header, the scan's candidates (bam_scan.hip) and the chain over them (bam_chain.cpp), with
// what to say when one of them refuses the bytes.  Every message begins with the stage's own prefix.  Internal: nothing here is
// part of include/pbsim3_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "bam_chain.h"
#include "bam_scan.h"
#include "ctx.h"

namespace pbsim {

// who speaks: "pbsim_truth_bam_eval: ", and what the stage keeps in HBM, for the out-of-memory message's bracket
struct BamStage {
  std::string who;
  const char *holds;
};
int bam_stage_oom(const BamStage &g, const char *what, size_t want);
// a buffer of this call alone, exactly n bytes (256 at least)
int bam_stage_alloc(const BamStage &g, DevBuf &b, int64_t n, const char *what);

struct BamStream {
  std::string what;              // "truth file 0", "the query"; empty where the stage has one file only
  const char *a_what = "a query";  // in the refusal of 2^36 inflated bytes
  DevBuf d;
  int64_t N = 0, H = 0;  // inflated bytes; the first record's offset
  BamHeader hd;
  std::vector<std::string> ref_names;
  std::vector<uint64_t> rec;
  const uint8_t *bytes() const { return (const uint8_t *)d.p; }
};

// the container: src[0, n) into s->d (N bytes and kBamSlack zero bytes behind them); ends with the stream synchronised
int bam_inflate_stream(pbsim_ctx *c, const BamStage &g, const uint8_t *src, int64_t n, BamStream *s);
// the header (with every l_ref), then the records: s->hd, s->ref_names, s->H, s->rec packed as pk
int bam_locate(pbsim_ctx *c, const BamStage &g, BamStream *s, BamScan *scan, BamScanPolicy policy, BamPacking pk);

// The phases on the stream's own clock (PBSIM_TRACE): an event where each ends.  What the host does between two events -- the
// chain walk, the tables -- falls into the phase it belongs to, since the stream is idle meanwhile.
struct BamPhases {
  bool on = getenv("PBSIM_TRACE") != nullptr;
  hipStream_t st;
  const char *tag;  // "eval": the lines begin "[pbsim eval]"
  std::vector<hipEvent_t> ev;
  std::vector<std::string> name;
  BamPhases(hipStream_t s, const char *t) : st(s), tag(t) { mark(""); }
  ~BamPhases() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  void mark(const std::string &what) {
    if (!on) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    ev.push_back(e);
    name.push_back(what);
  }
  // one line per phase, then "total: <summary>"
  void print(const std::string &summary) {
    if (!on || ev.empty()) return;
    (void)hipEventSynchronize(ev.back());
    float total = 0;
    for (size_t k = 1; k < ev.size(); k++) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, ev[k - 1], ev[k]);
      total += ms;
      fprintf(stderr, "[pbsim %s] %9.2f ms  %s\n", tag, ms, name[k].c_str());
    }
    fprintf(stderr, "[pbsim %s] %9.2f ms  total: %s\n", tag, total, summary.c_str());
  }
};

}  // namespace pbsim
