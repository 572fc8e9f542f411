// bam_genome.cpp -- the genome into HBM, squeezed and prepared record by record (kernels.hip's k_lines_* and k_hp_*), and the
// way of a stage's text to its sink: what pbsim_bam_errors and pbsim_bam_pileup share (bam_genome.h).
#include "bam_genome.h"

#include <algorithm>
#include <string>

#include "kernels.h"

namespace pbsim {

int load_genome(pbsim_ctx *c, const BamStage &stage, const pbsim_errors_ref *refs, int n_refs, Genome *g) {
  hipStream_t st = c->stream;
  auto alloc = [&](DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(stage, b, n, what); };
  int64_t total = 0, longest = 0;
  for (int r = 0; r < n_refs; r++) {
    g->at.push_back(total);
    total += (refs[r].bytes + 63) / 64 * 64 + 64;
    longest = std::max(longest, refs[r].bytes);
  }
  g->total = total;
  const int64_t line_tiles = (longest + 4095) / 4096, hp_tiles = (longest + kHpTile - 1) / kHpTile;
  DevBuf d_lines, d_tmp, d_tiles, d_flags;
  if (!alloc(g->seq, total, "the genome's bases") || !alloc(g->hp, total, "the genome's homopolymer classes") ||
      !alloc(d_lines, longest + 64, "a genome record's lines") || !alloc(d_tmp, (line_tiles + 1 + line_tiles / 1024 + 16) * 8, "the squeeze's scratch") ||
      !alloc(d_tiles, (hp_tiles + 1) * 4 * 8, "the preparation's scratch") || !alloc(d_flags, (int64_t)sizeof(DeviceFlags), "the preparation's flags"))
    return PBSIM_FAILED;
  HIP_OK(hipMemsetAsync(g->seq.p, 0, (size_t)total, st));
  HIP_OK(hipMemsetAsync(g->hp.p, 0, (size_t)total, st));
  int64_t *tmp = d_tmp.as<int64_t>();
  for (int r = 0; r < n_refs; r++) {
    const int64_t bytes = refs[r].bytes;
    int64_t kept = 0;
    if (bytes > 0) {
      const int64_t n_tiles = (bytes + 4095) / 4096;
      HIP_OK(hipMemcpyAsync(d_lines.p, refs[r].lines, (size_t)bytes, hipMemcpyHostToDevice, st));
      launch_squeeze_lines(d_lines.as<uint8_t>(), bytes, g->seq.as<uint8_t>() + g->at[(size_t)r], tmp + 1, tmp + 1 + n_tiles + 1, tmp, st);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(&kept, tmp, 8, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));  // (the staging buffer is the next record's too)
    }
    g->len.push_back(kept);
    if (kept > 0) {
      const int64_t n = (kept + kHpTile - 1) / kHpTile;
      int64_t *t = d_tiles.as<int64_t>();
      HIP_OK(hipMemsetAsync(d_flags.p, 0, sizeof(DeviceFlags), st));
      launch_prepare_reference(g->seq.as<uint8_t>() + g->at[(size_t)r], g->hp.as<uint8_t>() + g->at[(size_t)r], 0, kept, t, t + (n + 1), t + 2 * (n + 1),
                               t + 3 * (n + 1), 0, d_flags.as<DeviceFlags>(), st);
      HIP_OK(hipGetLastError());
    }
  }
  HIP_OK(hipStreamSynchronize(st));  // (the scratch goes with this frame)
  return PBSIM_SUCCEEDED;
}

int deliver_text(hipStream_t st, const BamStage &stage, std::deque<FileText> &texts, int64_t n_text, int64_t piece_bytes,
                 int (*on_text)(void *user, const char *bytes, int64_t n, int64_t offset), void *user) {
  const int64_t piece = std::min(piece_bytes, n_text);
  HostBuf pinned[2];
  hipEvent_t done[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; k++) {
    if (pinned[k].ensure((size_t)piece) != hipSuccess) {
      (void)hipGetLastError();
      return fail(stage.who + "no pinned host memory for a piece of " + std::to_string(piece) + " bytes of text");
    }
  }
  struct Events {
    hipEvent_t *e;
    ~Events() {
      for (int k = 0; k < 2; k++)
        if (e[k]) (void)hipEventDestroy(e[k]);
    }
  } guard = {done};
  for (int k = 0; k < 2; k++) HIP_OK(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
  struct Piece {
    size_t f;
    int64_t at, n;
  };
  std::vector<Piece> pieces;
  for (size_t f = 0; f < texts.size(); f++)
    for (int64_t at = 0; at < texts[f].n; at += piece) pieces.push_back({f, at, std::min(piece, texts[f].n - at)});
  auto start_copy = [&](const Piece &p, int which) {
    hipError_t e = hipMemcpyAsync(pinned[which].p, texts[p.f].d.as<char>() + p.at, (size_t)p.n, hipMemcpyDeviceToHost, st);
    return e != hipSuccess ? e : hipEventRecord(done[which], st);
  };
  HIP_OK(start_copy(pieces[0], 0));
  int64_t offset = 0;
  for (size_t k = 0; k < pieces.size(); k++) {
    const int which = (int)(k & 1);
    if (k + 1 < pieces.size()) HIP_OK(start_copy(pieces[k + 1], which ^ 1));
    HIP_OK(hipEventSynchronize(done[which]));
    if (!on_text(user, (const char *)pinned[which].p, pieces[k].n, offset)) return fail("sink aborted (text)");
    offset += pieces[k].n;
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace pbsim
