// engine_internal.h -- helpers of engine.cpp that its siblings (deflate_host.cpp, units.cpp, sample.cpp) use.  Internal: nothing here is part of
// include/pbsim3_amd.h.
#pragma once
#include "ctx.h"

namespace pbsim {
int upload(DevBuf &b, const void *src, size_t n, hipStream_t s);
int ensure_header_tables(pbsim_ctx *c);
int ensure_qs_tabs(pbsim_ctx *c, bool hp11);
int ensure_class_tables(pbsim_ctx *c);
int read_flags(pbsim_ctx *c, DeviceFlags *f);  // the selected slot's flags, through pinned staging
// K0 of the context's current unit on its own stream (upper-case, homopolymer lengths, census into census_out), synchronous
int prepare_reference(pbsim_ctx *c, uint8_t *d_seq, int64_t len, int keep_first_case, int64_t census_out[kHpSlots]);
int64_t batch_capacity(const pbsim_ctx *c);  // reads a batch of the current unit is sized to
// the finalized batch of the selected slot to the sink (text or members), waiting for its text emission first when deferred
// (deflate_host.cpp)
int deliver(pbsim_ctx *c, const pbsim_sink *sink);

// What the drivers do with a batch once its quota cut is known (finalize_cut): emit its text and hand it to a pbsim_sink
// (finalize_text, deliver), or export its rows into the device arrays of a pbsim_array_sink (arrays.cpp).  Both quota loops,
// simulate_wgs (engine.cpp) and simulate_units_range (units.cpp), run either.
struct BatchOutput {
  const pbsim_sink *sink;            // text (may be null: the text stays in HBM)
  const pbsim_array_sink *arrays;    // non-null: arrays instead of text
};
int emit_batch(pbsim_ctx *c, const BatchOutput &o, pbsim_batch_info *info);  // on the selected slot, after finalize_cut
int deliver_batch(pbsim_ctx *c, const BatchOutput &o);
int simulate_wgs(pbsim_ctx *c, const BatchOutput &out);
int simulate_units_range(pbsim_ctx *c, int64_t first_read, int64_t n_reads, const BatchOutput &out);
// arrays.cpp: the sizes of the batch's final tasks, the sink's alloc, the export kernels (asynchronous) ...
int export_batch(pbsim_ctx *c, const pbsim_array_sink *sink, pbsim_batch_info *info);
// ... and, once they are through, the batch's statistics and the sink's on_batch
int deliver_arrays(pbsim_ctx *c, const pbsim_array_sink *sink);

// A driver that does not wait for a batch's text emission in finalize_text (the batch's statistics are added on the host
// meanwhile; deliver() waits before it hands text to a sink); every emission has landed when the driver returns.
struct DeferTextSync {
  pbsim_ctx *c;
  bool prev;
  explicit DeferTextSync(pbsim_ctx *ctx) : c(ctx), prev(ctx->defer_text_sync) { c->defer_text_sync = true; }
  ~DeferTextSync() {
    for (Slot &sl : c->slots)
      if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    c->defer_text_sync = prev;
  }
};
}  // namespace pbsim
