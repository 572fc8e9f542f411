// arrays.cpp -- pbsim_simulate_arrays: the reads of the context's current unit as device arrays (include/pbsim3_amd.h,
// pbsim_read_arrays) instead of FASTQ/SAM + MAF text.  The quota loops are the text drivers' own (simulate_wgs, engine.cpp;
// simulate_units_range, units.cpp); what differs is what a batch becomes once its quota cut is known: export_batch (sizes,
// the sink's alloc, the export kernels, asynchronous) and deliver_arrays (wait, statistics, the sink's on_batch).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "ctx.h"
#include "engine_internal.h"

using namespace pbsim;

static void fill_export_args(pbsim_ctx *c, ExportArgs *e, int64_t n_final) {
  Slot &sl = c->s();
  memset(e, 0, sizeof *e);
  e->first_read = sl.b_first;
  e->n_reads = n_final;
  e->pass_num = c->p.pass_num;
  e->is_qs = c->p.method == PBSIM_METHOD_QS;
  e->unit = (uint32_t)sl.ref.unit;
  e->len = sl.d_len.as<int32_t>();
  e->off = sl.d_off.as<int32_t>();
  e->out_len = sl.d_out_len.as<int32_t>();
  e->maf_len = sl.d_maf_len.as<int32_t>();
  e->nsub = sl.d_nsub.as<int32_t>();
  e->nins = sl.d_nins.as<int32_t>();
  e->ndel = sl.d_ndel.as<int32_t>();
  e->task_of_slot = sl.d_task_of_slot.as<int32_t>();
  e->wave_cap = sl.d_wave_cap.as<int32_t>();
  e->wave_off = sl.d_wave_off.as<int64_t>();
  e->scratch = sl.d_scratch.as<uint8_t>();
  e->task_off = sl.d_rt_len.as<int64_t>();
  if (c->p.strategy != PBSIM_STRATEGY_WGS) {
    e->read_unit = c->d_read_unit.as<int32_t>() + (sl.b_first - 1);
    e->read_minus = c->d_read_minus.as<uint8_t>() + (sl.b_first - 1);
  }
}

// every array the sink handed over lies in device memory of the context's device, 16-byte aligned (the kernels store
// whole 16-byte chunks)
static int check_array(const pbsim_ctx *c, const void *p, const char *name, bool required) {
  char buf[200];
  if (!p) {
    if (!required) return PBSIM_SUCCEEDED;
    snprintf(buf, sizeof buf, "pbsim_simulate_arrays: the sink's alloc left %s NULL", name);
    return fail(buf);
  }
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    snprintf(buf, sizeof buf, "pbsim_simulate_arrays: %s is not memory the HIP runtime knows (host memory?)", name);
    return fail(buf);
  }
  if (at.type != hipMemoryTypeDevice || at.device != c->device) {
    snprintf(buf, sizeof buf, "pbsim_simulate_arrays: %s is not device memory of device %d (type %d, device %d)", name,
             c->device, (int)at.type, at.device);
    return fail(buf);
  }
  if (reinterpret_cast<uintptr_t>(p) & 15) {
    snprintf(buf, sizeof buf, "pbsim_simulate_arrays: %s is not 16-byte aligned", name);
    return fail(buf);
  }
  return PBSIM_SUCCEEDED;
}

static int check_arrays(const pbsim_ctx *c, const pbsim_read_arrays &r, int64_t bases) {
  const bool b = bases > 0;  // (no bases: the per-base arrays may be empty)
  return check_array(c, r.seq, "seq", b) && check_array(c, r.qual, "qual", b) && check_array(c, r.ref_pos, "ref_pos", false) &&
         check_array(c, r.offsets, "offsets", true) && check_array(c, r.read_number, "read_number", true) &&
         check_array(c, r.pass_index, "pass_index", true) && check_array(c, r.unit, "unit", true) &&
         check_array(c, r.strand, "strand", true) && check_array(c, r.ref_start, "ref_start", true) &&
         check_array(c, r.ref_span, "ref_span", true) && check_array(c, r.n_sub, "n_sub", true) &&
         check_array(c, r.n_ins, "n_ins", true) && check_array(c, r.n_del, "n_del", true);
}

extern "C++" int pbsim::export_batch(pbsim_ctx *c, const pbsim_array_sink *sink, pbsim_batch_info *info) {
  Slot &sl = c->s();
  DeviceFlags *flags = sl.d_flags.as<DeviceFlags>();
  pbsim_batch_info bi = sl.b_info;
  const int64_t n_tasks = bi.n_final * c->p.pass_num;
  sl.b_exported = false;
  sl.stats_fetched = false;  // deliver_arrays fetches the counters behind the export
  if (n_tasks > 0) {
    HIP_OK(sl.d_rt_len.ensure((n_tasks + 1) * 8));
    HIP_OK(hipMemsetAsync(&flags->sums[1], 0, 5 * sizeof(int64_t), sl.stream));
    ExportArgs e;
    fill_export_args(c, &e, bi.n_final);
    launch_export_sizes(e, flags, sl.d_scan_tmp.as<int64_t>(), sl.stream);
    DeviceFlags f;
    if (!read_flags(c, &f)) return PBSIM_FAILED;
    bi.bases = f.sums[3];
    bi.ref_bases = f.sums[4];
    bi.maf_columns = f.sums[5];
    pbsim_read_arrays ra;
    memset(&ra, 0, sizeof ra);
    if (!sink->alloc(sink->user, n_tasks, bi.bases, &ra)) return fail("pbsim_simulate_arrays: the sink's alloc refused a batch");
    if (!check_arrays(c, ra, bi.bases)) return PBSIM_FAILED;
    e.bases = bi.bases;
    e.out.seq = ra.seq;
    e.out.qual = ra.qual;
    e.out.ref_pos = bi.bases > 0 ? ra.ref_pos : nullptr;
    e.out.offsets = ra.offsets;
    e.out.read_number = ra.read_number;
    e.out.pass_index = ra.pass_index;
    e.out.unit = ra.unit;
    e.out.strand = ra.strand;
    e.out.ref_start = ra.ref_start;
    e.out.ref_span = ra.ref_span;
    e.out.n_sub = ra.n_sub;
    e.out.n_ins = ra.n_ins;
    e.out.n_del = ra.n_del;
    launch_export(e, sl.b_slots_max, flags, sl.stream);
    HIP_OK(hipGetLastError());
    sl.b_exported = true;
  }
  sl.b_info = bi;
  sl.b_finalized = true;
  if (info) *info = bi;
  return PBSIM_SUCCEEDED;
}

extern "C++" int pbsim::deliver_arrays(pbsim_ctx *c, const pbsim_array_sink *sink) {
  Slot &sl = c->s();
  if (!sl.b_exported) return PBSIM_SUCCEEDED;  // (a batch without final tasks)
  sl.b_exported = false;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipStreamSynchronize(sl.stream));
  if (!c->defer_account && !pbsim_batch_account(c)) return PBSIM_FAILED;
  if (!sink->on_batch(sink->user, &sl.b_info)) return fail("pbsim_simulate_arrays: the sink's on_batch aborted the run");
  return PBSIM_SUCCEEDED;
}

extern "C" {

int pbsim_simulate_arrays(pbsim_ctx *c, const pbsim_array_sink *sink) {
  if (!c) return fail("bad argument");
  if (!sink || !sink->alloc || !sink->on_batch)
    return fail("pbsim_simulate_arrays: a sink with both callbacks (alloc, on_batch) is required");
  if (c->p.method == PBSIM_METHOD_SAMPLE)
    return fail("pbsim_simulate_arrays: the sampling method has no array output (its quality strings come from the sample "
                "profile; use pbsim_simulate_sample)");
  NEED_DEVICE(c);
  const BatchOutput out{nullptr, sink};
  if (c->p.strategy == PBSIM_STRATEGY_WGS) return simulate_wgs(c, out);
  if (!c->d_seq || c->n_units < 1) return fail("no transcripts/templates set");
  return simulate_units_range(c, 1, c->trans_reads, out);
}

}  // extern "C"
