// bam_consensus.cpp -- pbsim_bam_consensus: the consensus FASTA of the aligned reads of BAM files against their genome (the rule:
// include/pbsim3_amd.h, tests/consensus_model.py).  The host's part has the flow of pbsim_bam_pileup (bam_pileup.cpp): the genome
// into HBM, the table zeroed, then per file its front half (bam_file_front.h) and the column pass, which here also logs the
// inserted bases of the anchored I ops; the logs outlive their files, the streams do not.  Then once the site pass; the ins_sites
// compacted into slots, the logs tallied into the slots' cells; the base pass, the FASTA and its way to the sink.  The kernels are
// bam_errors.hip's, bam_pileup.hip's and bam_consensus.hip's.  Everything up to the base pass's first half is consensus_front
// (bam_consensus_front.h), which pbsim_bam_call goes through as well.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "bam_consensus.h"
#include "bam_consensus_front.h"
#include "bam_genome.h"
#include "bam_file_front.h"
#include "kernels.h"

namespace pbsim {

namespace {

const char kWho[] = "pbsim_bam_consensus: ";
const BamStage kStage = {kWho, "the stage holds the genome at 2 bytes per base, the cells at 32 bytes per position, a class byte per position, one file's inflated stream and 69 bytes per record, 8 bytes per inserted base of every file, 20 bytes per base of the insertions at the ins_sites in HBM at once, and the text, and does not chunk"};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

struct FileLog {
  DevBuf d;
  int64_t cap = 0, n = 0;
};

}  // namespace

int consensus_front(pbsim_ctx *c, const BamStage &stage, BamPhases &ph, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files,
                    int n_files, int32_t exclude_flags, int32_t min_mapq, int32_t min_baseq, int64_t min_depth, int32_t max_ins, ConsFront *out) {
  hipStream_t st = c->stream;
  auto alloc = [&](DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(stage, b, n, what); };
  ConsFront &fr = *out;
  Genome &genome = fr.genome;
  if (!load_genome(c, stage, refs, n_refs, &genome)) return PBSIM_FAILED;
  ph.mark("genome");
  const ErrGenome g = {genome.seq.as<uint8_t>(), genome.hp.as<uint8_t>()};
  const int64_t total = genome.total;
  DevBuf &d_table = fr.d_table, &d_cls = fr.d_cls, &d_cells = fr.d_cells, &d_pile = fr.d_pile, &d_cons = fr.d_cons;
  DevBuf d_counts;
  if (!alloc(d_table, total * kPileWidth * 4, "the cells of every position") || !alloc(d_cls, total, "the sites' classes") ||
      !alloc(d_cells, kErrCells * 8, "the record counts") || !alloc(d_pile, kPileCells * 8, "the counts") ||
      !alloc(d_cons, kConsCells * 8, "the base counts") || !alloc(d_counts, (int64_t)n_files * 16, "the logs' counters"))
    return PBSIM_FAILED;
  uint32_t *table = d_table.as<uint32_t>();
  unsigned long long *cells = d_cells.as<unsigned long long>(), *pile = d_pile.as<unsigned long long>(), *cons = d_cons.as<unsigned long long>();
  unsigned long long *counts = d_counts.as<unsigned long long>();  // per file: the most entries of its log, the entries asked for
  HIP_OK(hipMemsetAsync(d_table.p, 0, (size_t)total * kPileWidth * 4, st));
  HIP_OK(hipMemsetAsync(d_cells.p, 0, kErrCells * 8, st));
  HIP_OK(hipMemsetAsync(cells + kErrCellFault, 0xff, 8, st));
  HIP_OK(hipMemsetAsync(d_pile.p, 0, kPileCells * 8, st));
  HIP_OK(hipMemsetAsync(d_cons.p, 0, kConsCells * 8, st));
  HIP_OK(hipMemsetAsync(d_counts.p, 0, (size_t)n_files * 16, st));
  ph.mark("zero");
  int64_t &n_all = fr.n_all, &inflated = fr.inflated, &segments = fr.segments, &logged = fr.logged;
  std::deque<FileLog> logs;
  for (int f = 0; f < n_files; f++) {
    BamFileFront pf;
    if (!bam_file_front(c, stage, ph, refs, n_refs, genome, files, f, n_files, exclude_flags, min_mapq, cells, false, &pf)) return PBSIM_FAILED;
    inflated += pf.s.N, n_all += pf.n_rec, segments += pf.n_seg;
    if (pf.n_seg > 0) {
      // the log, sized from the CIGAR sums of the scored records: every inserted base can leave one entry
      logs.emplace_back();
      FileLog &log = logs.back();
      uint64_t most = 0, asked = 0;
      launch_consensus_log_size(pf.recs, counts + 2 * f, st);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(&most, counts + 2 * f, 8, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      log.cap = (int64_t)most;
      if (!alloc(log.d, log.cap * 8, "the log of inserted bases")) return PBSIM_FAILED;
      const ConsLog to = {log.d.as<unsigned long long>(), counts + 2 * f + 1, log.cap};
      launch_consensus_columns(pf.recs, pf.er, g, pf.d_seg.as<ErrSegment>(), pf.n_seg, (uint32_t)min_baseq, table, pile, to, (uint32_t)max_ins, st);
      HIP_OK(hipGetLastError());
      ph.mark("columns");
      HIP_OK(hipMemcpyAsync(&asked, counts + 2 * f + 1, 8, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      if ((int64_t)asked > log.cap)
        return fail(stage.who + "the column pass met " + std::to_string(asked) + " inserted bases where the records' CIGARs sum to " +
                    std::to_string(log.cap));
      log.n = (int64_t)asked;
      logged += log.n;
    }
    HIP_OK(hipStreamSynchronize(st));  // the stream and the per-record arrays go with this frame
  }
  // ---- the sites, once
  std::string &names = fr.names;
  std::vector<int64_t> &name_at = fr.name_at;
  for (int r = 0; r < n_refs; r++) {
    name_at.push_back((int64_t)names.size());
    names += refs[r].name;
  }
  name_at.push_back((int64_t)names.size());
  DevBuf &d_at = fr.d_at, &d_len = fr.d_len, &d_name_at = fr.d_name_at, &d_names = fr.d_names;
  if (!alloc(d_at, n_refs * 8, "the genome records' places") || !alloc(d_len, n_refs * 8, "the genome records' lengths") ||
      !alloc(d_name_at, (n_refs + 1) * 8, "the genome records' names") || !alloc(d_names, (int64_t)names.size() + 1, "the genome records' names"))
    return PBSIM_FAILED;
  HIP_OK(hipMemcpyAsync(d_at.p, genome.at.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_len.p, genome.len.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_name_at.p, name_at.data(), name_at.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, st));
  const PileGenome pg = fr.pg = {n_refs, total, d_at.as<int64_t>(), d_len.as<int64_t>(), d_name_at.as<int64_t>(), d_names.as<char>(), g.seq, g.hp};
  const uint8_t *cls = d_cls.as<uint8_t>();
  launch_pileup_sites(pg, table, min_depth, d_cls.as<uint8_t>(), pile, st);
  HIP_OK(hipGetLastError());
  ph.mark("sites");
  // ---- the slots: the ins_sites in order, the longest insertion logged at each, the cells behind them
  const int64_t tiles = fr.tiles = (total + kConsTile - 1) / kConsTile;
  DevBuf &d_tile = fr.d_tile, &d_scan_tmp = fr.d_scan_tmp, &d_pos = fr.d_pos, &d_slot_len = fr.d_slot_len, &d_slot_off = fr.d_slot_off,
         &d_slot_cell = fr.d_slot_cell;
  if (!alloc(d_tile, (tiles + 1) * 8, "the tiles") || !alloc(d_scan_tmp, (tiles / 1024 + 8) * 8, "the scan's scratch")) return PBSIM_FAILED;
  int64_t *tile = d_tile.as<int64_t>();
  int64_t n_slots = 0, &n_cells = fr.n_cells;
  launch_consensus_slot_sizes(pg, cls, tile, st);
  HIP_OK(hipGetLastError());
  launch_exclusive_scan_i64(tile, tile, tiles, d_scan_tmp.as<int64_t>(), tile + tiles, st);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(&n_slots, tile + tiles, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ConsSlots &slots = fr.slots = {n_slots, nullptr, nullptr, nullptr, nullptr};
  if (n_slots > 0) {
    DevBuf d_slot_tmp;
    if (!alloc(d_pos, n_slots * 8, "the ins_sites' places") || !alloc(d_slot_len, (n_slots + 1) * 8, "the insertions' lengths") ||
        !alloc(d_slot_off, (n_slots + 1) * 8, "the insertions' cells' places") || !alloc(d_slot_tmp, (n_slots / 1024 + 8) * 8, "the scan's scratch"))
      return PBSIM_FAILED;
    launch_consensus_slot_fill(pg, cls, tile, d_pos.as<int64_t>(), st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemsetAsync(d_slot_len.p, 0, (size_t)(n_slots + 1) * 8, st));
    slots.pos = d_pos.as<int64_t>(), slots.len = d_slot_len.as<int64_t>(), slots.off = d_slot_off.as<int64_t>();
    ph.mark("slots");
    for (const FileLog &log : logs) {
      launch_consensus_lengths(ConsLog{log.d.as<unsigned long long>(), nullptr, log.cap}, log.n, total, cls, slots, st);
      HIP_OK(hipGetLastError());
    }
    launch_exclusive_scan_i64(slots.len, d_slot_off.as<int64_t>(), n_slots, d_slot_tmp.as<int64_t>(), d_slot_off.as<int64_t>() + n_slots, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&n_cells, d_slot_off.as<int64_t>() + n_slots, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));  // (the scan's scratch goes with this frame)
    ph.mark("lengths");
    if (!alloc(d_slot_cell, n_cells * 5 * 4, "the insertions' cells")) return PBSIM_FAILED;
    HIP_OK(hipMemsetAsync(d_slot_cell.p, 0, (size_t)std::max<int64_t>(n_cells * 5 * 4, 1), st));
    slots.cell = d_slot_cell.as<uint32_t>();
    for (const FileLog &log : logs) {
      launch_consensus_tally(ConsLog{log.d.as<unsigned long long>(), nullptr, log.cap}, log.n, total, cls, slots, st);
      HIP_OK(hipGetLastError());
    }
    ph.mark("tally");
  }
  HIP_OK(hipStreamSynchronize(st));
  logs.clear();
  // ---- the bases: what every position emits, and where every record's bases and bytes begin
  DevBuf &d_part = fr.d_part, &d_base_at = fr.d_base_at, &d_byte_at = fr.d_byte_at;
  if (!alloc(d_part, n_refs * 8, "the genome records' parts") || !alloc(d_base_at, (n_refs + 1) * 8, "the genome records' bases") ||
      !alloc(d_byte_at, n_refs * 8, "the genome records' bytes"))
    return PBSIM_FAILED;
  const ConsRecords rec = fr.rec = {d_part.as<int64_t>(), d_base_at.as<int64_t>(), d_byte_at.as<int64_t>()};
  launch_consensus_base_sizes(pg, table, cls, slots, (uint32_t)max_ins, rec, tile, cons, st);
  HIP_OK(hipGetLastError());
  return PBSIM_SUCCEEDED;
}

namespace {

int consensus_bam(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files, const pbsim_consensus_opts &o,
                  const pbsim_consensus_sink *sink, pbsim_consensus_result *result) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "consensus");
  const bool want_text = sink && sink->on_text;
  ConsFront fr;
  if (!consensus_front(c, kStage, ph, refs, n_refs, files, n_files, o.exclude_flags, o.min_mapq, o.min_baseq, o.min_depth, o.max_ins, &fr)) return PBSIM_FAILED;
  const Genome &genome = fr.genome;
  const PileGenome &pg = fr.pg;
  const ConsSlots &slots = fr.slots;
  const ConsRecords &rec = fr.rec;
  const std::vector<int64_t> &name_at = fr.name_at;
  const uint8_t *cls = fr.d_cls.as<uint8_t>();
  int64_t *tile = fr.d_tile.as<int64_t>();
  const int64_t tiles = fr.tiles, n_all = fr.n_all, inflated = fr.inflated, segments = fr.segments, logged = fr.logged, n_slots = slots.n, n_cells = fr.n_cells;
  DevBuf &d_cells = fr.d_cells, &d_pile = fr.d_pile, &d_cons = fr.d_cons, &d_scan_tmp = fr.d_scan_tmp, &d_base_at = fr.d_base_at, &d_byte_at = fr.d_byte_at;
  launch_exclusive_scan_i64(tile, tile, tiles, d_scan_tmp.as<int64_t>(), tile + tiles, st);
  HIP_OK(hipGetLastError());
  launch_consensus_record_bases(pg, rec.part, tile, d_base_at.as<int64_t>(), st);
  HIP_OK(hipGetLastError());
  std::vector<int64_t> base_at((size_t)n_refs + 1), byte_at((size_t)n_refs);
  HIP_OK(hipMemcpyAsync(base_at.data(), d_base_at.p, ((size_t)n_refs + 1) * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("bases");
  int64_t n_text = 0;
  for (int r = 0; r < n_refs; r++) {
    const int64_t n = base_at[(size_t)r + 1] - base_at[(size_t)r];
    byte_at[(size_t)r] = n_text;
    n_text += (name_at[(size_t)r + 1] - name_at[(size_t)r]) + 2 + n + (n == 0 ? 0 : o.line_width ? (n + o.line_width - 1) / o.line_width : 1);
  }
  // ---- the text
  std::deque<FileText> texts;
  if (want_text) {
    texts.emplace_back();
    FileText &t = texts.back();
    t.n = n_text;
    if (!alloc(t.d, t.n, "the text")) return PBSIM_FAILED;
    HIP_OK(hipMemcpyAsync(d_byte_at.p, byte_at.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
    launch_consensus_base_fill(pg, cls, slots, o.fill, (int64_t)o.line_width, rec, tile, t.d.as<char>(), st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("text");
  }
  std::vector<uint64_t> h_cells(kErrCells), h_pile(kPileCells), h_cons(kConsCells);
  HIP_OK(hipMemcpyAsync(h_cells.data(), d_cells.p, kErrCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_pile.data(), d_pile.p, kPileCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_cons.data(), d_cons.p, kConsCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (want_text && n_text > 0 && !deliver_text(st, kStage, texts, n_text, o.piece_bytes, sink->on_text, sink->user)) return PBSIM_FAILED;
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("deliver");
  if (sink && sink->on_record)
    for (int r = 0; r < n_refs; r++)
      if (!sink->on_record(sink->user, r, genome.len[(size_t)r], base_at[(size_t)r + 1] - base_at[(size_t)r])) return fail("sink aborted (records)");
  // ---- what the caller is told
  for (int k = 0; k < kPileCounts; k++) result->counts[k] = (int64_t)h_cells[(size_t)kErrCellCounts + (size_t)k];
  for (int k = 0; k < kPileSites; k++) result->sites[k] = (int64_t)h_pile[(size_t)kPileCellSites + (size_t)k];
  result->ins_unanchored = (int64_t)h_pile[kPileCellUnanchored];
  result->max_depth = (int64_t)h_pile[kPileCellMaxDepth];
  for (int k = 0; k < kConsBases; k++) result->bases[k] = (int64_t)h_cons[(size_t)kConsCellBases + (size_t)k];
  result->ins_sites = (int64_t)h_cons[kConsCellInsSites];
  result->ins_longest = (int64_t)h_cons[kConsCellLongest];
  result->ins_capped = (int64_t)h_cons[kConsCellCapped];
  for (int k = 0; k < kConsLenBins; k++) result->ins_len[k] = (int64_t)h_cons[(size_t)kConsCellInsLen + (size_t)k];
  result->text_bytes = n_text;
  {
    char sum[400];
    snprintf(sum, sizeof sum,
             "%d genome records, %lld positions, %d files, %.1f MB inflated, %lld records, %lld segments, %lld log entries (%.1f MB), %lld ins_sites, "
             "%lld insertion cells, %lld bases, %.1f MB of text",
             n_refs, (long long)result->sites[kPsSites], n_files, inflated / 1e6, (long long)n_all, (long long)segments, (long long)logged, logged * 8 / 1e6,
             (long long)n_slots, (long long)n_cells, (long long)result->bases[kCbOut], n_text / 1e6);
    ph.print(sum);
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_bam_consensus(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files,
                                   const pbsim_consensus_opts *opts, const pbsim_consensus_sink *sink, pbsim_consensus_result *result) {
  using pbsim::fail;
  if (!c || !refs || n_refs < 1 || !files || n_files < 1 || !result) return fail("pbsim_bam_consensus: bad argument");
  for (int f = 0; f < n_files; f++)
    if (files[f].n < 0 || (files[f].n > 0 && !files[f].bam)) return fail("pbsim_bam_consensus: bad argument");
  pbsim_consensus_opts o;
  std::string err;
  if (!pbsim::consensus_check_opts(opts, &o, &err) || !pbsim::errors_check_genome(refs, n_refs, &err)) return fail("pbsim_bam_consensus: " + err);
  memset(result, 0, sizeof *result);
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::consensus_bam(c, refs, n_refs, files, n_files, o, sink, result);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
    memset(result, 0, sizeof *result);
  }
  return ok;
}
