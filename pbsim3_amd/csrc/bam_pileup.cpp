// bam_pileup.cpp -- pbsim_bam_pileup: the pileup of the aligned reads of BAM files against their genome (the rule:
// include/pbsim3_amd.h, tests/pileup_model.py).  The host's part has the flow of pbsim_bam_errors (bam_errors.cpp): the genome into
// HBM (bam_genome.cpp), the table zeroed, then per file its stream and records (bam_stream.cpp), the references by name
// (bam_errors_rule.cpp), the record pass and the segments (bam_errors.hip) and the column pass; then once the site pass, the text
// and its way to the sink; the per-file part up to the segments is pbsim_bam_consensus's too (bam_pileup_front.h); the kernels are inflate.hip's, bam_scan.hip's, bam_errors.hip's and bam_pileup.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "bam_genome.h"
#include "bam_pileup.h"
#include "bam_pileup_front.h"
#include "bam_scan.h"
#include "bam_stream.h"
#include "ctx.h"
#include "kernels.h"

namespace pbsim {

// One file up to its segments (bam_pileup_front.h): the flow of pbsim_bam_errors's first half.
int pileup_file_front(pbsim_ctx *c, const BamStage &stage, BamPhases &ph, const pbsim_errors_ref *refs, int n_refs, const Genome &genome,
                      const pbsim_errors_file *files, int f, int n_files, int32_t exclude_flags, int32_t min_mapq, unsigned long long *cells,
                      PileFile *pf) {
  hipStream_t st = c->stream;
  auto alloc = [&](DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(stage, b, n, what); };
  // ---- 1. the stream into HBM, and its records
  BamStream &s = pf->s;
  s.a_what = "a file";
  if (n_files > 1) s.what = "file " + std::to_string(f);
  const std::string where = stage.who + s.what + (s.what.empty() ? "" : ": ");
  if (!bam_inflate_stream(c, stage, (const uint8_t *)files[f].bam, files[f].n, &s)) return PBSIM_FAILED;
  ph.mark("inflate");
  {
    BamScan scan;
    if (!bam_locate(c, stage, &s, &scan, kBamScanAny, kBamSamplePacking)) return PBSIM_FAILED;
  }
  ph.mark("locate");
  const int64_t n_rec = pf->n_rec = (int64_t)s.rec.size();
  if (n_rec >= ((int64_t)1 << 32) - 1) return fail(where + std::to_string(n_rec) + " records: a file of 2^32 - 1 records or more is not taken (a segment names its record in 32 bits)");
  // ---- 2. its references, by name
  std::vector<int32_t> map;
  {
    std::string err;
    if (!errors_ref_map(refs, n_refs, s.ref_names, files[f].ref_name, "file " + std::to_string(f), &map, &err)) return fail(stage.who + err);
  }
  std::vector<int64_t> ref_at(std::max<size_t>(map.size(), 1), -1), ref_len(std::max<size_t>(map.size(), 1), 0);
  for (size_t r = 0; r < map.size(); r++) {
    if (map[r] < 0) continue;
    const int64_t have = genome.len[(size_t)map[r]];
    if (s.hd.ref_len[r] != have)
      return fail(where + "the reference \"" + (files[f].ref_name ? std::string(files[f].ref_name) : s.ref_names[r]) + "\" has l_ref " +
                  std::to_string(s.hd.ref_len[r]) + " in the file's header, and the genome's record of that name has " + std::to_string(have) +
                  " bases: this is not the genome the reads were aligned to");
    ref_at[r] = genome.at[(size_t)map[r]];
    ref_len[r] = have;
  }
  if (n_rec == 0) return PBSIM_SUCCEEDED;
  DevBuf &d_ref_at = pf->d_ref_at, &d_ref_len = pf->d_ref_len, &d_rec = pf->d_rec, &d_st = pf->d_st, &d_cig_at = pf->d_cig_at, &d_n_ops = pf->d_n_ops,
         &d_sums = pf->d_sums, &d_nm = pf->d_nm, &d_n_seg = pf->d_n_seg, &d_scan_tmp = pf->d_scan_tmp, &d_seg = pf->d_seg;
  if (!alloc(d_ref_at, (int64_t)ref_at.size() * 8, "the references' places") || !alloc(d_ref_len, (int64_t)ref_len.size() * 8, "the references' lengths") ||
      !alloc(d_rec, n_rec * 8, "the record list") || !alloc(d_st, n_rec, "the records' classes") || !alloc(d_cig_at, n_rec * 8, "the records' CIGARs") ||
      !alloc(d_n_ops, n_rec * 4, "the records' op counts") || !alloc(d_sums, n_rec * 32, "the records' CIGAR sums") ||
      !alloc(d_nm, n_rec * 8, "the records' NM values") || !alloc(d_n_seg, (n_rec + 1) * 8, "the records' segment counts") ||
      !alloc(d_scan_tmp, (n_rec / 1024 + 8) * 8, "the scan's scratch"))
    return PBSIM_FAILED;
  HIP_OK(hipMemcpyAsync(d_ref_at.p, ref_at.data(), ref_at.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_ref_len.p, ref_len.data(), ref_len.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_rec.p, s.rec.data(), (size_t)n_rec * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(d_sums.p, 0, (size_t)n_rec * 32, st));
  HIP_OK(hipMemsetAsync(d_nm.p, 0, (size_t)n_rec * 8, st));
  const ErrRefs er = pf->er = {(int32_t)map.size(), d_ref_at.as<int64_t>(), d_ref_len.as<int64_t>()};
  const ErrRecs recs = pf->recs = {s.bytes(),
                                   d_rec.as<uint64_t>(),
                                   n_rec,
                                   d_st.as<uint8_t>(),
                                   d_cig_at.as<int64_t>(),
                                   d_n_ops.as<uint32_t>(),
                                   d_sums.as<int64_t>(),
                                   d_nm.as<int64_t>(),
                                   d_n_seg.as<int64_t>(),
                                   nullptr};  // (the records' column counts are the errors stage's column pass's alone)
  // ---- 3. the records
  launch_errors_records(recs, er, exclude_flags, min_mapq, nullptr, cells, st);
  HIP_OK(hipGetLastError());
  uint64_t fault = 0;
  HIP_OK(hipMemcpyAsync(&fault, cells + kErrCellFault, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("records");
  if (fault != ~(uint64_t)0)
    return fail(where + "the record at inflated byte offset " + std::to_string(fault) +
                " is malformed: a CIGAR op code above 8, or an aux field that runs past the record or has an unknown type");
  // ---- 4. the segments and their columns
  int64_t &n_seg = pf->n_seg;
  launch_exclusive_scan_i64(recs.n_seg, recs.n_seg, n_rec, d_scan_tmp.as<int64_t>(), recs.n_seg + n_rec, st);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(&n_seg, recs.n_seg + n_rec, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (n_seg > 0) {
    if (!alloc(d_seg, n_seg * (int64_t)sizeof(ErrSegment), "the segments")) return PBSIM_FAILED;
    launch_errors_records(recs, er, exclude_flags, min_mapq, d_seg.as<ErrSegment>(), cells, st);
    HIP_OK(hipGetLastError());
    ph.mark("segments");
  }
  return PBSIM_SUCCEEDED;
}

namespace {

const char kWho[] = "pbsim_bam_pileup: ";
const BamStage kStage = {kWho, "the stage holds the genome at 2 bytes per base, the cells at 32 bytes per position, a class byte per position, one file's inflated stream and 69 bytes per record in HBM at once, and the text, and does not chunk"};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

int pileup_bam(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files, const pbsim_pileup_opts &o,
               const pbsim_pileup_sink *sink, pbsim_pileup_result *result) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "pileup");
  const bool want_text = sink && sink->on_text, want_cells = sink && sink->on_cells;
  Genome genome;
  if (!load_genome(c, kStage, refs, n_refs, &genome)) return PBSIM_FAILED;
  ph.mark("genome");
  const ErrGenome g = {genome.seq.as<uint8_t>(), genome.hp.as<uint8_t>()};
  const int64_t total = genome.total;
  // the table shares the genome's offsets: 64 positions and more of padding lie behind every record
  DevBuf d_table, d_cls, d_cells, d_pile;
  if (!alloc(d_table, total * kPileWidth * 4, "the cells of every position") || !alloc(d_cls, total, "the sites' classes") ||
      !alloc(d_cells, kErrCells * 8, "the record counts") || !alloc(d_pile, kPileCells * 8, "the counts"))
    return PBSIM_FAILED;
  uint32_t *table = d_table.as<uint32_t>();
  unsigned long long *cells = d_cells.as<unsigned long long>(), *pile = d_pile.as<unsigned long long>();
  HIP_OK(hipMemsetAsync(d_table.p, 0, (size_t)total * kPileWidth * 4, st));
  HIP_OK(hipMemsetAsync(d_cells.p, 0, kErrCells * 8, st));
  HIP_OK(hipMemsetAsync(cells + kErrCellFault, 0xff, 8, st));
  HIP_OK(hipMemsetAsync(d_pile.p, 0, kPileCells * 8, st));
  ph.mark("zero");
  int64_t n_all = 0, inflated = 0, segments = 0;
  for (int f = 0; f < n_files; f++) {
    PileFile pf;
    if (!pileup_file_front(c, kStage, ph, refs, n_refs, genome, files, f, n_files, o.exclude_flags, o.min_mapq, cells, &pf)) return PBSIM_FAILED;
    inflated += pf.s.N, n_all += pf.n_rec, segments += pf.n_seg;
    if (pf.n_seg > 0) {
      launch_pileup_columns(pf.recs, pf.er, g, pf.d_seg.as<ErrSegment>(), pf.n_seg, (uint32_t)o.min_baseq, table, pile, st);
      HIP_OK(hipGetLastError());
      ph.mark("columns");
    }
    HIP_OK(hipStreamSynchronize(st));  // the stream and the per-record arrays go with this frame
  }
  // ---- 5. the sites, once
  std::string names;
  std::vector<int64_t> name_at;
  for (int r = 0; r < n_refs; r++) {
    name_at.push_back((int64_t)names.size());
    names += refs[r].name;
  }
  name_at.push_back((int64_t)names.size());
  DevBuf d_at, d_len, d_name_at, d_names;
  if (!alloc(d_at, n_refs * 8, "the genome records' places") || !alloc(d_len, n_refs * 8, "the genome records' lengths") ||
      !alloc(d_name_at, (n_refs + 1) * 8, "the genome records' names") || !alloc(d_names, (int64_t)names.size() + 1, "the genome records' names"))
    return PBSIM_FAILED;
  HIP_OK(hipMemcpyAsync(d_at.p, genome.at.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_len.p, genome.len.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_name_at.p, name_at.data(), name_at.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, st));
  const PileGenome pg = {n_refs, total, d_at.as<int64_t>(), d_len.as<int64_t>(), d_name_at.as<int64_t>(), d_names.as<char>(), g.seq, g.hp};
  launch_pileup_sites(pg, table, o.min_depth, d_cls.as<uint8_t>(), pile, st);
  HIP_OK(hipGetLastError());
  ph.mark("sites");
  // ---- 6. the text
  std::deque<FileText> texts;
  int64_t n_text = 0;
  if (want_text) {
    const int64_t tiles = (total + kPileTile - 1) / kPileTile;
    DevBuf d_tile, d_scan_tmp;
    texts.emplace_back();
    FileText &t = texts.back();
    if (!alloc(d_tile, (tiles + 1) * 8, "the text's tiles") || !alloc(d_scan_tmp, (tiles / 1024 + 8) * 8, "the scan's scratch")) return PBSIM_FAILED;
    int64_t *tile = d_tile.as<int64_t>();
    launch_pileup_text_sizes(pg, table, d_cls.as<uint8_t>(), o.format, tile, st);
    HIP_OK(hipGetLastError());
    launch_exclusive_scan_i64(tile, tile, tiles, d_scan_tmp.as<int64_t>(), tile + tiles, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&t.n, tile + tiles, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (t.n > 0) {
      if (!alloc(t.d, t.n, "the text")) return PBSIM_FAILED;
      launch_pileup_text_fill(pg, table, d_cls.as<uint8_t>(), o.format, tile, t.d.as<char>(), st);
      HIP_OK(hipGetLastError());
    }
    n_text = t.n;
    HIP_OK(hipStreamSynchronize(st));  // (the tiles go with this frame)
    ph.mark("text");
  }
  std::vector<uint64_t> h_cells(kErrCells), h_pile(kPileCells);
  HIP_OK(hipMemcpyAsync(h_cells.data(), d_cells.p, kErrCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_pile.data(), d_pile.p, kPileCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (want_text && n_text > 0 && !deliver_text(st, kStage, texts, n_text, o.piece_bytes, sink->on_text, sink->user)) return PBSIM_FAILED;
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("deliver");
  if (want_cells) {
    std::vector<uint32_t> host;
    for (int r = 0; r < n_refs; r++) {
      const int64_t n = genome.len[(size_t)r] * kPileWidth;
      host.resize((size_t)std::max<int64_t>(n, 1));
      if (n > 0) HIP_OK(hipMemcpy(host.data(), table + genome.at[(size_t)r] * kPileWidth, (size_t)n * 4, hipMemcpyDeviceToHost));
      if (!sink->on_cells(sink->user, r, host.data(), genome.len[(size_t)r])) return fail("sink aborted (cells)");
    }
    ph.mark("cells");
  }
  // ---- what the caller is told
  const struct {
    int64_t *to;
    int from, n;
  } parts[] = {{result->sites, kPileCellSites, kPileSites},        {result->cell_sums, kPileCellSums, kPileWidth},
               {&result->ins_unanchored, kPileCellUnanchored, 1},  {&result->max_depth, kPileCellMaxDepth, 1},
               {result->hp_called, kPileCellHpCalled, kPileHp},    {result->hp_sub, kPileCellHpSub, kPileHp},
               {result->hp_del, kPileCellHpDel, kPileHp},          {result->hp_ins, kPileCellHpIns, kPileHp}};
  for (int k = 0; k < kPileCounts; k++) result->counts[k] = (int64_t)h_cells[(size_t)kErrCellCounts + (size_t)k];
  for (const auto &p : parts)
    for (int k = 0; k < p.n; k++) p.to[k] = (int64_t)h_pile[(size_t)p.from + (size_t)k];
  {
    char sum[300];
    snprintf(sum, sizeof sum, "%d genome records, %lld positions, %d files, %.1f MB inflated, %lld records, %lld segments, %lld columns, %.1f MB of text",
             n_refs, (long long)result->sites[kPsSites], n_files, inflated / 1e6, (long long)n_all, (long long)segments,
             (long long)(result->cell_sums[0] + result->cell_sums[1] + result->cell_sums[2] + result->cell_sums[3] + result->cell_sums[kPcOther] +
                         result->cell_sums[kPcDel] + result->cell_sums[kPcMasked]),
             n_text / 1e6);
    ph.print(sum);
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_bam_pileup(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files,
                                const pbsim_pileup_opts *opts, const pbsim_pileup_sink *sink, pbsim_pileup_result *result) {
  using pbsim::fail;
  if (!c || !refs || n_refs < 1 || !files || n_files < 1 || !result) return fail("pbsim_bam_pileup: bad argument");
  for (int f = 0; f < n_files; f++)
    if (files[f].n < 0 || (files[f].n > 0 && !files[f].bam)) return fail("pbsim_bam_pileup: bad argument");
  pbsim_pileup_opts o;
  std::string err;
  if (!pbsim::pileup_check_opts(opts, &o, &err) || !pbsim::errors_check_genome(refs, n_refs, &err)) return fail("pbsim_bam_pileup: " + err);
  memset(result, 0, sizeof *result);
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::pileup_bam(c, refs, n_refs, files, n_files, o, sink, result);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
    memset(result, 0, sizeof *result);
  }
  return ok;
}
