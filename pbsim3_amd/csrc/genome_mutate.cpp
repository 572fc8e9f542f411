// genome_mutate.cpp -- pbsim_genome_mutate: a variant genome as FASTA and its truth variants as VCF, drawn from a genome and a seed
// (the rule: include/pbsim3_amd.h, tests/mutate_model.py).  The host's part: the genome into HBM as the BAM stages hold it
// (load_genome, bam_genome.h); the event pass; the deleted set as a max-scan of the deletion runs' ends; the base pass's sizes, the
// tiles' scan, the FASTA and the origin map; the line pass's sizes, the tiles' scan again, the header -- written here -- and the
// lines behind it; both texts to the sink (deliver_text), then the records and their origin maps.  The kernels are
// genome_mutate.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "bam_errors.h"
#include "bam_genome.h"
#include "genome_mutate.h"
#include "kernels.h"

namespace pbsim {

namespace {

const char kWho[] = "pbsim_genome_mutate: ";
const BamStage kStage = {kWho, "the stage holds the genome at 2 bytes per base, three bytes and one 8-byte end per position, the texts and, where the origin map is asked for, 4 bytes per written base in HBM at once, and does not chunk"};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

int mutate_genome(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_mutate_opts &o, const pbsim_mutate_sink *sink,
                  pbsim_mutate_result *result) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "mutate");
  const bool want_fasta = sink && sink->on_fasta, want_vcf = sink && sink->on_vcf, want_origin = sink && sink->on_origin;
  Genome genome;
  if (!load_genome(c, kStage, refs, n_refs, &genome)) return PBSIM_FAILED;
  ph.mark("genome");
  const int64_t total = genome.total, tiles = (total + kMutTile - 1) / kMutTile;
  int64_t bases_in = 0;
  for (int r = 0; r < n_refs; r++) {
    if (genome.len[(size_t)r] >= kMutMaxBases)
      return fail(std::string(kWho) + "genome record " + std::to_string(r) + " (" + refs[r].name + ") has " + std::to_string(genome.len[(size_t)r]) +
                  " bases: a record must have fewer than " + std::to_string(kMutMaxBases));
    bases_in += genome.len[(size_t)r];
  }
  std::string names;
  std::vector<int64_t> name_at;
  for (int r = 0; r < n_refs; r++) {
    name_at.push_back((int64_t)names.size());
    names += refs[r].name;
  }
  name_at.push_back((int64_t)names.size());
  DevBuf d_at, d_len, d_name_at, d_names, d_kind, d_ilen, d_end, d_max, d_tile, d_scan_tmp, d_cells, d_rec_n, d_part, d_base_at, d_byte_at;
  if (!alloc(d_at, n_refs * 8, "the genome records' places") || !alloc(d_len, n_refs * 8, "the genome records' lengths") ||
      !alloc(d_name_at, (n_refs + 1) * 8, "the genome records' names") || !alloc(d_names, (int64_t)names.size() + 1, "the genome records' names") ||
      !alloc(d_kind, total, "the positions' kinds") || !alloc(d_ilen, total * 2, "the indels' lengths") ||
      !alloc(d_end, total * 8, "the deletion runs' ends") || !alloc(d_max, tiles * 8, "the tiles' ends") || !alloc(d_tile, (tiles + 1) * 8, "the tiles") ||
      !alloc(d_scan_tmp, (tiles / 1024 + 8) * 8, "the scan's scratch") || !alloc(d_cells, kMutCells * 8, "the counts") ||
      !alloc(d_rec_n, (int64_t)n_refs * 8, "the genome records' variants") || !alloc(d_part, n_refs * 8, "the genome records' parts") ||
      !alloc(d_base_at, (n_refs + 1) * 8, "the genome records' bases") || !alloc(d_byte_at, n_refs * 8, "the genome records' bytes"))
    return PBSIM_FAILED;
  HIP_OK(hipMemcpyAsync(d_at.p, genome.at.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_len.p, genome.len.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_name_at.p, name_at.data(), name_at.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(d_cells.p, 0, kMutCells * 8, st));
  HIP_OK(hipMemsetAsync(d_rec_n.p, 0, (size_t)n_refs * 8, st));
  // (hp is not read: the stage has no use for the homopolymer classes)
  const PileGenome pg = {n_refs, total, d_at.as<int64_t>(), d_len.as<int64_t>(), d_name_at.as<int64_t>(), d_names.as<char>(), genome.seq.as<uint8_t>(),
                         nullptr};
  const MutSites sites = {d_kind.as<uint8_t>(), d_ilen.as<uint16_t>(), d_end.as<unsigned long long>(), d_max.as<unsigned long long>()};
  unsigned long long *cells = d_cells.as<unsigned long long>();
  int64_t *tile = d_tile.as<int64_t>();
  // ---- the events and the deleted set
  launch_mutate_events(pg, o, sites, cells, st);
  HIP_OK(hipGetLastError());
  ph.mark("events");
  launch_mutate_tile_scan(sites, tiles, st);
  HIP_OK(hipGetLastError());
  ph.mark("scan");
  // ---- the bases: what every position emits, and where every record's bases and bytes begin
  launch_mutate_base_sizes(pg, sites, d_part.as<int64_t>(), tile, cells, st);
  HIP_OK(hipGetLastError());
  launch_exclusive_scan_i64(tile, tile, tiles, d_scan_tmp.as<int64_t>(), tile + tiles, st);
  HIP_OK(hipGetLastError());
  launch_mutate_record_bases(pg, d_part.as<int64_t>(), tile, d_base_at.as<int64_t>(), st);
  HIP_OK(hipGetLastError());
  std::vector<int64_t> base_at((size_t)n_refs + 1), byte_at((size_t)n_refs);
  HIP_OK(hipMemcpyAsync(base_at.data(), d_base_at.p, ((size_t)n_refs + 1) * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("bases");
  int64_t n_fasta = 0, longest_out = 0;
  for (int r = 0; r < n_refs; r++) {
    const int64_t n = base_at[(size_t)r + 1] - base_at[(size_t)r];
    byte_at[(size_t)r] = n_fasta;
    n_fasta += (name_at[(size_t)r + 1] - name_at[(size_t)r]) + 2 + n + (n == 0 ? 0 : o.line_width ? (n + o.line_width - 1) / o.line_width : 1);
    longest_out = std::max(longest_out, n);
  }
  const int64_t bases_out = base_at[(size_t)n_refs];
  std::deque<FileText> fasta;
  DevBuf d_origin;
  if (want_fasta || want_origin) {
    char *text = nullptr;
    if (want_fasta) {
      fasta.emplace_back();
      fasta.back().n = n_fasta;
      if (!alloc(fasta.back().d, n_fasta, "the FASTA")) return PBSIM_FAILED;
      text = fasta.back().d.as<char>();
      HIP_OK(hipMemcpyAsync(d_byte_at.p, byte_at.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
    }
    if (want_origin && !alloc(d_origin, bases_out * 4, "the origin map")) return PBSIM_FAILED;
    launch_mutate_base_fill(pg, o, sites, d_base_at.as<int64_t>(), d_byte_at.as<int64_t>(), tile, text, want_origin ? d_origin.as<int32_t>() : nullptr, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));  // (byte_at has been read)
    ph.mark("fasta");
  }
  // ---- the lines: the base pass's tiles are free again
  int64_t n_lines = 0;
  launch_mutate_line_sizes(pg, sites, tile, cells, d_rec_n.as<unsigned long long>(), st);
  HIP_OK(hipGetLastError());
  launch_exclusive_scan_i64(tile, tile, tiles, d_scan_tmp.as<int64_t>(), tile + tiles, st);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(&n_lines, tile + tiles, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("lines");
  std::vector<const char *> name_of((size_t)n_refs);
  for (int r = 0; r < n_refs; r++) name_of[(size_t)r] = refs[r].name;
  const std::string header = mutate_header_text(o, name_of.data(), genome.len.data(), n_refs);
  const int64_t n_vcf = (int64_t)header.size() + n_lines;
  std::deque<FileText> vcf;
  if (want_vcf) {
    vcf.emplace_back();
    FileText &t = vcf.back();
    t.n = n_vcf;
    if (!alloc(t.d, t.n, "the VCF")) return PBSIM_FAILED;
    HIP_OK(hipMemcpyAsync(t.d.p, header.data(), header.size(), hipMemcpyHostToDevice, st));
    launch_mutate_line_fill(pg, o, sites, tile, t.d.as<char>() + header.size(), st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("vcf");
  }
  std::vector<uint64_t> h_cells(kMutCells), h_rec_n((size_t)n_refs);
  HIP_OK(hipMemcpyAsync(h_cells.data(), d_cells.p, kMutCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_rec_n.data(), d_rec_n.p, (size_t)n_refs * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (want_fasta && n_fasta > 0 && !deliver_text(st, kStage, fasta, n_fasta, o.piece_bytes, sink->on_fasta, sink->user)) return PBSIM_FAILED;
  if (want_vcf && !deliver_text(st, kStage, vcf, n_vcf, o.piece_bytes, sink->on_vcf, sink->user)) return PBSIM_FAILED;
  HIP_OK(hipStreamSynchronize(st));
  std::vector<int32_t> h_origin;
  if (want_origin) h_origin.resize((size_t)std::max<int64_t>(longest_out, 1));
  for (int r = 0; r < n_refs; r++) {
    const int64_t l_out = base_at[(size_t)r + 1] - base_at[(size_t)r];
    if (sink && sink->on_record && !sink->on_record(sink->user, r, genome.len[(size_t)r], l_out, (int64_t)h_rec_n[(size_t)r]))
      return fail("sink aborted (records)");
    if (!want_origin) continue;
    if (l_out > 0) HIP_OK(hipMemcpy(h_origin.data(), d_origin.as<int32_t>() + base_at[(size_t)r], (size_t)l_out * 4, hipMemcpyDeviceToHost));
    if (!sink->on_origin(sink->user, r, h_origin.data(), l_out)) return fail("sink aborted (origin)");
  }
  ph.mark("deliver");
  // ---- what the caller is told
  result->records = n_refs, result->bases_in = bases_in, result->eligible = (int64_t)h_cells[kMutCellEligible], result->bases_out = bases_out;
  for (int k = 0; k < kMutTypes; k++) result->drawn[k] = (int64_t)h_cells[(size_t)kMutCellDrawn + (size_t)k];
  result->void_del = (int64_t)h_cells[kMutCellVoidDel], result->dropped = (int64_t)h_cells[kMutCellDropped], result->merged = (int64_t)h_cells[kMutCellMerged];
  result->substituted = (int64_t)h_cells[kMutCellSubstituted], result->inserted = (int64_t)h_cells[kMutCellInserted];
  result->deleted = (int64_t)h_cells[kMutCellDeleted];
  result->variants = (int64_t)h_cells[kMutCellVariants];
  for (int k = 0; k < kMutTypes; k++) result->types[k] = (int64_t)h_cells[(size_t)kMutCellTypes + (size_t)k];
  result->ref_bases = (int64_t)h_cells[kMutCellRefBases], result->alt_bases = (int64_t)h_cells[kMutCellAltBases];
  result->longest_ref = (int64_t)h_cells[kMutCellLongestRef], result->longest_alt = (int64_t)h_cells[kMutCellLongestAlt];
  result->header_bytes = (int64_t)header.size(), result->vcf_bytes = n_vcf, result->fasta_bytes = n_fasta;
  if ((int64_t)h_cells[kMutCellBasesOut] != bases_out)
    return fail(std::string(kWho) + "the base pass counted " + std::to_string(h_cells[kMutCellBasesOut]) + " bases where the tiles sum to " +
                std::to_string(bases_out));
  {
    char sum[400];
    snprintf(sum, sizeof sum, "%d genome records, %lld positions in %lld tiles, %lld bases out, %lld variants, %.1f MB of FASTA, %.3f MB of VCF",
             n_refs, (long long)bases_in, (long long)tiles, (long long)bases_out, (long long)result->variants, n_fasta / 1e6, n_vcf / 1e6);
    ph.print(sum);
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_genome_mutate(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const pbsim_mutate_opts *opts, const pbsim_mutate_sink *sink,
                                   pbsim_mutate_result *result) {
  using pbsim::fail;
  if (!c || !refs || n_refs < 1 || !result) return fail("pbsim_genome_mutate: bad argument");
  pbsim_mutate_opts o;
  std::string err;
  if (!pbsim::mutate_check_opts(opts, &o, &err) || !pbsim::errors_check_genome(refs, n_refs, &err)) return fail("pbsim_genome_mutate: " + err);
  memset(result, 0, sizeof *result);
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::mutate_genome(c, refs, n_refs, o, sink, result);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
    memset(result, 0, sizeof *result);
  }
  return ok;
}
