// vcf_apply.cpp -- pbsim_vcf_apply: the lines of a VCF applied to a genome, per haplotype (the rule: include/pbsim3_amd.h,
// tests/apply_model.py).  The host's part: the genome into HBM as the BAM stages hold it (load_genome, bam_genome.h); the contig
// names' sorted hash table (vcf_compare.h); the text into a buffer; the line table's sizes, the tiles' scan and the fill; the parse;
// the sort of (site, line) (bs_sort_pairs); the clusters from the max-scan of the lines' reach and the walk; the marks; the base
// pass's sizes, the tiles' scan, the FASTA and the origin map; the tally with the annotated text's sizes, the scan again, the header
// -- written here -- and the lines behind it; both texts to the sink (deliver_text), then the records and their origin maps.  The
// kernels are vcf_apply.hip's.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "bam_errors.h"
#include "bam_genome.h"
#include "bam_sort.h"
#include "genome_mutate.h"
#include "kernels.h"
#include "vcf_apply.h"

namespace pbsim {

namespace {

const char kWho[] = "pbsim_vcf_apply: ";
const BamStage kStage = {kWho, "the stage holds the genome at 2 bytes per base, the VCF text, 105 bytes per data line, the sort's scratch, two 4-byte marks and one 8-byte end per position, the texts and, where the origin map is asked for, 4 bytes per written base in HBM at once, and does not chunk"};

int alloc(DevBuf &b, int64_t n, const char *what) { return bam_stage_alloc(kStage, b, n, what); }

int apply_vcf(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const std::vector<std::string> &used, const void *vcf, int64_t n_vcf,
              const pbsim_apply_opts &o, const pbsim_apply_sink *sink, pbsim_apply_result *result) {
  hipStream_t st = c->stream;
  BamPhases ph(st, "apply");
  const bool want_fasta = sink && sink->on_fasta, want_text = sink && sink->on_text, want_origin = sink && sink->on_origin;
  Genome genome;
  if (!load_genome(c, kStage, refs, n_refs, &genome)) return PBSIM_FAILED;
  ph.mark("genome");
  const int64_t total = genome.total, pos_tiles = (total + kApPosTile - 1) / kApPosTile;
  int64_t bases_in = 0;
  for (int r = 0; r < n_refs; r++) {
    if (genome.len[(size_t)r] >= kApMaxBases)
      return fail(std::string(kWho) + "genome record " + std::to_string(r) + " (" + refs[r].name + ") has " + std::to_string(genome.len[(size_t)r]) +
                  " bases: a record must have fewer than " + std::to_string(kApMaxBases));
    bases_in += genome.len[(size_t)r];
  }
  // ---- the names (the VCF's for the lookup, the records' own for the FASTA) and the text
  std::vector<uint64_t> hash;
  std::vector<int32_t> record;
  compare_name_table(used, &hash, &record);
  std::string names, own_names;
  std::vector<int64_t> name_at, own_at;
  for (int r = 0; r < n_refs; r++) {
    name_at.push_back((int64_t)names.size()), own_at.push_back((int64_t)own_names.size());
    names += used[(size_t)r], own_names += refs[r].name;
  }
  name_at.push_back((int64_t)names.size()), own_at.push_back((int64_t)own_names.size());
  const int64_t tiles = (n_vcf + kApTile - 1) / kApTile;
  DevBuf d_at, d_len, d_hash, d_record, d_name_at, d_names, d_own_at, d_own, d_bytes, d_tile, d_scan_tmp, d_cells, d_rec_n, d_part, d_base_at, d_byte_at;
  if (!alloc(d_at, n_refs * 8, "the genome records' places") || !alloc(d_len, n_refs * 8, "the genome records' lengths") ||
      !alloc(d_hash, n_refs * 8, "the names' hashes") || !alloc(d_record, n_refs * 4, "the names' records") ||
      !alloc(d_name_at, (n_refs + 1) * 8, "the contigs' names") || !alloc(d_names, (int64_t)names.size() + 1, "the contigs' names") ||
      !alloc(d_own_at, (n_refs + 1) * 8, "the genome records' names") || !alloc(d_own, (int64_t)own_names.size() + 1, "the genome records' names") ||
      !alloc(d_bytes, tiles * kApTile + 64, "the VCF text") || !alloc(d_tile, (std::max(tiles, pos_tiles) + 1) * 8, "the tiles") ||
      !alloc(d_scan_tmp, (std::max(tiles, pos_tiles) / 1024 + 8) * 8, "the scan's scratch") || !alloc(d_cells, kApCells * 8, "the counts") ||
      !alloc(d_rec_n, (int64_t)n_refs * 8, "the genome records' lines") || !alloc(d_part, n_refs * 8, "the genome records' parts") ||
      !alloc(d_base_at, (n_refs + 1) * 8, "the genome records' bases") || !alloc(d_byte_at, n_refs * 8, "the genome records' bytes"))
    return PBSIM_FAILED;
  HIP_OK(hipMemcpyAsync(d_at.p, genome.at.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_len.p, genome.len.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_hash.p, hash.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_record.p, record.data(), (size_t)n_refs * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_name_at.p, name_at.data(), name_at.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_names.p, names.data(), names.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_own_at.p, own_at.data(), own_at.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_own.p, own_names.data(), own_names.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(d_bytes.p, 0, (size_t)(tiles * kApTile + 64), st));
  if (n_vcf > 0) HIP_OK(hipMemcpyAsync(d_bytes.p, vcf, (size_t)n_vcf, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(d_cells.p, 0, kApCells * 8, st));
  HIP_OK(hipMemsetAsync(d_rec_n.p, 0, (size_t)n_refs * 8, st));
  const ApText text = {d_bytes.as<uint8_t>(), n_vcf, tiles};
  const CmpGenome g = {n_refs, d_at.as<int64_t>(), d_len.as<int64_t>(), genome.seq.as<uint8_t>(), d_hash.as<uint64_t>(), d_record.as<int32_t>(),
                       d_name_at.as<int64_t>(), d_names.as<char>()};
  // (hp is not read: the stage has no use for the homopolymer classes)
  const PileGenome pg = {n_refs, total, d_at.as<int64_t>(), d_len.as<int64_t>(), d_own_at.as<int64_t>(), d_own.as<char>(), genome.seq.as<uint8_t>(), nullptr};
  unsigned long long *cells = d_cells.as<unsigned long long>();
  int64_t *tile = d_tile.as<int64_t>();
  HIP_OK(hipStreamSynchronize(st));  // (the caller's text has been read)
  ph.mark("upload");
  // ---- the line table
  launch_apply_line_sizes(text, tile, st);
  HIP_OK(hipGetLastError());
  launch_exclusive_scan_i64(tile, tile, tiles, d_scan_tmp.as<int64_t>(), tile + tiles, st);
  HIP_OK(hipGetLastError());
  int64_t n_lines = 0;
  HIP_OK(hipMemcpyAsync(&n_lines, tile + tiles, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (n_lines >= kApMaxLines)
    return fail(std::string(kWho) + "the file has " + std::to_string(n_lines) + " data lines: it must have fewer than " + std::to_string(kApMaxLines));
  const int64_t line_tiles = (n_lines + kApLineTile - 1) / kApLineTile;
  DevBuf d_line, d_key, d_val, d_key2, d_val2, d_sort_tmp, d_reach, d_reach_tile, d_start, d_text_tile, d_text_tmp;
  if (!alloc(d_line, n_lines * (int64_t)sizeof(ApLine), "the lines") || !alloc(d_key, n_lines * 8, "the lines' sites") ||
      !alloc(d_val, n_lines * 4, "the lines' numbers") || !alloc(d_key2, n_lines * 8, "the sorted sites") ||
      !alloc(d_val2, n_lines * 4, "the sorted lines") || !alloc(d_reach, n_lines * 8, "the lines' reach") ||
      !alloc(d_reach_tile, (line_tiles + 1) * 8, "the tiles' reach") || !alloc(d_start, n_lines, "the clusters' starts") ||
      !alloc(d_text_tile, (line_tiles + 1) * 8, "the text's tiles") || !alloc(d_text_tmp, (line_tiles / 1024 + 8) * 8, "the scan's scratch"))
    return PBSIM_FAILED;
  ApLine *line = d_line.as<ApLine>();
  launch_apply_line_fill(text, tile, line, st);
  HIP_OK(hipGetLastError());
  ph.mark("lines");
  // ---- parse, sort, the collisions
  launch_apply_parse(text, g, line, n_lines, o.haplotype, o.sample, d_key.as<uint64_t>(), d_val.as<uint32_t>(), cells, st);
  HIP_OK(hipGetLastError());
  ph.mark("parse");
  if (n_lines > 0) {
    int end_bit = 33;  // the keys go up to n_refs << 33
    while (end_bit < 64 && ((uint64_t)n_refs >> (end_bit - 33)) != 0) end_bit++;
    size_t tb = 0;
    HIP_OK(bs_sort_pairs(nullptr, &tb, d_key.as<uint64_t>(), d_key2.as<uint64_t>(), d_val.as<uint32_t>(), d_val2.as<uint32_t>(), n_lines, end_bit, st));
    if (!alloc(d_sort_tmp, (int64_t)tb, "the sort's scratch")) return PBSIM_FAILED;
    HIP_OK(bs_sort_pairs(d_sort_tmp.p, &tb, d_key.as<uint64_t>(), d_key2.as<uint64_t>(), d_val.as<uint32_t>(), d_val2.as<uint32_t>(), n_lines, end_bit, st));
  }
  ph.mark("sort");
  const uint64_t *key = d_key2.as<uint64_t>();
  const uint32_t *val = d_val2.as<uint32_t>();
  launch_apply_reach(line, n_lines, key, val, n_refs, d_reach.as<unsigned long long>(), d_reach_tile.as<unsigned long long>(), st);
  HIP_OK(hipGetLastError());
  launch_apply_tile_scan(d_reach_tile.as<unsigned long long>(), line_tiles, st);
  HIP_OK(hipGetLastError());
  launch_apply_cluster(n_lines, key, n_refs, d_reach.as<unsigned long long>(), d_reach_tile.as<unsigned long long>(), d_start.as<uint8_t>(), st);
  HIP_OK(hipGetLastError());
  launch_apply_walk(line, n_lines, key, val, n_refs, d_start.as<uint8_t>(), cells, st);
  HIP_OK(hipGetLastError());
  ph.mark("collisions");
  // ---- the marks: the sort's buffers have been read
  HIP_OK(hipStreamSynchronize(st));
  d_key.release(), d_key2.release(), d_val.release(), d_val2.release(), d_sort_tmp.release(), d_reach.release(), d_reach_tile.release(), d_start.release();
  DevBuf d_ins_at, d_span_at, d_end, d_max;
  if (!alloc(d_ins_at, total * 4, "the positions' insertions") || !alloc(d_span_at, total * 4, "the positions' spans") ||
      !alloc(d_end, total * 8, "the spans' ends") || !alloc(d_max, (pos_tiles + 1) * 8, "the tiles' ends"))
    return PBSIM_FAILED;
  HIP_OK(hipMemsetAsync(d_ins_at.p, 0, (size_t)total * 4, st));
  HIP_OK(hipMemsetAsync(d_span_at.p, 0, (size_t)total * 4, st));
  HIP_OK(hipMemsetAsync(d_end.p, 0, (size_t)total * 8, st));
  HIP_OK(hipMemsetAsync(d_max.p, 0, (size_t)(pos_tiles + 1) * 8, st));
  const ApMarks marks = {d_ins_at.as<uint32_t>(), d_span_at.as<uint32_t>(), d_end.as<unsigned long long>(), d_max.as<unsigned long long>()};
  launch_apply_marks(line, n_lines, d_at.as<int64_t>(), marks, st);
  HIP_OK(hipGetLastError());
  launch_apply_tile_scan(marks.tile, pos_tiles, st);
  HIP_OK(hipGetLastError());
  ph.mark("marks");
  // ---- the bases: what every position emits, and where every record's bases and bytes begin
  launch_apply_base_sizes(pg, text, line, marks, d_part.as<int64_t>(), tile, cells, st);
  HIP_OK(hipGetLastError());
  launch_exclusive_scan_i64(tile, tile, pos_tiles, d_scan_tmp.as<int64_t>(), tile + pos_tiles, st);
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
    n_fasta += (own_at[(size_t)r + 1] - own_at[(size_t)r]) + 2 + n + (n == 0 ? 0 : o.line_width ? (n + o.line_width - 1) / o.line_width : 1);
    longest_out = std::max(longest_out, n);
    if (n >= kApMaxBases)
      return fail(std::string(kWho) + "genome record " + std::to_string(r) + " (" + refs[r].name + ") would have " + std::to_string(n) +
                  " bases: a written record must have fewer than " + std::to_string(kApMaxBases));
  }
  const int64_t bases_out = base_at[(size_t)n_refs];
  std::deque<FileText> fasta;
  DevBuf d_origin;
  if (want_fasta || want_origin) {
    char *out = nullptr;
    if (want_fasta) {
      fasta.emplace_back();
      fasta.back().n = n_fasta;
      if (!alloc(fasta.back().d, n_fasta, "the FASTA")) return PBSIM_FAILED;
      out = fasta.back().d.as<char>();
      HIP_OK(hipMemcpyAsync(d_byte_at.p, byte_at.data(), (size_t)n_refs * 8, hipMemcpyHostToDevice, st));
    }
    if (want_origin && !alloc(d_origin, bases_out * 4, "the origin map")) return PBSIM_FAILED;
    launch_apply_base_fill(pg, text, line, marks, o.line_width, d_base_at.as<int64_t>(), d_byte_at.as<int64_t>(), tile, out,
                           want_origin ? d_origin.as<int32_t>() : nullptr, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));  // (byte_at has been read)
    ph.mark("fasta");
  }
  // ---- the tally and the annotated text
  int64_t *text_tile = d_text_tile.as<int64_t>();
  launch_apply_text_sizes(text, line, n_lines, o.lines, text_tile, cells, d_rec_n.as<unsigned long long>(), st);
  HIP_OK(hipGetLastError());
  launch_exclusive_scan_i64(text_tile, text_tile, line_tiles, d_text_tmp.as<int64_t>(), text_tile + line_tiles, st);
  HIP_OK(hipGetLastError());
  int64_t n_body = 0;
  std::vector<uint64_t> h_cells(kApCells), h_rec_n((size_t)n_refs);
  if (line_tiles > 0) HIP_OK(hipMemcpyAsync(&n_body, text_tile + line_tiles, 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_cells.data(), d_cells.p, kApCells * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(h_rec_n.data(), d_rec_n.p, (size_t)n_refs * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ph.mark("tally");
  if (h_cells[kApCellTooLong] != 0)
    return fail(std::string(kWho) + std::to_string(h_cells[kApCellTooLong]) + " data lines are longer than " + std::to_string(kApMaxSpan) + " bytes");
  if (o.haplotype != 0 && n_lines > 0 && h_cells[kApCellHasSample] == 0)
    return fail(std::string(kWho) + "no data line has a sample column " + std::to_string(o.sample));
  const int64_t n_head = (int64_t)strlen(kApTextHeader), n_text = n_head + n_body;
  std::deque<FileText> texts;
  if (want_text) {
    texts.emplace_back();
    FileText &t = texts.back();
    t.n = n_text;
    if (!alloc(t.d, t.n, "the annotated text")) return PBSIM_FAILED;
    HIP_OK(hipMemcpyAsync(t.d.p, kApTextHeader, (size_t)n_head, hipMemcpyHostToDevice, st));
    launch_apply_text_fill(text, line, n_lines, o.lines, text_tile, t.d.as<char>() + n_head, st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st));
    ph.mark("text");
  }
  if (want_fasta && n_fasta > 0 && !deliver_text(st, kStage, fasta, n_fasta, o.piece_bytes, sink->on_fasta, sink->user)) return PBSIM_FAILED;
  if (want_text && !deliver_text(st, kStage, texts, n_text, o.piece_bytes, sink->on_text, sink->user)) return PBSIM_FAILED;
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
  auto cell = [&](int x) { return (int64_t)h_cells[(size_t)x]; };
  result->lines = cell(kApCellLines);
  result->malformed = cell(kApCellClass + kApMalformed), result->unknown_contig = cell(kApCellClass + kApUnknownContig);
  result->no_call = cell(kApCellClass + kApNoCall), result->ref_allele = cell(kApCellClass + kApRefAllele);
  result->unsupported = cell(kApCellClass + kApUnsupported), result->ref_mismatch = cell(kApCellClass + kApRefMismatch);
  result->filtered = cell(kApCellClass + kApFiltered), result->no_change = cell(kApCellClass + kApNoChange);
  result->overlap = cell(kApCellClass + kApOverlap), result->applied = cell(kApCellClass + kApApplied);
  for (int k = 0; k < kApTypes; k++) result->types[k] = cell(kApCellTypes + k);
  result->bases_in = bases_in, result->bases_out = bases_out;
  result->inserted = cell(kApCellInserted), result->deleted = cell(kApCellDeleted), result->substituted = cell(kApCellSubstituted);
  result->longest_cluster = cell(kApCellLongestCluster);
  result->fasta_bytes = n_fasta, result->text_bytes = n_text;
  if (result->lines != n_lines)
    return fail(std::string(kWho) + "the tally counted " + std::to_string(result->lines) + " data lines where the line table has " + std::to_string(n_lines));
  if (cell(kApCellBasesOut) != bases_out || bases_out != bases_in + result->inserted - result->deleted)
    return fail(std::string(kWho) + "the base pass counted " + std::to_string(cell(kApCellBasesOut)) + " bases where the tiles sum to " +
                std::to_string(bases_out) + " and the applied lines leave " + std::to_string(bases_in + result->inserted - result->deleted));
  {
    char sum[400];
    snprintf(sum, sizeof sum, "%d genome records, %lld positions in %lld tiles, %.3f MB of VCF, %lld data lines in %lld tiles, %lld applied, %lld bases out, "
             "%.1f MB of FASTA, %.3f MB of text", n_refs, (long long)bases_in, (long long)pos_tiles, n_vcf / 1e6, (long long)n_lines, (long long)line_tiles,
             (long long)result->applied, (long long)bases_out, n_fasta / 1e6, n_text / 1e6);
    ph.print(sum);
  }
  return PBSIM_SUCCEEDED;
}

}  // namespace
}  // namespace pbsim

extern "C" int pbsim_vcf_apply(pbsim_ctx *c, const pbsim_errors_ref *refs, int n_refs, const char *const *ref_names, const void *vcf, int64_t n_vcf,
                               const pbsim_apply_opts *opts, const pbsim_apply_sink *sink, pbsim_apply_result *result) {
  using pbsim::fail;
  if (!c || !refs || n_refs < 1 || !result || n_vcf < 0 || (n_vcf > 0 && !vcf)) return fail("pbsim_vcf_apply: bad argument");
  pbsim_apply_opts o;
  std::string err;
  std::vector<std::string> used;
  if (!pbsim::apply_check_opts(opts, &o, &err) || !pbsim::errors_check_genome(refs, n_refs, &err)) return fail("pbsim_vcf_apply: " + err);
  std::vector<const char *> own((size_t)n_refs);
  for (int r = 0; r < n_refs; r++) own[(size_t)r] = refs[r].name;
  if (!pbsim::compare_check_names(own.data(), ref_names, n_refs, &used, &err)) return fail("pbsim_vcf_apply: " + err);
  memset(result, 0, sizeof *result);
  NEED_DEVICE(c);
  HIP_OK(hipSetDevice(c->device));
  const int ok = pbsim::apply_vcf(c, refs, n_refs, used, vcf, n_vcf, o, sink, result);
  if (!ok) {  // the context stays usable: nothing of this call is left in flight when its buffers have gone
    const std::string why = pbsim::g_err;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    pbsim::g_err = why;
    memset(result, 0, sizeof *result);
  }
  return ok;
}
