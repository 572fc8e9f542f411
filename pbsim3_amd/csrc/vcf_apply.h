// vcf_apply.h -- pbsim_vcf_apply (vcf_apply.cpp) in its parts.  The first half is free of HIP (vcf_apply_rule.cpp): the option check,
// the sample's name looked up in the #CHROM line, the report text and the annotated text's header, so that it compiles alone (the
// contig names and their hash table are vcf_compare.h's); the second is the device side (vcf_apply.hip), left out where
// PBSIM_APPLY_NO_HIP is defined.  Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

// a line's class byte: 0 applied, the classes in the order of pbsim_apply_result, kApOverlap behind them
enum : int { kApApplied = 0, kApMalformed, kApUnknownContig, kApNoCall, kApRefAllele, kApUnsupported, kApRefMismatch, kApFiltered, kApNoChange, kApOverlap,
             kApClasses };
// types[]
enum : int { kAtSnv = 0, kAtIns, kAtDel, kAtComplex, kApTypes };
constexpr int64_t kApDefaultPiece = (int64_t)8 << 20;  // piece_bytes 0
constexpr int64_t kApMaxLines = 2147483647;            // the data lines stay below: a line number is 32 bits wide
constexpr int64_t kApMaxSpan = 2147483647;             // no line is longer: a column's span is 32 bits wide
constexpr int64_t kApMaxBases = 2147483647;            // a record has fewer bases: a position is an int32 of the origin map

// opts (nullptr: the defaults) checked and completed: piece_bytes 0 becomes the default.  false: *err says which one is bad.
bool apply_check_opts(const pbsim_apply_opts *opts, pbsim_apply_opts *out, std::string *err);
// the 0-based sample column of `name` in the first line that begins with #CHROM; -1: none
int32_t apply_sample_column(const char *vcf, int64_t n, const char *name);
// the report text (pbsim_apply_report)
std::string apply_report_text(const pbsim_apply_result &r);
// the annotated text's header line
extern const char kApTextHeader[];

}  // namespace pbsim

#ifndef PBSIM_APPLY_NO_HIP
#include <hip/hip_runtime.h>

#include "bam_pileup.h"
#include "vcf_compare.h"

namespace pbsim {

constexpr int kApTile = 1024;          // bytes of a tile of the line table's passes: one workgroup's, four per lane
constexpr int kApLineTile = 256;       // lines of a tile of the passes over the lines
constexpr int kApPosTile = kPileTile;  // positions of a tile of the passes over the genome's buffers

// the small cells the passes add into, one behind the other in one buffer of unsigned long long
enum : int {
  kApCellLines = 0,
  kApCellClass,                             // [kApClasses]: applied, the eight classes, overlap
  kApCellTypes = kApCellClass + kApClasses, // [kApTypes] of the applied lines
  kApCellInserted = kApCellTypes + kApTypes,
  kApCellDeleted,
  kApCellSubstituted,
  kApCellBasesOut,
  kApCellLongestCluster,
  kApCellTooLong,    // the data lines longer than kApMaxSpan (the parse)
  kApCellHasSample,  // the data lines that have the sample column (the parse)
  kApCells
};

// What the passes keep of one data line.  The spans are offsets from `start`; a span of 0 bytes is a column the line lacks or that
// is empty.  X is never copied: it is x_n bytes of the line's ALT at start + x_off, to be upper-cased.
struct ApLine {
  int64_t start;  // in the text buffer
  uint32_t chrom_n, pos_off, pos_n, ref_off, ref_n, alt_off, alt_n;
  int32_t r;      // the genome record
  uint32_t s, d;  // the form's start (0-based) and the genome bases replaced
  uint32_t x_off, x_n;
  uint32_t allele;  // the chosen number, where has_allele
  uint32_t by;      // an overlap: the number of the applied line it ran into
  uint8_t cls;      // kApApplied (until the collisions are found: left), a class, kApOverlap
  uint8_t type;
  uint8_t has_allele;
  uint8_t pad;
};

struct ApText {
  const uint8_t *bytes;  // zero bytes behind the text up to the tiles' end, and 64 behind that
  int64_t n, tiles;
};

// what the applied lines leave at the positions of the genome's buffers
struct ApMarks {
  uint32_t *ins_at;          // the applied insertion at this position: its line's index + 1; 0: none.  The insertion behind a
                             // record's last base lies at the record's first padding byte, which no other record owns.
  uint32_t *span_at;         // the same of the applied span that begins here
  unsigned long long *end;   // a span's start: the buffer index behind its last position; else 0
  unsigned long long *tile;  // [tiles]: the largest end of the tile; after the tile scan the largest of the tiles in front
};

// The passes; the rule: include/pbsim3_amd.h.
//   line_sizes  : the data lines that begin in every tile into tile_n
//   line_fill   : (tile_off: the scan of tile_n) every data line's start into line[].start
//   parse       : one lane per data line: spans, allele, class, form.  key[i] = (r << 33 | s << 1 | d > 0) of a line that is left,
//                 (n << 33) of one a class took out; val[i] = i; cells (zeroed): TooLong, HasSample
//   reach       : key and val sorted: reach[i] = (r << 32 | s + d) of the line at place i, 0 of one a class took out; every tile of
//                 kApLineTile places' largest into tile_max
//   tile_scan   : tile[t] becomes the largest of tile[0 .. t - 1]; one workgroup
//   cluster     : start[i] = 1 where the line at place i begins a cluster (a line a class took out: always)
//   walk        : one lane per cluster's first place walks it with the rule: cls and by of its lines, the longest into cells
//   marks       : the applied lines into m (zeroed), every tile of kApPosTile positions' largest end into m.tile by atomic maximum;
//                 then tile_scan over m.tile
//   base_sizes  : what every position emits: a tile's bases into tile_n, the records' parts (as the consensus has them), BasesOut
//   base_fill   : (tile_off: the scan of tile_n; base_at by launch_mutate_record_bases) the FASTA into text where that is asked
//                 for, the origin map into origin where that is
//   text_sizes  : the tally into cells, every record's applied lines into rec_n (zeroed), every tile of kApLineTile lines' annotated
//                 bytes into tile_n
//   text_fill   : (tile_off: the scan) the annotated lines into text
void launch_apply_line_sizes(ApText t, int64_t *tile_n, hipStream_t st);
void launch_apply_line_fill(ApText t, const int64_t *tile_off, ApLine *line, hipStream_t st);
void launch_apply_parse(ApText t, CmpGenome g, ApLine *line, int64_t n_lines, int32_t haplotype, int32_t sample, uint64_t *key, uint32_t *val,
                        unsigned long long *cells, hipStream_t st);
void launch_apply_reach(const ApLine *line, int64_t n_lines, const uint64_t *key, const uint32_t *val, int32_t n_refs, unsigned long long *reach,
                        unsigned long long *tile_max, hipStream_t st);
void launch_apply_tile_scan(unsigned long long *tile, int64_t tiles, hipStream_t st);
void launch_apply_cluster(int64_t n_lines, const uint64_t *key, int32_t n_refs, const unsigned long long *reach, const unsigned long long *tile_max,
                          uint8_t *start, hipStream_t st);
void launch_apply_walk(ApLine *line, int64_t n_lines, const uint64_t *key, const uint32_t *val, int32_t n_refs, const uint8_t *start,
                       unsigned long long *cells, hipStream_t st);
void launch_apply_marks(const ApLine *line, int64_t n_lines, const int64_t *at, ApMarks m, hipStream_t st);
void launch_apply_base_sizes(PileGenome g, ApText t, const ApLine *line, ApMarks m, int64_t *part, int64_t *tile_n, unsigned long long *cells,
                             hipStream_t st);
void launch_apply_base_fill(PileGenome g, ApText t, const ApLine *line, ApMarks m, int32_t line_width, const int64_t *base_at, const int64_t *byte_at,
                            const int64_t *tile_off, char *text, int32_t *origin, hipStream_t st);
void launch_apply_text_sizes(ApText t, const ApLine *line, int64_t n_lines, int32_t all_lines, int64_t *tile_n, unsigned long long *cells,
                             unsigned long long *rec_n, hipStream_t st);
void launch_apply_text_fill(ApText t, const ApLine *line, int64_t n_lines, int32_t all_lines, const int64_t *tile_off, char *text, hipStream_t st);

}  // namespace pbsim
#endif
