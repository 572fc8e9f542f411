// vcf_compare.h -- pbsim_vcf_compare (vcf_compare.cpp) in its parts.  The first half is free of HIP (vcf_compare_rule.cpp): the
// option check, the contig names' hashes and the report text, so that it compiles alone; the second is the device side
// (vcf_compare.hip), left out where PBSIM_COMPARE_NO_HIP is defined.  Internal: nothing here is part of include/pbsim3_amd.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pbsim3_amd.h"

namespace pbsim {

// files[][] of pbsim_compare_result; the classes are also a line's class byte (1 .. 6), kCmpDup behind them
enum : int { kCfLines = 0, kCfMalformed, kCfUnknownContig, kCfUnsupported, kCfRefMismatch, kCfFiltered, kCfNoChange, kCfDup, kCfCompared, kCfShifted,
             kCfLongestShift, kCmpFileCells };
// types[][]: the rows and the columns
enum : int { kCtSnv = 0, kCtIns, kCtDel, kCtComplex, kCmpTypes };
enum : int { kCnTruth = 0, kCnFound, kCnCalls, kCnTp, kCnFp, kCnFpSite, kCmpTypeCells };
constexpr int kCmpBins = 5, kCmpLengthCells = 4, kCmpMsBins = 64;
constexpr int64_t kCmpDefaultPiece = (int64_t)8 << 20;  // piece_bytes 0
constexpr int64_t kCmpMaxLines = 2147483647;            // both files' data lines together stay below: a line number is 32 bits wide
constexpr int64_t kCmpMaxSpan = 2147483647;             // no line is longer: a column's span is 32 bits wide

// the length bin of an insertion of n bases or a deletion of n positions: 1, 2-5, 6-15, 16-49, 50+
constexpr int compare_bin(int64_t n) { return n <= 1 ? 0 : n <= 5 ? 1 : n <= 15 ? 2 : n <= 49 ? 3 : 4; }

// opts (nullptr: the defaults) checked and completed: piece_bytes 0 becomes the default.  false: *err says which one is bad.
bool compare_check_opts(const pbsim_compare_opts *opts, pbsim_compare_opts *out, std::string *err);
// the names the VCFs use for the genome's n records: ref_names where given, else own; none missing or empty, no two equal
bool compare_check_names(const char *const *own, const char *const *ref_names, int n, std::vector<std::string> *used, std::string *err);
// FNV-1a over a name's bytes: what the parse lane computes of CHROM
uint64_t compare_name_hash(const char *bytes, size_t n);
// the names' (hash, record) pairs in ascending order of (hash, record): the table the parse lane searches
void compare_name_table(const std::vector<std::string> &used, std::vector<uint64_t> *hash, std::vector<int32_t> *record);
// the report text (pbsim_compare_report)
std::string compare_report_text(const pbsim_compare_result &r);
// the annotated text's header line
extern const char kCmpTextHeader[];

}  // namespace pbsim

#ifndef PBSIM_COMPARE_NO_HIP
#include <hip/hip_runtime.h>

namespace pbsim {

constexpr int kCmpTile = 1024;  // bytes of a tile of the line table's passes: one workgroup's, four per lane

// the small cells the tally adds into, one behind the other in one buffer of unsigned long long
enum : int {
  kCmpCellFiles = 0,
  kCmpCellTypes = kCmpCellFiles + 2 * kCmpFileCells,
  kCmpCellLengths = kCmpCellTypes + kCmpTypes * kCmpTypeCells,
  kCmpCellMs = kCmpCellLengths + 2 * kCmpBins * kCmpLengthCells,
  kCmpCellTooLong = kCmpCellMs + kCmpMsBins * 2,  // the data lines longer than kCmpMaxSpan (the parse)
  kCmpCells
};

// a data line's verdict byte
enum : int { kCvNone = 0, kCvFound, kCvMissed, kCvTp, kCvFpSite, kCvFp };
constexpr int kCmpDup = 7;  // the class byte of a line whose form an earlier line of its file has

// What the passes keep of one data line.  The spans are offsets from `start`; a span of 0 bytes is a column the line lacks or
// that is empty.  X is never copied: it is x_n bytes of the line's ALT, byte i at start + x_off + (i + x_rot) % x_n, upper-cased.
struct CmpLine {
  int64_t start;  // in the text buffer
  uint32_t chrom_n, pos_off, pos_n, ref_off, ref_n, alt_off, alt_n;
  int32_t r;      // the genome record
  uint32_t s, d;  // the form's start (0-based) and the genome bases replaced
  uint32_t x_off, x_n, x_rot;
  uint32_t ms, shift;
  uint32_t mate;  // the matching line's number in the other file, 0: none
  uint8_t cls;    // 0: compared; 1 .. 6: the class that took it out; kCmpDup
  uint8_t verdict;
  uint8_t type;
  uint8_t pad;
};

// the two texts in one buffer: file 0 (truth) at [0, n[0]), file 1 (calls) at [base1, base1 + n[1]), base1 = tiles0 * kCmpTile;
// zero bytes between and behind them
struct CmpText {
  const uint8_t *bytes;
  int64_t n[2];
  int64_t tiles0, tiles;  // the truth's tiles, both files'
};

// the genome as load_genome leaves it, and the contig names' table
struct CmpGenome {
  int32_t n;
  const int64_t *at, *len;
  const uint8_t *seq;
  const uint64_t *hash;    // [n] ascending
  const int32_t *record;   // [n] beside it
  const int64_t *name_at;  // [n + 1] into names, by record
  const char *names;
};

// The passes; the rule: include/pbsim3_amd.h.
//   line_sizes: the data lines that begin in every tile into tile_n
//   line_fill : (tile_off: the scan of tile_n) every data line's start into line[].start
//   parse     : one lane per data line: spans, class, form; lines below n0 are the truth's.  key[i] = (r << 32 | s) of a line that
//               is left, (n << 32) of one a class took out; val[i] = i; cells[kCmpCellTooLong] counts lines past kCmpMaxSpan
//   match     : key and val sorted: one lane per place marks dup, finds the mate, the verdict
//   text_sizes: the tally into cells (zeroed) and every tile of 256 lines' annotated bytes into tile_n
//   text_fill : (tile_off: the scan) the annotated lines into text
void launch_compare_line_sizes(CmpText t, int64_t *tile_n, hipStream_t st);
void launch_compare_line_fill(CmpText t, const int64_t *tile_off, CmpLine *line, hipStream_t st);
void launch_compare_parse(CmpText t, CmpGenome g, CmpLine *line, int64_t n_lines, int64_t n0, int32_t min_ms, uint64_t *key, uint32_t *val,
                          unsigned long long *cells, hipStream_t st);
void launch_compare_match(CmpText t, CmpLine *line, int64_t n_lines, int64_t n0, const uint64_t *key, const uint32_t *val, int32_t n_refs, hipStream_t st);
constexpr int kCmpTextTile = 256;  // lines of a tile of the text's passes
void launch_compare_text_sizes(CmpText t, const CmpLine *line, int64_t n_lines, int64_t n0, int32_t all_lines, int64_t *tile_n, unsigned long long *cells,
                               hipStream_t st);
void launch_compare_text_fill(CmpText t, const CmpLine *line, int64_t n_lines, int64_t n0, int32_t all_lines, const int64_t *tile_off, char *text,
                              hipStream_t st);

}  // namespace pbsim
#endif
