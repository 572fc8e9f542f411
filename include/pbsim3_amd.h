/* pbsim3_amd.h -- C ABI of the MI355X-native pbsim3 hot path.
 *
 * The reference (yukiteruono/pbsim3 v3.0.5, one translation unit) has no
 * plugin or FFI seam: its boundary is the process (argv -> files).  The
 * internal seam this library replaces is the family
 *     int simulate_by_errhmm(void)        src/pbsim.cpp:3594
 *     int simulate_by_qshmm(void)         src/pbsim.cpp:1955
 *     int simulate_by_errhmm_trans(void)  src/pbsim.cpp:4114
 * together with the loaders/table builders they consume through globals
 * (set_errhmm :5640, set_qshmm :5570, set_mut :5471, get_genome_seq :997).
 * Every entry point below cites the reference lines it stands in for.
 *
 * Conventions (mirroring the reference): functions return PBSIM_SUCCEEDED (1)
 * or PBSIM_FAILED (0) like SUCCEEDED/FAILED (pbsim.cpp:16-17); the message the
 * reference would have printed as "ERROR: ..." is available from
 * pbsim_last_error().  A context is single-owner (one host thread, one GPU).
 * All pointers are plain host pointers unless the name says `_device`.
 *
 * The library is the HIP product: there is no CPU fallback.  Every compute
 * entry point fails (returns 0, pbsim_last_error() says why) when no gfx950
 * device is usable.
 */
#ifndef PBSIM3_AMD_H
#define PBSIM3_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBSIM_SUCCEEDED 1
#define PBSIM_FAILED 0

#define PBSIM_STRATEGY_WGS 1   /* pbsim.cpp:34 */
#define PBSIM_STRATEGY_TRANS 2 /* pbsim.cpp:35 */
#define PBSIM_STRATEGY_TEMPL 3 /* pbsim.cpp:36 */
#define PBSIM_METHOD_QS 1      /* pbsim.cpp:37 */
#define PBSIM_METHOD_ERR 2     /* pbsim.cpp:38 */
#define PBSIM_METHOD_SAMPLE 3  /* pbsim.cpp:39 (METHOD_SAM; the store/reuse variants :40-41 are file handling of the caller) */

/* Validated simulation parameters = the fields of `struct sim_t`
 * (pbsim.cpp:51-77) that the hot path reads.  pbsim_params_default() applies
 * set_sim_param()'s defaults (pbsim.cpp:1539-1685). */
typedef struct pbsim_params {
  int32_t strategy;     /* PBSIM_STRATEGY_*                       */
  int32_t method;       /* PBSIM_METHOD_*                         */
  uint32_t seed;        /* --seed                  (pbsim.cpp:417) */
  int32_t pass_num;     /* --pass-num              (pbsim.cpp:494) */
  double depth;         /* --depth                 (pbsim.cpp:351) */
  double accuracy_mean; /* --accuracy-mean, already int(x*100)*0.01 (pbsim.cpp:1660) */
  double len_mean;      /* --length-mean           (pbsim.cpp:469) */
  double len_sd;        /* --length-sd             (pbsim.cpp:477) */
  double hp_del_bias;   /* --hp-del-bias           (pbsim.cpp:514) */
  int64_t len_min;      /* --length-min            (pbsim.cpp:363) */
  int64_t len_max;      /* --length-max            (pbsim.cpp:375) */
  int64_t sub_ratio;    /* --difference-ratio      (pbsim.cpp:405) */
  int64_t ins_ratio;
  int64_t del_ratio;
  char id_prefix[64];   /* --id-prefix             (pbsim.cpp:347) */
} pbsim_params;

/* Per-unit results = the `sim.res_*` block (pbsim.cpp:63-70) plus the two
 * histograms' derived values, computed exactly as pbsim.cpp:4082-4105. */
typedef struct pbsim_stats {
  int64_t res_num;       /* reads                                      */
  int64_t res_pass_num;  /* reads * pass_num                           */
  int64_t res_len_total; /* simulated bases over all passes            */
  int64_t res_len_min, res_len_max;
  int64_t res_sub_num, res_ins_num, res_del_num;
  double res_depth;
  double res_len_mean, res_len_sd;
  double res_accuracy_mean, res_accuracy_sd;
  double res_sub_rate, res_ins_rate, res_del_rate;
} pbsim_stats;

/* What one batch produced (device-resident until pbsim_batch_fetch). */
typedef struct pbsim_batch_info {
  int64_t first_read;    /* 1-based index of the first read of the batch          */
  int64_t n_reads;       /* reads simulated speculatively                         */
  int64_t n_final;       /* leading reads that are final under the quota rule     */
  int32_t quota_reached; /* 1: the unit's quota loop ends inside this batch       */
  int32_t need_truncated_read; /* 1: read first_read+n_final must be re-drawn with
                            the truncated length (pbsim.cpp:3795-3800)            */
  int64_t len_total_after; /* pass-0 bases accumulated after the n_final reads    */
  int64_t bases;         /* read bases over all passes of the n_final reads       */
  int64_t read_text_bytes; /* FASTQ (pass_num==1) or SAM text bytes               */
  int64_t maf_text_bytes;  /* MAF text bytes                                      */
  int64_t ref_bases;     /* reference bases consumed (roofline accounting)        */
  int64_t maf_columns;   /* MAF columns written      (roofline accounting)        */
} pbsim_batch_info;

/* Receiver of finished text, called in read order; the bytes are exactly what
 * the reference fprintf()s into its gzip/samtools pipes (pbsim.cpp:4012-4078).
 * Return 0 from a callback to abort the simulation. */
typedef struct pbsim_sink {
  void *user;
  int (*on_read_text)(void *user, const char *text, int64_t bytes); /* FASTQ or SAM records */
  int (*on_maf_text)(void *user, const char *text, int64_t bytes);  /* MAF records          */
} pbsim_sink;

typedef struct pbsim_ctx pbsim_ctx;

/* ---- lifecycle -------------------------------------------------------------- */
void pbsim_params_default(pbsim_params *p);                     /* pbsim.cpp:1539-1685 */
pbsim_ctx *pbsim_create(const pbsim_params *p, int device);     /* main() setup, pbsim.cpp:538-578, 662 */
void pbsim_destroy(pbsim_ctx *ctx);
const char *pbsim_last_error(void);
const char *pbsim_version(void);

/* ---- model tables -----------------------------------------------------------
 * All seven model files the reference ships load (QSHMM-ONT-HQ's 52- and 56-state classes through the reference's own flat
 * indexing of struct qshmm_t, pbsim.cpp:160-166, 5606-5626).  Two shapes of model FILE are refused with PBSIM_FAILED and an
 * error text -- no shipped model has either:
 *   - an ERRHMM model with a hole inside its own accuracy range (a class between acc_min and acc_max without lines): the
 *     reference walks such a read with the rate_mag left over from whichever out-of-range read came before it
 *     (pbsim.cpp:3829-3833 sets it only outside the range), i.e. its output depends on the order of the reads;
 *   - a QSHMM file whose state / column numbers index past the end of tp[] (pbsim.cpp:5606-5626 has no bounds check: the
 *     reference overwrites whatever lies behind the struct). */
int pbsim_load_errhmm(pbsim_ctx *ctx, const char *path);        /* set_errhmm :5640 + tables :3633-3789 */
int pbsim_load_qshmm(pbsim_ctx *ctx, const char *path);         /* set_qshmm  :5570 + tables :1991-2170 */

/* ---- reference sequence of the current unit ---------------------------------
 * `seq` is the raw record (no newlines) as get_genome_seq() assembles it
 * (pbsim.cpp:1014-1033); upper-casing and the per-base homopolymer length
 * (pbsim.cpp:1035-1065) are done on the GPU.  record_index is genome.num
 * (1-based).  The _device form takes a pointer already in this GPU's HBM. */
int pbsim_set_reference(pbsim_ctx *ctx, const uint8_t *seq, int64_t len, int64_t record_index);
int pbsim_set_reference_device(pbsim_ctx *ctx, const void *seq_device, int64_t len, int64_t record_index);
/* Optional: hand the NEXT record over early.  Its upload and preparation (toupper + homopolymer lengths, get_genome_seq
 * pbsim.cpp:1014-1065) run on a stream of their own beside the simulation of the current record; the next
 * pbsim_set_reference* call with the same pointer and length adopts the result instead of doing the work again (any other
 * call drops it).  The bytes must not change in between.  wgs only. */
int pbsim_prefetch_reference(pbsim_ctx *ctx, const uint8_t *seq, int64_t len);
int pbsim_prefetch_reference_device(pbsim_ctx *ctx, const void *seq_device, int64_t len);
/* --hp-del-bias != 1 needs the homopolymer census of ALL records first
 * (pbsim.cpp:677-696): call once per record, then pbsim_finish_hp_census(). */
int pbsim_add_hp_census(pbsim_ctx *ctx, const uint8_t *seq, int64_t len);
int pbsim_finish_hp_census(pbsim_ctx *ctx);

/* ---- transcriptome units (strategy trans) -----------------------------------
 * All transcripts are handed over at once; ids are NUL-terminated strings.
 * Replaces the streaming reader inside simulate_by_errhmm_trans
 * (pbsim.cpp:4428-4485) and get_transcript_inf (:1075). */
int pbsim_set_transcripts(pbsim_ctx *ctx, int64_t n, const char *const *ids, const int64_t *plus_exp,
                          const int64_t *minus_exp, const uint8_t *const *seqs, const int64_t *lens);

/* ---- templates (strategy templ): each FASTA record of --template is one unit that is
 * read once, full length, '+' strand (get_templ_inf :1366, simulate_by_*_templ :5055-5103). */
int pbsim_set_templates(pbsim_ctx *ctx, int64_t n, const char *const *ids, const uint8_t *const *seqs,
                        const int64_t *lens);

/* ---- whole-unit drivers = the reference seam --------------------------------
 * pbsim_simulate_wgs  : one FASTA record, quota loop included
 *                       (simulate_by_errhmm :3792-4080 / simulate_by_qshmm :2173-2385)
 * pbsim_simulate_trans: every transcript (simulate_by_errhmm_trans :4428-4770) */
int pbsim_simulate_wgs(pbsim_ctx *ctx, const pbsim_sink *sink);
int pbsim_simulate_trans(pbsim_ctx *ctx, const pbsim_sink *sink);
int pbsim_simulate_templ(pbsim_ctx *ctx, const pbsim_sink *sink); /* simulate_by_errhmm_templ :4807 / _qshmm_templ :3055 */
/* Read-block shard of a unit set (multi-GPU front-end, one rank per GPU): reads first_read .. first_read + n_reads - 1 of
 * the global numbering sim.res_num of simulate_by_*_trans / _templ (pbsim.cpp:4516-4522 assigns reads to transcripts in
 * file order).  Every byte of a read depends only on (seed, read, pass, event), so the shards of all ranks concatenated
 * in read order are the bytes pbsim_simulate_trans delivers; the statistics cover the shard only (the caller sums them).
 * pbsim_unit_reads: reads of the whole set (sum of the expression values, or the number of templates). */
int pbsim_simulate_units_range(pbsim_ctx *ctx, int64_t first_read, int64_t n_reads, const pbsim_sink *sink);
int64_t pbsim_unit_reads(pbsim_ctx *ctx);

/* ---- reads as device arrays -------------------------------------------------
 * The same reads as the text drivers, handed over as arrays in HBM instead of FASTQ/SAM + MAF text.  A task is one read
 * of one pass; task t = r * pass_num + h holds read r (in read order) and pass h, the order in which the text drivers write
 * their records (pbsim.cpp:3986-4078 wgs errhmm; the MAF emit of wgs qshmm :2352-2383, trans :4736-4767 / :2984-3015,
 * templ :5306-5337 / :3502-3533).  Per base:
 *   seq       the bytes of the FASTQ sequence line (pass_num 1, pbsim.cpp:4014) or of the SAM SEQ field (:4017)
 *   qual      the quality bytes of the same record minus 33 (ERRHMM: all 0, its quality line is all '!', :4007-4010)
 *   ref_pos   0-based forward-strand coordinate of the reference base in the same MAF column, -1 where the MAF reference
 *             line holds '-' (an inserted base); in the record (wgs) or in the transcript / template (trans, templ).
 *             Read base i of a '+' task sits in the MAF column that holds its (i+1)-th read byte; of a '-' task in the
 *             column that holds its (q-i)-th (the MAF lines are in reference orientation, :3981-3984)
 * Per task:
 *   offsets      [tasks + 1] exclusive scan of the tasks' base counts (task t's bases are [offsets[t], offsets[t+1]))
 *   read_number  the number in the read's id, sim.res_num (:4013)
 *   pass_index   h (the /h of a SAM id, :4016)
 *   unit         wgs: the record_index given to pbsim_set_reference*; trans/templ: the unit's 0-based load order
 *   strand       0 '+', 1 '-': the strand of the MAF read line (:4074)
 *   ref_start, ref_span   start and size of the MAF reference line (:4047-4063)
 *   n_sub, n_ins, n_del   the walk's error counters of the task (sim.res_sub_num etc. are their sums, :3986-4005) */
typedef struct pbsim_read_arrays {
  uint8_t *seq, *qual;   /* [bases] */
  int32_t *ref_pos;      /* [bases]; NULL: not written */
  int64_t *offsets;      /* [tasks + 1] */
  int64_t *read_number;  /* [tasks] ... */
  int32_t *pass_index, *unit;
  uint8_t *strand;
  int64_t *ref_start;
  int32_t *ref_span, *n_sub, *n_ins, *n_del;
} pbsim_read_arrays;
/* alloc: the caller fills `out` with device pointers (on the context's device, 16-byte aligned) for exactly `tasks`
 * tasks and `bases` bases of the next batch; on_batch: the batch's arrays are complete (the context's stream has been
 * synchronised).  Both are called once per batch in read order; a batch without final tasks is skipped.  Return 0 from
 * either to abort the run: pbsim_simulate_arrays then returns 0 and the context stays usable. */
typedef struct pbsim_array_sink {
  void *user;
  int (*alloc)(void *user, int64_t tasks, int64_t bases, pbsim_read_arrays *out);
  int (*on_batch)(void *user, const pbsim_batch_info *info);
} pbsim_array_sink;
/* Runs the context's current unit like pbsim_simulate_wgs (wgs: the record set by pbsim_set_reference*) or
 * pbsim_simulate_trans (trans/templ: all loaded units), same reads, same statistics (pbsim_get_stats), but no text: each
 * batch's rows go into the sink's arrays.  pbsim_set_deflate and pbsim_set_bam_output do not apply.  The sampling
 * method is refused. */
int pbsim_simulate_arrays(pbsim_ctx *ctx, const pbsim_array_sink *sink);
/* Host-side readers of the reference's unit files for callers above the ABI that are not C++: parse `path` like
 * simulate_by_*_trans does its --transcript file (pbsim.cpp:4428-4485; get_transcript_inf :1075) resp. get_templ_inf its
 * --template FASTA (:1366) and hand the units over (pbsim_set_transcripts / pbsim_set_templates).
 * stats[0] = units, stats[1] = total expression value (trans) resp. total template length (templ). */
int pbsim_load_transcript_file(pbsim_ctx *ctx, const char *path, int64_t stats[2]);
int pbsim_load_template_file(pbsim_ctx *ctx, const char *path, int64_t stats[2]);
int pbsim_get_stats(pbsim_ctx *ctx, pbsim_stats *out);          /* pbsim.cpp:4082-4105, 5541-5562 */
/* Sampling method (--method sample, wgs only, single pass).  pbsim_set_sample_profile hands over what
 * get_sample_inf (pbsim.cpp:1155-1330) leaves in its filtered profile: the quality strings that passed the
 * length / accuracy filter, in file order (the caller parses the FASTQ, keeps the statistics and the
 * sample_profile_<ID> files).  pbsim_simulate_sample = simulate_by_sample (pbsim.cpp:1694-1949) for the
 * current reference record. */
int pbsim_set_sample_profile(pbsim_ctx *ctx, int64_t n, const uint8_t *const *quals, const int64_t *lens);
int pbsim_simulate_sample(pbsim_ctx *ctx, const pbsim_sink *sink);
/* get_sample_inf itself (pbsim.cpp:1155-1330) on the context's GPU: the FASTQ's bytes go through HBM, every record's 4th
 * line is summed and filtered there (length range: the params' len_min / len_max; accuracy range: the arguments, already
 * int(x*100)*0.01 as pbsim.cpp:1620 leaves them) and the kept strings are packed into the pool pbsim_simulate_sample
 * reads -- the context is then in the state pbsim_set_sample_profile leaves.  *out = the numbers print_sample_stats prints
 * (pbsim.cpp:1336-1360) and the stored profile's .stats file holds (:1317-1326), bit for bit the host parser's.  Failures
 * carry the reference's texts ("fastq is too long. Max acceptable length is 1000000." :1228/:1283, "fastq is too many. Max
 * acceptable number is 100000000." :1236, "there is no sample in the valid range of length and accuracy." :1294); the context
 * keeps the profile it had and stays usable.  A tables-only context refuses ("no HIP device").
 *   pbsim_sample_profile_from_bytes   the bytes in host memory
 *   pbsim_sample_profile_from_device  the bytes in the memory of the context's GPU (complete when the call is made)
 *   pbsim_load_sample_fastq           a file: plain, BGZF (inflated by this GPU, the bytes stay in its memory) or other gzip
 *                                     (zlib on the host); a pipe or an empty file goes through the host's stdio parse
 *   pbsim_sample_profile_text         the kept strings one per line = the bytes of sample_profile_<ID>.fastq (:1264);
 *                                     *bytes = their size; dst may be NULL to ask for it (else cap >= *bytes)
 *   pbsim_set_sample_chunk_bytes      FASTQ bytes per window of the pass through HBM (0: the default, 64 MiB; 16 to 2^30).
 *                                     The result does not depend on it. */
typedef struct pbsim_sample_stats {
  int64_t num, len_min, len_max, len_total;                                         /* all reads (pbsim.cpp:1232-1245) */
  int64_t num_filtered, len_min_filtered, len_max_filtered, len_total_filtered;     /* kept reads (:1257-1271)         */
  double len_mean_filtered, len_sd_filtered, accuracy_mean_filtered, accuracy_sd_filtered;  /* :1298-1315               */
} pbsim_sample_stats;
int pbsim_sample_profile_from_bytes(pbsim_ctx *ctx, const void *fastq, int64_t n, double accuracy_min, double accuracy_max,
                                    pbsim_sample_stats *out);
int pbsim_sample_profile_from_device(pbsim_ctx *ctx, const void *d_fastq, int64_t n, double accuracy_min, double accuracy_max,
                                     pbsim_sample_stats *out);
int pbsim_load_sample_fastq(pbsim_ctx *ctx, const char *path, double accuracy_min, double accuracy_max, pbsim_sample_stats *out);
int pbsim_sample_profile_text(pbsim_ctx *ctx, char *dst, int64_t cap, int64_t *bytes);
int pbsim_set_sample_chunk_bytes(pbsim_ctx *ctx, int64_t bytes);
/* The same profile from a BAM, unaligned (PacBio, dorado) or aligned: bit for bit -- statistics, kept strings, pool -- the
 * profile the calls above make from the FASTQ that `samtools fastq` (default options) writes from that BAM.  A BAM is a stream
 * whose first four bytes, behind any gzip layer, are "BAM\1".  Records with flag 0x100 (secondary) or 0x800 (supplementary)
 * are skipped; every other record is one read of l_seq qualities, quality byte q standing for the character min(q, 93) + 33,
 * taken from the last byte to the first with flag 0x10 (the read's own orientation).  Names, bases, CIGARs and tags are only
 * stepped over.  The record starts are found by a parallel test of every byte position and decided by a walk along
 * block_size from the first record; the stream passes through HBM in windows of pbsim_set_sample_chunk_bytes inflated
 * bytes, an unfinished record carried in front of the next one (a record may be larger than a window).
 * Failures, besides the texts above (l_seq > 1 000 000 is "fastq is too long...", as its FASTQ line would be):
 *   "<path>: truncated BAM header"                                       the header overruns the stream
 *   "<path>: malformed or truncated BAM record at inflated offset <n>"   block_size < 32 + l_read_name + 4 n_cigar_op +
 *       (l_seq + 1) / 2 + l_seq or > 64 MiB, l_read_name == 0, a name without its NUL, refID / next_refID outside [-1, n_ref),
 *       pos / next_pos < -1, or a record that runs past the end of the stream
 *   "<path>: BAM record <index> (<read name>) has no qualities"          l_seq > 0 and a first quality byte 0xFF; <index>
 *       counts every record of the file from 1
 * (<path> is "BAM bytes" where there is no file).  The context keeps the profile it had and stays usable.
 *   pbsim_load_sample                       a file of either format -- FASTQ exactly as pbsim_load_sample_fastq reads it, or BAM
 *                                           (BGZF inflated by this GPU, other gzip by zlib, or not compressed)
 *   pbsim_sample_profile_from_bam_bytes     the inflated BAM bytes in host memory
 *   pbsim_sample_profile_from_bam_device    the inflated BAM bytes in the memory of the context's GPU */
int pbsim_load_sample(pbsim_ctx *ctx, const char *path, double accuracy_min, double accuracy_max, pbsim_sample_stats *out);
int pbsim_sample_profile_from_bam_bytes(pbsim_ctx *ctx, const void *bam, int64_t n, double accuracy_min, double accuracy_max,
                                        pbsim_sample_stats *out);
int pbsim_sample_profile_from_bam_device(pbsim_ctx *ctx, const void *d_bam, int64_t n, double accuracy_min, double accuracy_max,
                                         pbsim_sample_stats *out);
/* SAM header the reference's main() writes when it opens the samtools pipe for a
 * unit (pass_num > 1; pbsim.cpp:721-722 wgs, :784-785 trans/templ).  Returns the
 * byte count (excluding the NUL), or the size needed when buf is NULL/too small. */
int64_t pbsim_sam_header(pbsim_ctx *ctx, char *buf, int64_t cap);
/* pass_num > 1 only: make the read sink receive BAM alignment records (SAMv1 4.2, uncompressed,
 * one per subread, what `samtools view -b` would build from the SAM text of pbsim.cpp:4016-4027)
 * instead of SAM text; pbsim_bam_header() gives the bytes that precede the first record.  The
 * caller BGZF-frames the stream (the CLI does, replacing the samtools child of pbsim.cpp:716). */
int pbsim_set_bam_output(pbsim_ctx *ctx, int on);
int64_t pbsim_bam_header(pbsim_ctx *ctx, char *buf, int64_t cap);
/* The truth as aligned BAM instead of MAF (any strategy x method that writes MAF, any pass_num).  While on, everything that
 * delivers the MAF stream -- pbsim_sink::on_maf_text, pbsim_record_sink::on_maf_text, pbsim_batch_fetch's maf_text, with
 * pbsim_set_deflate their BGZF members -- delivers one BAM alignment record (SAMv1 4.2) per task instead of one MAF block, in
 * the same task order and under the same offsets contract; pbsim_batch_info::maf_text_bytes counts those bytes.  The read
 * stream, the statistics and pbsim_simulate_arrays are untouched.  A record: refID = wgs 0, trans / templ the unit's 0-based
 * load order; pos = the MAF reference line's start; mapq 60; bin = reg2bin(pos, pos + span) (low 16 bits); flag 0 / 16 for a
 * '+' / '-' MAF read line; read_name = the id of the FASTQ / SAM record; CIGAR = the maximal M / I / D runs of the MAF columns
 * in reference orientation ('-' on the reference line: I, on the read line: D); SEQ / QUAL = the MAF read line without its
 * '-' and the qualities in the same orientation (ERRHMM: zeros); one tag, NM = n_sub + n_ins + n_del of the task.  More than
 * 65535 runs: n_cigar_op 2 with <q>S<span>N and the runs in a CG:B,I tag behind NM (SAMv1 4.2.2).
 * pbsim_truth_bam_header / pbsim_job_truth_bam_header: the bytes in front of the first record ("BAM\1", @HD, one @SQ per
 * reference -- wgs: "ref" with the record's length; trans / templ: every loaded unit, its MAF name cut at the first whitespace
 * byte -- , @PG, the reference list); same return convention as pbsim_bam_header.  Unit names that are empty after the cut, equal
 * to another unit's or outside SAMv1's RNAME character set make pbsim_set_truth_bam (units already loaded) or the first
 * simulate call fail; the message names the unit. */
int pbsim_set_truth_bam(pbsim_ctx *ctx, int on);
int64_t pbsim_truth_bam_header(pbsim_ctx *ctx, char *buf, int64_t cap);
int64_t pbsim_job_truth_bam_header(pbsim_ctx *ctx, int64_t record, char *buf, int64_t cap);
/* Compression on the GPU, replacing the `gzip -c` children of pbsim.cpp:708-730 and the BGZF layer of
 * `samtools view -b` (pbsim.cpp:716).  pbsim_set_deflate(ctx, mask): bit 0 makes the read sink, bit 1
 * the MAF sink receive gzip members (RFC 1952) instead of text: one member per 32 KiB of text, each carrying the BGZF 'BC'
 * extra field (SAMv1 4.1), so the concatenation is a valid multi-member .gz and, for BAM records, a
 * valid BAM container once the caller has written a compressed header in front and the BGZF EOF marker
 * behind.  Decompressed bytes are exactly the text the sink would have received otherwise.
 * Bit 2 (with bits 0 and 1): the two sinks are independent -- on_read_text is then called from a second host thread
 * while on_maf_text runs on the caller's (two files are written side by side; never one callback concurrently with itself).
 * pbsim_batch_fetch_deflated is the batch-level primitive (after pbsim_batch_finalize; caps from
 * pbsim_deflate_bound).  pbsim_deflate_buffer runs host bytes through the same kernels (file headers). */
int pbsim_set_deflate(pbsim_ctx *ctx, int mask);
int64_t pbsim_deflate_bound(int64_t text_bytes);
int pbsim_batch_fetch_deflated(pbsim_ctx *ctx, char *read_gz, int64_t read_cap, char *maf_gz, int64_t maf_cap,
                               int64_t *read_gz_bytes, int64_t *maf_gz_bytes);
int pbsim_deflate_buffer(pbsim_ctx *ctx, const void *src, int64_t n, void *dst, int64_t cap, int64_t *out_bytes);
/* Decompression on the GPU, for BGZF input (SAMv1 4.1: gzip members of at most 64 KiB of output, each with a 'BC' extra
 * field giving its size -- what bgzip writes, and what pbsim_deflate_buffer and the CLI's .fq.gz / .maf.gz / .bam are).
 * pbsim_inflate_bound needs no context and no device: the inflated size of the BGZF buffer src[0..n) from its member
 * headers and trailers, or -1 when the buffer is not BGZF (other gzip, a missing 'BC' field, an ISIZE over 65536, a member
 * that runs past the end).  pbsim_inflate_buffer inflates every member at once into dst (cap bytes at least the bound) and
 * checks each member's CRC-32 and ISIZE; other gzip, a corrupt member ("gzip member at byte offset N: <reason>") and a
 * tables-only context give PBSIM_FAILED, and the context stays usable. */
int64_t pbsim_inflate_bound(const void *src, int64_t n);
int pbsim_inflate_buffer(pbsim_ctx *ctx, const void *src, int64_t n, void *dst, int64_t cap, int64_t *out_bytes);
/* A finished truth BAM, sorted by coordinate and indexed on the GPU: what `samtools sort` and `samtools index -c` would make of
 * a file of pbsim_set_truth_bam's records.  bam[0..n) is the whole file: BGZF members of any legal size, "BAM\1", header text,
 * reference list, then records that are all placed and single-end (0 <= refID < n_ref, pos >= 0, next_refID = next_pos = -1,
 * tlen = 0); anything else fails with a message that names the inflated byte offset of the first record that does not fit.
 * The file is inflated into HBM, every byte position is tested against those fields in parallel, the host walks the
 * block_size chain over the hits (that walk alone decides what a record is), the records are sorted by (refID, pos) -- stable:
 * ties keep their input order, so the output is a function of the input alone -- and gathered into a second stream, which leaves
 * as BGZF members of 32 KiB of text behind a header that differs in one place: its @HD line says SO:coordinate (the SO: value
 * replaced; "@HD\tVN:1.6\tSO:coordinate\n" in front of a text without @HD; l_text adjusted).  The header is compressed as
 * members of its own, the file ends with the BGZF EOF block, and the 16-bit bin fields of the records stay as they are.
 * on_bam receives the sorted file piece by piece in offset order; on_index then the whole .csi file, once: CSIv1, BGZF with
 * EOF block, min_shift 14, depth the smallest value >= 5 with 2^(14 + 3 depth) >= the longest reference, l_aux 0, the trailing
 * n_no_coor (0) present.  A record's bin is reg2bin(pos, end, 14, depth) of the CSI specification, end = pos + the reference
 * span of its CIGAR (M D N = X; a span of 0 counts as 1; a <q>S<span>N record takes its span from the N).  A bin's chunks are
 * the maximal runs of records, consecutive in file order on that reference, that have the bin -- one chunk per run, not merged
 * further -- from the virtual offset of the run's first record to that of the record behind its last (the EOF block's
 * coffset << 16 behind the file's last record); a virtual offset is (offset of the member that holds the record's first
 * byte) << 16 | offset in that member's text.  loffset of a bin that covers [s, s + len) is the virtual offset of the first
 * record in file order on that reference with end > s.  Bins ascend by number, chunks keep file order; a reference with
 * records ends with the pseudo-bin ((1 << 3 (depth + 1)) - 1) / 7 + 1: loffset 0, two chunks (first record's offset, end of
 * the last; n_mapped = its record count, n_unmapped = 0); a reference without records has n_bin = 0.
 * stats (may be NULL): records, references with records, inflated record bytes, index bins (pseudo-bins not counted).
 * A callback that returns 0 aborts the call.  The stage holds the inflated stream, the sorted stream and their compressed
 * pieces in HBM at once and does not chunk: a file that does not fit fails with the bytes the refused allocation needed.
 * A tables-only context fails as pbsim_inflate_buffer does.  After any failure the context stays usable and on_index has not
 * been called. */
typedef struct pbsim_sorted_bam_sink {
  void *user;
  int (*on_bam)(void *user, const char *bytes, int64_t n, int64_t offset); /* the sorted file, in offset order */
  int (*on_index)(void *user, const char *bytes, int64_t n);               /* the .csi file, once, whole */
} pbsim_sorted_bam_sink;
int pbsim_truth_bam_sort(pbsim_ctx *ctx, const void *bam, int64_t n, const pbsim_sorted_bam_sink *sink, int64_t stats[4]);
/* A mapper's BAM scored against the truth on the GPU: how many simulated reads were mapped back to where they came from, by
 * MAPQ (what `paftools mapeval` tells of a PAF).  truth[0..n_truth), n_truth >= 1: files of pbsim_set_truth_bam's records, in
 * task order or sorted (the records pbsim_truth_bam_sort accepts); query[0..n): any BAM, in any order, with secondary,
 * supplementary, unmapped and paired records.  Each file is BGZF (inflated on the GPU), one plain gzip stream (inflated by
 * zlib on the host) or an uncompressed BAM stream.
 * References are matched by name, never by refID.  ref_name (NULL: none) replaces the name of a truth file's reference and is
 * legal only where the file has exactly one (a wgs truth file calls its reference "ref": ref_name is the FASTA record the
 * mapper saw).  A query reference that no truth file names matches nothing.  Reads are matched by read name, the bytes in
 * front of the NUL, over all truth files; a name that occurs twice in the truth (a file given twice, files that repeat a name) is
 * refused with the name and both files.
 * A query record with flag & 0x100 is secondary, else with flag & 0x800 supplementary, else primary.  A primary whose name
 * the truth does not have is unknown.  Of the known primaries of one name the one at the smallest inflated offset is the
 * first, the others are duplicates.  A first primary with flag & 4 or refID < 0 is unmapped; every other one is scored.  The
 * interval of a record is [pos, pos + max(1, span)), span the sum of its CIGAR's M, D, N, = and X lengths (the <q>S<span>N
 * placeholder of a CG-tagged record gives its span so; the tag is not read).  A scored record is correct when its reference
 * has the truth's name, its flag & 16 is the truth's and, with inter = min(te, qe) - max(ts, qs) and union = max(te, qe) -
 * min(ts, qs) in 64-bit integers, inter > 0 and inter * 1000 >= overlap_permille * union; else it is wrong.
 * counts: truth records, query records, primary, secondary, supplementary, unknown, duplicate, unmapped, scored, correct,
 * wrong, missing (truth reads without a first primary).  hist[2 q], hist[2 q + 1]: the scored records of MAPQ q and the wrong
 * ones among them.  on_verdicts (sink or the callback may be NULL) is called once with one byte per truth record, in truth
 * file order then record order: 0 missing, 1 unmapped, 2 wrong, 3 correct; a return of 0 aborts the call.
 * opts (NULL: the defaults): overlap_permille 1 .. 1000 (0: the default, 100); hash_bits 0 or 64: read names are looked up by
 * all 64 bits of their hash; 1 .. 63: by that many bits only -- for tests, which so drive every lookup through collisions: the
 * results must not differ, since a lookup always compares the name bytes (the duplicate check then costs the square of a run).
 * tests/mapeval_model.py states the rule in plain Python.  The stage holds every inflated stream in HBM at once and does not
 * chunk: a file that does not fit fails with the bytes the refused allocation needed.  A malformed record fails with its
 * inflated offset, a query of more than 2^36 inflated bytes is refused, a tables-only context fails as pbsim_inflate_buffer
 * does.  After any failure the context stays usable and on_verdicts has not been called. */
typedef struct pbsim_eval_truth {
  const void *bytes;
  int64_t n;
  const char *ref_name; /* NULL: the file's own reference names */
} pbsim_eval_truth;
typedef struct pbsim_eval_opts {
  int32_t overlap_permille;
  int32_t hash_bits;
} pbsim_eval_opts;
typedef struct pbsim_eval_sink {
  void *user;
  int (*on_verdicts)(void *user, const unsigned char *bytes, int64_t n);
} pbsim_eval_sink;
int pbsim_truth_bam_eval(pbsim_ctx *ctx, const pbsim_eval_truth *truth, int n_truth, const void *query, int64_t n,
                         const pbsim_eval_opts *opts, const pbsim_eval_sink *sink, int64_t counts[12], int64_t hist[512]);
/* The report text of counts and hist, no device needed: one line "# truth_records=N query_records=N primary=N secondary=N
 * supplementary=N unknown=N duplicate=N unmapped=N scored=N correct=N wrong=N missing=N", then for each MAPQ from 255 down
 * that has scored records "Q\t<mapq>\t<n>\t<wrong>\t<cum n>\t<cum wrong>\t<cum wrong * 1000000 / cum n>\t<cum n * 1000000 /
 * truth records>" (sums from 255 down to this MAPQ, integer division).  Returns the text's length, and writes it (no NUL)
 * where buf holds cap >= that many bytes; -1: bad argument. */
int64_t pbsim_eval_report(const int64_t counts[12], const int64_t hist[512], char *buf, int64_t cap);
/* The depth of coverage of a BAM on the GPU: how many records cover each reference position (what `samtools depth -a`,
 * `bedtools genomecov -bga` or `mosdepth` tell).  bam[0..n) is a truth BAM, sorted or not, or a mapper's BAM: BGZF (inflated
 * on the GPU), one plain gzip stream (zlib on the host) or an uncompressed BAM stream; any record pbsim_truth_bam_eval takes
 * as a query record is taken here.
 * A record is skipped, and counted, in this order: skipped_flag if flag & exclude_flags (default 0x704: unmapped, secondary,
 * QC-fail, duplicate; supplementary records count); else skipped_unplaced if refID < 0 or pos < 0; else skipped_mapq if
 * mapq < min_mapq.  Nothing more of a skipped record is looked at.  Every other record is counted.
 * The CIGAR of a counted record is its CIGAR field -- except where n_cigar_op == 2, op 0 is S with length l_seq, op 1 is N and
 * the record has a CG tag of type B,I: then it is the array in that tag (SAMv1 4.2.2; truth records of more than 65535 runs
 * are written so, and the placeholder taken literally covers nothing).  The tag is looked for in such a record only, by
 * walking its aux fields by type (A c C s S i I f Z H B); an aux field that runs past the record or has an unknown type
 * fails the call with the record's inflated offset, and so does a CIGAR op code above 8 in a counted record.
 * The reference position starts at pos and advances over M D N = X.  M, = and X cover; D covers when count_deletions is not 0
 * (the default: the truth of an error-laden long read has a deletion every few dozen bases); N never covers; I S H P
 * neither advance nor cover.  Positions at or beyond the reference's l_ref are not counted, and a record that loses at least
 * one covered position so is counted in clipped.  A record that covers nothing is counted and adds no depth.
 * depth[ref][p] is the number of counted records that cover p, an int32: a file of 2^31 records or more is refused.  All of it
 * is integer arithmetic: the result is a function of the input alone, whatever the order of the records.
 * The text, through on_text in offset order, in pieces of at most piece_bytes (a piece may end inside a line), the references
 * in header order, none for a reference with l_ref == 0, name the bytes in front of the first NUL:
 *   format 0, bedgraph: the maximal runs of equal depth over [0, l_ref), zero runs too: "name\tstart\tend\tdepth\n";
 *   format 1, window (window >= 1): for k = 0, 1, ..: [k window, min((k + 1) window, l_ref)): "name\tstart\tend\tsum\tmean_milli\n",
 *   sum the 64-bit sum of the depths, mean_milli = sum * 1000 / (end - start), integer division.
 * counts: records, counted, skipped_flag, skipped_unplaced, skipped_mapq, clipped.  hist[d]: over all references the positions
 * of depth d, hist[255] those of depth >= 255.  on_refs, once and before any text: per reference l_ref, covered positions
 * (depth >= 1), the 64-bit sum of depths, the largest depth.  on_depth, after the text and only where it is not NULL: a host
 * copy of each reference's depths, in header order.  sink and each callback may be NULL; a callback that returns 0 aborts
 * the call.  tests/depth_model.py states the rule in plain Python.
 * The stage holds the inflated stream and the depth array -- 4 bytes per reference position, 12 GB for a 3 Gbp header -- in HBM
 * at once and does not chunk: what does not fit fails with the bytes the refused allocation needed.  format outside 0 and 1,
 * window < 1 with format 1, min_mapq outside 0 .. 255 and a negative piece_bytes fail before any device work; a malformed
 * record fails with its inflated offset, a file of 2^36 inflated bytes or more is refused, a tables-only context fails as
 * pbsim_inflate_buffer does.  After any failure the context stays usable. */
typedef struct pbsim_depth_opts { /* NULL: {0x704, 0, 1, 0, 0, 0} */
  int32_t exclude_flags, min_mapq, count_deletions;
  int32_t format;      /* 0 bedgraph, 1 window */
  int64_t window;      /* format 1: >= 1 */
  int64_t piece_bytes; /* 0: the default; else the most text one on_text call carries (tests drive many pieces with it) */
} pbsim_depth_opts;
typedef struct pbsim_depth_sink {
  void *user;
  int (*on_text)(void *user, const char *bytes, int64_t n, int64_t offset); /* in offset order; may be NULL */
  int (*on_refs)(void *user, int32_t n_ref, const char *const *names,
                 const int64_t *rows /* n_ref x 4: l_ref, covered, sum, max */); /* once, before any on_text; may be NULL */
  int (*on_depth)(void *user, int32_t ref, const int32_t *depth, int64_t l_ref); /* host copy, per reference in order, after
                                                                                     the text; may be NULL: then nothing is copied */
} pbsim_depth_sink;
int pbsim_bam_depth(pbsim_ctx *ctx, const void *bam, int64_t n, const pbsim_depth_opts *opts,
                    const pbsim_depth_sink *sink, int64_t counts[6], int64_t hist[256]);
/* The report text, no device needed: one line "# records=N counted=N skipped_flag=N skipped_unplaced=N skipped_mapq=N
 * clipped=N", then per reference with l_ref > 0 "R\t<name>\t<l_ref>\t<covered>\t<sum>\t<max>\t<sum * 1000 / l_ref>" (integer
 * division), then for each d with hist[d] > 0, ascending, "H\t<d>\t<positions>".  names[r]: NUL-terminated.  Returns the text's
 * length, and writes it (no NUL) where buf holds cap >= that many bytes; -1: bad argument. */
int64_t pbsim_depth_report(const int64_t counts[6], int32_t n_ref, const char *const *names, const int64_t *rows,
                           const int64_t hist[256], char *buf, int64_t cap);
/* A summary of the reads of one or more BAM files on the GPU: lengths, error rates, qualities (what `samtools stats`, NanoStat
 * or cramino tell) -- of a real run, the numbers --length-mean / --length-sd / --length-min / --length-max, --accuracy-mean,
 * --difference-ratio and the sampling method's --accuracy-min / --accuracy-max ask for; of a simulated run, whether the reads
 * came out that way.  files[0..n_files), n_files >= 1: each is BGZF (inflated on the GPU), one plain gzip stream (zlib on the
 * host) or an uncompressed BAM stream, an unaligned BAM, a truth BAM or a mapper's BAM.  The files are taken one after the
 * other and summed into one result (a wgs job writes one truth file per FASTA record); headers are not compared; a file's
 * stream is freed when its pass is done.  Every quantity is an integer: the result is a function of the input alone.
 * Classes of a record, tested in this order: skipped_flag if flag & exclude_flags (default 0x900: each read counts once;
 * nothing more of such a record is looked at); else unaligned if flag & 4, refID < 0, pos < 0 or n_cigar_op == 0 (length and
 * quality only); else skipped_mapq if mapq < min_mapq (skipped wholly); else aligned.  counted = unaligned + aligned.
 * Length, over counted records with l_seq >= 1 (a counted record with l_seq == 0 adds to no_seq and takes no part in length or
 * quality): len_row = n, bases, min, max, mean_milli = bases * 1000 / n, sd = isqrt((n * sumsq - bases^2) / n^2), median = the
 * element (n - 1) / 2 of the ascending lengths, N10 .. N90: Nx the length of the first record, in descending order, at which
 * running sum * 100 >= x * bases.  All divisions are integer divisions; with n == 0 every field is 0.
 * Alignment, over aligned records.  The CIGAR is resolved as pbsim_bam_depth resolves it (the <l_seq>S<span>N placeholder is
 * replaced by the CG:B,I array).  m = the M, = and X lengths, ins the I, del the D lengths, ins_events / del_events the ops of
 * that kind with length >= 1, soft, hard; cols = m + ins + del.  NM is the first aux field named NM of type c C s S i I, found
 * by walking the aux fields by type until what is wanted (NM; the CG array where the CIGAR is the placeholder) has been found;
 * a record without one, or with a negative value, adds to no_nm; one with nm < ins + del, nm - ins - del > m or cols == 0 adds to
 * nm_bad; every other aligned record is scored, sub = nm - ins - del, identity_ppm = (cols - nm) * 1000000 / cols,
 * hist_identity[identity_ppm / 1000] += 1.  An aux field that runs past the record or has an unknown type, met on that walk,
 * or a CIGAR op code above 8, in an aligned record, fails the call with the record's inflated offset.
 * Quality, over counted records with l_seq >= 1: a first quality byte 0xFF adds to no_qual, and the record takes no part.
 * Else per base q' = min(q, 127), hist_q[q'] += 1; per read esum = the sum of E[q'], E[q] = round(2^32 10^(-q/10)),
 * acc_ppm = 1000000 - esum * 1000000 / (l_seq << 32), hist_qacc[acc_ppm / 1000] += 1: the sampling method's accuracy
 * 1 - mean(10^(-Q/10)) in fixed point, so that it does not depend on the order of the additions (it is not the double the
 * sampling profile computes).
 * counts: records, skipped_flag, unaligned, skipped_mapq, aligned, no_seq, no_qual, no_nm, nm_bad, scored.  totals, the first
 * nine over scored records: cols, sub, ins, del, ins_events, del_events, soft, hard, identity_sum; then the sum of acc_ppm, the
 * number of reads it is over, and the sum of q' over all their bases.
 * The per-read text, only where sink->on_text is not NULL (nothing of it is computed otherwise), in offset order, in pieces of
 * at most piece_bytes (a piece may end inside a line), one line per counted record, in file order and then record order:
 *   name\tclass\tlength\tcols\tnm\tins\tdel\tsoft\tidentity_ppm\tmean_q_milli\tacc_ppm\n
 * name the read name's bytes in front of the first NUL, class A (aligned) or U, length l_seq; cols, ins, del, soft of an aligned
 * record, nm where it has a value that is not negative, identity_ppm where it is scored, mean_q_milli = the sum of q' * 1000 /
 * l_seq and acc_ppm where it has qualities; a field its record does not define is "*".  The first callback comes when every
 * file has been read: after a failure no callback has seen partial text.
 * tests/stats_model.py states the rule in plain Python.  exclude_flags outside 0 .. 65535, min_mapq outside 0 .. 255 and a
 * negative piece_bytes fail before any device work; a file of 2^36 inflated bytes or more and 2^31 records or more in total are
 * refused; an allocation that does not fit fails with the bytes it needed; a tables-only context fails as pbsim_inflate_buffer
 * does.  After any failure the context stays usable. */
typedef struct pbsim_stats_file {
  const void *bam;
  int64_t n;
} pbsim_stats_file;
typedef struct pbsim_stats_opts { /* NULL: {0x900, 0, 0} */
  int32_t exclude_flags, min_mapq;
  int64_t piece_bytes; /* 0: the default; else the most text one on_text call carries */
} pbsim_stats_opts;
typedef struct pbsim_stats_sink {
  void *user;
  int (*on_text)(void *user, const char *bytes, int64_t n, int64_t offset); /* in offset order; may be NULL */
} pbsim_stats_sink;
int pbsim_bam_stats(pbsim_ctx *ctx, const pbsim_stats_file *files, int n_files, const pbsim_stats_opts *opts,
                    const pbsim_stats_sink *sink, int64_t counts[10], int64_t len_row[16], int64_t totals[12],
                    int64_t hist_q[128], int64_t hist_identity[1001], int64_t hist_qacc[1001]);
/* The report text, no device needed: "# records=N skipped_flag=N unaligned=N skipped_mapq=N aligned=N no_seq=N no_qual=N no_nm=N
 * nm_bad=N scored=N"; "L" and the sixteen values of len_row; "E\t<sub>\t<ins>\t<del>\t<cols>", their three rates in ppm of
 * cols, the sub : ins : del split in permille of sub + ins + del, and identity_sum / scored; "Q\t<acc_sum / acc_reads>\t<q_sum
 * * 1000 / the bases of hist_q>" (integer divisions; 0 where the divisor is 0); then "HQ\t<q>\t<bases>", "HI\t<bin>\t<reads>" and
 * "HA\t<bin>\t<reads>" for the bins that are not empty, ascending.  Returns the text's length, and writes it (no NUL) where buf
 * holds cap >= that many bytes; -1: bad argument. */
int64_t pbsim_stats_report(const int64_t counts[10], const int64_t len_row[16], const int64_t totals[12],
                           const int64_t hist_q[128], const int64_t hist_identity[1001], const int64_t hist_qacc[1001],
                           char *buf, int64_t cap);
/* The error profile of the aligned reads of one or more BAM files against the genome they were aligned to, on the GPU: the
 * substitution matrix, the indel length spectrum, deletions by homopolymer class with the --hp-del-bias they suggest, the
 * reported qualities against the errors found, and NM checked against the genome (what `samtools stats -r`, alfred or NanoOK
 * tell).  No MD tag, no = / X ops and no NM tag are needed: the genome lies in HBM beside the records.
 * The genome: refs[0..n_refs), n_refs >= 1, each {name, lines, bytes}: name NUL-terminated and compared as bytes, two equal
 * names are refused; lines[0..bytes) are the record's sequence lines, line feeds allowed and dropped.  Each record is prepared
 * as the simulator prepares its reference (tests/ref_prep_model.py): a-z upper-cased, and one class byte per base, the length of
 * its homopolymer run up to 11 (beyond: 11 odd, 10 even), N class 1; a run never joins the next record's.  The whole genome
 * stays in HBM, 2 bytes per base, while the files pass one after another.
 * files[0..n_files), n_files >= 1, each {bam, n, ref_name}: BGZF (inflated on the GPU), one plain gzip stream or an uncompressed
 * BAM stream.  A file's reference is looked up in the genome by its name -- by ref_name where that is not NULL, which is refused
 * for a file that has not exactly one reference (a wgs truth file calls its reference "ref").  Found with an l_ref that is not
 * the record's number of bases, the call fails and names both.
 * Every quantity is an integer: the result is a function of the input alone, whatever the order of records or files.
 * Class of a record, tested in this order: skipped_flag if flag & exclude_flags (default 0x900); unaligned if flag & 4, refID
 * outside 0 .. n_ref - 1, pos < 0 or n_cigar_op == 0; skipped_mapq if mapq < min_mapq; skipped_ref if the genome lacks its
 * reference; else aligned.  Nothing more of a record of the first four classes is looked at.  The CIGAR of an aligned record is
 * resolved as pbsim_bam_depth resolves it (the <l_seq>S<span>N placeholder is replaced by the CG:B,I array) and NM is found as
 * pbsim_bam_stats finds it; an aux field that runs past the record or has an unknown type, met on that walk, or a CIGAR op code
 * above 8, fails the call with the record's inflated offset.  An aligned record is no_seq if l_seq == 0; else misfit if the
 * CIGAR's query length (M I S = X) is not l_seq or pos + its span (M D N = X) > l_ref; else scored.  Only a scored record's
 * bases, qualities and reference bases are read.
 * Columns of a scored record.  r, the reference class: A C G T -> 0 .. 3, every other byte 4.  b, the read class, from the
 * 4-bit code: 1 2 4 8 -> 0 .. 3; 0 (=) -> r, and 4 in an inserted base, which has no r; every other code 4.  An M, = or X
 * column adds to pair[5 r + b] and is ambiguous if r or b is 4, else a match if r == b, else a sub.  With v the reference
 * base's class byte, hp_cols[v] counts the M = X and D columns, hp_sub[v] the sub columns, hp_del[v] the D columns.  An I op of
 * length >= 1 adds to ins_events and ins_len[min(length, 63)], each of its bases to ins and ins_base[b]; a D op of length >= 1
 * to del_events and del_len[min(length, 63)], each of its bases to del and del_base[r].  S adds to soft, H to hard, N only
 * advances, P and ops of length 0 do nothing.  Where the record has qualities (the first byte is not 0xFF), with q' = min(q,
 * 127): qcal[q'][0] counts the M = X columns that are not ambiguous, qcal[q'][1] the sub columns, qcal[q'][2] the inserted bases.
 * Per scored record: cols = m + ins + del; with cols >= 1 identity_ppm = match * 1000000 / cols (integer division),
 * hist_identity[identity_ppm / 1000] += 1; nm_derived = sub + ins + del; no_nm if it has no NM or a negative one, else
 * nm_unchecked if ambiguous > 0, else nm_agree if NM == nm_derived, else nm_differ.
 * counts: records, skipped_flag, unaligned, skipped_mapq, skipped_ref, aligned, no_seq, misfit, scored, no_nm, nm_unchecked,
 * nm_agree, nm_differ, with_qual.  totals, over scored records: cols, match, sub, ambiguous, ins, del, ins_events, del_events,
 * soft, hard, identity_sum.
 * The fit, over the classes v = 1 .. 10: x = v - 1, c = hp_cols[v], d = hp_del[v]; W = sum c, Sx = sum c x, Sxx = sum c x^2,
 * Sy = sum d, Sxy = sum d x; Num = W Sxy - Sx Sy, Den = Sxx Sy - Sx Sxy.  fit_ok = 1 only where Sy > 0 and Den > 0; then
 * fit_bias_milli = 1000 + floor(9000 Num / Den), floored toward minus infinity and held to +-2^62, and fit_suggest_milli is
 * that value held to 1000 .. 10000; else all three are 0.  It is the weighted least-squares line of the deletion rate on the
 * class, slope over intercept: the simulator's deletion rate is proportional to 1 + (bias - 1) (v - 1) / 9 (pbsim.cpp:673-697).
 * The per-read text, only where sink->on_text is not NULL, in offset order, in pieces of at most piece_bytes (a piece may end
 * inside a line), one line per aligned record, in file order and then record order:
 *   name\tclass\tlength\tcols\tmatch\tsub\tambiguous\tins\tdel\tsoft\tnm_tag\tnm_derived\tidentity_ppm\n
 * class S (scored), N (no_seq) or F (misfit); length l_seq; cols, ins, del, soft from the CIGAR; nm_tag where NM is there and
 * not negative; match, sub, ambiguous and nm_derived of a scored record; identity_ppm where it has cols >= 1; a field its record
 * does not define is "*".  The first callback comes when every file has been read.
 * tests/errors_model.py states the rule in plain Python.  exclude_flags outside 0 .. 65535, min_mapq outside 0 .. 255, a
 * negative piece_bytes, a missing name and two equal names fail before any device work; a file of 2^36 inflated bytes or more
 * and 2^32 - 1 records or more in one file are refused; the stage holds the genome, one file's inflated stream and 93 bytes per
 * record (101 with the text) in HBM at once and does not chunk: an allocation that does not fit fails with the bytes it needed; a tables-only
 * context fails as pbsim_inflate_buffer does.  After any failure the context stays usable. */
typedef struct pbsim_errors_ref {
  const char *name;
  const void *lines;
  int64_t bytes;
} pbsim_errors_ref;
typedef struct pbsim_errors_file {
  const void *bam;
  int64_t n;
  const char *ref_name; /* NULL: the file's own reference names */
} pbsim_errors_file;
typedef struct pbsim_errors_opts { /* NULL: {0x900, 0, 0} */
  int32_t exclude_flags, min_mapq;
  int64_t piece_bytes; /* 0: the default; else the most text one on_text call carries */
} pbsim_errors_opts;
typedef struct pbsim_errors_sink {
  void *user;
  int (*on_text)(void *user, const char *bytes, int64_t n, int64_t offset); /* in offset order; may be NULL */
} pbsim_errors_sink;
typedef struct pbsim_errors_result {
  int64_t counts[14];
  int64_t totals[11];
  int64_t pair[25];
  int64_t hp_cols[12], hp_sub[12], hp_del[12];
  int64_t ins_len[64], del_len[64];
  int64_t ins_base[5], del_base[5];
  int64_t qcal[128][3];
  int64_t hist_identity[1001];
  int64_t fit_ok, fit_bias_milli, fit_suggest_milli;
} pbsim_errors_result;
int pbsim_bam_errors(pbsim_ctx *ctx, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files,
                     const pbsim_errors_opts *opts, const pbsim_errors_sink *sink, pbsim_errors_result *result);
/* The report text, no device needed (the three fit fields are not read: the fit is made again from hp_cols and hp_del):
 * "# records=N skipped_flag=N .. with_qual=N", the counts by their names; "E" and the first ten totals, then sub, ins and del in
 * ppm of cols and identity_sum / the reads of hist_identity; five lines "M\t<A C G T N>" with the row of pair; "HP\t<v>\t<cols>\t
 * <sub>\t<del>\t<del * 1000000 / cols>" per class with cols > 0; "B\t<fit_ok>\t<fit_bias_milli>\t<fit_suggest_milli>"; "IL\t<bin>\t
 * <events>" and "DL\t<bin>\t<events>" for the bins that are not empty; "IB" and "DB" with the five values of ins_base and
 * del_base; "QC\t<q>\t<cols>\t<sub>\t<ins>\t<empirical Q milli>" per q with a value that is not 0, the last floor(-10000 log10(sub
 * / cols)) in double arithmetic, "*" where cols or sub is 0; "HI\t<bin>\t<reads>".  Integer divisions; 0 where the divisor is 0.
 * Returns the text's length, and writes it (no NUL) where buf holds cap >= that many bytes; -1: bad argument. */
int64_t pbsim_errors_report(const pbsim_errors_result *result, char *buf, int64_t cap);
/* The pileup of the aligned reads of one or more BAM files against the genome they were aligned to, on the GPU: per reference
 * position what the reads say there, the call of every site and the sites where the pile does not spell the genome (what
 * `samtools mpileup`, `samtools consensus`, pysamstats --type variation or bam-readcount tell).
 * The genome (refs), the files, the references looked up by name, the l_ref check, the container kinds and every refusal are
 * pbsim_bam_errors's; so are the classes of a record (skipped_flag with exclude_flags, default 0x900; unaligned; skipped_mapq
 * with min_mapq; skipped_ref; aligned; then no_seq, misfit, scored) and the resolution of the CIGAR with the CG placeholder.  Only
 * a scored record adds to the pileup.  counts: records, skipped_flag, unaligned, skipped_mapq, skipped_ref, aligned, no_seq,
 * misfit, scored.
 * Cells.  Every position p of every genome record has eight cells: 0 .. 3 A C G T, 4 other, 5 del, 6 ins, 7 masked.  A cell is
 * an unsigned 32-bit number and additions to it are modulo 2^32 (below 2^32 scored records only the ins cell can wrap, through
 * that many I ops at one anchor); everything made from cells (depth, the sums) is 64-bit arithmetic on the cells' values.
 * Columns.  r, the reference class, and b, the read class, are pbsim_bam_errors's (codes 1 2 4 8 -> 0 .. 3, code 0 -> r, every
 * other code 4; a genome byte that is not A C G T has r = 4).  An M, = or X column at reference position p adds 1 to cell b of p
 * -- unless the record has qualities (its first quality byte is not 0xFF) and the base's quality byte is below min_baseq
 * (default 0): then it adds 1 to masked and nothing else.  A record without qualities is never masked.  A D column adds 1 to
 * del.  N only advances; S, H, P and ops of length 0 do nothing.
 * Insertions.  An I op of length >= 1 that begins where the record's reference position is q adds 1 to ins of q - 1 where
 * q > pos, whichever op moved the position there; with q == pos (nothing of the reference consumed yet) it adds 1 to
 * ins_unanchored and to no position.  Inserted bases are not looked at and their qualities mask nothing.
 * Sites, over every position of every genome record.  depth = A + C + G + T + other + del (ins and masked are no part of it).
 * A site is ref_n if the genome's class is 4; else low if depth < min_depth (default 1: an uncovered site is low); else called.
 * The call is the largest of the five cells A C G T del; among equals the genome's own class wins if it is one of them, else the
 * first in that order (so a called site whose five cells are all 0 -- only other there, or min_depth 0 -- calls the genome's
 * base).  A called site is concordant if the call is the genome's class, a del_site if the call is del, else a sub_site;
 * apart from that it is an ins_site if 2 ins > depth.  discordant counts the called sites that are a sub_site, a del_site or
 * an ins_site, each once.  sites[]: sites, ref_n, low, called, concordant, sub_site, del_site, ins_site, discordant.
 * cell_sums[k]: the sum of cell k over all positions.  max_depth: the largest depth of any position.  hp_called[v], hp_sub[v],
 * hp_del[v], hp_ins[v]: the called sites, sub_sites, del_sites and ins_sites by the genome's class byte v, min(v, 11) as
 * pbsim_bam_errors takes it: the consensus errors inside homopolymers.
 * The text, only where sink->on_text is not NULL, in offset order, in pieces of at most piece_bytes (a piece may end inside a
 * line), genome records in their order and positions ascending; format 0 (sites): the discordant sites only; format 1 (all):
 * every position.  One line per site:
 *   name\tpos1\tref\tdepth\tA\tC\tG\tT\tN\tdel\tins\tmasked\tcall\tclass\n
 * name the genome record's; pos1 = p + 1; ref the prepared genome byte; N the other cell; call one of A C G T, * for del, and .
 * where the site is not called; class one of ref_n, low, match, sub, del, match+ins, sub+ins, del+ins.
 * The cells themselves, only where sink->on_cells is not NULL: a host copy per genome record in order, l_ref x 8 values,
 * position-major, after the text.
 * tests/pileup_model.py states the rule in plain Python.  exclude_flags outside 0 .. 65535, min_mapq and min_baseq outside
 * 0 .. 255, min_depth < 0, format outside 0 and 1, a negative piece_bytes, a missing name and two equal names fail before any
 * device work; a file of 2^36 inflated bytes or more and 2^32 - 1 records or more in one file are refused.  The stage holds in
 * HBM at once the genome at 2 bytes per base, the cells at 32 bytes per position, a class byte per position, one file's inflated
 * stream and 69 bytes per record (and the text), and does not chunk: an allocation that does not fit fails with the bytes it
 * needed; a tables-only context fails as pbsim_inflate_buffer does.  After any failure the context stays usable. */
typedef struct pbsim_pileup_opts { /* NULL: {0x900, 0, 0, 0, 1, 0} */
  int32_t exclude_flags, min_mapq, min_baseq;
  int32_t format;      /* 0 sites, 1 all */
  int64_t min_depth;
  int64_t piece_bytes; /* 0: the default; else the most text one on_text call carries */
} pbsim_pileup_opts;
typedef struct pbsim_pileup_sink {
  void *user;
  int (*on_text)(void *user, const char *bytes, int64_t n, int64_t offset); /* in offset order; may be NULL */
  int (*on_cells)(void *user, int32_t ref, const uint32_t *cells, int64_t l_ref); /* host copy, l_ref x 8, per genome record in
                                                                                      order, after the text; may be NULL */
} pbsim_pileup_sink;
typedef struct pbsim_pileup_result {
  int64_t counts[9];
  int64_t sites[9];
  int64_t cell_sums[8];
  int64_t ins_unanchored, max_depth;
  int64_t hp_called[12], hp_sub[12], hp_del[12], hp_ins[12];
} pbsim_pileup_result;
int pbsim_bam_pileup(pbsim_ctx *ctx, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files,
                     const pbsim_pileup_opts *opts, const pbsim_pileup_sink *sink, pbsim_pileup_result *result);
/* The report text, no device needed: "# records=N skipped_flag=N .. scored=N", the counts by their names; "S" and the nine values
 * of sites, then discordant * 1000000 / called (integer division; 0 where called is 0) and the consensus quality floor(-10000
 * log10(discordant / called)) in double arithmetic, "*" where either is 0; "C" and the eight values of cell_sums, then
 * ins_unanchored and max_depth; "HP\t<v>\t<called>\t<sub>\t<del>\t<ins>" per class with a value that is not 0.  Returns the text's
 * length, and writes it (no NUL) where buf holds cap >= that many bytes; -1: bad argument. */
int64_t pbsim_pileup_report(const pbsim_pileup_result *result, char *buf, int64_t cap);
/* The consensus FASTA of the aligned reads of one or more BAM files against the genome they were aligned to, on the GPU: the
 * sequence the pile of reads spells, as `samtools consensus` or a polisher would hand it back.
 * Front half.  The genome, the files, the references by name, the record classes, the CIGAR resolution, the cells and the sites
 * are exactly pbsim_bam_pileup's, with the same options exclude_flags, min_mapq, min_baseq and min_depth: counts[9], sites[9],
 * ins_unanchored and max_depth equal pbsim_bam_pileup's on the same input.
 * Insertion cells.  An I op of length L >= 1 of a scored record that is anchored at position a (the pileup's rule: a = q - 1 with
 * q > pos) adds, for every offset j with 0 <= j < min(L, max_ins), 1 to cell b of (a, j), b the read class of the inserted
 * base's 4-bit code: 1 2 4 8 -> 0 .. 3, every other code (0 included) -> 4.  Inserted bases' qualities mask nothing.  The cells
 * are unsigned 32-bit numbers, additions modulo 2^32; n(a, j) is the sum of the five cells, so n(a, 0) is the pileup's ins cell
 * of a.  Unanchored insertions add nowhere.
 * The consensus of a position p of a genome record.  A ref_n or low site emits one byte: with fill 0 `N`, with fill 1 the
 * prepared genome byte.  A called site emits its call (A C G T); a site that calls del emits nothing.  A called site that is an
 * ins_site (2 ins > depth) then emits the insertion: for j = 0, 1, .. while j < max_ins and 2 n(p, j) > depth(p) the largest
 * of the A C G T cells of (p, j), among equals the first, and `N` where all four are 0.  n(p, j) does not increase with j, so
 * the insertion is a prefix and its first base is there exactly when the site is an ins_site.
 * The FASTA.  Genome records in their order, each `>name\n`, then its consensus bases in lines of line_width bases (0: one
 * line) with `\n` after every line, the last partial one included; a record of no consensus bases is its header line alone.
 * bases[]: out (all bases written), kept (concordant sites), sub, ins (inserted bases emitted), fill, del (called sites that
 * emit nothing): out = kept + sub + ins + fill and sites = kept + sub + del + fill.  ins_sites; ins_longest, the longest
 * insertion emitted; ins_capped, the ins_sites whose insertion has exactly max_ins bases; ins_len[v], the ins_sites by
 * min(length, 63); text_bytes, the size of the FASTA (also where no text is asked for).
 * Sink.  on_text: the FASTA in offset order in pieces of at most piece_bytes; on_record(user, ref, l_ref, l_cons): per genome
 * record in order, after the text, its length and that of its consensus.  Either may be NULL; with no on_text no text is made,
 * but the result is complete.
 * tests/consensus_model.py states the rule in plain Python.  fill outside 0 and 1, max_ins outside 1 .. 65535, line_width
 * outside 0 .. 2^20 and everything pbsim_bam_pileup refuses fail before any device work.  Beside what the pileup holds in HBM
 * the stage keeps 8 bytes per inserted base of an anchored I op (below max_ins) until the sites are called, then 20 bytes per
 * base of the longest insertion seen at each ins_site.  After any failure the context stays usable and the result is zeroed. */
typedef struct pbsim_consensus_opts { /* NULL: {0x900, 0, 0, 0, 1, 1024, 60, 0} */
  int32_t exclude_flags, min_mapq, min_baseq;
  int32_t fill;        /* 0: N at a ref_n or low site, 1: the prepared genome byte */
  int64_t min_depth;
  int32_t max_ins;     /* 1 .. 65535: the most bases one insertion emits */
  int32_t line_width;  /* 0 .. 2^20, 0: one line per record */
  int64_t piece_bytes; /* 0: the default; else the most text one on_text call carries */
} pbsim_consensus_opts;
typedef struct pbsim_consensus_sink {
  void *user;
  int (*on_text)(void *user, const char *bytes, int64_t n, int64_t offset); /* in offset order; may be NULL */
  int (*on_record)(void *user, int32_t ref, int64_t l_ref, int64_t l_cons);  /* per genome record, after the text; may be NULL */
} pbsim_consensus_sink;
typedef struct pbsim_consensus_result {
  int64_t counts[9];
  int64_t sites[9];
  int64_t ins_unanchored, max_depth;
  int64_t bases[6];
  int64_t ins_sites, ins_longest, ins_capped;
  int64_t ins_len[64];
  int64_t text_bytes;
} pbsim_consensus_result;
int pbsim_bam_consensus(pbsim_ctx *ctx, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files,
                        const pbsim_consensus_opts *opts, const pbsim_consensus_sink *sink, pbsim_consensus_result *result);
/* The report text, no device needed: the "#" line of the counts and the "S" line as pbsim_pileup_report writes them; "K" and the
 * six values of bases, then ins_sites, ins_longest and ins_capped; "IL\t<bin>\t<sites>" for the bins of ins_len that are not
 * empty.  Returns the text's length, and writes it (no NUL) where buf holds cap >= that many bytes; -1: bad argument. */
int64_t pbsim_consensus_report(const pbsim_consensus_result *result, char *buf, int64_t cap);
/* The differences between the genome and what the pile of aligned reads of one or more BAM files spells, as VCFv4.2, on the GPU:
 * the haploid variants the reads support, each as one event.
 * Front half.  Everything up to the insertion every ins_site emits is pbsim_bam_consensus's, with the same options exclude_flags,
 * min_mapq, min_baseq, min_depth and max_ins: counts[9], sites[9], ins_unanchored and max_depth equal that stage's.
 * What a position p spells, E(p).  A ref_n or low site spells the prepared genome byte (the consensus with fill 1); a called
 * site spells its call, or nothing where it calls del; an ins_site -- a del_site that is one included -- then spells its insertion
 * as the consensus emits it.
 * Groups.  Within one genome record every position that is not a del_site is an anchor.  An anchor's group is the anchor and the
 * run of del_sites directly behind it, up to the next anchor or the record's end; the record's first anchor also takes the
 * del_sites in front of it (VCF's rule for an event at position 1: the base behind it is included).  No group crosses into
 * another genome record.  A genome record that has positions and no anchor writes nothing: it counts in unplaced_records and its
 * positions in unplaced_sites.
 * Records.  For a group over positions lo .. hi REF is the prepared genome bytes of lo .. hi and ALT is E(lo) .. E(hi) joined; a
 * record is written exactly when ALT differs from REF as byte strings (a deleted base that the insertion at its own site puts
 * back gives none).  The records are ascending and do not overlap; applied to the prepared genome they give the consensus with
 * fill 1.  The line: name, POS = lo + 1, `.`, REF, ALT, `.`, `.`, `DP=d;MS=m;TYPE=t`, tab-separated.  DP is the depth at the
 * group's anchor.  MS, the minimum support, is the smallest over the group of: the call's cell at a sub_site, the del cell at
 * every del_site, n(p, j) for every inserted base emitted.  TYPE: snv where both strings have one byte; ins where REF has one
 * byte and ALT begins with it; del where ALT has one byte and REF begins with it; else complex.  QUAL and FILTER are `.`: the
 * stage has no probability model.  No sample columns, no left-normalisation.
 * The header, written by the host in front of the records: fileformat, source, one contig line per genome record in order (empty
 * ones included), three INFO lines (DP, MS, TYPE), the column line.  It counts in text_bytes.
 * types[]: snv, ins, del, complex; ref_bases, alt_bases: the bytes of all REF and all ALT strings; longest_ref, longest_alt;
 * header_bytes; text_bytes, header and records (also where no text is asked for).
 * Sink.  on_text: the VCF in offset order in pieces of at most piece_bytes; on_record(user, ref, l_ref, n_variants): per genome
 * record in order, after the text.  Either may be NULL; with no on_text no text is made, but the result is complete.
 * tests/call_model.py states the rule in plain Python.  max_ins outside 1 .. 65535 and everything pbsim_bam_pileup refuses fail
 * before any device work.  The stage holds what pbsim_bam_consensus holds, and the text.  One lane walks a whole group: a
 * deletion run of n positions costs n steps of one lane.  After any failure the context stays usable and the result is zeroed. */
typedef struct pbsim_call_opts { /* NULL: {0x900, 0, 0, 1024, 1, 0} */
  int32_t exclude_flags, min_mapq, min_baseq;
  int32_t max_ins;     /* 1 .. 65535: the most bases one insertion emits */
  int64_t min_depth;
  int64_t piece_bytes; /* 0: the default; else the most text one on_text call carries */
} pbsim_call_opts;
typedef struct pbsim_call_sink {
  void *user;
  int (*on_text)(void *user, const char *bytes, int64_t n, int64_t offset);    /* in offset order; may be NULL */
  int (*on_record)(void *user, int32_t ref, int64_t l_ref, int64_t n_variants); /* per genome record, after the text; may be NULL */
} pbsim_call_sink;
typedef struct pbsim_call_result {
  int64_t counts[9];
  int64_t sites[9];
  int64_t ins_unanchored, max_depth;
  int64_t variants;
  int64_t types[4];
  int64_t ref_bases, alt_bases, longest_ref, longest_alt;
  int64_t unplaced_records, unplaced_sites;
  int64_t header_bytes, text_bytes;
} pbsim_call_result;
int pbsim_bam_call(pbsim_ctx *ctx, const pbsim_errors_ref *refs, int n_refs, const pbsim_errors_file *files, int n_files,
                   const pbsim_call_opts *opts, const pbsim_call_sink *sink, pbsim_call_result *result);
/* The report text, no device needed: the "#" line of the counts and the "S" line as pbsim_pileup_report writes them; "V" and
 * variants, the four types, ref_bases, alt_bases, longest_ref, longest_alt, unplaced_records and unplaced_sites.  Returns the
 * text's length, and writes it (no NUL) where buf holds cap >= that many bytes; -1: bad argument. */
int64_t pbsim_call_report(const pbsim_call_result *result, char *buf, int64_t cap);
/* A variant genome and its truth variants drawn from a genome and a seed on the GPU: SNVs, insertions and deletions, the variant
 * genome as FASTA (to simulate from) and the variants as VCFv4.2 in the dialect pbsim_bam_call writes, so that a call set can be
 * compared with the truth (pbsim_vcf_compare).  No BAM is read: refs are the genome's records as pbsim_bam_errors takes them (the line
 * feeds dropped, a-z upper-cased, each record on its own; two equal names, a missing name and a record of 2^31 - 1 bases or more
 * are refused; empty records are allowed).
 * Draws.  D(r, p, sub, j) is word j % 4 of philox4x32_10(ctr = (j / 4, sub, p, r), key = (seed, 0x4D555441)) shifted right by one
 * (31 bits), r the record's index in refs and p the 0-based position.  Nothing else enters a draw: the result does not depend on
 * tiles, grids or the other records' contents.
 * Events.  A position is eligible where its prepared byte is A, C, G or T; every other position draws nothing.  At an eligible p,
 * e = D(r, p, 0, 0) % 1000000: e < snv_ppm an snv, e < snv_ppm + ins_ppm an ins, e < snv_ppm + ins_ppm + del_ppm a del, else
 * nothing.  An ins or del has length L = 1 + the number of leading draws j = 0, 1, .. with D(r, p, 1, j) % 1000000 < ext_ppm, at
 * most max_indel.  A del at p covers p + 1 .. p + L, cut at the record's end and in front of the first byte that is not A C G T
 * (pbsim_bam_call spells the genome's byte at a ref_n site: a deleted N would not come back); a run cut to nothing is no event
 * and counts in void_del.  drawn[]: the snv, ins and del events that are left.
 * The deleted set is the union of all del runs, whatever happens to the events that drew them; a record's position 0 is never in
 * it.  At a deleted position an snv or ins is `dropped`, a del is `merged`: its run still counts in the union.
 * What p spells, E(p): nothing where p is deleted; at an snv "ACGT"[(i + 1 + D(r, p, 0, 1) % 3) % 4], i the genome's base; at an
 * ins the genome's byte, then L bases "ACGT"[D(r, p, 2, j) % 4], j = 0 .. L - 1; else the prepared byte.
 * FASTA.  Per record in order `>name`, then E(0) .. E(n - 1) joined in lines of line_width (0: one line), the layout of
 * pbsim_bam_consensus; an empty record writes only its header line.
 * VCF.  The positions that are not deleted are anchors; an anchor's group is the anchor and the deleted run behind it.  REF is the
 * group's prepared bytes, ALT is E(anchor); a line is written exactly where they differ: name, POS = anchor + 1, `.`, REF, ALT,
 * `.`, `.`, `TYPE=t`, tab-separated, t snv, ins or del as pbsim_bam_call types them (complex cannot arise).  No
 * left-normalisation.  The header, written by the host, counts in vcf_bytes: fileformat, source,
 * `##pbsim_mutate=seed=..;snv_ppm=..;ins_ppm=..;del_ppm=..;ext_ppm=..;max_indel=..`, one contig line per record, the TYPE INFO
 * line as pbsim_bam_call words it, the column line.
 * Origin map (where on_origin is set): one int32 per written base of a record: p for the base that stands for genome position p,
 * kept or substituted; -1 - p for a base inserted behind p.  With the per-base reference coordinates of pbsim_simulate_arrays it
 * takes a read simulated from the variant genome back to the original one.
 * Result.  variants = sum(types) = sum(drawn) - dropped - merged; bases_out = bases_in + inserted - deleted; substituted =
 * types[snv].  fasta_bytes and vcf_bytes are complete also where no text is asked for.
 * Sink.  on_fasta, then on_vcf: each text in offset order in pieces of at most piece_bytes; then per genome record in order
 * on_record(user, ref, l_ref, l_out, n_variants) and on_origin(user, ref, origin, l_out), origin a host copy that holds during the
 * call.  Each may be NULL; a text or map that is not asked for is not made.
 * tests/mutate_model.py states the rule in plain Python.  Bad options fail before any device work.  The stage holds the genome at
 * 2 bytes per base (as the BAM stages prepare it), three bytes and one 8-byte end per position, the texts and, where asked for, 4 bytes per written base in HBM at
 * once, and does not chunk; an allocation that does not fit fails with the bytes it needed.  One lane walks a whole deletion
 * group and writes a whole insertion.  After any failure the context stays usable and the result is zeroed. */
typedef struct pbsim_mutate_opts { /* NULL: {1, 1000, 100, 100, 500000, 50, 60, 0} */
  uint32_t seed;
  int32_t snv_ppm, ins_ppm, del_ppm; /* each 0 .. 1000000, their sum at most 1000000: events per million eligible positions */
  int32_t ext_ppm;                   /* 0 .. 999999: an indel grows by one base with this chance per million */
  int32_t max_indel;                 /* 1 .. 65535 */
  int32_t line_width;                /* 0 .. 1048576; 0: one line per record */
  int64_t piece_bytes;               /* 0: the default; else the most text one on_fasta or on_vcf call carries */
} pbsim_mutate_opts;
typedef struct pbsim_mutate_sink {
  void *user;
  int (*on_fasta)(void *user, const char *bytes, int64_t n, int64_t offset); /* in offset order; may be NULL */
  int (*on_vcf)(void *user, const char *bytes, int64_t n, int64_t offset);   /* in offset order, after the FASTA; may be NULL */
  int (*on_record)(void *user, int32_t ref, int64_t l_ref, int64_t l_out, int64_t n_variants); /* per genome record; may be NULL */
  int (*on_origin)(void *user, int32_t ref, const int32_t *origin, int64_t l_out);             /* behind its on_record; may be NULL */
} pbsim_mutate_sink;
typedef struct pbsim_mutate_result {
  int64_t records, bases_in, eligible, bases_out;
  int64_t drawn[3]; /* snv, ins, del */
  int64_t void_del, dropped, merged;
  int64_t substituted, inserted, deleted; /* bases */
  int64_t variants;
  int64_t types[3]; /* snv, ins, del */
  int64_t ref_bases, alt_bases, longest_ref, longest_alt;
  int64_t header_bytes, vcf_bytes, fasta_bytes;
} pbsim_mutate_result;
int pbsim_genome_mutate(pbsim_ctx *ctx, const pbsim_errors_ref *refs, int n_refs, const pbsim_mutate_opts *opts, const pbsim_mutate_sink *sink,
                        pbsim_mutate_result *result);
/* The report text, no device needed: a "#" line with the names and an "M" line with the values of the result in its order, the
 * arrays spread (drawn_snv, drawn_ins, drawn_del; snv, ins, del), tab-separated.  Returns the text's length, and writes it (no
 * NUL) where buf holds cap >= that many bytes; -1: bad argument. */
int64_t pbsim_mutate_report(const pbsim_mutate_result *result, char *buf, int64_t cap);
/* A call set scored against the truth variants on the GPU: two VCF texts over one genome, every indel moved to its leftmost
 * placement first, so that `c1 6 A AA` and `c1 3 A AA` over GCAAAAT are one insertion.  refs are the genome's records as
 * pbsim_bam_errors takes them (prepared: the line feeds dropped, a-z upper-cased).  ref_names (NULL: the records' own names) gives
 * per genome record the contig name the VCFs use for it; a missing or empty name and two equal names are refused.
 * Lines.  A line ends at \n; a \r just in front of that \n is dropped; the last line needs no \n.  Empty lines and lines that begin
 * with # are not data lines.  Data lines are numbered from 1 per file.  Columns are separated by tabs: CHROM, POS, ID, REF, ALT,
 * QUAL, FILTER, INFO; FILTER is present where the line has seven columns, INFO where it has eight.
 * Classes.  The first that applies takes a data line out.  malformed: fewer than five columns, an empty CHROM, REF or ALT, a POS
 * that is not one or more digits with a value 1 .. 2^31 - 1.  unknown_contig: CHROM is none of the names, byte by byte.
 * unsupported: REF or ALT, a-z upper-cased, holds a byte outside ACGTN (so `,`, `<`, `*`, `.`).  ref_mismatch: REF runs past the
 * record's end or differs from the prepared genome bytes at POS - 1.  filtered: FILTER is present and neither `.` nor `PASS`; in
 * the calls also MS < min_ms, MS the value of the leading digits (held to 2^31 - 1) behind the first `MS=` that begins INFO or
 * follows a `;` in it, 0 without one.  no_change: REF equals ALT.
 * The form (r, s, d, X) of a line that is left: r the genome record, s = POS - 1; while REF and ALT both have bytes and their last
 * bytes agree both lose the last byte; while both have bytes and their first bytes agree both lose the first byte and s grows by 1;
 * if exactly one is empty now the other, Y, moves left: while s > 0 and the genome's byte at s - 1 equals Y's last byte, Y is
 * rotated right by one and s falls by 1.  The walk stays inside the record.  d is the length of what is left of REF, X what is
 * left of ALT, upper-cased: no padding base.  Type: snv where d = 1 and |X| = 1; ins where d = 0; del where |X| = 0; else complex.
 * Duplicates.  Within one file a line whose form equals that of an earlier line of the file is `dup`; the others are compared.
 * Verdicts.  Forms are equal where r, s, d and the bytes of X are.  A compared truth line is `found` where a compared call has an
 * equal form, else `missed`; a compared call is `tp` where a compared truth line has an equal form, else `fp_site` where one has
 * the same (r, s), else `fp`.  MATE is the number of the line with the equal form in the other file, else 0.
 * Result.  files[truth, calls][]: lines, malformed, unknown_contig, unsupported, ref_mismatch, filtered, no_change, dup, compared,
 * shifted (lines the left move moved, dup ones included), longest_shift (steps).  types[snv, ins, del, complex][]: truth, found,
 * calls, tp, fp (fp_site included), fp_site.  lengths[ins, del][bin][]: truth, found, calls, tp, the bin by |X| of an ins and d of
 * a del: 1, 2-5, 6-15, 16-49, 50+.  ms[min(MS, 63)][]: tp, fp of the compared calls.  text_bytes: the annotated text's size under
 * `lines`, also where no text is asked for.
 * The annotated text (sink->on_text, in offset order in pieces of at most piece_bytes; NULL: none is made): the header line
 * `#file line CHROM POS REF ALT type start ref_len alt verdict mate` (tab-separated, as every line), then one line per data line,
 * truth first, each file in order: T or C, the line's number, CHROM, POS, REF, ALT as in the file (`.` for a column the line lacks
 * or that is empty), the type, s + 1, d, X (`.` where X is empty; all four `.` for a line a class took out), the verdict or the
 * class, MATE.  lines 0 leaves out `found` and `tp`; lines 1 writes every data line.
 * tests/compare_model.py states the rule in plain Python.  lines outside 0 .. 1, a negative min_ms or piece_bytes and a bad name
 * fail before any device work.  Limits: both files' data lines together number below 2^31; no data line is longer than 2^31 - 1
 * bytes; the genome's limits are pbsim_bam_errors's.  The stage holds the genome (2 bytes per base), both texts, 104 bytes per data
 * line, the sort's scratch and the annotated text in HBM at once and does not chunk.  One lane parses a whole line and walks a whole left move: a
 * tandem repeat of n bases costs n steps of one lane; one lane walks its run of lines at one (r, s), quadratic in the run's length.
 * After any failure the context stays usable and the result is zeroed. */
typedef struct pbsim_compare_opts { /* NULL: {0, 0, 0} */
  int32_t lines;       /* 0: the annotated text leaves out found and tp; 1: every data line */
  int32_t min_ms;      /* 0 .. 2^31 - 1: a call with MS below it is filtered */
  int64_t piece_bytes; /* 0: the default; else the most text one on_text call carries */
} pbsim_compare_opts;
typedef struct pbsim_compare_sink {
  void *user;
  int (*on_text)(void *user, const char *bytes, int64_t n, int64_t offset); /* in offset order; may be NULL */
} pbsim_compare_sink;
typedef struct pbsim_compare_result {
  int64_t files[2][11];
  int64_t types[4][6];
  int64_t lengths[2][5][4];
  int64_t ms[64][2];
  int64_t text_bytes;
} pbsim_compare_result;
int pbsim_vcf_compare(pbsim_ctx *ctx, const pbsim_errors_ref *refs, int n_refs, const char *const *ref_names, const void *truth, int64_t n_truth,
                      const void *calls, int64_t n_calls, const pbsim_compare_opts *opts, const pbsim_compare_sink *sink,
                      pbsim_compare_result *result);
/* The report text, no device needed: "#" and the names of files[], "T" and "C" with the values; "P\t<type>" per type and for `all`
 * with truth, found, calls, tp, fp, fp_site, recall_ppm = found * 1000000 / truth and precision_ppm = tp * 1000000 / calls (integer
 * division; 0 where the denominator is 0); "L\t<ins|del>\t<bin>" with the four numbers for the bins that are not all 0;
 * "Q\t<ms>" with tp, fp and the sums of tp and fp over this bin and all higher ones -- what min_ms = ms would leave -- for the bins
 * that are not empty.  Returns the text's length, and writes it (no NUL) where buf holds cap >= that many bytes; -1: bad argument. */
int64_t pbsim_compare_report(const pbsim_compare_result *result, char *buf, int64_t cap);
/* A VCF applied to a genome on the GPU, per haplotype: the genome's records with the lines' alleles spliced in, as FASTA (to
 * simulate from), with an origin map on request.  It is the operation pbsim_bam_call's records and pbsim_genome_mutate's VCF are
 * defined by: the latter's VCF applied to its genome gives its FASTA.  Haplotypes 1 and 2 of a phased VCF give the two genomes of a
 * diploid sample.  refs and ref_names are pbsim_vcf_compare's.
 * Lines and columns.  Exactly pbsim_vcf_compare's.  Column 9 is FORMAT, column 10 + `sample` is the sample.
 * The allele.  ALT is split at commas into alleles 1 .. k.  With haplotype 0 the allele is 1.  With haplotype h = 1 or 2 FORMAT must
 * be `GT` or begin with `GT:`; the genotype is the sample column up to its first `:`, one or two fields of `.` or decimal digits
 * separated by one `/` or `|`; a genotype of one field serves both haplotypes; the allele is the value of field h.
 * Classes.  The first that applies takes a data line out.  malformed: any of pbsim_vcf_compare's malformed conditions, or an empty
 * allele between commas; with h != 0 also a missing sample column, a FORMAT that is not as above, a genotype that is not of that
 * shape (more than two fields too), an allele number above k.  unknown_contig: as there.  no_call: the field is `.`.  ref_allele:
 * the field's value is 0.  unsupported: REF or the chosen allele, a-z upper-cased, holds a byte outside ACGTN; the other alleles of
 * the line are not looked at.  ref_mismatch, filtered (FILTER only: there is no MS rule here), no_change (REF equals the allele): as
 * there.
 * The form (r, s, d, X) of a line that is left: r the genome record, s = POS - 1; while REF and the allele both have bytes and their
 * first bytes agree both lose the first byte and s grows by 1; then, while both have bytes and their last bytes agree both lose the
 * last byte.  The prefix goes first: VCF's padding base is the first one, so pbsim_genome_mutate's `A -> ACA` stays an insertion
 * behind its anchor.  d is the length of what is left of REF, X what is left of the allele, upper-cased.  There is no left move.
 * Types as pbsim_vcf_compare.  s = l_ref with d = 0 is legal: an insertion behind the record's last base.
 * Order and collisions.  The lines that are left are taken in order of (r, s, insertions before spans, line number), with end = 0 at
 * the start of each record.  An insertion (d = 0) is applied where s >= end and no insertion at this (r, s) has been applied.  A
 * span (d > 0) is applied where s >= end, and then end = s + d.  Every other line is `overlap`; its `by` is the number of the applied
 * line it ran into: the span that owns end, or the earlier insertion.  This is the greedy rule of `bcftools consensus`: a line that
 * lost blocks nothing (of [0,10), [5,20), [15,18) the first and the third are applied).  An insertion at the start of an applied
 * span and one at its end are both applied.
 * What comes out.  Per record, for p = 0 .. l_ref: the X of the insertion applied at p; then, for p < l_ref, the X of the span
 * applied at p, or nothing where p lies inside an applied span behind its start, or the prepared genome byte.  The FASTA layout is
 * pbsim_genome_mutate's; an empty record writes its header line only.
 * Origin map (where on_origin is set): one int32 per written base of a record: p for a kept base; s + i for byte i < min(d, |X|) of
 * a span's X; -1 - (s + d - 1) for the rest of a span's X; -1 - (s - 1) for the bytes of an insertion at s >= 1; -2^31 for the bytes
 * of an insertion at s = 0.  This is pbsim_genome_mutate's encoding plus the one value it never needs: its insertions have an anchor.
 * Result.  lines; one count per class; overlap; applied; types[snv, ins, del, complex] of the applied lines; bases_in; bases_out;
 * over the applied lines inserted (the sum of |X| - min(d, |X|)), deleted (of d - min), substituted (of min): bases_out = bases_in +
 * inserted - deleted; longest_cluster (below); fasta_bytes and text_bytes, both complete without their texts.
 * The annotated text (on_text): the header line `#line CHROM POS REF ALT allele type start ref_len alt verdict by` (tab-separated,
 * as every line), then one line per data line in file order: the line's number, CHROM, POS, REF, ALT, the type, s + 1, d and X
 * spelled as pbsim_vcf_compare spells them, `allele` the chosen number in front of the type (`.` for a malformed line and a
 * no_call), the verdict `applied`, `overlap` or the class, `by` (0 except for overlap).  lines 0 leaves out `applied`.
 * Sink.  on_fasta, then on_text: each text in offset order in pieces of at most piece_bytes; then per genome record in order
 * on_record(user, ref, l_ref, l_out, n_applied) and on_origin(user, ref, origin, l_out), origin a host copy that holds during the
 * call.  Each may be NULL; a text or map that is not asked for is not made.
 * tests/apply_model.py states the rule in plain Python.  Bad options and names fail before any device work.  With haplotype 1 or 2
 * a file that has data lines, none of them with the sample column, fails: "no data line has a sample column N".  Limits: the data
 * lines number below 2^31; no data line is longer than 2^31 - 1 bytes; a record has fewer than 2^31 - 1 bases; the genome's other
 * limits are pbsim_bam_errors's.  The stage holds the genome (2 bytes per base), the VCF text, 72 bytes per data line and 33 more
 * with the sort's scratch while the collisions are found, two 4-byte marks and one 8-byte end per position, the texts and, where asked for,
 * 4 bytes per written base in HBM at once and does not chunk.  One lane parses a whole line and writes a whole X.  The collisions
 * are found without a walk over all lines: the sorted lines are cut into clusters where a line begins at or behind the largest
 * s + d of all lines in front of it (and is not an insertion just behind an insertion of its (r, s)); such a line is applied
 * whatever came before, and one lane walks each cluster with the rule above, so a cluster of n lines costs n steps of one lane.
 * Clusters are one line long in any sane VCF; longest_cluster reports the longest.  After any failure the context stays usable and
 * the result is zeroed. */
typedef struct pbsim_apply_opts { /* NULL: {0, 0, 0, 60, 0} */
  int32_t haplotype;   /* 0: the first ALT of every line; 1, 2: that allele of the sample's GT */
  int32_t sample;      /* 0-based sample column, read where haplotype != 0 */
  int32_t lines;       /* 0: the annotated text leaves out `applied`; 1: every data line */
  int32_t line_width;  /* 0 .. 1048576; 0: one line per record */
  int64_t piece_bytes; /* 0: the default; else the most text one on_fasta or on_text call carries */
} pbsim_apply_opts;
typedef struct pbsim_apply_sink {
  void *user;
  int (*on_fasta)(void *user, const char *bytes, int64_t n, int64_t offset); /* in offset order; may be NULL */
  int (*on_text)(void *user, const char *bytes, int64_t n, int64_t offset);  /* in offset order, after the FASTA; may be NULL */
  int (*on_record)(void *user, int32_t ref, int64_t l_ref, int64_t l_out, int64_t n_applied); /* per genome record; may be NULL */
  int (*on_origin)(void *user, int32_t ref, const int32_t *origin, int64_t l_out);            /* behind its on_record; may be NULL */
} pbsim_apply_sink;
typedef struct pbsim_apply_result {
  int64_t lines;
  int64_t malformed, unknown_contig, no_call, ref_allele, unsupported, ref_mismatch, filtered, no_change;
  int64_t overlap, applied;
  int64_t types[4]; /* snv, ins, del, complex */
  int64_t bases_in, bases_out, inserted, deleted, substituted;
  int64_t longest_cluster;
  int64_t fasta_bytes, text_bytes;
} pbsim_apply_result;
int pbsim_vcf_apply(pbsim_ctx *ctx, const pbsim_errors_ref *refs, int n_refs, const char *const *ref_names, const void *vcf, int64_t n_vcf,
                    const pbsim_apply_opts *opts, const pbsim_apply_sink *sink, pbsim_apply_result *result);
/* The report text, no device needed: a "#" line with the names and an "A" line with the values of the result in its order, types
 * spread (snv, ins, del, complex), tab-separated.  Returns the text's length, and writes it (no NUL) where buf holds cap >= that
 * many bytes; -1: bad argument. */
int64_t pbsim_apply_report(const pbsim_apply_result *result, char *buf, int64_t cap);
/* The 0-based sample column that `name` has in the first line of the VCF text that begins with `#CHROM` (its columns behind
 * FORMAT), no device needed; -1: no such line or no such name. */
int32_t pbsim_apply_sample(const void *vcf, int64_t n_vcf, const char *name);
/* An aligned BAM whose records lie on a variant genome, placed on the original genome on the GPU: the link between the truth BAM
 * of reads simulated from pbsim_genome_mutate's or pbsim_vcf_apply's FASTA and the stages that work against the original genome
 * (a mapper, pbsim_truth_bam_eval, pbsim_bam_errors).  refs are the ORIGINAL genome's records as pbsim_bam_errors takes them;
 * origins holds one origin map per genome record, as the on_origin of those two stages delivers it; file is the BAM (BGZF, gzip
 * or uncompressed), ref_name as in pbsim_bam_errors.  pos, bin, CIGAR and NM are made anew; every other byte of a record stays.
 * 1. References.  The file's reference k goes by its name (or by ref_name, for a file with exactly one reference) to a genome
 * record; a name the genome lacks fails the call.  Its l_ref must be the length of that record's origin map, else the call fails
 * with both numbers: "not the genome these reads came from".  In the lifted header every l_ref, and the LN: of the @SQ line whose
 * SN: is the reference's name, is the original record's length; an SO: value of a leading @HD line becomes `unsorted`; nothing
 * else of the text changes.
 * 2. Origin map.  One int32 per variant base: o >= 0 a kept or substituted base of original position o; -1 - p a base inserted
 * behind p; -2^31 a base inserted in front of position 0.  Checked on the device before use: kept values rise strictly and stay
 * below the original length; an inserted base names the last kept value in front of it, or -2^31 where there is none.  A violation
 * fails the call with the reference's name and the first faulty variant position.
 * 3. `unaligned`, copied unchanged: flag & 4, refID outside [0, n_ref), pos < 0, or no CIGAR.
 * 4. `unsupported`, dropped: the resolved CIGAR (the CG:B,I array where the field is the <l_seq>S<span>N placeholder) holds an N
 * or P op.  A record with an op code above 8, with aux fields that run past it or have an unknown type, with a CIGAR that runs
 * past its reference or, where l_seq != 0, a query length that is not l_seq fails the call with its inflated offset.
 * Columns, in order; M stands for M, = and X; v is the variant base, o = origin[v].
 * 5. An M column with o >= 0 becomes M at o; with o < 0 it becomes I.   6. An I column stays I.
 * 7. A D column with o >= 0 becomes D; with o < 0 it vanishes.
 * 8. In front of an M or D column with o >= 0, once an M column has been emitted, o - 1 - o_prev D columns stand for the original
 * bases the variant genome deleted; o_prev is the origin of the nearest kept variant base below v, -1 without one.
 * 9. In front of the first emitted M column and behind the last every I column becomes S and every D column is dropped, gap
 * columns included.  H ops in front of the CIGAR's first column stay as one H at the left end, the others as one at the right end;
 * S likewise inside them, merged with the new S.
 * 10. A record without an M column left is dropped: `unplaced`.   11. pos is the origin of the first M column.
 * 12. Adjacent equal ops merge; nothing else is canonicalised (2D1I3D may stand).  Output ops are M, I, D, S, H.
 * 13. bin = reg2bin(pos, pos + span), span the M and D columns.
 * 14. NM = sub + ins + del against the original genome: sub per M column as pbsim_bam_errors counts it (the prepared bytes; a column
 * with a code outside ACGT on either side is no sub; `=` in SEQ agrees).  A record with l_seq = 0 gets no NM: `no_seq`.
 * 15. Aux fields: NM first; with more than 65535 ops the field is <l_seq>S<span>N and CG:B,I follows NM (SAMv1 4.2.2), so an input
 * placeholder whose lifted CIGAR fits comes back as a real CIGAR; then every field of the input in order except those tagged NM or CG.
 * 16. Records keep their order.   17. The file leaves as BGZF as pbsim_truth_bam_sort writes it: the header in members of its own,
 * the EOF block at the end, through sink->on_bam in offset order.
 * Result.  counts: records, unaligned, unsupported, unplaced, lifted, moved (pos or the resolved CIGAR differs), no_seq,
 * long_cigar_in, long_cigar_out (the last three among the lifted).  totals over the lifted records: cols_in, cols_out (M + I + D
 * of the lifted core), m, ins, del, soft, sub, gap_del (rule 8's columns that stayed), bases_to_ins (M columns with o < 0),
 * dels_vanished (D columns with o < 0), bytes_in, bytes_out.
 * tests/lift_model.py states the rule in plain Python.  The stage holds the inflated stream, the lifted stream, their compressed
 * pieces, the genome at 2 bytes per base, 8 bytes per variant base (origin and the max-scan of its kept values), 4 bytes per
 * lifted op and 181 bytes per record in HBM at once and does not chunk: an allocation that does not fit fails with the bytes it
 * needed.  One wave takes a whole record, 64 columns at a time.  After any failure the context stays usable and the result is zeroed. */
typedef struct pbsim_lift_origin {
  const int32_t *origin;
  int64_t n;
} pbsim_lift_origin;
typedef struct pbsim_lift_sink {
  void *user;
  int (*on_bam)(void *user, const char *bytes, int64_t n, int64_t offset); /* in offset order; may be NULL */
} pbsim_lift_sink;
typedef struct pbsim_lift_result {
  int64_t counts[9];
  int64_t totals[12];
} pbsim_lift_result;
int pbsim_bam_lift(pbsim_ctx *ctx, const pbsim_errors_ref *refs, int n_refs, const pbsim_lift_origin *origins /* one per genome record */,
                   const pbsim_errors_file *file, const pbsim_lift_sink *sink, pbsim_lift_result *result);
/* The report text, no device needed: a "#" line with the names and an "L" line with the values of the result in its order,
 * tab-separated.  Returns the text's length, and writes it (no NUL) where buf holds cap >= that many bytes; -1: bad argument. */
int64_t pbsim_lift_report(const pbsim_lift_result *result, char *buf, int64_t cap);

/* ---- batch primitives (used by the drivers above, bench.py, multi-GPU) ------
 * pbsim_batch_walk     header draw + bucketing + HMM walk of reads
 *                      [first_read, first_read+n_reads) of the current unit,
 *                      speculatively un-truncated; *pass0_bases = their pass-0
 *                      output bases.  truncate_remaining >= 0 (n_reads must be
 *                      1) applies the quota truncation of pbsim.cpp:3795-3800
 *                      with quota-len_total = truncate_remaining.
 * pbsim_batch_finalize places the quota cut given the pass-0 bases simulated
 *                      before this batch and emits FASTQ|SAM + MAF text for the
 *                      final reads into device buffers.
 * pbsim_batch_fetch    copies the text to host memory (either may be NULL). */
int pbsim_batch_walk(pbsim_ctx *ctx, int64_t first_read, int64_t n_reads, int64_t truncate_remaining,
                     int64_t *pass0_bases);
/* Asynchronous halves of pbsim_batch_walk, and batch slots: a context owns
 * pbsim_slot_count() independent batch slots (buffers + HIP stream each);
 * pbsim_select_slot() chooses the one the pbsim_batch_* calls act on.  Beginning
 * batch k+1 on another slot before ending batch k keeps the GPU busy while the
 * longest reads of batch k drain (the drivers above do exactly that). */
int pbsim_slot_count(void);
int pbsim_select_slot(pbsim_ctx *ctx, int slot);
int pbsim_batch_walk_begin(pbsim_ctx *ctx, int64_t first_read, int64_t n_reads, int64_t truncate_remaining);
int pbsim_batch_walk_end(pbsim_ctx *ctx, int64_t *pass0_bases);
int pbsim_batch_finalize(pbsim_ctx *ctx, int64_t len_total_before, pbsim_batch_info *info);
int pbsim_batch_fetch(pbsim_ctx *ctx, char *read_text, char *maf_text);
/* after pbsim_batch_walk_end: the header draws and pass-0 results of the batch's reads, n_reads values each (any pointer may
 * be NULL): raw length drawn (before the clip to the record, pbsim.cpp:3793-3794), length walked, pass-0 bases produced.  What
 * the quota rule (pbsim.cpp:3792-3800) is a function of -- measurement / test hook. */
int pbsim_batch_fetch_lengths(pbsim_ctx *ctx, int32_t *rawlen, int32_t *len, int32_t *out_len_pass0);
/* adds the n_final reads of the finalized batch to the unit's statistics */
int pbsim_batch_account(pbsim_ctx *ctx);
/* resets the per-unit statistics (init_sim_res, pbsim.cpp:1437) */
int pbsim_reset_stats(pbsim_ctx *ctx);
/* quota of the current unit: (long long)(depth*len), pbsim.cpp:705 */
int64_t pbsim_unit_quota(pbsim_ctx *ctx);
/* reads the engine sizes one batch to (from the scratch budget) */
int64_t pbsim_batch_capacity(pbsim_ctx *ctx);
/* scratch pool per slot in bytes (default: PBSIM_SCRATCH_MB env or 8 GiB) */
int pbsim_set_scratch_bytes(pbsim_ctx *ctx, int64_t bytes);
/* A context sizes its pools for the jobs it runs and keeps them (re-allocating tens of GB stalls a job for seconds): one that
 * switches to another KIND of job -- output delivered through a sink, then left in HBM; another pass count -- should give the
 * old pools back first.  Releases the slots' scratch pools, text and compression buffers and the page-locked host blocks a
 * several-rank job compresses into (those go back by themselves only after sixteen jobs that did not use them: giving a block
 * back and page-locking it again cost tens of milliseconds each); nothing may be in flight. */
int pbsim_release_pools(pbsim_ctx *ctx);

/* ---- the whole job on one or several GPUs -------------------------------------
 * main() runs its records one after the other (pbsim.cpp:667-759).  Here ALL records of the genome are made resident in
 * HBM (288 GB holds any genome the reference can read: 3 bytes per base there, 2 here) and ONE pipeline of read batches
 * runs across them: batches of record n+1 start as soon as record n has enough reads in flight, so the tail of a record
 * (its last text emission, its truncated last reads, pbsim.cpp:3795-3800) hides behind the next record's walks.
 *
 * Several GPUs: one context per GPU ("rank"), every rank holds every record (C1: the caller broadcasts them) and runs
 * the same job; a round of the pipeline gives rank r the r-th block of the round's reads.  The ranks only exchange
 * integers through the caller's pbsim_comm: per round ONE all-gather (C3) of the blocks' pass-0 bases and largest raw
 * length (places every rank's quota prefix and tells whether any read of the round can touch the quota) together with the
 * PREVIOUS round's text sizes (every rank learns the byte range of its text inside the record's stream) -- plus a second one for
 * the cut in the one round of a record that reaches the quota; per record three collectives for the
 * statistics (C2: counters, min/max, the two histograms; the order-dependent accuracy sum is folded in read order).  The
 * concatenation of all ranks' text in offset order is byte for byte what one GPU delivers, and so are the statistics.
 *
 * pbsim_comm: blocking collectives over the `world` ranks, called by every rank in the same order (the job is
 * deterministic in the gathered values, so the ranks stay in lockstep by construction).  torch.distributed (backend nccl
 * = RCCL), RCCL itself, MPI or -- for several contexts inside one process -- a host barrier all fit. */
#define PBSIM_OP_SUM 0
#define PBSIM_OP_MIN 1
#define PBSIM_OP_MAX 2
typedef struct pbsim_comm {
  void *user;
  int32_t rank, world;
  /* every rank contributes n values; recv holds world * n, rank-major */
  int (*all_gather_i64)(void *user, const int64_t *send, int64_t n, int64_t *recv);
  /* element-wise reduction over the ranks, in place; op = PBSIM_OP_* */
  int (*all_reduce_i64)(void *user, int64_t *buf, int64_t n, int32_t op);
  /* optional (C1): `bytes` bytes at `ptr` (device memory of this rank's GPU when on_device, else host memory) of rank
   * `root` to every rank.  NULL: the caller has every rank load the records itself. */
  int (*broadcast)(void *user, void *ptr, int64_t bytes, int32_t root, int32_t on_device);
  /* optional: called by a rank whose job failed for a reason the other ranks cannot know yet.  It must make the collectives
   * the other ranks are waiting in (or will enter) return 0, or end their processes.  Failures the library can foresee travel
   * in the status words of its own exchanges and all ranks return PBSIM_FAILED together; for the rest (a HIP error between two
   * exchanges) a communicator without `abort` leaves the other ranks waiting: the caller must then tear the process group
   * down when pbsim_job_run fails on any rank.  NULL is allowed. */
  int (*abort)(void *user);
} pbsim_comm;

/* Receiver of a job's output.  Text arrives as (record, bytes, offset): `offset` is the position of the piece inside the
 * record's read stream resp. MAF stream (what the reference writes into <prefix>_NNNN.fq|sam / .maf after any header the
 * caller puts in front), so every rank can pwrite() its pieces into the final file; on one GPU the offsets simply run up.
 * on_record_done is called on EVERY rank, in record order, with the statistics of the whole record (identical on all
 * ranks) and the total size of its two streams.  Return 0 to abort. */
typedef struct pbsim_record_sink {
  void *user;
  int (*on_read_text)(void *user, int64_t record, const char *text, int64_t bytes, int64_t offset);
  int (*on_maf_text)(void *user, int64_t record, const char *text, int64_t bytes, int64_t offset);
  int (*on_record_done)(void *user, int64_t record, const pbsim_stats *stats, int64_t read_bytes, int64_t maf_bytes);
} pbsim_record_sink;

/* Records are numbered 1.. in the order they are added (genome.num).  The bytes are uploaded and prepared (toupper +
 * homopolymer lengths, pbsim.cpp:1014-1065) asynchronously; pbsim_job_run simulates every record added since the last
 * pbsim_job_clear.  --hp-del-bias != 1 needs no separate census pass here: the census of all resident records is known
 * before the first walk (pbsim.cpp:677-696).  wgs, methods errhmm / qshmm. */
int pbsim_job_add_record(pbsim_ctx *ctx, const uint8_t *seq, int64_t len);
int pbsim_job_add_record_device(pbsim_ctx *ctx, const void *seq_device, int64_t len);
/* The record as it lies in its FASTA file: `lines` = its sequence lines, line feeds included (`bytes` of them; memory of a
 * mapped file will do), `len` = bytes - line feeds.  The copy loop of get_genome_seq (pbsim.cpp:1014-1033: every byte of the
 * lines except the line feeds) runs on the GPU behind the upload; the call fails when the GPU keeps another count than `len`. */
int pbsim_job_add_record_lines(pbsim_ctx *ctx, const uint8_t *lines, int64_t bytes, int64_t len);
/* C1 in one call: rank `root` passes the record (the others may pass NULL); with comm->broadcast the bytes travel GPU to
 * GPU, without it every rank must pass them. */
int pbsim_job_add_record_comm(pbsim_ctx *ctx, const uint8_t *seq, int64_t len, const pbsim_comm *comm, int32_t root);
int64_t pbsim_job_records(pbsim_ctx *ctx);
/* The job's records announced in advance (their number and lengths): pbsim_job_run may then be called BEFORE they have all been
 * added, and pbsim_job_add_record* may be called from another thread while it runs -- in order, each with the announced length.
 * The job begins as soon as record 1 is resident and prepared and begins a later record's first round when that record is, so
 * the upload / broadcast (C1) and preparation (K0) of records 2.. hide behind the rounds in front of them: what a caller that
 * hands over FRESH records waits for is record 1's share, not the genome's (main() reads its records one at a time,
 * pbsim.cpp:666-759; bench.py `value_from_fresh_records`).  With --hp-del-bias != 1 the job waits for every record first (the
 * homopolymer census of all records precedes the first read, pbsim.cpp:677-696).  pbsim_job_feed_abort: the feeding thread gives
 * up (a read error, a failed broadcast); a pbsim_job_run that waits for a record then fails with `why` (it also gives up by
 * itself after 600 s).  pbsim_job_begin / pbsim_job_clear forget the announcement. */
int pbsim_job_expect(pbsim_ctx *ctx, int64_t n_records, const int64_t *lens);
int pbsim_job_feed_abort(pbsim_ctx *ctx, const char *why);
/* drops the records; the next one added is record `first_record` (a genome larger than HBM runs as several jobs whose
 * numbering continues; --hp-del-bias != 1 then needs pbsim_add_hp_census / pbsim_finish_hp_census over ALL records first:
 * pbsim_job_run of a job with first_record > 1 fails without it rather than taking a census per record group).
 * pbsim_job_clear = pbsim_job_begin(ctx, 1). */
int pbsim_job_begin(pbsim_ctx *ctx, int64_t first_record);
int pbsim_job_clear(pbsim_ctx *ctx);
/* By default a record's rounds run back to back (its tail reads and its statistics hide behind the next record's rounds).
 * pbsim_job_set_interleave(ctx, k): the rounds of up to k consecutive records alternate instead, the record that is furthest
 * behind first -- the bytes of k records then arrive side by side, which is what a caller wants who writes a file pair per
 * record onto a file system that takes a few GB/s per file (the CLI sets 4).  Same bytes, same offsets, same statistics. */
int pbsim_job_set_interleave(pbsim_ctx *ctx, int records);
/* comm == NULL: this GPU alone.  sink may be NULL (text stays in HBM: measurements) and so may any of its callbacks. */
int pbsim_job_run(pbsim_ctx *ctx, const pbsim_comm *comm, const pbsim_record_sink *sink);
/* SAM / BAM header of record `record` of the job (pbsim_sam_header / pbsim_bam_header are those of the current unit) */
int64_t pbsim_job_sam_header(pbsim_ctx *ctx, int64_t record, char *buf, int64_t cap);
int64_t pbsim_job_bam_header(pbsim_ctx *ctx, int64_t record, char *buf, int64_t cap);
/* what the last pbsim_job_run did, for bench.py: [0] reads walked (speculation included), [1] reads delivered,
 * [2] rounds, [3] bases delivered (all passes), [4] wall microseconds, [5] microseconds this rank waited in collectives,
 * [6] reference bases consumed and [7] MAF columns written by the delivered reads (roofline accounting) */
int pbsim_job_counters(pbsim_ctx *ctx, int64_t out[8]);
/* where this rank's round loop spent the wall time of the last pbsim_job_run, microseconds: [0] wall; the loop waited
 * [1] for walks (pbsim_batch_walk_end of the round in front), [2] for the cut and the text sizes, [3] for the previous round's
 * bytes to reach host memory (GPU compression + link), [4] in the per-round collectives, [5] accounting statistics,
 * [6] for a record's truncated tail reads at its merge (exposed tail), [7] for the delivery thread at a merge, [8] for a free
 * slot (or for an announced record to arrive, pbsim_job_expect), [9] in the statistics merge (C2), [10] enqueueing rounds, [11] stepping tail reads between rounds; [12] time the
 * delivery thread was busy (compression + copies + sink callbacks; runs beside the loop); [13] top-up rounds, [14] truncated
 * tail reads walked by this rank, [15] rounds kept in flight. */
int pbsim_job_breakdown(pbsim_ctx *ctx, double out[16]);

/* Which exchange of the round sequence this rank's pbsim_job_run is about to enter, readable from inside a pbsim_comm callback
 * (same thread): [0] the kind of exchange -- 6 = "AC", the ONE all-gather of a round that is expected to stay clear of the
 * quota (8 words per rank: [0] pass-0 bases of the block, [1] walk status, [2] largest raw length drawn in the block, [3] status
 * of the text sizes, [4] 1 if [5..7] hold the PREVIOUS round's delivery: compressed read bytes, MAF bytes, status); 1 = "A" of
 * a round that is expected to reach the quota (same 8 words, no delivery part) and 7 = its "BC" ([0] final reads of the block,
 * [1] a truncated read is due, [2] len_total behind the block, [3] status, [4..7] the previous round's delivery); 2 = "B" on its
 * own (a round begun as clear that can touch the quota after all: same words, no delivery part); 3 = the pending round's byte
 * counts on their own (3 words: at a record's merge, at the end of the job); 4 = a record's statistics merge (three
 * collectives); 5 = the agreement on pool size and caps in front of the round loop;
 * [1] record (0-based index in the job), [2] first read of the round (rank r walks [2] + r * [3] ..), [3] reads per rank,
 * [4] ranks, [5] the record's len_total and [7] its next read in front of the round, [6] its quota.  For communicators that
 * model or replay the other ranks (bench.py --replay-ranks measures an N-rank job's per-rank critical path on one GPU). */
int pbsim_job_progress(pbsim_ctx *ctx, int64_t out[8]);

/* The sampling method (pbsim_simulate_sample, pbsim.cpp:1694-1949) on several ranks, for the current record: one context per
 * GPU, every rank has set the same reference and profile.  The copies of one string are a chain, strings are independent, and
 * the test `len_total < quota` at a read's start (pbsim.cpp:1749) is the wgs quota rule's prefix dependence -- a round gives
 * rank r the r-th run of a sweep's strings, three all-gathers of a few integers place the quota prefix, the cut and every
 * rank's byte range.  The sink receives (record, bytes, offset) like a job's (record = the record_index of
 * pbsim_set_reference); on_record_done reports the merged statistics on every rank (pbsim_get_stats too).  The concatenation
 * of all ranks' bytes in offset order is what pbsim_simulate_sample delivers on one GPU. */
int pbsim_simulate_sample_comm(pbsim_ctx *ctx, const pbsim_comm *comm, const pbsim_record_sink *sink);

/* Statistics primitives for callers that shard a unit set over several contexts themselves (trans / templ:
 * pbsim_simulate_units_range per rank): keep the per-task accuracy values while accounting (before simulating), then
 * merge -- afterwards pbsim_get_stats on every rank reports the whole unit set exactly as one GPU would
 * (pbsim.cpp:4082-4105, the order-dependent sum of :4003 included).  pbsim_stats_add_tasks accounts tasks given as plain
 * arrays (device-free; tests of the merge). */
int pbsim_stats_keep_values(pbsim_ctx *ctx, int on);
int pbsim_stats_merge(pbsim_ctx *ctx, const pbsim_comm *comm);
int pbsim_stats_add_tasks(pbsim_ctx *ctx, int64_t first_task, int64_t n, const int32_t *out_len, const int32_t *nsub,
                          const int32_t *nins, const int32_t *ndel, const double *qsum);
/* the ":::: Simulation stats ::::" block of print_simulation_stats (pbsim.cpp:5541-5564); unit = genome.num (wgs).
 * Returns the byte count (excluding the NUL), or the size needed when buf is NULL / too small. */
int64_t pbsim_format_stats(const pbsim_params *p, const pbsim_stats *s, int64_t unit, char *buf, int64_t cap);

/* ---- the command line as a library call ------------------------------------------
 * Everything `pbsim` does for one rank: the reference's options (pbsim.cpp:257-282) and set_sim_param validation
 * (:1451-1688), the stderr report blocks, the <prefix>_NNNN.ref files, the output files.  comm == NULL: this GPU alone.
 * With a communicator every rank calls it with the same argv; rank 0 prints the report and creates the files, every rank
 * writes its own byte ranges of them.  The `pbsim` binary calls this from one host thread per GPU of --devices (host
 * barrier or RCCL communicator); pbsim3_amd/run_multi.py calls it from one process per GPU under torchrun
 * (torch.distributed).  Returns the process exit status (0, or 255 like the reference's exit(-1)). */
int pbsim_cli_main(int argc, char **argv, const pbsim_comm *comm, int device);

/* ---- RCCL communicator of a one-process-per-GPU launch ------------------------------
 * `pbsim --devices` runs its ranks as threads of one process (ncclCommInitAll or a host barrier).  A launcher that starts one
 * PROCESS per GPU (torchrun, mpirun, a shell loop) gets its pbsim_comm here: rank 0 makes the id (ncclGetUniqueId, 128 bytes),
 * the launcher's side channel carries it to the others, every rank enters pbsim_rccl_comm_create with it (ncclCommInitRank:
 * collective over the `world` ranks, one distinct GPU each).  The communicator's callbacks run ncclAllGather (C3),
 * ncclAllReduce (C2) and ncclBroadcast (C1) on a stream of their own, small messages through page-locked staging, every wait
 * polled with a watchdog (PBSIM_COMM_TIMEOUT_S) -- what SURVEY 8(e) names; the reference has no analogue (one process, libc
 * only, pbsim.cpp:4-14).  librccl is opened at run time.
 * pbsim_rccl_unique_id: writes the id (returns its size; with id == NULL or cap too small only the size), 0 on failure.
 * pbsim_rccl_comm_create_file: the same with a file as the side channel -- rank 0 publishes the id at `path` (written whole,
 * then renamed), the others wait for it (PBSIM_RENDEZVOUS_TIMEOUT_S, default 120); rank 0 removes the file once every rank has joined (use a
 * path of the launch's own: a stale file of a crashed launch would be read as this launch's id).
 * pbsim_rccl_comm_info: [0] the ranks RCCL itself counts in the communicator (ncclCommCount), [1] this rank's number there,
 * [2] the device, [3] collectives issued so far.  NULL / PBSIM_FAILED + pbsim_last_error() on failure. */
#define PBSIM_RCCL_ID_BYTES 128
int64_t pbsim_rccl_unique_id(void *id, int64_t cap);
pbsim_comm *pbsim_rccl_comm_create(const void *id, int64_t id_bytes, int32_t rank, int32_t world, int32_t device);
pbsim_comm *pbsim_rccl_comm_create_file(const char *path, int32_t rank, int32_t world, int32_t device);
int pbsim_rccl_comm_info(const pbsim_comm *comm, int64_t out[4]);
void pbsim_rccl_comm_destroy(pbsim_comm *comm);

/* ---- host placement of a rank ----------------------------------------------------------
 * The reference is one thread on one socket; a rank here is a thread that feeds one GPU and receives its output over PCIe.
 * Binds the calling thread -- and the threads and page-locked buffers it creates afterwards -- to the CPUs and the memory of
 * the NUMA node GPU `device` is attached to (sysfs: KFD topology -> PCI address -> numa_node / local_cpulist).  Call it
 * before the first HIP call of the thread's process (pbsim_cli_main does, per rank).  `what` (optional) receives a one-line
 * description, empty when there was nothing to bind to (one node, no topology, PBSIM_NUMA_BIND=0).  Always succeeds. */
int pbsim_bind_host_to_device(int device, char *what, int64_t cap);

/* ---- measurement hooks (bench.py) -------------------------------------------
 * Accumulated HIP-event time of the walk kernel launches since the last reset,
 * measured on the engine's own stream, and the number of launches. */
int pbsim_prof_reset(pbsim_ctx *ctx);
int pbsim_prof_get(pbsim_ctx *ctx, double *walk_ms, int64_t *walk_launches, double *total_ms);
/* pbsim_prof_get counts the walk launches of batches; a launch that carries one truncated tail read (pbsim.cpp:3795-3800:
 * the latency of a single lane, no bytes to speak of) is counted here instead */
int pbsim_prof_tail(pbsim_ctx *ctx, double *tail_ms, int64_t *tail_launches);
/* milliseconds since the reset during which at least one walk kernel ran (the launches of different slots overlap) */
int pbsim_prof_walk_busy(pbsim_ctx *ctx, double *busy_ms);
/* launches of a wave walker (one wave per task: k_walk_errhmm_coop / k_walk_qshmm_coop) since the last reset (or creation) */
int64_t pbsim_prof_wave_launches(pbsim_ctx *ctx);
/* The scratch rows of a task (two MAF rows, a quality row for the quality-score methods) are laid out for factor x length + 64
 * columns.  2 is the reference's own bound (its buffers are 2 * len_max + 1, pbsim.cpp:5488); a context starts there, keeps the
 * largest need its walks have reported and lays the next batches out with a little more -- a batch in which a read runs out of
 * row all the same is walked again at 2 inside pbsim_batch_walk_end.  [0] the factor the next batches get, [1] the largest
 * (columns - 64) / length seen, [2] batches walked twice.  PBSIM_SCRATCH_FACTOR fixes the factor. */
int pbsim_scratch_state(pbsim_ctx *ctx, double out[3]);
/* the two kernels next in line, timed with HIP events on the streams they run on, since the last reset:
 * [0] ms, [1] launches, [2] bytes read (scratch rows), [3] bytes written (text) of the text emission (k_text_*);
 * [4] ms, [5] launches, [6] text bytes in, [7] member bytes out of k_deflate_chunks */
int pbsim_prof_secondary(pbsim_ctx *ctx, double out[8]);
/* raw HIP stream handle (hipStream_t) of the engine, for external event timing */
void *pbsim_stream(pbsim_ctx *ctx);
/* hipDeviceSynchronize on the context's GPU: the bracket of a timed region for a host that holds no HIP runtime handle of its
 * own (bench.py --no-torch: a process with the system runtime only, which rocprofv3 traces without changing how copies run) */
int pbsim_device_synchronize(pbsim_ctx *ctx);

/* ---- known-answer hooks (tests) ---------------------------------------------
 * Philox4x32-10 block as the kernels compute it, on the host build of the same
 * header (no GPU needed). */
void pbsim_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* sha256-able dumps of the host-built tables (Q13 fixtures): returns bytes
 * written, or the size needed when buf is NULL. which: 0 prob2len (int32
 * [len_rand_value+1]), 1 prob2acc (uint8 [acc_rand_value+1]), 2 class tables.
 * Test infrastructure as well, read back from the device behind the context's stream: what the preparation kernels
 * (k_hp_breaks / k_hp_carry / k_hp_final) made of the context's CURRENT unit -- 3 the prepared sequence bytes, ref_len of
 * them (trans / templ: the units in load order, each followed by one line feed); 4 the hp bytes, ref_len of them -- refused
 * (-1, pbsim_last_error) when bit 7 of the sequence bytes carries hp == 11 instead (--hp-del-bias 1, no byte >= 0x80), as
 * the array is not written then; 5 the twelve int64 census counts of the most recent preparation alone (pbsim_set_reference*,
 * an adopted prefetch, pbsim_set_transcripts / pbsim_set_templates / their file loaders); 6 the census accumulated by
 * pbsim_add_hp_census so far.  3, 4 and 5 are valid only directly behind one of the preparations listed: pbsim_add_hp_census
 * prepares its record in the same buffers (and rewrites the bit-7 state) without making it the current unit, so a dump taken
 * between it and the next pbsim_set_reference* returns that record's bytes, cut to the old ref_len, beside the old census.
 * Returns -1 for an unknown `which` or when there is nothing to dump. */
int64_t pbsim_dump_table(pbsim_ctx *ctx, int which, void *buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PBSIM3_AMD_H */
