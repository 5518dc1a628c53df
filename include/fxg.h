/*
 * fxg.h -- C-ABI of the MI355X (gfx950) FASTQ preprocessing engine.
 *
 * This is the drop-in boundary for the fastx_toolkit hot path: the per-read loop bodies of
 *   fastq_quality_trimmer     (reference src/fastq_quality_trimmer/fastq_quality_trimmer.c:91-103)
 *   fastq_quality_filter      (src/fastq_quality_filter/fastq_quality_filter.c:78-129,150-156)
 *   fastx_clipper             (src/fastx_clipper/fastx_clipper.cpp:159-241,257-320 +
 *                              src/libfastx/sequence_alignment.cpp:113-129,340-428,496-650)
 *   fastx_trimmer             (src/fastx_trimmer/fastx_trimmer.c:120-148)
 *   fastx_reverse_complement  (src/fastx_reverse_complement/fastx_reverse_complement.c:43-104)
 * run as batched HIP kernels over a Structure-of-Arrays batch instead of once per
 * fastx_read_next_record() (src/libfastx/fastx.h:120-142).  The reference has no FFI of its own; the
 * host-side C layer that keeps the libfastx record API and the tools' command lines on top of these
 * entry points lives in fastx_toolkit_amd/host/ (see INTEGRATION.md).  Further down: the neighbouring per-read
 * tools (fastq_masker, fastx_artifacts_filter, fastq_to_fasta), fastx_quality_stats as a reduction, the
 * clipper's read-to-read history, and FASTQ text parsed/formatted on the device.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes only.  Every function returns 0 on success or a negative
 *    FXG_E_* code; fxg_last_error(ctx) describes the most recent failure on that context.
 *  - All fxg_batch / fxg_out pointers are DEVICE pointers (hipMalloc'ed by the caller or through
 *    fxg_malloc_device).  bases/qual/res/out_bases/out_qual must be 16-byte aligned.
 *  - Work is enqueued on the context's HIP stream and is asynchronous; fxg_sync() waits for it.  The
 *    context owns a stream of its own (non-blocking: NOT ordered with the legacy default stream);
 *    fxg_set_stream() makes it use the caller's, which is how to order it with other device work.
 *  - A context is not thread-safe: one thread at a time per context; contexts are independent.
 *  - There is no CPU fallback anywhere: without a usable HIP device fxg_ctx_create() fails.
 */
#ifndef FXG_H
#define FXG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FXG_ABI_VERSION 6

/* ---- error codes ---- */
#define FXG_OK            0
#define FXG_E_INVALID    -1   /* bad argument / unsupported stage combination */
#define FXG_E_HIP        -2   /* a HIP runtime call failed */
#define FXG_E_NOMEM      -3
#define FXG_E_DEVICE     -4   /* device-side failure flag (scan time-out, invalid nucleotide, ...) */

/* ---- pipeline stages.  Supported chains: [CLIP][QTRIM][QFILTER], [REVCOMP][FTRIM|FTRIM_END], [MASK], [ARTIFACTS], [NFILTER] ---- */
#define FXG_STAGE_CLIP      0x01u  /* fastx_clipper            */
#define FXG_STAGE_QTRIM     0x02u  /* fastq_quality_trimmer    */
#define FXG_STAGE_QFILTER   0x04u  /* fastq_quality_filter     */
#define FXG_STAGE_REVCOMP   0x08u  /* fastx_reverse_complement */
#define FXG_STAGE_FTRIM     0x10u  /* fastx_trimmer -f/-l      */
#define FXG_STAGE_FTRIM_END 0x20u  /* fastx_trimmer -t/-m      */
#define FXG_STAGE_MASK      0x40u  /* fastq_masker             (reference src/fastq_masker/fastq_masker.c:92-108) */
#define FXG_STAGE_ARTIFACTS 0x80u  /* fastx_artifacts_filter   (src/fastx_artifacts_filter/fastx_artifacts_filter.c:56-112) */
#define FXG_STAGE_NFILTER   0x100u /* fastq_to_fasta's N-discard (src/fastq_to_fasta/fastq_to_fasta.c:79-82) */

/* fastx_clipper switches (fastx_clipper.cpp:90-146) */
#define FXG_CLIP_DISCARD_NON_CLIPPED 0x1u /* -c */
#define FXG_CLIP_DISCARD_CLIPPED     0x2u /* -C */
#define FXG_CLIP_KEEP_N              0x4u /* -n */
#define FXG_CLIP_ADAPTER_ONLY        0x8u /* -k */

#define FXG_MAX_ADAPTER 99           /* fastx_clipper.cpp:40 MAX_ADAPTER_LEN 100 incl. NUL */
#define FXG_MAX_READ_LEN 65535u      /* device limit; the reference reader stops at 24999 (fastx.h:33) */

/* Per-read result word written to fxg_out.res[r]:
 *   bits  0..15  new length (bases kept; for dropped reads the length at the point of the drop)
 *   bit   16     keep
 *   bits 17..20  drop reason (FXG_R_*)
 *   bit   21     adapter found and clipped (clipper's i > 0)
 *   bit   22     adapter found at index 0 ("adapter-only", fastx_clipper.cpp:289-295; counted even when -k keeps it) */
#define FXG_RES_LEN(w)     ((uint32_t)(w) & 0xFFFFu)
#define FXG_RES_KEEP(w)    (((uint32_t)(w) >> 16) & 1u)
#define FXG_RES_REASON(w)  (((uint32_t)(w) >> 17) & 0xFu)
#define FXG_RES_CLIPPED(w) (((uint32_t)(w) >> 21) & 1u)
#define FXG_RES_ADAPTER_ONLY(w) (((uint32_t)(w) >> 22) & 1u)

enum fxg_reason {
    FXG_R_KEPT = 0,
    FXG_R_CLIP_TOO_SHORT = 1,     /* fastx_clipper.cpp:297-300 */
    FXG_R_CLIP_ADAPTER_ONLY = 2,  /* :289-295 */
    FXG_R_CLIP_NO_ADAPTER = 3,    /* :302-305 (-c) */
    FXG_R_CLIP_ADAPTER_FOUND = 4, /* :307-310 (-C) */
    FXG_R_CLIP_N = 5,             /* :312-315 */
    FXG_R_QTRIM = 6,              /* fastq_quality_trimmer.c:101 */
    FXG_R_QFILTER = 7,            /* fastq_quality_filter.c:155 */
    FXG_R_FTRIM = 8,              /* fastx_trimmer.c:127,137,140 */
    FXG_R_CLIP_K_MODE = 9,        /* fastx_clipper.cpp:317 (-k: only adapter-only reads are written) */
    FXG_R_ARTIFACT = 10,          /* fastx_artifacts_filter.c:101-109 */
    FXG_R_HAS_N = 11              /* fastq_to_fasta.c:80-81 */
};

/* slots of the u64 counter block (feeds the tools' -v reports, a12) */
enum fxg_counter {
    FXG_C_INPUT = 0,
    FXG_C_KEPT = 1,
    FXG_C_KEPT_BASES = 2,
    FXG_C_CLIP_TOO_SHORT = 3,
    FXG_C_CLIP_ADAPTER_ONLY = 4,
    FXG_C_CLIP_NO_ADAPTER = 5,
    FXG_C_CLIP_ADAPTER_FOUND = 6,
    FXG_C_CLIP_N = 7,
    FXG_C_QTRIM_DROPPED = 8,
    FXG_C_QFILTER_DROPPED = 9,
    FXG_C_FTRIM_DROPPED = 10,
    FXG_C_CLIP_OUT = 11,          /* reads that survive the clip stage */
    FXG_C_QTRIM_OUT = 12,         /* reads that survive the quality-trim stage */
    FXG_C_MASKED_READS = 13,      /* fastq_masker.c:100-101 */
    FXG_C_MASKED_NT = 14,         /* fastq_masker.c:97 */
    FXG_C_ERRORS = 15,            /* device error bits, see FXG_DEV_ERR_* */
    FXG_C_ARTIFACT_DROPPED = 16,
    FXG_NCOUNTERS = 24
};
#define FXG_DEV_ERR_SCAN_TIMEOUT 0x1u
#define FXG_DEV_ERR_BAD_BASE     0x2u  /* fastx_reverse_complement.c:67-68 "Invalid nucleotide value" */

/* Tool parameters, one block for the whole chain (flag meaning = the reference's getopt handlers). */
typedef struct fxg_params {
    uint32_t stages;              /* FXG_STAGE_* mask */
    int32_t  qoffset;             /* -Q, fastx_args.c:43 (default 33) */
    int32_t  qt_threshold;        /* fastq_quality_trimmer -t (strtol; may be negative) */
    int32_t  qt_min_len;          /* fastq_quality_trimmer -l */
    int32_t  qf_min_quality;      /* fastq_quality_filter -q */
    int32_t  qf_min_percent;      /* fastq_quality_filter -p, 0 = flag omitted (quirk F2) */
    char     adapter[100];        /* fastx_clipper -a, NUL terminated */
    uint32_t clip_min_len;        /* fastx_clipper -l (default 5) */
    int32_t  clip_keep_delta;     /* fastx_clipper -d N, already += strlen(adapter) when N>0 (:153-154) */
    int32_t  clip_min_adapter_len;/* fastx_clipper -M */
    uint32_t clip_flags;          /* FXG_CLIP_* */
    int32_t  ft_first;            /* fastx_trimmer -f (1-based, default 1) */
    int32_t  ft_last;             /* fastx_trimmer -l (0 = to the end) */
    uint32_t ft_trim_end;         /* fastx_trimmer -t */
    uint32_t ft_min_len;          /* fastx_trimmer -m */
    int32_t  mask_min_quality;    /* fastq_masker -q (default 10) */
    uint32_t mask_char;           /* fastq_masker -r (default 'N') */
    uint32_t nf_keep_n;           /* fastq_to_fasta -n: keep reads with N (the stage then only checks the alphabet) */
} fxg_params;

/* Input batch (replaces the one-record FASTX struct, fastx.h:62-117): row r of bases/qual starts at
 * r*stride; its length is len[r], or fixed_len when len == NULL.  qual == NULL means FASTA input
 * (only CLIP / REVCOMP / FTRIM* make sense then).  Quality bytes are the raw ASCII characters; the
 * -Q offset is folded into the thresholds on the host side of the launch. */
typedef struct fxg_batch {
    const uint8_t  *bases;
    const uint8_t  *qual;
    const uint16_t *len;
    uint32_t        fixed_len;
    uint32_t        stride;
    uint64_t        n;
} fxg_batch;

/* Output.  res is mandatory.  If out_bases != NULL the kept reads are stream-compacted in input order:
 * their (transformed) bases and qualities are concatenated without gaps into out_bases/out_qual
 * (same offsets in both), which is what fastx_write_record (fastx.c:440-473) would print line by
 * line.  out_len / kept_index / out_off (all optional) describe kept read k = 0..kept-1.
 * counters (optional, device u64[FXG_NCOUNTERS]) is overwritten by each run. */
typedef struct fxg_out {
    uint32_t *res;
    uint8_t  *out_bases;
    uint8_t  *out_qual;
    uint16_t *out_len;
    uint32_t *kept_index;
    uint64_t *out_off;
    uint64_t *counters;
} fxg_out;

/* Memory contract: the bytes a kernel may touch through each pointer, counted from the pointer.  "Granule": the 16-byte aligned block that holds
 * an array's last byte.  An input may be read up to the end of that granule (aligned 16-byte loads; a granule never crosses a page), and what is
 * read there never reaches a result.  Nothing before a pointer is read, and nothing outside an output's range is written.
 *   fxg_batch.bases, .qual   read   n * stride bytes (+ granule)      every row whole, also past len[r]; qual may be NULL.  A kernel may read
 *                                                                       less: the rows kernels fetch only the 16-byte chunks of .bases that
 *                                                                       hold kept prefixes (fxg_rows.h, FXG_ROWS_SPARSE_BASES)
 *   fxg_batch.len            read   n uint16 (+ granule)               NULL: every read is fixed_len long
 *   fxg_out.res              write  n uint32
 *   fxg_out.out_bases, .out_qual   write  n * stride bytes            the capacity; the kept reads fill counters[FXG_C_KEPT_BASES] <= n * stride of it
 *   fxg_out.out_len          write  n uint16      kept_index: n uint32      out_off: n uint64      (entries 0 .. kept - 1 hold values)
 *   fxg_out.counters         write  FXG_NCOUNTERS uint64
 *   fxg_run_quality_stats    d_hist: read and written, hist_cols * FXG_QS_CLASSES * FXG_QS_BINS uint64; the batch as fxg_batch above
 *   text path (below)        d_text: read text_len + 16 bytes (the 16 are slack: their values never matter); d_line: 2 * cap_lines uint32;
 *                            d_len, d_flags: cap_lines / lines_per_record entries; packed rows: records * stride rounded up to 16 bytes (whole
 *                            16-byte chunks are written); d_out: text_len + records + 16 bytes; d_res, d_pk_*: records entries / the packed stream.
 *   barcode split (below)    d_text: read as for the text path; d_line: the line starts ls[0 .. lines_per_record * records] (first half only);
 *                            d_rec_bin: write records uint16; d_out: write exactly ls[lines_per_record * records] - ls[0] bytes (the records
 *                            themselves), never a byte past them.
 *   fasta reflow (below)     d_text: read as for the text path (text_len + 16 bytes); d_line: 2 * cap_lines uint32 as for the text path, of which
 *                            the line starts ls[0 .. lines] are read back; d_out: write exactly info->out_bytes bytes, never a byte past them,
 *                            and none at all when the request is refused.
 *   fasta uncollapse (below) d_text: the bytes of the records' lines (text_len + 16 readable, as for the text path); d_line: 2 * cap_lines uint32,
 *                            read at entries 0 .. 2 * records - 1 of either half; d_len: read records uint16; d_out: write exactly
 *                            info->out_bytes bytes, never a byte past them, and none at all when the request is refused.
 *   bases change (below)     d_text: read as for the text path (text_len + 16 bytes), written only inside the records' bases lines, from a
 *                            line's start to its chomped end; d_line: 2 * cap_lines uint32, read at entries lines_per_record * r + 1 of
 *                            either half.
 *   collapse rows (below)    d_bases: read only inside [d_off[k], d_off[k] + d_len[k]) of records k = 0 .. records - 1, rounded out to 16-byte
 *                            granules, and never past the granule that holds the last record's last byte; d_off, d_len, d_kept_index: read at
 *                            entries 0 .. records - 1; d_text: the id lines of the records d_kept_index names; d_line: 2 * cap_lines uint32,
 *                            read at entries 2 * d_kept_index[k] of either half.
 * tests/test_emu_bounds.py runs the kernels' bodies with every array against a guard page at these ends; tests/test_gpu_bounds.py surrounds every
 * array with poison (inputs) and canaries (outputs) on the device. */

typedef struct fxg_ctx fxg_ctx;

/* ---- context ---- */
int  fxg_abi_version(void);
int  fxg_ctx_create(int device_id, fxg_ctx **out);
void fxg_ctx_destroy(fxg_ctx *ctx);
const char *fxg_last_error(const fxg_ctx *ctx);
int  fxg_set_stream(fxg_ctx *ctx, void *hip_stream);   /* NULL = the context's own stream */
int  fxg_sync(fxg_ctx *ctx);
int  fxg_device_info(fxg_ctx *ctx, int *compute_units, size_t *total_mem, char *name, size_t name_cap);

/* ---- memory helpers so that a C host needs no HIP headers ---- */
int  fxg_malloc_device(fxg_ctx *ctx, size_t bytes, void **dptr);
int  fxg_free_device(fxg_ctx *ctx, void *dptr);
int  fxg_malloc_host(fxg_ctx *ctx, size_t bytes, void **hptr);     /* pinned */
int  fxg_free_host(fxg_ctx *ctx, void *hptr);
int  fxg_memcpy_h2d(fxg_ctx *ctx, void *dst, const void *src, size_t bytes);   /* async on the ctx stream */
int  fxg_memcpy_d2h(fxg_ctx *ctx, void *dst, const void *src, size_t bytes);   /* async on the ctx stream */
int  fxg_memset_device(fxg_ctx *ctx, void *dst, int value, size_t bytes);

/* ---- timing on the stream the kernels run on (HIP events) ---- */
int  fxg_timer_start(fxg_ctx *ctx);
int  fxg_timer_stop(fxg_ctx *ctx, float *elapsed_ms);               /* synchronises on the stop event */

/* ---- the hot path ---- */
/* General entry: runs the chain described by p->stages over the batch. */
int  fxg_run_pipeline(fxg_ctx *ctx, const fxg_batch *in, const fxg_params *p, const fxg_out *out);

/* Per-tool entry points (thin wrappers that fill fxg_params and call fxg_run_pipeline). */
int  fxg_run_qtrim_qfilter(fxg_ctx *ctx, const fxg_batch *in, int qoffset,
                           int use_trim, int trim_threshold, int trim_min_len,
                           int use_filter, int filter_min_quality, int filter_min_percent,
                           const fxg_out *out);
int  fxg_run_clip(fxg_ctx *ctx, const fxg_batch *in, const char *adapter, uint32_t min_len,
                  int keep_delta, int min_adapter_len, uint32_t clip_flags, const fxg_out *out);
int  fxg_run_revcomp_trim(fxg_ctx *ctx, const fxg_batch *in, int reverse_complement,
                          int first_base, int last_base, const fxg_out *out);

/* Copies the counter block to the host after synchronising; returns FXG_E_DEVICE if the kernels
 * raised an error bit (counters[FXG_C_ERRORS]). */
int  fxg_read_counters(fxg_ctx *ctx, const uint64_t *d_counters, uint64_t host_counters[FXG_NCOUNTERS]);
/* A compacting launch whose bounded waits ran out (FXG_DEV_ERR_SCAN_TIMEOUT: the launch's workgroups were not being scheduled -- a GPU shared with
 * another process) is not an error any more: fxg_read_counters does the launch again in a form that cannot wait on another workgroup (decisions, block
 * sums, scan, gather: csrc/fxg_fallback.h) and returns the counters of that.  This is how many launches of the context went that way; a host that
 * wants to tell its user compares it before and after.  (The caller's batch and output arrays must still be what the launch was given.) */
int  fxg_scan_recoveries(const fxg_ctx *ctx);

/* Deterministic synthetic reads generated straight into device memory. */
int  fxg_synth_generate(fxg_ctx *ctx, uint64_t seed, uint64_t first_read, uint64_t n, uint32_t read_len,
                        int with_adapter, uint8_t *d_bases, uint8_t *d_qual, uint32_t stride);

/* ---- FASTA / FASTQ text on the device: index + check + pack (replaces fastx.c:314-404) and format
 * (replaces fastx.c:440-473).  Handled on the device: four-line FASTQ and two-line FASTA records (fastx.c:86-116), lines cut at
 * their first CR or LF (chomp.c:36-41, so CRLF in gives LF out), ASCII and -- per record -- numeric quality lines
 * (fastx.c:137-167, :382-390), upper-case ACGTN bases, qualities within -15..93 after -Q, collapsed FASTA ids for the -v
 * tallies (fastx.c:475-495).  Malformed input is only detected (info->irregular != 0); the caller then parses that block
 * with the host reader, which owns the reference's error messages.  All calls synchronise. ---- */
typedef struct fxg_text_info {
    uint64_t lines;          /* complete lines in the block */
    uint64_t records;        /* complete records = lines / lines_per_record */
    uint64_t consumed;       /* bytes they occupy; the next block starts there */
    uint32_t max_len, min_len;
    uint32_t irregular;      /* 0 = regular; FXG_TEXT_IRR_* bits otherwise */
    uint32_t first_bad;      /* smallest record index flagged by the index pass (0xFFFFFFFF if none) */
    uint32_t numeric_records;/* records whose quality line holds numbers */
    uint32_t has_cr;         /* the block contains CR bytes (lines were cut at them) */
} fxg_text_info;
#define FXG_TEXT_IRR_CR        0x01u   /* (not raised any more: CR is chomped on the device) */
#define FXG_TEXT_IRR_PREFIX    0x02u
#define FXG_TEXT_IRR_SEQLEN    0x04u
#define FXG_TEXT_IRR_QUALLEN   0x08u
#define FXG_TEXT_IRR_BASE      0x10u
#define FXG_TEXT_IRR_QUAL      0x20u
#define FXG_TEXT_IRR_TAIL      0x40u
#define FXG_TEXT_IRR_NUL       0x80u   /* a NUL byte: the reference's lines are C strings, the host reader cuts them there */
#define FXG_REC_NUMERIC_QUAL   0x01u   /* d_flags[record]: numeric quality line */

/* d_text: device, readable up to text_len + 16 bytes, every line '\n'-terminated (the caller appends one at end of input).
 * lines_per_record: 4 = FASTQ, 2 = FASTA.  d_line: device u32[2 * cap_lines] -- line starts in the first half, line ends
 * (after chomp) in the second; cap_lines >= lines_per_record * records + 1.  d_len: device u16[cap_lines / lines_per_record];
 * d_flags: device u8[cap_lines / lines_per_record]. */
int  fxg_fastq_index(fxg_ctx *ctx, const uint8_t *d_text, uint64_t text_len, int at_eof, int lines_per_record, uint32_t *d_line,
                     uint64_t cap_lines, uint16_t *d_len, uint8_t *d_flags, fxg_text_info *info);
/* rows: device arrays of at least records * stride rounded up to 16 bytes; qualities become Phred+33 codes (d_qual NULL for FASTA).
 * The line arrays and flags are the caller's: they may come from fxg_fastq_index on another context of the same device, and the pack may be the
 * first call a context ever sees (it makes what device state it needs itself). */
int  fxg_fastq_pack(fxg_ctx *ctx, const uint8_t *d_text, uint64_t text_len, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines,
                    const uint8_t *d_flags, uint64_t records, uint32_t stride, int qoffset, uint8_t *d_bases, uint8_t *d_qual, uint32_t *irregular);
/* Writes "@name\nSEQ\n+name2\nQUAL\n" (or ">name\nSEQ\n": FASTA input, or out_fasta) for every kept record (res keep bit) in input
 * order.  Forward outputs are the slice [fwd_start, fwd_start + len) of the input lines; pass the engine's packed arrays + out_off
 * for reverse-complemented / masked output (reverse != 0 when they are reversed).  d_rows_qual / stride: the batch's quality rows
 * (numeric quality lines are printed from them).  d_out needs text_len + records + 16 bytes (an empty third line still gets its '+').
 * The qualities of record r that a numeric line is sized and printed from are those of its input positions [fwd_start, fwd_start + len)
 * for forward output, [rl - fwd_start - len, rl - fwd_start) (rl: the read's length) for reversed packed output, and [0, len) for packed
 * output that is not reversed -- the masker's, which keeps every read whole.  No stage chain trims and then masks, so packed arrays with
 * reverse == 0 and fwd_start != 0 are refused (FXG_E_INVALID with a message). */
int  fxg_fastq_format(fxg_ctx *ctx, const uint8_t *d_text, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines, const uint8_t *d_flags,
                      uint64_t records, const uint32_t *d_res, uint32_t fwd_start, int reverse, const uint8_t *d_pk_bases, const uint8_t *d_pk_qual,
                      const uint64_t *d_pk_off, const uint8_t *d_rows_qual, uint32_t stride, int qoffset, int out_fasta, uint8_t *d_out,
                      uint64_t *out_bytes);
/* fxg_fastq_format with output modes: the ids and the quality encoding of the records written (fastq_to_fasta -r, fastx_renamer,
 * fastq_quality_converter).  All modes zero: exactly fxg_fastq_format.  d_res may be NULL when opts->d_len is given: a block that went through
 * no stage, every record kept whole (then no packed arrays and fwd_start 0).  The block's size is known before anything is written: more than
 * opts->out_cap bytes is refused (FXG_E_INVALID, fxg_last_error says how many) with d_out untouched; unknown mode values are refused too. */
#define FXG_ID_INPUT     0u   /* the input's own name lines */
#define FXG_ID_ORDINAL   1u   /* the record's running number (fastq_to_fasta.c -r, fastx_renamer.c -n COUNT) */
#define FXG_ID_SEQUENCE  2u   /* the record's OUTPUT bases (fastx_renamer.c -n SEQ) */
#define FXG_QUAL_AS_INPUT 0u  /* every record in the encoding it came in */
#define FXG_QUAL_ASCII    1u  /* characters, code + Q (fastx.c:406-419) */
#define FXG_QUAL_NUMERIC  2u  /* numbers joined by blanks (fastx.c:421-438) */
#define FXG_OUT_CAP_UNCHECKED (~0ull)   /* out_cap: the caller vouches for d_out (fxg_fastq_format's documented capacity) */
typedef struct {
    uint32_t id_mode;      /* FXG_ID_INPUT (0) | FXG_ID_ORDINAL | FXG_ID_SEQUENCE */
    uint32_t id_both;      /* FASTQ out: the '+' line carries the new id too (fastx_renamer.c:93,97); 0: name2 as in the input */
    uint64_t ordinal_base; /* kept record of rank k (0-based, in this block) is named base + k + 1, as "%llu" */
    uint32_t qual_mode;    /* FXG_QUAL_AS_INPUT (0) | FXG_QUAL_ASCII | FXG_QUAL_NUMERIC */
    uint64_t out_cap;      /* bytes d_out can take */
    const uint16_t *d_len; /* used when d_res == NULL: every record is kept whole, its length from fxg_fastq_index */
} fxg_format_opts;
int  fxg_fastq_format_opts(fxg_ctx *ctx, const uint8_t *d_text, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines, const uint8_t *d_flags,
                           uint64_t records, const uint32_t *d_res, uint32_t fwd_start, int reverse, const uint8_t *d_pk_bases, const uint8_t *d_pk_qual,
                           const uint64_t *d_pk_off, const uint8_t *d_rows_qual, uint32_t stride, int qoffset, int out_fasta, uint8_t *d_out,
                           uint64_t *out_bytes, const fxg_format_opts *opts);
/* FASTA records stand for `count` reads when their identifier is "id-count" (fastx.c:475-495).  weighted[0..6] = read-count
 * weighted tallies over the block: input, kept, clip too-short, adapter-only, no-adapter, adapter-found, has-N.
 * Precondition: the context has run fxg_fastq_index, fxg_fastq_pack, fxg_fastq_format[_opts] or fxg_fasta_reflow before.  On a context that has not,
 * a call with records > 0 is refused: FXG_E_INVALID, "fxg_fasta_weights: index the block first", weighted[] all zero, nothing launched. */
int  fxg_fasta_weights(fxg_ctx *ctx, const uint8_t *d_text, const uint32_t *d_line, uint64_t cap_lines, uint64_t records, const uint32_t *d_res,
                       uint64_t weighted[8]);
/* fastx_barcode_splitter (reference scripts/fastx_barcode_splitter.pl): a stable partition of a block's records into `bins` bins by their
 * barcode.  The table holds `entries` entries in the script's order (a barcode, then its --partial shortenings): entry e's bases are
 * bases[e * FXG_MAX_BARCODE ...], upper-case A/C/G/T, len[e] <= barcode_len of them, and it names bin[e] < bins.  Bin bins - 1 is
 * `unmatched` (an entry may name it too).  A record's window is the first (eol == 0) or last min(barcode_len, bases) bytes of its bases line
 * without the '\n'; an entry's mismatches are the window's length minus the bytes equal to the entry's minus the NUL bytes past the entry's
 * end, plus barcode_len - len[e].  The record goes to the first entry with the fewest mismatches, if those are below barcode_len and at most
 * `mismatches`; to bin bins - 1 otherwise.  Every byte of the window is compared as it is (CR, NUL, lower case). */
#define FXG_MAX_BARCODE 64
#define FXG_MAX_BARCODE_BINS 4096
typedef struct fxg_barcode_set {
    const uint8_t  *bases;        /* host, entries * FXG_MAX_BARCODE bytes */
    const uint32_t *len;          /* host, entries */
    const uint32_t *bin;          /* host, entries */
    uint32_t entries;             /* any number, 0 included (then every record is unmatched) */
    uint32_t barcode_len;         /* 1 .. FXG_MAX_BARCODE (0 only without entries) */
    uint32_t mismatches;
    uint32_t eol;                 /* 0: --bol, 1: --eol */
    uint32_t bins;                /* 1 .. FXG_MAX_BARCODE_BINS, unmatched included */
} fxg_barcode_set;
/* Encodes the table and uploads it; it serves every fxg_barcode_split on this context until the next prepare. */
int  fxg_barcode_prepare(fxg_ctx *ctx, const fxg_barcode_set *set);
/* Splits the `records` complete records of a block indexed by fxg_fastq_index (d_line, cap_lines as given to it; d_text 4-byte aligned).
 * d_out receives bin 0's records, then bin 1's, ..., each bin's in input order and as their input bytes; bin_bytes[b] / bin_records[b]
 * (host, bins entries each) say how many.  d_rec_bin (optional): the bin of every record.  Synchronises. */
int  fxg_barcode_split(fxg_ctx *ctx, const uint8_t *d_text, uint64_t text_len, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines,
                       uint64_t records, uint16_t *d_rec_bin, uint8_t *d_out, uint64_t *bin_bytes, uint64_t *bin_records);
/* fasta_formatter (reference src/fasta_formatter/fasta_formatter.cpp:136-201, sequence_writers.h:31-109): multi-line FASTA reflowed on the
 * device.  The block is split at '\n'; only complete lines count.  Lines of length 0 are skipped, a line whose first byte is '>' starts a
 * record and is its id line H, every other line is appended to the open record's bases B as its bytes are (CR, NUL, lower case and blanks
 * are kept).  A record goes out as "H\n B\n" (width 0), as "H\n" and B in lines of `width` bytes (a shorter last line, never an empty one),
 * or as "H[1:]\t B\n" (tabular, which wins over width); a record without bases as "H\n" / "H[1:]\n" with keep_empty, not at all without.
 * Blocks chain through one number: open_bases_in is how many bases of the record open at the block's start are already written (0: no record
 * is open), info->open_bases is that number for the next block, which starts at info->consumed.  What closes a record -- the '\n' after
 * its last bases if one is due, or the id line of a record without bases -- is written when the next header line or the end of input
 * (at_eof) comes, so a call with text_len == 0, at_eof != 0 and open_bases_in > 0 writes that newline.  consumed ends after the last complete
 * line, except that, not at the end of input, the block's last header line is not consumed while no non-empty sequence line follows it: it
 * closes the record before it in this block and is read again with the next one.  (So consumed == 0 before the end of input means: the block
 * must grow.)  A non-empty sequence line with no header before it in the block while open_bases_in == 0 is refused; the host keeps such
 * input (sequence lines before the first header) away from the device.  The block's output size is known before anything is written: more
 * than out_cap bytes is refused (FXG_E_INVALID, the message says how many) with d_out untouched; 2 * text_len + 2 always suffices (width 1
 * doubles the bases).  d_text, text_len, d_line, cap_lines: as for the text path, cap_lines >= lines + 1 (refused otherwise, the message
 * says how many), every offset inside a block is 32-bit (text_len <= 0xFFFFFFF0), output offsets are 64-bit.  Synchronises.  With profiling
 * on, a call records three intervals: classify + segmented scan, sizes + scans, copy. */
typedef struct fxg_reflow_opts {
    uint32_t width;        /* -w: 0 = one line per record */
    uint32_t tabular;      /* -t */
    uint32_t keep_empty;   /* -e */
    uint64_t out_cap;      /* bytes d_out can take */
} fxg_reflow_opts;
typedef struct fxg_reflow_info {
    uint64_t lines;        /* complete lines in the block */
    uint64_t headers;      /* of which header lines */
    uint64_t consumed;     /* the next block starts there */
    uint64_t out_bytes;    /* written to d_out */
    uint64_t open_bases;   /* open_bases_in of the next block */
} fxg_reflow_info;
int  fxg_fasta_reflow(fxg_ctx *ctx, const uint8_t *d_text, uint64_t text_len, int at_eof, uint64_t open_bases_in, const fxg_reflow_opts *opts,
                      uint32_t *d_line, uint64_t cap_lines, uint8_t *d_out, fxg_reflow_info *info);
/* fastx_uncollapser (reference src/fastx_uncollapser/fastx_uncollapser.cpp:73-98, src/libfastx/fastx.c:440-495): collapsed FASTA expanded on
 * the device.  The block has been through fxg_fastq_index with lines_per_record == 2 (d_text, d_line, cap_lines, records and d_len as that call
 * left them).  Record r stands for count(r) reads: the number after the first '-' of its id as atoi reads it, 1 if there is no dash or the number
 * is not positive (fastx.c:475-495).  It goes out count(r) times as ">%llu\nBASES\n"; the numbers run through the block's copies in input
 * order, copy g (0-based) is named ordinal_base + g + 1.  Input ids and CR bytes do not survive.
 * The output can be many times the input, so a call writes the longest run of WHOLE copies from copy_begin on that fits out_cap bytes:
 * copies [copy_begin, info->copy_end), info->out_bytes bytes from d_out[0] on, and the caller walks the block window by window until copy_end
 * == info->copies.  A call with copy_begin == 0 makes the block's scans, in a workspace of the context that no other entry uses; a call with
 * copy_begin > 0 reuses the scans of the last fxg_fasta_uncollapse call with copy_begin == 0 on this context.  That this call was on the same
 * block is the caller's promise: the entry only notices a different number of records or another ordinal_base.  copy_begin == copies is a
 * valid call that writes nothing.
 * Refused (FXG_E_INVALID with a message) with d_out untouched: an out_cap smaller than copy copy_begin (the message says how many bytes it
 * needs); copy_begin > copies; ordinal_base + copies past 2^64 - 1; a window with copies of more than 2^27 records or of more than 2^27
 * further pieces of 16 copies (one launch each: give it a smaller out_cap; info is zeroed); text_len > 2^28.  The last one is what keeps every offset exact: byte
 * offsets, copies and pieces are 64-bit and no scan checks for overflow.  A record takes at least four bytes of text, so 2^28 bytes hold at
 * most 2^26 records whose (bases + 23) sum to less than 2^31, and a count is below 2^31: the block's output stays below 2^62 bytes.
 * d_out: exactly info->out_bytes bytes are written, never a byte past them.  Synchronises.  With profiling on, a call with copy_begin == 0
 * records three intervals: counts + scan, sizes + scans + window, copy; a later window of the block records the last two (its first: the window alone). */
typedef struct fxg_uncollapse_opts {
    uint64_t ordinal_base;   /* copies written by the blocks before this one: copy g of the block is named ordinal_base + g + 1 */
    uint64_t copy_begin;     /* first copy of the block this call writes.  > 0: the scans of the context's last call with copy_begin == 0 are used as they
                              * are, and that they are THIS block's is the caller's duty: the context remembers (records, ordinal_base) and nothing of the
                              * text (a caller reuses one buffer for block after block, so its address says nothing).  Another block with the same two
                              * numbers is accepted and written from the other block's scans; a context with no scans, other records or another
                              * ordinal_base is refused, "... copy_begin > 0 continues a block ...", d_out untouched. */
    uint64_t out_cap;        /* bytes d_out can take */
} fxg_uncollapse_opts;
typedef struct fxg_uncollapse_info {
    uint64_t copies;         /* of the whole block */
    uint64_t copy_end;       /* this call wrote copies [copy_begin, copy_end) */
    uint64_t out_bytes;      /* written to d_out */
} fxg_uncollapse_info;
int  fxg_fasta_uncollapse(fxg_ctx *ctx, const uint8_t *d_text, uint64_t text_len, const uint32_t *d_line, uint64_t cap_lines, uint64_t records,
                          const uint16_t *d_len, const fxg_uncollapse_opts *opts, uint8_t *d_out, fxg_uncollapse_info *info);
/* fasta_nucleotide_changer (reference src/fasta_nucleotide_changer/fasta_nucleotide_changer.c:101-115): the bases lines of an indexed block
 * rewritten in place.  The block has been through fxg_fastq_index (d_text, text_len, lines_per_record, d_line, cap_lines and records as that
 * call was given and left them).  (from, to) is ('T', 'U') -- DNA to RNA, the tool's -r -- or ('U', 'T') -- RNA to DNA, -d.  The call walks
 * the bases line of every record, line lines_per_record * r + 1 from its start to its chomped end: every `from` byte becomes `to` in
 * d_text and is counted; the smallest record whose bases line holds a `to` byte is reported (the reference stops there with a message);
 * a bases byte outside upper-case A C G T N U raises FXG_TEXT_IRR_BASE.  Every `from` byte of every record is rewritten whatever the other
 * two results say.  Nothing but `from` bytes of bases lines is written: ids, '+' lines, quality lines, a CR before the newline, the
 * newlines and the 16 bytes behind the text stay.  The block then goes out through fxg_fastq_format with out_fasta = 1, over
 * first_to_record records when a `to` byte was found.
 * Refused (FXG_E_INVALID with a message, nothing launched, info zeroed with first_to_record = ~0): another (from, to); lines_per_record not
 * 2 or 4; a null d_text or d_line with records > 0; a null info; more records than cap_lines or text_len can hold.  records == 0 is a valid
 * call that launches nothing.  The context needs no call before this one.  Synchronises.  With profiling on, a call records one interval. */
typedef struct fxg_bases_change_info {
    uint64_t changed;          /* `from` bytes rewritten, whole call */
    uint64_t first_to_record;  /* smallest record index whose bases line holds a `to` byte; ~0ull: none */
    uint32_t irregular;        /* FXG_TEXT_IRR_BASE if any bases byte is outside upper-case A C G T N U */
} fxg_bases_change_info;
int  fxg_bases_change(fxg_ctx *ctx, uint8_t *d_text, uint64_t text_len, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines,
                      uint64_t records, int from, int to, fxg_bases_change_info *info);
/* fastx_collapser (reference src/fastx_collapser/fastx_collapser.cpp:112-122): identical reads merged on the device.  A context holds one
 * set of sequences across blocks:
 *   fxg_collapse_begin   empties the set (device memory of an earlier set is kept and reused);
 *   fxg_collapse_add     one block that has been through fxg_fastq_index (d_text, text_len, lines_per_record, d_line, cap_lines, records and
 *                        d_len as that call was given and left them): the bases line of every record is checked against upper-case A C G T N,
 *                        copied into the set's arena and inserted, with the record's read count -- 1 for FASTQ, the number after the first
 *                        '-' of a FASTA id as atoi reads it, 1 if there is none or it is not positive (fastx.c:475-495).  Counts add up modulo
 *                        2^64.  A byte outside the alphabet, an empty bases line or a d_len entry that is not its line's length makes the
 *                        block irregular: info->irregular = FXG_TEXT_IRR_BASE, info->first_bad the smallest such record of the block, and
 *                        NOTHING of the block stays in the set -- the call returns FXG_OK and the set is what it was.  Blocks are added in
 *                        input order: the order of equal counts in the output depends on it.  Synchronises.
 *   fxg_collapse_add_rows  one block of packed rows into the same set, arena and record numbering, without leaving the device: record k is
 *                        d_len[k] bytes at d_bases + d_off[k] (no alignment), which is what fxg_run_pipeline leaves in out_bases / out_off /
 *                        out_len for kept read k, with records = counters[FXG_C_KEPT].  The rows came from a pack that checked the alphabet,
 *                        so it is not checked again.  The count source is optional: d_kept_index (fxg_out.kept_index) with the d_text, d_line,
 *                        cap_lines and lines_per_record of the indexed block the rows were packed from.  With lines_per_record == 2 record k
 *                        counts what the id line of source record d_kept_index[k] says, as above; with 4, or without a count source (all
 *                        five arguments null / 0), every record counts 1.  A d_len entry of zero makes the block irregular exactly as an
 *                        empty bases line does: FXG_TEXT_IRR_BASE, first_bad the smallest such k, nothing of the block in the set, FXG_OK.
 *                        first_base / last_base (0 or 1, 0: the whole row) cut every row as fastx_trimmer -f / -l does before it goes in:
 *                        bases first_base .. min(last_base, d_len[k]) counted from 1; a row that ends before first_base is left out as the
 *                        trimmer leaves it out -- it gets no record number, and info->records / ->reads tell how many went in.  (The engine
 *                        runs no chain of CLIP and FTRIM in one launch; this is how clip | trim | collapse stays on the device.)
 *                        Blocks of text and blocks of rows may alternate within one set; everything after the copy -- the table, the
 *                        rebuild rule, order and write -- is the same code.  Synchronises.
 *   fxg_collapse_order   after the last block: numbers the distinct sequences in first-occurrence order, downloads 16 bytes per distinct
 *                        sequence (hash and count), replays the reference's container on the host -- a std::unordered_map filled in that
 *                        order, iterated, stable-sorted by count, read backwards -- and sizes the output.  The result is byte-identical to the
 *                        reference built with HAVE_CXX11 == 1 against the libstdc++ this library was built with: records in descending count
 *                        order, equal counts in the reverse of that map's iteration order.  info->out_bytes is the whole output,
 *                        info->out_reads the second number of the reference's -v report (see below).
 *   fxg_collapse_write   the longest run of WHOLE records from rank_begin on that fits out_cap bytes, ranks [rank_begin, window->rank_end),
 *                        window->out_bytes bytes from d_out[0] on: ">rank-count\nBASES\n" with rank counted from 1.  The reference prints a
 *                        count after truncation to int (a sum of 2^31 prints as -2147483648, one of 2^32 as 0) and adds those ints into the
 *                        size_t of its report; both are reproduced, the sort uses the untruncated sums.  Exactly out_bytes bytes are written,
 *                        never a byte past them.  rank_begin == uniques is a valid call that writes nothing.  Synchronises.
 * Refused (FXG_E_INVALID with a message, nothing launched, d_out untouched): add, order or write before begin; add or order after order; write
 * before order; more than 2^40 - 2 records in a set; a null pointer with records > 0; lines_per_record other than 2 or 4; more records than
 * cap_lines or text_len can hold, text_len above 0xFFFFFFF0; add_rows with only some of the count source's arguments, or with a count source and
 * lines_per_record other than 2 or 4, or with a last_base before first_base; rank_begin above uniques; an out_cap smaller than record rank_begin (the message
 * says how many bytes it needs).  A device allocation that fails is FXG_E_NOMEM and says how many bytes the set wanted; the set is then as it
 * was before the call.  What a refused call leaves in its results: add and order refused for the set's state (no set, or an ordered one) leave
 * *info zeroed with first_bad = ~0ull; add refused for its arguments leaves the set's counts as they are (records, reads, uniques, slots,
 * rebuilds), irregular = 0 and first_bad = ~0ull (add_rows as add in both); a refused write leaves *window zeroed with rank_end = rank_begin.
 * The set is resident: its device memory is about the bases + 18 bytes per record + 48 to 96 bytes per distinct sequence (a table that is at
 * most half full), and fxg_collapse_order needs 8 more per record and 40 per distinct sequence while it runs; the host replay takes about 48
 * bytes per distinct sequence.  With profiling on, add records an interval for lengths + scan + copy + check, one for a rebuild of the table
 * if the block caused one, and one for the insert; add_rows records the same three (its first: lengths + scan + copy rows + counts, and the
 * download of the block's byte count between the scan and the copy, which sizes the arena); order records two (mark + scan + scatter; sizes + scan), write one. */
typedef struct fxg_collapse_opts {
    /* Both fields are test and measurement aids: they never change a result.  A null opts is {0, 0}. */
    uint64_t initial_slots;  /* slots of the table at first, rounded up to a power of two, 4 at the least; 0: the default, 65 536.  The table
                              * is rebuilt at twice the size or more whenever a block could fill it beyond a half. */
    uint32_t hash_bits;      /* 0: all 64.  k: only the low k bits of a sequence's hash reach the slot index and the fingerprint, so k = 1 puts
                              * every key on two probe chains and makes every probe compare bytes.  The order still uses the whole hash. */
} fxg_collapse_opts;
typedef struct fxg_collapse_info {
    uint64_t records;        /* in the set */
    uint64_t reads;          /* their counts together */
    uint64_t uniques;        /* distinct sequences */
    uint64_t slots;          /* of the table */
    uint64_t rebuilds;       /* of the table since begin */
    uint64_t first_bad;      /* add: the smallest irregular record of the block, ~0ull if none */
    uint64_t out_reads;      /* order: the printed (int) counts added into a size_t, the reference's "representing N reads" of its Output line */
    uint64_t out_bytes;      /* order: bytes of the whole output */
    uint32_t irregular;      /* add: FXG_TEXT_IRR_BASE if the block was refused as irregular */
} fxg_collapse_info;
typedef struct fxg_collapse_window {
    uint64_t rank_end;       /* this call wrote ranks [rank_begin, rank_end) */
    uint64_t out_bytes;      /* written to d_out */
} fxg_collapse_window;
int  fxg_collapse_begin(fxg_ctx *ctx, const fxg_collapse_opts *opts);
int  fxg_collapse_add(fxg_ctx *ctx, const uint8_t *d_text, uint64_t text_len, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines,
                      uint64_t records, const uint16_t *d_len, fxg_collapse_info *info);
int  fxg_collapse_add_rows(fxg_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_off, const uint16_t *d_len, uint64_t records,
                           uint32_t first_base, uint32_t last_base, const uint32_t *d_kept_index, const uint8_t *d_text, const uint32_t *d_line, uint64_t cap_lines, int lines_per_record,
                           fxg_collapse_info *info);
int  fxg_collapse_order(fxg_ctx *ctx, fxg_collapse_info *info);
int  fxg_collapse_write(fxg_ctx *ctx, uint64_t rank_begin, uint64_t out_cap, uint8_t *d_out, fxg_collapse_window *window);
int  fxg_host_register(fxg_ctx *ctx, void *ptr, size_t bytes);     /* page-lock an existing host buffer for async copies */
int  fxg_host_unregister(fxg_ctx *ctx, void *ptr);

/* fastx_quality_stats (src/fastx_quality_stats/fastx_quality_stats.c:166-216, read_file): adds the batch to
 *     d_hist[column][class][byte]      uint64, hist_cols x FXG_QS_CLASSES x FXG_QS_BINS, hist_cols >= batch stride
 * = how many reads have a base of class A,C,G,T,N (0..4) at that column with that quality byte (the byte stored in `qual`,
 * i.e. quality value + the offset the rows were packed with; 0 when the batch has no qualities).  Count, sum, min, max and
 * the quartiles the tool prints (:218-340) are functions of this histogram.  The caller zeroes d_hist before the first batch. */
#define FXG_QS_CLASSES 5
#define FXG_QS_BINS 128
int  fxg_run_quality_stats(fxg_ctx *ctx, const fxg_batch *in, uint64_t *d_hist, uint32_t hist_cols);

/* fastx_clipper on variable-length input.  The reference aligner keeps ONE query buffer and one matrix for the whole run: the
 * matrix never shrinks (sequence_alignment.cpp:135-136), every loop runs to the width of the longest read so far (:157, :375,
 * sequence_alignment.h:109), and set_sequences assigns each read into the same std::string -- so a read shorter than an earlier
 * one is aligned together with the stale tail that earlier reads left behind it, and can be clipped or discarded because of
 * it.  With history on (on != 0; the call also resets the buffer to that of a fresh process) the CLIP stage
 * reproduces this: the reads of a batch, and of successive fxg_run_* calls on this context, form one sequence in call order.
 * Off (the default), every read is aligned on its own, which is identical for input of one fixed length.  Sharding a
 * variable-length clipper job over several contexts is only exact with history off on both sides.
 * One history is one reference process, and that has ONE adapter: its matrix keeps the height of the adapter as it keeps the width of the
 * longest read, and only the reads' side of that is reproduced here.  A CLIP run whose adapter differs from that of the first CLIP run since
 * fxg_set_clip_history(ctx, on != 0) is refused -- FXG_E_INVALID, "clip history: the adapter differs from the one this history began with;
 * fxg_set_clip_history(ctx, 1) begins another" -- with nothing launched, no output touched and the history as it was.  Runs without a CLIP stage,
 * fxg_run_quality_stats and the text calls neither see nor move the history. */
int  fxg_set_clip_history(fxg_ctx *ctx, int on);

/* ---- several GPUs.  The reference is one process over one stream of reads (e.g.
 * fastq_quality_trimmer.c:76-124); here reads shard by contiguous index range, one context per GPU, and the ONLY exchange is each
 * shard's counter block: concatenating the shards' packed outputs in shard order reproduces the single-GPU output.  These three
 * helpers are host arithmetic / I/O; they need no context and no device.  How the counter blocks travel is the caller's
 * business: an RCCL all-gather between processes (fastx_toolkit_amd/distributed.py), plain memory between the threads of one
 * process (host/fxh_lanes.c, host/fxh_parts.c). ---- */
int  fxg_device_count(void);   /* HIP devices visible to this process (0 if none) */
/* NUMA node of the host memory nearest to HIP device `device` (its PCI function's /sys/bus/pci/devices/<id>/numa_node), -1 if unknown.
 * The boxes are two-socket machines with four GPUs per node: a host process whose page-locked buffers sit on the other socket uploads
 * across the socket link (host/fxh_lanes.c binds a run that uses one GPU to that node's CPUs before it creates its threads and buffers). */
int  fxg_device_numa_node(int device);
/* reads [*lo, *hi) of an n-read job owned by shard `rank` of `world`:  rank * n / world  ..  (rank + 1) * n / world */
int  fxg_shard_range(uint64_t n, uint32_t rank, uint32_t world, uint64_t *lo, uint64_t *hi);
/* gathered: world counter blocks in shard order (world * FXG_NCOUNTERS values).  totals (optional): the job's counters (sums;
 * the device error words are OR-ed).  read_off / byte_off (optional): kept reads / kept bytes of the shards before `rank`,
 * i.e. where this shard's kept_index / out_off entries and its packed bytes start in the job's output. */
int  fxg_epilogue(const uint64_t *gathered, uint32_t world, uint32_t rank, uint64_t totals[FXG_NCOUNTERS],
                  uint64_t *read_off, uint64_t *byte_off);
/* The concatenation: write this shard's `bytes` bytes of packed output (host memory) at `offset` of the open file `fd`
 * (pwrite until done; shards may write concurrently, in any order). */
int  fxg_concat_pwrite(int fd, const void *host_buf, uint64_t bytes, uint64_t offset);
/* The concatenation kept on the devices (one process driving several GPUs): copy this shard's `bytes` bytes of packed
 * output from `d_src` (memory of context `src`) to `d_dst + byte_off` (memory of context `dst`, the job's assembled output) -- over xGMI
 * when the contexts sit on different GPUs (hipMemcpyPeerAsync on `src`'s stream, behind the pass that produced the slice).  The caller
 * waits for every source context (fxg_sync) before it reads the assembled output. */
int  fxg_concat_peer(fxg_ctx *dst, void *d_dst, uint64_t byte_off, fxg_ctx *src, const void *d_src, uint64_t bytes);

/* The exchange itself for a C host, one process per GPU: the counter blocks travel by ONE RCCL all-gather (192 bytes per rank, over
 * xGMI inside a node) -- SURVEY 8e's ncclAllReduce + ncclAllGather folded into one collective, since the gathered blocks give both the
 * totals and the offsets.  librccl.so is opened at run time (dlopen), so a single-GPU installation needs no RCCL.
 *   fxg_comm_create : ranks meet through `rendezvous_file` (a path all of them can reach): rank 0 writes the RCCL unique id there,
 *                     the others wait up to timeout_s seconds for it; every rank then joins the communicator of `world` ranks on its
 *                     context's device.  The file may be removed once every rank has returned.
 *   fxg_epilogue_rccl : d_counters = this rank's counter block on the device (fxg_out.counters of the pass just enqueued; NULL = the
 *                     context's own).  Enqueues the all-gather on the context's stream behind the pass, waits for it, and applies
 *                     fxg_epilogue.  gathered (optional, world * FXG_NCOUNTERS values) receives the blocks in rank order. */
typedef struct fxg_comm fxg_comm;
int  fxg_comm_create(fxg_ctx *ctx, const char *rendezvous_file, uint32_t rank, uint32_t world, int timeout_s, fxg_comm **comm);
void fxg_comm_destroy(fxg_comm *comm);
int  fxg_epilogue_rccl(fxg_ctx *ctx, fxg_comm *comm, const uint64_t *d_counters, uint64_t totals[FXG_NCOUNTERS],
                       uint64_t *read_off, uint64_t *byte_off, uint64_t *gathered);

/* Kernel-level timing: when enabled, every fxg_run_pipeline brackets its dominant kernel (not the
 * memset / counter-reduce helpers) with HIP events on the launch stream; fxg_last_kernel_ms waits for
 * that launch and returns its duration. */
int  fxg_set_profiling(fxg_ctx *ctx, int enabled);
int  fxg_last_kernel_ms(fxg_ctx *ctx, float *elapsed_ms);
/* The durations of the last profiled launches (a ring of 64), oldest first, without disturbing launches that are still being
 * enqueued back to back: a timed loop records its own launches and reads them all after its final synchronisation (bench.py). */
int  fxg_profiled_kernel_ms(fxg_ctx *ctx, float *elapsed_ms, uint32_t cap, uint32_t *n);

/* Name and launch geometry of the dominant kernel of the last fxg_run_pipeline (for profiling). */
int  fxg_last_launch_info(const fxg_ctx *ctx, char *kernel_name, size_t cap, uint32_t *grid, uint32_t *block,
                          uint32_t *lds_bytes, uint32_t *tile_reads);

#ifdef __cplusplus
}
#endif
#endif /* FXG_H */
