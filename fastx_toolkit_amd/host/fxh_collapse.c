/* fxh_collapse.c -- fastx_collapser's run.  The input is read in blocks through the prefetch of fxh_io.c, in input order on one context: the
 * order of equal counts in the output depends on the order the sequences first appear in.  Every block is indexed (fxg_fastq_index), a FASTQ
 * block goes through fxg_fastq_pack for its quality lines, and fxg_collapse_add checks the bases and merges the block's reads into the
 * context's set.  A block the device calls irregular goes through the record API, which owns the reference's messages: a bad record ends the
 * run there with that message and status 1 -- nothing has been written by then, the output is written after the last read, so the -o file
 * exists and is empty as the reference's does.  If the record API accepts the block (CR bytes in odd places, numeric quality lines, a '+'
 * line with a name ...), its records are rewritten into a plain two-line FASTA block -- the id kept, ">x" for a FASTQ record, which counts 1 --
 * and that block is added.  There is no merging on the CPU: this project has no CPU fallback, and a library without the four entries makes
 * the tool say so and exit 1.
 * After the last block fxg_collapse_order numbers and orders the set, and its windows go through two device output buffers: a window is
 * downloaded on a second context's stream and handed to the writer thread while the next one is written.  The result is global, so there
 * are no lanes, no parts, no second GPU and no FXH_WORLD here.  See fxh_collapse.h.
 * With a stage chain (fxh_collapse_run_chain, fastx_clip_collapser: clip, or clip + trim) the reads a block keeps never leave the device between
 * the chain and the set: every block, FASTA as well, is indexed and packed, fxg_run_pipeline compacts the reads the clip stage keeps (out_bases /
 * out_off / out_len / kept_index) and fxg_collapse_add_rows copies those rows into the set's arena -- cut to the trim stage's first .. last base
 * on the way, if there is one -- with the ids of a FASTA block as the count source.
 * The run is one context in input order already, which is what the clipper's one aligner needs (fxg_set_clip_history).  A block the
 * device calls irregular goes the same way as above and takes the device path, chain included, after its rewrite. */
#include "fxh_priv.h"
#include "fxh_collapse.h"

/* the entries the run needs; a library without them (the CPU tier's stock look-alike) leaves the references null */
extern int fxg_collapse_begin(fxg_ctx *, const fxg_collapse_opts *) __attribute__((weak));
extern int fxg_collapse_add(fxg_ctx *, const uint8_t *, uint64_t, int, const uint32_t *, uint64_t, uint64_t, const uint16_t *, fxg_collapse_info *) __attribute__((weak));
extern int fxg_collapse_order(fxg_ctx *, fxg_collapse_info *) __attribute__((weak));
extern int fxg_collapse_write(fxg_ctx *, uint64_t, uint64_t, uint8_t *, fxg_collapse_window *) __attribute__((weak));
/* the chain run alone needs this one */
extern int fxg_collapse_add_rows(fxg_ctx *, const uint8_t *, const uint64_t *, const uint16_t *, uint64_t, uint32_t, uint32_t, const uint32_t *, const uint8_t *, const uint32_t *, uint64_t, int,
                                 fxg_collapse_info *) __attribute__((weak));

#define FXH_CL_WINDOW_MIN ((size_t)1 << 20)            /* a window holds at least this: far more than the largest record (bases of 24 998 and more never get here) */
#define FXH_CL_WINDOW_MAX ((size_t)1 << 28)

typedef struct {
    fxg_ctx *ctx, *down;                                 /* the kernels' context; one whose stream only carries the downloads */
    uint8_t *d_text, *d_bases, *d_qual, *d_flags, *d_out[2]; uint32_t *d_line; uint16_t *d_len;
    size_t d_text_cap, d_bases_cap, d_qual_cap, d_flags_cap, d_line_cap, d_len_cap;
    size_t window;                                       /* bytes of d_out[s] and h_out[s] */
    char *h_out[2];
    char *fa; size_t fa_cap;                             /* a block the record API took, rewritten as two-line FASTA */
    int slot, pend; size_t pend_bytes;                   /* the buffers of the next window; the download in flight (-1: none) and its size */
    const void *pinned[8]; int npinned;
    int lpr, qoffset;
    fxg_collapse_info info;                              /* of the last add */
    struct fxh_writer *w;
    fxh_awriter aw;
    /* the chain run: its params, what fxg_run_pipeline writes, the input records of the last block, the stages' totals */
    const fxg_params *p;
    uint8_t *d_kept_bases; uint32_t *d_res, *d_kept_index; uint16_t *d_kept_len; uint64_t *d_kept_off, *d_counters;
    size_t d_kept_bases_cap, d_res_cap, d_kept_index_cap, d_kept_len_cap, d_kept_off_cap;
    uint64_t block_records;
    fxh_totals *stages;
} cpath;

#define DEV_CHECK_ON(c, call) do { if ((call) != FXG_OK) errx(1, "%s: %s", #call, fxg_last_error(c)); } while (0)
#define DEV_CHECK(u, call) DEV_CHECK_ON((u)->ctx, call)

static void dev_grow(cpath *u, void **p, size_t *cap, size_t want)
{
    if (*cap >= want) return;
    if (*p) (void)fxg_free_device(u->ctx, *p);
    *p = NULL; *cap = 0;
    want += want / 8 + 4096;
    DEV_CHECK(u, fxg_malloc_device(u->ctx, want, p));
    *cap = want;
}

/* the reader's buffers are page-locked the first time a block comes out of them (a failure only makes the upload slower) */
static void dev_pin(cpath *u, const struct fxh_reader *rd)
{
    for (int i = 0; i < u->npinned; ++i) if (u->pinned[i] == rd->buf) return;
    if (u->npinned == (int)(sizeof u->pinned / sizeof u->pinned[0])) return;
    u->pinned[u->npinned++] = rd->buf;
    (void)fxg_host_register(u->ctx, rd->buf, rd->cap + 1);
}

static size_t count_nl(const char *p, size_t n)
{
    size_t c = 0;
    const char *e = p + n;
    while (p < e && (p = (const char *)memchr(p, '\n', (size_t)(e - p))) != NULL) { ++c; ++p; }
    return c;
}

/* One block of whole lines into the set: upload, index, (FASTQ) pack, add.  Returns 1 with *used = the bytes of its whole records, or 0: the
 * device calls it irregular, or it holds no whole record, and nothing of it is in the set. */
static int dev_block(cpath *u, const char *p, size_t len, int eof, int lpr, size_t *used)
{
    *used = 0;
    if (len == 0) return 1;
    if (len > 0xFFFFFF00u) return 0;
    const size_t cap_lines = count_nl(p, len) + 2;
    fxg_text_info ti;
    dev_grow(u, (void **)&u->d_text, &u->d_text_cap, len + 64);
    dev_grow(u, (void **)&u->d_line, &u->d_line_cap, 2 * cap_lines * sizeof(uint32_t));
    dev_grow(u, (void **)&u->d_len, &u->d_len_cap, (cap_lines / (size_t)lpr + 4) * sizeof(uint16_t));
    dev_grow(u, (void **)&u->d_flags, &u->d_flags_cap, cap_lines / (size_t)lpr + 4);
    DEV_CHECK(u, fxg_memcpy_h2d(u->ctx, u->d_text, p, len));
    DEV_CHECK(u, fxg_fastq_index(u->ctx, u->d_text, len, eof, lpr, u->d_line, cap_lines, u->d_len, u->d_flags, &ti));
    if (ti.irregular || ti.records == 0) return 0;
    const uint64_t n = ti.records;
    if (lpr == 4) {                                      /* the quality lines: the pack's check */
        const uint32_t stride = ti.max_len;
        uint32_t irr = 0;
        if (n * stride > (uint64_t)8 * len + (1u << 20)) return 0;      /* ragged beyond reason, as the lanes rule (fxh_lanes.c) */
        dev_grow(u, (void **)&u->d_bases, &u->d_bases_cap, (size_t)n * stride + 32);
        dev_grow(u, (void **)&u->d_qual, &u->d_qual_cap, (size_t)n * stride + 32);
        DEV_CHECK(u, fxg_fastq_pack(u->ctx, u->d_text, len, lpr, u->d_line, cap_lines, u->d_flags, n, stride, u->qoffset, u->d_bases, u->d_qual, &irr));
        if (irr) return 0;
    }
    DEV_CHECK(u, fxg_collapse_add(u->ctx, u->d_text, ti.consumed, lpr, u->d_line, cap_lines, n, u->d_len, &u->info));
    if (u->info.irregular) return 0;
    *used = (size_t)ti.consumed;
    return 1;
}

/* dev_block of the chain run: upload, index, pack, the chain, the kept rows into the set.  Same returns. */
static int dev_block_chain(cpath *u, const char *p, size_t len, int eof, int lpr, size_t *used)
{
    *used = 0;
    u->block_records = 0;
    if (len == 0) return 1;
    if (len > 0xFFFFFF00u) return 0;
    const size_t cap_lines = count_nl(p, len) + 2;
    fxg_text_info ti;
    dev_grow(u, (void **)&u->d_text, &u->d_text_cap, len + 64);
    dev_grow(u, (void **)&u->d_line, &u->d_line_cap, 2 * cap_lines * sizeof(uint32_t));
    dev_grow(u, (void **)&u->d_len, &u->d_len_cap, (cap_lines / (size_t)lpr + 4) * sizeof(uint16_t));
    dev_grow(u, (void **)&u->d_flags, &u->d_flags_cap, cap_lines / (size_t)lpr + 4);
    DEV_CHECK(u, fxg_memcpy_h2d(u->ctx, u->d_text, p, len));
    DEV_CHECK(u, fxg_fastq_index(u->ctx, u->d_text, len, eof, lpr, u->d_line, cap_lines, u->d_len, u->d_flags, &ti));
    if (ti.irregular || ti.records == 0) return 0;
    const uint64_t n = ti.records;
    const uint32_t stride = ti.max_len;
    uint32_t irr = 0;
    if (n * stride > (uint64_t)8 * len + (1u << 20)) return 0;          /* ragged beyond reason, as the lanes rule (fxh_lanes.c) */
    dev_grow(u, (void **)&u->d_bases, &u->d_bases_cap, (size_t)n * stride + 32);
    if (lpr == 4) dev_grow(u, (void **)&u->d_qual, &u->d_qual_cap, (size_t)n * stride + 32);      /* the quality lines: the pack's check; no stage of the chain reads them */
    DEV_CHECK(u, fxg_fastq_pack(u->ctx, u->d_text, len, lpr, u->d_line, cap_lines, u->d_flags, n, stride, u->qoffset, u->d_bases, lpr == 4 ? u->d_qual : NULL, &irr));
    if (irr) return 0;
    dev_grow(u, (void **)&u->d_kept_bases, &u->d_kept_bases_cap, (size_t)n * stride + 32);
    dev_grow(u, (void **)&u->d_res, &u->d_res_cap, (size_t)n * sizeof(uint32_t));
    dev_grow(u, (void **)&u->d_kept_index, &u->d_kept_index_cap, (size_t)n * sizeof(uint32_t));
    dev_grow(u, (void **)&u->d_kept_len, &u->d_kept_len_cap, (size_t)n * sizeof(uint16_t));
    dev_grow(u, (void **)&u->d_kept_off, &u->d_kept_off_cap, (size_t)n * sizeof(uint64_t));
    const fxg_batch in = {u->d_bases, NULL, ti.min_len == ti.max_len ? NULL : u->d_len, ti.max_len, stride, n};
    const fxg_out out = {u->d_res, u->d_kept_bases, NULL, u->d_kept_len, u->d_kept_index, u->d_kept_off, u->d_counters};
    fxg_params pp = *u->p;
    uint64_t ctr[FXG_NCOUNTERS], weighted[8];
    const int trim = (pp.stages & FXG_STAGE_FTRIM) != 0;                 /* no launch runs CLIP and FTRIM together: the rows are cut on their way into the set */
    const uint32_t first = trim ? (uint32_t)pp.ft_first : 1u, last = trim ? (uint32_t)pp.ft_last : 0u;
    pp.stages &= ~FXG_STAGE_FTRIM;
    pp.qoffset = 33;
    DEV_CHECK(u, fxg_run_pipeline(u->ctx, &in, &pp, &out));
    DEV_CHECK(u, fxg_read_counters(u->ctx, u->d_counters, ctr));       /* synchronises */
    if (lpr == 2) DEV_CHECK(u, fxg_fasta_weights(u->ctx, u->d_text, u->d_line, cap_lines, n, u->d_res, weighted));
    if (lpr == 2) DEV_CHECK(u, fxg_collapse_add_rows(u->ctx, u->d_kept_bases, u->d_kept_off, u->d_kept_len, ctr[FXG_C_KEPT], first, last, u->d_kept_index, u->d_text, u->d_line, cap_lines, 2, &u->info));
    else DEV_CHECK(u, fxg_collapse_add_rows(u->ctx, u->d_kept_bases, u->d_kept_off, u->d_kept_len, ctr[FXG_C_KEPT], first, last, NULL, NULL, NULL, 0, 0, &u->info));
    if (u->info.irregular) errx(1, "internal error: the chain kept a read without bases (kept read %llu of a block)", (unsigned long long)u->info.first_bad);
    fxh_add_counters(u->stages, ctr, n, lpr == 2 ? weighted : NULL);
    u->block_records = n;
    *used = (size_t)ti.consumed;
    return 1;
}

/* The whole records of the reader's block through the record API -- a bad one ends the run inside fxh_next_raw or fxh_decode_quality with the
 * reference's message -- rewritten as two-line FASTA and added.  Returns 0 at the end of the input. */
static int record_block(cpath *u, FASTX *fx)
{
    struct fxh_rawrec rec;
    size_t at = 0;
    int rc;
    memset(&rec, 0, sizeof rec);
    while ((rc = fxh_next_raw(fx, &rec, 0)) == 1) {
        if (fx->read_fastq) (void)fxh_decode_quality(fx, &rec, fx->quality, NULL);      /* (the reference's messages for a bad quality line) */
        const size_t name_len = fx->read_fastq ? 1 : rec.name_len, need = at + name_len + rec.seq_len + 3;
        if (need > u->fa_cap) {
            u->fa_cap = need + need / 2 + ((size_t)1 << 20);
            if (!(u->fa = (char *)realloc(u->fa, u->fa_cap))) errx(1, "out of memory (%zu bytes for a rewritten block)", u->fa_cap);
        }
        u->fa[at++] = '>';
        if (fx->read_fastq) u->fa[at++] = 'x'; else { memcpy(u->fa + at, rec.name, rec.name_len); at += rec.name_len; }
        u->fa[at++] = '\n';
        memcpy(u->fa + at, rec.seq, rec.seq_len); at += rec.seq_len;
        u->fa[at++] = '\n';
    }
    if (at) {
        size_t used = 0;
        if (!(u->p ? dev_block_chain : dev_block)(u, u->fa, at, 1, 2, &used) || used != at) errx(1, "internal error: a block the record API accepted is irregular to the device after its rewrite");
    }
    return rc != 0;
}

/* the download in flight: wait for it and hand it to the writer thread */
static void dev_drain(cpath *u)
{
    if (u->pend < 0) return;
    DEV_CHECK_ON(u->down, fxg_sync(u->down));
    fxh_awriter_submit_ext(&u->aw, u->w, u->h_out[u->pend], u->pend_bytes);      /* (returns once the write before this one is done) */
    u->pend = -1;
}

static void dev_open(cpath *u, FASTX *fx)
{
    memset(u, 0, sizeof *u);
    u->w = fx->writer; u->pend = -1;
    u->lpr = fx->read_fastq ? 4 : 2;
    u->qoffset = fx->fastq_ascii_quality_offset;
    int dev[FXH_MAX_LANES];
    (void)fxh_device_list(dev, FXH_MAX_LANES);
    const int rc = fxg_ctx_create(dev[0], &u->ctx);
    if (rc != FXG_OK) errx(1, "no usable GPU (device %d): the engine has no CPU fallback (fxg_ctx_create = %d)", dev[0], rc);
    if (fxg_ctx_create(dev[0], &u->down) != FXG_OK) errx(1, "a second context on device %d failed", dev[0]);
    DEV_CHECK(u, fxg_collapse_begin(u->ctx, NULL));
}

/* the chain run's share of dev_open: the counter block, and one aligner for the whole run */
static void dev_open_chain(cpath *u, const fxg_params *p, fxh_totals *stages)
{
    u->p = p; u->stages = stages;
    DEV_CHECK(u, fxg_malloc_device(u->ctx, FXG_NCOUNTERS * sizeof(uint64_t), (void **)&u->d_counters));
    if (p->stages & FXG_STAGE_CLIP) DEV_CHECK(u, fxg_set_clip_history(u->ctx, 1));
}

/* the set's records, window by window */
static void dev_write(cpath *u, size_t window, uint64_t uniques)
{
    u->window = window;
    for (int s = 0; s < 2; ++s) {
        DEV_CHECK(u, fxg_malloc_device(u->ctx, u->window + 64, (void **)&u->d_out[s]));
        DEV_CHECK(u, fxg_malloc_host(u->ctx, u->window, (void **)&u->h_out[s]));
    }
    uint64_t rank = 0;
    while (rank < uniques) {
        const int s = u->slot;
        fxg_collapse_window win;
        DEV_CHECK(u, fxg_collapse_write(u->ctx, rank, u->window, u->d_out[s], &win));
        dev_drain(u);                                    /* the window before: its download ran beside this window's kernel */
        DEV_CHECK_ON(u->down, fxg_memcpy_d2h(u->down, u->h_out[s], u->d_out[s], (size_t)win.out_bytes));
        u->pend = s; u->pend_bytes = (size_t)win.out_bytes;
        u->slot = s ^ 1;
        rank = win.rank_end;
    }
    dev_drain(u);
    fxh_awriter_stop(&u->aw);
}

static void dev_close(cpath *u)
{
    for (int i = 0; i < u->npinned; ++i) (void)fxg_host_unregister(u->ctx, (void *)u->pinned[i]);
    for (int s = 0; s < 2; ++s) {
        if (u->h_out[s]) (void)fxg_free_host(u->ctx, u->h_out[s]);
        if (u->d_out[s]) (void)fxg_free_device(u->ctx, u->d_out[s]);
    }
    if (u->d_text) (void)fxg_free_device(u->ctx, u->d_text);
    if (u->d_line) (void)fxg_free_device(u->ctx, u->d_line);
    if (u->d_len) (void)fxg_free_device(u->ctx, u->d_len);
    if (u->d_flags) (void)fxg_free_device(u->ctx, u->d_flags);
    if (u->d_bases) (void)fxg_free_device(u->ctx, u->d_bases);
    if (u->d_qual) (void)fxg_free_device(u->ctx, u->d_qual);
    void *chain[] = {u->d_kept_bases, u->d_res, u->d_kept_index, u->d_kept_len, u->d_kept_off, u->d_counters};
    for (size_t i = 0; i < sizeof chain / sizeof chain[0]; ++i) if (chain[i]) (void)fxg_free_device(u->ctx, chain[i]);
    free(u->fa);
    fxg_ctx_destroy(u->down);
    fxg_ctx_destroy(u->ctx);
}

int fxh_collapse_run_chain(FASTX *fx, const fxg_params *chain, void (*open_writer)(FASTX *), fxh_collapse_totals *tot, fxh_totals *stages)
{
    memset(tot, 0, sizeof *tot);
    if (chain) memset(stages, 0, sizeof *stages);
    if (!fxg_collapse_begin || !fxg_collapse_add || !fxg_collapse_order || !fxg_collapse_write)
        errx(1, "this libfxg.so has no fxg_collapse_begin / _add / _order / _write: reads are merged on the GPU only, and there is no CPU fallback");
    if (chain && !fxg_collapse_add_rows)
        errx(1, "this libfxg.so has no fxg_collapse_add_rows: the reads a stage chain keeps go into the set on the GPU only, and there is no CPU fallback");
    struct fxh_reader *rd = fx->reader;
    if (!fxh_read_buffer_bytes()) {
        struct stat sb;
        fxh_reader_reserve(rd, (size_t)(fstat(rd->fd, &sb) == 0 && S_ISFIFO(sb.st_mode) ? 16 : 64) << 20);
    }
    fxh_prefetch pf;
    memset(&pf, 0, sizeof pf);
    char *spare = NULL;
    cpath u;
    dev_open(&u, fx);
    if (chain) dev_open_chain(&u, chain, stages);
    for (;;) {
        fxh_next_block(&pf, rd, &spare);
        char *p = rd->buf + rd->beg;
        size_t len = rd->end - rd->beg, used;
        const int eof = rd->eof;
        if (eof && len > 0 && p[len - 1] != '\n') { p[len++] = '\n'; rd->end++; }      /* (the reader's buffers hold cap + 1 bytes) */
        dev_pin(&u, rd);
        const uint64_t before = u.info.records;
        if ((u.p ? dev_block_chain : dev_block)(&u, p, len, eof, u.lpr, &used)) {
            rd->beg += used;
            fx->input_line_number += (unsigned long long)u.lpr * (u.p ? u.block_records : u.info.records - before);      /* (the record API's messages carry the line in the whole input) */
            if (eof) break;
        } else if (!record_block(&u, fx)) break;
    }
    fxh_prefetch_stop(&pf);
    fxg_collapse_info info;
    DEV_CHECK(&u, fxg_collapse_order(u.ctx, &info));
    if (open_writer) {
        if (info.records == 0) { dev_close(&u); return 0; }        /* nothing was kept: nothing is opened, nothing written */
        open_writer(fx);
        u.w = fx->writer;
    }
    const size_t window = rd->cap < FXH_CL_WINDOW_MIN ? FXH_CL_WINDOW_MIN : rd->cap > FXH_CL_WINDOW_MAX ? FXH_CL_WINDOW_MAX : rd->cap;
    dev_write(&u, window, info.uniques);
    dev_close(&u);
    tot->input_sequences = (size_t)info.records; tot->input_reads = (size_t)info.reads;
    tot->output_sequences = (size_t)info.uniques; tot->output_reads = (size_t)info.out_reads;
    return 1;
}

void fxh_collapse_run(FASTX *fx, fxh_collapse_totals *tot) { (void)fxh_collapse_run_chain(fx, NULL, NULL, tot, NULL); }
