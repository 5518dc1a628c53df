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
 * are no lanes, no parts, no second GPU and no FXH_WORLD here.  See fxh_collapse.h. */
#include "fxh_priv.h"
#include "fxh_collapse.h"

/* the entries the run needs; a library without them (the CPU tier's stock look-alike) leaves the references null */
extern int fxg_collapse_begin(fxg_ctx *, const fxg_collapse_opts *) __attribute__((weak));
extern int fxg_collapse_add(fxg_ctx *, const uint8_t *, uint64_t, int, const uint32_t *, uint64_t, uint64_t, const uint16_t *, fxg_collapse_info *) __attribute__((weak));
extern int fxg_collapse_order(fxg_ctx *, fxg_collapse_info *) __attribute__((weak));
extern int fxg_collapse_write(fxg_ctx *, uint64_t, uint64_t, uint8_t *, fxg_collapse_window *) __attribute__((weak));

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
        if (!dev_block(u, u->fa, at, 1, 2, &used) || used != at) errx(1, "internal error: a block the record API accepted is irregular to the device after its rewrite");
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
    free(u->fa);
    fxg_ctx_destroy(u->down);
    fxg_ctx_destroy(u->ctx);
}

void fxh_collapse_run(FASTX *fx, fxh_collapse_totals *tot)
{
    memset(tot, 0, sizeof *tot);
    if (!fxg_collapse_begin || !fxg_collapse_add || !fxg_collapse_order || !fxg_collapse_write)
        errx(1, "this libfxg.so has no fxg_collapse_begin / _add / _order / _write: reads are merged on the GPU only, and there is no CPU fallback");
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
    for (;;) {
        fxh_next_block(&pf, rd, &spare);
        char *p = rd->buf + rd->beg;
        size_t len = rd->end - rd->beg, used;
        const int eof = rd->eof;
        if (eof && len > 0 && p[len - 1] != '\n') { p[len++] = '\n'; rd->end++; }      /* (the reader's buffers hold cap + 1 bytes) */
        dev_pin(&u, rd);
        const uint64_t before = u.info.records;
        if (dev_block(&u, p, len, eof, u.lpr, &used)) {
            rd->beg += used;
            fx->input_line_number += (unsigned long long)u.lpr * (u.info.records - before);      /* (the record API's messages carry the line in the whole input) */
            if (eof) break;
        } else if (!record_block(&u, fx)) break;
    }
    fxh_prefetch_stop(&pf);
    fxg_collapse_info info;
    DEV_CHECK(&u, fxg_collapse_order(u.ctx, &info));
    const size_t window = rd->cap < FXH_CL_WINDOW_MIN ? FXH_CL_WINDOW_MIN : rd->cap > FXH_CL_WINDOW_MAX ? FXH_CL_WINDOW_MAX : rd->cap;
    dev_write(&u, window, info.uniques);
    dev_close(&u);
    tot->input_sequences = (size_t)info.records; tot->input_reads = (size_t)info.reads;
    tot->output_sequences = (size_t)info.uniques; tot->output_reads = (size_t)info.out_reads;
}
