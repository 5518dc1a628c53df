/* fxh_uncollapse.c -- fastx_uncollapser's run.  The input is read in blocks through the prefetch of fxh_io.c; every block is validated as the
 * lane of a tool without a stage validates it (fxg_fastq_index + fxg_fastq_pack) and then expanded by fxg_fasta_uncollapse on one context, window
 * by window through two device output buffers: a window is downloaded on a second context's stream and handed to the writer thread while the
 * next one is expanded.  The running number is serial: a block's ordinal base is the base of the block before it plus that block's copies, so
 * there are no lanes, no second GPU and no FXH_WORLD here.  A block the device path does not take -- irregular in any way, ragged beyond reason,
 * larger than the entry's limit -- ends the device path: the rest of the input goes through the record API, which owns the reference's messages,
 * from that block's first byte on and numbered from where the device stopped.  A library without the entry runs the whole input that way: the
 * reference's own four lines over fastx.h.  See fxh_uncollapse.h. */
#include "fxh_priv.h"
#include "fxh_uncollapse.h"

/* the entry the device path needs; a library without it (the CPU tier's look-alike) leaves the reference null */
extern int fxg_fasta_uncollapse(fxg_ctx *, const uint8_t *, uint64_t, const uint32_t *, uint64_t, uint64_t, const uint16_t *, const fxg_uncollapse_opts *, uint8_t *,
                                fxg_uncollapse_info *) __attribute__((weak));

#define FXH_UC_BLOCK_MAX ((size_t)1 << 28)             /* fxg_fasta_uncollapse takes no larger block (include/fxg.h) */
#define FXH_UC_WINDOW_MIN ((size_t)1 << 20)            /* a window holds at least this: far more than the largest copy (fxg_fastq_index flags bases of 24 998 and more as irregular, and such a block never gets here) */

/* ---- the record path ---- */
static void write_copies(FASTX *fx, size_t *seqid)       /* fastx_uncollapser.cpp:84-89 */
{
    const int count = get_reads_count(fx);
    for (int i = 0; i < count; ++i) {
        snprintf(fx->name, sizeof fx->name, "%zu", *seqid);
        ++*seqid;
        fastx_write_record(fx);
    }
}

/* fastx_read_next_record where the blocks come from the prefetch (the read-ahead thread owns the file's position once it runs) */
static int next_record(FASTX *fx, fxh_prefetch *pf, char **spare)
{
    struct fxh_rawrec rec;
    memset(&rec, 0, sizeof rec);
    for (;;) {
        const int rc = fxh_next_raw(fx, &rec, 0);
        if (rc == 0) return 0;
        if (rc == 1) break;
        fxh_next_block(pf, fx->reader, spare);           /* the record is not whole in this block (and the input has not ended) */
    }
    memcpy(fx->name, rec.name, rec.name_len); fx->name[rec.name_len] = 0;
    memcpy(fx->nucleotides, rec.seq, rec.seq_len); fx->nucleotides[rec.seq_len] = 0;
    fx->num_input_sequences++;
    fx->num_input_reads += (size_t)get_reads_count(fx);
    return 1;
}

/* ---- the device path ---- */
typedef struct {
    fxg_ctx *ctx, *down;                                 /* the kernels' context; one whose stream only carries the downloads */
    uint8_t *d_text, *d_bases, *d_flags, *d_out[2]; uint32_t *d_line; uint16_t *d_len;
    size_t d_text_cap, d_bases_cap, d_flags_cap, d_line_cap, d_len_cap;
    size_t window;                                       /* bytes of d_out[s] and h_out[s] */
    char *h_out[2];
    int slot, pend; size_t pend_bytes;                   /* the buffers of the next window; the download in flight (-1: none) and its size */
    const void *pinned[8]; int npinned;
    uint64_t base;                                       /* copies written so far: the next block's ordinal base */
    uint64_t sequences;
    struct fxh_writer *w;
    fxh_awriter aw;
} upath;

#define DEV_CHECK_ON(c, call) do { if ((call) != FXG_OK) errx(1, "%s: %s", #call, fxg_last_error(c)); } while (0)
#define DEV_CHECK(u, call) DEV_CHECK_ON((u)->ctx, call)

static void dev_grow(upath *u, void **p, size_t *cap, size_t want)
{
    if (*cap >= want) return;
    if (*p) (void)fxg_free_device(u->ctx, *p);
    *p = NULL; *cap = 0;
    want += want / 8 + 4096;
    DEV_CHECK(u, fxg_malloc_device(u->ctx, want, p));
    *cap = want;
}

/* the reader's buffers are page-locked the first time a block comes out of them (a failure only makes the upload slower) */
static void dev_pin(upath *u, const struct fxh_reader *rd)
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

/* the download in flight: wait for it and hand it to the writer thread */
static void dev_drain(upath *u)
{
    if (u->pend < 0) return;
    DEV_CHECK_ON(u->down, fxg_sync(u->down));
    fxh_awriter_submit_ext(&u->aw, u->w, u->h_out[u->pend], u->pend_bytes);      /* (returns once the write before this one is done) */
    u->pend = -1;
}

/* One block: upload, validate, then its windows.  Returns 1 with *used = the bytes of its whole records, or 0: the record path takes the input
 * from this block on (nothing of the block has been written). */
static int dev_block(upath *u, const char *p, size_t len, int eof, size_t *used)
{
    *used = 0;
    if (len == 0) return 1;
    if (len > FXH_UC_BLOCK_MAX) return 0;
    const size_t cap_lines = count_nl(p, len) + 2;
    fxg_text_info ti;
    dev_grow(u, (void **)&u->d_text, &u->d_text_cap, len + 64);
    dev_grow(u, (void **)&u->d_line, &u->d_line_cap, 2 * cap_lines * sizeof(uint32_t));
    dev_grow(u, (void **)&u->d_len, &u->d_len_cap, (cap_lines / 2 + 4) * sizeof(uint16_t));
    dev_grow(u, (void **)&u->d_flags, &u->d_flags_cap, cap_lines / 2 + 4);
    DEV_CHECK(u, fxg_memcpy_h2d(u->ctx, u->d_text, p, len));
    DEV_CHECK(u, fxg_fastq_index(u->ctx, u->d_text, len, eof, 2, u->d_line, cap_lines, u->d_len, u->d_flags, &ti));
    if (ti.irregular || ti.records == 0) return 0;
    const uint64_t n = ti.records;
    const uint32_t stride = ti.max_len;
    if (n * stride > (uint64_t)8 * len + (1u << 20)) return 0;      /* ragged beyond reason, as the lanes rule (fxh_lanes.c) */
    uint32_t irr = 0;
    dev_grow(u, (void **)&u->d_bases, &u->d_bases_cap, (size_t)n * stride + 32);
    DEV_CHECK(u, fxg_fastq_pack(u->ctx, u->d_text, len, 2, u->d_line, cap_lines, u->d_flags, n, stride, 33, u->d_bases, NULL, &irr));      /* the alphabet check */
    if (irr) return 0;
    fxg_uncollapse_opts o = {u->base, 0, u->window};
    fxg_uncollapse_info info;
    do {
        const int s = u->slot;
        DEV_CHECK(u, fxg_fasta_uncollapse(u->ctx, u->d_text, ti.consumed, u->d_line, cap_lines, n, u->d_len, &o, u->d_out[s], &info));
        dev_drain(u);                                    /* the window before: its download ran beside this window's kernels */
        if (info.out_bytes) {
            DEV_CHECK_ON(u->down, fxg_memcpy_d2h(u->down, u->h_out[s], u->d_out[s], (size_t)info.out_bytes));
            u->pend = s; u->pend_bytes = (size_t)info.out_bytes;
            u->slot = s ^ 1;
        }
        o.copy_begin = info.copy_end;
    } while (info.copy_end < info.copies);
    u->base += info.copies;
    u->sequences += n;
    *used = (size_t)ti.consumed;
    return 1;
}

static void dev_open(upath *u, const struct fxh_reader *rd, struct fxh_writer *w)
{
    memset(u, 0, sizeof *u);
    u->w = w; u->pend = -1;
    int dev[FXH_MAX_LANES];
    (void)fxh_device_list(dev, FXH_MAX_LANES);
    const int rc = fxg_ctx_create(dev[0], &u->ctx);
    if (rc != FXG_OK) errx(1, "no usable GPU (device %d): the engine has no CPU fallback (fxg_ctx_create = %d)", dev[0], rc);
    if (fxg_ctx_create(dev[0], &u->down) != FXG_OK) errx(1, "a second context on device %d failed", dev[0]);
    u->window = rd->cap < FXH_UC_WINDOW_MIN ? FXH_UC_WINDOW_MIN : rd->cap > FXH_UC_BLOCK_MAX ? FXH_UC_BLOCK_MAX : rd->cap;
    for (int s = 0; s < 2; ++s) {
        DEV_CHECK(u, fxg_malloc_device(u->ctx, u->window + 64, (void **)&u->d_out[s]));
        DEV_CHECK(u, fxg_malloc_host(u->ctx, u->window, (void **)&u->h_out[s]));
    }
}

/* the last window is written; everything of the device path goes */
static void dev_close(upath *u)
{
    dev_drain(u);
    fxh_awriter_stop(&u->aw);
    for (int i = 0; i < u->npinned; ++i) (void)fxg_host_unregister(u->ctx, (void *)u->pinned[i]);
    for (int s = 0; s < 2; ++s) { (void)fxg_free_host(u->ctx, u->h_out[s]); (void)fxg_free_device(u->ctx, u->d_out[s]); }
    if (u->d_text) (void)fxg_free_device(u->ctx, u->d_text);
    if (u->d_line) (void)fxg_free_device(u->ctx, u->d_line);
    if (u->d_len) (void)fxg_free_device(u->ctx, u->d_len);
    if (u->d_flags) (void)fxg_free_device(u->ctx, u->d_flags);
    if (u->d_bases) (void)fxg_free_device(u->ctx, u->d_bases);
    fxg_ctx_destroy(u->down);
    fxg_ctx_destroy(u->ctx);
}

void fxh_uncollapse_run(FASTX *fx, fxh_totals *tot)
{
    size_t seqid = 1;
    memset(tot, 0, sizeof *tot);
    if (!fxg_fasta_uncollapse || getenv("FXH_HOST_PARSE")) {
        while (fastx_read_next_record(fx)) write_copies(fx, &seqid);
    } else {
        struct fxh_reader *rd = fx->reader;
        if (!fxh_read_buffer_bytes()) {
            struct stat sb;
            fxh_reader_reserve(rd, (size_t)(fstat(rd->fd, &sb) == 0 && S_ISFIFO(sb.st_mode) ? 16 : 64) << 20);
        }
        fxh_prefetch pf;
        memset(&pf, 0, sizeof pf);
        char *spare = NULL;
        upath u;
        dev_open(&u, rd, fx->writer);
        for (;;) {
            fxh_next_block(&pf, rd, &spare);
            char *p = rd->buf + rd->beg;
            size_t len = rd->end - rd->beg, used;
            const int eof = rd->eof;
            if (eof && len > 0 && p[len - 1] != '\n') { p[len++] = '\n'; rd->end++; }      /* (the reader's buffers hold cap + 1 bytes) */
            dev_pin(&u, rd);
            if (!dev_block(&u, p, len, eof, &used)) break;
            rd->beg += used;
            if (eof) break;
        }
        dev_close(&u);
        /* what is left -- nothing, after a regular input -- through the record API, its line numbers and the running number carried over */
        fx->input_line_number += 2 * u.sequences;
        seqid = (size_t)u.base + 1;
        while (next_record(fx, &pf, &spare)) write_copies(fx, &seqid);
        fxh_prefetch_stop(&pf);
        tot->input_sequences = (size_t)u.sequences;
        tot->input_reads = tot->output_sequences = tot->output_reads = (size_t)u.base;
    }
    tot->input_sequences += num_input_sequences(fx); tot->input_reads += num_input_reads(fx);
    tot->output_sequences += num_output_sequences(fx); tot->output_reads += num_output_reads(fx);
}
