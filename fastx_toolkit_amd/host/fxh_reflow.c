/* fxh_reflow.c -- fasta_formatter's run.  The input is read in blocks through the prefetch of fxh_io.c; every block goes through
 * fxg_fasta_reflow on one context, in input order (the carry from block to block is serial), and the writer thread appends the blocks'
 * outputs in order.  A block's output comes back on a second context's stream while the next block is uploaded and reflowed; the upload
 * itself is not overlapped: where a block starts is only known once the block before it says how much it consumed.  An input whose first non-empty line is not a header line -- or that is empty, or a library without the entry --
 * takes the host path instead: a plain loop that restates the reference's loop and its writers and owns their corners (sequence lines
 * before the first header, no header at all, the tabular writer's abort).  See fxh_reflow.h. */
#include "fxh_priv.h"
#include "fxh_reflow.h"

/* the entry the device path needs; a library without it (the CPU tier's look-alike) leaves the reference null */
extern int fxg_fasta_reflow(fxg_ctx *, const uint8_t *, uint64_t, int, uint64_t, const fxg_reflow_opts *, uint32_t *, uint64_t, uint8_t *, fxg_reflow_info *)
    __attribute__((weak));

#define FXH_REFLOW_BLOCK_MAX ((size_t)0xFFFFFFF0u)      /* the device's line index holds 32-bit offsets: a block, and so a line, ends below this */

static void put(struct fxh_writer *w, const char *p, size_t n)
{
    while (n > 0) {                                      /* (pieces: a record may be larger than the writer's buffer should ever become) */
        const size_t k = n < ((size_t)4 << 20) ? n : ((size_t)4 << 20);
        memcpy(fxh_writer_reserve(w, k), p, k);
        w->len += k;
        p += k; n -= k;
    }
}

/* ---- the host path ---- */
typedef struct { char *p; size_t n, cap; } hbuf;
static void hbuf_add(hbuf *b, const char *p, size_t n)
{
    if (b->n + n > b->cap) {
        b->cap = (b->n + n) * 2 + 4096;
        b->p = (char *)realloc(b->p, b->cap);
        if (!b->p) err(1, "out of memory");
    }
    memcpy(b->p + b->n, p, n);
    b->n += n;
}

typedef struct {
    const fxh_reflow_opts *o;
    struct fxh_writer *w;
    hbuf id, bases, part;                                /* the open record; a line that the block's end cut */
    int first, failed;
} hpath;

/* one record through the writer the options pick (sequence_writers.h:31-109) */
static void hp_write(hpath *h)
{
    const fxh_reflow_opts *o = h->o;
    if (h->bases.n == 0 && !o->keep_empty) return;
    if (o->tabular) {
        if (h->id.n == 0) { h->failed = 1; return; }     /* the reference takes substr(1) of an empty id here and aborts */
        put(h->w, h->id.p + 1, h->id.n - 1);
        if (h->bases.n) { put(h->w, "\t", 1); put(h->w, h->bases.p, h->bases.n); }
        put(h->w, "\n", 1);
        return;
    }
    put(h->w, h->id.p, h->id.n);
    put(h->w, "\n", 1);
    if (h->bases.n == 0) return;
    if (o->width == 0) { put(h->w, h->bases.p, h->bases.n); put(h->w, "\n", 1); return; }
    for (size_t s = 0; s < h->bases.n; s += o->width) {
        const size_t k = h->bases.n - s < o->width ? h->bases.n - s : o->width;
        put(h->w, h->bases.p + s, k);
        put(h->w, "\n", 1);
    }
}

static void hp_line(hpath *h, const char *p, size_t n)   /* fasta_formatter.cpp:172-194 */
{
    if (n == 0) return;
    if (p[0] == '>') {
        if (h->first) h->first = 0; else hp_write(h);
        h->id.n = 0; hbuf_add(&h->id, p, n);
        h->bases.n = 0;
    } else hbuf_add(&h->bases, p, n);
}

static void hp_feed(hpath *h, const char *p, size_t n)
{
    while (n > 0) {
        const char *e = (const char *)memchr(p, '\n', n);
        if (!e) { hbuf_add(&h->part, p, n); return; }
        const size_t k = (size_t)(e - p);
        if (h->part.n) { hbuf_add(&h->part, p, k); hp_line(h, h->part.p, h->part.n); h->part.n = 0; }
        else hp_line(h, p, k);
        p += k + 1; n -= k + 1;
    }
}

static int run_host(const fxh_reflow_opts *o, struct fxh_reader *rd, fxh_prefetch *pf, char **spare, struct fxh_writer *w)
{
    hpath h;
    memset(&h, 0, sizeof h);
    h.o = o; h.w = w; h.first = 1;
    for (;;) {
        hp_feed(&h, rd->buf + rd->beg, rd->end - rd->beg);
        rd->beg = rd->end;
        if (rd->eof) break;
        fxh_next_block(pf, rd, spare);
    }
    if (h.part.n) hp_line(&h, h.part.p, h.part.n);       /* a last line without '\n' is still a line */
    hp_write(&h);
    free(h.id.p); free(h.bases.p); free(h.part.p);
    if (h.failed) {
        fxh_writer_flush(w);
        fprintf(stderr, "fasta_formatter: tabular output [-t] needs a sequence identifier, and the input has no '>' line\n");
        return 1;
    }
    return 0;
}

/* ---- the device path ---- */
typedef struct {
    fxg_ctx *ctx, *down;                                 /* the kernels' context; one whose stream only carries the downloads */
    fxg_reflow_opts opts;
    uint8_t *d_text, *d_out[2]; uint32_t *d_line;
    size_t d_text_cap, d_out_cap[2], d_line_cap;
    char *h_out[2]; size_t h_out_cap[2];
    int pend; size_t pend_bytes;                         /* the download in flight: its buffers' index (-1: none) and size */
    const void *pinned[8]; int npinned;
    uint64_t carry, blocks;
    struct fxh_writer *w;
    fxh_awriter aw;
} dpath;

#define DEV_CHECK_ON(c, call) do { if ((call) != FXG_OK) errx(1, "%s: %s", #call, fxg_last_error(c)); } while (0)
#define DEV_CHECK(d, call) DEV_CHECK_ON((d)->ctx, call)

static void dev_grow(dpath *d, void **p, size_t *cap, size_t want)
{
    if (*cap >= want) return;
    if (*p) (void)fxg_free_device(d->ctx, *p);
    *p = NULL; *cap = 0;
    want += want / 8 + 4096;
    DEV_CHECK(d, fxg_malloc_device(d->ctx, want, p));
    *cap = want;
}

/* the reader's buffers are page-locked the first time a block comes out of them (a failure only makes the upload slower) */
static void dev_pin(dpath *d, const struct fxh_reader *rd)
{
    for (int i = 0; i < d->npinned; ++i) if (d->pinned[i] == rd->buf) return;
    if (d->npinned == (int)(sizeof d->pinned / sizeof d->pinned[0])) return;
    d->pinned[d->npinned++] = rd->buf;
    (void)fxg_host_register(d->ctx, rd->buf, rd->cap + 1);
}

static size_t count_nl(const char *p, size_t n)
{
    size_t c = 0;
    const char *e = p + n;
    while (p < e && (p = (const char *)memchr(p, '\n', (size_t)(e - p))) != NULL) { ++c; ++p; }
    return c;
}

/* the download in flight: wait for it and hand it to the writer thread */
static void dev_drain(dpath *d)
{
    if (d->pend < 0) return;
    DEV_CHECK_ON(d->down, fxg_sync(d->down));
    fxh_awriter_submit_ext(&d->aw, d->w, d->h_out[d->pend], d->pend_bytes);      /* (returns once the write before this one is done) */
    d->pend = -1;
}

/* one block: upload, reflow, then the block before it to the writer and this one's output on its way back; returns the bytes consumed */
static size_t dev_block(dpath *d, const char *p, size_t len, int eof)
{
    const size_t cap_lines = count_nl(p, len) + 1;
    const int s = (int)(d->blocks & 1u);                 /* the other pair of output buffers may still be on its way to the file */
    fxg_reflow_info info;
    dev_grow(d, (void **)&d->d_text, &d->d_text_cap, len + 64);
    dev_grow(d, (void **)&d->d_line, &d->d_line_cap, 2 * cap_lines * sizeof(uint32_t));
    dev_grow(d, (void **)&d->d_out[s], &d->d_out_cap[s], 2 * len + 2 + 64);
    if (len) DEV_CHECK(d, fxg_memcpy_h2d(d->ctx, d->d_text, p, len));
    d->opts.out_cap = 2 * (uint64_t)len + 2;
    DEV_CHECK(d, fxg_fasta_reflow(d->ctx, d->d_text, len, eof, d->carry, &d->opts, d->d_line, cap_lines, d->d_out[s], &info));
    d->carry = info.open_bases;
    dev_drain(d);                                        /* the block before: its download ran beside this block's upload and kernels */
    if (info.out_bytes) {
        if (d->h_out_cap[s] < info.out_bytes) {
            if (d->h_out[s]) (void)fxg_free_host(d->ctx, d->h_out[s]);
            d->h_out_cap[s] = (size_t)info.out_bytes + (size_t)info.out_bytes / 8 + 4096;
            DEV_CHECK(d, fxg_malloc_host(d->ctx, d->h_out_cap[s], (void **)&d->h_out[s]));
        }
        DEV_CHECK_ON(d->down, fxg_memcpy_d2h(d->down, d->h_out[s], d->d_out[s], (size_t)info.out_bytes));
        d->pend = s; d->pend_bytes = (size_t)info.out_bytes;
        d->blocks++;
    }
    return (size_t)info.consumed;
}

/* A block from which nothing could be consumed, with more of it unread than the prefetch carries over: a line longer than the block.  The
 * rest of the run reads into one buffer of its own that doubles until the line fits, up to the limit of the device's line index. */
static void run_device_grow(dpath *d, struct fxh_reader *rd, fxh_prefetch *pf)
{
    fxh_prefetch_stop(pf);                               /* (the input has not ended, so a request is in flight: it is finished first) */
    pf->started = 0;
    size_t n = rd->end - rd->beg, cap = 2 * rd->cap;
    const size_t ahead = pf->filled;
    int eof = pf->eof;
    while (cap < n + ahead + 1) cap *= 2;
    if (cap > FXH_REFLOW_BLOCK_MAX) cap = FXH_REFLOW_BLOCK_MAX;
    char *buf = (char *)malloc(cap + 1);
    if (!buf) err(1, "out of memory");
    memcpy(buf, rd->buf + rd->beg, n);
    if (ahead) { memcpy(buf + n, pf->buf + pf->gap, ahead); n += ahead; }
    rd->beg = rd->end;
    for (;;) {
        while (!eof && n < cap) {
            const ssize_t k = pf->regular ? pread(pf->fd, buf + n, cap - n, pf->offset) : read(pf->fd, buf + n, cap - n);
            if (k < 0) { if (errno == EINTR) continue; err(1, "read failed"); }
            if (k == 0) { eof = 1; break; }
            if (pf->regular) pf->offset += k;
            n += (size_t)k;
        }
        if (eof && n > 0 && buf[n - 1] != '\n') buf[n++] = '\n';
        const size_t used = dev_block(d, buf, n, eof);
        if (eof) break;
        if (used == 0) {
            if (cap >= FXH_REFLOW_BLOCK_MAX) errx(1, "a line of the input is longer than %zu bytes: the device's line index holds 32-bit offsets", FXH_REFLOW_BLOCK_MAX);
            cap = cap * 2 > FXH_REFLOW_BLOCK_MAX ? FXH_REFLOW_BLOCK_MAX : cap * 2;
            buf = (char *)realloc(buf, cap + 1);
            if (!buf) err(1, "out of memory");
            continue;
        }
        memmove(buf, buf + used, n - used);
        n -= used;
    }
    dev_drain(d);
    free(buf);
}

static int run_device(const fxh_reflow_opts *o, struct fxh_reader *rd, fxh_prefetch *pf, char **spare, struct fxh_writer *w)
{
    dpath d;
    memset(&d, 0, sizeof d);
    d.w = w;
    d.opts.width = o->width; d.opts.tabular = o->tabular ? 1u : 0u; d.opts.keep_empty = o->keep_empty ? 1u : 0u;
    int dev[FXH_MAX_LANES];
    (void)fxh_device_list(dev, FXH_MAX_LANES);
    const int rc = fxg_ctx_create(dev[0], &d.ctx);
    if (rc != FXG_OK) errx(1, "no usable GPU (device %d): the engine has no CPU fallback (fxg_ctx_create = %d)", dev[0], rc);
    if (fxg_ctx_create(dev[0], &d.down) != FXG_OK) errx(1, "a second context on device %d failed", dev[0]);
    d.pend = -1;
    for (;;) {
        char *p = rd->buf + rd->beg;
        size_t len = rd->end - rd->beg;
        const int eof = rd->eof;
        if (eof && len > 0 && p[len - 1] != '\n') p[len++] = '\n';      /* (the reader's buffers hold cap + 1 bytes) */
        if (len > FXH_REFLOW_BLOCK_MAX) errx(1, "a block of %zu bytes: FXH_READ_BUFFER_MB is too large for the device's 32-bit line index", len);
        dev_pin(&d, rd);
        const size_t used = dev_block(&d, p, len, eof);
        if (eof) break;
        rd->beg += used;
        if (rd->end - rd->beg > pf->gap) { run_device_grow(&d, rd, pf); break; }
        fxh_next_block(pf, rd, spare);
    }
    dev_drain(&d);
    fxh_awriter_stop(&d.aw);
    for (int i = 0; i < d.npinned; ++i) (void)fxg_host_unregister(d.ctx, (void *)d.pinned[i]);
    for (int s = 0; s < 2; ++s) if (d.h_out[s]) (void)fxg_free_host(d.ctx, d.h_out[s]);
    if (d.d_text) (void)fxg_free_device(d.ctx, d.d_text);
    if (d.d_line) (void)fxg_free_device(d.ctx, d.d_line);
    for (int s = 0; s < 2; ++s) if (d.d_out[s]) (void)fxg_free_device(d.ctx, d.d_out[s]);
    fxg_ctx_destroy(d.down);
    fxg_ctx_destroy(d.ctx);
    return 0;
}

int fxh_reflow_run(const fxh_reflow_opts *o)
{
    size_t cap = (size_t)64 << 20;
    struct fxh_reader *rd = fxh_reader_open(o->in ? o->in : "-", cap);
    {
        struct stat sb;
        if (fstat(rd->fd, &sb) == 0 && S_ISFIFO(sb.st_mode)) cap = (size_t)16 << 20;
        if (fxh_read_buffer_bytes()) cap = fxh_read_buffer_bytes();
        if (cap != rd->cap) { free(rd->buf); rd->cap = cap; rd->buf = (char *)malloc(cap + 1); if (!rd->buf) err(1, "out of memory"); }
    }
    struct fxh_writer *w = fxh_writer_open_file(o->out ? o->out : "-", 0);
    fxh_prefetch pf;
    memset(&pf, 0, sizeof pf);
    char *spare = NULL;
    fxh_next_block(&pf, rd, &spare);
    for (;;) {                                             /* the first non-empty line decides */
        while (rd->beg < rd->end && rd->buf[rd->beg] == '\n') ++rd->beg;
        if (rd->beg < rd->end || rd->eof) break;
        fxh_next_block(&pf, rd, &spare);
    }
    const int host = rd->beg == rd->end || rd->buf[rd->beg] != '>' || !fxg_fasta_reflow;
    const int rc = host ? run_host(o, rd, &pf, &spare, w) : run_device(o, rd, &pf, &spare, w);
    fxh_prefetch_stop(&pf);
    fxh_writer_close(w);
    return rc;
}
