/* fxh_nucchange.c -- fasta_nucleotide_changer's run.  The input is read in blocks through the prefetch of fxh_io.c.  Every block is indexed
 * (fxg_fastq_index), its bases lines are checked and rewritten in place by fxg_bases_change, and it goes out through the formatter as it is
 * (fxg_fastq_format with out_fasta = 1) into one of two device output buffers: a block is downloaded on a second context's stream and handed to
 * the writer thread while the next one is processed.  FASTQ blocks also go through fxg_fastq_pack, which checks their quality lines; its base
 * check knows no U, so in -d mode it comes after the change (which leaves A C G T N behind) and in -r mode before it (a U is the error case
 * there anyway).  FASTA blocks skip the pack: fxg_bases_change checks every bases byte against upper-case A C G T N U itself, and the one
 * letter of those that pack would refuse in -r mode, U, is that mode's offender.
 * The run stops at the first record that holds the mode's target letter, and its message carries the line number in the whole input, so the
 * blocks go through one context in input order: no lanes, no parts, no second GPU, no FXH_WORLD.  A block the device path does not take --
 * irregular in any way, without a whole record, ragged beyond reason -- ends the device path: the rest of the input goes through the record
 * API, which owns the reference's messages, from that block's first byte on, with the line number, the tallies and the change count carried
 * over.  A library without the entry runs the whole input that way: the reference's own loop over fastx.h.  See fxh_nucchange.h. */
#include "fxh_priv.h"
#include "fxh_nucchange.h"

/* the entry the device path needs; a library without it (the CPU tier's look-alike) leaves the reference null */
extern int fxg_bases_change(fxg_ctx *, uint8_t *, uint64_t, int, const uint32_t *, uint64_t, uint64_t, int, int, fxg_bases_change_info *) __attribute__((weak));

typedef struct { char from, to; const char *mode; } nmode;

/* ---- the record path ---- */
static void offender(const nmode *m, unsigned long long line)       /* fasta_nucleotide_changer.c:105-106 */
{
    errx(1, "Error: found '%c' nucleotide on line %lld. (input should not contain '%c' nucleotides in %s mode)", m->to, (long long)line, m->to, m->mode);
}

static void change_record(FASTX *fx, const nmode *m, size_t *changed)      /* fasta_nucleotide_changer.c:103-114 */
{
    for (char *p = fx->nucleotides; *p; ++p) {
        if (*p == m->to) offender(m, fx->input_line_number);       /* (exit() closes the writer: what was written before stays) */
        if (*p == m->from) { *p = m->to; ++*changed; }
    }
    fastx_write_record(fx);
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
    if (fx->read_fastq) {
        memcpy(fx->name2, rec.name2, rec.name2_len); fx->name2[rec.name2_len] = 0;
        fxh_decode_quality(fx, &rec, fx->quality, NULL);     /* (the reference's messages for a bad quality line) */
        fx->read_fastq_ascii = rec.is_ascii;
    }
    fx->num_input_sequences++;
    fx->num_input_reads += (size_t)get_reads_count(fx);
    return 1;
}

/* ---- the device path ---- */
typedef struct {
    fxg_ctx *ctx, *down;                                 /* the kernels' context; one whose stream only carries the downloads */
    uint8_t *d_text, *d_bases, *d_qual, *d_flags, *d_out[2]; uint32_t *d_line, *d_res; uint16_t *d_len;
    size_t d_text_cap, d_bases_cap, d_qual_cap, d_flags_cap, d_line_cap, d_res_cap, d_len_cap, d_out_cap[2];
    char *h_out[2]; size_t h_out_cap[2];
    void *h_res; size_t h_res_cap;                       /* the lengths, then the res[] made from them */
    int slot, pend; size_t pend_bytes;                   /* the buffers of the next block; the download in flight (-1: none) and its size */
    const void *pinned[8]; int npinned;
    int lpr, qoffset;
    uint64_t sequences, reads, changed;                  /* what the device path has written so far */
    unsigned long long offender_line;                    /* != 0: a record with the target letter ended the run at this input line */
    struct fxh_writer *w;
    fxh_awriter aw;
} npath;

#define DEV_CHECK_ON(c, call) do { if ((call) != FXG_OK) errx(1, "%s: %s", #call, fxg_last_error(c)); } while (0)
#define DEV_CHECK(u, call) DEV_CHECK_ON((u)->ctx, call)

static void dev_grow(npath *u, void **p, size_t *cap, size_t want)
{
    if (*cap >= want) return;
    if (*p) (void)fxg_free_device(u->ctx, *p);
    *p = NULL; *cap = 0;
    want += want / 8 + 4096;
    DEV_CHECK(u, fxg_malloc_device(u->ctx, want, p));
    *cap = want;
}

static void host_grow(npath *u, void **p, size_t *cap, size_t want)
{
    if (*cap >= want) return;
    if (*p) (void)fxg_free_host(u->ctx, *p);
    *p = NULL; *cap = 0;
    want += want / 8 + 4096;
    DEV_CHECK(u, fxg_malloc_host(u->ctx, want, p));
    *cap = want;
}

/* the reader's buffers are page-locked the first time a block comes out of them (a failure only makes the upload slower) */
static void dev_pin(npath *u, const struct fxh_reader *rd)
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
static void dev_drain(npath *u)
{
    if (u->pend < 0) return;
    DEV_CHECK_ON(u->down, fxg_sync(u->down));
    fxh_awriter_submit_ext(&u->aw, u->w, u->h_out[u->pend], u->pend_bytes);      /* (returns once the write before this one is done) */
    u->pend = -1;
}

/* One block: upload, index, check and change, format, download.  Returns 1 with *used = the bytes of its whole records (offender_line set when
 * the run ends inside it: the records before the offender are on their way out), or 0: the record path takes the input from this block on
 * (nothing of the block has been written). */
static int dev_block(npath *u, const nmode *m, const char *p, size_t len, int eof, size_t *used)
{
    *used = 0;
    if (len == 0) return 1;
    if (len > 0xFFFFFF00u) return 0;
    const int lpr = u->lpr;
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
    if (n * stride > (uint64_t)8 * len + (1u << 20)) return 0;      /* ragged beyond reason, as the lanes rule (fxh_lanes.c) */
    fxg_bases_change_info ci;
    uint32_t irr = 0;
    if (lpr == 4) {
        dev_grow(u, (void **)&u->d_bases, &u->d_bases_cap, (size_t)n * stride + 32);
        dev_grow(u, (void **)&u->d_qual, &u->d_qual_cap, (size_t)n * stride + 32);
    }
    if (lpr == 4 && m->from == 'T') {                    /* -r: the pack's base check first (it refuses a U, this mode's offender: the record path's to report) */
        DEV_CHECK(u, fxg_fastq_pack(u->ctx, u->d_text, len, lpr, u->d_line, cap_lines, u->d_flags, n, stride, u->qoffset, u->d_bases, u->d_qual, &irr));
        if (irr) return 0;
    }
    DEV_CHECK(u, fxg_bases_change(u->ctx, u->d_text, ti.consumed, lpr, u->d_line, cap_lines, n, m->from, m->to, &ci));
    if (ci.irregular) return 0;
    if (lpr == 4 && m->from == 'U') {                    /* -d: the pack sees the rewritten bases, A C G T N */
        DEV_CHECK(u, fxg_fastq_pack(u->ctx, u->d_text, len, lpr, u->d_line, cap_lines, u->d_flags, n, stride, u->qoffset, u->d_bases, u->d_qual, &irr));
        if (irr) return 0;
    }
    const uint64_t nout = ci.first_to_record < n ? ci.first_to_record : n;
    uint64_t out_bytes = 0;
    const int s = u->slot;
    if (nout) {
        /* every record is kept whole: a res[] from the indexed lengths, for the formatter and for the read-count tallies of FASTA ids */
        host_grow(u, &u->h_res, &u->h_res_cap, (size_t)nout * (sizeof(uint16_t) + sizeof(uint32_t)) + 2 * sizeof(uint32_t));
        uint16_t *l16 = (uint16_t *)u->h_res;
        uint32_t *res = (uint32_t *)(l16 + nout + (nout & 1u));
        dev_grow(u, (void **)&u->d_res, &u->d_res_cap, (size_t)nout * sizeof(uint32_t));
        DEV_CHECK(u, fxg_memcpy_d2h(u->ctx, l16, u->d_len, (size_t)nout * sizeof(uint16_t)));
        DEV_CHECK(u, fxg_sync(u->ctx));
        for (uint64_t i = 0; i < nout; ++i) res[i] = (1u << 16) | l16[i];
        DEV_CHECK(u, fxg_memcpy_h2d(u->ctx, u->d_res, res, (size_t)nout * sizeof(uint32_t)));
        uint64_t weighted[8] = {0};
        if (lpr == 2) DEV_CHECK(u, fxg_fasta_weights(u->ctx, u->d_text, u->d_line, cap_lines, nout, u->d_res, weighted));
        else weighted[0] = nout;
        dev_grow(u, (void **)&u->d_out[s], &u->d_out_cap[s], (size_t)ti.consumed + (size_t)n + 64);
        DEV_CHECK(u, fxg_fastq_format(u->ctx, u->d_text, lpr, u->d_line, cap_lines, u->d_flags, nout, u->d_res, 0, 0, NULL, NULL, NULL, lpr == 4 ? u->d_qual : NULL,
                                      stride, u->qoffset, 1, u->d_out[s], &out_bytes));
        u->reads += weighted[0];
    }
    dev_drain(u);                                        /* the block before: its download ran beside this block's kernels */
    if (out_bytes) {
        host_grow(u, (void **)&u->h_out[s], &u->h_out_cap[s], (size_t)out_bytes);
        DEV_CHECK_ON(u->down, fxg_memcpy_d2h(u->down, u->h_out[s], u->d_out[s], (size_t)out_bytes));
        u->pend = s; u->pend_bytes = (size_t)out_bytes;
        u->slot = s ^ 1;
    }
    if (nout < n) u->offender_line = (unsigned long long)lpr * (u->sequences + nout + 1);       /* input_line_number after that record was read */
    else u->changed += ci.changed;
    u->sequences += nout;
    *used = (size_t)ti.consumed;
    return 1;
}

static void dev_open(npath *u, FASTX *fx)
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
}

/* the last block is written; everything of the device path goes */
static void dev_close(npath *u)
{
    dev_drain(u);
    fxh_awriter_stop(&u->aw);
    for (int i = 0; i < u->npinned; ++i) (void)fxg_host_unregister(u->ctx, (void *)u->pinned[i]);
    for (int s = 0; s < 2; ++s) {
        if (u->h_out[s]) (void)fxg_free_host(u->ctx, u->h_out[s]);
        if (u->d_out[s]) (void)fxg_free_device(u->ctx, u->d_out[s]);
    }
    if (u->h_res) (void)fxg_free_host(u->ctx, u->h_res);
    if (u->d_text) (void)fxg_free_device(u->ctx, u->d_text);
    if (u->d_line) (void)fxg_free_device(u->ctx, u->d_line);
    if (u->d_len) (void)fxg_free_device(u->ctx, u->d_len);
    if (u->d_flags) (void)fxg_free_device(u->ctx, u->d_flags);
    if (u->d_bases) (void)fxg_free_device(u->ctx, u->d_bases);
    if (u->d_qual) (void)fxg_free_device(u->ctx, u->d_qual);
    if (u->d_res) (void)fxg_free_device(u->ctx, u->d_res);
    fxg_ctx_destroy(u->down);
    fxg_ctx_destroy(u->ctx);
}

void fxh_nucchange_run(FASTX *fx, int rna_to_dna, fxh_totals *tot, size_t *changed)
{
    const nmode m = {rna_to_dna ? 'U' : 'T', rna_to_dna ? 'T' : 'U', rna_to_dna ? "RNA-to-DNA" : "DNA-to-RNA"};
    memset(tot, 0, sizeof *tot);
    *changed = 0;
    if (!fxg_bases_change || getenv("FXH_HOST_PARSE")) {
        while (fastx_read_next_record(fx)) change_record(fx, &m, changed);
    } else {
        struct fxh_reader *rd = fx->reader;
        if (!fxh_read_buffer_bytes()) {
            struct stat sb;
            fxh_reader_reserve(rd, (size_t)(fstat(rd->fd, &sb) == 0 && S_ISFIFO(sb.st_mode) ? 16 : 64) << 20);
        }
        fxh_prefetch pf;
        memset(&pf, 0, sizeof pf);
        char *spare = NULL;
        npath u;
        dev_open(&u, fx);
        for (;;) {
            fxh_next_block(&pf, rd, &spare);
            char *p = rd->buf + rd->beg;
            size_t len = rd->end - rd->beg, used;
            const int eof = rd->eof;
            if (eof && len > 0 && p[len - 1] != '\n') { p[len++] = '\n'; rd->end++; }      /* (the reader's buffers hold cap + 1 bytes) */
            dev_pin(&u, rd);
            if (!dev_block(&u, &m, p, len, eof, &used)) break;
            rd->beg += used;
            if (eof || u.offender_line) break;
        }
        const unsigned long long line = u.offender_line;
        const uint64_t sequences = u.sequences, reads = u.reads, dev_changed = u.changed;
        dev_close(&u);
        if (line) {                                      /* the records before the offender are written: finish the output (-z: a whole gzip stream), then the reference's end */
            fxh_prefetch_stop(&pf);
            fastx_finish(fx);
            offender(&m, line);
        }
        /* what is left -- nothing, after a regular input -- through the record API, its line numbers and the change count carried over */
        fx->input_line_number += (unsigned long long)u.lpr * sequences;
        *changed = (size_t)dev_changed;
        while (next_record(fx, &pf, &spare)) change_record(fx, &m, changed);
        fxh_prefetch_stop(&pf);
        tot->input_sequences = tot->output_sequences = (size_t)sequences;
        tot->input_reads = tot->output_reads = (size_t)reads;
    }
    tot->input_sequences += num_input_sequences(fx); tot->input_reads += num_input_reads(fx);
    tot->output_sequences += num_output_sequences(fx); tot->output_reads += num_output_reads(fx);
}
