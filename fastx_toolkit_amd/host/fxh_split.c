/* fxh_split.c -- fastx_barcode_splitter's run: barcode table, format sniff, blocks of stdin cut at record boundaries, lanes (one context and
 * one thread each) that index and split a block on the device, and an ordered writer that appends every block's K + 1 slices to their files.
 * Behaviour: the reference's scripts/fastx_barcode_splitter.pl; see fxh_split.h. */
#include "fxh_priv.h"
#include "fxh_split.h"

#include <stdarg.h>

/* ---- messages ---- */
typedef struct { char *p; size_t n, cap; } fxh_sb;

static void sb_add(fxh_sb *s, const void *p, size_t n)
{
    if (s->n + n + 1 > s->cap) {
        s->cap = (s->n + n + 1) * 2;
        s->p = (char *)realloc(s->p, s->cap);
        if (!s->p) err(1, "out of memory");
    }
    memcpy(s->p + s->n, p, n);
    s->n += n;
}
static void sb_str(fxh_sb *s, const char *z) { sb_add(s, z, strlen(z)); }
static void sb_fmt(fxh_sb *s, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
static void sb_fmt(fxh_sb *s, const char *fmt, ...)
{
    char tmp[512];
    va_list ap;
    va_start(ap, fmt);
    const int k = vsnprintf(tmp, sizeof tmp, fmt, ap);
    va_end(ap);
    sb_add(s, tmp, k < 0 ? 0 : ((size_t)k < sizeof tmp ? (size_t)k : sizeof tmp - 1));
}
static void __attribute__((noreturn)) sb_die(fxh_sb *s)
{
    sb_add(s, "\n", 1);
    fflush(stdout);
    (void)!write(STDERR_FILENO, s->p, s->n);
    exit(255);
}

void fxh_split_die(const char *fmt, ...)
{
    char tmp[4096];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(tmp, sizeof tmp, fmt, ap);
    va_end(ap);
    fxh_sb s = {0};
    sb_str(&s, tmp);
    sb_die(&s);
}

/* ---- the barcode table ---- */
typedef struct {
    uint8_t *bases;             /* entries x FXG_MAX_BARCODE */
    uint32_t *len, *bin;
    uint32_t entries, cap, BL;
    char **name;                /* bins; the last is "unmatched" */
    uint32_t nbins, name_cap;
} fxh_table;

static int is_ws(int c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }
static int is_word(int c) { return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '_'; }

static uint32_t table_bin(fxh_table *t, const char *id, size_t n)
{
    for (uint32_t b = 0; b < t->nbins; ++b)
        if (strlen(t->name[b]) == n && memcmp(t->name[b], id, n) == 0) return b;
    if (t->nbins == t->name_cap) {
        t->name_cap = t->name_cap ? 2 * t->name_cap : 64;
        t->name = (char **)realloc(t->name, t->name_cap * sizeof(char *));
        if (!t->name) err(1, "out of memory");
    }
    t->name[t->nbins] = strndup(id, n);
    if (!t->name[t->nbins]) err(1, "out of memory");
    return t->nbins++;
}

static void table_push(fxh_table *t, const char *bases, uint32_t n, uint32_t bin)
{
    if (t->entries == t->cap) {
        t->cap = t->cap ? 2 * t->cap : 64;
        t->bases = (uint8_t *)realloc(t->bases, (size_t)t->cap * FXG_MAX_BARCODE);
        t->len = (uint32_t *)realloc(t->len, t->cap * sizeof(uint32_t));
        t->bin = (uint32_t *)realloc(t->bin, t->cap * sizeof(uint32_t));
        if (!t->bases || !t->len || !t->bin) err(1, "out of memory");
    }
    memset(t->bases + (size_t)t->entries * FXG_MAX_BARCODE, 0, FXG_MAX_BARCODE);
    memcpy(t->bases + (size_t)t->entries * FXG_MAX_BARCODE, bases, n);
    t->len[t->entries] = n;
    t->bin[t->entries] = bin;
    ++t->entries;
}

/* The script's loader: '#' lines skipped, the rest split on whitespace into identifier and barcode (upper-cased), checked in its order with its
 * messages; --partial adds the shortened entries behind each barcode.  Bins: identifiers in order of first appearance, `unmatched` last. */
static void table_load(fxh_table *t, const fxh_split_opts *o)
{
    FILE *f = fopen(o->bcfile, "rb");
    if (!f) fxh_split_die("Error: failed to open barcode file (%s)", o->bcfile);
    fxh_sb all = {0};
    char chunk[65536];
    size_t k;
    while ((k = fread(chunk, 1, sizeof chunk, f)) > 0) sb_add(&all, chunk, k);
    fclose(f);
    memset(t, 0, sizeof *t);
    char *longest = NULL;                   /* bases of the first barcode over FXG_MAX_BARCODE (reported after the script's own checks) */
    size_t pos = 0;
    long line = 0;
    uint32_t BL = 0;
    while (pos < all.n) {
        const char *ln = all.p + pos;
        const char *e = (const char *)memchr(ln, '\n', all.n - pos);
        const size_t L = e ? (size_t)(e - ln) : all.n - pos;
        pos += L + (e ? 1 : 0);
        ++line;
        if (L > 0 && ln[0] == '#') continue;
        size_t i = 0;
        while (i < L && is_ws((unsigned char)ln[i])) ++i;
        const size_t i0 = i;
        while (i < L && !is_ws((unsigned char)ln[i])) ++i;
        const size_t i1 = i;
        while (i < L && is_ws((unsigned char)ln[i])) ++i;
        const size_t b0 = i;
        while (i < L && !is_ws((unsigned char)ln[i])) ++i;
        const size_t b1 = i;
        char *bc = (char *)malloc(b1 - b0 + 1);
        if (!bc) err(1, "out of memory");
        for (size_t j = b0; j < b1; ++j) { const char c = ln[j]; bc[j - b0] = (c >= 'a' && c <= 'z') ? (char)(c - 32) : c; }
        const size_t n = b1 - b0;
        int ok = n > 0;
        for (size_t j = 0; j < n; ++j) ok &= bc[j] == 'A' || bc[j] == 'C' || bc[j] == 'G' || bc[j] == 'T';
        if (!ok) {
            fxh_sb s = {0};
            sb_str(&s, "Error: bad barcode value ("); sb_add(&s, bc, n); sb_str(&s, ") at barcode file ("); sb_str(&s, o->bcfile);
            sb_fmt(&s, ") line %ld", line);
            sb_die(&s);
        }
        int word = i1 > i0;
        for (size_t j = i0; j < i1; ++j) word &= is_word((unsigned char)ln[j]);
        if (!word) {
            fxh_sb s = {0};
            sb_str(&s, "Error: bad identifier value ("); sb_add(&s, ln + i0, i1 - i0); sb_str(&s, ") at barcode file ("); sb_str(&s, o->bcfile);
            sb_fmt(&s, ") line %ld (must be alphanumeric)", line);
            sb_die(&s);
        }
        if ((long)n <= (long)o->mismatches) {
            fxh_sb s = {0};
            sb_str(&s, "Error: badcode("); sb_add(&s, ln + i0, i1 - i0); sb_str(&s, ", "); sb_add(&s, bc, n);
            sb_fmt(&s, ") is shorter or equal to maximum number of mismatches (%d). This makes no sense. Specify fewer  mismatches.", o->mismatches);
            sb_die(&s);
        }
        if (BL == 0) BL = (uint32_t)n;
        if (n != BL) fxh_split_die("Error: found barcodes in different lengths. this feature is not supported yet.");
        if (n > FXG_MAX_BARCODE) { if (!longest) longest = strndup(bc, n); free(bc); continue; }
        const uint32_t bin = (i1 - i0 == 9 && memcmp(ln + i0, "unmatched", 9) == 0) ? UINT32_MAX : table_bin(t, ln + i0, i1 - i0);
        table_push(t, bc, (uint32_t)n, bin);
        for (int p = 1; p <= o->partial; ++p) table_push(t, o->eol ? bc : bc + p, (uint32_t)n - (uint32_t)p, bin);
        free(bc);
    }
    free(all.p);
    if (longest) fxh_split_die("Error: barcode %s is longer than %d bases (not supported)", longest, FXG_MAX_BARCODE);
    const uint32_t un = table_bin(t, "unmatched", 9);      /* the last bin */
    if (t->nbins > FXG_MAX_BARCODE_BINS) fxh_split_die("Error: %u barcode identifiers besides 'unmatched' (at most %d are supported)", t->nbins - 1, FXG_MAX_BARCODE_BINS - 1);
    for (uint32_t e = 0; e < t->entries; ++e) if (t->bin[e] == UINT32_MAX) t->bin[e] = un;
    t->BL = BL;
    if (o->debug) {
        fxh_sb s = {0};
        sb_str(&s, "barcode\tsequence\n");
        for (uint32_t e = 0; e < t->entries; ++e) {
            sb_str(&s, t->name[t->bin[e]]); sb_add(&s, "\t", 1); sb_add(&s, t->bases + (size_t)e * FXG_MAX_BARCODE, t->len[e]); sb_add(&s, "\n", 1);
        }
        (void)!write(STDERR_FILENO, s.p, s.n);
        free(s.p);
    }
}

/* ---- lanes and the ordered writer ---- */
enum { L_IDLE, L_QUEUED, L_DONE };

typedef struct fxh_split_lane {
    pthread_t th;
    int id, device, state;
    fxg_ctx *ctx;
    /* the block: host copy (page-locked), its records, where it goes */
    char *in; size_t in_cap, len, recs;
    uint64_t block;
    int want_bins;                         /* copy every record's bin back (--debug), or only the last one's */
    int drop_last;                         /* the block ends the input, whose last FASTQ quality line had no '\n': its record is written without it */
    char *out;
    uint16_t *rec_bin; size_t rb_cap;
    uint64_t *bin_bytes, *bin_records;
    /* device */
    uint8_t *d_text, *d_out, *d_flags; uint32_t *d_line; uint16_t *d_len, *d_rec_bin;
    size_t d_text_cap, d_out_cap, d_line_cap, d_len_cap, d_flags_cap, d_rb_cap;
    char errmsg[640];
} fxh_split_lane;

typedef struct {
    pthread_mutex_t mu;
    pthread_cond_t cv;
    fxh_split_lane *lane;
    int nlanes, quit;
    uint64_t blocks;                       /* submitted so far */
    int finished;                          /* no more blocks */
    int lpr, debug;
    const fxh_table *t;
    /* writer */
    int *fd;
    char **wbuf; size_t *wlen;
    uint64_t *counts;
} fxh_split_run_t;

#define FXH_SPLIT_WBUF ((size_t)256 << 10)   /* slices below this size are gathered per file before they are written */

static void write_all(int fd, const char *p, size_t n)
{
    while (n > 0) {
        const ssize_t k = write(fd, p, n);
        if (k < 0) { if (errno == EINTR) continue; err(1, "write failed"); }
        p += k; n -= (size_t)k;
    }
}

static void out_append(fxh_split_run_t *R, uint32_t b, const char *p, size_t n)
{
    if (n == 0) return;
    if (R->wlen[b] + n > FXH_SPLIT_WBUF) { write_all(R->fd[b], R->wbuf[b], R->wlen[b]); R->wlen[b] = 0; }
    if (n >= FXH_SPLIT_WBUF) { write_all(R->fd[b], p, n); return; }
    if (!R->wbuf[b] && !(R->wbuf[b] = (char *)malloc(FXH_SPLIT_WBUF))) err(1, "out of memory");
    memcpy(R->wbuf[b] + R->wlen[b], p, n);
    R->wlen[b] += n;
}

#define LANE_CHECK(ln, call)                                                                                                          \
    do {                                                                                                                              \
        if ((call) != FXG_OK) {                                                                                                       \
            snprintf((ln)->errmsg, sizeof (ln)->errmsg, "%s: %s", #call, fxg_last_error((ln)->ctx));                                \
            return -1;                                                                                                                \
        }                                                                                                                             \
    } while (0)

static int grow_device(fxh_split_lane *ln, void **p, size_t *cap, size_t want)
{
    if (*cap >= want) return 0;
    if (*p) (void)fxg_free_device(ln->ctx, *p);
    *p = NULL; *cap = 0;
    want += want / 8 + 4096;
    LANE_CHECK(ln, fxg_malloc_device(ln->ctx, want, p));
    *cap = want;
    return 0;
}

/* one block on the lane's device: upload, line index, split, the slices back */
static int lane_block(fxh_split_run_t *R, fxh_split_lane *ln)
{
    const size_t len = ln->len, recs = ln->recs, lines = recs * (size_t)R->lpr;
    const size_t cap_lines = lines + 2, per = cap_lines / (size_t)R->lpr + 1;
    if (grow_device(ln, (void **)&ln->d_text, &ln->d_text_cap, len + 64) || grow_device(ln, (void **)&ln->d_out, &ln->d_out_cap, len + 64) ||
        grow_device(ln, (void **)&ln->d_line, &ln->d_line_cap, 2 * cap_lines * sizeof(uint32_t)) ||
        grow_device(ln, (void **)&ln->d_len, &ln->d_len_cap, per * sizeof(uint16_t)) || grow_device(ln, (void **)&ln->d_flags, &ln->d_flags_cap, per) ||
        grow_device(ln, (void **)&ln->d_rec_bin, &ln->d_rb_cap, per * sizeof(uint16_t)))
        return -1;
    LANE_CHECK(ln, fxg_memcpy_h2d(ln->ctx, ln->d_text, ln->in, len));
    fxg_text_info info;
    LANE_CHECK(ln, fxg_fastq_index(ln->ctx, ln->d_text, len, 1, R->lpr, ln->d_line, cap_lines, ln->d_len, ln->d_flags, &info));
    if (info.records != recs) {
        snprintf(ln->errmsg, sizeof ln->errmsg, "block %llu: the device found %llu records, the host %zu", (unsigned long long)ln->block,
                 (unsigned long long)info.records, recs);
        return -1;
    }
    LANE_CHECK(ln, fxg_barcode_split(ln->ctx, ln->d_text, len, R->lpr, ln->d_line, cap_lines, recs, ln->d_rec_bin, ln->d_out, ln->bin_bytes,
                                     ln->bin_records));
    LANE_CHECK(ln, fxg_memcpy_d2h(ln->ctx, ln->out, ln->d_out, len));
    if (ln->want_bins) LANE_CHECK(ln, fxg_memcpy_d2h(ln->ctx, ln->rec_bin, ln->d_rec_bin, recs * sizeof(uint16_t)));
    else LANE_CHECK(ln, fxg_memcpy_d2h(ln->ctx, ln->rec_bin, ln->d_rec_bin + (recs - 1), sizeof(uint16_t)));
    LANE_CHECK(ln, fxg_sync(ln->ctx));
    return 0;
}

typedef struct { fxh_split_run_t *R; fxh_split_lane *ln; } lane_arg;

static void *lane_thread(void *arg)
{
    fxh_split_run_t *R = ((lane_arg *)arg)->R;
    fxh_split_lane *ln = ((lane_arg *)arg)->ln;
    free(arg);
    for (;;) {
        pthread_mutex_lock(&R->mu);
        while (ln->state != L_QUEUED && !R->quit) pthread_cond_wait(&R->cv, &R->mu);
        const int quit = ln->state != L_QUEUED;
        pthread_mutex_unlock(&R->mu);
        if (quit) break;
        if (lane_block(R, ln) != 0) {
            fflush(stdout);
            fprintf(stderr, "fastx_barcode_splitter: GPU %d: %s\n", ln->device, ln->errmsg);
            exit(1);
        }
        pthread_mutex_lock(&R->mu);
        ln->state = L_DONE;
        pthread_cond_broadcast(&R->cv);
        pthread_mutex_unlock(&R->mu);
    }
    return NULL;
}

/* --debug: the script's two lines per record, from the block's text and the records' bins */
static void debug_block(const fxh_split_run_t *R, const fxh_split_lane *ln)
{
    fxh_sb s = {0};
    const char *p = ln->in, *end = ln->in + ln->len;
    for (size_t r = 0; r < ln->recs; ++r) {
        const char *l0 = (const char *)memchr(p, '\n', (size_t)(end - p)) + 1;           /* the bases line */
        const char *l1 = (const char *)memchr(l0, '\n', (size_t)(end - l0));
        sb_str(&s, "sequence "); sb_add(&s, l0, (size_t)(l1 - l0)); sb_str(&s, ": \n");
        sb_str(&s, "sequence "); sb_add(&s, l0, (size_t)(l1 - l0)); sb_str(&s, " matched barcode: "); sb_str(&s, R->t->name[ln->rec_bin[r]]);
        sb_add(&s, "\n", 1);
        p = l1 + 1;
        for (int k = 2; k < R->lpr; ++k) p = (const char *)memchr(p, '\n', (size_t)(end - p)) + 1;
    }
    if (s.n) (void)!write(STDERR_FILENO, s.p, s.n);
    free(s.p);
}

static void *writer_thread(void *arg)
{
    fxh_split_run_t *R = (fxh_split_run_t *)arg;
    const uint32_t bins = R->t->nbins;
    for (uint64_t k = 0;; ++k) {
        fxh_split_lane *ln = &R->lane[k % (uint64_t)R->nlanes];
        pthread_mutex_lock(&R->mu);
        while (!(k < R->blocks && ln->state == L_DONE && ln->block == k) && !(R->finished && k >= R->blocks)) pthread_cond_wait(&R->cv, &R->mu);
        const int done = R->finished && k >= R->blocks;
        pthread_mutex_unlock(&R->mu);
        if (done) break;
        if (R->debug) debug_block(R, ln);
        const uint32_t last_bin = ln->rec_bin[ln->want_bins ? ln->recs - 1 : 0];
        size_t off = 0;
        for (uint32_t b = 0; b < bins; ++b) {
            const size_t nb = (size_t)ln->bin_bytes[b];
            out_append(R, b, ln->out + off, nb - (ln->drop_last && b == last_bin ? 1u : 0u));
            off += nb;
            R->counts[b] += ln->bin_records[b];
        }
        pthread_mutex_lock(&R->mu);
        ln->state = L_IDLE;
        pthread_cond_broadcast(&R->cv);
        pthread_mutex_unlock(&R->mu);
    }
    for (uint32_t b = 0; b < bins; ++b) if (R->wlen[b]) write_all(R->fd[b], R->wbuf[b], R->wlen[b]);
    return NULL;
}

static size_t count_nl(const char *p, size_t n)
{
    size_t c = 0;
    const char *e = p + n;
    while (p < e && (p = (const char *)memchr(p, '\n', (size_t)(e - p))) != NULL) { ++c; ++p; }
    return c;
}

static int cmp_names(const void *a, const void *b, void *t)
{
    char **name = (char **)t;
    return strcmp(name[*(const uint32_t *)a], name[*(const uint32_t *)b]);
}

int fxh_split_run(const fxh_split_opts *o)
{
    fxh_table t;
    table_load(&t, o);

    /* stdin: the first byte picks the format (before any output file exists) */
    size_t cap = (size_t)64 << 20;
    {
        struct stat sb;
        if (fstat(STDIN_FILENO, &sb) == 0 && S_ISFIFO(sb.st_mode)) cap = (size_t)16 << 20;
        if (fxh_read_buffer_bytes()) cap = fxh_read_buffer_bytes();
    }
    struct fxh_reader *rd = fxh_reader_open("-", cap);
    fxh_prefetch pf;
    memset(&pf, 0, sizeof pf);
    char *spare = NULL;
    fxh_next_block(&pf, rd, &spare);
    if (rd->end == rd->beg) fxh_split_die("Error: unknown file format. First character = '' (expecting > or @)");
    const char first = rd->buf[rd->beg];
    if (first != '@' && first != '>') {
        fxh_sb s = {0};
        sb_str(&s, "Error: unknown file format. First character = '"); sb_add(&s, &first, 1); sb_str(&s, "' (expecting > or @)");
        sb_die(&s);
    }
    const int fastq = first == '@', lpr = fastq ? 4 : 2;
    if (o->debug) { const char *m = fastq ? "Detected FASTQ format\n" : "Detected FASTA format\n"; (void)!write(STDERR_FILENO, m, strlen(m)); }

    /* every output file, created (truncated) before the first record */
    fxh_split_run_t R;
    memset(&R, 0, sizeof R);
    const uint32_t bins = t.nbins;
    R.t = &t; R.lpr = lpr; R.debug = o->debug;
    R.fd = (int *)calloc(bins, sizeof(int));
    R.wbuf = (char **)calloc(bins, sizeof(char *));
    R.wlen = (size_t *)calloc(bins, sizeof(size_t));
    R.counts = (uint64_t *)calloc(bins, sizeof(uint64_t));
    char **fname = (char **)calloc(bins, sizeof(char *));
    if (!R.fd || !R.wbuf || !R.wlen || !R.counts || !fname) err(1, "out of memory");
    for (uint32_t b = 0; b < bins; ++b) {
        if (asprintf(&fname[b], "%s%s%s", o->prefix, t.name[b], o->suffix) < 0) err(1, "out of memory");
        R.fd[b] = open(fname[b], O_WRONLY | O_CREAT | O_TRUNC, 0666);
        if (R.fd[b] < 0) fxh_split_die("Error: failed to create output file (%s)", fname[b]);
    }

    /* lanes: FXH_LANES per GPU (default 2) over FXG_DEVICES, consecutive blocks on different GPUs */
    int dev[FXH_MAX_LANES];
    const int ndev = fxh_device_list(dev, FXH_MAX_LANES);
    int per = 2;
    { const char *e = getenv("FXH_LANES"); if (e) per = atoi(e); if (per < 1) per = 1; }
    int nl = 0;
    for (int k = 0; k < per; ++k) for (int d = 0; d < ndev && nl < FXH_MAX_LANES; ++d) ++nl;
    R.nlanes = nl;
    R.lane = (fxh_split_lane *)calloc((size_t)nl, sizeof(fxh_split_lane));
    if (!R.lane) err(1, "out of memory");
    pthread_mutex_init(&R.mu, NULL);
    pthread_cond_init(&R.cv, NULL);
    for (int i = 0; i < nl; ++i) {
        fxh_split_lane *ln = &R.lane[i];
        ln->id = i; ln->device = dev[i % ndev]; ln->state = L_IDLE; ln->want_bins = o->debug;
        int rc = fxg_ctx_create(ln->device, &ln->ctx);
        if (rc != FXG_OK) errx(1, "no usable GPU (device %d): the engine has no CPU fallback (fxg_ctx_create = %d)", ln->device, rc);
        fxg_barcode_set set;
        memset(&set, 0, sizeof set);
        set.bases = t.bases; set.len = t.len; set.bin = t.bin; set.entries = t.entries; set.barcode_len = t.BL;
        set.mismatches = (uint32_t)o->mismatches; set.eol = (uint32_t)o->eol; set.bins = bins;
        if (fxg_barcode_prepare(ln->ctx, &set) != FXG_OK) errx(1, "fxg_barcode_prepare: %s", fxg_last_error(ln->ctx));
        ln->bin_bytes = (uint64_t *)calloc(bins, sizeof(uint64_t));
        ln->bin_records = (uint64_t *)calloc(bins, sizeof(uint64_t));
        if (!ln->bin_bytes || !ln->bin_records) err(1, "out of memory");
        lane_arg *a = (lane_arg *)malloc(sizeof *a);
        if (!a) err(1, "out of memory");
        a->R = &R; a->ln = ln;
        if (pthread_create(&ln->th, NULL, lane_thread, a) != 0) err(1, "pthread_create");
    }
    pthread_t wth;
    if (pthread_create(&wth, NULL, writer_thread, &R) != 0) err(1, "pthread_create");

    /* blocks cut at record boundaries; the end of input gets the '\n' it may lack (only a FASTQ quality line keeps it missing) */
    size_t extra = 0;
    int appended = 0;
    for (;;) {
        char *p = rd->buf + rd->beg;
        size_t len = rd->end - rd->beg;
        const int eof = rd->eof;
        if (eof && len > 0 && p[len - 1] != '\n') { p[len++] = '\n'; appended = 1; }       /* (the reader's buffers hold cap + 1 bytes) */
        const size_t nls = count_nl(p, len);
        const size_t recs = nls / (size_t)lpr;
        size_t cut = 0;
        if (recs > 0) {
            size_t q = len;
            for (size_t k = 0; k <= nls % (size_t)lpr; ++k) q = (size_t)((const char *)memrchr(p, '\n', q) - p);
            cut = q + 1;
        }
        if (eof) extra = nls % (size_t)lpr;
        if (cut > 0) {
            fxh_split_lane *ln = &R.lane[R.blocks % (uint64_t)nl];
            pthread_mutex_lock(&R.mu);
            while (ln->state != L_IDLE) pthread_cond_wait(&R.cv, &R.mu);
            pthread_mutex_unlock(&R.mu);
            if (ln->in_cap < cut + 64) {
                if (ln->in) (void)fxg_free_host(ln->ctx, ln->in);
                if (ln->out) (void)fxg_free_host(ln->ctx, ln->out);
                ln->in_cap = cut + cut / 8 + 4096;
                if (fxg_malloc_host(ln->ctx, ln->in_cap, (void **)&ln->in) != FXG_OK || fxg_malloc_host(ln->ctx, ln->in_cap, (void **)&ln->out) != FXG_OK)
                    errx(1, "fxg_malloc_host: %s", fxg_last_error(ln->ctx));
            }
            if (ln->rb_cap < recs) {
                free(ln->rec_bin);
                ln->rb_cap = recs + recs / 8 + 64;
                ln->rec_bin = (uint16_t *)malloc(ln->rb_cap * sizeof(uint16_t));
                if (!ln->rec_bin) err(1, "out of memory");
            }
            memcpy(ln->in, p, cut);
            pthread_mutex_lock(&R.mu);
            ln->len = cut; ln->recs = recs; ln->block = R.blocks++;
            ln->drop_last = eof && appended && fastq && extra == 0;
            ln->state = L_QUEUED;
            pthread_cond_broadcast(&R.cv);
            pthread_mutex_unlock(&R.mu);
        }
        if (eof) break;
        rd->beg += cut;
        fxh_next_block(&pf, rd, &spare);
    }
    fxh_prefetch_stop(&pf);
    pthread_mutex_lock(&R.mu);
    R.finished = 1;
    pthread_cond_broadcast(&R.cv);
    pthread_mutex_unlock(&R.mu);
    pthread_join(wth, NULL);
    pthread_mutex_lock(&R.mu);
    R.quit = 1;
    pthread_cond_broadcast(&R.cv);
    pthread_mutex_unlock(&R.mu);
    for (int i = 0; i < nl; ++i) pthread_join(R.lane[i].th, NULL);
    for (uint32_t b = 0; b < bins; ++b) if (close(R.fd[b]) != 0) err(1, "close failed (%s)", fname[b]);
    for (int i = 0; i < nl; ++i) fxg_ctx_destroy(R.lane[i].ctx);

    if (extra) {
        static const char *what[] = {"", "sequences", "sequence name2", "quality scores"};
        fxh_split_die("Error: bad input file, expecting line with %s", what[extra]);
    }
    if (!o->quiet) {
        uint32_t *ord = (uint32_t *)malloc(bins * sizeof(uint32_t));
        if (!ord) err(1, "out of memory");
        for (uint32_t b = 0; b < bins; ++b) ord[b] = b;
        qsort_r(ord, bins, sizeof(uint32_t), cmp_names, t.name);
        uint64_t total = 0;
        fputs("Barcode\tCount\tLocation\n", stdout);
        for (uint32_t i = 0; i < bins; ++i) {
            printf("%s\t%llu\t%s\n", t.name[ord[i]], (unsigned long long)R.counts[ord[i]], fname[ord[i]]);
            total += R.counts[ord[i]];
        }
        printf("total\t%llu\n", (unsigned long long)total);
        free(ord);
    }
    if (fflush(stdout) != 0) err(1, "write failed");
    return 0;
}
