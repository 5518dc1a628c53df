/* fxh_rank.c -- the rank-per-GPU job of the one-file run (fxh_strands.c; fxh_priv.h). */
/* FXH_WORLD = n > 1 with FXH_RANK = 0 .. n-1: n processes, one per GPU, each over its byte range of the input.  Where a rank's text goes in the ONE file is only
 * known once every rank has decided its range, so the formatted chunks stay on the device (the arena: HBM holds any realistic range) until the ranks have
 * exchanged their counter blocks -- one RCCL all-gather (fxg_epilogue_rccl) -- and then go down and out at base + local offset.  Three exchanges: the counter
 * blocks; "rank 0 has made the file's pages" (or not); "every rank has written its part".  Each runs under a watch, so nobody waits for a dead rank for ever. */
#include "fxh_priv.h"
#include <sys/mman.h>

/* what only a rank of a rank-per-GPU job has */
struct fxh_rank {
    int rank, world;
    fxh_lane lane;                         /* the context that owns the arena and the communicator */
    fxg_ctx *ctx;
    fxg_comm *comm;
    uint8_t *arena;                        /* this rank's formatted text, on the device until the exchange has said where it goes */
    uint64_t arena_cap;
    uint64_t *d_block;
    uint64_t base, job_total;              /* the exchange's answer: the bytes of the ranks before this one, and of all */
    /* the drain: mu / cv are its own (it runs when the strands and the allocator are gone: no other lock is held with them) */
    pthread_mutex_t mu;
    pthread_cond_t cv;
    int out_fd;
    char *map;                             /* this rank's slice of the file, where rank 0 has made its pages */
    uint64_t map_base;                     /* file offset of map[0] (the page this rank's slice starts in) */
    int drain_errno;                       /* errno of the first piece of this rank's text that did not get into the file */
    int drained_by_copy;
    double t_drain;
};

/* the counter block a rank contributes to the job's one all-gather (u64[FXG_NCOUNTERS], text level): records and reads in and out, the BYTES of its
 * formatted output where the batch ABI has kept bases -- so that fxg_epilogue's exclusive scan is the rank's offset in the file -- and the -v tallies */
enum { FXH_B_IN_SEQ = FXG_C_INPUT, FXH_B_OUT_SEQ = FXG_C_KEPT, FXH_B_OUT_BYTES = FXG_C_KEPT_BASES, FXH_B_BAD = FXG_C_ERRORS,
       FXH_B_IN_READS = 17, FXH_B_OUT_READS = 18, FXH_B_CLIP_IN = 19, FXH_B_CLIP_LEN = 20 };
#define FXH_BAD_IRREGULAR ((uint64_t)1 << 40)      /* (above the device's own error bits) */
/* every tally of fxh_totals and its place in the block: a new one is added HERE, and crosses in both directions (the clip tallies are 32-bit unsigned in
 * fxh_totals, like the reference's: the job's sums are narrowed to that on the way back) */
#define FXH_B_TALLIES(X) \
    X(FXH_B_IN_SEQ, input_sequences) X(FXH_B_OUT_SEQ, output_sequences) X(FXH_B_IN_READS, input_reads) X(FXH_B_OUT_READS, output_reads) \
    X(FXH_B_CLIP_IN, clip_input) X(FXG_C_CLIP_TOO_SHORT, clip_too_short) X(FXG_C_CLIP_ADAPTER_ONLY, clip_adapter_only) X(FXG_C_CLIP_NO_ADAPTER, clip_no_adapter) \
    X(FXG_C_CLIP_ADAPTER_FOUND, clip_adapter_found) X(FXG_C_CLIP_N, clip_n) X(FXG_C_QTRIM_DROPPED, qtrim_dropped) \
    X(FXG_C_MASKED_READS, masked_reads) X(FXG_C_MASKED_NT, masked_nucleotides)
static void fxh_block_from_totals(uint64_t *blk, const fxh_totals *t)
{
#define X(i, f) blk[i] = t->f;
    FXH_B_TALLIES(X)
#undef X
}
static void fxh_totals_from_block(fxh_totals *t, const uint64_t *blk)
{
#define X(i, f) t->f = (__typeof__(t->f))blk[i];
    FXH_B_TALLIES(X)
#undef X
}

/* FXH_RENDEZVOUS, else <output>.rdv: where the ranks of a job meet */
void fxh_rendezvous_name(const FASTX *fx, char *dst, size_t cap)
{
    const char *re = getenv("FXH_RENDEZVOUS");
    if (re && *re) snprintf(dst, cap, "%s", re); else snprintf(dst, cap, "%s.rdv", fx->output_file_name);
}

/* rank mode: nobody waits for a dead rank for ever.  An all-gather that a rank never joins does not return (RCCL has no time-out of its own), so every
 * exchange runs under a watch: FXH_RANK_TIMEOUT seconds (default 900) without the other ranks' answer end this rank with a message and exit code 1. */
typedef struct { pthread_mutex_t mu; pthread_cond_t cv; pthread_t th; int done, secs, rank, world; const char *what; } fxh_watch;
static void *fxh_watch_main(void *arg)
{
    fxh_watch *w = (fxh_watch *)arg;
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    ts.tv_sec += w->secs;
    pthread_mutex_lock(&w->mu);
    int rc = 0;
    while (!w->done && rc != ETIMEDOUT) rc = pthread_cond_timedwait(&w->cv, &w->mu, &ts);
    const int late = !w->done;
    pthread_mutex_unlock(&w->mu);
    if (late) {
        warnx("rank %d of %d: no answer from the other ranks within %d s (%s): a rank has died or is stuck (FXH_RANK_TIMEOUT)", w->rank, w->world, w->secs, w->what);
        fflush(NULL);
        _exit(1);
    }
    return NULL;
}
static void fxh_watch_start(fxh_watch *w, int rank, int world, const char *what)
{
    memset(w, 0, sizeof *w);
    pthread_mutex_init(&w->mu, NULL); pthread_cond_init(&w->cv, NULL);
    w->secs = (int)fxh_env_long("FXH_RANK_TIMEOUT", 900, 1, 7 * 86400); w->rank = rank; w->world = world; w->what = what;
    if (pthread_create(&w->th, NULL, fxh_watch_main, w) != 0) err(1, "pthread_create");
}
static void fxh_watch_stop(fxh_watch *w)
{
    pthread_mutex_lock(&w->mu);
    w->done = 1;
    pthread_cond_broadcast(&w->cv);
    pthread_mutex_unlock(&w->mu);
    pthread_join(w->th, NULL);
}

/* one exchange of the job: this rank's block up, ncclAllGather (fxg_epilogue_rccl), every rank's block and the totals back */
static void fxh_rank_exchange(fxh_rank *R, const uint64_t *blk, uint64_t *totals, uint64_t *byte_off, uint64_t *gathered, const char *what)
{
    fxh_watch w;
    uint64_t read_off = 0;
    fxh_watch_start(&w, R->rank, R->world, what);
    FXG_CHECK(&R->lane.st, fxg_memcpy_h2d(R->ctx, R->d_block, blk, FXG_NCOUNTERS * sizeof(uint64_t)));
    const int erc = fxg_epilogue_rccl(R->ctx, R->comm, R->d_block, totals, &read_off, byte_off, gathered);
    fxh_watch_stop(&w);
    if (erc != 0) errx(1, "rank %d of %d: %s failed (%d): %s", R->rank, R->world, what, erc, fxg_last_error(R->ctx));
}

/* one process per GPU: FXG_DEVICE if the launcher set it (listed: the caller's choice stands), else the rank's turn among the GPUs of the box */
int fxh_rank_device(int rank, int listed)
{
    if (getenv("FXG_DEVICE") || getenv("FXG_DEVICES")) return listed;
    const int nd = fxg_device_count();
    g_hip_touched = 1;
    return nd > 0 ? rank % nd : 0;
}

/* the context that owns the arena and the communicator, the arena (8/7 of the range bounds its output), the communicator */
fxh_rank *fxh_rank_open(const FASTX *fx, int rank, int world, int device, int out_fd, uint64_t in_total)
{
    static fxh_rank R_;                          /* (static: zeroed, and alive for the whole process) */
    fxh_rank *R = &R_;
    R->rank = rank; R->world = world; R->out_fd = out_fd;
    pthread_mutex_init(&R->mu, NULL); pthread_cond_init(&R->cv, NULL);
    R->lane.device = device;
    fxh_lane_open_ctx(&R->lane);
    R->ctx = R->lane.st.ctx;
    R->arena_cap = fxh_format_file_bound(&g_fmt, in_total);
    if (fxg_malloc_device(R->ctx, (size_t)R->arena_cap, (void **)&R->arena) != 0 || !R->arena)
        errx(1, "rank %d of %d: %.1f GB of device memory for this rank's share of the output are not to be had (%s); start more ranks", rank, world,
             1e-9 * (double)R->arena_cap, fxg_last_error(R->ctx));
    FXG_CHECK(&R->lane.st, fxg_malloc_device(R->ctx, FXG_NCOUNTERS * sizeof(uint64_t), (void **)&R->d_block));
    /* stdout is the tool's data and report channel (the -v report goes there when -o names a file): a collective library told to talk
     * (NCCL_DEBUG=VERSION / INFO in the job's environment) talks to stderr, unless the user has sent it somewhere already */
    if (getenv("NCCL_DEBUG") && !getenv("NCCL_DEBUG_FILE")) (void)setenv("NCCL_DEBUG_FILE", "/dev/stderr", 0);
    char rdv[PATH_MAX + 16];
    fxh_rendezvous_name(fx, rdv, sizeof rdv);
    /* (and whatever it prints unasked -- RCCL 2.26 greets with its version, the runtime's and the host name on stdout -- goes to stderr as well:
     * descriptor 1 is descriptor 2 while the communicator is made) */
    fflush(stdout);
    const int saved_out = dup(STDOUT_FILENO);
    if (saved_out >= 0) (void)dup2(STDERR_FILENO, STDOUT_FILENO);
    /* (under a watch like the exchanges: the rendezvous time-out covers the wait for the record, not a communicator that a missing rank never completes) */
    fxh_watch cw;
    fxh_watch_start(&cw, rank, world, "the rendezvous (making the communicator)");
    const int crc = fxg_comm_create(R->ctx, rdv, (uint32_t)rank, (uint32_t)world, (int)fxh_env_long("FXH_RENDEZVOUS_TIMEOUT", 120, 1, 86400), &R->comm);
    fxh_watch_stop(&cw);
    fflush(stdout);
    if (saved_out >= 0) { (void)dup2(saved_out, STDOUT_FILENO); close(saved_out); }
    if (crc != 0) errx(1, "rank %d of %d: no communicator (%d): %s", rank, world, crc, fxg_last_error(R->ctx));
    return R;
}

void fxh_rank_close(fxh_rank *R) { if (R->ctx) fxg_ctx_destroy(R->ctx); }

/* a chunk's text stays on the device: copied behind the format kernels into the arena at its local offset.  0 = it does not fit. */
int fxh_rank_place(fxh_rank *R, fxh_lane *ln, uint64_t off, uint64_t bytes)
{
    if (off + bytes > R->arena_cap) return 0;    /* (cannot happen: 8/7 of the range bounds its output) */
    FXG_CHECK(&ln->st, fxg_concat_peer(R->ctx, R->arena, off, ln->st.ctx, ln->st.d_out_text, bytes));
    FXG_CHECK(&ln->st, fxg_sync(ln->st.ctx));
    return 1;
}

/* The exchange of the job: every rank's counter block, one ncclAllGather behind nothing (the strands have synchronised).  A rank that met
 * something irregular still takes part -- with its flag up -- so that ALL ranks leave together and rank 0 alone runs the input as one stream.
 * Sets R->base / R->job_total, turns *mine into the JOB's totals (rank 0 reports them); returns whether the job is abandoned. */
static int fxh_rank_counters(fxh_rank *R, fxh_totals *mine, uint64_t local_bytes, int clip_auto, uint64_t clip_len, int bad, uint64_t *gathered)
{
    uint64_t blk[FXG_NCOUNTERS] = {0}, totals[FXG_NCOUNTERS], byte_off = 0;
    fxh_block_from_totals(blk, mine);
    blk[FXH_B_OUT_BYTES] = local_bytes; blk[FXH_B_CLIP_LEN] = clip_len; blk[FXH_B_BAD] = bad ? FXH_BAD_IRREGULAR : 0;
    fxh_rank_exchange(R, blk, totals, &byte_off, gathered, "the exchange of the counter blocks");
    if (totals[FXH_B_BAD]) bad = 1;
    /* the clipper is exact across ranks while ALL reads of the job have one length */
    uint64_t len0 = 0;
    for (int g = 0; g < R->world && clip_auto && !bad; ++g) bad = !fxh_one_length(&len0, gathered[(size_t)g * FXG_NCOUNTERS + FXH_B_CLIP_LEN]);
    R->base = byte_off; R->job_total = totals[FXH_B_OUT_BYTES];
    memset(mine, 0, sizeof *mine);
    fxh_totals_from_block(mine, totals);
    return bad;
}

/* rank 0: the job's pages, to the byte (or, abandoned: the allocator stops where it is; the file is emptied by the caller).  Then, unless abandoned,
 * "the pages are there" (or not: another file system -- positional writes then): rank 0 says, everybody hears; also the barrier between the last
 * fallocate() and the first copy.  Returns whether this rank copies into pages that exist. */
static int fxh_rank_pages(fxh_rank *R, fxh_sink *prealloc, int bad, uint64_t *gathered)
{
    int pages = 0, alloc_e = 0;
    if (prealloc) {
        alloc_e = fxh_sink_end(prealloc, !bad, R->job_total);
        if (!bad && !alloc_e && ftruncate(R->out_fd, (off_t)R->job_total) != 0) alloc_e = errno;      /* what the estimate overshot goes back */
        pages = !bad && !alloc_e;
    }
    if (bad) return 0;
    uint64_t blkp[FXG_NCOUNTERS] = {0}, totalsp[FXG_NCOUNTERS], offp = 0;
    blkp[FXH_B_IN_SEQ] = (uint64_t)pages; blkp[FXH_B_BAD] = (uint64_t)alloc_e;
    fxh_rank_exchange(R, blkp, totalsp, &offp, gathered, "waiting for rank 0 to have made the output file's pages");
    if (totalsp[FXH_B_BAD]) {
        if (R->rank == 0) warnx("writing output failed: %s", strerror(alloc_e));
        fflush(NULL);
        _exit(1);
    }
    return gathered[FXH_B_IN_SEQ] != 0;          /* (rank 0's block) */
}

typedef struct { fxh_rank *R; const char *src; size_t len; uint64_t off; int *busy; } fxh_djob;
static void fxh_rank_drain_task(void *arg)
{
    fxh_djob *j = (fxh_djob *)arg;
    fxh_rank *R = j->R;
    int e = 0;
    if (R->map) {                                /* pages that exist (rank 0 made them): a copy, and this thread drops its own page-table entries */
        char *dst = R->map + (j->off - R->map_base);
        memcpy(dst, j->src, j->len);
        const uintptr_t a = ((uintptr_t)dst + 4095u) & ~(uintptr_t)4095u, b = ((uintptr_t)dst + j->len) & ~(uintptr_t)4095u;
        if (b > a) (void)madvise((void *)a, (size_t)(b - a), MADV_DONTNEED);
    } else {
        errno = 0;
        e = fxg_concat_pwrite(R->out_fd, j->src, j->len, j->off) != 0 ? (errno ? errno : EIO) : 0;
    }
    pthread_mutex_lock(&R->mu);
    if (e && !R->drain_errno) R->drain_errno = e;        /* reported to the job (the last exchange), not died of: the other ranks are waiting */
    *j->busy = 0;
    pthread_cond_broadcast(&R->cv);
    pthread_mutex_unlock(&R->mu);
}

/* this rank's text: down from the arena in pieces, each put where it belongs -- base (the bytes of the ranks before) + its place in the arena.
 * A piece that does not get into the file (no space, a file size limit) is not died of here: the other ranks are waiting for this one. */
static void fxh_rank_drain(fxh_rank *R, int pages, uint64_t local_bytes)
{
    const double t0 = fxh_now();
    if (pages && local_bytes) {
        R->map_base = R->base & ~(uint64_t)4095u;
        void *m = mmap(NULL, (size_t)(R->base + local_bytes - R->map_base), PROT_READ | PROT_WRITE, MAP_SHARED, R->out_fd, (off_t)R->map_base);
        if (m != MAP_FAILED) R->map = (char *)m;     /* (no mapping -- a descriptor without read access --: positional writes into the same pages) */
    }
    if (!pages && ftruncate(R->out_fd, (off_t)R->job_total) != 0) R->drain_errno = errno;      /* (every rank says the same size; no rank's bytes lie beyond it) */
    enum { NBMAX = 9 };
    const size_t piece = (size_t)fxh_env_long("FXH_DRAIN_MB", 32, 1, 1024) << 20;
    const int nth = (int)fxh_env_long("FXH_DRAIN_THREADS", R->map ? 4 : 2, 1, NBMAX - 1), NB = nth + 1;      /* copies want company, writers only queue at the inode */
    char *hb[NBMAX]; int busy[NBMAX] = {0}; fxh_djob dj[NBMAX];
    fxh_pool dpool;
    fxh_pool_start(&dpool, nth, (unsigned)NB);
    for (int k = 0; k < NB; ++k) FXG_CHECK(&R->lane.st, fxg_malloc_host(R->ctx, piece, (void **)&hb[k]));
    int k = 0;
    for (uint64_t o = 0; o < local_bytes; o += piece, k = (k + 1) % NB) {
        const size_t n = local_bytes - o < piece ? (size_t)(local_bytes - o) : piece;
        pthread_mutex_lock(&R->mu);
        while (busy[k]) pthread_cond_wait(&R->cv, &R->mu);
        const int failed = R->drain_errno;
        if (!failed) busy[k] = 1;
        pthread_mutex_unlock(&R->mu);
        if (failed) break;
        FXG_CHECK(&R->lane.st, fxg_memcpy_d2h(R->ctx, hb[k], R->arena + o, n));
        FXG_CHECK(&R->lane.st, fxg_sync(R->ctx));
        dj[k].R = R; dj[k].src = hb[k]; dj[k].len = n; dj[k].off = R->base + o; dj[k].busy = &busy[k];
        fxh_pool_submit(&dpool, fxh_rank_drain_task, &dj[k]);
    }
    fxh_pool_stop(&dpool);
    R->drained_by_copy = R->map != NULL;
    if (R->map) { munmap(R->map, (size_t)(R->base + local_bytes - R->map_base)); R->map = NULL; }
    R->t_drain = fxh_now() - t0;
}

/* The job is done when EVERY rank's text is in the file, and rank 0's exit code says so: a last exchange, each rank's errno (0: written).  A rank
 * that died on the way never joins it -- the watch (or the transport) ends the wait -- so rank 0 never reports a file that has a hole as done. */
static void fxh_rank_written(fxh_rank *R, const FASTX *fx, uint64_t *gathered)
{
    uint64_t blk2[FXG_NCOUNTERS] = {0}, totals2[FXG_NCOUNTERS], off2 = 0;
    blk2[FXH_B_BAD] = (uint64_t)R->drain_errno;
    fxh_rank_exchange(R, blk2, totals2, &off2, gathered, "waiting for every rank to have written its part");
    if (!totals2[FXH_B_BAD]) return;
    if (R->drain_errno) warnx("rank %d of %d: writing output failed: %s", R->rank, R->world, strerror(R->drain_errno));
    if (R->rank == 0)
        for (int g = 1; g < R->world; ++g) {
            const uint64_t e = gathered[(size_t)g * FXG_NCOUNTERS + FXH_B_BAD];
            if (e) warnx("rank %d of %d could not write its part of the output (%s): %s is incomplete", g, R->world, strerror((int)e), fx->output_file_name);
        }
    fflush(NULL);
    _exit(1);
}

/* The strands of this rank are through (local_bytes of text in the arena, their tallies in *mine, `bad`: something irregular was met): the job's three
 * exchanges and the drain between them.  prealloc: the sink whose allocator is making the job's pages (rank 0 on a tmpfs), else NULL.  Returns whether
 * the job is abandoned; otherwise the text is in the file, *mine is the JOB's totals and *job_total the file's size. */
int fxh_rank_finish(fxh_rank *R, const FASTX *fx, fxh_sink *prealloc, fxh_totals *mine, uint64_t local_bytes, int clip_auto, uint64_t clip_len, int bad, uint64_t *job_total)
{
    uint64_t *gathered = (uint64_t *)calloc((size_t)R->world * FXG_NCOUNTERS, sizeof(uint64_t));
    if (!gathered) err(1, "out of memory");
    bad = fxh_rank_counters(R, mine, local_bytes, clip_auto, clip_len, bad, gathered);
    const int pages = fxh_rank_pages(R, prealloc, bad, gathered);
    if (!bad) {
        fxh_rank_drain(R, pages, local_bytes);
        fxh_rank_written(R, fx, gathered);
    }
    free(gathered);
    fxg_comm_destroy(R->comm);
    *job_total = R->job_total;
    return bad;
}

void fxh_rank_report(const fxh_rank *R, long long my_start, long long my_end, uint64_t local_bytes)
{
    fprintf(stderr, "fxh timing rank %d of %d: input bytes [%lld, %lld), %.3f GB of text held on the device, written at offset %llu of %llu in %.3f s (%s)\n", R->rank, R->world,
            my_start, my_end, 1e-9 * (double)local_bytes, (unsigned long long)R->base, (unsigned long long)R->job_total, R->t_drain,
            R->drained_by_copy ? "copies into pages rank 0 made" : "positional writes");
}
