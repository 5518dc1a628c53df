/* fxh_strands.c -- `tool -i in.fq -o out.fq`, ONE output file, at the speed of the sharded run (fxh_priv.h). */
/* ---------------------------------------------------------------------------------------------- */
/* The reference writes one output stream (fastx.c:251-271: one fdopen; fastx.c:440-473).  The sharded run of fxh_parts.c is fast because */
/* it has k of everything -- k byte ranges read side by side, k x lanes on the device, k output FILES -- and that last k is what no        */
/* reference command line has.  Here the same input goes to ONE file, written at exact offsets by many threads:                             */
/*   * the input file is cut into CHUNKS (16 MB) at record boundaries found by pattern and proven by induction, exactly like the parts       */
/*     (chunk c ends where chunk c + 1 begins; a chunk that is not a whole number of regular records stops the attempt);                   */
/*   * STRANDS (one thread + one engine context each, FXH_STRANDS per GPU) draw chunk numbers from one counter, so the chunk order IS the   */
/*     output order; a strand reads its chunk with parallel pread(), uploads, indexes, decides and formats it on the device;                */
/*   * the formatted SIZE of a chunk is known before its text comes down.  Sizes are published in an array; the file offset of chunk c is   */
/*     the sum of the sizes before it (a running scan advanced by whoever publishes), so it is known as soon as every earlier chunk has     */
/*     been DECIDED -- not written, not even downloaded.  The smallest unfinished chunk never waits for anybody, every strand owns its      */
/*     buffers, so there is no deadlock by construction.  No second pass over the input, no text held back in HBM: the two-phase form       */
/*     (sizes first, text later) would serialise upload and download on the PCIe link, which is the resource the run is bound by;           */
/*   * the SINK.  One inode of a tmpfs (or any page cache) takes fresh pages from ONE thread at a time: concurrent pwrite() serialise on    */
/*     the inode lock (4 GB/s with 8 threads against 9 with one), concurrent faults on a shared mapping on the mapping's locks (5 GB/s),     */
/*     k files take 30-90 GB/s (profiles/r05/a_one_file_write.txt).  What does scale is copying into pages that EXIST: fallocate()          */
/*     allocates without zeroing or copying at 18 GB/s as long as nobody faults on the file meanwhile, and 16 threads then copy into the     */
/*     mapping at 30 GB/s.  So allocation and copies take turns behind a gate (fxh_sf_alloc_main), the allocator runs ahead in 128 MB        */
/*     windows -- from the first milliseconds of the process, while the device is still starting and nothing is there to be written --       */
/*     and the copies drop their page-table entries themselves (MADV_DONTNEED, shared mmap_lock), so the process does not spend 0.2 s        */
/*     unmapping at exit.  Measured with the tool's own access pattern: 10 GB into one tmpfs file in 0.65 s after a 0.25 s head start,       */
/*     against 1.4 s through one pwrite() stream and 1.6 s ungated (profiles/r05/d_one_file_gate.txt).  Other file systems get pwrite().    */
/* Anything irregular (a malformed record, a cut that was not a boundary, a clipper input whose reads are not all of one length) abandons   */
/* the attempt exactly like the sharded run: it lives in a forked child, which empties the file and leaves with FXH_EXIT_ABANDON, and the   */
/* parent -- which has not touched the GPU -- runs the input as one stream, so messages, exit codes and partial output are the reference's. */
/* The file in its own order: the run's state; the SINK (allocator, write-at, open / end / close); the STRANDS (reader, copy task, device thread); */
/* the CUTS; the ATTEMPT (eligible? -- cuts -- the fork frame of fxh_parts.c -- the child: sink, placement, strands, finish, abandon or report).    */
/* The rank-per-GPU job is fxh_rank.c, the task pool fxh_io.c.                                                                                      */
/* LOCKS: a strand's mu (its slots), the run's mu / cv (sizes and offsets, the clipper's length, ALL of the sink's state: the sink borrows them),   */
/* the sink's gate (fallocate exclusive, copies shared).  No thread ever holds two of them at once: every wait and every hold below is entered     */
/* with nothing else held, so there is no lock order to get wrong.                                                                                  */
/* ---------------------------------------------------------------------------------------------- */
#include "fxh_priv.h"
#include <sys/mman.h>
#include <sys/vfs.h>
#ifndef TMPFS_MAGIC
#define TMPFS_MAGIC 0x01021994
#endif

#define FXH_TICKET_DONE ((uint64_t)-1)
#define FXH_MAX_STRANDS FXH_MAX_LANES


/* the sink (rank 0 of a rank job makes the job's pages with it: fxh_sink_end is fxh_rank.c's to call) */
struct fxh_sink {
    pthread_mutex_t *mu;                   /* the run's mutex and condition variable: everything below except the gate's own business is under them */
    pthread_cond_t *cv;
    int out_fd, mapped;
    int prealloc;                          /* rank mode, rank 0, a tmpfs: the allocator makes the JOB's pages while the ranks compute (nobody copies meanwhile) */
    char *map;
    uint64_t map_len, alloc_end, need, window;
    uint64_t alloc_in_total;               /* the input the allocator's estimate is about: this process's (strands) or the job's (rank 0 of a rank job) */
    uint64_t in_done, out_done;            /* input bytes decided so far and what they came to: the measured ratio (fxh_sink_progress) */
    uint64_t ratio_after;                  /* input bytes that must have been decided before the measured output/input ratio counts (64 MB) */
    int keep_surplus;                      /* FXH_ONE_FILE_KEEP_SURPLUS=1: measurements of the run without it */
    uint64_t given_back;                   /* pages the head start made and the output turned out not to need, returned during the run */
    uint64_t alloc_final; int alloc_final_set;      /* the exact size, once known: strands -- every chunk published; rank job -- the exchange */
    int alloc_errno, alloc_stop, alloc_capped;      /* alloc_capped: the head start met ENOSPC -- from here on only what a copy asks for */
    pthread_t th_alloc;
    pthread_rwlock_t gate;                 /* fallocate() exclusive, copies shared; writer-preferring */
    double t_alloc, t_copy, t_copy_wait;   /* t_copy*: summed over the copy tasks, under mu */
    uint64_t alloc_calls;
};

/* ---- the run ---- */
typedef struct fxh_sf fxh_sf;
typedef struct fxh_strand fxh_strand;
typedef struct { fxh_strand *s; int fd; char *dst; size_t n; off_t off; } fxh_rjob;
typedef struct { fxh_strand *s; int slot; } fxh_wjob;

struct fxh_strand {
    int id;
    fxh_sf *S;
    fxh_lane ln;                           /* the engine context, its device buffers and the two page-locked output buffers (fxh_lanes.c) */
    pthread_t th_gpu, th_rd;
    pthread_mutex_t mu;
    pthread_cond_t cv;
    /* input slots: filled by the strand's reader in ticket order, emptied by its device thread */
    char *in[2];
    size_t in_len[2];
    uint64_t in_ticket[2];
    int in_full[2];
    int rd_pending;                        /* pread slices of the chunk being read that have not finished */
    fxh_rjob rjob[16];
    /* output slots: ln.out[0 .. nout), from the device thread to the copy tasks */
    size_t out_len[FXH_LANE_OUT_SLOTS];
    uint64_t out_off[FXH_LANE_OUT_SLOTS];
    int out_full[FXH_LANE_OUT_SLOTS];
    fxh_wjob wjob[FXH_LANE_OUT_SLOTS];
    uint64_t cur_ticket;
    fxh_totals tot;
    uint64_t chunks;
    double t_read, t_wait_in, t_gpu, t_wait_out, t_wait_off, t_release;
};

struct fxh_sf {
    FASTX *fx;
    const fxg_params *p;
    int in_fd, lpr, clip_auto;
    off_t *cut;                            /* chunk c is the input bytes [cut[c], cut[c + 1]) */
    uint64_t nchunks, in_total;
    size_t in_cap;
    uint64_t next_ticket;                  /* atomic: the next chunk nobody has taken */
    int nstrands, nread_slices, nout, release;
    fxh_strand *st;
    fxh_pool rpool, wpool;
    /* sizes -> offsets, the clipper's one read length, the sink's allocator state: all under mu / cv */
    pthread_mutex_t mu;
    pthread_cond_t cv;
    uint64_t *size, *offset;
    uint8_t *have;
    uint64_t scanned, scan_off, published;
    uint64_t clip_len;
    fxh_sink sink;
    fxh_rank *R;                           /* rank mode (fxh_rank.c): the chunks' text goes to this rank's arena instead of the sink; else NULL */
};

static void fxh_sf_abort(fxh_sf *S)
{
    FXH_ABORT_SET();
    for (int i = 0; i < S->nstrands; ++i) { pthread_mutex_lock(&S->st[i].mu); pthread_cond_broadcast(&S->st[i].cv); pthread_mutex_unlock(&S->st[i].mu); }
    pthread_mutex_lock(&S->mu); pthread_cond_broadcast(&S->cv); pthread_mutex_unlock(&S->mu);
}

/* ---- the sink ---- */
/* how far the allocation should reach now (mu held): everything, once every size is known; before that the output expected from the
 * chunks decided so far -- and, while there are none, a quarter of the input (at most 8 GB): the head start the device's start-up gives */
static uint64_t fxh_sink_goal(const fxh_sink *K)
{
    uint64_t goal;
    if (K->alloc_final_set) goal = K->alloc_final;
    else if (K->in_done >= K->ratio_after && K->in_done) {
        const long double r = (long double)K->out_done / (long double)K->in_done;
        goal = (uint64_t)(r * 1.02L * (long double)K->alloc_in_total) + K->window / 4;
    } else {
        goal = K->alloc_in_total / 4;
        if (goal > ((uint64_t)8 << 30)) goal = (uint64_t)8 << 30;
    }
    if (K->alloc_capped && !K->alloc_final_set) goal = K->need;      /* no room to run ahead in: exactly what the copies need */
    if (!K->alloc_final_set && goal < K->need) goal = K->need;
    if (goal > K->map_len) goal = K->map_len;
    return goal;
}

/* The allocator.  Allocation and copies exclude each other (the gate: fallocate() exclusive, every copied megabyte shared, the allocator preferred),
 * and the allocator is EAGER: it runs ahead of the copies towards the expected size of the output whenever it gets the file.  What it allocates before
 * the first chunk comes back from the device costs nothing, and the sooner it is through, the longer the copies have the file to themselves at full
 * parallelism.  (Measured alternative: copies first while their pages exist, the allocator only in the sink's idle moments and with priority when a
 * copy waits for pages -- 45 against 53-56 Mreads/s: the sink then spends the run switching, each switch waiting for the running copies to drain;
 * profiles/r05/g_e2e_one_file_copies_first.txt.) */
static void *fxh_sink_alloc_main(void *arg)
{
    fxh_sink *K = (fxh_sink *)arg;
    pthread_mutex_lock(K->mu);
    while (!K->alloc_stop && !FXH_ABORTED() && !K->alloc_errno) {
        const uint64_t goal = fxh_sink_goal(K);
        if (K->alloc_end >= goal) {
            if (K->alloc_final_set) break;                   /* the whole output has its pages */
            /* A tool that keeps little: the head start (a quarter of the input, made before anything was known) is several times what the output will take.
             * Those pages go back NOW, in the shadow of the run, instead of in the ftruncate() at its end, which the caller waits for.  What stays -- the
             * estimate plus a window -- lies above every byte a copy can be holding: off + len <= bytes decided so far <= the estimate. */
            if (K->mapped && !K->keep_surplus && K->in_done >= K->ratio_after && K->in_done && K->alloc_end > 2 * goal + K->window) {
                const uint64_t keep = (goal + K->window + 4095u) & ~(uint64_t)4095u, end = K->alloc_end;
                K->alloc_end = keep;                         /* first: nobody starts a copy beyond it from here on */
                pthread_mutex_unlock(K->mu);
                pthread_rwlock_wrlock(&K->gate);
                const double t0 = fxh_now();
                (void)fallocate(K->out_fd, FALLOC_FL_PUNCH_HOLE | FALLOC_FL_KEEP_SIZE, (off_t)keep, (off_t)(end - keep));      /* (if it fails the pages stay until the end, as before) */
                const double dt = fxh_now() - t0;
                pthread_rwlock_unlock(&K->gate);
                pthread_mutex_lock(K->mu);
                K->t_alloc += dt; K->given_back += end - keep;
                continue;
            }
            pthread_cond_wait(K->cv, K->mu);
            continue;
        }
        const uint64_t a = K->alloc_end;
        uint64_t step = goal - a < K->window ? goal - a : K->window;
        step = (step + 4095u) & ~(uint64_t)4095u;
        if (a + step > K->map_len) step = K->map_len - a;
        pthread_mutex_unlock(K->mu);
        pthread_rwlock_wrlock(&K->gate);                     /* no copy faults on the file while its pages are being made */
        const double t0 = fxh_now();
        int rc;
        do rc = fallocate(K->out_fd, 0, (off_t)a, (off_t)step); while (rc != 0 && errno == EINTR);
        const int e = rc != 0 ? errno : 0;
        const double dt = fxh_now() - t0;
        pthread_rwlock_unlock(&K->gate);
        pthread_mutex_lock(K->mu);
        K->t_alloc += dt; K->alloc_calls++;
        /* ENOSPC on pages nobody has asked for yet (the head start is a guess made before any output size is known; a filter that keeps 1 % needs a fraction
         * of it) is not the run's problem: stop running ahead and fail only when a copy really cannot get its pages (advisor, round 5) */
        if (e == ENOSPC && a >= K->need && !K->alloc_final_set && !K->alloc_capped) K->alloc_capped = 1;
        else if (e) K->alloc_errno = e; else K->alloc_end = a + step;
        pthread_cond_broadcast(K->cv);
    }
    pthread_mutex_unlock(K->mu);
    return NULL;
}

/* (mu held) what fxh_sf_publish feeds the sink: so much more input has been decided, and came to so much output */
static void fxh_sink_progress(fxh_sink *K, uint64_t in_bytes, uint64_t out_bytes) { K->in_done += in_bytes; K->out_done += out_bytes; }
/* (mu held) the exact size of the output is known */
static void fxh_sink_set_final(fxh_sink *K, uint64_t total) { K->alloc_final = total; K->alloc_final_set = 1; }

/* `len` bytes to offset `off` of the file: a copy into the mapping once their pages exist, or a positional write.  -1: they cannot get there (no room for
 * the pages -- the one-stream run meets the same wall and reports it the way it always did, with the output it got that far --, or, which cannot
 * happen, beyond the mapping: 8/7 of the input bounds the output): the caller abandons the run */
static int fxh_sink_write_at(fxh_sink *K, const char *src, size_t len, uint64_t off)
{
    double t0 = fxh_now(), t_wait = 0;
    int rc = 0;
    if (len && K->mapped && off + len > K->map_len) rc = -1;
    else if (len && K->mapped) {
        pthread_mutex_lock(K->mu);
        while (K->alloc_end < off + len && !K->alloc_errno && !FXH_ABORTED()) {
            if (K->need < off + len) { K->need = off + len; pthread_cond_broadcast(K->cv); }
            pthread_cond_wait(K->cv, K->mu);
        }
        const int e = K->alloc_errno;
        pthread_mutex_unlock(K->mu);
        t_wait = fxh_now() - t0;
        if (e) rc = -1;
        else if (!FXH_ABORTED()) {
            /* the whole buffer under one hold of the gate.  The allocator is preferred, so the sink strictly alternates: a window of pages, then
             * EVERY copy that has piled up meanwhile side by side (copies are only fast many at a time), then the next window.  (A megabyte per
             * hold let the allocator in sooner and the copies trickle: 48.7 against 54.6 Mreads/s, profiles/r05/h_e2e_one_file_piecewise.txt.) */
            const double tw = fxh_now();
            pthread_rwlock_rdlock(&K->gate);
            t_wait += fxh_now() - tw;
            memcpy(K->map + off, src, len);
            /* the pages stay in the file; only this process's view of them goes, now and by this thread, instead of at exit and by one */
            const uint64_t a = (off + 4095u) & ~(uint64_t)4095u, b = (off + len) & ~(uint64_t)4095u;
            if (b > a) (void)madvise(K->map + a, (size_t)(b - a), MADV_DONTNEED);
            pthread_rwlock_unlock(&K->gate);
        }
    } else if (len) {
        size_t done = 0;
        while (done < len && !FXH_ABORTED()) {
            const ssize_t k = pwrite(K->out_fd, src + done, len - done, (off_t)(off + done));
            if (k < 0) { if (errno == EINTR) continue; err(1, "writing output failed"); }
            done += (size_t)k;
        }
    }
    const double dt = fxh_now() - t0 - t_wait;
    pthread_mutex_lock(K->mu); K->t_copy += dt; K->t_copy_wait += t_wait; pthread_mutex_unlock(K->mu);
    return rc;
}

/* the sink of `w0`'s file: a tmpfs file written from offset 0 gets the gated mapping, everything else positional writes.  The allocator starts HERE, before
 * the caller looks for its device or makes a context.  in_total: this process's input; rank 0 of a rank job (ranked, rank) allocates for job_in_total. */
static void fxh_sink_open(fxh_sink *K, pthread_mutex_t *mu, pthread_cond_t *cv, const struct fxh_writer *w0, const char *name, uint64_t in_total, int ranked, int rank, uint64_t job_in_total)
{
    struct statfs fs;
    K->mu = mu; K->cv = cv; K->out_fd = w0->fd;
    const char *sk = getenv("FXH_ONE_FILE_SINK");        /* "map" | "pwrite": force one (tests) */
    int want_map = sk ? strcmp(sk, "map") == 0 : (fstatfs(w0->fd, &fs) == 0 && (unsigned long)fs.f_type == (unsigned long)TMPFS_MAGIC);
    if (w0->off != 0) want_map = 0;
    K->alloc_in_total = in_total;
    K->window = (uint64_t)fxh_env_long("FXH_ONE_FILE_WINDOW_MB", 128, 1, 1 << 16) << 20;
    K->ratio_after = (uint64_t)fxh_env_long("FXH_ONE_FILE_RATIO_MB", 64, 0, 1 << 20) << 20;
    K->keep_surplus = getenv("FXH_ONE_FILE_KEEP_SURPLUS") != NULL;
    if (want_map && ranked) {
        /* A rank job: the ranks' text stays in HBM until the exchange, and then every rank wants the file at once -- through the one inode lock if the pages
         * still have to be made.  So rank 0 makes the JOB's pages meanwhile: the same eager allocator, alone on the file (nobody copies before the exchange),
         * towards the output expected from the WHOLE input at rank 0's own measured ratio, to the exact size once the exchange has said it.  The ranks then
         * copy into pages that exist, each through a mapping of its own slice (separate processes: separate page tables). */
        want_map = 0;
        if (rank == 0) {
            K->alloc_in_total = job_in_total;
            K->map_len = (fxh_format_file_bound(&g_fmt, job_in_total) + 4095u) & ~(uint64_t)4095u;
            if (fallocate(w0->fd, 0, 0, 4096) == 0) {
                K->prealloc = 1; K->alloc_end = 4096;
                pthread_rwlock_init(&K->gate, NULL);
                if (pthread_create(&K->th_alloc, NULL, fxh_sink_alloc_main, K) != 0) err(1, "pthread_create");
            }
        }
    }
    if (want_map) {
        K->map_len = (fxh_format_file_bound(&g_fmt, in_total) + 4095u) & ~(uint64_t)4095u;      /* an empty third line still gets its '+': at most 8/7 of the input */
        void *m = MAP_FAILED;
        if (ftruncate(w0->fd, (off_t)K->map_len) == 0) m = mmap(NULL, (size_t)K->map_len, PROT_READ | PROT_WRITE, MAP_SHARED, w0->fd, 0);
        if (m != MAP_FAILED && fallocate(w0->fd, 0, 0, 4096) == 0) {
            K->map = (char *)m; K->mapped = 1; K->alloc_end = 4096;
            pthread_rwlockattr_t ra;
            pthread_rwlockattr_init(&ra);
            pthread_rwlockattr_setkind_np(&ra, PTHREAD_RWLOCK_PREFER_WRITER_NONRECURSIVE_NP);      /* the allocator is one against many: it goes first */
            pthread_rwlock_init(&K->gate, &ra);
            if (pthread_create(&K->th_alloc, NULL, fxh_sink_alloc_main, K) != 0) err(1, "pthread_create");      /* from the first millisecond on */
        } else {                                          /* no mapping or no fallocate() here: positional writes */
            if (m != MAP_FAILED) munmap(m, (size_t)K->map_len);
            if (ftruncate(w0->fd, 0) != 0) warn("%s", name);
        }
    }
}

/* the allocator has nothing more to wait for: the exact size is known (have_total; it goes on to it), or it stops where it is.  Joined; its errno. */
int fxh_sink_end(fxh_sink *K, int have_total, uint64_t total)
{
    pthread_mutex_lock(K->mu);
    if (have_total) fxh_sink_set_final(K, total); else K->alloc_stop = 1;
    pthread_cond_broadcast(K->cv);
    pthread_mutex_unlock(K->mu);
    if (K->mapped || K->prealloc) pthread_join(K->th_alloc, NULL);
    return K->alloc_errno;
}

/* the mapping goes; done: the file gets its size (what the estimate overshot goes back) */
static void fxh_sink_close(fxh_sink *K, int done, uint64_t total)
{
    if (!K->mapped) return;
    munmap(K->map, (size_t)K->map_len);
    if (done && ftruncate(K->out_fd, (off_t)total) != 0) err(1, "writing output failed");
}

/* ---- the strands ---- */
/* the lane's hook: the chunk's formatted size is known (fxh_lane_run, after the format kernels, before the download) */
static void fxh_sf_publish(fxh_lane *ln, uint64_t bytes)
{
    fxh_strand *s = (fxh_strand *)ln->owner;
    fxh_sf *S = s->S;
    const uint64_t t = s->cur_ticket;
    pthread_mutex_lock(&S->mu);
    S->size[t] = bytes; S->have[t] = 1; S->published++;
    fxh_sink_progress(&S->sink, (uint64_t)(S->cut[t + 1] - S->cut[t]), bytes);
    while (S->scanned < S->nchunks && S->have[S->scanned]) { S->offset[S->scanned] = S->scan_off; S->scan_off += S->size[S->scanned]; S->scanned++; }
    if (S->published == S->nchunks && !S->sink.prealloc) fxh_sink_set_final(&S->sink, S->scan_off);      /* (a rank job's size is the exchange's to say) */
    pthread_cond_broadcast(&S->cv);
    pthread_mutex_unlock(&S->mu);
}

/* rank mode: the chunk's text stays on the device -- copied behind the format kernels into the arena at the sum of the sizes before it (the local
 * offset: known once every earlier chunk of THIS rank has been decided).  1 = placed, -1 = the run is being abandoned. */
static int fxh_sf_place(fxh_lane *ln, uint64_t bytes)
{
    fxh_strand *s = (fxh_strand *)ln->owner;
    fxh_sf *S = s->S;
    const uint64_t t = s->cur_ticket;
    const double t0 = fxh_now();
    pthread_mutex_lock(&S->mu);
    while (S->scanned <= t && !FXH_ABORTED()) pthread_cond_wait(&S->cv, &S->mu);
    const uint64_t off = S->offset[t];
    pthread_mutex_unlock(&S->mu);
    s->t_wait_off += fxh_now() - t0;
    if (FXH_ABORTED()) return -1;
    if (!fxh_rank_place(S->R, ln, off, bytes)) { fxh_sf_abort(S); return -1; }
    return 1;
}

static void fxh_sf_read_task(void *arg)
{
    fxh_rjob *j = (fxh_rjob *)arg;
    fxh_strand *s = j->s;
    if (fxh_pread_full(j->fd, j->dst, j->n, j->off) < j->n) fxh_sf_abort(s->S);      /* the file shrank under the run */
    pthread_mutex_lock(&s->mu);
    s->rd_pending--;
    pthread_cond_broadcast(&s->cv);
    pthread_mutex_unlock(&s->mu);
}

static void *fxh_strand_reader(void *arg)
{
    fxh_strand *s = (fxh_strand *)arg;
    fxh_sf *S = s->S;
    for (int k = 0;; k ^= 1) {
        pthread_mutex_lock(&s->mu);
        while (s->in_full[k] && !FXH_ABORTED()) pthread_cond_wait(&s->cv, &s->mu);
        pthread_mutex_unlock(&s->mu);
        if (FXH_ABORTED()) break;
        const uint64_t t = __atomic_fetch_add(&S->next_ticket, 1, __ATOMIC_RELAXED);      /* drawn with a free buffer in hand: the smallest open chunk always has one */
        if (t >= S->nchunks) {
            pthread_mutex_lock(&s->mu);
            s->in_ticket[k] = FXH_TICKET_DONE; s->in_full[k] = 1;
            pthread_cond_broadcast(&s->cv);
            pthread_mutex_unlock(&s->mu);
            break;
        }
        const double t0 = fxh_now();
        const off_t off = S->cut[t];
        size_t n = (size_t)(S->cut[t + 1] - off);
        int ns = S->nread_slices;
        if ((size_t)ns > n / ((size_t)1 << 20)) ns = (int)(n / ((size_t)1 << 20));
        if (ns < 1) ns = 1;
        const size_t per = (n + (size_t)ns - 1) / (size_t)ns;
        pthread_mutex_lock(&s->mu); s->rd_pending = ns; pthread_mutex_unlock(&s->mu);
        for (int i = 0; i < ns; ++i) {
            const size_t o = (size_t)i * per;
            fxh_rjob *j = &s->rjob[i];
            j->s = s; j->fd = S->in_fd; j->dst = s->in[k] + o; j->off = off + (off_t)o; j->n = o >= n ? 0 : (n - o < per ? n - o : per);
            if (i + 1 < ns) fxh_pool_submit(&S->rpool, fxh_sf_read_task, j);
        }
        fxh_sf_read_task(&s->rjob[ns - 1]);                 /* the last slice on this thread */
        pthread_mutex_lock(&s->mu);
        while (s->rd_pending > 0) pthread_cond_wait(&s->cv, &s->mu);
        pthread_mutex_unlock(&s->mu);
        if (FXH_ABORTED()) break;
        if (t + 1 == S->nchunks && s->in[k][n - 1] != '\n') s->in[k][n++] = '\n';       /* the reference takes a last line without its newline (chomp.c:36-41) */
        s->t_read += fxh_now() - t0;
        pthread_mutex_lock(&s->mu);
        s->in_len[k] = n; s->in_ticket[k] = t; s->in_full[k] = 1;
        pthread_cond_broadcast(&s->cv);
        pthread_mutex_unlock(&s->mu);
    }
    return NULL;
}

static void fxh_sf_write_task(void *arg)
{
    fxh_wjob *j = (fxh_wjob *)arg;
    fxh_strand *s = j->s;
    if (fxh_sink_write_at(&s->S->sink, s->ln.out[j->slot], s->out_len[j->slot], s->out_off[j->slot]) != 0) fxh_sf_abort(s->S);
    pthread_mutex_lock(&s->mu);
    s->out_full[j->slot] = 0;
    pthread_cond_broadcast(&s->cv);
    pthread_mutex_unlock(&s->mu);
}

static void *fxh_strand_gpu(void *arg)
{
    fxh_strand *s = (fxh_strand *)arg;
    fxh_sf *S = s->S;
    fxh_lane *ln = &s->ln;
    fxh_lane_open_ctx(ln);
    for (int k = 0; k < 2; ++k) (void)fxg_host_register(ln->st.ctx, s->in[k], S->in_cap);      /* page-locked: the upload is real DMA */
    int j = 0;
    for (int k = 0;; k ^= 1) {
        double t0 = fxh_now();
        pthread_mutex_lock(&s->mu);
        while (!s->in_full[k] && !FXH_ABORTED()) pthread_cond_wait(&s->cv, &s->mu);
        const uint64_t t = s->in_ticket[k];
        const size_t len = s->in_len[k];
        pthread_mutex_unlock(&s->mu);
        s->t_wait_in += fxh_now() - t0;
        if (FXH_ABORTED() || t == FXH_TICKET_DONE) break;
        t0 = fxh_now();
        pthread_mutex_lock(&s->mu);
        while (!S->R && s->out_full[j] && !FXH_ABORTED()) pthread_cond_wait(&s->cv, &s->mu);
        pthread_mutex_unlock(&s->mu);
        s->t_wait_out += fxh_now() - t0;
        if (FXH_ABORTED()) break;
        t0 = fxh_now();
        ln->text_base = NULL; ln->text_cap = 0;
        ln->text = s->in[k]; ln->len = len; ln->records = FXH_RECORDS_UNKNOWN; ln->slot = j;
        s->cur_ticket = t;
        fxh_lane_run(ln);
        s->t_gpu += fxh_now() - t0;
        int ok = ln->handled;
        if (ok && S->clip_auto) {                            /* the clipper's lanes are exact while ALL reads have one length: every chunk the same one */
            pthread_mutex_lock(&S->mu);
            ok = ln->fixed_len && fxh_one_length(&S->clip_len, ln->fixed_len);
            pthread_mutex_unlock(&S->mu);
        }
        if (!ok) { fxh_sf_abort(S); break; }                 /* whatever it is, the one-stream run owns the reference's behaviour for it */
        fxh_add_counters(&s->tot, ln->ctr, ln->records, ln->lpr == 2 ? ln->weighted : NULL);
        s->chunks++;
        pthread_mutex_lock(&s->mu);                          /* the text is on the device: the reader may fill the buffer again */
        s->in_full[k] = 0;
        pthread_cond_broadcast(&s->cv);
        pthread_mutex_unlock(&s->mu);
        if (S->R) continue;                              /* rank mode: the text is in the arena already (fxh_sf_place) */
        t0 = fxh_now();
        pthread_mutex_lock(&S->mu);
        while (S->scanned <= t && !FXH_ABORTED()) pthread_cond_wait(&S->cv, &S->mu);
        const uint64_t off = S->offset[t];
        pthread_mutex_unlock(&S->mu);
        s->t_wait_off += fxh_now() - t0;
        if (FXH_ABORTED()) break;
        pthread_mutex_lock(&s->mu);
        s->out_len[j] = ln->out_len; s->out_off[j] = off; s->out_full[j] = 1;
        pthread_cond_broadcast(&s->cv);
        pthread_mutex_unlock(&s->mu);
        s->wjob[j].s = s; s->wjob[j].slot = j;
        fxh_pool_submit(&S->wpool, fxh_sf_write_task, &s->wjob[j]);
        j = (j + 1) % S->nout;
    }
    pthread_mutex_lock(&s->mu);                              /* the strand's text is in the file (or the run is over) before its buffers may go */
    for (;;) {
        int busy = 0;
        for (int q = 0; q < S->nout; ++q) busy |= s->out_full[q];
        if (!busy || FXH_ABORTED()) break;
        pthread_cond_wait(&s->cv, &s->mu);
    }
    pthread_mutex_unlock(&s->mu);
    if (S->release && !FXH_ABORTED()) {
        const double t0 = fxh_now();
        for (int k = 0; k < 2; ++k) (void)fxg_host_unregister(ln->st.ctx, s->in[k]);
        fxh_lane_release(ln);
        s->t_release = fxh_now() - t0;
    }
    return NULL;
}

/* ---- the cuts ---- */
/* the cuts, found side by side before anything runs */
typedef struct { int fd, lpr; off_t start, size; size_t chunk; off_t *cut; uint64_t c0, c1; int bad; } fxh_cutjob;
static void *fxh_cut_main(void *arg)
{
    fxh_cutjob *j = (fxh_cutjob *)arg;
    for (uint64_t c = j->c0; c < j->c1 && !j->bad; ++c) {
        const off_t from = j->start + (off_t)(c * (uint64_t)j->chunk);
        off_t f = fxh_find_cut(j->fd, from, j->size, j->lpr, (size_t)64 << 10);
        if (f < 0) f = fxh_find_cut(j->fd, from, j->size, j->lpr, 0);
        if (f < 0) f = j->size;                              /* no record starts behind it: the chunk in front runs to the end (and is then checked like any other) */
        j->cut[c] = f;
    }
    return NULL;
}

/* The chunk boundaries of one byte range [lo, hi) of the input: cut[0] = lo, cut[n] = hi, every cut in between the start of a record (found by pattern, several
 * threads).  Returns the cuts (caller frees) with *nchunks_io / *longest set, or NULL when the range cannot be cut into chunks of about `chunk` bytes (records
 * longer than a chunk, no record pattern in reach): such an input runs as one stream. */
static off_t *fxh_range_cuts(int fd, int lpr, off_t lo, off_t hi, off_t file_size, size_t chunk, uint64_t *nchunks_io, size_t *longest_out)
{
    uint64_t nchunks = *nchunks_io;
    off_t *cut = (off_t *)calloc(nchunks + 1, sizeof(off_t));
    if (!cut) err(1, "out of memory");
    cut[0] = lo; cut[nchunks] = hi;
    fxh_cutjob cj[8];
    pthread_t th[8];
    const int nt = nchunks > 64 ? 8 : 1;
    for (int i = 0; i < nt; ++i) {
        cj[i].fd = fd; cj[i].lpr = lpr; cj[i].start = lo; cj[i].size = file_size; cj[i].chunk = chunk; cj[i].cut = cut; cj[i].bad = 0;
        cj[i].c0 = 1 + (nchunks - 1) * (uint64_t)i / (uint64_t)nt; cj[i].c1 = 1 + (nchunks - 1) * (uint64_t)(i + 1) / (uint64_t)nt;
    }
    for (int i = 1; i < nt; ++i) if (pthread_create(&th[i], NULL, fxh_cut_main, &cj[i]) != 0) err(1, "pthread_create");
    fxh_cut_main(&cj[0]);
    for (int i = 1; i < nt; ++i) pthread_join(th[i], NULL);
    int bad = 0;
    for (int i = 0; i < nt; ++i) bad |= cj[i].bad;
    while (!bad && nchunks > 1 && cut[nchunks - 1] >= hi) nchunks--;      /* a last nominal cut whose record start is the range's end: no chunk there */
    cut[nchunks] = hi;
    size_t longest = 0;
    for (uint64_t c = 0; c < nchunks && !bad; ++c) {
        if (cut[c + 1] <= cut[c]) bad = 1;               /* records longer than a chunk, or no record pattern in reach: one stream */
        else if ((size_t)(cut[c + 1] - cut[c]) > longest) longest = (size_t)(cut[c + 1] - cut[c]);
    }
    if (bad || longest > chunk + chunk / 2) { free(cut); return NULL; }
    *nchunks_io = nchunks; *longest_out = longest;
    return cut;
}


/* ---- the attempt ---- */
/* what is to be run: the unread input [start, file_size) of the file, this process's byte range of it, and that range's chunks */
typedef struct { off_t start, file_size, my_start, my_end; off_t *cut; uint64_t nchunks; size_t longest; } fxh_plan;

/* is this command line the one-file run's?  Sets where the unread input begins in the file, and the file's size. */
static int fxh_one_file_eligible(const FASTX *fx, const fxg_params *p, int ranked, fxh_plan *pl)
{
    const struct fxh_reader *rd = fx->reader;
    const struct fxh_writer *w0 = fx->writer;
    struct stat sb, ob;
    const char *sw = getenv("FXH_ONE_FILE");
    if (sw && atoi(sw) == 0) return 0;
    if (!fxh_attempt_eligible(fx, p, &sb)) return 0;
    if (!w0 || w0->fd < 0 || !w0->positional || w0->len != 0 || fstat(w0->fd, &ob) != 0 || !S_ISREG(ob.st_mode)) return 0;
    if (w0->off != 0) return 0;                  /* (the strands and the rank drain place their bytes counted from the file's first byte: a writer that does not start there runs as one stream) */
    if (ob.st_dev == sb.st_dev && ob.st_ino == sb.st_ino) return 0;
    const off_t pos = lseek(rd->fd, 0, SEEK_CUR);
    if (pos < 0) return 0;
    pl->start = pos - (off_t)(rd->end - rd->beg); pl->file_size = sb.st_size;      /* where the unread input begins in the file */
    if (pl->start < 0 || pl->start >= pl->file_size) return 0;
    /* from about half a gigabyte on the strands pay for their contexts: 0.64 GB 0.193 against 0.197 s, 1.3 GB 0.246 / 0.197, 2.6 GB 0.361 / 0.239,
     * 5.1 GB 0.660 / 0.364, 20.5 GB 1.79 / 1.13 (one stream / this run, profiles/r05/l_e2e_one_file_by_size.txt) */
    const long min_mb = fxh_env_long("FXH_ONE_FILE_MIN_MB", 512, 0, 1 << 30);
    if (!ranked && (long long)(pl->file_size - pl->start) < ((long long)min_mb << 20)) return 0;
    return 1;
}

/* Whether a job runs by ranks is decided HERE, before any rank meets another, and it must be the same decision in every rank: a rank that left
 * on a check of its own range alone would leave the others waiting in the rendezvous (the communicator has no watch of its own).  So every rank
 * looks at EVERY rank's range -- the same cuts, the same verdict (a few thousand small reads for a file of 100 GB) -- and keeps the cuts of its own.
 * Rank g takes byte range g of `world` (cut at record starts found by pattern, as the parts of fxh_parts.c; every rank computes the same cuts). */
static int fxh_world_cuts(int fd, int lpr, size_t chunk, int rank, int world, fxh_plan *pl)
{
    off_t lo = pl->start;
    for (int g = 1; g <= world; ++g) {
        const off_t hi = g == world ? pl->file_size
                                    : fxh_find_cut(fd, pl->start + (off_t)((unsigned long long)(pl->file_size - pl->start) * (unsigned)g / (unsigned)world), pl->file_size, lpr, 0);
        uint64_t n = hi > lo ? ((uint64_t)(hi - lo) + chunk - 1) / chunk : 0;
        size_t longest = 0;
        /* an input too small for that many ranks, or some rank's range cannot be cut: no rank starts, rank 0 runs the input as one stream */
        off_t *c = hi < 0 || hi <= lo ? NULL : fxh_range_cuts(fd, lpr, lo, hi, pl->file_size, chunk, &n, &longest);
        if (!c) { free(pl->cut); pl->cut = NULL; return 0; }
        if (g - 1 == rank) { pl->my_start = lo; pl->my_end = hi; pl->cut = c; pl->nchunks = n; pl->longest = longest; } else free(c);
        lo = hi;
    }
    return 1;
}

/* the chunks of this process's range; afterwards pl->longest is the buffer a chunk needs */
static int fxh_one_file_cuts(int fd, int lpr, int rank, int world, int ranked, fxh_plan *pl)
{
    size_t chunk = (size_t)fxh_env_long("FXH_STRAND_KB", 0, 0, 1 << 22) << 10;     /* (tests: chunks of a few KB) */
    if (!chunk) chunk = (size_t)fxh_env_long("FXH_STRAND_MB", 16, 1, 1024) << 20;      /* 16 MB: 54.6 against 51.7 Mreads/s with 8 (profiles/r05/f_e2e_one_file_timeline.txt) */
    pl->my_start = pl->start; pl->my_end = pl->file_size;
    if (world > 1) return fxh_world_cuts(fd, lpr, chunk, rank, world, pl);
    pl->nchunks = ((uint64_t)(pl->my_end - pl->my_start) + chunk - 1) / chunk;
    if (pl->nchunks < 2 && !ranked) return 0;
    pl->cut = fxh_range_cuts(fd, lpr, pl->my_start, pl->my_end, pl->file_size, chunk, &pl->nchunks, &pl->longest);
    return pl->cut != NULL;
}

/* pools, the rank's context and communicator (rank mode), the strands: started, run, joined.  Returns whether the run is to be abandoned. */
static int fxh_strands_run(fxh_sf *S, const int *dev, int ndev, int ranked, int rank, int world)
{
    const fxg_params *p = S->p;
    FASTX *fx = S->fx;
    /* Four strands per GPU, four preads in flight each (16 reading threads: what one tmpfs file gives, 31 GB/s).  Four feed the sink as well as six or eight -- it is the
     * sink that bounds a run whose output is large -- and cost less to start and to take down: 64 M reads 60.8 / 59.3 / 54.9 Mreads/s with 4 / 6 / 8 strands, the child gone
     * 1.04 / 1.06 / 1.15 s after the fork (profiles/r05/r_e2e_one_file_strands.txt); 2.6 GB of input 0.239 against 0.268 s (l_). */
    int per = (int)fxh_env_long("FXH_STRANDS", 4, 1, FXH_MAX_STRANDS);
    int ns = per * ndev;
    if (ns > FXH_MAX_STRANDS) ns = FXH_MAX_STRANDS;
    if ((uint64_t)ns > S->nchunks) ns = (int)S->nchunks;
    S->nstrands = ns;
    S->nread_slices = (int)fxh_env_long("FXH_STRAND_READERS", 4, 1, 16);
    S->st = (fxh_strand *)calloc((size_t)ns, sizeof(fxh_strand));
    if (!S->st) err(1, "out of memory");
    fxh_pool_start(&S->rpool, (int)fxh_env_long("FXH_IO_THREADS", ns * (S->nread_slices - 1) > 0 ? ns * (S->nread_slices - 1) : 1, 1, 64), (unsigned)(ns * 16));
    /* copies into the mapping: one thread per output buffer; positional writes: ONE stream (more of them only queue at the inode lock, 27 against 40 Mreads/s) */
    S->release = (int)fxh_env_long("FXH_STRAND_RELEASE", 0, 0, 1);
    S->nout = (int)fxh_env_long("FXH_STRAND_OUT_SLOTS", 4, 2, FXH_LANE_OUT_SLOTS);      /* output buffers per strand: what the strands can put aside while the allocator has the file */
    fxh_pool_start(&S->wpool, S->sink.mapped ? (int)fxh_env_long("FXH_COPY_THREADS", 16, 1, 64) : 1, (unsigned)(S->nout * ns));
    const int revcomp = (p->stages & (FXG_STAGE_REVCOMP | FXG_STAGE_MASK)) != 0;
    if (ranked) S->R = fxh_rank_open(fx, rank, world, dev[0], S->sink.out_fd, S->in_total);
    for (int i = 0; i < ns; ++i) {
        fxh_strand *s = &S->st[i];
        s->id = i; s->S = S;
        pthread_mutex_init(&s->mu, NULL); pthread_cond_init(&s->cv, NULL);
        for (int k = 0; k < 2; ++k) if (posix_memalign((void **)&s->in[k], 4096, S->in_cap) != 0) err(1, "out of memory");
        fxh_lane *ln = &s->ln;
        ln->id = i; ln->device = dev[i % ndev]; ln->p = p; ln->revcomp = revcomp;
        ln->fwd_start = (p->stages & FXG_STAGE_FTRIM) && p->ft_first > 1 ? (uint32_t)p->ft_first - 1u : 0u;
        ln->qoffset = fx->fastq_ascii_quality_offset;
        ln->reverse = (p->stages & FXG_STAGE_REVCOMP) != 0; ln->lpr = S->lpr; ln->has_q = fx->read_fastq; ln->out_fasta = !fx->write_fastq;
        ln->clip_guard = S->clip_auto;
        ln->on_size = fxh_sf_publish; ln->owner = s;
        if (ranked) ln->on_place = fxh_sf_place;
        if (pthread_create(&s->th_rd, NULL, fxh_strand_reader, s) != 0) err(1, "pthread_create");      /* reading starts while the device does */
    }
    for (int i = 0; i < ns; ++i) if (pthread_create(&S->st[i].th_gpu, NULL, fxh_strand_gpu, &S->st[i]) != 0) err(1, "pthread_create");
    for (int i = 0; i < ns; ++i) { pthread_join(S->st[i].th_gpu, NULL); }
    int bad = FXH_ABORTED();
    if (bad) fxh_sf_abort(S);                    /* (readers that were between two checks) */
    for (int i = 0; i < ns; ++i) pthread_join(S->st[i].th_rd, NULL);
    fxh_pool_stop(&S->rpool);
    fxh_pool_stop(&S->wpool);
    if (!bad && S->scanned != S->nchunks) bad = 1;      /* (every thread that moved it has been joined) */
    return bad;
}

/* Abandoned.  Every thread has been joined, the contexts go, the file is emptied through its own descriptor -- which the parent
 * shares -- and the process leaves with _exit: no exit handler of this half-finished attempt gets to run. */
static void fxh_one_file_abandon(fxh_sf *S, FASTX *fx, int rank, int timing)
{
    struct fxh_writer *w0 = fx->writer;
    for (int i = 0; i < S->nstrands; ++i) if (S->st[i].ln.st.ctx) fxg_ctx_destroy(S->st[i].ln.st.ctx);
    fxh_sink_close(&S->sink, 0, 0);
    if (S->R) fxh_rank_close(S->R);
    w0->len = 0;
    if (rank == 0 && (ftruncate(w0->fd, w0->off) != 0 || lseek(w0->fd, w0->off, SEEK_SET) < 0)) warn("%s", fx->output_file_name);
    if (timing) fprintf(stderr, "fxh timing one file: abandoned, contexts destroyed, output emptied\n");
    fflush(NULL);
    _exit(FXH_EXIT_ABANDON);
}

/* FXH_TIMING: the strands' lines, the run's, the rank's (t: the child's start, the start and the end of the placement) */
static void fxh_one_file_report(const fxh_sf *S, int ndev, const double t[3], uint64_t total, const fxh_plan *pl)
{
    const fxh_sink *K = &S->sink;
    const int ns = S->nstrands;
    double rd_s = 0, gpu_s = 0, win = 0, wout = 0, woff = 0, init = 0, rel = 0;
    for (int i = 0; i < ns; ++i) {
        const fxh_strand *s = &S->st[i];
        rd_s += s->t_read; gpu_s += s->t_gpu; win += s->t_wait_in; wout += s->t_wait_out; woff += s->t_wait_off; init += s->ln.t_init; rel += s->t_release;
        if (s->ln.t_call[7] > 0)
            fprintf(stderr, "fxh timing strand %d: %.0f chunks, ms per chunk: h2d %.3f index %.3f pack %.3f pipeline %.3f counters %.3f format %.3f d2h+sync %.3f\n", i, s->ln.t_call[7],
                    1e3 * s->ln.t_call[0] / s->ln.t_call[7], 1e3 * s->ln.t_call[1] / s->ln.t_call[7], 1e3 * s->ln.t_call[2] / s->ln.t_call[7], 1e3 * s->ln.t_call[3] / s->ln.t_call[7],
                    1e3 * s->ln.t_call[4] / s->ln.t_call[7], 1e3 * s->ln.t_call[5] / s->ln.t_call[7], 1e3 * s->ln.t_call[6] / s->ln.t_call[7]);
    }
    fprintf(stderr, "fxh timing one file (%d strands on %d GPU(s), %llu chunks, sink %s): run %.3f s (set-up %.3f, placement %.3f); summed over strands: context %.3f read %.3f wait-input %.3f device %.3f wait-outbuf %.3f wait-offset %.3f release %.3f; "
                    "sink: %llu fallocate calls %.3f s (to %.2f GB for %.2f GB of output, %.1f MB given back on the way), copies %.3f s + %.3f s at the gate (summed over %d threads)\n",
            ns, ndev, (unsigned long long)S->nchunks, K->mapped ? "gated mapping" : "pwrite", fxh_now() - t[0], t[1] - t[0], t[2] - t[1], init, rd_s, win, gpu_s, wout, woff, rel,
            (unsigned long long)K->alloc_calls, K->t_alloc, 1e-9 * (double)K->alloc_end, 1e-9 * (double)total, 1e-6 * (double)K->given_back, K->t_copy, K->t_copy_wait, S->wpool.nth);
    if (S->R) fxh_rank_report(S->R, (long long)pl->my_start, (long long)pl->my_end, S->scan_off);
    if (K->prealloc) fprintf(stderr, "fxh timing rank 0: the job's pages: %llu fallocate calls, %.3f s\n", (unsigned long long)K->alloc_calls, K->t_alloc);
}

/* the child of the fork: open the sink, place, run the strands, finish (a rank: with the job), then either abandon or report */
static int fxh_one_file_child(FASTX *fx, const fxg_params *p, fxh_totals *tot, int rank, int world, int ranked, const fxh_plan *pl)
{
    struct fxh_writer *w0 = fx->writer;
    const int timing = getenv("FXH_TIMING") != NULL;
    double t[3] = { fxh_now(), 0, 0 };
    static fxh_sf S_;                            /* (static: zeroed, and alive for the whole child) */
    fxh_sf *S = &S_;
    S->fx = fx; S->p = p; S->in_fd = fx->reader->fd; S->lpr = fx->read_fastq ? 4 : 2; S->cut = pl->cut; S->nchunks = pl->nchunks; S->in_total = (uint64_t)(pl->my_end - pl->my_start);
    S->in_cap = (pl->longest + 4096 + 4095) & ~(size_t)4095;
    S->clip_auto = (p->stages & FXG_STAGE_CLIP) != 0 && getenv("FXH_CLIP_PARALLEL") == NULL;
    pthread_mutex_init(&S->mu, NULL); pthread_cond_init(&S->cv, NULL);
    S->size = (uint64_t *)calloc(S->nchunks, sizeof(uint64_t)); S->offset = (uint64_t *)calloc(S->nchunks, sizeof(uint64_t)); S->have = (uint8_t *)calloc(S->nchunks, 1);
    if (!S->size || !S->offset || !S->have) err(1, "out of memory");

    int dev[FXH_MAX_LANES];
    int ndev = fxh_device_list(dev, FXH_MAX_LANES);
    if (ranked) { dev[0] = fxh_rank_device(rank, dev[0]); ndev = 1; }
    fxh_sink_open(&S->sink, &S->mu, &S->cv, w0, fx->output_file_name, S->in_total, ranked, rank, (uint64_t)(pl->file_size - pl->start));

    /* Placement AFTER the allocator has started: finding the GPU's NUMA node can take 50 ms (the runtime has to be asked where visibility variables hide the
     * topology), which is a gigabyte of pages at the allocator's rate.  The allocator thread then follows the calling thread onto the GPU's node. */
    cpu_set_t cpus_before;
    t[1] = fxh_now();
    if (ndev == 1) (void)fxh_bind_near_device(dev[0], &cpus_before);      /* buffers and the output's pages are touched (and page-locked) on the GPU's node; every thread below inherits it */
    if (S->sink.mapped || S->sink.prealloc) { cpu_set_t now_set; if (sched_getaffinity(0, sizeof now_set, &now_set) == 0) (void)pthread_setaffinity_np(S->sink.th_alloc, sizeof now_set, &now_set); }
    t[2] = fxh_now();

    int bad = fxh_strands_run(S, dev, ndev, ranked, rank, world);
    if (!S->sink.prealloc) (void)fxh_sink_end(&S->sink, 0, 0);      /* (a rank job's allocator goes on until the exchange has said the size) */
    fxh_totals mine;
    memset(&mine, 0, sizeof mine);
    for (int i = 0; i < S->nstrands; ++i) fxh_totals_add(&mine, &S->st[i].tot);
    uint64_t total = S->scan_off;
    if (ranked) bad = fxh_rank_finish(S->R, fx, S->sink.prealloc ? &S->sink : NULL, &mine, S->scan_off, S->clip_auto, S->clip_len, bad, &total);      /* (from here on `mine` is the JOB's: rank 0 reports it) */
    if (bad) fxh_one_file_abandon(S, fx, rank, timing);
    fxh_sink_close(&S->sink, 1, total);
    w0->off += (off_t)total;                     /* the writer closes with the descriptor where a write() stream would have left it */
    *tot = mine;
    fx->num_input_sequences = tot->input_sequences; fx->num_input_reads = tot->input_reads;
    fx->num_output_sequences = tot->output_sequences; fx->num_output_reads = tot->output_reads;
    if (timing) fxh_one_file_report(S, ndev, t, total, pl);
    if (rank > 0) {                              /* the job's report is rank 0's */
        if (w0->fd != STDOUT_FILENO) close(w0->fd);
        w0->fd = -1;
        fflush(NULL);
        _exit(0);
    }
    return 0;
}

static int fxh_one_file_attempt(FASTX *fx, const fxg_params *p, fxh_totals *tot, const int rank, const int world)
{
    const int ranked = world > 1 || getenv("FXH_RANK_MODE") != NULL;      /* (FXH_RANK_MODE=1: the rank path with a world of one -- the GPU tier's way to the real RCCL) */
    fxh_plan pl;
    memset(&pl, 0, sizeof pl);
    if (!fxh_one_file_eligible(fx, p, ranked, &pl)) return -1;
    if (!fxh_one_file_cuts(fx->reader->fd, fx->read_fastq ? 4 : 2, rank, world, ranked, &pl)) return -1;
    const int forked = fxh_attempt_fork("one file");     /* the frame of fxh_parts.c: the attempt runs in a child, anything irregular abandons it to one stream */
    if (forked == 0) return fxh_one_file_child(fx, p, tot, rank, world, ranked, &pl);
    /* forked < 0: no process to run the attempt in.  Alone, that means one stream.  In a job the other ranks are on their way to the rendezvous: this rank cannot
     * take part (no fork over a live runtime), so it says so and ends the job -- the others' watch (around the rendezvous, fxh_rank.c) ends them. */
    if (forked < 0 && world > 1) err(1, "rank %d of %d: fork", rank, world);
    free(pl.cut);
    if (forked > 0 && rank == 0 && ftruncate(fx->writer->fd, fx->writer->off) != 0) warn("%s", fx->output_file_name);      /* abandoned (no rank has written: the file is rank 0's again) */
    return -1;
}

/* 0 = done (in the child of the attempt's fork: the caller goes on to print its reports); -1 = run as one stream (not eligible, or the attempt was abandoned).
 * FXH_WORLD = n > 1 with FXH_RANK = 0 .. n-1: n processes, one per GPU (FXG_DEVICE, default rank mod #GPUs), started by any launcher -- or by hand --
 * with the SAME command line; they meet through FXH_RENDEZVOUS (default: <output>.rdv).  Rank 0 prints the -v report of the whole job. */
int fxh_run_one_file(FASTX *fx, const fxg_params *p, fxh_totals *tot)
{
    const int world = (int)fxh_env_long("FXH_WORLD", 1, 1, 4096), rank = (int)fxh_env_long("FXH_RANK", 0, 0, world - 1);
    if (world > 1 && rank == 0) {
        /* A rendezvous record that a killed run of the same command left under the same name (no FXG_COMM_JOB: the job token is 0 both times) must be gone before
         * any other rank of THIS job can look at it: rank 0 removes the name here, first thing -- fxg_comm_create does it again, but only after the runtime and
         * RCCL have started, seconds during which a rank that is already polling could read the dead job's id twice unchanged and take it (advisor, round 5). */
        char rdv[PATH_MAX + 16];
        fxh_rendezvous_name(fx, rdv, sizeof rdv);
        (void)unlink(rdv);
    }
    const int rc = fxh_one_file_attempt(fx, p, tot, rank, world);
    if (world > 1 && rc != 0 && rank > 0) {      /* not a job for ranks (a pipe, a tiny input) or abandoned: rank 0 runs it as one stream, the reference's way */
        if (fx->writer && fx->writer->fd >= 0 && fx->writer->fd != STDOUT_FILENO) close(fx->writer->fd);
        fx->writer->fd = -1;
        fflush(NULL);
        _exit(0);
    }
    return rc;
}
