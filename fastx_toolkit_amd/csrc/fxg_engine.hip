// fxg_engine.hip -- host side of the C-ABI declared in include/fxg.h (gfx950 only).
#include "fxg_host.h"
#include "fxg_text.h"
#include "fxg_history.h"
#include "fxg_stats.h"
#include "fxg_fallback.h"
#include "fxg_barcode.h"
#include "fxg_reflow.h"
#include "fxg_uncollapse.h"
#include "fxg_nucchange.h"
#include "fxg_collapse.h"

extern "C" int fxg_abi_version(void) { return FXG_ABI_VERSION; }

extern "C" int fxg_ctx_create(int device_id, fxg_ctx **out)
{
    if (!out) return FXG_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device_id < 0 || device_id >= ndev) return FXG_E_HIP;
    fxg_ctx *c = (fxg_ctx *)calloc(1, sizeof(fxg_ctx));
    if (!c) return FXG_E_NOMEM;
    c->device = device_id;
    hipDeviceProp_t prop;
    if (hipSetDevice(device_id) != hipSuccess || hipGetDeviceProperties(&prop, device_id) != hipSuccess ||
        hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) { fxg_ctx_destroy(c); return FXG_E_HIP; }
    c->cus = prop.multiProcessorCount;
    c->stream = c->own_stream;
    c->knobs = fxg_knobs_read(FXG_KNOBS_CONTEXT);
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipMalloc((void **)&c->errflag, (FXG_CTRL_WORDS + FXG_TICKET_GROUPS * FXG_TICKET_STRIDE) * sizeof(u32)) != hipSuccess ||
        hipMalloc((void **)&c->counters_scratch, FXG_NCOUNTERS * sizeof(u64)) != hipSuccess) { fxg_ctx_destroy(c); return FXG_E_HIP; }
    *out = c;
    return FXG_OK;
}

// also the one way out of a fxg_ctx_create that failed half way: whatever exists by then is released, nothing else is touched
extern "C" void fxg_ctx_destroy(fxg_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)hipFree(c->status); (void)hipFree(c->errflag); (void)hipFree(c->counters_scratch);
    (void)hipFree(c->text_ws); (void)hipFree(c->text_state); (void)hipFree(c->fb_blk);
    (void)hipFree(c->hist_buf[0]); (void)hipFree(c->hist_buf[1]); (void)hipFree(c->hist_w); (void)hipFree(c->hist_ws); (void)hipFree(c->stats_ws); (void)hipFree(c->clip_ck);
    (void)hipFree(c->bc_tab); (void)hipFree(c->bc_ws); (void)hipFree(c->rf_ws); (void)hipFree(c->uc_ws); (void)hipFree(c->nc_res);
    if (c->cl) {
        (void)hipFree(c->cl->arena); (void)hipFree(c->cl->off); (void)hipFree(c->cl->cnt); (void)hipFree(c->cl->len); (void)hipFree(c->cl->slots);
        (void)hipFree(c->cl->tmp); (void)hipFree(c->cl->ord); (void)hipFree(c->cl->res);
        free(c->cl);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (int i = 0; i < FXG_KEV_RING; ++i) { if (c->kev0[i]) (void)hipEventDestroy(c->kev0[i]); if (c->kev1[i]) (void)hipEventDestroy(c->kev1[i]); }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    free(c);
}

extern "C" const char *fxg_last_error(const fxg_ctx *c) { return c ? c->err : "null context"; }

extern "C" int fxg_set_stream(fxg_ctx *c, void *s)
{
    if (!c) return FXG_E_INVALID;
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return FXG_OK;
}

extern "C" int fxg_sync(fxg_ctx *c)
{
    if (!c) return FXG_E_INVALID;
    FXG_HIP(c, hipStreamSynchronize(c->stream));
    return FXG_OK;
}

extern "C" int fxg_device_info(fxg_ctx *c, int *cus, size_t *total_mem, char *name, size_t cap)
{
    if (!c) return FXG_E_INVALID;
    hipDeviceProp_t prop;
    FXG_HIP(c, hipGetDeviceProperties(&prop, c->device));
    if (cus) *cus = prop.multiProcessorCount;
    if (total_mem) *total_mem = prop.totalGlobalMem;
    if (name && cap) snprintf(name, cap, "%s (%s)", prop.name, prop.gcnArchName);
    return FXG_OK;
}

extern "C" int fxg_malloc_device(fxg_ctx *c, size_t bytes, void **p)
{
    if (!c || !p) return FXG_E_INVALID;
    FXG_HIP(c, hipSetDevice(c->device));
    FXG_HIP(c, hipMalloc(p, bytes ? bytes : 16));
    return FXG_OK;
}
extern "C" int fxg_free_device(fxg_ctx *c, void *p) { if (!c) return FXG_E_INVALID; FXG_HIP(c, hipFree(p)); return FXG_OK; }
extern "C" int fxg_malloc_host(fxg_ctx *c, size_t bytes, void **p)
{
    if (!c || !p) return FXG_E_INVALID;
    FXG_HIP(c, hipHostMalloc(p, bytes ? bytes : 16, hipHostMallocPortable));   // usable by every GPU of a multi-GPU run
    return FXG_OK;
}
extern "C" int fxg_free_host(fxg_ctx *c, void *p) { if (!c) return FXG_E_INVALID; FXG_HIP(c, hipHostFree(p)); return FXG_OK; }
extern "C" int fxg_memcpy_h2d(fxg_ctx *c, void *d, const void *s, size_t n)
{
    if (!c) return FXG_E_INVALID;
    FXG_HIP(c, hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, c->stream));
    return FXG_OK;
}
extern "C" int fxg_memcpy_d2h(fxg_ctx *c, void *d, const void *s, size_t n)
{
    if (!c) return FXG_E_INVALID;
    FXG_HIP(c, hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, c->stream));
    return FXG_OK;
}
extern "C" int fxg_memset_device(fxg_ctx *c, void *d, int v, size_t n)
{
    if (!c) return FXG_E_INVALID;
    FXG_HIP(c, hipMemsetAsync(d, v, n, c->stream));
    return FXG_OK;
}

extern "C" int fxg_timer_start(fxg_ctx *c)
{
    if (!c) return FXG_E_INVALID;
    FXG_HIP(c, hipEventRecord(c->ev0, c->stream));
    return FXG_OK;
}
extern "C" int fxg_timer_stop(fxg_ctx *c, float *ms)
{
    if (!c || !ms) return FXG_E_INVALID;
    FXG_HIP(c, hipEventRecord(c->ev1, c->stream));
    FXG_HIP(c, hipEventSynchronize(c->ev1));
    FXG_HIP(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return FXG_OK;
}


int fxg_enqueue_finish_counters(fxg_ctx *c, const FxgKArgs &ka, u64 *counters)
{
    FXG_LAUNCH(c, fxg_kernel_finish_counters, 1, 64, 0, (const u64 *)ka.tally, ka.stages, (const u32 *)c->errflag, (const u64 *)(c->errflag + 2),
               counters ? counters : c->counters_scratch);
    return FXG_OK;
}


// ------------------------------------------------------------------------------------------------
// clip history: the stale tail of the reference aligner's query buffer (fxg_history.h)
// ------------------------------------------------------------------------------------------------
extern "C" int fxg_set_clip_history(fxg_ctx *c, int on)
{
    if (!c) return FXG_E_INVALID;
    FXG_HIP(c, hipSetDevice(c->device));
    if (on && !c->hist_buf[0]) {
        FXG_HIP(c, hipMalloc((void **)&c->hist_buf[0], FXG_HIST_CAP));
        FXG_HIP(c, hipMalloc((void **)&c->hist_buf[1], FXG_HIST_CAP));
        FXG_HIP(c, hipMalloc((void **)&c->hist_w, 2 * sizeof(u32)));
    }
    if (on) {                                               // a fresh aligner: empty buffer, width 0
        FXG_HIP(c, hipMemsetAsync(c->hist_buf[0], 0, FXG_HIST_CAP, c->stream));
        FXG_HIP(c, hipMemsetAsync(c->hist_buf[1], 0, FXG_HIST_CAP, c->stream));
        FXG_HIP(c, hipMemsetAsync(c->hist_w, 0, 2 * sizeof(u32), c->stream));
    }
    c->hist_on = on ? 1 : 0; c->hist_wcap = 0; c->hist_cur = 0; c->hist_has_adapter = 0;
    return FXG_OK;
}

// Builds the extended queries of one batch, points the plan's clip stage at them and moves the buffer on.  A batch that cannot see a stale tail
// (fxg_hist_shortcut) only moves the buffer on: the clip kernel then reads the batch itself.
static int fxg_hist_prepass(fxg_ctx *c, const fxg_batch *in, u32 estride, FxgPlan &pl)
{
    const int cur = c->hist_cur;
    if (fxg_hist_shortcut(in, c->hist_wcap)) {
        FXG_LAUNCH(c, fxg_kernel_hist_fixed, (FXG_HIST_CAP + FXG_BLOCK - 1) / FXG_BLOCK, FXG_BLOCK, 0, (const uint8_t *)in->bases, (u64)in->n, in->fixed_len, in->stride,
                   (const uint8_t *)c->hist_buf[cur], (const u32 *)(c->hist_w + cur), c->hist_buf[cur ^ 1], c->hist_w + (cur ^ 1));
        fxg_plan_clip_from_batch(&pl, in);
    } else {
        const FxgHistWs w = fxg_hist_ws(in, pl.ka.tile_reads, estride);
        FXG_TRY(fxg_ws_grow(c, c->hist_ws, c->hist_ws_cap, w.bytes, w.bytes + w.bytes / 8));
        const FxgHist h = fxg_hist_args(in, pl.ka.tile_reads, estride, w, c->hist_ws, c->hist_buf[cur], c->hist_w + cur, c->hist_buf[cur ^ 1], c->hist_w + (cur ^ 1));
        FXG_LAUNCH(c, fxg_kernel_hist_tiles, w.ntiles, FXG_BLOCK, 0, h);
        FXG_LAUNCH(c, fxg_kernel_hist_blocks, w.nblk, FXG_BLOCK, 0, h);
        FXG_LAUNCH(c, fxg_kernel_hist_top, (in->stride + 2u + FXG_BLOCK - 1) / FXG_BLOCK, FXG_BLOCK, 0, h, w.nblk);
        FXG_LAUNCH(c, fxg_kernel_hist_extend, w.ntiles, FXG_BLOCK, 0, h);
        fxg_plan_clip_from(&pl, h.ext, estride, (u64)in->n * estride, h.wlen);
    }
    fxg_hist_advance(in, &c->hist_cur, &c->hist_wcap);
    return FXG_OK;
}

static int fxg_launch_plan(fxg_ctx *c, FxgPlan &pl, u64 *ctr);

extern "C" int fxg_run_pipeline(fxg_ctx *c, const fxg_batch *in, const fxg_params *p, const fxg_out *out)
{
    if (!c || !in || !p || !out) return FXG_E_INVALID;
    FxgPlan pl;
    bool hist; u32 estride;
    FXG_TRY(fxg_plan_request(in, p, out, c->hist_on != 0, c->hist_wcap, &pl, &hist, &estride, c->err, sizeof c->err, fxg_knobs_read(FXG_KNOBS_REQUEST)));
    if (in->n == 0) {
        if (out->counters) FXG_HIP(c, hipMemsetAsync(out->counters, 0, FXG_NCOUNTERS * sizeof(u64), c->stream));
        return FXG_OK;
    }
    if (hist) {
        // the reference's matrix keeps the height of its adapter as it keeps the width of its longest read; only the reads' side of that is reproduced, so a
        // history has one adapter (include/fxg.h).  Refused before anything is launched: the history stays as it was.
        if (c->hist_has_adapter && strcmp(c->hist_adapter, pl.ka.adapter) != 0)
            return fxg_fail(c, FXG_E_INVALID, "clip history: the adapter differs from the one this history began with; fxg_set_clip_history(ctx, 1) begins another");
        snprintf(c->hist_adapter, sizeof c->hist_adapter, "%s", pl.ka.adapter);
        c->hist_has_adapter = 1;
        FXG_HIP(c, hipSetDevice(c->device));
        FXG_TRY(fxg_hist_prepass(c, in, estride, pl));
    }
    // what fxg_read_counters needs to do a compacting pass again, should its waits time out (fxg_fallback.h)
    c->fb_req.valid = 0;
    if (pl.ka.compact) { c->fb_req.in = *in; c->fb_req.p = *p; c->fb_req.out = *out; c->fb_req.hist = hist; c->fb_req.estride = estride; c->fb_req.valid = 1; }
    return fxg_launch_plan(c, pl, (u64 *)out->counters);
}

// the clipper's instances live in translation units of their own (fxg_engine_clip.hip): the unit that holds the planned one launches it
static int fxg_launch_clip(fxg_ctx *c, FxgPlan &pl, u64 *ctr)
{
    int rc;
#define FXG_CLIP_TRY_UNIT(K) if ((rc = FXG_CLIP_UNIT_FN(K)(c, pl, ctr)) != FXG_CLIP_NOT_MINE) return rc;
    FXG_CLIP_FOR_UNITS(FXG_CLIP_TRY_UNIT)
#undef FXG_CLIP_TRY_UNIT
    return fxg_fail(c, FXG_E_INVALID, "no clip instance %d", pl.amax);
}

// the launch of a planned pass: the instance the plan names (fxg_instances.h)
static int fxg_launch_plan(fxg_ctx *c, FxgPlan &pl, u64 *ctr)
{
    switch (pl.inst) {
#define FXG_INST_LAUNCH(ID, KERNEL, NAME, ROWS, AMAX, REV, MODE, NW, H, R) case FXG_INST_##ID: return fxg_launch_tiles(c, KERNEL, pl, ctr, ROWS);
    FXG_INSTANCES(FXG_INST_LAUNCH)
#undef FXG_INST_LAUNCH
    default: return fxg_launch_clip(c, pl, ctr);
    }
}

extern "C" int fxg_run_quality_stats(fxg_ctx *c, const fxg_batch *in, uint64_t *d_hist, uint32_t hist_cols)
{
    if (!c) return FXG_E_INVALID;
    const FxgKnobs kn = fxg_knobs_read(FXG_KNOBS_REQUEST);
    FXG_TRY(fxg_stats_check(in, d_hist, hist_cols, c->err, sizeof c->err));
    if (in->n == 0) return FXG_OK;
    FXG_HIP(c, hipSetDevice(c->device));
    // one workgroup per CU (its LDS holds the 100 KB block histogram); fewer when the batch is small
    u64 nwg = (in->n + 255) / 256;
    if (nwg > (u64)c->cus) nwg = (u64)c->cus;
    FxgStatsArgs a = fxg_stats_args(in, d_hist, hist_cols, (u32)nwg);
    const size_t need = (size_t)a.nwg * FXG_QS_PART_WORDS;
    FXG_TRY(fxg_ws_grow(c, c->stats_ws, c->stats_ws_cap, need, need));
    a.partial = c->stats_ws;
    a.round_robin = kn.qs_round_robin;      // FXG_QS_ROUND_ROBIN (measurement knob)
    const u32 lds = FXG_QS_LDS_WORDS * sizeof(u32);
    FXG_TRY(fxg_kernel_lds(c, fxg_kernel_quality_stats, lds));
    FXG_TRY(fxg_kernel_lds(c, fxg_kernel_quality_stats_odd, lds));
    const u32 nstrips = (in->stride + FXG_QS_STRIP - 1) / FXG_QS_STRIP;
    for (u32 s0 = 0; s0 < nstrips; s0 += FXG_QS_WAVES) {       // one pass per block of 160 columns (one pass for reads up to 160)
        a.strip0 = s0;
        if (s0 == 0) FXG_PROFILE_BEGIN(c);
        u32 pr = 0, pp = 0;
        // dense batches of odd length 17 .. 159: the piece form that keeps LDS block and counter half per byte, a kernel (and a register allocation) of its own
        if (a.round_robin == 1u && (a.fixed_len & 1u) && fxg_stats_piece_plan(a, &pr, &pp)) FXG_LAUNCH(c, fxg_kernel_quality_stats_odd, a.nwg, FXG_QS_TBLOCK, lds, a);
        else FXG_LAUNCH(c, fxg_kernel_quality_stats, a.nwg, FXG_QS_TBLOCK, lds, a);
        if (s0 == 0) FXG_PROFILE_END(c);
        FXG_LAUNCH(c, fxg_kernel_quality_stats_fold, (FXG_QS_PART_WORDS + FXG_QS_FOLD_E - 1) / FXG_QS_FOLD_E, 256, 0, a);
    }
    fxg_note_launch(c, "fxg_kernel_quality_stats", a.nwg, FXG_QS_TBLOCK, lds, 64u * FXG_QS_UNROLL);
    return FXG_OK;
}

static void fxg_params_default(fxg_params *p)
{
    memset(p, 0, sizeof *p);
    p->qoffset = 33;
    strcpy(p->adapter, "CCTTAAGG");   // fastx_clipper.cpp:68
    p->clip_min_len = 5;              // :69
    p->ft_first = 1;
    p->mask_min_quality = 10;         // fastq_masker.c:47-48
    p->mask_char = 'N';
}

extern "C" int fxg_run_qtrim_qfilter(fxg_ctx *c, const fxg_batch *in, int qoffset, int use_trim, int trim_threshold,
                                     int trim_min_len, int use_filter, int filter_min_quality, int filter_min_percent,
                                     const fxg_out *out)
{
    fxg_params p;
    fxg_params_default(&p);
    p.qoffset = qoffset;
    if (use_trim) { p.stages |= FXG_STAGE_QTRIM; p.qt_threshold = trim_threshold; p.qt_min_len = trim_min_len; }
    if (use_filter) { p.stages |= FXG_STAGE_QFILTER; p.qf_min_quality = filter_min_quality; p.qf_min_percent = filter_min_percent; }
    return fxg_run_pipeline(c, in, &p, out);
}

extern "C" int fxg_run_clip(fxg_ctx *c, const fxg_batch *in, const char *adapter, uint32_t min_len, int keep_delta,
                            int min_adapter_len, uint32_t clip_flags, const fxg_out *out)
{
    fxg_params p;
    fxg_params_default(&p);
    p.stages = FXG_STAGE_CLIP;
    if (adapter) { strncpy(p.adapter, adapter, sizeof p.adapter - 1); p.adapter[sizeof p.adapter - 1] = 0; }
    p.clip_min_len = min_len; p.clip_keep_delta = keep_delta; p.clip_min_adapter_len = min_adapter_len; p.clip_flags = clip_flags;
    return fxg_run_pipeline(c, in, &p, out);
}

extern "C" int fxg_run_revcomp_trim(fxg_ctx *c, const fxg_batch *in, int reverse_complement, int first_base, int last_base,
                                    const fxg_out *out)
{
    fxg_params p;
    fxg_params_default(&p);
    if (reverse_complement) p.stages |= FXG_STAGE_REVCOMP;
    if (first_base != 1 || last_base != 0 || !reverse_complement) { p.stages |= FXG_STAGE_FTRIM; p.ft_first = first_base; p.ft_last = last_base; }
    return fxg_run_pipeline(c, in, &p, out);
}

// The last compacting pass once more, in the form that cannot wait (fxg_fallback.h).  Everything goes behind the failed launch on the same stream.
static int fxg_redo_without_scanner(fxg_ctx *c)
{
    const FxgKArgs failed = c->fb.ka;
    u64 *const counters = c->fb.counters;
    // 1. the decisions: the same request planned without the packed outputs -- the kernel instance the plan picks for a decision-only pass has no scanner
    //    and no wait (the row-per-lane kernel of fxg_rows.h only exists in its compacting form).  A run with clip history keeps the extended queries the
    //    failed pass built: the aligner's buffer has moved on once for this batch and must not move again.
    fxg_out o2 = c->fb_req.out;
    o2.out_bases = o2.out_qual = nullptr; o2.out_len = nullptr; o2.kept_index = nullptr; o2.out_off = nullptr;
    FxgPlan pl;
    FXG_TRY(fxg_make_plan(&c->fb_req.in, &c->fb_req.p, &o2, &pl, c->err, sizeof c->err, c->fb_req.hist ? c->fb_req.estride : 0u, fxg_knobs_read(FXG_KNOBS_REQUEST)));
    if (c->fb_req.hist) fxg_plan_clip_from(&pl, failed.clip_src, failed.clip_stride, failed.clip_total, failed.wlen);
    FXG_HIP(c, hipSetDevice(c->device));
    FXG_TRY(fxg_launch_plan(c, pl, counters));
    // 2. + 3. block sums -> prefixes -> every kept read to its place
    FxgFbArgs f;
    f.ka = failed;                               // the arrays and folded parameters of the pass as it was asked for
    f.ka.errflag = c->errflag;
    f.nblk = (u32)((f.ka.n + FXG_FB_BLOCK - 1u) / FXG_FB_BLOCK);
    const size_t need = 2 * (size_t)f.nblk + 2;
    FXG_TRY(fxg_ws_grow(c, c->fb_blk, c->fb_blk_cap, need, need));
    f.blk = c->fb_blk;
    FXG_LAUNCH(c, fxg_kernel_fb_sums, f.nblk, FXG_FB_BLOCK, 0, f);
    FXG_LAUNCH(c, fxg_kernel_fb_scan, 1, FXG_FB_BLOCK, 0, f);
    if (f.ka.stages & FXG_STAGE_REVCOMP) FXG_LAUNCH(c, (fxg_kernel_fb_gather<true, false>), f.nblk, FXG_FB_BLOCK, 0, f);
    else if (f.ka.stages & FXG_STAGE_MASK) FXG_LAUNCH(c, (fxg_kernel_fb_gather<false, true>), f.nblk, FXG_FB_BLOCK, 0, f);
    else FXG_LAUNCH(c, (fxg_kernel_fb_gather<false, false>), f.nblk, FXG_FB_BLOCK, 0, f);
    // a base that has no complement: found by the gather, reported like the tile kernels do
    if (f.ka.stages & FXG_STAGE_REVCOMP) FXG_LAUNCH(c, fxg_kernel_fb_errors, 1, 1, 0, (const u32 *)c->errflag, counters ? counters : c->counters_scratch);
    c->recoveries++;
    return FXG_OK;
}

extern "C" int fxg_scan_recoveries(const fxg_ctx *c) { return c ? c->recoveries : 0; }

extern "C" int fxg_read_counters(fxg_ctx *c, const uint64_t *d_counters, uint64_t host[FXG_NCOUNTERS])
{
    if (!c || !host) return FXG_E_INVALID;
    const FxgKnobs kn = fxg_knobs_read(FXG_KNOBS_REQUEST);
    const u64 *src = d_counters ? (const u64 *)d_counters : c->counters_scratch;
    FXG_HIP(c, hipMemcpyAsync(host, src, FXG_NCOUNTERS * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    FXG_HIP(c, hipStreamSynchronize(c->stream));
    if ((host[FXG_C_ERRORS] & FXG_DEV_ERR_SCAN_TIMEOUT) && c->fb.valid && c->fb_req.valid && src == (c->fb.counters ? c->fb.counters : c->counters_scratch) && !kn.no_scan_fallback) {
        // the launch these counters belong to gave up waiting (its workgroups were not being scheduled): the same work again without anything that waits
        c->fb.valid = 0; c->fb_req.valid = 0;
        FXG_TRY(fxg_redo_without_scanner(c));
        FXG_HIP(c, hipMemcpyAsync(host, src, FXG_NCOUNTERS * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        FXG_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (host[FXG_C_ERRORS] & FXG_DEV_ERR_SCAN_TIMEOUT) return fxg_fail(c, FXG_E_DEVICE, "device: look-back scan timed out");
    if (host[FXG_C_ERRORS] & FXG_DEV_ERR_BAD_BASE)
        return fxg_fail(c, FXG_E_DEVICE, "Invalid nucleotide value in reverse_complement_base()");   // fastx_reverse_complement.c:67-68
    return FXG_OK;
}

extern "C" int fxg_synth_generate(fxg_ctx *c, uint64_t seed, uint64_t first, uint64_t n, uint32_t L, int with_adapter,
                                  uint8_t *bases, uint8_t *qual, uint32_t stride)
{
    if (!c || !bases || L == 0 || stride < L) return FXG_E_INVALID;
    if ((((uintptr_t)bases | (uintptr_t)qual) & 15u) != 0) return fxg_fail(c, FXG_E_INVALID, "synth: buffers must be 16-byte aligned");
    if (n == 0) return FXG_OK;
    const u32 lds = 2 * fxg_r16(FXG_SYNTH_TILE * stride);
    if (lds > 160 * 1024) return fxg_fail(c, FXG_E_INVALID, "synth: stride %u too large", stride);
    FXG_HIP(c, hipSetDevice(c->device));
    FXG_TRY(fxg_kernel_lds(c, fxg_kernel_synth, lds));      // (its LDS follows the stride: raised only, like the tile kernels')
    const u64 blocks = (n + FXG_SYNTH_TILE - 1) / FXG_SYNTH_TILE;
    if (blocks > 0x7FFFFFFFull) return fxg_fail(c, FXG_E_INVALID, "synth: too many reads for one launch");
    FXG_LAUNCH(c, fxg_kernel_synth, (u32)blocks, FXG_BLOCK, lds, (u64)seed, (u64)first, (u64)n, L, with_adapter, bases, qual, stride);
    return FXG_OK;
}

// ------------------------------------------------------------------------------------------------
// FASTQ text on the device
// ------------------------------------------------------------------------------------------------
// the device-side state of the text calls: made by the first of them that needs it, whichever that is
static int fxg_text_state_ensure(fxg_ctx *c)
{
    if (!c->text_state) FXG_HIP(c, hipMalloc((void **)&c->text_state, sizeof(FxgTextState)));
    return FXG_OK;
}

static int fxg_text_reserve(fxg_ctx *c, size_t words)
{
    FXG_TRY(fxg_text_state_ensure(c));
    const size_t cap = words + words / 4 + 4096;
    return fxg_ws_grow(c, c->text_ws, c->text_ws_cap, words, cap);
}

// in-place exclusive scan of data[0..n); tmp must hold the block-sum levels (n/1024 + n/1024^2 + ... + 8 words)
static int fxg_scan_u64(fxg_ctx *c, u64 *data, u64 n, u64 *tmp)
{
    if (n == 0) return FXG_OK;
    const u64 nb = (n + FXG_SCAN_PER_BLOCK - 1) / FXG_SCAN_PER_BLOCK;
    FXG_LAUNCH(c, fxg_kernel_scan_blocks, (u32)nb, FXG_BLOCK, 0, data, n, tmp);
    if (nb > 1) {
        FXG_TRY(fxg_scan_u64(c, tmp, nb, tmp + nb));
        FXG_LAUNCH(c, fxg_kernel_scan_add, (u32)nb, FXG_BLOCK, 0, data, n, (const u64 *)tmp);
    }
    return FXG_OK;
}

// The line index of a block of text (text_len > 0): the newline census per segment, its scan, the line starts and ends scattered into d_ls / d_le.  The one wait
// for *lines comes behind the scatter, or (fit_first: fxg_fasta_reflow) ahead of it, and nothing is scattered unless the lines fit.
static int fxg_line_index(fxg_ctx *c, const uint8_t *d_text, u64 text_len, u32 *d_ls, u32 *d_le, u64 cap_lines, bool fit_first, u64 *lines)
{
    const u64 nseg = (text_len + FXG_TEXT_SEG - 1) / FXG_TEXT_SEG;
    FXG_TRY(fxg_text_reserve(c, (size_t)(nseg + nseg / 512 + 4096)));
    const FxgTextState init = fxg_text_state_init();
    FXG_HIP(c, hipMemcpyAsync(c->text_state, &init, sizeof init, hipMemcpyHostToDevice, c->stream));
    u64 *seg = c->text_ws;
    FXG_LAUNCH(c, fxg_kernel_nl_count, (u32)nseg, FXG_BLOCK, 0, d_text, text_len, seg, c->text_state);
    // total newlines = last exclusive prefix + last count: keep the last count before the scan overwrites it
    u64 last_count = 0, last_off = 0;
    FXG_HIP(c, hipMemcpyAsync(&last_count, seg + (nseg - 1), sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    FXG_TRY(fxg_scan_u64(c, seg, nseg, seg + nseg));
    FXG_HIP(c, hipMemcpyAsync(&last_off, seg + (nseg - 1), sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (fit_first) {
        FXG_HIP(c, hipStreamSynchronize(c->stream));
        FXG_TRY(fxg_rf_lines_fit(last_off + last_count, cap_lines, c->err, sizeof c->err));
    }
    FXG_LAUNCH(c, fxg_kernel_nl_scatter, (u32)nseg, FXG_BLOCK, 0, d_text, text_len, (const u64 *)seg, d_ls, d_le, cap_lines);
    if (!fit_first) FXG_HIP(c, hipStreamSynchronize(c->stream));
    *lines = last_off + last_count;
    return FXG_OK;
}

extern "C" int fxg_fastq_index(fxg_ctx *c, const uint8_t *d_text, uint64_t text_len, int at_eof, int lines_per_record, uint32_t *d_line,
                               uint64_t cap_lines, uint16_t *d_len, uint8_t *d_flags, fxg_text_info *info)
{
    if (!c) return FXG_E_INVALID;
    FXG_TRY(fxg_text_index_check(d_text, text_len, lines_per_record, d_line, d_len, d_flags, info, c->err, sizeof c->err));
    if (text_len == 0) return FXG_OK;
    FXG_HIP(c, hipSetDevice(c->device));
    const u64 lpr = (u64)lines_per_record;
    u32 *d_ls = d_line, *d_le = d_line + cap_lines;
    u64 lines = 0;
    FXG_TRY(fxg_line_index(c, d_text, text_len, d_ls, d_le, cap_lines, false, &lines));
    const u64 n = fxg_text_records(lines, lpr, cap_lines);
    if (n == 0) { fxg_text_info_fill(info, nullptr, lines, lpr, 0, 0, text_len, at_eof); return FXG_OK; }
    const u32 grid = (u32)((n + FXG_BLOCK - 1) / FXG_BLOCK);
    if (lines_per_record == 4) FXG_LAUNCH(c, fxg_kernel_text_records<4>, grid, FXG_BLOCK, 0, d_text, (const u32 *)d_ls, d_le, n, d_len, d_flags, c->text_state);
    else FXG_LAUNCH(c, fxg_kernel_text_records<2>, grid, FXG_BLOCK, 0, d_text, (const u32 *)d_ls, d_le, n, d_len, d_flags, c->text_state);
    FxgTextState st;
    u32 consumed = 0;
    FXG_HIP(c, hipMemcpyAsync(&st, c->text_state, sizeof st, hipMemcpyDeviceToHost, c->stream));
    FXG_HIP(c, hipMemcpyAsync(&consumed, d_ls + lpr * n, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    FXG_HIP(c, hipStreamSynchronize(c->stream));
    fxg_text_info_fill(info, &st, lines, lpr, n, consumed, text_len, at_eof);
    return FXG_OK;
}

extern "C" int fxg_fastq_pack(fxg_ctx *c, const uint8_t *d_text, uint64_t text_len, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines,
                              const uint8_t *d_flags, uint64_t n, uint32_t stride, int qoffset, uint8_t *d_bases, uint8_t *d_qual, uint32_t *irregular)
{
    if (!c) return FXG_E_INVALID;
    FXG_TRY(fxg_text_pack_check(d_text, lines_per_record, d_line, d_flags, n, stride, d_bases, d_qual, irregular, c->err, sizeof c->err));
    if (n == 0) return FXG_OK;
    FXG_HIP(c, hipSetDevice(c->device));
    const u32 *d_ls = d_line, *d_le = d_line + cap_lines;
    const u64 nchunks = (n * (u64)stride + 15) >> 4;
    u64 grid = (nchunks + FXG_BLOCK - 1) / FXG_BLOCK;
    if (grid > 65536) grid = 65536;
    FXG_TRY(fxg_text_state_ensure(c));      // (a context that has indexed nothing: the line arrays are another context's)
    FXG_HIP(c, hipMemsetAsync(&c->text_state->irregular, 0, sizeof(u32), c->stream));
    if (lines_per_record == 4) FXG_LAUNCH(c, (fxg_kernel_text_pack<false, 4>), (u32)grid, FXG_BLOCK, 0, d_text, (u64)text_len, d_ls, d_le, d_flags, (u64)n, stride, qoffset, d_bases, c->text_state);
    else FXG_LAUNCH(c, (fxg_kernel_text_pack<false, 2>), (u32)grid, FXG_BLOCK, 0, d_text, (u64)text_len, d_ls, d_le, d_flags, (u64)n, stride, qoffset, d_bases, c->text_state);
    if (d_qual) {
        FXG_LAUNCH(c, (fxg_kernel_text_pack<true, 4>), (u32)grid, FXG_BLOCK, 0, d_text, (u64)text_len, d_ls, d_le, d_flags, (u64)n, stride, qoffset, d_qual, c->text_state);
        // records with numeric quality lines (rare: one pass over the flags, the parse itself only where a flag is set)
        FXG_LAUNCH(c, fxg_kernel_text_numeric, (u32)((n + FXG_BLOCK - 1) / FXG_BLOCK), FXG_BLOCK, 0, d_text, d_ls, d_le, d_flags, (u64)n, stride, d_qual);
    }
    FXG_HIP(c, hipMemcpyAsync(irregular, &c->text_state->irregular, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    FXG_HIP(c, hipStreamSynchronize(c->stream));
    return FXG_OK;
}

extern "C" int fxg_fastq_format_opts(fxg_ctx *c, const uint8_t *d_text, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines, const uint8_t *d_flags,
                                     uint64_t n, const uint32_t *d_res, uint32_t fwd_start, int reverse, const uint8_t *d_pk_bases, const uint8_t *d_pk_qual,
                                     const uint64_t *d_pk_off, const uint8_t *d_rows_qual, uint32_t stride, int qoffset, int out_fasta, uint8_t *d_out,
                                     uint64_t *out_bytes, const fxg_format_opts *opts)
{
    if (!c) return FXG_E_INVALID;
    FXG_TRY(fxg_text_format_opts_check(d_text, lines_per_record, d_line, d_flags, n, d_res, fwd_start, d_pk_bases, d_pk_qual, d_pk_off, d_rows_qual, out_fasta, d_out, out_bytes, opts, c->err, sizeof c->err));
    FXG_TRY(fxg_text_format_source_check(d_pk_bases, reverse, fwd_start, c->err, sizeof c->err));
    if (n == 0) return FXG_OK;
    FXG_HIP(c, hipSetDevice(c->device));
    FXG_TRY(fxg_text_reserve(c, (size_t)(n + n / 512 + 4096)));
    u64 *item = c->text_ws;
    FxgFormatArgs a = fxg_text_format_args(d_text, d_line, cap_lines, d_flags, item, n, d_res, fwd_start, reverse, d_pk_bases, d_pk_qual, d_pk_off, d_rows_qual, stride, qoffset, out_fasta, d_out);
    fxg_text_format_args_opts(&a, opts);
    const u32 nb = (u32)((n + FXG_BLOCK - 1) / FXG_BLOCK);
    if (lines_per_record == 4) FXG_LAUNCH(c, fxg_kernel_text_sizes<4>, nb, FXG_BLOCK, 0, a, item);
    else FXG_LAUNCH(c, fxg_kernel_text_sizes<2>, nb, FXG_BLOCK, 0, a, item);
    FXG_TRY(fxg_scan_u64(c, item, n, item + n));
    u64 *d_tot = item + n, tot[2] = {0, 0};                    // (the scan is done with its block sums)
    if (lines_per_record == 4) FXG_LAUNCH(c, fxg_kernel_text_total<4>, 1, 1, 0, a, d_tot);
    else FXG_LAUNCH(c, fxg_kernel_text_total<2>, 1, 1, 0, a, d_tot);
    FXG_HIP(c, hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, c->stream));
    if (opts->out_cap != FXG_OUT_CAP_UNCHECKED) {              // nothing may be written before the total is known to fit
        FXG_HIP(c, hipStreamSynchronize(c->stream));
        FXG_TRY(fxg_text_format_fits(tot[0], opts->out_cap, c->err, sizeof c->err));
    }
    const u32 fgrid = (u32)((n * 16 + FXG_BLOCK - 1) / FXG_BLOCK);
    if (lines_per_record == 4) FXG_LAUNCH(c, fxg_kernel_text_format<4>, fgrid, FXG_BLOCK, 0, a);
    else FXG_LAUNCH(c, fxg_kernel_text_format<2>, fgrid, FXG_BLOCK, 0, a);
    FXG_HIP(c, hipStreamSynchronize(c->stream));
    *out_bytes = tot[0];
    return FXG_OK;
}

extern "C" int fxg_fastq_format(fxg_ctx *c, const uint8_t *d_text, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines, const uint8_t *d_flags,
                                uint64_t n, const uint32_t *d_res, uint32_t fwd_start, int reverse, const uint8_t *d_pk_bases, const uint8_t *d_pk_qual,
                                const uint64_t *d_pk_off, const uint8_t *d_rows_qual, uint32_t stride, int qoffset, int out_fasta, uint8_t *d_out,
                                uint64_t *out_bytes)
{
    const fxg_format_opts plain = fxg_text_format_opts_plain();
    if (!d_res) return FXG_E_INVALID;
    return fxg_fastq_format_opts(c, d_text, lines_per_record, d_line, cap_lines, d_flags, n, d_res, fwd_start, reverse, d_pk_bases, d_pk_qual, d_pk_off, d_rows_qual, stride, qoffset, out_fasta,
                                 d_out, out_bytes, &plain);
}

extern "C" int fxg_fasta_weights(fxg_ctx *c, const uint8_t *d_text, const uint32_t *d_line, uint64_t cap_lines, uint64_t n, const uint32_t *d_res,
                                 uint64_t weighted[8])
{
    if (!c || !d_text || !d_line || !d_res || !weighted) return FXG_E_INVALID;
    memset(weighted, 0, 8 * sizeof(uint64_t));
    if (n == 0) return FXG_OK;
    FXG_HIP(c, hipSetDevice(c->device));
    if (!c->text_state) return fxg_fail(c, FXG_E_INVALID, "fxg_fasta_weights: index the block first");
    FXG_HIP(c, hipMemsetAsync(c->text_state->weighted, 0, sizeof c->text_state->weighted, c->stream));
    FXG_LAUNCH(c, fxg_kernel_text_weights, (u32)((n + FXG_BLOCK - 1) / FXG_BLOCK), FXG_BLOCK, 0, d_text, d_line, d_line + cap_lines, d_res, (u64)n, c->text_state);
    FXG_HIP(c, hipMemcpyAsync(weighted, c->text_state->weighted, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    FXG_HIP(c, hipStreamSynchronize(c->stream));
    return FXG_OK;
}

// ------------------------------------------------------------------------------------------------
// fastx_barcode_splitter (fxg_barcode.h): classify, scan, scatter
// ------------------------------------------------------------------------------------------------
extern "C" int fxg_barcode_prepare(fxg_ctx *c, const fxg_barcode_set *set)
{
    if (!c || !set) return FXG_E_INVALID;
    c->bc_ready = 0;
    const u32 E = set->entries;
    const size_t room = E ? E : 1;
    FXG_TRY(fxg_bc_set_check(set, c->err, sizeof c->err));
    FxgBcEntry *tab = (FxgBcEntry *)calloc(room, sizeof(FxgBcEntry));
    if (!tab) return FXG_E_NOMEM;
    int rc = fxg_bc_set_encode(set, tab, c->err, sizeof c->err);
    if (rc == FXG_OK && hipSetDevice(c->device) != hipSuccess) rc = fxg_fail(c, FXG_E_HIP, "hipSetDevice failed");
    if (rc == FXG_OK) rc = fxg_ws_grow(c, c->bc_tab, c->bc_tab_cap, room, room);      // (its own message: the wait for the stream or the allocation)
    if (rc == FXG_OK && E > 0 && (hipMemcpyAsync(c->bc_tab, tab, (size_t)E * sizeof(FxgBcEntry), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                                  hipStreamSynchronize(c->stream) != hipSuccess))
        rc = fxg_fail(c, FXG_E_HIP, "upload of the barcode table failed");
    free(tab);
    if (rc != FXG_OK) return rc;
    c->bc_entries = E; c->bc_len = set->barcode_len; c->bc_mm = set->mismatches; c->bc_eol = set->eol ? 1u : 0u; c->bc_bins = set->bins;
    c->bc_ready = 1;
    return FXG_OK;
}

extern "C" int fxg_barcode_split(fxg_ctx *c, const uint8_t *d_text, uint64_t text_len, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines,
                                 uint64_t n, uint16_t *d_rec_bin, uint8_t *d_out, uint64_t *bin_bytes, uint64_t *bin_records)
{
    if (!c) return FXG_E_INVALID;
    const u32 bins = c->bc_ready ? c->bc_bins : 0u;
    FXG_TRY(fxg_bc_split_check(bins, d_text, text_len, lines_per_record, d_line, cap_lines, n, d_out, bin_bytes, bin_records, c->err, sizeof c->err));
    if (n == 0) return FXG_OK;
    FXG_HIP(c, hipSetDevice(c->device));
    const u64 tiles = (n + FXG_BC_TILE - 1) / FXG_BC_TILE;
    if (tiles > 0xFFFFFFFFull) return fxg_fail(c, FXG_E_INVALID, "fxg_barcode_split: too many records");
    const u64 N = (u64)bins * tiles;
    const u64 levels = N / 512 + 64;                         // fxg_scan_u64's block sums: N / 1024 + N / 1024^2 + ... + 8 per level
    const u64 words = N + levels + 2 * (u64)bins + (d_rec_bin ? 0 : (n + 3) / 4);
    const size_t cap = words + words / 4 + 4096;
    FXG_TRY(fxg_ws_grow(c, c->bc_ws, c->bc_ws_cap, words, cap));
    FxgBcArgs a;
    a.text = d_text; a.ls = d_line; a.n = n; a.lpr = (u32)lines_per_record; a.tiles = (u32)tiles;
    a.tab = c->bc_tab; a.entries = c->bc_entries; a.BL = c->bc_len; a.mismatches = c->bc_mm; a.eol = c->bc_eol; a.bins = bins;
    a.hist_bytes = c->bc_ws;
    u64 *tmp = c->bc_ws + N;
    a.totals = tmp + levels;
    a.rec_bin = d_rec_bin ? d_rec_bin : (uint16_t *)(a.totals + 2 * bins);
    a.out = d_out;
    FXG_HIP(c, hipMemsetAsync(a.totals, 0, 2 * bins * sizeof(u64), c->stream));
    FXG_LAUNCH(c, fxg_kernel_bc_classify, (u32)tiles, FXG_BC_TILE, 2 * bins * sizeof(u32), a);
    FXG_TRY(fxg_scan_u64(c, a.hist_bytes, N, tmp));
    FXG_LAUNCH(c, fxg_kernel_bc_scatter, (u32)tiles, FXG_BC_TILE, 0, a);
    FXG_HIP(c, hipMemcpyAsync(bin_bytes, a.totals, bins * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    FXG_HIP(c, hipMemcpyAsync(bin_records, a.totals + bins, bins * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    FXG_HIP(c, hipStreamSynchronize(c->stream));
    return FXG_OK;
}

// ------------------------------------------------------------------------------------------------
// fasta_formatter (fxg_reflow.h): line index, classify + segmented scan, sizes + scans, copy
// ------------------------------------------------------------------------------------------------
// in-place segmented exclusive scan of (s, kf)[0..n); tmp holds both arrays of every level of block aggregates
static int fxg_rf_segscan(fxg_ctx *c, u64 *s, u64 *kf, u64 n, u64 *tmp)
{
    const u64 nb = (n + FXG_RF_SCAN_BLOCK - 1) / FXG_RF_SCAN_BLOCK;
    FXG_LAUNCH(c, fxg_kernel_rf_segscan_blocks, (u32)nb, FXG_BLOCK, 0, s, kf, n, tmp, tmp + nb);
    if (nb > 1) {
        FXG_TRY(fxg_rf_segscan(c, tmp, tmp + nb, nb, tmp + 2 * nb));
        FXG_LAUNCH(c, fxg_kernel_rf_segscan_add, (u32)nb, FXG_BLOCK, 0, s, kf, n, (const u64 *)tmp, (const u64 *)(tmp + nb));
    }
    return FXG_OK;
}

// with profiling on, a call leaves three entries in the event ring: classify + segmented scan, sizes + scans, copy
extern "C" int fxg_fasta_reflow(fxg_ctx *c, const uint8_t *d_text, uint64_t text_len, int at_eof, uint64_t open_bases_in, const fxg_reflow_opts *opts,
                                uint32_t *d_line, uint64_t cap_lines, uint8_t *d_out, fxg_reflow_info *info)
{
    if (!c) return FXG_E_INVALID;
    FXG_TRY(fxg_rf_check(d_text, text_len, opts, d_line, cap_lines, info, c->err, sizeof c->err));
    FXG_HIP(c, hipSetDevice(c->device));
    u64 L = 0;
    if (text_len) FXG_TRY(fxg_line_index(c, d_text, text_len, d_line, d_line + cap_lines, cap_lines, true, &L));      // the line starts, by the newline kernels of the text path
    const u64 M = L + 2, words = fxg_rf_ws_words(L);
    FXG_TRY(fxg_ws_grow(c, c->rf_ws, c->rf_ws_cap, (size_t)words, (size_t)(words + words / 4 + 4096)));
    const FxgRfArgs a = fxg_rf_args(d_text, d_line, L, at_eof, open_bases_in, opts, c->rf_ws, d_out);
    const u32 grid = (u32)((M + FXG_BLOCK - 1) / FXG_BLOCK);
    FXG_HIP(c, hipMemsetAsync(a.res, 0, FXG_RF_RES_WORDS * sizeof(u64), c->stream));
    FXG_PROFILE_BEGIN(c);
    FXG_LAUNCH(c, fxg_kernel_rf_classify, grid, FXG_BLOCK, 0, a);
    FXG_TRY(fxg_rf_segscan(c, a.seg_s, a.seg_kf, M, fxg_rf_levels(a)));
    FXG_PROFILE_END(c);
    FXG_PROFILE_BEGIN(c);
    FXG_LAUNCH(c, fxg_kernel_rf_sizes, grid, FXG_BLOCK, 0, a);
    FXG_TRY(fxg_scan_u64(c, a.size, M, fxg_rf_levels(a)));
    FXG_TRY(fxg_scan_u64(c, a.pieces, M, fxg_rf_levels(a)));
    FXG_LAUNCH(c, fxg_kernel_rf_finish, 1, 1, 0, a);
    FXG_PROFILE_END(c);
    u64 res[FXG_RF_RES_WORDS];
    FXG_HIP(c, hipMemcpyAsync(res, a.res, sizeof res, hipMemcpyDeviceToHost, c->stream));
    FXG_HIP(c, hipStreamSynchronize(c->stream));                // nothing may be written before the total is known to fit
    FXG_TRY(fxg_rf_results(res, L, opts->out_cap, d_out != nullptr, info, c->err, sizeof c->err));
    const u64 np = res[FXG_RF_RES_PIECES];
    FXG_PROFILE_BEGIN(c);
    if (res[FXG_RF_RES_OUT_BYTES]) {
        const u64 hgrid = ((L + 1) * 16 + FXG_BLOCK - 1) / FXG_BLOCK, tgrid = (np * 16 + FXG_BLOCK - 1) / FXG_BLOCK;
        if (hgrid > 0x7FFFFFFFull || tgrid > 0x7FFFFFFFull) return fxg_fail(c, FXG_E_INVALID, "fxg_fasta_reflow: too many pieces for one launch");
        FXG_LAUNCH(c, fxg_kernel_rf_copy_heads, (u32)hgrid, FXG_BLOCK, 0, a);
        if (np) FXG_LAUNCH(c, fxg_kernel_rf_copy_tails, (u32)tgrid, FXG_BLOCK, 0, a, np);
    }
    FXG_PROFILE_END(c);
    FXG_HIP(c, hipStreamSynchronize(c->stream));
    fxg_note_launch(c, "fxg_kernel_rf_copy", c->last_grid, c->last_block, c->last_lds, c->last_tile);      // (several kernels: no one geometry to report, the last one stays)
    return FXG_OK;
}

// ------------------------------------------------------------------------------------------------
// fastx_uncollapser (fxg_uncollapse.h): counts + scan, sizes + scans + window, copy
// ------------------------------------------------------------------------------------------------
// with profiling on, a call leaves three entries in the event ring (two when copy_begin > 0: the scans are the block's first call's)
extern "C" int fxg_fasta_uncollapse(fxg_ctx *c, const uint8_t *d_text, uint64_t text_len, const uint32_t *d_line, uint64_t cap_lines, uint64_t records,
                                    const uint16_t *d_len, const fxg_uncollapse_opts *opts, uint8_t *d_out, fxg_uncollapse_info *info)
{
    if (!c) return FXG_E_INVALID;
    FXG_TRY(fxg_uc_check(d_text, text_len, d_line, cap_lines, records, d_len, opts, info, c->err, sizeof c->err));
    FXG_HIP(c, hipSetDevice(c->device));
    const u64 n = records, M = n + 1, words = fxg_uc_ws_words(n);
    if (opts->copy_begin == 0) {
        c->uc_ready = 0;
        FXG_TRY(fxg_ws_grow(c, c->uc_ws, c->uc_ws_cap, (size_t)words, (size_t)(words + words / 4 + 4096)));
    } else if (!c->uc_ready || c->uc_records != n || c->uc_base != opts->ordinal_base)
        return fxg_fail(c, FXG_E_INVALID, "fxg_fasta_uncollapse: copy_begin > 0 continues a block, and the context holds no scans of %llu records numbered from %llu on",
                        (unsigned long long)n, (unsigned long long)opts->ordinal_base + 1ull);
    const FxgUcArgs a = fxg_uc_args(d_text, d_line, cap_lines, n, d_len, opts->ordinal_base, c->uc_ws, d_out);
    const u32 grid = (u32)((M + FXG_BLOCK - 1) / FXG_BLOCK);
    if (opts->copy_begin == 0) {
        FXG_PROFILE_BEGIN(c);
        FXG_LAUNCH(c, fxg_kernel_uc_counts, grid, FXG_BLOCK, 0, a);
        FXG_TRY(fxg_scan_u64(c, a.cnt, M, fxg_uc_levels(a)));
        FXG_PROFILE_END(c);
    }
    FXG_PROFILE_BEGIN(c);
    if (opts->copy_begin == 0) {
        FXG_LAUNCH(c, fxg_kernel_uc_sizes, grid, FXG_BLOCK, 0, a);
        FXG_TRY(fxg_scan_u64(c, a.size, M, fxg_uc_levels(a)));
        FXG_TRY(fxg_scan_u64(c, a.pieces, M, fxg_uc_levels(a)));
    }
    FXG_LAUNCH(c, fxg_kernel_uc_window, 1, 1, 0, a, (u64)opts->copy_begin, (u64)opts->out_cap);
    FXG_PROFILE_END(c);
    u64 res[FXG_UC_RES_WORDS];
    FXG_HIP(c, hipMemcpyAsync(res, a.res, sizeof res, hipMemcpyDeviceToHost, c->stream));
    FXG_HIP(c, hipStreamSynchronize(c->stream));                // nothing may be written before the window is known to fit
    if (opts->copy_begin == 0) { c->uc_records = n; c->uc_base = opts->ordinal_base; c->uc_ready = 1; }
    FxgUcWindow w;
    FXG_TRY(fxg_uc_results(res, opts, d_out != nullptr, info, &w, c->err, sizeof c->err));
    // the copy launches cover the window, not the block: a group of 16 lanes per record and per further piece that holds copies of it
    const u64 hgrid = info->out_bytes ? ((w.r_hi - w.r_lo + 1) * 16 + FXG_BLOCK - 1) / FXG_BLOCK : 0, tgrid = ((w.p_hi - w.p_lo) * 16 + FXG_BLOCK - 1) / FXG_BLOCK;
    if (hgrid > 0x7FFFFFFFull || tgrid > 0x7FFFFFFFull) {
        memset(info, 0, sizeof *info);
        return fxg_fail(c, FXG_E_INVALID, "fxg_fasta_uncollapse: the window holds copies of too many records or pieces for one launch (2^27 groups); give it a smaller out_cap");
    }
    FXG_PROFILE_BEGIN(c);
    if (hgrid) FXG_LAUNCH(c, fxg_kernel_uc_copy_heads, (u32)hgrid, FXG_BLOCK, 0, a, w);
    if (tgrid) FXG_LAUNCH(c, fxg_kernel_uc_copy_tails, (u32)tgrid, FXG_BLOCK, 0, a, w);
    FXG_PROFILE_END(c);
    FXG_HIP(c, hipStreamSynchronize(c->stream));
    if (hgrid) fxg_note_launch(c, tgrid > hgrid ? "fxg_kernel_uc_copy_tails" : "fxg_kernel_uc_copy_heads", (u32)(tgrid > hgrid ? tgrid : hgrid), FXG_BLOCK, 0, 0);      // the larger of the two copy launches
    return FXG_OK;
}

// ------------------------------------------------------------------------------------------------
// fasta_nucleotide_changer (fxg_nucchange.h): one launch, groups of 16 lanes that take a record at a time
// ------------------------------------------------------------------------------------------------
// (C linkage from its declaration in include/fxg.h.  Its rows in the table of first calls, tests/context_state_cases.py: bases_change_other_contexts_lines,
// bases_change_no_records.)
int fxg_bases_change(fxg_ctx *c, uint8_t *d_text, uint64_t text_len, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines, uint64_t records,
                     int from, int to, fxg_bases_change_info *info)
{
    if (!c) return FXG_E_INVALID;
    FXG_TRY(fxg_nc_check(d_text, text_len, lines_per_record, d_line, cap_lines, records, from, to, info, c->err, sizeof c->err));
    if (records == 0) return FXG_OK;
    FXG_HIP(c, hipSetDevice(c->device));
    if (!c->nc_res) FXG_HIP(c, hipMalloc((void **)&c->nc_res, FXG_NC_RES_WORDS * sizeof(u64)));
    u64 res[FXG_NC_RES_WORDS];
    fxg_nc_res_init(res);
    FXG_HIP(c, hipMemcpyAsync(c->nc_res, res, sizeof res, hipMemcpyHostToDevice, c->stream));      // (pageable: the copy is staged before the call returns)
    const FxgNcArgs a = fxg_nc_args(d_text, lines_per_record, d_line, cap_lines, records, from, to, c->nc_res);
    const u64 grid = fxg_nc_grid(records);                       // FXG_NC_GRID_MAX at the most
    FXG_PROFILE_BEGIN(c);
    FXG_LAUNCH(c, fxg_kernel_bases_change, (u32)grid, FXG_BLOCK, 0, a);
    FXG_PROFILE_END(c);
    FXG_HIP(c, hipMemcpyAsync(res, c->nc_res, sizeof res, hipMemcpyDeviceToHost, c->stream));
    FXG_HIP(c, hipStreamSynchronize(c->stream));
    fxg_nc_results(res, info);
    fxg_note_launch(c, "fxg_kernel_bases_change", (u32)grid, FXG_BLOCK, 0, 0);
    return FXG_OK;
}

// ------------------------------------------------------------------------------------------------
// fastx_collapser (fxg_collapse.h): the set of a context -- copy + check, rebuild, insert per block; mark, scan, scatter, replay, sizes; windows
// ------------------------------------------------------------------------------------------------
// the backend of fxg_cl_begin / _add / _order / _write: the context's stream
struct FxgClEngine {
    fxg_ctx *c; char *err; size_t cap;
    int alloc(void **p, u64 bytes, const char *what)
    {
        if (hipMalloc(p, bytes) == hipSuccess) return FXG_OK;
        (void)hipGetLastError();
        *p = nullptr;
        return fxg_fail(c, FXG_E_NOMEM, "fxg_collapse: the set wanted %llu bytes for %s, and the device did not have them", (unsigned long long)bytes, what);
    }
    void release(void *p) { (void)hipStreamSynchronize(c->stream); (void)hipFree(p); }
    int zero(void *p, u64 bytes) { FXG_HIP(c, hipMemsetAsync(p, 0, bytes, c->stream)); return FXG_OK; }
    int copy(void *dst, const void *src, u64 bytes) { FXG_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream)); return FXG_OK; }
    int up(void *dst, const void *src, u64 bytes) { FXG_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream)); return sync(); }
    int down(void *dst, const void *src, u64 bytes) { FXG_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); return sync(); }
    int sync() { FXG_HIP(c, hipStreamSynchronize(c->stream)); return FXG_OK; }
    int scan(u64 *data, u64 n, u64 *levels) { return fxg_scan_u64(c, data, n, levels); }
    int lens(const uint16_t *dlen, u64 n, u64 *tmp) { FXG_LAUNCH(c, fxg_kernel_cl_lens, (u32)((n + FXG_BLOCK) / FXG_BLOCK), FXG_BLOCK, 0, dlen, n, tmp); return FXG_OK; }
    int copy_check(const FxgClAddArgs &a) { FXG_LAUNCH(c, fxg_kernel_cl_copy, (u32)fxg_cl_grid(a.n * FXG_CL_LANES, FXG_CL_GRID_MAX), FXG_BLOCK, 0, a); return FXG_OK; }
    int init(u64 *slots, u64 nslots) { FXG_LAUNCH(c, fxg_kernel_cl_init, (u32)fxg_cl_grid(nslots, FXG_CL_SLOT_GRID_MAX), FXG_BLOCK, 0, slots, nslots); return FXG_OK; }
    int rebuild(const u64 *old, u64 nold, const FxgClSet &s, u32 hash_bits) { FXG_LAUNCH(c, fxg_kernel_cl_rebuild, (u32)fxg_cl_grid(nold, FXG_CL_SLOT_GRID_MAX), FXG_BLOCK, 0, old, nold, s, hash_bits); return FXG_OK; }
    int insert(const FxgClSet &s, u64 rec0, u64 n, u32 hash_bits)
    {
        const u64 grid = (n + FXG_BLOCK - 1) / FXG_BLOCK;            // a block's records are fewer than 2^31 (its line index is 32 bits wide)
        FXG_LAUNCH(c, fxg_kernel_cl_insert, (u32)grid, FXG_BLOCK, 0, s, rec0, n, hash_bits);
        fxg_note_launch(c, "fxg_kernel_cl_insert", (u32)grid, FXG_BLOCK, FXG_CL_STAGE_BYTES, FXG_BLOCK);
        return FXG_OK;
    }
    int mark(const FxgClSet &s, u64 *flags) { FXG_LAUNCH(c, fxg_kernel_cl_mark, (u32)fxg_cl_grid(s.nslots, FXG_CL_SLOT_GRID_MAX), FXG_BLOCK, 0, s, flags); return FXG_OK; }
    int scatter(const FxgClOrd &o) { FXG_LAUNCH(c, fxg_kernel_cl_scatter, (u32)fxg_cl_grid(o.s.nslots, FXG_CL_SLOT_GRID_MAX), FXG_BLOCK, 0, o); return FXG_OK; }
    int sizes(const FxgClOrd &o) { FXG_LAUNCH(c, fxg_kernel_cl_sizes, (u32)fxg_cl_grid(o.uniques + 1, FXG_CL_SLOT_GRID_MAX), FXG_BLOCK, 0, o); return FXG_OK; }
    int window(const FxgClOrd &o, u64 rank_begin, u64 out_cap) { FXG_LAUNCH(c, fxg_kernel_cl_window, 1, 1, 0, o, rank_begin, out_cap); return FXG_OK; }
    int write(const FxgClOrd &o, u64 rank_begin, u64 rank_end)
    {
        const u64 grid = ((rank_end - rank_begin) * FXG_CL_LANES + FXG_BLOCK - 1) / FXG_BLOCK;
        FXG_LAUNCH(c, fxg_kernel_cl_write, (u32)grid, FXG_BLOCK, 0, o, rank_begin, rank_end);
        fxg_note_launch(c, "fxg_kernel_cl_write", (u32)grid, FXG_BLOCK, 0, 0);
        return FXG_OK;
    }
    void interval_begin() { if (c->profiling) (void)hipEventRecord(c->kev0[c->kev_count % FXG_KEV_RING], c->stream); }
    void interval_end() { if (c->profiling) { (void)hipEventRecord(c->kev1[c->kev_count % FXG_KEV_RING], c->stream); c->kev_count++; } }
};

// (C linkage from their declarations in include/fxg.h, as fxg_bases_change above.  Their rows in the table of first calls, tests/context_state_cases.py: collapse_*.)
int fxg_collapse_begin(fxg_ctx *c, const fxg_collapse_opts *opts)
{
    if (!c) return FXG_E_INVALID;
    FXG_HIP(c, hipSetDevice(c->device));
    if (!c->cl && !(c->cl = (FxgClState *)calloc(1, sizeof(FxgClState)))) return FXG_E_NOMEM;
    FxgClEngine b = {c, c->err, sizeof c->err};
    return fxg_cl_begin(b, *c->cl, opts);
}

// a context without a set: every call but begin is refused by the state's own checks
static FxgClState *fxg_cl_state(fxg_ctx *c, FxgClState *none) { memset(none, 0, sizeof *none); return c->cl ? c->cl : none; }

int fxg_collapse_add(fxg_ctx *c, const uint8_t *d_text, uint64_t text_len, int lines_per_record, const uint32_t *d_line, uint64_t cap_lines, uint64_t records,
                     const uint16_t *d_len, fxg_collapse_info *info)
{
    if (!c) return FXG_E_INVALID;
    FxgClState none;
    FxgClEngine b = {c, c->err, sizeof c->err};
    FXG_HIP(c, hipSetDevice(c->device));
    return fxg_cl_add(b, *fxg_cl_state(c, &none), d_text, text_len, lines_per_record, d_line, cap_lines, records, d_len, info);
}

int fxg_collapse_order(fxg_ctx *c, fxg_collapse_info *info)
{
    if (!c) return FXG_E_INVALID;
    FxgClState none;
    FxgClEngine b = {c, c->err, sizeof c->err};
    FXG_HIP(c, hipSetDevice(c->device));
    return fxg_cl_order(b, *fxg_cl_state(c, &none), info);
}

int fxg_collapse_write(fxg_ctx *c, uint64_t rank_begin, uint64_t out_cap, uint8_t *d_out, fxg_collapse_window *window)
{
    if (!c) return FXG_E_INVALID;
    FxgClState none;
    FxgClEngine b = {c, c->err, sizeof c->err};
    FXG_HIP(c, hipSetDevice(c->device));
    return fxg_cl_write(b, *fxg_cl_state(c, &none), rank_begin, out_cap, d_out, window);
}

#include "fxg_collapse_rows_engine.h"      // fxg_collapse_add_rows: its launches and its entry

extern "C" int fxg_host_register(fxg_ctx *c, void *ptr, size_t bytes)
{
    if (!c || !ptr) return FXG_E_INVALID;
    FXG_HIP(c, hipHostRegister(ptr, bytes, hipHostRegisterPortable));
    return FXG_OK;
}
extern "C" int fxg_host_unregister(fxg_ctx *c, void *ptr)
{
    if (!c || !ptr) return FXG_E_INVALID;
    FXG_HIP(c, hipHostUnregister(ptr));
    return FXG_OK;
}

// ------------------------------------------------------------------------------------------------
// several GPUs: shard ranges, the epilogue arithmetic and the concatenation (host only)
// ------------------------------------------------------------------------------------------------
extern "C" int fxg_device_numa_node(int device)
{
    char id[64] = {0}, path[128];
    if (hipDeviceGetPCIBusId(id, (int)sizeof id - 1, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char *q = id; *q; ++q) if (*q >= 'A' && *q <= 'F') *q = (char)(*q - 'A' + 'a');       // sysfs names are lower case
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", id);
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

extern "C" int fxg_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

extern "C" int fxg_concat_peer(fxg_ctx *dst, void *d_dst, uint64_t byte_off, fxg_ctx *src, const void *d_src, uint64_t bytes)
{
    if (!dst || !src || (!d_dst && bytes) || (!d_src && bytes)) return FXG_E_INVALID;
    if (!bytes) return FXG_OK;
    FXG_HIP(src, hipSetDevice(src->device));
    if (dst->device == src->device) FXG_HIP(src, hipMemcpyAsync((char *)d_dst + byte_off, d_src, bytes, hipMemcpyDeviceToDevice, src->stream));
    else FXG_HIP(src, hipMemcpyPeerAsync((char *)d_dst + byte_off, dst->device, d_src, src->device, bytes, src->stream));
    return FXG_OK;
}

// the multi-GPU host code (shard ranges, epilogue, concatenation, RCCL transport) is fxg_comm.h: it reaches device memory through
// these hooks only, so that the CPU tier compiles the very same code over host memory (tests/emu/fxg_stub.cpp)
#define FXG_COMM_FAIL(c, code, ...) fxg_fail(c, code, __VA_ARGS__)
#define FXG_COMM_SET_DEVICE(c) (hipSetDevice((c)->device) == hipSuccess)
#define FXG_COMM_MALLOC(pp, bytes) (hipMalloc((void **)(pp), (bytes)) == hipSuccess)
#define FXG_COMM_FREE(p) ((void)hipFree(p))
#define FXG_COMM_STREAM(c) ((void *)(c)->stream)
#define FXG_COMM_SCRATCH(c) ((const uint64_t *)(c)->counters_scratch)
static const char *fxg_comm_d2h_sync(fxg_ctx *c, void *dst, const void *src, size_t bytes)
{
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? nullptr : hipGetErrorString(e);
}
#include "fxg_comm.h"

extern "C" int fxg_set_profiling(fxg_ctx *c, int enabled)
{
    if (!c) return FXG_E_INVALID;
    if (enabled && !c->kev_ready) {                          // the event ring is made on first use: all 2 x FXG_KEV_RING events, or none
        FXG_HIP(c, hipSetDevice(c->device));
        hipError_t e = hipSuccess;
        for (int i = 0; i < FXG_KEV_RING && e == hipSuccess; ++i) { e = hipEventCreate(&c->kev0[i]); if (e == hipSuccess) e = hipEventCreate(&c->kev1[i]); }
        if (e != hipSuccess) {                               // a ring with holes would be recorded into and waited on through null events
            for (int i = 0; i < FXG_KEV_RING; ++i) {
                if (c->kev0[i]) (void)hipEventDestroy(c->kev0[i]);
                if (c->kev1[i]) (void)hipEventDestroy(c->kev1[i]);
                c->kev0[i] = c->kev1[i] = nullptr;
            }
            c->profiling = 0;
            return fxg_fail(c, FXG_E_HIP, "hipEventCreate failed: %s (profiling stays off)", hipGetErrorString(e));
        }
        c->kev_ready = 1;
    }
    c->profiling = enabled ? 1 : 0;
    c->kev_count = 0;
    return FXG_OK;
}

#ifdef FXG_ABLATION
// timing experiments only (scripts/ablate.py): the phase clocks fxg_kernel_rows adds up in the control block, words 10..
extern "C" int fxg_debug_phase_clocks(fxg_ctx *c, uint64_t out[11])
{
    if (!c || !out) return FXG_E_INVALID;
    FXG_HIP(c, hipStreamSynchronize(c->stream));
    FXG_HIP(c, hipMemcpy(out, c->errflag + 10, 11 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return FXG_OK;
}
#endif

extern "C" int fxg_last_kernel_ms(fxg_ctx *c, float *ms)
{
    if (!c || !ms) return FXG_E_INVALID;
    if (!c->kev_count) return fxg_fail(c, FXG_E_INVALID, "no profiled launch recorded");
    const int k = (int)((c->kev_count - 1) % FXG_KEV_RING);
    FXG_HIP(c, hipEventSynchronize(c->kev1[k]));
    FXG_HIP(c, hipEventElapsedTime(ms, c->kev0[k], c->kev1[k]));
    return FXG_OK;
}

extern "C" int fxg_profiled_kernel_ms(fxg_ctx *c, float *ms, uint32_t cap, uint32_t *n)
{
    if (!c || !ms || !n) return FXG_E_INVALID;
    const u64 have = c->kev_count < FXG_KEV_RING ? c->kev_count : FXG_KEV_RING;
    const u32 k = (u32)(have < cap ? have : cap);
    *n = 0;
    for (u32 i = 0; i < k; ++i) {                            // oldest first
        const int slot = (int)((c->kev_count - k + i) % FXG_KEV_RING);
        FXG_HIP(c, hipEventSynchronize(c->kev1[slot]));
        FXG_HIP(c, hipEventElapsedTime(&ms[i], c->kev0[slot], c->kev1[slot]));
    }
    *n = k;
    return FXG_OK;
}

extern "C" int fxg_last_launch_info(const fxg_ctx *c, char *name, size_t cap, uint32_t *grid, uint32_t *block, uint32_t *lds,
                                    uint32_t *tile)
{
    if (!c) return FXG_E_INVALID;
    if (name && cap) snprintf(name, cap, "%s", c->last_kernel);
    if (grid) *grid = c->last_grid;
    if (block) *block = c->last_block;
    if (lds) *lds = c->last_lds;
    if (tile) *tile = c->last_tile;
    return FXG_OK;
}

#ifndef FXG_SPLIT      // a single-unit build: the clip instances here as well
#include "fxg_engine_clip.hip"
#endif
