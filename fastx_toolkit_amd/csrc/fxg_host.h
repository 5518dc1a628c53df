// fxg_host.h -- what the translation units of the engine share on the host side: the context, the error macros, the launch of one instance of a tile
// kernel.  The engine is built from several translation units compiled side by side (fastx_toolkit_amd/build.py): fxg_engine.hip (every entry point of the
// C-ABI and every kernel but the clipper's) and fxg_engine_clip.hip once per unit of clip instances (-DFXG_CLIP_TU=k; fxg_clip_instances.h lists the units
// and says why).  Compiled alone (no -DFXG_SPLIT: the variant / matrix / ablation builds of scripts/) fxg_engine.hip includes the clip file and is the one
// translation unit it used to be.
#pragma once
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <fcntl.h>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>

#include "fxg_attr.h"
#include "fxg_plan.h"
#include "fxg_rows.h"

struct FxgTextState;
struct FxgClState;

struct fxg_ctx {
    int device;
    int cus;
    hipStream_t own_stream;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
#define FXG_KEV_RING 64
    hipEvent_t kev0[FXG_KEV_RING], kev1[FXG_KEV_RING];  // around the dominant kernel of the last FXG_KEV_RING launches when profiling
    int profiling;
    u64 kev_count;          // profiled launches since fxg_set_profiling(1)
    int kev_ready;          // every event of both rings exists
    u64 *status;            // FXG_STATUS_WORDS(status_cap) granules: tile totals [cap], prefixes [2 * cap], batch bases
    size_t status_cap;      // in tiles
    u32 epoch;              // tag of the granules of the current launch (1..255); 0 = never valid
    FxgFitCache fit;        // occupancy answer per (kernel, LDS size); what the kernels' LDS attributes were set to is the process's to know (fxg_attr.h)
    FxgKnobs knobs;         // the CONTEXT rows of fxg_knobs.h, read once (fxg_ctx_create)
    u32 *errflag;           // [0] device error bits; tile dispensers start at word FXG_TICKET_STRIDE
    u64 *counters_scratch;  // used when the caller passes no counter block
    u64 *text_ws;           // newline census / scan levels / format items
    size_t text_ws_cap;     // in u64 words
    FxgTextState *text_state;
    // clip history (fxg_set_clip_history): the reference aligner's query buffer, carried from batch to batch
    int hist_on;
    int hist_has_adapter;   // a batch went through this history: the adapter of every later one must be the same (one history is one reference process)
    char hist_adapter[FXG_MAX_ADAPTER + 1];
    u32 hist_wcap;          // host-side upper bound of the buffer width (the exact width lives on the device)
    int hist_cur;           // which of hist_buf[2] / hist_w[2] is current
    uint8_t *hist_buf[2];
    u32 *hist_w;            // [2]
    uint8_t *hist_ws;       // M, BT, ext, wlen
    size_t hist_ws_cap;
    float *clip_ck;         // fxg_clip_two_pass_k: checkpoint scratch, FxgPlan.ck_per_wg floats per workgroup
    size_t clip_ck_cap;     // in floats
    u32 *stats_ws;          // fxg_run_quality_stats: one u32 partial histogram per workgroup
    size_t stats_ws_cap;    // in u32 words
    char err[512];
    char last_kernel[96];
    u32 last_grid, last_block, last_lds, last_tile;
    // the last compacting launch, kept so that it can be done again without the scanner when its waits timed out (fxg_fallback.h)
    struct { FxgKArgs ka; u64 *counters; int valid; } fb;                                      // the launch (fxg_launch_tiles): its arguments as the kernel got them
    struct { fxg_batch in; fxg_params p; fxg_out out; bool hist; u32 estride; int valid; } fb_req;      // the request (fxg_run_pipeline)
    u64 *fb_blk; size_t fb_blk_cap;     // block sums / prefixes of the fallback
    int recoveries;                     // launches redone that way since the context was made (fxg_scan_recoveries)
    // barcode splitter (fxg_barcode_prepare / _split): the encoded table and the workspace of the per-(bin, tile) counts
    struct FxgBcEntry *bc_tab;
    size_t bc_tab_cap;                  // in entries
    u32 bc_entries, bc_len, bc_mm, bc_eol, bc_bins;
    int bc_ready;
    u64 *bc_ws;
    size_t bc_ws_cap;                   // in u64 words
    u64 *rf_ws;                         // fxg_fasta_reflow: the items' arrays, the scans' levels, the result words (fxg_reflow.h)
    size_t rf_ws_cap;                   // in u64 words
    u64 *uc_ws;                         // fxg_fasta_uncollapse: the records' arrays, the scans' levels, the result words (fxg_uncollapse.h); kept from window to window
    size_t uc_ws_cap;                   // in u64 words
    u64 uc_records, uc_base;            // what the scans in uc_ws were made for (a call with copy_begin > 0 must name the same)
    int uc_ready;
    u64 *nc_res;                        // fxg_bases_change: the launch's result words (fxg_nucchange.h)
    FxgClState *cl;                     // fxg_collapse_*: the set and what the host knows of it (fxg_collapse.h), made by the first fxg_collapse_begin
};

__attribute__((unused)) static int fxg_fail(fxg_ctx *ctx, int code, const char *fmt, ...)
{
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof ctx->err, fmt, ap);
        va_end(ap);
    }
    return code;
}

#define FXG_HIP(ctx, call)                                                                              \
    do {                                                                                                \
        hipError_t e__ = (call);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return fxg_fail(ctx, FXG_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)
#define FXG_TRY(call) do { const int rc__ = (call); if (rc__ != FXG_OK) return rc__; } while (0)

// the -v report counters of a launch: the tile kernel tallied them, one tiny kernel lays them out (defined with that kernel, in fxg_engine.hip)
#define FXG_INTERNAL __attribute__((visibility("hidden")))      /* between the engine's translation units; not part of the C-ABI */
FXG_INTERNAL int fxg_enqueue_finish_counters(fxg_ctx *c, const FxgKArgs &ka, u64 *counters);
// the clip instances, one launch function per unit (fxg_engine_clip.hip): FXG_CLIP_NOT_MINE for a plan whose instance another unit holds
#define FXG_CLIP_NOT_MINE 1
#define FXG_CLIP_UNIT_FN_(K) fxg_launch_clip_unit##K
#define FXG_CLIP_UNIT_FN(K) FXG_CLIP_UNIT_FN_(K)
#define FXG_CLIP_DECLARE_UNIT(K) FXG_INTERNAL int FXG_CLIP_UNIT_FN(K)(fxg_ctx *c, FxgPlan &pl, u64 *ctr);
FXG_CLIP_FOR_UNITS(FXG_CLIP_DECLARE_UNIT)

#define FXG_LAUNCH(c, kernel, grid, block, lds, ...) do { hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, (c)->stream, __VA_ARGS__); FXG_HIP(c, hipGetLastError()); } while (0)      // one launch on the context's stream, checked
// with profiling on, what is queued between the pair is one entry of the event ring (fxg_last_kernel_ms, fxg_profiled_kernel_ms)
#define FXG_PROFILE_BEGIN(c) do { if ((c)->profiling) FXG_HIP(c, hipEventRecord((c)->kev0[(c)->kev_count % FXG_KEV_RING], (c)->stream)); } while (0)
#define FXG_PROFILE_END(c) do { if ((c)->profiling) { FXG_HIP(c, hipEventRecord((c)->kev1[(c)->kev_count % FXG_KEV_RING], (c)->stream)); (c)->kev_count++; } } while (0)

// what fxg_last_launch_info reports: the dominant kernel of the last call and its geometry
static inline void fxg_note_launch(fxg_ctx *c, const char *kname, u32 grid, u32 block, u32 lds, u32 tile)
{
    snprintf(c->last_kernel, sizeof c->last_kernel, "%s", kname);
    c->last_grid = grid; c->last_block = block; c->last_lds = lds; c->last_tile = tile;
}

// A workspace that only grows: at least `need` units at p afterwards.  A block too small goes, after the work queued on the stream that may still use it, and
// one of `cap` units (need plus the site's margin; `bytes` where that is not cap elements of T) takes its place: p and have are null / 0 if that allocation fails.  *fresh: the block is new.
template <typename T>
static int fxg_ws_grow(fxg_ctx *c, T *&p, size_t &have, size_t need, size_t cap, bool *fresh = nullptr, size_t bytes = 0)
{
    if (fresh) *fresh = have < need;
    if (have >= need) return FXG_OK;
    if (p) FXG_HIP(c, hipStreamSynchronize(c->stream));
    (void)hipFree(p); p = nullptr; have = 0;
    FXG_HIP(c, hipMalloc((void **)&p, bytes ? bytes : cap * sizeof(T)));
    have = cap;
    return FXG_OK;
}

// The dynamic-LDS attribute of a kernel covers `lds` afterwards: set through the process's table (fxg_attr.h), which only ever raises it.  The context's device is current.
template <typename K>
static int fxg_kernel_lds(fxg_ctx *c, K kernel, u32 lds)
{
    hipError_t e = hipSuccess;
    if (fxg_attr_cover(fxg_attr_process_table(), c->device, (const void *)kernel, lds,
                       [&](u32 v) { e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v); return e == hipSuccess ? 0 : 1; }))
        return fxg_fail(c, FXG_E_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize, %u) failed: %s", lds, hipGetErrorString(e));
    return FXG_OK;
}

// dynamic-LDS attribute and occupancy of a kernel: asked once per (kernel, LDS size), not per launch.  What is set when is fxg_fit_decide's to say (fxg_attr.h,
// shared with the CPU tier): one kernel alternating between LDS sizes, in this context or in another one of the process, is never launched with more than was last set.
template <typename K>
static int fxg_kernel_fit(fxg_ctx *c, K kernel, const char *kname, u32 lds, int *per_cu, u32 block = FXG_TBLOCK)
{
    hipError_t e = hipSuccess;
    const char *what = "hipFuncSetAttribute";
    const int rc = fxg_fit_decide(fxg_attr_process_table(), c->fit, c->device, (const void *)kernel, lds, per_cu,
        [&](u32 v) { e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v); return e == hipSuccess ? 0 : 1; },
        [&](int *n) { what = "hipOccupancyMaxActiveBlocksPerMultiprocessor"; e = hipOccupancyMaxActiveBlocksPerMultiprocessor(n, kernel, (int)block, lds); return e == hipSuccess ? 0 : 1; });
    if (rc != 0) return fxg_fail(c, FXG_E_HIP, "%s failed for %s (lds=%u): %s", what, kname, lds, hipGetErrorString(e));
    if (*per_cu < 1) return fxg_fail(c, FXG_E_INVALID, "%s does not fit on a CU (lds=%u)", kname, lds);
    return FXG_OK;
}

// u64 words of the inter-workgroup state for `cap` tiles: totals, two prefixes per tile, two per scanner batch (batches of >= 256 tiles)
#define FXG_STATUS_WORDS(cap) (3 * (size_t)(cap) + 2 * ((size_t)(cap) / 256 + 2))

// one instance of a tile kernel for a planned pass (the instance tables: fxg_instances.h, fxg_clip_instances.h)
template <typename K>
static int fxg_launch_tiles(fxg_ctx *c, K kernel, FxgPlan &pl, u64 *counters, bool rows_kernel = false)
{
    FxgKArgs &ka = pl.ka;
    const char *const kname = fxg_inst_name(pl.inst, pl.amax);
    const u32 lds = pl.lds, block = pl.block;
    const u64 ck_per_wg = pl.ck_per_wg;
    FXG_HIP(c, hipSetDevice(c->device));
    int per_cu = 0;
    FXG_TRY(fxg_kernel_fit(c, kernel, kname, lds, &per_cu, block));
    // Tiles are dispensed by ticket, so nothing depends on every workgroup being resident: fill the chip.
    const int most = block == 64u ? 16 : 8;      // single-wave workgroups (fxg_rows.h, the two-pass clip instances): the LDS allows sixteen per CU
    int use = per_cu > most ? most : per_cu;
    if (c->knobs.blocks_per_cu > 0) use = c->knobs.blocks_per_cu;
    u64 workers = (u64)c->cus * (u64)use;
    if (c->knobs.workers > 0 && workers > (u64)c->knobs.workers) workers = (u64)c->knobs.workers;
    if (workers > ka.ntiles) workers = ka.ntiles;
    if (workers < 1) workers = 1;
    // more workgroups: the scanner(s) (fxg_device.h); fxg_kernel_rows runs several once there is work for them
    ka.nscan = !ka.compact ? 0u : (rows_kernel && workers >= 64u * FXG_ROWS_NSCAN ? (u32)FXG_ROWS_NSCAN : 1u);
    if (ka.compact && rows_kernel && c->knobs.nscan > 0) ka.nscan = (u32)c->knobs.nscan;
    const u64 grid = workers + ka.nscan;

    if (ka.compact) {
        bool fresh = false;
        const size_t cap = (size_t)ka.ntiles + (size_t)ka.ntiles / 4 + 1024;
        FXG_TRY(fxg_ws_grow(c, c->status, c->status_cap, ka.ntiles, cap, &fresh, FXG_STATUS_WORDS(cap) * sizeof(u64)));
        // granules carry the launch's epoch, so the arrays are only cleared when they are new or the 8-bit epoch wraps
        c->epoch = c->epoch >= 255u ? 1u : c->epoch + 1u;
        if (fresh || c->epoch == 1u) FXG_HIP(c, hipMemsetAsync(c->status, 0, FXG_STATUS_WORDS(c->status_cap) * sizeof(u64), c->stream));
        ka.agg = c->status;
        ka.pfx = c->status + c->status_cap;
        ka.bbase = c->status + 3 * c->status_cap;
        ka.tag = c->epoch;
    }
    ka.clip_ck = nullptr;
    if (ck_per_wg) {                             // checkpoint rows of the two-pass clipper (fxg_clip_two_pass_k): written and read by the same thread
        const size_t need = (size_t)grid * (size_t)ck_per_wg;
        FXG_TRY(fxg_ws_grow(c, c->clip_ck, c->clip_ck_cap, need, need));
        ka.clip_ck = c->clip_ck;
    }
#if defined(FXG_ABLATION) || defined(FXG_DBG_BITS)
    { const char *dbg = getenv("FXG_DEBUG"); ka.debug = dbg ? (u32)atoi(dbg) : 0u; }
#endif
    ka.errflag = c->errflag;                     // control block (zeroed before every launch), layout at FXG_CTRL_WORDS
    ka.ticket = c->errflag + FXG_CTRL_WORDS;
    ka.extra = (u64 *)(c->errflag + 2);
    ka.role = c->errflag + 8;
    ka.tally = (u64 *)(c->errflag + 32);
    // Dispenser g serves the workgroups with blockIdx % groups == g, so every group needs a worker even if the scanner role
    // falls to its members: eight groups only when each has more workgroups than there are scanners.
    { u32 g = c->knobs.ticket_groups > 0 ? (u32)c->knobs.ticket_groups : FXG_TICKET_GROUPS; ka.ticket_groups = grid >= (u64)(ka.nscan + 1u) * g ? g : 1u; }
    FXG_HIP(c, hipMemsetAsync(c->errflag, 0, (FXG_CTRL_WORDS + FXG_TICKET_GROUPS * FXG_TICKET_STRIDE) * sizeof(u32), c->stream));
    c->fb.valid = 0;
    if (ka.compact) {                            // what fxg_read_counters needs to do this launch again should its waits time out
        c->fb.ka = ka; c->fb.counters = counters; c->fb.valid = 1;
        if (c->knobs.test_scan_timeout) {            // "somebody already gave up": every wait of this launch that lasts ends without a result
            static const u32 up = FXG_DEV_ERR_SCAN_TIMEOUT;
            FXG_HIP(c, hipMemcpyAsync(c->errflag, &up, sizeof up, hipMemcpyHostToDevice, c->stream));
        }
    }

    FXG_PROFILE_BEGIN(c);
    FXG_LAUNCH(c, kernel, (u32)grid, block, lds, ka);
    FXG_PROFILE_END(c);
    FXG_TRY(fxg_enqueue_finish_counters(c, ka, counters));      // -v report counters: the tile kernel tallied them; one tiny kernel lays them out
    fxg_note_launch(c, kname, (u32)grid, block, lds, ka.tile_reads);
    return FXG_OK;
}
