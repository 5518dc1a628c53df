// fxg_knobs.h -- THE list of the environment variables the engine reads, and the one function that reads them.  Nothing else under csrc/ calls getenv
// (but FXG_DEBUG, which only the ablation / debug builds have: fxg_host.h, and FXG_COMM_JOB, the rendezvous name of fxg_comm.h, which is no launch knob).
// The plan (fxg_plan.h) takes the struct as a parameter, so what a request runs is a function of the request, the context and this struct -- in the engine
// and in the CPU tier's emulator alike (tests/test_plan_cpu.py holds every row below to its parsing).
//
// A row: the scope (REQUEST: read at the top of every entry point that uses one -- fxg_run_pipeline, fxg_run_quality_stats, fxg_read_counters -- so a
// change between two calls on one context takes effect; CONTEXT: read once, by fxg_ctx_create), the field of FxgKnobs, the variable, how its text is
// parsed, the accepted range, the value of the field when the variable is unset or its number is outside the range, and what the knob is for.
//   INT   atoi of the text (the empty string is 0)
//   TRI   -1 unset, else atoi != 0: three states, for choices the plan makes itself when nobody asks
//   FLAG  1 when set at all -- to "0" or to the empty string too
//   UL0   strtoul with base 0 (so 0x.. and 0.. work)
#pragma once
#include <climits>
#include <cstdlib>

#include "fxg_device.h"

#define FXG_KNOB_TABLE(X) \
    X(REQUEST, tile,             "FXG_TILE",              INT,  INT_MIN, INT_MAX, 0,  "reads per tile of the tile kernels: a power of two up to the instance's block size (checked there: fxg_pick_tile)") \
    X(REQUEST, rows,             "FXG_ROWS",              INT,  INT_MIN, INT_MAX, 1,  "the rows kernels (fxg_rows.h): 0 never, 1 where they are ahead (unset), 2 and more wherever one exists") \
    X(REQUEST, clip_global,      "FXG_CLIP_GLOBAL",       TRI,  0,       1,       -1, "the two-pass clip forms run their DP over the batch (1) or over the staged tile (0); unset: the plan decides") \
    X(REQUEST, rev_dw,           "FXG_REV_DW",            TRI,  0,       1,       -1, "reverse complement with dword-aligned window loads (fxg_kernel_tiles<0,5>) forced on or off (measurements)") \
    X(REQUEST, clip_k_one_pass,  "FXG_CLIP_K_ONE_PASS",   FLAG, 0,       1,       0,  "adapters of 17..99 bases never run the two-pass form with checkpoint scratch") \
    X(REQUEST, no_packed_clip,   "FXG_NO_PACKED_CLIP",    FLAG, 0,       1,       0,  "every clip request runs the general two-word form") \
    X(REQUEST, clip_depth,       "FXG_CLIP_DEPTH_RT",     INT,  2,       4,       0,  "slots between a clip tile's decision and its write-out at most (unset: FXG_CLIP_DEPTH)") \
    X(REQUEST, qs_round_robin,   "FXG_QS_ROUND_ROBIN",    UL0,  0,       UINT_MAX, 1, "FxgStatsArgs::round_robin (fxg_stats.h): 0 = one static slice per workgroup, tested loads; 3 = the row-strip form where the piece form would run") \
    X(REQUEST, no_scan_fallback, "FXG_NO_SCAN_FALLBACK",  FLAG, 0,       1,       0,  "fxg_read_counters reports a look-back time-out instead of doing the pass again without the scanner") \
    X(CONTEXT, blocks_per_cu,    "FXG_BLOCKS_PER_CU",     INT,  1,       16,      0,  "workgroups per CU of a tile launch (unset: what fits, at most 8, 16 for one-wave workgroups)") \
    X(CONTEXT, workers,          "FXG_WORKERS",           INT,  1,       INT_MAX, 0,  "cap on the worker workgroups of a launch (tests)") \
    X(CONTEXT, nscan,            "FXG_NSCAN",             INT,  1,       64,      0,  "forced number of scanner waves of the rows kernels (tests)") \
    X(CONTEXT, test_scan_timeout, "FXG_TEST_SCAN_TIMEOUT", INT, 1,       INT_MAX, 0,  "every compacting launch starts with the time-out flag up (GPU tier: the redo without the scanner)") \
    X(CONTEXT, ticket_groups,    "FXG_TICKET_GROUPS",     INT,  1,       FXG_TICKET_GROUPS, 0, "tile dispensers of a launch at most")

struct FxgKnobs {
    int tile, rows, clip_global, rev_dw, clip_k_one_pass, no_packed_clip, clip_depth, no_scan_fallback;
    unsigned qs_round_robin;
    int blocks_per_cu, workers, nscan, test_scan_timeout, ticket_groups;
};
enum FxgKnobScope { FXG_KNOBS_REQUEST, FXG_KNOBS_CONTEXT };

static inline long long fxg_knob_INT(const char *e, long long lo, long long hi, long long unset) { return e && atoi(e) >= lo && atoi(e) <= hi ? atoi(e) : unset; }
static inline long long fxg_knob_TRI(const char *e, long long, long long, long long unset) { return e ? atoi(e) != 0 : unset; }
static inline long long fxg_knob_FLAG(const char *e, long long, long long, long long) { return e != nullptr; }
static inline long long fxg_knob_UL0(const char *e, long long, long long, long long unset) { return e ? (long long)(unsigned)strtoul(e, nullptr, 0) : unset; }

// the knobs of one scope as the environment has them now; the fields of the other scope at their unset values
static inline FxgKnobs fxg_knobs_read(FxgKnobScope scope)
{
    FxgKnobs k;
#define FXG_KNOB_READ(SCOPE, FIELD, NAME, KIND, LO, HI, UNSET, WHAT) k.FIELD = (decltype(k.FIELD))fxg_knob_##KIND(scope == FXG_KNOBS_##SCOPE ? getenv(NAME) : nullptr, LO, HI, UNSET);
    FXG_KNOB_TABLE(FXG_KNOB_READ)
#undef FXG_KNOB_READ
    return k;
}
