// fxg_attr.h -- the decision of fxg_kernel_fit (fxg_host.h): when a kernel's MaxDynamicSharedMemorySize attribute is set, and to what.  Host only and free of
// the runtime, so that the engine and the CPU tier (tests/emu/attr_emu.cpp) compile this one copy, like the plan code of fxg_plan.h.
//
// The invariant: AT EVERY LAUNCH, THE VALUE LAST SET FOR THAT KERNEL ON THAT DEVICE IN THE PROCESS IS AT LEAST THE LAUNCH'S DYNAMIC LDS SIZE.
// The attribute belongs to the function in the process (and device), not to a context: several contexts of one process (the host layer makes one per lane
// and per device) launch the same kernels with different LDS sizes (fxg_plan_lds varies with stride, tile and depth).  So what was set is remembered in ONE
// table per process, keyed by (device, kernel), under a lock, and the attribute is only ever raised: nobody can lower what somebody else relies on.  The
// table grows with the kernels it meets -- it has no capacity to run out of -- and the lock is held across the runtime's call, so that the table and the
// runtime never disagree about which of two racing sets came last.
//
// What a context keeps for itself is the occupancy answer per (kernel, LDS size), FXG_FIT_SLOTS of them: a hit there means this context went through the
// table with that very size before, and since the table never lowers, the attribute still covers it.
#pragma once
#include <cstdint>
#include <mutex>
#include <vector>

struct FxgAttrEntry { int device; const void *kernel; uint32_t lds_max; };
struct FxgAttrTable {
    std::mutex mu;
    std::vector<FxgAttrEntry> set;      // one entry per (device, kernel) whose attribute was ever set
};

// the process's table (the engine's; the CPU tier replays sequences into tables of its own)
static inline FxgAttrTable &fxg_attr_process_table()
{
    static FxgAttrTable t;
    return t;
}

// Makes sure the attribute of `kernel` on `device` covers `lds`: calls set(lds) -- the runtime's call, 0 for success -- only when nothing as large was set
// before, and remembers the value only when the call succeeded.  Returns what set returned, 0 when there was nothing to do.
template <typename Set>
static inline int fxg_attr_cover(FxgAttrTable &t, int device, const void *kernel, uint32_t lds, Set set)
{
    std::lock_guard<std::mutex> hold(t.mu);
    FxgAttrEntry *e = nullptr;
    for (FxgAttrEntry &x : t.set) if (x.device == device && x.kernel == kernel) { e = &x; break; }
    if (e && e->lds_max >= lds) return 0;
    const int rc = set(lds);
    if (rc != 0) return rc;
    if (e) e->lds_max = lds;
    else t.set.push_back(FxgAttrEntry{device, kernel, lds});
    return 0;
}

// a context's occupancy answers
#define FXG_FIT_SLOTS 8
struct FxgFitCache {
    const void *kernel[FXG_FIT_SLOTS];
    uint32_t lds[FXG_FIT_SLOTS];
    int per_cu[FXG_FIT_SLOTS];
    int next;                           // next slot to evict
};

static inline bool fxg_fit_cached(const FxgFitCache &f, const void *kernel, uint32_t lds, int *per_cu)
{
    for (int i = 0; i < FXG_FIT_SLOTS; ++i)
        if (f.kernel[i] == kernel && f.lds[i] == lds) { *per_cu = f.per_cu[i]; return true; }
    return false;
}

static inline void fxg_fit_remember(FxgFitCache &f, const void *kernel, uint32_t lds, int per_cu)
{
    int slot = -1;
    for (int i = 0; i < FXG_FIT_SLOTS; ++i) if (!f.kernel[i]) { slot = i; break; }
    if (slot < 0) { slot = f.next; f.next = (f.next + 1) % FXG_FIT_SLOTS; }
    f.kernel[slot] = kernel; f.lds[slot] = lds; f.per_cu[slot] = per_cu;
}

// The whole decision for one launch: *per_cu from the context's cache, or set (through the table, when needed) and ask(&per_cu) -- the runtime's occupancy
// question, 0 for success.  Returns the first non-zero answer of set / ask, else 0.
template <typename Set, typename Ask>
static inline int fxg_fit_decide(FxgAttrTable &t, FxgFitCache &f, int device, const void *kernel, uint32_t lds, int *per_cu, Set set, Ask ask)
{
    if (fxg_fit_cached(f, kernel, lds, per_cu)) return 0;
    int rc = fxg_attr_cover(t, device, kernel, lds, set);
    if (rc != 0) return rc;
    rc = ask(per_cu);
    if (rc != 0) return rc;
    if (*per_cu >= 1) fxg_fit_remember(f, kernel, lds, *per_cu);
    return 0;
}
