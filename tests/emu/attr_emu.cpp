// attr_emu.cpp -- test-only door to the engine's decision about the kernels' dynamic-LDS attribute (csrc/fxg_attr.h: fxg_fit_decide), which fxg_kernel_fit
// runs before every launch of a tile kernel.  A sequence of launches (context, device, kernel, LDS size) is replayed through that very function, in one
// "process" (a table of its own) with one occupancy cache per context, and every call of the runtime's setter comes back as a log entry.  What the log means
// -- whether every launch was covered by what was last set -- is for tests/test_context_state_cpu.py to judge, not for this file.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../fastx_toolkit_amd/csrc/fxg_attr.h"

struct fxg_emu_attr_set { uint64_t step; int32_t device, kernel; uint32_t lds; };

// launches [0, n): ctx[i] < nctx, kernel[i] >= 0.  log: the sets in order, at most `cap` written.  *asked: occupancy questions (cache misses).
// Returns the number of sets, or -1 for a bad sequence.
extern "C" long long fxg_emu_attr_replay(const int32_t *ctx, const int32_t *device, const int32_t *kernel, const uint32_t *lds, uint64_t n, int32_t nctx,
                                         fxg_emu_attr_set *log, uint64_t cap, uint64_t *asked)
{
    if (nctx < 1 || nctx > 64) return -1;
    FxgAttrTable table;
    std::vector<FxgFitCache> fit((size_t)nctx);
    memset(fit.data(), 0, fit.size() * sizeof(FxgFitCache));
    uint64_t sets = 0, asks = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (ctx[i] < 0 || ctx[i] >= nctx || kernel[i] < 0) return -1;
        const void *k = (const void *)(uintptr_t)((uint64_t)kernel[i] + 1u) ;      // (a kernel is its address to the engine; 0 is the empty slot)
        int per_cu = 0;
        const int rc = fxg_fit_decide(table, fit[(size_t)ctx[i]], device[i], k, lds[i], &per_cu,
            [&](uint32_t v) { if (sets < cap) log[sets] = fxg_emu_attr_set{i, device[i], kernel[i], v}; ++sets; return 0; },
            [&](int *p) { ++asks; *p = 1; return 0; });
        if (rc != 0 || per_cu != 1) return -1;
    }
    if (asked) *asked = asks;
    return (long long)sets;
}
