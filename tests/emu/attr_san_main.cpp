// attr_san_main.cpp -- stand-alone program for a sanitizer build (thread, or address + undefined): several threads, a context's occupancy cache each, decide
// launches of the same kernels through ONE process table (csrc/fxg_attr.h) while a stand-in for the runtime records what was last set.  After every
// decision the thread checks the invariant for its own launch: the value last set for (device, kernel) is at least the launch's LDS size.  Exit 0: held.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../fastx_toolkit_amd/csrc/fxg_attr.h"

enum { DEVICES = 2, KERNELS = 69, THREADS = 6, LAUNCHES = 20000 };
static std::atomic<uint32_t> runtime_attr[DEVICES][KERNELS];      // what the "runtime" holds: written only inside the table's lock, by set()
static std::atomic<long> broken, lowered, sets;

static void lane(FxgAttrTable *table, int t)
{
    FxgFitCache fit;
    memset(&fit, 0, sizeof fit);
    const int device = t % DEVICES;
    uint32_t x = 12345u + 977u * (uint32_t)t;
    for (int i = 0; i < LAUNCHES; ++i) {
        x = x * 1664525u + 1013904223u;
        const int k = (int)((x >> 8) % KERNELS);
        const uint32_t lds = ((x >> 20) % 7u) * 9216u + ((x >> 4) & 16u);
        int per_cu = 0;
        const int rc = fxg_fit_decide(*table, fit, device, (const void *)(uintptr_t)(k + 1), lds, &per_cu,
            [&](uint32_t v) { if (v < runtime_attr[device][k].load()) ++lowered; runtime_attr[device][k].store(v); ++sets; return 0; },
            [&](int *p) { *p = 2; return 0; });
        if (rc != 0 || per_cu != 2 || runtime_attr[device][k].load() < lds) ++broken;
    }
}

int main()
{
    FxgAttrTable table;
    std::vector<std::thread> th;
    for (int t = 0; t < THREADS; ++t) th.emplace_back(lane, &table, t);
    for (auto &x : th) x.join();
    printf("%ld sets, %zu table entries, %ld launches uncovered, %ld sets that lowered\n", sets.load(), table.set.size(), broken.load(), lowered.load());
    return broken.load() == 0 && lowered.load() == 0 && table.set.size() <= (size_t)DEVICES * KERNELS ? 0 : 1;
}
