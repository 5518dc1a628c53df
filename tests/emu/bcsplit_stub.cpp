// bcsplit_stub.cpp -- TEST-ONLY: the barcode splitter's two C-ABI entry points for the emulation stub (fxg_stub.cpp), over bcsplit_emu.cpp.
// tests/test_barcode_cpu.py links it with the stub's own objects into a libfxg.so of its own, so that host/fastx_barcode_splitter runs on a
// machine without a GPU.  The stub's context has no room for a table: they are kept here, one per context.
#include <cstdio>
#include <map>
#include <mutex>

#include "fxg_stub_ctx.h"

struct fxg_emu_bc_table;
extern "C" fxg_emu_bc_table *fxg_emu_bc_prepare(const fxg_barcode_set *set, int *rc, char *err, size_t cap);
extern "C" void fxg_emu_bc_free(fxg_emu_bc_table *t);
extern "C" int fxg_emu_bc_split(const fxg_emu_bc_table *t, const uint8_t *text, uint64_t text_len, int lpr, const uint32_t *ls, uint64_t cap_lines,
                                uint64_t n, uint16_t *rec_bin, uint8_t *out, uint64_t *bin_bytes, uint64_t *bin_records, char *err, size_t cap);

static std::mutex g_mu;
static std::map<fxg_ctx *, fxg_emu_bc_table *> g_tab;

extern "C" int fxg_barcode_prepare(fxg_ctx *c, const fxg_barcode_set *set)
{
    if (!c || !set) return FXG_E_INVALID;
    int rc = FXG_OK;
    fxg_emu_bc_table *t = fxg_emu_bc_prepare(set, &rc, c->err, sizeof c->err);
    std::lock_guard<std::mutex> g(g_mu);      // (as the engine: a refused table leaves the context without one)
    fxg_emu_bc_free(g_tab[c]);
    g_tab[c] = t;
    return rc;
}

extern "C" int fxg_barcode_split(fxg_ctx *c, const uint8_t *text, uint64_t text_len, int lpr, const uint32_t *line, uint64_t cap_lines, uint64_t n,
                                 uint16_t *rec_bin, uint8_t *out, uint64_t *bin_bytes, uint64_t *bin_records)
{
    if (!c) return FXG_E_INVALID;
    fxg_emu_bc_table *t;
    {
        std::lock_guard<std::mutex> g(g_mu);
        t = g_tab.count(c) ? g_tab[c] : nullptr;
    }
    return fxg_emu_bc_split(t, text, text_len, lpr, line, cap_lines, n, rec_bin, out, bin_bytes, bin_records, c->err, sizeof c->err);
}
