// collapse_stub.cpp -- TEST-ONLY: fxg_collapse_begin / _add / _order / _write for the emulation stub (fxg_stub.cpp), over collapse_emu.cpp.
// tests/test_collapse_cpu.py links it with the stub's own objects into a libfxg.so of its own, so that host/fastx_collapser runs on a machine
// without a GPU.  The stub's context has no room for a set, so the sets are kept beside it, one per context address.
#include <map>

#include "fxg_stub_ctx.h"

extern "C" void *fxg_emu_collapse_new(void);
extern "C" int fxg_emu_collapse_begin(void *h, const fxg_collapse_opts *opts, char *err, size_t cap);
extern "C" int fxg_emu_collapse_add(void *h, const uint8_t *text, uint64_t text_len, int lpr, const uint32_t *line, uint64_t cap_lines, uint64_t records, const uint16_t *len,
                                    fxg_collapse_info *info, char *err, size_t cap);
extern "C" int fxg_emu_collapse_order(void *h, fxg_collapse_info *info, char *err, size_t cap);
extern "C" int fxg_emu_collapse_write(void *h, uint64_t rank_begin, uint64_t out_cap, uint8_t *out, fxg_collapse_window *window, char *err, size_t cap);

static void *set_of(fxg_ctx *c)
{
    static std::map<fxg_ctx *, void *> sets;
    void *&h = sets[c];
    if (!h) h = fxg_emu_collapse_new();
    return h;
}

extern "C" int fxg_collapse_begin(fxg_ctx *c, const fxg_collapse_opts *opts) { return !c ? FXG_E_INVALID : fxg_emu_collapse_begin(set_of(c), opts, c->err, sizeof c->err); }
extern "C" int fxg_collapse_add(fxg_ctx *c, const uint8_t *text, uint64_t text_len, int lpr, const uint32_t *line, uint64_t cap_lines, uint64_t records, const uint16_t *len,
                                fxg_collapse_info *info)
{
    return !c ? FXG_E_INVALID : fxg_emu_collapse_add(set_of(c), text, text_len, lpr, line, cap_lines, records, len, info, c->err, sizeof c->err);
}
extern "C" int fxg_collapse_order(fxg_ctx *c, fxg_collapse_info *info) { return !c ? FXG_E_INVALID : fxg_emu_collapse_order(set_of(c), info, c->err, sizeof c->err); }
extern "C" int fxg_collapse_write(fxg_ctx *c, uint64_t rank_begin, uint64_t out_cap, uint8_t *out, fxg_collapse_window *window)
{
    return !c ? FXG_E_INVALID : fxg_emu_collapse_write(set_of(c), rank_begin, out_cap, out, window, c->err, sizeof c->err);
}
