// collapse_rows_stub.cpp -- TEST-ONLY: the four collapse entries of collapse_stub.cpp (included whole) plus fxg_collapse_add_rows for the
// emulation stub (fxg_stub.cpp), over collapse_rows_emu.cpp.  tests/test_collapse_rows_cpu.py links it with the stub's own objects into a
// libfxg.so of its own, so that host/fastx_clip_collapser runs on a machine without a GPU.
#include "collapse_stub.cpp"

extern "C" int fxg_emu_collapse_add_rows(void *h, const uint8_t *bases, const uint64_t *off, const uint16_t *len, uint64_t records, uint32_t first, uint32_t last, const uint32_t *kept_index,
                                         const uint8_t *text, const uint32_t *line, uint64_t cap_lines, int lpr, fxg_collapse_info *info, char *err, size_t cap);

extern "C" int fxg_collapse_add_rows(fxg_ctx *c, const uint8_t *bases, const uint64_t *off, const uint16_t *len, uint64_t records, uint32_t first, uint32_t last, const uint32_t *kept_index,
                                     const uint8_t *text, const uint32_t *line, uint64_t cap_lines, int lpr, fxg_collapse_info *info)
{
    return !c ? FXG_E_INVALID : fxg_emu_collapse_add_rows(set_of(c), bases, off, len, records, first, last, kept_index, text, line, cap_lines, lpr, info, c->err, sizeof c->err);
}
