// uncollapse_stub.cpp -- TEST-ONLY: fxg_fasta_uncollapse for the emulation stub (fxg_stub.cpp), over uncollapse_emu.cpp.  tests/test_uncollapse_cpu.py
// links it with the stub's own objects into a libfxg.so of its own, so that host/fastx_uncollapser takes its device path on a machine without a GPU.
#include "fxg_stub_ctx.h"

extern "C" int fxg_emu_fasta_uncollapse(const uint8_t *text, uint64_t text_len, const uint32_t *line, uint64_t cap_lines, uint64_t records, const uint16_t *len,
                                        const fxg_uncollapse_opts *opts, uint8_t *out, fxg_uncollapse_info *info, char *err, size_t cap);

extern "C" int fxg_fasta_uncollapse(fxg_ctx *c, const uint8_t *text, uint64_t text_len, const uint32_t *line, uint64_t cap_lines, uint64_t records, const uint16_t *len,
                                    const fxg_uncollapse_opts *opts, uint8_t *out, fxg_uncollapse_info *info)
{
    if (!c) return FXG_E_INVALID;
    return fxg_emu_fasta_uncollapse(text, text_len, line, cap_lines, records, len, opts, out, info, c->err, sizeof c->err);
}
