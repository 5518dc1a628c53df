// reflow_stub.cpp -- TEST-ONLY: fxg_fasta_reflow for the emulation stub (fxg_stub.cpp), over reflow_emu.cpp.  tests/test_reflow_cpu.py links
// it with the stub's own objects into a libfxg.so of its own, so that host/fasta_formatter takes its device path on a machine without a GPU.
#include "fxg_stub_ctx.h"

extern "C" int fxg_emu_fasta_reflow(const uint8_t *text, uint64_t text_len, int at_eof, uint64_t open_in, const fxg_reflow_opts *opts, uint32_t *line,
                                    uint64_t cap_lines, uint8_t *out, fxg_reflow_info *info, char *err, size_t cap);

extern "C" int fxg_fasta_reflow(fxg_ctx *c, const uint8_t *text, uint64_t text_len, int at_eof, uint64_t open_in, const fxg_reflow_opts *opts, uint32_t *line,
                                uint64_t cap_lines, uint8_t *out, fxg_reflow_info *info)
{
    if (!c) return FXG_E_INVALID;
    return fxg_emu_fasta_reflow(text, text_len, at_eof, open_in, opts, line, cap_lines, out, info, c->err, sizeof c->err);
}
