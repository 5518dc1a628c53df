// nucchange_stub.cpp -- TEST-ONLY: fxg_bases_change for the emulation stub (fxg_stub.cpp), over nucchange_emu.cpp.  tests/test_nucchange_cpu.py
// links it with the stub's own objects into a libfxg.so of its own, so that host/fasta_nucleotide_changer takes its device path on a machine without a GPU.
#include "fxg_stub_ctx.h"

extern "C" int fxg_emu_bases_change(uint8_t *text, uint64_t text_len, int lpr, const uint32_t *line, uint64_t cap_lines, uint64_t records, int from, int to,
                                    fxg_bases_change_info *info, char *err, size_t cap);

extern "C" int fxg_bases_change(fxg_ctx *c, uint8_t *text, uint64_t text_len, int lpr, const uint32_t *line, uint64_t cap_lines, uint64_t records, int from, int to,
                                fxg_bases_change_info *info)
{
    if (!c) return FXG_E_INVALID;
    return fxg_emu_bases_change(text, text_len, lpr, line, cap_lines, records, from, to, info, c->err, sizeof c->err);
}
