// fmtopts_stub.cpp -- TEST-ONLY: fxg_fastq_format_opts for the emulation stub (fxg_stub.cpp).  tests/test_format_opts_cpu.py links it with the
// stub's own objects into a libfxg.so of its own, so that the output modes of the device formatter (ids, quality encoding) and the tools built
// on them run on a machine without a GPU.  The host half -- what is refused, the arguments, the capacity check -- is the engine's own
// (csrc/fxg_text.h); the kernels' per-thread bodies run one lane after the other, the scan between them is a serial sum.
#include <cstring>
#include <vector>

#include "fxg_stub_ctx.h"
#include "../../fastx_toolkit_amd/csrc/fxg_kernels.h"
#include "../../fastx_toolkit_amd/csrc/fxg_text.h"

extern "C" int fxg_fastq_format_opts(fxg_ctx *c, const uint8_t *text, int lpr, const uint32_t *d_line, uint64_t cap_lines, const uint8_t *flags, uint64_t n, const uint32_t *res,
                                     uint32_t fwd_start, int reverse, const uint8_t *pk_bases, const uint8_t *pk_qual, const uint64_t *pk_off, const uint8_t *rows_qual, uint32_t stride,
                                     int qoffset, int out_fasta, uint8_t *out, uint64_t *out_bytes, const fxg_format_opts *opts)
{
    if (!c) return FXG_E_INVALID;
    int rc = fxg_text_format_opts_check(text, lpr, d_line, flags, n, res, fwd_start, pk_bases, pk_qual, pk_off, rows_qual, out_fasta, out, out_bytes, opts, c->err, sizeof c->err);
    if (rc == FXG_OK) rc = fxg_text_format_source_check(pk_bases, reverse, fwd_start, c->err, sizeof c->err);
    if (rc != FXG_OK || n == 0) return rc;
    std::vector<u64> item(n);
    FxgFormatArgs a = fxg_text_format_args(text, d_line, cap_lines, flags, item.data(), n, res, fwd_start, reverse, pk_bases, pk_qual, pk_off, rows_qual, stride, qoffset, out_fasta, out);
    fxg_text_format_args_opts(&a, opts);
    u64 run = 0;
    for (u64 r = 0; r < n; ++r) {                               // sizes, then the exclusive scan (offset in the low bits, rank above)
        const u64 v = lpr == 4 ? fxg_text_size_record<4>(a, r) : fxg_text_size_record<2>(a, r);
        item[r] = run;
        run += v;
    }
    u64 tot[2];
    if (lpr == 4) fxg_text_total<4>(a, tot); else fxg_text_total<2>(a, tot);
    if (opts->out_cap != FXG_OUT_CAP_UNCHECKED && (rc = fxg_text_format_fits(tot[0], opts->out_cap, c->err, sizeof c->err)) != FXG_OK) return rc;
    for (u64 r = 0; r < n; ++r)
        for (u32 l = 0; l < 16; ++l) { if (lpr == 4) fxg_text_format_record<4>(a, r, l); else fxg_text_format_record<2>(a, r, l); }
    *out_bytes = tot[0];
    return FXG_OK;
}

// the closed form under the ordinal ids, for the test that holds it against a plain loop
extern "C" uint64_t fxg_emu_dec_width_sum(uint64_t first, uint64_t count) { return fxg_dec_width_sum(first, count); }
// a numeric quality line by the 16 lanes of a group in lock step (fxg_text_write_numeric's host form), for the test that holds it against "%d" joined by blanks
extern "C" void fxg_emu_write_numeric(uint8_t *qd, const uint8_t *src, uint32_t len) { fxg_text_write_numeric_group(qd, src, len); }
