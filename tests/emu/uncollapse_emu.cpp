// uncollapse_emu.cpp -- TEST-ONLY serial CPU emulation of fxg_fasta_uncollapse (csrc/fxg_uncollapse.h): the per-record and per-lane bodies the
// kernels run, driven record by record, piece by piece and lane by lane, with the engine's own checks.  The scans are serial.  A context keeps
// the scans of a block from window to window; here every call makes them again, which gives the same arrays.  tests/test_uncollapse_cpu.py
// calls it through ctypes (with every array against a guard page), uncollapse_stub.cpp puts it behind the C-ABI for the tool, and
// uncollapse_san_main.cpp runs it under the sanitizers.  Not part of the product library.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fastx_toolkit_amd/csrc/fxg_uncollapse.h"

static void emu_uc_scan(u64 *d, u64 n) { u64 run = 0; for (u64 i = 0; i < n; ++i) { const u64 v = d[i]; d[i] = run; run += v; } }

extern "C" int fxg_emu_fasta_uncollapse(const uint8_t *text, uint64_t text_len, const uint32_t *line, uint64_t cap_lines, uint64_t records, const uint16_t *len,
                                        const fxg_uncollapse_opts *opts, uint8_t *out, fxg_uncollapse_info *info, char *err, size_t cap)
{
    char own[256];
    if (!err) { err = own; cap = sizeof own; }
    int rc = fxg_uc_check(text, text_len, line, cap_lines, records, len, opts, info, err, cap);
    if (rc != FXG_OK) return rc;
    const u64 n = records, M = n + 1;
    std::vector<u64> ws(fxg_uc_ws_words(n), 0);
    const FxgUcArgs a = fxg_uc_args(text, line, cap_lines, n, len, opts->ordinal_base, ws.data(), out);
    for (u64 r = 0; r < M; ++r) a.cnt[r] = fxg_uc_count(a, r);            // fxg_kernel_uc_counts
    emu_uc_scan(a.cnt, M);
    for (u64 r = 0; r < M; ++r) fxg_uc_size(a, r, &a.size[r], &a.pieces[r]);      // fxg_kernel_uc_sizes
    emu_uc_scan(a.size, M);
    emu_uc_scan(a.pieces, M);
    fxg_uc_window(a, opts->copy_begin, opts->out_cap);
    FxgUcWindow w;
    if ((rc = fxg_uc_results(a.res, opts, out != nullptr, info, &w, err, cap)) != FXG_OK) return rc;
    if (!info->out_bytes) return FXG_OK;
    for (u64 h = 0; h <= w.r_hi - w.r_lo; ++h)
        for (u32 l = 0; l < 16u; ++l) fxg_uc_copy_head(a, w, h, l);
    for (u64 p = w.p_lo; p < w.p_hi; ++p)
        for (u32 l = 0; l < 16u; ++l) fxg_uc_copy_tail(a, w, p, l);
    return FXG_OK;
}
