// reflow_emu.cpp -- TEST-ONLY serial CPU emulation of fxg_fasta_reflow (csrc/fxg_reflow.h): the per-item and per-lane bodies the kernels
// run, driven item by item and lane by lane, with the engine's own checks.  The segmented scan keeps the kernels' structure (blocks of
// FXG_RF_SCAN_BLOCK items, their aggregates scanned the same way, the carries added), the plain scans are serial.  tests/test_reflow_cpu.py
// calls it through ctypes (with every array against a guard page), reflow_stub.cpp puts it behind the C-ABI for the tool, and
// reflow_san_main.cpp runs it under the sanitizers.  Not part of the product library.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fastx_toolkit_amd/csrc/fxg_reflow.h"

static void emu_segscan(u64 *s, u64 *kf, u64 n)
{
    const u64 nb = (n + FXG_RF_SCAN_BLOCK - 1) / FXG_RF_SCAN_BLOCK;
    std::vector<u64> as(nb), akf(nb);
    for (u64 b = 0; b < nb; ++b) {                                        // fxg_kernel_rf_segscan_blocks
        FxgRfSeg run = {0ull, 0ull};
        for (u64 i = b * FXG_RF_SCAN_BLOCK; i < n && i < (b + 1) * FXG_RF_SCAN_BLOCK; ++i) {
            const FxgRfSeg v = {s[i], kf[i]};
            s[i] = run.s; kf[i] = run.kf;
            run = fxg_rf_combine(run, v);
        }
        as[b] = run.s; akf[b] = run.kf;
    }
    if (nb <= 1) return;
    emu_segscan(as.data(), akf.data(), nb);
    for (u64 i = 0; i < n; ++i) {                                         // fxg_kernel_rf_segscan_add
        const FxgRfSeg carry = {as[i / FXG_RF_SCAN_BLOCK], akf[i / FXG_RF_SCAN_BLOCK]}, mine = {s[i], kf[i]};
        const FxgRfSeg r = fxg_rf_combine(carry, mine);
        s[i] = r.s; kf[i] = r.kf;
    }
}

static void emu_scan(u64 *d, u64 n) { u64 run = 0; for (u64 i = 0; i < n; ++i) { const u64 v = d[i]; d[i] = run; run += v; } }

extern "C" int fxg_emu_fasta_reflow(const uint8_t *text, uint64_t text_len, int at_eof, uint64_t open_in, const fxg_reflow_opts *opts, uint32_t *line,
                                    uint64_t cap_lines, uint8_t *out, fxg_reflow_info *info, char *err, size_t cap)
{
    char own[256];
    if (!err) { err = own; cap = sizeof own; }
    int rc = fxg_rf_check(text, text_len, opts, line, cap_lines, info, err, cap);
    if (rc != FXG_OK) return rc;
    u64 L = 0;
    if (text_len) {
        for (u64 p = 0; p < text_len; ++p) L += text[p] == '\n';
        if ((rc = fxg_rf_lines_fit(L, cap_lines, err, cap)) != FXG_OK) return rc;
        u64 j = 0;
        line[0] = 0u;
        for (u64 p = 0; p < text_len; ++p) if (text[p] == '\n') line[++j] = (u32)(p + 1);
    }
    std::vector<u64> ws(fxg_rf_ws_words(L), 0);
    const FxgRfArgs a = fxg_rf_args(text, line, L, at_eof, open_in, opts, ws.data(), out);
    const u64 M = L + 2;
    for (u64 i = 0; i < M; ++i) a.res[FXG_RF_RES_HEADERS] += fxg_rf_classify(a, i);
    emu_segscan(a.seg_s, a.seg_kf, M);
    for (u64 i = 0; i < M; ++i) {
        u64 sz = 0, pc = 0;
        u32 bad = 0;
        if (i <= L) fxg_rf_size(a, i, &sz, &pc, &bad);
        a.size[i] = sz; a.pieces[i] = pc;
        a.res[FXG_RF_RES_BAD] |= bad;
    }
    emu_scan(a.size, M);
    emu_scan(a.pieces, M);
    fxg_rf_finish(a);
    if ((rc = fxg_rf_results(a.res, L, opts->out_cap, out != nullptr, info, err, cap)) != FXG_OK) return rc;
    if (!a.res[FXG_RF_RES_OUT_BYTES]) return FXG_OK;
    for (u64 i = 0; i <= L; ++i)
        for (u32 l = 0; l < 16u; ++l) fxg_rf_copy_head(a, i, l);
    for (u64 p = 0; p < a.res[FXG_RF_RES_PIECES]; ++p)
        for (u32 l = 0; l < 16u; ++l) fxg_rf_copy_tail(a, p, l);
    return FXG_OK;
}
