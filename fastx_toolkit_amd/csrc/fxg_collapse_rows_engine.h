// fxg_collapse_rows_engine.h -- the engine's side of fxg_collapse_add_rows (fxg_collapse.h: fxg_cl_add_rows and its three kernels): the
// collapser's backend with the launches of the rows entry, and the entry itself.  Included by fxg_engine.hip behind the four entries of the set,
// whose backend (FxgClEngine) and state lookup (fxg_cl_state) it uses.
#pragma once

struct FxgClRowsEngine : FxgClEngine {
    FxgClRowsEngine(fxg_ctx *ctx) : FxgClEngine{ctx, ctx->err, sizeof ctx->err} {}
    int row_lens(const uint16_t *rlen, u64 n, u32 first, u32 last, u64 *bytes, u64 *num)
    {
        FXG_LAUNCH(c, fxg_kernel_cl_row_lens, (u32)((n + FXG_BLOCK) / FXG_BLOCK), FXG_BLOCK, 0, rlen, n, first, last, bytes, num);
        return FXG_OK;
    }
    int copy_rows(const FxgClRowsArgs &a) { FXG_LAUNCH(c, fxg_kernel_cl_copy_rows, (u32)fxg_cl_grid(a.n * FXG_CL_LANES, FXG_CL_GRID_MAX), FXG_BLOCK, 0, a); return FXG_OK; }
    int row_counts(const FxgClRowsArgs &a) { FXG_LAUNCH(c, fxg_kernel_cl_row_counts, (u32)fxg_cl_grid(a.n, FXG_CL_GRID_MAX), FXG_BLOCK, 0, a); return FXG_OK; }
};

// (C linkage from its declaration in include/fxg.h, as the four entries before it)
int fxg_collapse_add_rows(fxg_ctx *c, const uint8_t *d_bases, const uint64_t *d_off, const uint16_t *d_len, uint64_t records, uint32_t first_base, uint32_t last_base,
                          const uint32_t *d_kept_index, const uint8_t *d_text, const uint32_t *d_line, uint64_t cap_lines, int lines_per_record, fxg_collapse_info *info)
{
    if (!c) return FXG_E_INVALID;
    FxgClState none;
    FxgClRowsEngine b(c);
    FXG_HIP(c, hipSetDevice(c->device));
    return fxg_cl_add_rows(b, *fxg_cl_state(c, &none), d_bases, (const u64 *)d_off, d_len, records, first_base, last_base, d_kept_index, d_text, d_line, cap_lines, lines_per_record, info);
}
