// collapse_rows_emu.cpp -- TEST-ONLY serial CPU emulation of fxg_collapse_add_rows (csrc/fxg_collapse.h) on top of collapse_emu.cpp, which it
// includes whole: the same sets, the same backend, plus the launches of the rows entry run row by row and lane by lane over the caller's
// arrays.  A library built from this file has every fxg_emu_collapse_* export of collapse_emu.cpp and fxg_emu_collapse_add_rows.
// tests/test_collapse_rows_cpu.py calls it through ctypes (the caller's arrays against guard pages), collapse_rows_stub.cpp puts it behind the
// C-ABI for the tool, and collapse_rows_san_main.cpp runs it under the sanitizers.  Not part of the product library.
#include "collapse_emu.cpp"

struct EmuClRowsBackend : EmuClBackend {
    int row_lens(const uint16_t *rlen, u64 n, u32 first, u32 last, u64 *bytes, u64 *num)      // fxg_kernel_cl_row_lens
    {
        for (u64 r = 0; r <= n; ++r) fxg_cl_row_len(rlen, n, first, last, r, bytes, num);
        return FXG_OK;
    }
    int copy_rows(const FxgClRowsArgs &a)                        // fxg_kernel_cl_copy_rows
    {
        for (u64 r = 0; r < a.n; ++r) {
            bool bad = false;
            for (u32 l = 0; l < FXG_CL_LANES; ++l) bad |= fxg_cl_copy_row(a, r, l);
            if (bad) { fxg_cl_a_min(a.s.res + FXG_CL_RES_FIRST_BAD, r); a.s.res[FXG_CL_RES_IRREGULAR] |= 1ull; }
        }
        return FXG_OK;
    }
    int row_counts(const FxgClRowsArgs &a)                       // fxg_kernel_cl_row_counts
    {
        for (u64 r = 0; r < a.n; ++r) a.s.res[FXG_CL_RES_READS] += fxg_cl_row_count(a, r);
        return FXG_OK;
    }
};

extern "C" int fxg_emu_collapse_add_rows(void *h, const uint8_t *bases, const uint64_t *off, const uint16_t *len, uint64_t records, uint32_t first, uint32_t last,
                                         const uint32_t *kept_index, const uint8_t *text, const uint32_t *line, uint64_t cap_lines, int lpr, fxg_collapse_info *info, char *err, size_t cap)
{
    char own[256];
    EmuClRowsBackend b;
    b.err = err ? err : own; b.cap = err ? cap : sizeof own;
    return fxg_cl_add_rows(b, *(FxgClState *)h, bases, (const u64 *)off, len, records, first, last, kept_index, text, line, cap_lines, lpr, info);
}
