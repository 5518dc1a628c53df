// bcsplit_emu.cpp -- TEST-ONLY serial CPU emulation of the barcode splitter's three launches (csrc/fxg_barcode.h): the per-record and
// per-lane bodies the kernels run, driven tile by tile and lane by lane.  tests/test_barcode_cpu.py calls it through ctypes (with every
// array against a guard page) and bcsplit_stub.cpp puts it behind the C-ABI for the tool.  Not part of the product library.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fastx_toolkit_amd/csrc/fxg_barcode.h"

struct fxg_emu_bc_table { std::vector<FxgBcEntry> tab; u32 BL, mismatches, eol, bins; };

extern "C" {
// the engine's own checks and encoding of fxg_barcode_prepare; null on a refused table, with the engine's code in *rc (may be null) and its message in err
fxg_emu_bc_table *fxg_emu_bc_prepare(const fxg_barcode_set *set, int *rc, char *err, size_t cap)
{
    fxg_emu_bc_table *t = new fxg_emu_bc_table;
    int r = set ? fxg_bc_set_check(set, err, cap) : FXG_E_INVALID;
    if (r == FXG_OK) { t->tab.resize(set->entries); r = fxg_bc_set_encode(set, t->tab.data(), err, cap); }
    if (rc) *rc = r;
    if (r != FXG_OK) { delete t; return nullptr; }
    t->BL = set->barcode_len; t->mismatches = set->mismatches; t->eol = set->eol ? 1u : 0u; t->bins = set->bins;
    return t;
}

void fxg_emu_bc_free(fxg_emu_bc_table *t) { delete t; }

// fxg_barcode_split over host memory: classify (one record at a time: the tile histograms, the bins' totals), the exclusive scan over
// (bin, tile), the scatter (rank inside the tile, then the copy by 16 lanes, lane by lane)
int fxg_emu_bc_split(const fxg_emu_bc_table *t, const uint8_t *text, uint64_t text_len, int lpr, const uint32_t *ls, uint64_t cap_lines, uint64_t n,
                     uint16_t *rec_bin, uint8_t *out, uint64_t *bin_bytes, uint64_t *bin_records, char *err, size_t cap)
{
    const u32 bins = t ? t->bins : 0u;
    const int rc = fxg_bc_split_check(bins, text, text_len, lpr, ls, cap_lines, n, out, bin_bytes, bin_records, err, cap);
    if (rc != FXG_OK || n == 0) return rc;
    const u64 tiles = (n + FXG_BC_TILE - 1) / FXG_BC_TILE;
    std::vector<u64> hb(bins * tiles, 0);
    std::vector<uint16_t> own(rec_bin ? 0 : n);
    uint16_t *rb = rec_bin ? rec_bin : own.data();
    const FxgBcEntry *tab = t->tab.empty() ? nullptr : t->tab.data();
    for (u64 r = 0; r < n; ++r) {
        const u32 b = fxg_bc_record_bin(text, ls, (u32)lpr, r, tab, (u32)t->tab.size(), t->BL, t->mismatches, t->eol, bins - 1);
        const u64 size = ls[(u64)lpr * (r + 1)] - ls[(u64)lpr * r];
        rb[r] = (uint16_t)b;
        hb[(u64)b * tiles + r / FXG_BC_TILE] += size;
        bin_bytes[b] += size;
        bin_records[b] += 1;
    }
    u64 sb = 0;
    for (u64 i = 0; i < bins * tiles; ++i) { const u64 b = hb[i]; hb[i] = sb; sb += b; }
    u32 s_bin[FXG_BC_TILE], s_size[FXG_BC_TILE];
    for (u64 tile = 0; tile < tiles; ++tile) {
        const u64 r0 = tile * FXG_BC_TILE;
        const u32 live = (u32)(n - r0 < FXG_BC_TILE ? n - r0 : FXG_BC_TILE);
        for (u32 i = 0; i < FXG_BC_TILE; ++i) {
            s_bin[i] = i < live ? rb[r0 + i] : 0xFFFFFFFFu;
            s_size[i] = i < live ? ls[(u64)lpr * (r0 + i + 1)] - ls[(u64)lpr * (r0 + i)] : 0u;
        }
        for (u32 i = 0; i < live; ++i) {
            const u64 dst = hb[(u64)s_bin[i] * tiles + tile] + fxg_bc_rank_bytes(s_bin, s_size, i);
            for (u32 l = 0; l < 16; ++l) fxg_bc_copy(out + dst, text + ls[(u64)lpr * (r0 + i)], s_size[i], l, 16);
        }
    }
    return 0;
}
}
