// nucchange_emu.cpp -- TEST-ONLY serial CPU emulation of fxg_bases_change (csrc/fxg_nucchange.h): the per-lane body the kernel runs, driven record
// by record and lane by lane, with the engine's own checks; the wave's reductions are plain sums and minima here.  tests/test_nucchange_cpu.py
// calls it through ctypes (with the text between guard pages), nucchange_stub.cpp puts it behind the C-ABI for the tool, and
// nucchange_san_main.cpp runs it under the sanitizers.  Not part of the product library.
#include <cstdlib>
#include <cstring>

#include "../../fastx_toolkit_amd/csrc/fxg_nucchange.h"

extern "C" int fxg_emu_bases_change(uint8_t *text, uint64_t text_len, int lpr, const uint32_t *line, uint64_t cap_lines, uint64_t records, int from, int to,
                                    fxg_bases_change_info *info, char *err, size_t cap)
{
    char own[256];
    if (!err) { err = own; cap = sizeof own; }
    const int rc = fxg_nc_check(text, text_len, lpr, line, cap_lines, records, from, to, info, err, cap);
    if (rc != FXG_OK || records == 0) return rc;
    u64 res[FXG_NC_RES_WORDS];
    fxg_nc_res_init(res);
    const FxgNcArgs a = fxg_nc_args(text, lpr, line, cap_lines, records, from, to, res);
    const u64 grid = fxg_nc_grid(records), groups = grid * (FXG_BLOCK / FXG_NC_LANES);      // the launch's workgroups and groups of lanes: each takes its trips
    for (u64 g = 0; g < groups; ++g)
        for (u32 l = 0; l < FXG_NC_LANES; ++l) {
            u32 flags = 0;
            u64 first = FXG_NC_NONE;
            res[fxg_nc_slot(g / (FXG_BLOCK / FXG_NC_LANES))] += fxg_nc_lane(a, g, groups, l, &flags, &first);
            if (first < res[FXG_NC_RES_FIRST_TO]) res[FXG_NC_RES_FIRST_TO] = first;
            if (flags & FXG_NC_BAD) res[FXG_NC_RES_IRREGULAR] |= 1ull;
        }
    fxg_nc_results(res, info);
    return FXG_OK;
}
