// fxg_engine_clip.hip -- the clip instances of fxg_kernel_tiles, in seven groups so that they can be compiled side by side (fxg_host.h).
// -DFXG_CLIP_TU=1 .. 7 compiles one group; without it (included by fxg_engine.hip in a single-unit build) all of them.  A launch that no
// group's switch takes goes on to the next group's, in the order 1, 2, 4, 6, 3, 5, 7.
#include "fxg_host.h"

#define FXG_TILES_A(N) (fxg_kernel_tiles<N, 0>)
#define FXG_TILES_C(N) (pl.ka.clip_global ? fxg_kernel_tiles<N, 0, true> : fxg_kernel_tiles<N, 0, false>)      // packed clip instances: the DP over the staged tile, or over the batch (fxg_plan.h)

#if !defined(FXG_CLIP_TU) || FXG_CLIP_TU == 1
// adapters of up to 16 bases: two passes in registers; and the general two-word form (positive codes: FXG_NO_PACKED_CLIP, one-pass corner cases)
int fxg_launch_clip_reg(fxg_ctx *c, FxgPlan &pl, u64 *ctr)
{
    switch (pl.amax) {
        case -4: return fxg_launch_tiles(c, FXG_TILES_C(-4), "fxg_kernel_tiles<-4,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, pl.block);
        case -8: return fxg_launch_tiles(c, FXG_TILES_C(-8), "fxg_kernel_tiles<-8,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, pl.block);
        case -9: return fxg_launch_tiles(c, FXG_TILES_C(-9), "fxg_kernel_tiles<-9,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, pl.block);
        case -10: return fxg_launch_tiles(c, FXG_TILES_C(-10), "fxg_kernel_tiles<-10,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, pl.block);
        case -11: return fxg_launch_tiles(c, FXG_TILES_C(-11), "fxg_kernel_tiles<-11,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, pl.block);
        case -12: return fxg_launch_tiles(c, FXG_TILES_C(-12), "fxg_kernel_tiles<-12,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, pl.block);
        case -13: return fxg_launch_tiles(c, FXG_TILES_C(-13), "fxg_kernel_tiles<-13,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, pl.block);
        case -14: return fxg_launch_tiles(c, FXG_TILES_C(-14), "fxg_kernel_tiles<-14,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, pl.block);
        case -15: return fxg_launch_tiles(c, FXG_TILES_C(-15), "fxg_kernel_tiles<-15,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, pl.block);
        case -16: return fxg_launch_tiles(c, FXG_TILES_C(-16), "fxg_kernel_tiles<-16,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, pl.block);
        case 16: return fxg_launch_tiles(c, FXG_TILES_A(16), "fxg_kernel_tiles<16,0> clip[+qtrim+qfilter]", pl.ka, pl.lds, ctr);
        case 32: return fxg_launch_tiles(c, FXG_TILES_A(32), "fxg_kernel_tiles<32,0> clip[+qtrim+qfilter]", pl.ka, pl.lds, ctr);
        case 64: return fxg_launch_tiles(c, FXG_TILES_A(64), "fxg_kernel_tiles<64,0> clip[+qtrim+qfilter]", pl.ka, pl.lds, ctr);
        default: return fxg_launch_tiles(c, FXG_TILES_A(100), "fxg_kernel_tiles<100,0> clip[+qtrim+qfilter]", pl.ka, pl.lds, ctr);
    }
}
#endif

#if !defined(FXG_CLIP_TU) || FXG_CLIP_TU == 2
// 17..100 columns: the in-place row with one start field, checkpoints in global scratch (fxg_clip_two_pass_k)
int fxg_launch_clip_k(fxg_ctx *c, FxgPlan &pl, u64 *ctr)
{
    switch (pl.amax) {
        case -20: return fxg_launch_tiles(c, FXG_TILES_C(-20), "fxg_kernel_tiles<-20,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg);
        case -24: return fxg_launch_tiles(c, FXG_TILES_C(-24), "fxg_kernel_tiles<-24,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg);
        case -28: return fxg_launch_tiles(c, FXG_TILES_C(-28), "fxg_kernel_tiles<-28,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg);
        case -32: return fxg_launch_tiles(c, FXG_TILES_C(-32), "fxg_kernel_tiles<-32,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg);
        case -36: return fxg_launch_tiles(c, FXG_TILES_C(-36), "fxg_kernel_tiles<-36,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg);
    default: return fxg_launch_clip_k_wide(c, pl, ctr);
    }
}
#endif

#if !defined(FXG_CLIP_TU) || FXG_CLIP_TU == 4
// ... its instances of more than 36 columns (three and two waves per SIMD: the longest compiles)
int fxg_launch_clip_k_wide(fxg_ctx *c, FxgPlan &pl, u64 *ctr)
{
    switch (pl.amax) {
        case -40: return fxg_launch_tiles(c, FXG_TILES_C(-40), "fxg_kernel_tiles<-40,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg);
        case -48: return fxg_launch_tiles(c, FXG_TILES_C(-48), "fxg_kernel_tiles<-48,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg);
        case -56: return fxg_launch_tiles(c, FXG_TILES_C(-56), "fxg_kernel_tiles<-56,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg);
    default: return fxg_launch_clip_k_wide_wide(c, pl, ctr);
    }
}
#endif

#if !defined(FXG_CLIP_TU) || FXG_CLIP_TU == 6
// ... 64, 80 and 100 columns
int fxg_launch_clip_k_wide_wide(fxg_ctx *c, FxgPlan &pl, u64 *ctr)
{
    switch (pl.amax) {
        case -64: return fxg_launch_tiles(c, FXG_TILES_C(-64), "fxg_kernel_tiles<-64,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg);
        case -80: return fxg_launch_tiles(c, FXG_TILES_C(-80), "fxg_kernel_tiles<-80,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg);
        case -100: return fxg_launch_tiles(c, FXG_TILES_C(-100), "fxg_kernel_tiles<-100,0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg);
    default: return fxg_launch_clip_k44_52(c, pl, ctr);      // (the buckets of round 6: below)
    }
}
#endif

// 44 / 52, 60 / 72 and 88 columns (the buckets of round 6), one translation unit each
#define FXG_K(N) case -N: return fxg_launch_tiles(c, FXG_TILES_C(-N), "fxg_kernel_tiles<-" #N ",0> clip(packed)[+qtrim+qfilter]", pl.ka, pl.lds, ctr, FXG_TBLOCK, false, pl.ck_per_wg)
#if !defined(FXG_CLIP_TU) || FXG_CLIP_TU == 3
int fxg_launch_clip_k44_52(fxg_ctx *c, FxgPlan &pl, u64 *ctr) { switch (pl.amax) { FXG_K(44); FXG_K(52); default: return fxg_launch_clip_k60_72(c, pl, ctr); } }
#endif
#if !defined(FXG_CLIP_TU) || FXG_CLIP_TU == 5
int fxg_launch_clip_k60_72(fxg_ctx *c, FxgPlan &pl, u64 *ctr) { switch (pl.amax) { FXG_K(60); FXG_K(72); default: return fxg_launch_clip_k88(c, pl, ctr); } }
#endif
#if !defined(FXG_CLIP_TU) || FXG_CLIP_TU == 7
int fxg_launch_clip_k88(fxg_ctx *c, FxgPlan &pl, u64 *ctr) { switch (pl.amax) { FXG_K(88); default: return fxg_fail(c, FXG_E_INVALID, "no clip instance %d", pl.amax); } }
#endif
#undef FXG_K
#undef FXG_TILES_A
#undef FXG_TILES_C
