// fxg_engine_clip.hip -- the launch switches of the clip instances of fxg_kernel_tiles, one function per unit of fxg_clip_instances.h, generated from that
// unit's list.  -DFXG_CLIP_TU=k compiles unit k alone (the split build: fastx_toolkit_amd/build.py); without it (included by fxg_engine.hip in a
// single-unit build) all of them.  fxg_launch_clip (fxg_engine.hip) asks the units in turn.
#include "fxg_host.h"

// a packed instance: the DP over the staged tile, or over the batch (fxg_plan.h: clip_global)
#define FXG_CLIP_CASE_PACKED(N) case -N: return fxg_launch_tiles(c, (pl.ka.clip_global ? fxg_kernel_tiles<-N, 0, true> : fxg_kernel_tiles<-N, 0, false>), pl, ctr);
#define FXG_CLIP_CASE_GENERAL(N) case N: return fxg_launch_tiles(c, fxg_kernel_tiles<N, 0>, pl, ctr);
#define FXG_CLIP_DEFINE_UNIT(K) \
    int FXG_CLIP_UNIT_FN(K)(fxg_ctx *c, FxgPlan &pl, u64 *ctr) { switch (pl.amax) { FXG_CLIP_UNIT(K)(FXG_CLIP_CASE_PACKED, FXG_CLIP_CASE_GENERAL) default: return FXG_CLIP_NOT_MINE; } }

#ifdef FXG_CLIP_TU
FXG_CLIP_DEFINE_UNIT(FXG_CLIP_TU)
#else
FXG_CLIP_FOR_UNITS(FXG_CLIP_DEFINE_UNIT)
#endif
