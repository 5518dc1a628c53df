// fxg_instances.h -- THE list of the kernel instances fxg_run_pipeline launches besides the clipper's (those: fxg_clip_instances.h).  The plan
// (fxg_plan.h) names one of them, or FXG_INST_CLIP with FxgPlan.amax; the engine's launch switch (fxg_engine.hip: fxg_launch_plan), the CPU tier's emulator
// (tests/emu: its dispatch) and the name fxg_last_launch_info reports are expanded from the rows below, and nothing else turns a plan into an instance.
// (The test tier states the names on its own, tests/test_plan_cpu.py, and holds the two against each other.)
//
// A row: id, kernel, name, rows kernel (one wave per workgroup, several scanner waves: fxg_launch_tiles), and what the emulator runs in its place:
// AMAX, REV and MODE of fxg_kernel_tiles' decision, the dwords NW of a lane's piece of a quality row and the lanes H per read of fxg_kernel_rows, the
// reads R per lane of fxg_kernel_rows_multi (NW = 0: no rows kernel; a tile of a rows kernel is FXG_ROWS_T * R / H reads).
#pragma once
#include "fxg_clip_instances.h"
#include "fxg_kernels.h"
#include "fxg_rows.h"

// (The order of the rows is the order in which the kernels stand in the engine's code object -- the launch switch instantiates them; nothing relies on it.)
#define FXG_INSTANCES(X) \
    X(ROWS26X2, (fxg_kernel_rows<26, 2>),       "fxg_kernel_rows<26,2> qtrim+qfilter",        true,  0, false, 0, 26, 2, 1)      /* rows of 153..208 bytes: two lanes per read */ \
    X(ROWS38X2, (fxg_kernel_rows<38, 2>),       "fxg_kernel_rows<38,2> qtrim+qfilter",        true,  0, false, 0, 38, 2, 1)      /* 209..304 (FXG_ROWS=2) */ \
    X(MULTI4,   (fxg_kernel_rows_multi<10, 4>), "fxg_kernel_rows_multi<10,4> qtrim+qfilter",  true,  0, false, 0, 10, 1, 4)      /* 28..40: four reads per lane */ \
    X(MULTI3,   (fxg_kernel_rows_multi<14, 3>), "fxg_kernel_rows_multi<14,3> qtrim+qfilter",  true,  0, false, 0, 14, 1, 3)      /* 41..56: three */ \
    X(MULTI2,   (fxg_kernel_rows_multi<20, 2>), "fxg_kernel_rows_multi<20,2> qtrim+qfilter",  true,  0, false, 0, 20, 1, 2)      /* 57..79: two */ \
    X(ROWS26,   (fxg_kernel_rows<26>),          "fxg_kernel_rows<26> qtrim+qfilter",          true,  0, false, 0, 26, 1, 1)      /* 80..104: one lane per read */ \
    X(ROWS38,   (fxg_kernel_rows<38>),          "fxg_kernel_rows<38> qtrim+qfilter",          true,  0, false, 0, 38, 1, 1)      /* 105..152 */ \
    X(TILES00,  (fxg_kernel_tiles<0, 0>),       "fxg_kernel_tiles<0,0> qtrim+qfilter",        false, 0, false, 0, 0,  1, 1) \
    X(TILES03,  (fxg_kernel_tiles<0, 3>),       "fxg_kernel_tiles<0,3> mask",                 false, 0, false, 3, 0,  1, 1) \
    X(TILES04,  (fxg_kernel_tiles<0, 4>),       "fxg_kernel_tiles<0,4> base census",          false, 0, false, 4, 0,  1, 1) \
    X(TILES05,  (fxg_kernel_tiles<0, 5>),       "fxg_kernel_tiles<0,5> revcomp[+ftrim], dword-aligned windows", false, 0, true, 5, 0, 1, 1) \
    X(TILES02,  (fxg_kernel_tiles<0, 2>),       "fxg_kernel_tiles<0,2> revcomp[+ftrim]",      false, 0, true,  2, 0,  1, 1) \
    X(TILES01,  (fxg_kernel_tiles<0, 1>),       "fxg_kernel_tiles<0,1> ftrim",                false, 0, false, 1, 0,  1, 1)

#define FXG_INST_ID(ID, KERNEL, NAME, ROWS, AMAX, REV, MODE, NW, H, R) FXG_INST_##ID,
enum FxgInst { FXG_INSTANCES(FXG_INST_ID) FXG_INST_CLIP };       // FXG_INST_CLIP: the clip instance of FxgPlan.amax (fxg_clip_instances.h)

// Threads per workgroup of fxg_kernel_tiles<amax, mode>: the plan's statement of FxgTileBlock (fxg_kernels.h), which host-only builds do not see; every build
// that has the kernels holds the two against each other, instance by instance, below.  The rows kernels run one wave (FXG_ROWS_T lanes).
constexpr u32 fxg_tile_block(int amax, int mode) { return mode == 0 && amax < 0 && amax >= -16 ? (u32)FXG_CLIP_TBLOCK : (u32)FXG_TBLOCK; }

// what the plan needs of an instance: its name, threads per workgroup and the rows kernels' shape
struct FxgInstInfo { const char *name; u32 block, nw, h, r; };
#define FXG_INST_INFO(ID, KERNEL, NAME, ROWS, AMAX, REV, MODE, NW, H, R) {NAME, ROWS ? FXG_ROWS_T : fxg_tile_block(AMAX, MODE), NW, H, R},
constexpr FxgInstInfo fxg_inst_info[] = {FXG_INSTANCES(FXG_INST_INFO) {nullptr, 0u, 0u, 1u, 1u}};      // (the last one: FXG_INST_CLIP, whose name and block follow from amax)

// the names of the clip instances (negative amax: the packed instance of that bucket, positive: the general one)
#define FXG_CLIP_NAME_PACKED(N) "fxg_kernel_tiles<-" #N ",0> clip(packed)[+qtrim+qfilter]"
#define FXG_CLIP_NAME_GENERAL(N) "fxg_kernel_tiles<" #N ",0> clip[+qtrim+qfilter]"

#ifndef FXG_HOST_EMULATION
#define FXG_INST_BLOCK_IS(ID, KERNEL, NAME, ROWS, AMAX, REV, MODE, NW, H, R) static_assert(ROWS || fxg_tile_block(AMAX, MODE) == (u32)FxgTileBlock<AMAX, MODE>::threads, "fxg_tile_block is not " NAME "'s block size");
#define FXG_CLIP_BLOCK_IS_PACKED(N) static_assert(fxg_tile_block(-N, 0) == (u32)FxgTileBlock<-N, 0>::threads, "fxg_tile_block is not the packed clip instance's block size");
#define FXG_CLIP_BLOCK_IS_GENERAL(N) static_assert(fxg_tile_block(N, 0) == (u32)FxgTileBlock<N, 0>::threads, "fxg_tile_block is not the general clip instance's block size");
#define FXG_CLIP_BLOCK_IS_UNIT(K) FXG_CLIP_UNIT(K)(FXG_CLIP_BLOCK_IS_PACKED, FXG_CLIP_BLOCK_IS_GENERAL)
FXG_INSTANCES(FXG_INST_BLOCK_IS)
FXG_CLIP_FOR_UNITS(FXG_CLIP_BLOCK_IS_UNIT)
#endif

// the name fxg_last_launch_info reports for instance `inst` (FXG_INST_CLIP: of `amax`); null: there is no such instance
static inline const char *fxg_inst_name(int inst, int amax)
{
    if (inst != FXG_INST_CLIP) return inst >= 0 && inst < FXG_INST_CLIP ? fxg_inst_info[inst].name : nullptr;
    switch (amax) {
#define FXG_CLIP_NAME_CASE_PACKED(N) case -N: return FXG_CLIP_NAME_PACKED(N);
#define FXG_CLIP_NAME_CASE_GENERAL(N) case N: return FXG_CLIP_NAME_GENERAL(N);
#define FXG_CLIP_NAME_UNIT(K) FXG_CLIP_UNIT(K)(FXG_CLIP_NAME_CASE_PACKED, FXG_CLIP_NAME_CASE_GENERAL)
    FXG_CLIP_FOR_UNITS(FXG_CLIP_NAME_UNIT)
    default: return nullptr;
    }
}
