// fxg_clip_instances.h -- THE list of the clipper's kernel instances.  The plan (fxg_plan.h), the DP's column bound (fxg_kernels.h: fxg_clip_k_amin), the
// engine's launch switches (fxg_engine_clip.hip), the CPU tier's emulator (tests/emu) and the number of translation units the builds compile side by side
// are all expanded from the lists below: a bucket is added, removed or moved between units HERE and nowhere else.  (The test tier keeps one independent
// statement of the bucket set, tests/helpers.py CLIP_BUCKETS, and tests/test_clip_instances.py holds the two against each other.)
//
// A packed instance P(B) is fxg_kernel_tiles<-B, 0>: adapters padded to B columns, one u32 summary per cell.  Every padded column costs a full cell, so the
// buckets are fine-grained:
//   4, 8, 9 .. 16    two passes in registers (fxg_clip_two_pass), reads of any length;
//   20 .. 100        the in-place row with ONE start field (fxg_clip_row_k), one pass or two with checkpoints in global scratch (fxg_plan.h decides);
//   36               the 33/34-base TruSeq adapters;
//   56, 80           (round 5) 49..56 columns no longer pay for 64 (17.4 -> 27.7 ms between 48 and 49 bases, profiles/r04/p_clip_waves_by_adapter_len.txt)
//                    and 65..80 no longer for 100;
//   44, 52, 60, 72, 88   (round 6) a bucket every 4 columns to 64 and every 8 to 88, so that no adapter pays for more than 8 % .. 12 % of padding columns.
// A general instance G(N) is fxg_kernel_tiles<N, 0>: the two-word form for adapters of up to N bases (FXG_NO_PACKED_CLIP, the one-pass corner cases of
// fxg_plan.h, adapters of more than six distinct bytes and more than 16 columns).
//
// The units are the engine's translation units: fxg_engine_clip.hip is compiled once per unit (-DFXG_CLIP_TU=k) beside fxg_engine.hip, because the clip
// instances are most of what hipcc spends its time on -- as one unit of 100 kernels the build took three and a half minutes.  The memberships were chosen
// for build time (the instances of three and two waves per SIMD, beyond 36 columns, are the longest compiles), not for meaning: 1 holds the register forms
// and the general forms, 2 / 4 / 6 the older buckets of the one-start-field form, 3 / 5 / 7 the buckets of round 6.  The emulator's groups are the same units.
#pragma once
#include <hip/hip_runtime.h>

#define FXG_CLIP_UNIT1(P, G) P(4) P(8) P(9) P(10) P(11) P(12) P(13) P(14) P(15) P(16) G(16) G(32) G(64) G(100)
#define FXG_CLIP_UNIT2(P, G) P(20) P(24) P(28) P(32) P(36)
#define FXG_CLIP_UNIT3(P, G) P(44) P(52)
#define FXG_CLIP_UNIT4(P, G) P(40) P(48) P(56)
#define FXG_CLIP_UNIT5(P, G) P(60) P(72)
#define FXG_CLIP_UNIT6(P, G) P(64) P(80) P(100)
#define FXG_CLIP_UNIT7(P, G) P(88)
#define FXG_CLIP_FOR_UNITS(U) U(1) U(2) U(3) U(4) U(5) U(6) U(7)      // a unit number without a list above (or the other way round) does not compile / link

#define FXG_CLIP_UNIT_(K) FXG_CLIP_UNIT##K
#define FXG_CLIP_UNIT(K) FXG_CLIP_UNIT_(K)                              // (K may be a macro itself: -DFXG_CLIP_TU)
#define FXG_CLIP_NONE(N)
#define FXG_CLIP_ITEM(N) N,
#define FXG_CLIP_ONE(K) +1
#define FXG_CLIP_UNIT_PACKED(K) FXG_CLIP_UNIT(K)(FXG_CLIP_ITEM, FXG_CLIP_NONE)      // the packed buckets of unit K, each followed by a comma

constexpr int FXG_CLIP_UNITS = 0 FXG_CLIP_FOR_UNITS(FXG_CLIP_ONE);
constexpr int fxg_clip_buckets[] = {FXG_CLIP_FOR_UNITS(FXG_CLIP_UNIT_PACKED)};      // every packed bucket, in the order of the units (no order is relied on)
constexpr int FXG_CLIP_NBUCKETS = (int)(sizeof fxg_clip_buckets / sizeof fxg_clip_buckets[0]);

// the bucket of an adapter of `alen` bases: the smallest one that holds it (0: none does)
__host__ __device__ constexpr int fxg_clip_bucket(int alen)
{
    int b = 0;
    for (int i = 0; i < FXG_CLIP_NBUCKETS; ++i) if (fxg_clip_buckets[i] >= alen && (b == 0 || fxg_clip_buckets[i] < b)) b = fxg_clip_buckets[i];
    return b;
}
// the largest bucket below `amax` (0: there is none): adapters of up to that many bases run a smaller instance
__host__ __device__ constexpr int fxg_clip_bucket_below(int amax)
{
    int p = 0;
    for (int i = 0; i < FXG_CLIP_NBUCKETS; ++i) if (fxg_clip_buckets[i] < amax && fxg_clip_buckets[i] > p) p = fxg_clip_buckets[i];
    return p;
}
