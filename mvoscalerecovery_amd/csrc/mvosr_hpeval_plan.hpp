// mvosr_hpeval_plan.hpp — the LDS layout of height_pitch_eval_kernel (mvosr_hpeval.hip).
//
// As mvosr_heightpitch_plan.hpp: named byte offsets into the workgroup's dynamic LDS plus `total`, one function shared by the
// kernel (at the frame's own n, tn and the launch's n_hyp) and the launcher (at the header's max_feat, max_tri).  Every offset
// grows with the sizes and is a multiple of 16; no region is reused.  The frame (x, y, z, list) is written once; the hypotheses'
// tile, its counts and the list mask are rewritten for every case and every tile, so the request does not grow with the number
// of cases, nor with n_hyp beyond one tile of kHpMaxHyp (tests/test_hpeval_cases.py checks all of that with a host compiler).
//
// Plain C++ (<stdint.h> / <stddef.h> only).
#pragma once

#include "mvosr_heightpitch_plan.hpp"

namespace mvosr {

constexpr int kHpeMaxHyp = 4096;        // hypotheses per (frame, case), at most: tiles of kHpMaxHyp
constexpr int kHpeMaxCases = 1024;      // cases per launch, at most

// misc[] slots of height_pitch_eval_kernel: HM_* of the frame pass, then the replay's carried state and the refinement's sample
enum { HE_DONE = 12, HE_DEGEN = 13, HE_N = HM_N };
// red[] (doubles): three reduction slots of 2 kHpWaves each, then the case's best model (raw, then sign-fixed)
enum { HER_SUM = 0, HER_YZ = 2 * kHpWaves, HER_DEV = 4 * kHpWaves, HER_MODEL = 6 * kHpWaves /* [4] */, HER_N = 6 * kHpWaves + 8 };

template <typename U> struct HpEvalPlan {
    U x, y, z;      // double[n] each: the back-projected points, alive over every case
    U list;         // uint16[3 tn]: the point list as vertex ids
    U mods;         // [min(n_hyp, kHpMaxHyp)] unit (n, d) or (a, b, 0, c), kHpPlaneBytes each: one tile
    U cnts;         // int[min(n_hyp, kHpMaxHyp)] the tile's inlier counts
    U words;        // uint64[ceil(3 tn / 64)]: the best model's inliers among the LIST, one bit per list position
    U misc;         // int[HE_N]
    U red;          // double[HER_N]
    U total;
};
template <typename U> MVOSR_HP_HD inline HpEvalPlan<U> hpeval_plan(U n, U tn, U n_hyp) {
    HpEvalPlan<U> p;
    const U plane = hp_align16<U>(8u * n);
    const U tile = n_hyp < (U)kHpMaxHyp ? n_hyp : (U)kHpMaxHyp;
    p.x = 0;
    p.y = p.x + plane;
    p.z = p.y + plane;
    p.list = p.z + plane;
    p.mods = p.list + hp_align16<U>(6u * tn);
    p.cnts = p.mods + (U)kHpPlaneBytes * tile;
    p.words = p.cnts + hp_align16<U>(4u * tile);
    p.misc = p.words + hp_align16<U>(8u * ((3u * tn + 63u) / 64u));
    p.red = p.misc + 4u * HE_N;
    p.total = p.red + 8u * HER_N;
    return p;
}

}  // namespace mvosr
