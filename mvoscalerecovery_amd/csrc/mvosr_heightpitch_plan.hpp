// mvosr_heightpitch_plan.hpp — the LDS layout of height_pitch_kernel (mvosr_heightpitch.hip).
//
// As in mvosr_rescale_plan.hpp: a struct of named byte offsets into the workgroup's dynamic LDS plus `total`.  The kernel takes
// every LDS pointer from the plan evaluated at the frame's own (n, tn) and the launch's n_hyp; the launcher requests `total` of
// the same function at the header's (max_feat, max_tri, n_hyp).  Every offset grows with the sizes, so a frame that passes the
// kernel's `n <= max_feat && tn <= max_tri` guard lies inside what was requested; every offset is a multiple of 16 (the widest
// access is the 16-byte read of a hypothesis' plane), and no region is reused: nothing aliases
// (tests/test_heightpitch_cases.py checks all of that with a host compiler).
//
// Plain C++ (<stdint.h> / <stddef.h> only).
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MVOSR_HP_HD __host__ __device__
#else
#define MVOSR_HP_HD
#endif

namespace mvosr {

constexpr int kHpWaves = 8;             // wavefronts of a workgroup
constexpr int kHpMaxHyp = 512;          // hypotheses per frame, at most
constexpr int kHpPlaneBytes = 32;       // a hypothesis' unit (n, d): one double4

// misc[] slots of height_pitch_kernel
enum { HM_SINGULAR = 0, HM_BADID = 1, HM_BEST = 2, HM_BESTIC = 3, HM_USED = 4, HM_NIN = 5, HM_I0 = 6 /* [3] first inliers */,
       HM_CW = 16 /* [kHpWaves] kept rows per wavefront */, HM_N = 32 };
// red[] (doubles): three reduction slots of 2 kHpWaves each, then the frame's scalars
enum { HR_SUM = 0, HR_DEV = 2 * kHpWaves, HR_MODEL = 4 * kHpWaves /* [4] */, HR_NHAT = 4 * kHpWaves + 4 /* [3] */, HR_N = 4 * kHpWaves + 8 };

template <typename U> MVOSR_HP_HD inline U hp_align16(U v) { return (v + 15u) & ~(U)15; }

template <typename U> struct HeightPitchPlan {
    U x, y, z;      // double[n] each: the back-projected points (:67-68), alive to the end
    U list;         // uint16[3 tn]: the point list as vertex ids, 3 per kept row in row order (:114-116)
    U mods;         // [n_hyp] unit (n, d), kHpPlaneBytes each
    U cnts;         // int[n_hyp] inlier counts
    U words;        // uint64[ceil(n / 64)]: the inlier mask at 0.01 (:149), one ballot per 64 features
    U misc;         // int[HM_N]
    U red;          // double[HR_N]
    U total;
};
template <typename U> MVOSR_HP_HD inline HeightPitchPlan<U> heightpitch_plan(U n, U tn, U n_hyp) {
    HeightPitchPlan<U> p;
    const U plane = hp_align16<U>(8u * n);
    p.x = 0;
    p.y = p.x + plane;
    p.z = p.y + plane;
    p.list = p.z + plane;
    p.mods = p.list + hp_align16<U>(6u * tn);
    p.cnts = p.mods + (U)kHpPlaneBytes * n_hyp;
    p.words = p.cnts + hp_align16<U>(4u * n_hyp);
    p.misc = p.words + hp_align16<U>(8u * ((n + 63u) / 64u));
    p.red = p.misc + 4u * HM_N;
    p.total = p.red + 8u * HR_N;
    return p;
}

}  // namespace mvosr
