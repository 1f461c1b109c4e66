// mvosr_hpeval_carry_plan.hpp — the launch shapes and the LDS layout of the three kernels of mvosr_height_pitch_eval_tail_batch
// (mvosr_hpeval_carry.hip) and the layout of the carry record they hand from one chunk of a sequence to the next.
//
// As in mvosr_heightpitch_tail_plan.hpp: named byte offsets plus `total`, shared by the kernels and their launcher.  Only the
// resolve kernel uses LDS, and its plan does not grow with anything: a few words per wavefront.
//
// Plain C++ (<stdint.h> / <stddef.h> only).
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MVOSR_HEC_HD __host__ __device__
#else
#define MVOSR_HEC_HD
#endif

namespace mvosr {

constexpr int kHecWaves = 4;            // wavefronts of a workgroup, all three kernels
constexpr int kHecBlock = 256;          // ... and its threads: the resolve kernel's round of frames
constexpr int kHecTileF = 64;           // apply kernel: frames of a workgroup — one wavefront's lanes, so its stores are contiguous
constexpr int kHecTileE = 4;            // apply kernel: (case, budget) elements of a workgroup, one per wavefront
constexpr int kHecCarryHeader = 16;     // bytes of mvosr_height_pitch_eval_carry, in front of the record's arrays
constexpr int kHecCarryDoubles = 8;     // the six values, sum_y, sum_z — one double[n_cases * n_budgets] each
constexpr int kHecMaxCases = 1024;      // kHpeMaxCases
constexpr int kHecMaxBudgets = 16;      // kHpeMaxBudgets

static_assert(kHecBlock == kHecWaves * 64 && kHecTileF * kHecTileE == kHecBlock, "one thread per element of a tile");

// misc[] slots of the resolve kernel
enum { HEM_FIT = 0 /* [kHecWaves] last fitted frame per wavefront */, HEM_ERR = 8 /* [kHecWaves] 64-bit: first error per wavefront */,
       HEM_N = 16 };

template <typename U> MVOSR_HEC_HD inline U hec_align16(U v) { return (v + 15u) & ~(U)15; }

template <typename U> struct HpEvalTailPlan {
    U misc;         // int[HEM_N]
    U total;
};
template <typename U> MVOSR_HEC_HD inline HpEvalTailPlan<U> hpeval_tail_plan() {
    HpEvalTailPlan<U> p;
    p.misc = 0;
    p.total = hec_align16<U>(4u * (U)HEM_N);
    return p;
}

// The carry record: the header, then value[8][E] (doubles: ransac_height, refined_mean, refined_std, height_t_mean, refined_pitch,
// n_inliers, sum_y, sum_z) and degenerate[E] (uint8), E = n_cases * n_budgets, element (c, b) at c * n_budgets + b.
template <typename U> struct HpEvalCarryPlan { U value, degenerate, total; };
template <typename U> MVOSR_HEC_HD inline HpEvalCarryPlan<U> hpeval_carry_plan(U n_elem) {
    HpEvalCarryPlan<U> p;
    p.value = (U)kHecCarryHeader;
    p.degenerate = p.value + 8u * (U)kHecCarryDoubles * n_elem;
    p.total = hec_align16<U>(p.degenerate + n_elem);
    return p;
}

}  // namespace mvosr
