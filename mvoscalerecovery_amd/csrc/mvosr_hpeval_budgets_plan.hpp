// mvosr_hpeval_budgets_plan.hpp — the LDS layout of height_pitch_eval_budgets_kernel (mvosr_hpeval_budgets.hip).
//
// As mvosr_hpeval_plan.hpp, whose plan it takes whole: named byte offsets into the workgroup's dynamic LDS plus `total`, one
// function shared by the kernel (at the frame's own n, tn and the launch's last budget and number of budgets) and the launcher (at
// the header's max_feat, max_tri).  On top of hpeval_plan it adds ONE region: a snapshot of the replay's state per checkpoint,
// kHpeSnapBytes each, rewritten for every case.  Every offset is a multiple of 16; no region is reused.  The request exceeds
// hpeval_plan's by the snapshots only: it does not grow with the number of cases, nor with the last budget beyond one tile of
// kHpMaxHyp (tests/test_hpeval_budgets_cases.py checks all of that with a host compiler).
//
// Plain C++ (<stdint.h> / <stddef.h> only).
#pragma once

#include "mvosr_hpeval_plan.hpp"

namespace mvosr {

constexpr int kHpeMaxBudgets = 16;      // checkpoints per launch, at most

// the replay's carried state at a checkpoint (RansacReplay of mvosr_ransac.hpp; `used` is the budget unless the goal stop came
// earlier) and the best model as its tile held it (raw: the sign rule comes after)
struct HpeSnapshot { int32_t best, best_ic, used, done; double m[4]; };
constexpr int kHpeSnapBytes = 48;
static_assert(sizeof(HpeSnapshot) == kHpeSnapBytes && kHpeSnapBytes % 16 == 0, "a snapshot is 48 bytes");

// misc[] slot of height_pitch_eval_budgets_kernel beside HE_*: the next checkpoint of the case
enum { HB_NEXT = 14 };
static_assert(HB_NEXT > HE_DEGEN && HB_NEXT < HM_CW, "slots");

template <typename U> struct HpEvalBudgetsPlan {
    HpEvalPlan<U> frame;    // hpeval_plan(n, tn, the last budget): everything height_pitch_eval_kernel keeps
    U snap;                 // HpeSnapshot[n_budgets]
    U total;
};
template <typename U> MVOSR_HP_HD inline HpEvalBudgetsPlan<U> hpeval_budgets_plan(U n, U tn, U n_hyp_max, U n_budgets) {
    HpEvalBudgetsPlan<U> p;
    p.frame = hpeval_plan<U>(n, tn, n_hyp_max);
    p.snap = hp_align16<U>(p.frame.total);
    p.total = p.snap + (U)kHpeSnapBytes * n_budgets;
    return p;
}

}  // namespace mvosr
