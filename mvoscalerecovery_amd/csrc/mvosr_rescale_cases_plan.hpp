// mvosr_rescale_cases_plan.hpp — the LDS layout of flat_ransac_cases_kernel (mvosr_rescale_cases.hip).
//
// As mvosr_rescale_plan.hpp: named byte offsets into the workgroup's dynamic LDS plus `total`, one function shared by the kernel
// (at the frame's own feat_cnt and row count, and the launch's n_hyp) and the launcher (at the header's max_feat, max_tri).  Every
// offset grows with the sizes and is a multiple of 16, so a frame that passes the kernel's `<= max_feat / max_tri` guard lies
// inside what was requested (tests/test_rescale_cases_plan.py checks that, the alignments, and that regions that are live
// together do not overlap).  The offsets' type is a template parameter: the kernel carves in uint32_t, the launcher asks in size_t.
//
// What lives when.  Written ONCE per workgroup, read by every case: the survivors' planes x / y / z, the point list, and the
// counting form in `aux`.  Rewritten per case: the hypotheses' planes and their counts.  `aux` holds, while the form is built, the
// multiplicities `w` and the distinct vertices `dv`; a frame with at most kCasesPackMax distinct vertices then has their
// coordinates and multiplicities written side by side over the same room (`px`, `py`, `pz`, `pw` — the ids and multiplicities
// are in registers by then); a frame with more keeps `w` and `dv` and gathers.
//
// Plain C++ (<stdint.h> / <stddef.h> only): a host compiler reads it as it stands.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MVOSR_CASES_HD __host__ __device__
#else
#define MVOSR_CASES_HD
#endif

namespace mvosr {

constexpr int kCasesMaxHyp = 512;       // hypotheses per (frame, case), at most (mvosr_flat_ransac_batch's limit)
constexpr int kCasesMaxCases = 4096;    // cases per launch, at most
constexpr int kCasesPackMax = 1024;     // distinct kept vertices up to which the packed counting form is built
constexpr int kCasesPlaneBytes = 4 * sizeof(double);   // a hypothesis' unit (n, d): two double2

// misc[] slots of flat_ransac_cases_kernel (slots below CM_CW are zeroed at the start)
enum { CM_BAD = 0, CM_ND = 1, CM_CW = 16 /* [16] per-wave survivor counts */, CM_CW2 = 32 /* [16] per-wave kept-row counts */, CM_N = 48 };

template <typename U> MVOSR_CASES_HD inline U cases_align16(U v) { return (v + 15u) & ~(U)15u; }

template <typename U> struct CasesPlan {
    U x, y, z;      // double[n_all rounded up to even] each: the survivors, compacted in order
    U list;         // uint16[3 tn]: the point list as survivor-numbered vertex ids (3 per KEPT row: tn rows is the bound)
    U aux;          // the counting form, aux_bytes
    U mods;         // [n_hyp] unit (n, d), kCasesPlaneBytes each
    U cnts;         // int[n_hyp] inlier counts
    U misc;         // int[CM_N]
    U total;
    U aux_bytes;
    // in aux, while the form is built (and for good in the gather form):
    U w;            // int[n_all] multiplicity of a vertex in the list
    U dv;           // uint16[n_all] the distinct vertices
    // in aux, the packed form (n_items <= kCasesPackMax distinct vertices), written once w and dv are in registers:
    U px;           // double[3][n_items], then int[n_items]: at most 28 * min(n_all, kCasesPackMax) bytes
};
template <typename U> MVOSR_CASES_HD inline CasesPlan<U> cases_plan(U n_all, U tn, U n_hyp) {
    CasesPlan<U> p;
    const U plane = 8u * ((n_all + 1u) & ~(U)1u);
    const U build = cases_align16<U>(4u * n_all) + cases_align16<U>(2u * n_all);
    const U packed = cases_align16<U>(28u * (n_all < (U)kCasesPackMax ? n_all : (U)kCasesPackMax));
    p.aux_bytes = build > packed ? build : packed;
    p.x = 0;
    p.y = p.x + plane;
    p.z = p.y + plane;
    p.list = p.z + plane;
    p.aux = p.list + cases_align16<U>(6u * tn);
    p.mods = p.aux + p.aux_bytes;
    p.cnts = p.mods + (U)kCasesPlaneBytes * n_hyp;
    p.misc = p.cnts + cases_align16<U>(4u * n_hyp);
    p.total = p.misc + 4u * CM_N;
    p.w = p.aux;
    p.dv = p.aux + cases_align16<U>(4u * n_all);
    p.px = p.aux;
    return p;
}

}  // namespace mvosr
