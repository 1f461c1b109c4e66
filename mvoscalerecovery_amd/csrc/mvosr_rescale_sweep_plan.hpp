// mvosr_rescale_sweep_plan.hpp — the LDS layout of flat_selection_sweep_kernel (mvosr_rescale_sweep.hip).
//
// As mvosr_rescale_plan.hpp: named byte offsets into the workgroup's dynamic LDS plus `total`, one function shared by the kernel
// (at the frame's own feat_cnt and row count, and the launch's n_sel) and the launcher (at the header's max_feat, max_tri).  Every
// offset grows with the sizes and is a multiple of 16, so a frame that passes the kernel's `<= max_feat / max_tri` guard lies
// inside what was requested (tests/test_sweep_cases.py checks that, the alignments, and that regions that are live together do
// not overlap).  The offsets' type is a template parameter: the kernel carves in uint32_t, the launcher asks in size_t.
//
// What lives when.  Phase 1 (once per frame) reads the survivors' planes x / y / z in `work` and writes every row's height and
// its two bits per setting.  The planes are dead behind the barrier that ends it; phase 2 (one setting per wavefront) reads the
// heights and the bits, and every wavefront has a kSweepBins-word histogram of its own where the planes were.
//
// Plain C++ (<stdint.h> / <stddef.h> only): a host compiler reads it as it stands.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MVOSR_SWEEP_HD __host__ __device__
#else
#define MVOSR_SWEEP_HD
#endif

namespace mvosr {

constexpr int kSweepWaves = 16;         // wavefronts of a workgroup: the frame holds most of a CU's LDS, one workgroup per CU
constexpr int kSweepMaxSel = 16;        // settings per launch, at most: two bits each in a row's 32-bit word, one wavefront each
constexpr int kSweepBins = 256;         // the median search resolves 8 bits of the heights' patterns a pass

// misc[] slots of flat_selection_sweep_kernel (slots below SM_CW are zeroed at the start)
enum { SM_SINGULAR = 0, SM_BADID = 1, SM_CW = 16 /* [kSweepWaves] per-wave survivor counts */, SM_N = 32 };

template <typename U> MVOSR_SWEEP_HD inline U sweep_align16(U v) { return (v + 15u) & ~(U)15u; }

template <typename U> struct SweepPlan {
    U heights;      // double[tn] every row's height, by row (>= 0 where a row is loose: the patterns order like the values)
    U bits;         // uint32[tn] by row: bit 2 s = pitch < loose_s, bit 2 s + 1 = pitch < tight_s
    U misc;         // int[SM_N]
    U thr;          // double[2][n_sel] the sines of the loose, then of the tight thresholds
    U work;         // work_bytes
    U total;
    U work_bytes;
    // in work, phase 1:
    U x, y, z;      // double[n_all rounded up to even] each: the survivors, compacted in order
    // in work, phase 2:
    U hist;         // int[kSweepWaves][kSweepBins] a histogram per wavefront
};
template <typename U> MVOSR_SWEEP_HD inline SweepPlan<U> sweep_plan(U n_all, U tn, U n_sel) {
    SweepPlan<U> p;
    const U plane = 8u * ((n_all + 1u) & ~(U)1u);
    const U hist = 4u * (U)kSweepBins * (U)kSweepWaves;
    p.work_bytes = 3u * plane > hist ? 3u * plane : hist;
    p.heights = 0;
    p.bits = p.heights + sweep_align16<U>(8u * tn);
    p.misc = p.bits + sweep_align16<U>(4u * tn);
    p.thr = p.misc + 4u * SM_N;
    p.work = p.thr + 16u * n_sel;
    p.total = p.work + p.work_bytes;
    p.x = p.work;
    p.y = p.x + plane;
    p.z = p.y + plane;
    p.hist = p.work;
    return p;
}

}  // namespace mvosr
