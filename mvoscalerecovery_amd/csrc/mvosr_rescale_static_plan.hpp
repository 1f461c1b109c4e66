// mvosr_rescale_static_plan.hpp — the LDS layout of flat_static_tri_kernel (mvosr_rescale_static.hip).
//
// As mvosr_rescale_plan.hpp and mvosr_rescale_sweep_plan.hpp: named byte offsets into the workgroup's dynamic LDS plus `total`, one
// function shared by the kernel (at the frame's own survivor room and row count) and the launcher (at the header's max_feat,
// max_tri).  Every offset grows with the sizes and is a multiple of 16, so a frame that passes the kernel's `<= max_feat / max_tri`
// guard lies inside what was requested (tests/test_static_resident_cases.py checks that, the alignments, and that regions that are
// live together do not overlap).  The offsets' type is a template parameter: the kernel carves in uint32_t, the launcher asks in
// size_t, where a header may name any size and the request is refused by its byte count.
//
// What lives when.  The fused form's phase 1 reads the survivors' planes x / y / z in `work` and writes every row's height and its
// two bits.  The planes are dead behind the barrier that ends it; the median search's histogram (and behind it the short candidate
// list) takes their place.  The heights and flags stay to the end: the road model's 19 bins are counted from them.
// The given form (heights and flags read from global memory, in row form) is the plan at (0, 0): it keeps no row in LDS.
//
// Plain C++ (<stdint.h> / <stddef.h> only): a host compiler reads it as it stands.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "mvosr_rescale_plan.hpp"

#ifdef __HIPCC__
#define MVOSR_STATIC_HD __host__ __device__
#else
#define MVOSR_STATIC_HD
#endif

namespace mvosr {

constexpr int kStaticWaves = 16;        // wavefronts of a workgroup: the frame holds most of a CU's LDS, one workgroup per CU
constexpr int kStaticModelBins = 19;    // the road model's histogram (scale_calculator.py:297)

// misc[] of flat_static_tri_kernel: flat_selection_kernel's slots (FM_*, mvosr_rescale_plan.hpp), whose slot 9 — the plane fit's
// FM_ND — is this kernel's "a counted height is no positive finite number"
enum { FM_BADH = FM_ND };
static_assert(kStaticWaves <= FM_CW - FM_WSUM && FM_CW + kStaticWaves <= FM_N, "flat_static_tri_kernel: per-wave slots in misc");

template <typename U> MVOSR_STATIC_HD inline U static_align16(U v) { return (v + 15u) & ~(U)15u; }

template <typename U> struct StaticPlan {
    U heights;      // double[tn] every row's height, by row (>= 0 where a row is loose: the patterns order like the values)
    U flags;        // uint8[tn] every row's flags, by row
    U ext;          // uint64[4] smallest / largest loose height (bits), smallest above the median, the ranked candidate
    U misc;         // int[FM_N]
    U model;        // int[32] the road model's 19 bins
    U work;         // work_bytes
    U total;
    U work_bytes;
    // in work, phase 1:
    U x, y, z;      // double[n rounded up to even] each: the survivors, compacted in order
    // in work, from the barrier that ends phase 1:
    U hist;         // int[kFlatBins]; later the short candidate list, uint64[kFlatDirect]
};
template <typename U> MVOSR_STATIC_HD inline StaticPlan<U> static_plan(U n, U tn) {
    StaticPlan<U> p;
    const U plane = 8u * ((n + 1u) & ~(U)1u);
    const U hist = 4u * (U)kFlatBins;
    p.work_bytes = 3u * plane > hist ? 3u * plane : hist;
    p.heights = 0;
    p.flags = p.heights + static_align16<U>(8u * tn);
    p.ext = p.flags + static_align16<U>(tn);
    p.misc = p.ext + 4u * 8u;
    p.model = p.misc + 4u * (U)FM_N;
    p.work = p.model + 4u * 32u;
    p.total = p.work + p.work_bytes;
    p.x = p.work;
    p.y = p.x + plane;
    p.z = p.y + plane;
    p.hist = p.work;
    return p;
}

}  // namespace mvosr
