// mvosr_heightpitch_tail_plan.hpp — the LDS layout of the two kernels of mvosr_height_pitch_tail_batch
// (mvosr_heightpitch_tail.hip) and the layout of the carry record they hand from one chunk of a sequence to the next.
//
// As in mvosr_heightpitch_plan.hpp: a struct of named byte offsets into the workgroup's dynamic LDS plus `total`.  The kernels
// take their pointers from the plan evaluated at the list they hold — a source frame's features, or the carry-in's inliers —
// and the launcher requests `total` at max(max_feat, carry_cap); every offset grows with the size, every offset is a multiple
// of 16, and no region is reused (tests/test_heightpitch_resident_cases.py checks all of that with a host compiler).
//
// Plain C++ (<stdint.h> / <stddef.h> only).
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MVOSR_HPT_HD __host__ __device__
#else
#define MVOSR_HPT_HD
#endif

namespace mvosr {

constexpr int kHptWaves = 4;            // wavefronts of a workgroup
constexpr int kHptBlock = 256;          // ... one thread per node of the pairwise recursion (kHptNodes)
constexpr int kHptNodes = 256;          // nodes of an 8192-element list's pairwise recursion by heap index (mvosr_npsum.hpp)
constexpr int kHptMaxList = 8192;       // the longest list a tail sums: one buffer of np.add.reduce (kNpBufSize)
constexpr int kHptCarryHeader = 64;     // bytes of mvosr_height_pitch_carry, in front of the record's three arrays

// misc[] slots
enum { HTM_CW = 0 /* [kHptWaves] survivors per wavefront */, HTM_FIT = 8 /* [kHptWaves] last fitted frame per wavefront */,
       HTM_ERR = 16 /* [kHptWaves] 64-bit: first error per wavefront */, HTM_N = 32 };

template <typename U> MVOSR_HPT_HD inline U hpt_align16(U v) { return (v + 15u) & ~(U)15; }

template <typename U> struct HpTailPlan {
    U terms;        // double[n]: z sin + y cos of the source frame's inliers, in feature order
    U node;         // double[kHptNodes + 2]: the recursion's nodes, then the running sum's slot
    U misc;         // int[HTM_N]
    U total;
};
template <typename U> MVOSR_HPT_HD inline HpTailPlan<U> hptail_plan(U n) {
    HpTailPlan<U> p;
    p.terms = 0;
    p.node = p.terms + hpt_align16<U>(8u * n);
    p.misc = p.node + 8u * (U)(kHptNodes + 2);
    p.total = p.misc + 4u * (U)HTM_N;
    return p;
}

// The carry record: the header, then y[cap], z[cap] (doubles) and index[cap] (int32); cap is even, so every array is 8-byte aligned.
template <typename U> struct HpCarryPlan { U y, z, index, total; };
template <typename U> MVOSR_HPT_HD inline HpCarryPlan<U> hpcarry_plan(U cap) {
    HpCarryPlan<U> p;
    cap = (cap + 1u) & ~(U)1;
    p.y = (U)kHptCarryHeader;
    p.z = p.y + 8u * cap;
    p.index = p.z + 8u * cap;
    p.total = hpt_align16<U>(p.index + 4u * cap);
    return p;
}

}  // namespace mvosr
