// mvosr_reliability_plan.hpp — the LDS layout of reliability_kernel (mvosr_reliability.hip), by the convention of
// mvosr_rescale_plan.hpp: the kernel takes every LDS pointer from the plan, the launcher requests its `total`, both
// evaluated at the launch header's (max_feat, max_tri); the offsets' type is a template parameter (uint32_t in the kernel,
// size_t in the launcher).  tests/test_reliability_cases.py checks alignment, overlap and containment with a host compiler.
//
// Plain C++ (<stdint.h> / <stddef.h> only): a host compiler reads it as it stands.
#pragma once

#include "mvosr_rescale_plan.hpp"

namespace mvosr {

// misc[] slots of reliability_kernel
enum { RM_BAD = 0, RM_DONE = 1, RM_WSUM = 8 /* [kRsWaves] */, RM_N = 16 };

// An "offer" is a (row, slot) pair, numbered 3 * row + slot: slot 0, 1, 2 of a row sorted to (s0, s1, s2) is the edge
// (s0, s1), (s0, s2), (s1, s2).  With N = max_feat, T = max_tri:
template <typename U> struct ReliabilityPlan {
    U work;         // see below
    U st;           // int[N + 2] where a vertex's incident rows start
    U it;           // uint16[3 T] incident rows, vertex by vertex
    U r16;          // uint16[T][3] the rows, each sorted ascending
    U inc;          // uint16[6 T] incident offers, vertex by vertex, in the order the reference's loop meets them
    U first;        // uint32[ceil(3 T / 32)] bit o: offer o is its edge's first (smallest row naming both ends)
    U abn;          // uint32[ceil(3 T / 32)] bit o: the edge of offer o is abnormal
    U misc;         // int[RM_N]
    U total;
    U work_bytes, bits_bytes;
    // in the work area.  Build phase (dead once every offer has its two bits):
    U z, v;         // double[N rounded up to even] each: remapped depth, pixel row
    // late aliases, alive from the barrier after the bits:
    U rel;          // = z: double[N rounded up to even] the reliabilities
    U lstart;       // int[N + 2] where a vertex's incident offers start ([n]: twice the number of edges)
    U ptr;          // int[N + 2] the vertex's next offer
};
template <typename U> MVOSR_HD inline ReliabilityPlan<U> reliability_plan(U max_feat, U max_tri) {
    ReliabilityPlan<U> p;
    const U T = max_tri, plane = 8u * plan_even<U>(max_feat), ints = 4u * (max_feat + 2);
    p.work_bytes = 2 * plane + 16;                   // (>= plane + 2 * ints: ints <= plane / 2 + 8)
    p.bits_bytes = 4u * ((3u * T + 31) / 32);
    p.work = 0;
    p.st = p.work + p.work_bytes;
    p.it = p.st + ints;
    p.r16 = p.it + plan_align<U>(6u * T, 4);
    p.inc = p.r16 + plan_align<U>(6u * T, 4);
    p.first = p.inc + plan_align<U>(12u * T, 4);
    p.abn = p.first + p.bits_bytes;
    p.misc = p.abn + p.bits_bytes;
    p.total = p.misc + 4u * RM_N;
    p.z = p.work;
    p.v = p.z + plane;
    p.rel = p.work;
    p.lstart = p.rel + plane;
    p.ptr = p.lstart + ints;
    return p;
}

}  // namespace mvosr
