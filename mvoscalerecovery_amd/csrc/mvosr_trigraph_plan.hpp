// mvosr_trigraph_plan.hpp — the LDS layout of tri_graph_kernel (mvosr_trigraph.hip), by the convention of
// mvosr_rescale_plan.hpp: the kernel takes every LDS pointer from the plan, the launcher requests its `total`, both
// evaluated at the launch header's (max_feat, max_tri); the offsets' type is a template parameter (uint32_t in the kernel,
// size_t in the launcher).  tests/test_trigraph_cases.py checks alignment, overlap and containment with a host compiler.
//
// Plain C++ (<stdint.h> / <stddef.h> only): a host compiler reads it as it stands.
#pragma once

#include "mvosr_rescale_plan.hpp"

namespace mvosr {

// misc[] slots of tri_graph_kernel
enum { TM_BAD = 0, TM_SINGULAR = 1, TM_NFLAT = 2, TM_NSTEEP = 3, TM_NVALID = 4, TM_CNT = 5 /* [3] rows finished per round */,
       TM_WSUM = 8 /* [kRsWaves] */, TM_LEAVES = 16, TM_N = 20 };

// the `leaf` region, in doubles: the leaves' sums of one 8192-element chunk of np.add.reduce (a leaf has more than 64 elements
// unless the chunk is one), the running total, the walk's stack of partial sums (one per level), its stack of (lo, n, stage)
// ints, and the leaves' (start, length) as 16-bit pairs
enum { TL_SUMS = 0, TL_SLOT = 128, TL_VAL = 129 /* [9] */, TL_STACK = 138 /* 24 ints */, TL_TABLE = 150 /* 256 uint16 */, TL_N = 214 };
constexpr int kTgLeafSlots = TL_N;

// With N = max_feat, T = max_tri.  Alive from phase 1 to the end: h, p0, nb, lvl, flag, sel, misc.  The work area holds, one
// after the other: the vertex planes (from-points form, phase 1); the incident-rows table and the 16-bit rows (phases 2-3);
// the steep rows' heights packed in row order and the leaves' sums (phase 4); the final probabilities (phases 5-6).
template <typename U> struct TriGraphPlan {
    U work;         // see below
    U h;            // double[T] a row's mean height
    U p0;           // double[T] a row's initial probability
    U nb;           // uint16[T][3] a row's neighbours in the reference's list order, 0xFFFF: none
    U lvl;          // uint16[T] 1 + the round in which a flat row got its final probability, 0: not yet
    U flag;         // uint8[T] bit 0: flat (pitch < thr), bit 1: steep (pitch >= thr)
    U sel;          // uint32[ceil(N / 32)] bit i: feature i is a vertex of a valid row
    U misc;         // int[TM_N]
    U total;
    U work_bytes;
    // in the work area
    U x, y, z;      // phase 1, from-points form: double[N rounded up to even] each
    U st;           // phases 2-3: int[N + 2] where a vertex's incident rows start
    U it;           // phases 2-3: uint16[3 T] incident rows, vertex by vertex
    U r16;          // phases 2-3: uint16[T][3] the rows as given
    U hs;           // phase 4: double[T] the steep rows' heights in row order
    U leaf;         // phase 4: double[kTgLeafSlots]
    U p1;           // phases 5-6: double[T] a flat row's final probability
};
template <typename U> MVOSR_HD inline TriGraphPlan<U> trigraph_plan(bool pts, U max_feat, U max_tri) {
    TriGraphPlan<U> p;
    const U T = max_tri, plane = 8u * plan_even<U>(max_feat), ints = plan_align<U>(4u * (max_feat + 2), 8);
    const U rows16 = plan_align<U>(6u * T, 8);
    U w = ints + 2 * rows16;                                         // st, it, r16
    const U level = 8u * T + 8u * (U)kTgLeafSlots;                   // hs, leaf (>= p1)
    if (level > w) w = level;
    if (pts && 3 * plane > w) w = 3 * plane;
    p.work_bytes = plan_align<U>(w, 16);
    p.work = 0;
    p.h = p.work + p.work_bytes;
    p.p0 = p.h + 8u * T;
    p.nb = p.p0 + 8u * T;
    p.lvl = p.nb + rows16;
    p.flag = p.lvl + plan_align<U>(2u * T, 8);
    p.sel = p.flag + plan_align<U>(T, 8);
    p.misc = p.sel + plan_align<U>(4u * ((max_feat + 31) / 32), 8);
    p.total = p.misc + 4u * TM_N;
    p.x = p.work;
    p.y = p.x + plane;
    p.z = p.y + plane;
    p.st = p.work;
    p.it = p.st + ints;
    p.r16 = p.it + rows16;
    p.hs = p.work;
    p.leaf = p.hs + 8u * T;
    p.p1 = p.work;
    return p;
}

}  // namespace mvosr
