// mvosr_rescale_plan.hpp — the LDS layouts of the rescale-variant kernels (mvosr_rescale.hip), one plan per kernel.
//
// A plan is a struct of named byte offsets into the workgroup's dynamic LDS plus `total`.  The kernel takes every LDS
// pointer from its plan, evaluated at the sizes it carves from (a frame's own counts, or the launch header's); the launcher
// requests `total` of the same function evaluated at the header's (max_feat, max_tri, n_hyp).  Every offset grows with the
// sizes, so a frame that passes the kernel's `<= max_feat / max_tri` guard lies inside what was requested
// (tests/test_rescale_plan.py checks that, the alignments, and that no two regions that are live together overlap).
//
// The offsets' type is a template parameter: the kernels carve in uint32_t (LDS addresses are 32-bit; 64-bit offsets cost
// flat_selection_kernel scalar registers), the launchers ask in size_t, where a header may name any size and the request is
// refused by its byte count.
//
// Plain C++ (<stdint.h> / <stddef.h> only): a host compiler reads it as it stands.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MVOSR_HD __host__ __device__
#else
#define MVOSR_HD
#endif

namespace mvosr {

constexpr int kRsWaves = 8;             // wavefronts of a workgroup (flat_selection_kernel's device-resident form brings 16)
constexpr int kFlatBins = 2048;         // the level's search (mvosr_flat.hpp): one histogram pass resolves 11 bits of the candidates' range
constexpr int kFlatDirect = 64;         // ... and that few candidates left: wavefront 0 ranks them directly
constexpr int kGrowBins = 256;          // grow_median: an 8-bit radix pass
constexpr int kPlaneBytes = 4 * sizeof(double);   // a hypothesis' unit (n, d): one double4, or two double2

// misc[] slots of flat_selection_kernel and its siblings — the large kernel's and the static_tri kernel's plans hold the same
// int[FM_N] — (slots below FM_WSUM are zeroed at the start; slot 9 is the static_tri kernel's FM_BADH)
enum { FM_K = 0, FM_SINGULAR = 1, FM_BADID = 2, FM_KEPT = 3, FM_BIN = 4, FM_RANK = 5, FM_BINCNT = 6, FM_LE = 7, FM_LIST = 8, FM_ND = 9,
       FM_WSUM = 16 /* [16] per-wave bin totals */, FM_CW = 32 /* [16] per-wave counts of the ordered compactions */, FM_N = 48 };
// misc[] slots of region_grow_kernel
enum { GM_BAD = 0, GM_SINGULAR = 1, GM_KLEVEL = 2, GM_NFLAT = 3, GM_BIN = 4, GM_RANK = 5, GM_LE = 6 /* [2] */, GM_CHANGED = 8 /* [3] */,
       GM_WSUM = 16 /* [kRsWaves] */, GM_N = 32 };

template <typename U> MVOSR_HD inline U plan_even(U n) { return (n + 1) & ~(U)1; }
template <typename U> MVOSR_HD inline U plan_align(U v, U a) { return (v + (a - 1)) & ~(a - 1); }

// graph_inliers_kernel, carved from the frame's n
template <typename U> struct GraphPlan {
    U p;            // double2[n rounded up to even] {v, z}
    U cnt;          // uint32[n + 4] a vertex's two 16-bit tallies
    U flag;         // int[2] bad vertex id, features that passed (in 16 bytes)
    U total;
};
template <typename U> MVOSR_HD inline GraphPlan<U> graph_plan(U n) {
    GraphPlan<U> p;
    p.p = 0;
    p.cnt = p.p + 16u * plan_even<U>(n);
    p.flag = p.cnt + 4u * (n + 4);
    p.total = p.flag + 16;
    return p;
}

// flat_selection_kernel, carved from the frame's n_all and tn.  Stage form (dev = false): the vertex planes are dead once
// the normals are done and the histogram of the median search takes their place.  Device-resident form: the planes live on
// for the RANSAC, the histogram has its own room, and the hypotheses follow the flags.
template <typename U> struct FlatPlan {
    U heights;      // double[tn] every row's height, by row (>= 0: read as 64-bit patterns they order like the values)
    U ext;          // uint64[4] smallest / largest loose height (bits), smallest above the median, the ranked candidate
    U misc;         // int[FM_N]
    U x, y, z;      // double[n rounded up to even] each
    U hist;         // int[kFlatBins]; later the short candidate list, uint64[kFlatDirect]
    U flags;        // uint8[tn] every row's flags, by row
    U mods;         // dev: [n_hyp] unit (n, d), kPlaneBytes each, 16-aligned
    U cnts;         // dev: int[n_hyp] inlier counts
    U total;
    U heights_bytes, hist_bytes;   // room of the two regions the late aliases reuse
    // late aliases (dev), alive from the barrier after the last comparison of a height with the level:
    U list;         // = heights: uint16[3 per kept row] the point list; the distinct vertices, uint16[n], follow it at
                    //   the list's length rounded up to even where both fit heights_bytes (`dedup`)
    U w2;           // = hist: uint32[n / 2 + 1] two 16-bit multiplicities per word (`dedup` caps n at 2 kFlatBins - 2)
    U packed;       // = heights: double[3][n_items] + int[n_items] the distinct vertices' coordinates and multiplicities,
                    //   once the list and the distinct vertices are in registers (`packed`: 28 n_items + 8 <= heights_bytes)
};
template <typename U> MVOSR_HD inline FlatPlan<U> flat_plan(bool dev, U n, U tn, U n_hyp) {
    FlatPlan<U> p;
    const U plane = 8u * plan_even<U>(n);
    p.heights_bytes = 8u * tn;
    p.hist_bytes = 4u * kFlatBins;
    p.heights = 0;
    p.ext = p.heights + p.heights_bytes;
    p.misc = p.ext + 4 * 8;
    p.x = p.misc + 4u * FM_N;
    p.y = p.x + plane;
    p.z = p.y + plane;
    p.hist = dev ? p.z + plane : p.x;
    p.flags = dev ? p.hist + p.hist_bytes : p.x + (3 * plane > p.hist_bytes ? 3 * plane : p.hist_bytes);
    p.mods = plan_align<U>(p.flags + tn, 16);
    p.cnts = p.mods + kPlaneBytes * n_hyp;
    // (slack as the launchers have always asked for it: 16 bytes behind the last array, and in the device-resident form
    // 32 for the hypotheses' alignment, which takes 15 at most)
    p.total = p.flags + tn + (dev ? 32 + (kPlaneBytes + 4) * n_hyp : 0) + 16;
    p.list = p.heights;
    p.w2 = p.hist;
    p.packed = p.heights;
    return p;
}

// ransac_plane_kernel
template <typename U> struct RansacPlan {
    U mods;         // [n_hyp] unit (n, d), kPlaneBytes each
    U cnts;         // int[n_hyp] inlier counts
    U total;
};
template <typename U> MVOSR_HD inline RansacPlan<U> ransac_plan(U n_hyp) {
    RansacPlan<U> p;
    p.mods = 0;
    p.cnts = p.mods + kPlaneBytes * n_hyp;
    p.total = p.cnts + 4u * n_hyp + 16;
    return p;
}

// triangle_batch_kernel, carved from the frame's n
template <typename U> struct TriBatchPlan {
    U x, y, z;      // double[n rounded up to even] each
    U red;          // double[3][2 kRsWaves] one scratch slot per block reduction
    U flag;         // int[2] singular row, bad vertex id
    U total;
};
template <typename U> MVOSR_HD inline TriBatchPlan<U> tribatch_plan(U n) {
    TriBatchPlan<U> p;
    const U plane = 8u * plan_even<U>(n);
    p.x = 0;
    p.y = p.x + plane;
    p.z = p.y + plane;
    p.red = p.z + plane;
    p.flag = p.red + 8u * 3 * 2 * kRsWaves;
    p.total = p.flag + 32;
    return p;
}

// region_grow_kernel, carved from the launch header's max_feat and max_tri (T rows).  The work area holds, one after the
// other, the vertex planes (pts), the vertex -> incident rows table, and the labels.
template <typename U> struct GrowPlan {
    U hinv;         // double[T] 1 / height by row
    U ang;          // double[T] pitch by row
    U ext;          // uint64[8]: [0], [1] the medians' "smallest above", [2] the best root's key
    U work;
    U misc;         // int[GM_N]
    U hist;         // int[kGrowBins]
    U nb;           // uint16[T][3] joined neighbours (in a multiple of 16 bytes)
    U total;
    U work_bytes;
    // in the work area.  pts, phase 1 (dead once every row has its height and pitch):
    U x, y, z;      // double[max_feat rounded up to even] each
    // phases 3 and 4:
    U r16;          // uint16[T][3] the rows
    U inc;          // uint16[3 T] incident rows, vertex by vertex
    U start;        // int[n + 1] where a vertex's rows start (room for max_feat + 2)
    // late alias, phase 5 (the table is dead once the joined neighbours exist):
    U label;        // = work: int[T] labels, then int[T] sizes and seed flags at the roots
};
template <typename U> MVOSR_HD inline GrowPlan<U> grow_plan(bool pts, U max_feat, U max_tri) {
    GrowPlan<U> p;
    const U T = max_tri, plane = 8u * plan_even<U>(max_feat);
    const U table = plan_align<U>(12u * T + 4u * (max_feat + 2), 8);
    p.work_bytes = pts && 3 * plane > table ? 3 * plane : table;
    p.hinv = 0;
    p.ang = p.hinv + 8u * T;
    p.ext = p.ang + 8u * T;
    p.work = p.ext + 8 * 8;
    p.misc = p.work + p.work_bytes;
    p.hist = p.misc + 4u * GM_N;
    p.nb = p.hist + 4u * kGrowBins;
    p.total = p.nb + plan_align<U>(6u * T, 16);
    p.x = p.work;
    p.y = p.x + plane;
    p.z = p.y + plane;
    p.r16 = p.work;
    p.inc = p.r16 + 6u * T;
    p.start = p.inc + 6u * T;
    p.label = p.work;
    return p;
}

}  // namespace mvosr
