// mvosr_rescale_large_plan.hpp — the LDS layouts and the workspace layout of the rescale variant's kernels for frames beyond
// the LDS limit (mvosr_rescale_large.hip).  Same conventions as mvosr_rescale_plan.hpp: a plan is a struct of named byte
// offsets plus `total`, evaluated by the kernel and by its launcher alike.
//
// Nothing here grows with a frame: the LDS plans depend on the vote's tile and on n_hyp only.  What grows with a frame lives in
// the context's workspace (FlatLargeWs below), in HBM.
//
// Plain C++ (<stdint.h> / <stddef.h> only): a host compiler reads it as it stands.
#pragma once

#include "mvosr_rescale_plan.hpp"

namespace mvosr {

constexpr int kLargeWaves = 16;                 // wavefronts of a workgroup, both kernels
constexpr int kGraphLargeMaxTile = 8192;        // vertices whose tallies one sweep over the rows holds in LDS (64 KiB), at most

// graph_keep_large_kernel, carved from the launch's tile
template <typename U> struct GraphLargePlan {
    U total_cnt;    // int32[tile] incident rows of the tile's vertices
    U good_cnt;     // int32[tile] rows that vouch for them
    U flag;         // int[4] bad vertex id, features that passed (in 16 bytes)
    U total;
};
template <typename U> MVOSR_HD inline GraphLargePlan<U> graph_large_plan(U tile) {
    GraphLargePlan<U> p;
    p.total_cnt = 0;
    p.good_cnt = p.total_cnt + 4u * tile;
    p.flag = plan_align<U>(p.good_cnt + 4u * tile, 16);
    p.total = p.flag + 16;
    return p;
}
// the launcher's tile: the caller's, or one tile for a frame of up to kGraphLargeMaxTile features; never above that
template <typename U> MVOSR_HD inline U graph_large_tile(U asked, U max_feat) {
    U t = asked > 0 ? asked : (max_feat > 64 ? max_feat : (U)64);
    return t > (U)kGraphLargeMaxTile ? (U)kGraphLargeMaxTile : t;
}

// flat_ransac_large_kernel: fixed-size state only.  The hypotheses' planes are double4 here (ransac_count_resident streams them).
template <typename U> struct FlatLargePlan {
    U ext;          // uint64[4] smallest / largest loose height (bits), smallest above the median, the ranked candidate
    U misc;         // int[FM_N]
    U hist;         // int[kFlatBins]; later the short candidate list, uint64[kFlatDirect]
    U mods;         // [n_hyp] unit (n, d), kPlaneBytes each, 32-aligned
    U cnts;         // int[n_hyp] inlier counts
    U total;
};
template <typename U> MVOSR_HD inline FlatLargePlan<U> flat_large_plan(U n_hyp) {
    FlatLargePlan<U> p;
    p.ext = 0;
    p.misc = p.ext + 4 * 8;
    p.hist = p.misc + 4u * FM_N;
    p.mods = plan_align<U>(p.hist + 4u * kFlatBins, 32);
    p.cnts = p.mods + kPlaneBytes * n_hyp;
    p.total = plan_align<U>(p.cnts + 4u * n_hyp, 16);
    return p;
}

// flat_ransac_large_kernel's share of the context's workspace, in bytes from its start.  The survivors' planes are indexed like
// the batch's own planes (feat_off[f] + rank: a frame's survivors are no more than its features).  The row arrays are indexed
// f * max_tri + row: the launcher knows max_tri, not the rows' total (tri2_off lives in device memory).  Heights and flags have
// room here only where the caller gave no tri_height / tri_flags (with_heights / with_flags).
struct FlatLargeWs {
    size_t x, y, z;     // double[total_feat] each: the survivors, compacted in order (not used where keep == NULL)
    size_t heights;     // double[n_frames * max_tri]
    size_t list;        // int32[n_frames * 3 * max_tri] the point list: vertex ids of the kept rows, in row order
    size_t flags;       // uint8[n_frames * max_tri]
    size_t total;
};
inline FlatLargeWs flat_large_ws(size_t n_frames, size_t total_feat, size_t max_tri, bool with_planes, bool with_heights, bool with_flags) {
    FlatLargeWs w;
    const size_t plane = with_planes ? 8 * plan_even<size_t>(total_feat) : 0;
    const size_t rows = n_frames * max_tri;
    w.x = 0;
    w.y = w.x + plane;
    w.z = w.y + plane;
    w.heights = w.z + plane;
    w.list = w.heights + (with_heights ? 8 * rows : 0);
    w.flags = w.list + 12 * rows;
    w.total = plan_align<size_t>(w.flags + (with_flags ? rows : 0), 256) + 256;
    return w;
}

}  // namespace mvosr
