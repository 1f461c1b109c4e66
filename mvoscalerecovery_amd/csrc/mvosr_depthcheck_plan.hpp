// mvosr_depthcheck_plan.hpp — the shape of depthcheck_kernel (mvosr_depthcheck.hip) and the bin of a slope, shared by the kernel,
// its launcher and the host: the binning is plain arithmetic on one double and is tested on the host as it stands.
//
// A frame's n x n pairs are cut into ROW BLOCKS of kDcRows points (the i side: one point per thread, in registers) and J TILES of
// kDcTile points (the j side: z, y / z and the level of a tile in LDS, read by every lane at the same address).  A workgroup owns
// one row block and every j_split-th tile; the launcher picks j_split so that a launch of few frames still fills the device.
// Nothing of a frame is resident: n is bounded by the grid alone.
//
// A pair's result goes to one of kDcSlots words — the 59 bins of np.histogram(q, np.array(range(-40, 20)) * 50), then below,
// above, nan — of the level min(level_i, level_j); population p is the levels >= p, summed when the workgroup flushes.  The LDS
// histogram is kept in kDcCopies copies, a lane adds to copy (lane % kDcCopies) with the copy index fastest: the lanes of a
// wavefront that meet in one bin spread over kDcCopies banks, two lanes a word.
//
// Plain C++ (<stdint.h> / <stddef.h> only): a host compiler reads it as it stands.
#pragma once

#include "mvosr_rescale_plan.hpp"

namespace mvosr {

constexpr int kDcPops = 3;                    // every feature below the vanishing row; kept by the vote; selected as road
constexpr int kDcBins = 59;                   // MVOSR_DC_BINS: edges 50 * (k - 40), k = 0 .. 59
constexpr int kDcBelow = kDcBins;             // q < -2000 (-inf too)
constexpr int kDcAbove = kDcBins + 1;         // q > 950 (+inf too)
constexpr int kDcNan = kDcBins + 2;           // q is NaN
constexpr int kDcSlots = kDcBins + 3;         // MVOSR_DC_TABLE_WORDS
constexpr int kDcRows = 256;                  // the row block: one i per thread
constexpr int kDcTile = 512;                  // the j tile in LDS
constexpr int kDcCopies = 32;                 // copies of the LDS histogram, striped over the lanes
constexpr int kDcMaxSplit = 64;               // at most this many workgroups share a row block's tiles
constexpr int kDcLdsBytes = kDcTile * (8 + 8 + 4) + kDcPops * kDcSlots * kDcCopies * 4 + 16;   // the tile, the histogram, the tile's fill count
static_assert(kDcLdsBytes <= 40 * 1024, "four workgroups a CU");

// the lower edge of bin k: an integer, exact in a double
MVOSR_HD inline constexpr double depthcheck_edge(int k) { return 50.0 * (double)(k - 40); }

// The slot of a slope.  Bin k holds edge(k) <= q < edge(k + 1), bin 58 also q == 950; -0.0 compares equal to 0 and lands in bin 40.
// The scaled floor may be one off next to an edge (q + 2000 and the product are rounded), so the edges themselves decide.
// Written without branches: every lane of a wavefront takes the same path whatever its slope.
MVOSR_HD inline int depthcheck_slot(double q) {
    double s = (q + 2000.0) * 0.02;
    s = s >= 0.0 ? s : 0.0;                                       // (NaN and what lies below: any bin, replaced at the end)
    s = s <= (double)(kDcBins - 1) ? s : (double)(kDcBins - 1);
    int k = (int)s;
    const double lo = depthcheck_edge(k);
    k += (int)(k < kDcBins - 1 && q >= lo + 50.0) - (int)(q < lo);
    k = q < depthcheck_edge(0) ? kDcBelow : k;
    k = q > depthcheck_edge(kDcBins) ? kDcAbove : k;
    k = q != q ? kDcNan : k;
    return k;
}

// how a launch is cut: row blocks of the largest frame, and how many workgroups share a row block's tiles — enough for some
// workgroups per CU where the frames alone do not give them, never more than there are tiles
struct DepthCheckGrid { int64_t row_blocks, tiles, j_split; };
MVOSR_HD inline constexpr DepthCheckGrid depthcheck_grid(int64_t n_frames, int64_t max_feat, int64_t n_cu) {
    DepthCheckGrid g{};
    g.row_blocks = (max_feat + kDcRows - 1) / kDcRows;
    g.tiles = (max_feat + kDcTile - 1) / kDcTile;
    const int64_t have = n_frames * g.row_blocks, want = 4 * n_cu;
    int64_t s = have > 0 ? (want + have - 1) / have : 1;
    if (s > g.tiles) s = g.tiles;
    if (s > kDcMaxSplit) s = kDcMaxSplit;
    if (s < 1) s = 1;
    g.j_split = s;
    return g;
}

}  // namespace mvosr
