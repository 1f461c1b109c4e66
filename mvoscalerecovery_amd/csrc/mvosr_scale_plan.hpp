// mvosr_scale_plan.hpp — the LDS layouts of the scale kernels (mvosr_kernels.hip), one plan per kernel family.
//
// A plan is a struct of named byte offsets into the workgroup's dynamic LDS plus `total`.  A kernel takes every LDS pointer
// from its plan through the family's carve function; the launcher requests `total` of the same function at the batch header's
// max_feat.  lds_plan and dense_plan are carved from the frame's own n and every offset grows with n, so a frame that passes
// the kernels' `n <= max_feat` guard lies inside the request; tiled_plan is carved at max_feat itself.
// tests/test_scale_plan.py checks that, the alignments, that regions live together do not overlap, and that the totals are
// what they were before this header existed: they decide mvosr_lds_bytes, mvosr_max_lds_features, pick_waves' 8/16 crossover
// and the tiled kernel's eligibility.  Plain C++ (<stdint.h> only): a host compiler reads it as it stands.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MVOSR_HD __host__ __device__
#else
#define MVOSR_HD
#endif

namespace mvosr {
MVOSR_HD inline uint32_t align16(uint32_t v) { return (v + 15u) & ~15u; }

// red[]: one scratch slot of 2 * waves doubles per block reduction site.  (Slots 3 and 4 are unused: the fused road model's.)
constexpr int kRedSlots = 6;
enum { R_SEL_H = 0, R_SEL_CNT = 1, R_SEL_ABS = 2, R_MISC = 5 };
// Reserved in lds_plan: the road model's 169-bin histogram when it ran inside the scale kernel.  No scale kernel touches it;
// taking it (and red's two unused slots) out moves the LDS/dense switch-over and pick_waves' crossover: to be measured first.
constexpr uint32_t kReservedBytes = 4u * 176u;

// misc[]: ints.  A slot array holds one int per wavefront of the workgroup, kMaxWaves at most.
constexpr int kMaxWaves = 16, kMiscInts = 32 /* lds_plan, dense_plan */, kTiledMiscInts = 64 /* tiled_plan */;
enum { M_WCNT = 0 /* [kMaxWaves] per-wave counts */, M_WCNT2 = 16 /* [kMaxWaves] a second per-wave array (dense_feat, tiled) */,
       M_PENDV = 40, M_PENDH = 41 /* tiled: entries in the pending votes / pending heights */ };
static_assert(M_WCNT + kMaxWaves <= M_WCNT2 && M_WCNT2 + kMaxWaves <= kMiscInts, "the per-wave arrays end inside the smallest misc");
static_assert(M_WCNT2 + kMaxWaves <= M_PENDV && M_PENDH < kTiledMiscInts, "the tiled kernel's counters lie behind them, inside its misc");

// scale_frames_kernel / outlier_vote_kernel (a frame resident in LDS), carved from the frame's n
struct LdsPlan { uint32_t p, y, c, reserved, red, misc, total; };
MVOSR_HD inline LdsPlan lds_plan(int n, int waves) {
    LdsPlan p;
    const uint32_t npad = (uint32_t)((n + 1) & ~1);
    p.p = 0;                                      // double2 {v|x, z'} per feature
    p.y = p.p + 16u * npad;                       // y' per feature
    p.c = p.y + 8u * npad;                        // 16-bit vote counter per feature; later the selected bit-set, uint32[ceil(n / 32)]
    p.reserved = align16(p.c + 2u * npad + 16u);  // kReservedBytes
    p.red = p.reserved + kReservedBytes;          // reduction scratch: 2*waves doubles per site
    p.misc = p.red + 8u * (uint32_t)(kRedSlots * 2 * waves);
    p.total = p.misc + 4u * (uint32_t)kMiscInts;
    return p;
}

// the dense kernels and outlier_vote_dense_kernel (planes in global memory: LDS keeps what is hit by atomics), carved from the frame's n
struct DensePlan { uint32_t c, sel, red, misc, total; };
MVOSR_HD inline DensePlan dense_plan(int n, int waves) {
    DensePlan p;
    const uint32_t npad = (uint32_t)((n + 1) & ~1);
    p.c = 0;                                      // 16-bit vote counter per feature
    p.sel = align16(p.c + 2u * npad + 16u);       // the selected bit-set, uint32[ceil(n / 32)]
    p.red = p.sel + align16(4u * ((uint32_t)(n + 31) / 32u));
    p.misc = p.red + 8u * (uint32_t)(kRedSlots * 2 * waves);
    p.total = p.misc + 4u * (uint32_t)kMiscInts;
    return p;
}

// scale_frames_tiled_kernel, carved from the launch header's max_feat (only the tile index depends on it)
constexpr int kTileW = 512;                 // features per tile (MVOSR_TILE_W in the header; the host's index uses the same)
constexpr int kRing = 3;                    // tiles in the LDS ring: one barrier per tile (tile k-1 retires and tile k+2 takes its slot while the
                                            // rows of tile k are still being walked)
constexpr int kPendCap = 1024;              // pending votes for vertices whose tile has not arrived yet (4 B each) ...
constexpr int kPendCapH = 576;              // ... and pending heights (12 B each): what fits two workgroups per CU
struct TiledPlan { uint32_t ringA, ringB, ringH, ringC, used, pendV, pendH, toff, red, misc, total; };
MVOSR_HD inline TiledPlan tiled_plan(int n, int waves) {
    TiledPlan p;
    const uint32_t ntiles = (uint32_t)((n + kTileW - 1) / kTileW);
    constexpr uint32_t RW = (uint32_t)kRing * kTileW;            // vertices in the ring
    p.ringA = 0;                                                 // double2 {v, z'}
    p.ringB = p.ringA + 16u * RW;                                // double2 {x, y'}
    p.ringH = p.ringB + 16u * RW;                                // uint64 key of the largest flat height
    p.ringC = p.ringH + 8u * RW;                                 // int32 vote counters
    p.used = p.ringC + 4u * RW;                                  // uint8 "a tri2 row names this vertex"
    p.pendV = align16(p.used + RW);                              // vertex << 1 | (vote is -1)
    p.pendH = p.pendV + 4u * kPendCap;                           // key64 x kPendCapH, then vertex x kPendCapH
    p.toff = align16(p.pendH + 12u * kPendCapH);                 // the frame's tile index: 2 x (ntiles + 1) ints
    p.red = align16(p.toff + 8u * (ntiles + 2u));
    p.misc = p.red + 8u * (uint32_t)(kRedSlots * 2 * waves);
    p.total = p.misc + 4u * (uint32_t)kTiledMiscInts;
    return p;
}
}  // namespace mvosr
