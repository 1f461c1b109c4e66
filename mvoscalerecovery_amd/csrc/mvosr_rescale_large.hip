// mvosr_rescale_large.hip — the rescale variant's vote and flat_selection + RANSAC for frames beyond one workgroup's LDS
// (DESIGN.md §3.23).  Same results as graph_inliers_kernel<true> and flat_selection_kernel<true> (mvosr_rescale.hip), bit for bit,
// on every frame both take: the per-row and per-hypothesis arithmetic is the shared device functions' (mvosr_device.hpp,
// mvosr_ransac.hpp), called on global arrays instead of LDS arrays, the median is an exact order statistic, and every count is
// an integer.
//
//   graph_keep_large_kernel    GraphChecker.find_inliers + rescale.py:133-137   src/graph.py:18-36 of the reference
//   flat_ransac_large_kernel   flat_selection + scale_calculation_ransac         src/rescale.py:75-102,151-167
//
// One frame per workgroup, 16 wavefronts.  LDS holds fixed-size state only (mvosr_rescale_large_plan.hpp); whatever grows with
// the frame — the survivors' planes, the rows' heights and flags, the point list — is in HBM, in the context's workspace, and
// mostly in L2 while the frame's workgroup runs.  Data one thread writes to global memory and another thread of the SAME
// workgroup reads later is separated by __syncthreads() (a workgroup-scope release / acquire: the workgroup's wavefronts share
// one CU's vector cache).  fp64, -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mvosr.h"
#include "mvosr_device.hpp"
#include "mvosr_ransac.hpp"
#include "mvosr_flat.hpp"
#include "mvosr_host.hpp"
#include "mvosr_rescale_large_plan.hpp"

namespace mvosr {

constexpr int kLgBlock = kLargeWaves * kWave;
constexpr int kLgMaxHyp = 512;
constexpr int kLgPPT = 4;               // list entries a thread holds while the hypotheses stream past (chunks of 4096 entries)
static_assert(sizeof(double4) == kPlaneBytes, "a hypothesis' plane in the LDS plan");

// ---------------------------------------------------------------------------------------------
// The vote.  The rows are swept once per vertex tile: the tile's (total, good) tallies are 32-bit LDS words, a row adds at those
// of its three vertices that lie in the tile — integer LDS atomics only — and the tile's keep words are decided behind the sweep
// as 1 / 0.  Once every tile is counted, the failed ones become -1 where more than min_valid passed (rescale.py:133-137); a
// thread patches the words it wrote itself.  {v, z} are gathered from global memory.
// ---------------------------------------------------------------------------------------------
struct GraphLargeArgs {
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *z, *v;
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    const int32_t *dt_status;
    uint32_t good_bits;
    int32_t min_valid, max_feat, tile;
    int32_t *keep, *n_valid, *status;
};

__global__ __launch_bounds__(kLgBlock) void graph_keep_large_kernel(const GraphLargeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int n = a.feat_cnt[f];
    const int tid = threadIdx.x;
    if (n <= 0) { if (tid == 0) { if (a.status) a.status[f] = MVOSR_ST_ERR_EMPTY; if (a.n_valid) a.n_valid[f] = 0; } return; }
    const int64_t off = a.feat_off[f];
    const bool declined = a.dt_status && a.dt_status[f] != 0;
    if (declined || n > a.max_feat) {
        // a declined first triangulation, or more features than the header states: what the resident kernel does with either
        for (int i = tid; i < n; i += kLgBlock) a.keep[off + i] = -1;
        if (tid == 0) { if (a.status) a.status[f] = declined ? MVOSR_ST_ERR_EMPTY : MVOSR_ST_ERR_MASK; if (a.n_valid) a.n_valid[f] = 0; }
        return;
    }
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    const int T = a.tile;
    const auto lds = graph_large_plan<uint32_t>((uint32_t)T);
    int *tot = reinterpret_cast<int *>(smem + lds.total_cnt);
    int *god = reinterpret_cast<int *>(smem + lds.good_cnt);
    int *flag = reinterpret_cast<int *>(smem + lds.flag);                 // [0] bad vertex id, [1] features that passed
    const double *V = a.v + off, *Z = a.z + off;
    const int32_t *rows = a.tri + 3 * tb;
    int32_t *keep = a.keep + off;
    if (tid < 2) flag[tid] = 0;
    int mine = 0, bad = 0;
    for (int lo = 0; lo < n; lo += T) {
        const int cnt = min(T, n - lo);
        for (int j = tid; j < cnt; j += kLgBlock) { tot[j] = 0; god[j] = 0; }
        __syncthreads();
        for (int t = tid; t < tn; t += kLgBlock) {
            const TriIds q = load_tri(rows, t);
            if (!ids_in_range(q.a, q.b, q.c, n)) { bad = 1; continue; }  // (the whole row is left out, in every tile)
            const bool ia = (unsigned)(q.a - lo) < (unsigned)cnt, ib = (unsigned)(q.b - lo) < (unsigned)cnt, ic = (unsigned)(q.c - lo) < (unsigned)cnt;
            if (!(ia || ib || ic)) continue;
            const double v0 = V[q.a], z0 = Z[q.a], v1 = V[q.b], z1 = Z[q.b], v2 = V[q.c], z2 = Z[q.c];
            const int ca = (v0 - v1) * (z0 - z1) < 0.0;                   // graph.py:125
            const int cb = (v1 - v2) * (z1 - z2) < 0.0;                   // graph.py:126
            const int cc = (v0 - v2) * (z0 - z2) < 0.0;                   // graph.py:127
            const uint32_t g = a.good_bits >> (3 * (ca * 4 + cb * 2 + cc));   // graph.py:128,140-145
            if (ia) { atomicAdd(&tot[q.a - lo], 1); if (g & 1u) atomicAdd(&god[q.a - lo], 1); }          // graph.py:28-30
            if (ib) { atomicAdd(&tot[q.b - lo], 1); if ((g >> 1) & 1u) atomicAdd(&god[q.b - lo], 1); }
            if (ic) { atomicAdd(&tot[q.c - lo], 1); if ((g >> 2) & 1u) atomicAdd(&god[q.c - lo], 1); }
        }
        __syncthreads();
        // good/total > 0.5 (graph.py:34-35,131-132) in integers: 2*good > total; 0/0 is nan: dropped
        for (int j = tid; j < cnt; j += kLgBlock) {
            const int pass = (2u * (uint32_t)god[j] > (uint32_t)tot[j]) ? 1 : 0;
            keep[lo + j] = pass;
            mine += pass;
        }
        __syncthreads();                                                  // (the tallies are zeroed again at the top)
    }
    mine = wave_sum(mine);
    if (lane_id() == 0 && mine) atomicAdd(&flag[1], mine);
    if (bad) flag[0] = 1;
    __syncthreads();
    const int nv = flag[1];
    if (nv > a.min_valid) {                                               // rescale.py:133-137: ten or fewer left — the frame stays whole
        for (int lo = 0; lo < n; lo += T) {
            const int cnt = min(T, n - lo);
            for (int j = tid; j < cnt; j += kLgBlock) if (keep[lo + j] == 0) keep[lo + j] = -1;   // (this thread's own words)
        }
    }
    if (tid == 0) { if (a.n_valid) a.n_valid[f] = nv; if (a.status) a.status[f] = flag[0] ? MVOSR_ST_ERR_MASK : 0; }
}

// ---------------------------------------------------------------------------------------------
// flat_selection + the RANSAC plane fit.  The phases are flat_selection_kernel<true>'s, and so is each phase's rule: both kernels
// call mvosr_flat.hpp (this one the level's search in its ROLLED form).  The frame-sized arrays are global:
//   X, Y, Z   the survivors, compacted in order into the workspace (keep == NULL: the batch's own planes, read in place)
//   Hh, Fl    every row's height and flags: the caller's tri_height / tri_flags where given, else the workspace
//   L         the point list: int32 vertex ids of the kept rows in row order (M = 3 K entries; M may exceed 65 535)
// ---------------------------------------------------------------------------------------------
struct FlatLargeArgs {
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *x, *y, *z;
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    const int32_t *keep, *dt_status, *id_triples;
    const int64_t *frame_ids;
    double loose_deg, tight_deg, height_factor;
    int32_t n_hyp, ransac_min_points, max_feat, max_tri;
    double threshold, goal_fraction, absolute_reference;
    uint64_t seed; int64_t frame_base;
    double *tri_height; uint8_t *tri_flags;
    double *height_level, *raw_scale, *model;
    int32_t *status, *n_kept, *best_ic, *used, *hyp_counts;
    // the workspace (null where not needed)
    double *wx, *wy, *wz, *wh;
    uint8_t *wf;
    int32_t *wl;
};

// The members of the argument block that a frame needs once — the per-frame outputs' pointers, the sample inputs, the RANSAC's
// scalars — are read from the kernel's argument block where they are used (scalar loads from the constant address space; the
// block is the kernel's only argument, at offset 0): loaded at the kernel's entry, as `a.member` is, they occupied scalar
// registers through every phase and were spilled.
#if defined(__HIP_DEVICE_COMPILE__)
#define LG_LATE(member) (((const __attribute__((address_space(4))) FlatLargeArgs *)__builtin_amdgcn_kernarg_segment_ptr())->member)
#else
#define LG_LATE(member) (a.member)
#endif

__global__ __launch_bounds__(kLgBlock) void flat_ransac_large_kernel(const FlatLargeArgs a) {
    constexpr int BLK = kLgBlock, WAVES = kLargeWaves;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int n_all = a.feat_cnt[f];
    const int64_t off = a.feat_off[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const bool skip = a.dt_status && a.dt_status[f] != 0;
    // more features or rows than the header's max_feat / the call's max_tri (the workspace's row stride): refused, nothing touched
    const bool oversize = n_all > a.max_feat || tn > a.max_tri;
    if (const int refused = flat_entry_status(n_all, tn, skip, oversize)) {
        if (tid == 0) {
            LG_LATE(status)[f] = refused;
            LG_LATE(height_level)[f] = nan(""); LG_LATE(n_kept)[f] = 0;
            LG_LATE(raw_scale)[f] = nan(""); LG_LATE(best_ic)[f] = 0; LG_LATE(used)[f] = 0;
            for (int k = 0; k < 4; ++k) LG_LATE(model)[4 * f + k] = nan("");
        }
        return;
    }
    const auto lds = flat_large_plan<uint32_t>((uint32_t)a.n_hyp);
    unsigned long long *ext = reinterpret_cast<unsigned long long *>(smem + lds.ext);
    int *misc = reinterpret_cast<int *>(smem + lds.misc);
    int *hist = reinterpret_cast<int *>(smem + lds.hist);
    double4 *mods = reinterpret_cast<double4 *>(smem + lds.mods);
    int *cnts = reinterpret_cast<int *>(smem + lds.cnts);
    const int64_t rbase = f * (int64_t)a.max_tri;
    double *Hh = a.tri_height ? a.tri_height + tb : a.wh + rbase;
    uint8_t *Fl = a.tri_flags ? a.tri_flags + tb : a.wf + rbase;
    int32_t *L = a.wl + 3 * rbase;
    const int32_t *rows = a.tri + 3 * tb;
    flat_state_init(misc, ext);
    // ---- ordered compaction of the survivors (rescale.py:134-135: feature3d[valid_id])
    int n = n_all;
    const double *X = a.x + off, *Y = a.y + off, *Z = a.z + off;
    if (a.keep) {
        double *CX = a.wx + off, *CY = a.wy + off, *CZ = a.wz + off;
        n = flat_compact_survivors<WAVES>(n_all, a.keep + off, X, Y, Z, CX, CY, CZ, misc + FM_CW);
        X = CX; Y = CY; Z = CZ;
    }
    const double s_loose = flat_sin_deg(a.loose_deg), s_tight = flat_sin_deg(a.tight_deg);
    __syncthreads();
    // ---- phase 1: every row's height and flags, the loose ones counted and bounded
    {
        FlatLoose tally;
        for (int t = tid; t < tn; t += BLK) {
            const FlatRow r = flat_row(X, Y, Z, load_tri(rows, t), n);
            if (r.bad_id) misc[FM_BADID] = 1;
            if (r.singular) misc[FM_SINGULAR] = 1;
            const unsigned bits = r.bad_id ? 0u : flat_row_bits(r.mu, s_loose, s_tight, a.loose_deg, a.tight_deg);
            Hh[t] = r.h;
            Fl[t] = (uint8_t)bits;
            if (bits & 1u) tally.add(r.h);
        }
        tally.commit(misc, ext);
    }
    __syncthreads();
    const int k = misc[FM_K];
    // (the heights are read from global memory on every pass of the search)
    const double level = flat_level_search<WAVES, true>(reinterpret_cast<const unsigned long long *>(Hh), Fl, tn, k, ext, misc, hist,
                                                        a.height_factor).level;               // np.median, :91
    // ---- the kept rows (:94-96), wavefront by wavefront over contiguous row segments: the point list comes out in row order
    int s0, s1;
    ordered_segment(tn, BLK, s0, s1);
    int c = 0;
    for (int t0 = s0; t0 < s1; t0 += kWave) {
        const int t = t0 + lane;
        bool kp = false;
        if (t < s1) {
            uint8_t fl = Fl[t];
            kp = (fl & 2) && Hh[t] > level;
            if (kp) { fl |= 4; Fl[t] = fl; }
        }
        c += __popcll(__ballot(kp));
    }
    int base, K;
    ordered_prefix<WAVES>(misc + FM_CW, c, base, K);
    const int M = 3 * K;                                         // len(point_selected), :140
    const int H = a.n_hyp;
    const bool bad = misc[FM_BADID] || misc[FM_SINGULAR];
    const bool fit = !bad && M >= LG_LATE(ransac_min_points);           // :152
    if (fit) {
        for (int t0 = s0; t0 < s1; t0 += kWave) {
            const int t = t0 + lane;
            const bool kp = t < s1 && (Fl[t] & 4);               // (the flag this very thread wrote above)
            const int pos = 3 * ordered_rank(kp, base);
            if (kp) {
                const TriIds q = load_tri(rows, t);
                L[pos] = q.a; L[pos + 1] = q.b; L[pos + 2] = q.c;
            }
        }
        __syncthreads();
        // the hypotheses' planes, one thread each (ransac.py:10-11, estimate_road_norm.py:13-15)
        const uint64_t key = ransac_frame_key(LG_LATE(seed), (uint64_t)(LG_LATE(frame_ids) ? LG_LATE(frame_ids)[f] : LG_LATE(frame_base) + f));
        flat_build_hypotheses<BLK>(key, LG_LATE(id_triples) ? LG_LATE(id_triples) + (int64_t)f * H * 3 : nullptr, H, n, M, L, X, Y, Z, mods, cnts);
        __syncthreads();
        // inlier counts over the list as it is, repeats included (estimate_road_norm.py:17-18): a thread's list entries in registers,
        // their coordinates gathered by id once, the hypotheses streamed past them from LDS (mvosr_ransac.hpp)
        ransac_count_resident<false, kLgPPT, 1, BLK>(M, mods, cnts, H, LG_LATE(threshold),
            [&](int j, double &px, double &py, double &pz) { const int id = L[j]; px = X[id]; py = Y[id]; pz = Z[id]; });
        __syncthreads();
        if (LG_LATE(hyp_counts)) for (int h = tid; h < H; h += BLK) LG_LATE(hyp_counts)[(int64_t)f * H + h] = cnts[h];
    }
    if (wave == 0) {
        const int status = misc[FM_BADID] ? MVOSR_ST_ERR_MASK : (misc[FM_SINGULAR] ? MVOSR_ST_ERR_SINGULAR : (fit ? 0 : MVOSR_ST_RS_FEW));
        const FlatRansacResult r = flat_ransac_result(fit, status, mods, cnts, H, (double)M * LG_LATE(goal_fraction), LG_LATE(absolute_reference));
        if (lane == 0) {
            LG_LATE(height_level)[f] = level;
            LG_LATE(n_kept)[f] = K;
            LG_LATE(status)[f] = r.status;
            LG_LATE(raw_scale)[f] = r.raw;
            LG_LATE(best_ic)[f] = r.best_ic; LG_LATE(used)[f] = r.used;
            for (int kk = 0; kk < 4; ++kk) LG_LATE(model)[4 * f + kk] = r.m[kk];
        }
    }
}

template <typename Args>
static int lg_launch(mvosr_ctx *ctx, void (*kernel)(Args), const char *name, int64_t n_frames, size_t lds, const Args &a) {
    if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_ARG, "%s needs %zu B of LDS (> %d)", name, lds, ctx->max_lds_per_block);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_frames), dim3(kLgBlock), lds, ctx_stream(ctx), a);
    return check_launch(name);
}

}  // namespace mvosr

using namespace mvosr;

extern "C" {

int mvosr_graph_keep_large_batch(mvosr_ctx *ctx, const mvosr_batch *b, uint32_t good_bits, int32_t min_valid, const int32_t *dt_status,
                                 int32_t *keep, int32_t *n_valid, int32_t *status, int32_t tile) {
    if (!ctx || !b || !keep) return set_error(MVOSR_ERR_ARG, "graph_keep_large: null argument");
    if (!b->feat_off || !b->feat_cnt || !b->z || !b->v || !b->tri1_off || !b->tri1) return set_error(MVOSR_ERR_ARG, "graph_keep_large: missing z/v/tri1");
    if (b->n_frames <= 0) return MVOSR_OK;
    if (b->n_frames > INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "graph_keep_large: n_frames does not fit 32 bits");
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    GraphLargeArgs a = {};
    a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.z = b->z; a.v = b->v;
    a.tri_off = b->tri1_off; a.tri = b->tri1; a.tri_cnt = b->tri1_cnt; a.dt_status = dt_status;
    a.good_bits = good_bits; a.min_valid = min_valid; a.max_feat = b->max_feat;
    a.tile = graph_large_tile<int32_t>(tile, b->max_feat);
    a.keep = keep; a.n_valid = n_valid; a.status = status;
    return lg_launch(ctx, graph_keep_large_kernel, "graph_keep_large_kernel", b->n_frames, graph_large_plan<size_t>((size_t)a.tile).total, a);
}

int mvosr_flat_ransac_large_batch(mvosr_ctx *ctx, const mvosr_batch *b, const int32_t *keep, const mvosr_rescale_params *rp,
                                  const int32_t *id_triples, const int64_t *frame_ids, const int32_t *dt_status,
                                  const mvosr_rescale_outputs *o, int64_t max_tri) {
    if (!ctx || !b || !rp || !o) return set_error(MVOSR_ERR_ARG, "flat_ransac_large: null argument");
    if (!o->raw_scale || !o->height_level || !o->model || !o->best_ic || !o->used || !o->n_kept || !o->status)
        return set_error(MVOSR_ERR_ARG, "flat_ransac_large: a required output is null");
    if (!b->feat_off || !b->feat_cnt || !b->x || !b->y || !b->z || !b->tri2_off || !b->tri2) return set_error(MVOSR_ERR_ARG, "flat_ransac_large: missing x/y/z/tri2");
    if (rp->n_hyp < 1 || rp->n_hyp > kLgMaxHyp) return set_error(MVOSR_ERR_ARG, "flat_ransac_large: n_hyp must be in 1..%d", kLgMaxHyp);
    if (rp->ransac_min_points < 3) return set_error(MVOSR_ERR_ARG, "flat_ransac_large: ransac_min_points < 3");
    if (b->n_frames <= 0) return MVOSR_OK;
    if (b->max_feat < 0 || b->total_feat < 0) return set_error(MVOSR_ERR_ARG, "flat_ransac_large: max_feat / total_feat < 0");
    if (max_tri <= 0) max_tri = 2 * (int64_t)b->max_feat;
    if (max_tri < 1) max_tri = 1;
    // the point list's positions (3 per kept row) are ints
    if (3 * max_tri > INT32_MAX || b->n_frames > INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "flat_ransac_large: 3 * max_tri does not fit 32 bits");
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    const FlatLargeWs w = flat_large_ws((size_t)b->n_frames, (size_t)b->total_feat, (size_t)max_tri, keep != nullptr, !o->tri_height, !o->tri_flags);
    void *ws = nullptr;
    if ((rc = ctx_workspace_bytes(ctx, w.total, &ws))) return rc;
    char *base = static_cast<char *>(ws);
    FlatLargeArgs a = {};
    a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.x = b->x; a.y = b->y; a.z = b->z;
    a.tri_off = b->tri2_off; a.tri = b->tri2; a.tri_cnt = b->tri2_cnt;
    a.keep = keep; a.dt_status = dt_status; a.id_triples = id_triples; a.frame_ids = frame_ids;
    a.loose_deg = rp->loose_deg; a.tight_deg = rp->tight_deg; a.height_factor = rp->height_factor;
    a.n_hyp = rp->n_hyp; a.ransac_min_points = rp->ransac_min_points; a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri;
    a.threshold = rp->threshold; a.goal_fraction = rp->goal_fraction; a.absolute_reference = rp->absolute_reference;
    a.seed = rp->seed; a.frame_base = rp->frame_base;
    a.tri_height = o->tri_height; a.tri_flags = o->tri_flags; a.height_level = o->height_level; a.raw_scale = o->raw_scale; a.model = o->model;
    a.status = o->status; a.n_kept = o->n_kept; a.best_ic = o->best_ic; a.used = o->used; a.hyp_counts = o->hyp_counts;
    if (keep) { a.wx = reinterpret_cast<double *>(base + w.x); a.wy = reinterpret_cast<double *>(base + w.y); a.wz = reinterpret_cast<double *>(base + w.z); }
    if (!o->tri_height) a.wh = reinterpret_cast<double *>(base + w.heights);
    if (!o->tri_flags) a.wf = reinterpret_cast<uint8_t *>(base + w.flags);
    a.wl = reinterpret_cast<int32_t *>(base + w.list);
    return lg_launch(ctx, flat_ransac_large_kernel, "flat_ransac_large_kernel", b->n_frames, flat_large_plan<size_t>((size_t)rp->n_hyp).total, a);
}

}  // extern "C"
