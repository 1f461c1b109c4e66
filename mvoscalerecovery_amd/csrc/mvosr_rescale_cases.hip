// mvosr_rescale_cases.hip — C runs of a sequence at once for the `rescale` variant's device-resident RANSAC.
//
// The reference's RANSAC is unseeded (/root/reference/src/thirdparty/Ransac/ransac.py:6), so its author runs the same saved
// sequence ten times (/root/reference/test_off_line.sh:4-16) and averages the scores.  Both triangulations, the vote and
// flat_selection are the same in every run (/root/reference/src/rescale.py:113-148); only get_pitch_ransac's sample sequence
// (:155) differs.  flat_ransac_cases_kernel runs after ONE launch of flat_selection_kernel<true> (mvosr_flat_ransac_batch, asked
// for tri_flags) and does the plane fit of all cases of a frame, one workgroup per (frame, group of cases):
//
//   once per workgroup: the survivors' x / y / z compacted by keep >= 0 in order — as flat_selection_kernel<true> numbers them —,
//   the point list from the rows whose flag has bit 2 (kept), in row order, three ids each, repeats included (rescale.py:101),
//   and the counting form: the list's distinct vertices with their multiplicities;
//   per case: the hypotheses from ransac_draw3 keyed by the CASE's seed, their counts, the replay rule, the sign rule and the raw
//   scale (rescale.py:156-167) — flat_build_hypotheses and flat_ransac_result (mvosr_flat.hpp), which flat_selection_kernel<true>'s
//   tail calls as well, so that case c equals, bit for bit, what mvosr_flat_ransac_batch returns with rp->seed = case_seeds[c].
//
// fp64, compiled with -ffp-contract=off.  The counts are integer sums: they depend neither on the counting form nor on the order
// in which the distinct vertices were appended.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mvosr.h"
#include "mvosr_device.hpp"
#include "mvosr_ransac.hpp"
#include "mvosr_flat.hpp"
#include "mvosr_host.hpp"
#include "mvosr_rescale_cases_plan.hpp"

namespace mvosr {

constexpr int kCasesWaves = 16;         // the frame holds most of a CU's LDS — one workgroup per CU —, so the workgroup brings its own occupancy
// cases_per_group where the caller passes 0.  Measured (profiles/repeats_bench.json, 512 resident 2000-feature frames x 10 cases, this
// launch alone): G = 1 0.487 ms, 2 0.388, 5 0.317, 10 0.311 — the per-workgroup set-up (the frame's load, the list, the multiplicities)
// outweighs the narrower grid; ten launches of the single-run kernel take 0.791 ms
constexpr int kCasesDefaultGroup = 10;

struct CasesArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *x, *y, *z;
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    const int32_t *keep;           // [like x] a feature takes part iff keep[i] >= 0 (null: all)
    const int32_t *dt_status;      // [F] non-zero: declined triangulation, frame skipped (null: none)
    const uint8_t *tri_flags;      // [rows of tri2] bit 2: kept (what flat_selection_kernel<true> wrote)
    const int32_t *id_triples;     // [F][C][H][3] survivor-numbered vertex ids replacing the draw (null: draw)
    const int64_t *frame_ids;      // [F] sample-sequence counter of the frame (null: frame_base + f)
    const uint64_t *case_seeds;    // [C]
    int32_t n_hyp, ransac_min_points, max_feat, max_tri, n_cases, cases_per_group, n_groups;
    double threshold, goal_fraction, absolute_reference;
    int64_t frame_base;
    double *raw_scale, *model;     // [F][C], [F][C][4]
    int32_t *best_ic, *used, *status;   // [F][C]
    int32_t *hyp_counts;           // optional [F][C][H]
    int32_t *count_form;           // optional [F]
};

// every case of this workgroup's group is not fitted: NaN doubles, zero counts
__device__ __forceinline__ void cases_refuse(const CasesArgs &a, int64_t f, int g, int c_lo, int c_hi, int status) {
    for (int c = c_lo + (int)threadIdx.x; c < c_hi; c += (int)blockDim.x) {
        const int64_t fc = f * a.n_cases + c;
        a.raw_scale[fc] = nan(""); a.best_ic[fc] = 0; a.used[fc] = 0; a.status[fc] = status;
        for (int k = 0; k < 4; ++k) a.model[4 * fc + k] = nan("");
    }
    if (g == 0 && threadIdx.x == 0 && a.count_form) a.count_form[f] = MVOSR_CASES_FORM_NONE;
}

template <int WAVES>
__global__ __launch_bounds__(WAVES *kWave) void flat_ransac_cases_kernel(const CasesArgs a) {
    constexpr int BLK = WAVES * kWave;
    constexpr int kPackRegs = (kCasesPackMax + BLK - 1) / BLK;       // packed items a thread carries over the barrier
    static_assert(WAVES <= 16, "flat_ransac_cases_kernel: per-wave slots in misc");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x / (unsigned)a.n_groups;
    const int g = (int)(blockIdx.x % (unsigned)a.n_groups);
    const int C = a.n_cases, c_lo = g * a.cases_per_group, c_hi = min(C, c_lo + a.cases_per_group);
    const int n_all = a.feat_cnt[f];
    const int64_t off = a.feat_off[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const bool skip = a.dt_status && a.dt_status[f] != 0;
    // more features or rows than the launch's LDS was sized for: refused, LDS untouched
    const bool oversize = n_all > a.max_feat || tn > a.max_tri;
    if (const int refused = flat_entry_status(n_all, tn, skip, oversize)) {
        cases_refuse(a, f, g, c_lo, c_hi, refused);
        return;
    }
    const int H = a.n_hyp;
    const auto lds = cases_plan<uint32_t>((uint32_t)n_all, (uint32_t)tn, (uint32_t)H);
    double *X = reinterpret_cast<double *>(smem + lds.x);
    double *Y = reinterpret_cast<double *>(smem + lds.y);
    double *Z = reinterpret_cast<double *>(smem + lds.z);
    uint16_t *L = reinterpret_cast<uint16_t *>(smem + lds.list);
    int *W = reinterpret_cast<int *>(smem + lds.w);
    uint16_t *Dv = reinterpret_cast<uint16_t *>(smem + lds.dv);
    double2 *mods = reinterpret_cast<double2 *>(smem + lds.mods);
    int *cnts = reinterpret_cast<int *>(smem + lds.cnts);
    int *misc = reinterpret_cast<int *>(smem + lds.misc);
    if (tid < CM_CW) misc[tid] = 0;

    // ---- the survivors, compacted in order (rescale.py:134-135)
    const int n = flat_compact_survivors<WAVES>(n_all, a.keep ? a.keep + off : nullptr, a.x + off, a.y + off, a.z + off, X, Y, Z, misc + CM_CW);
    // ---- the kept rows, in row order (rescale.py:94-96, :101): the same segmented compaction over the flags
    for (int v = tid; v < n_all; v += BLK) W[v] = 0;
    int t0w, t1w;
    ordered_segment(tn, BLK, t0w, t1w);
    int base, K;
    {
        int c = 0;
        for (int t0 = t0w; t0 < t1w; t0 += kWave) {
            const int t = t0 + lane;
            c += __popcll(__ballot(t < t1w && (a.tri_flags[tb + t] & 4)));
        }
        ordered_prefix<WAVES>(misc + CM_CW2, c, base, K);
    }
    const int M = 3 * K;                                             // len(point_selected), rescale.py:140
    {
        int bad = 0;
        for (int t0 = t0w; t0 < t1w; t0 += kWave) {
            const int t = t0 + lane;
            const bool kp = t < t1w && (a.tri_flags[tb + t] & 4);
            const int pos = 3 * ordered_rank(kp, base);
            if (kp) {
                TriIds q = load_tri(a.tri + 3 * tb, t);
                if (!ids_in_range(q.a, q.b, q.c, n)) { bad = 1; q.a = q.b = q.c = 0; }
                L[pos] = (uint16_t)q.a; L[pos + 1] = (uint16_t)q.b; L[pos + 2] = (uint16_t)q.c;
            }
        }
        if (bad) misc[CM_BAD] = 1;
    }
    __syncthreads();
    if (misc[CM_BAD] || M < a.ransac_min_points) {                   // a kept row names a vertex that is no survivor / rescale.py:152
        cases_refuse(a, f, g, c_lo, c_hi, misc[CM_BAD] ? MVOSR_ST_ERR_MASK : MVOSR_ST_RS_FEW);
        return;
    }
    // ---- the counting form (estimate_road_norm.py:17-18 runs over every list entry, repeats included): the list names each of
    // its distinct vertices once per kept triangle, so a vertex is tested once per hypothesis and counts with its multiplicity
    for (int j = tid; j < M; j += BLK) atomicAdd(&W[L[j]], 1);
    __syncthreads();
    for (int v = tid; v < n; v += BLK) if (W[v]) Dv[atomicAdd(&misc[CM_ND], 1)] = (uint16_t)v;
    __syncthreads();
    const int n_items = misc[CM_ND];
    // ... and, with few enough of them, their coordinates and multiplicities side by side over the same room: the counting loop
    // then reads four contiguous arrays instead of gathering by id
    const bool packed = n_items <= kCasesPackMax;
    double *PX = reinterpret_cast<double *>(smem + lds.px), *PY = PX + n_items, *PZ = PY + n_items;
    int *PW = reinterpret_cast<int *>(PZ + n_items);
    if (packed) {
        double gx[kPackRegs], gy[kPackRegs], gz[kPackRegs];
        int gw[kPackRegs];
#pragma unroll
        for (int r = 0; r < kPackRegs; ++r) {
            const int j = tid + r * BLK;
            const int id = Dv[min(j, n_items - 1)];
            gx[r] = X[id]; gy[r] = Y[id]; gz[r] = Z[id]; gw[r] = W[id];
        }
        __syncthreads();                                             // (the ids and multiplicities have been read: their room is the arrays')
#pragma unroll
        for (int r = 0; r < kPackRegs; ++r) {
            const int j = tid + r * BLK;
            if (j < n_items) { PX[j] = gx[r]; PY[j] = gy[r]; PZ[j] = gz[r]; PW[j] = gw[r]; }
        }
    }
    if (g == 0 && tid == 0 && a.count_form) a.count_form[f] = packed ? MVOSR_CASES_FORM_PACKED : MVOSR_CASES_FORM_GATHER;
    __syncthreads();

    const uint64_t fcnt = (uint64_t)(a.frame_ids ? a.frame_ids[f] : a.frame_base + f);
    const double goal = (double)M * a.goal_fraction;                 // estimate_road_norm.py:68
    for (int c = c_lo; c < c_hi; ++c) {
        const int64_t fc = f * C + c;
        // the hypotheses' planes, one thread each (ransac.py:10-11, estimate_road_norm.py:13-15)
        const uint64_t key = ransac_frame_key(a.case_seeds[c], fcnt);
        flat_build_hypotheses<BLK>(key, a.id_triples ? a.id_triples + fc * H * 3 : nullptr, H, n, M, L, X, Y, Z, mods, cnts);
        __syncthreads();
        ransac_count_weighted<WAVES>(mods, cnts, H, n_items, a.threshold, packed,
            [&](int j, double &px, double &py, double &pz, int &wgt) { px = PX[j]; py = PY[j]; pz = PZ[j]; wgt = PW[j]; },
            [&](int j, double &px, double &py, double &pz, int &wgt) { const int id = Dv[j]; wgt = W[id]; px = X[id]; py = Y[id]; pz = Z[id]; });
        __syncthreads();
        if (a.hyp_counts) for (int h = tid; h < H; h += BLK) a.hyp_counts[fc * H + h] = cnts[h];
        if (wave == 0) {
            const FlatRansacResult r = flat_ransac_result(true, 0, mods, cnts, H, goal, a.absolute_reference);
            if (lane == 0) {
                a.status[fc] = r.status; a.raw_scale[fc] = r.raw; a.best_ic[fc] = r.best_ic; a.used[fc] = r.used;
                for (int kk = 0; kk < 4; ++kk) a.model[4 * fc + kk] = r.m[kk];
            }
        }
        __syncthreads();                                             // (the next case rewrites the planes and the counts)
    }
}

}  // namespace mvosr

using namespace mvosr;

extern "C" {

size_t mvosr_flat_ransac_cases_lds_bytes(int max_feat, int64_t max_tri, int n_hyp) {
    const size_t mf = max_feat > 0 ? (size_t)max_feat : 0;
    const size_t mt = max_tri > 0 ? (size_t)max_tri : 2 * mf;
    return cases_plan<size_t>(mf, mt, n_hyp > 0 ? (size_t)n_hyp : 0).total;
}

int mvosr_flat_ransac_cases_batch(mvosr_ctx *ctx, const mvosr_batch *b, const int32_t *keep, const mvosr_rescale_params *rp,
                                  const uint64_t *case_seeds, int32_t n_cases, int32_t cases_per_group, const int32_t *id_triples,
                                  const int64_t *frame_ids, const int32_t *dt_status, const uint8_t *tri_flags,
                                  const mvosr_rescale_cases_outputs *o, int64_t max_tri) {
    if (!ctx || !b || !rp || !o || !case_seeds || !tri_flags) return set_error(MVOSR_ERR_ARG, "flat_ransac_cases: null argument");
    if (!o->raw_scale || !o->model || !o->best_ic || !o->used || !o->status)
        return set_error(MVOSR_ERR_ARG, "flat_ransac_cases: a required output is null");
    if (!b->feat_off || !b->feat_cnt || !b->x || !b->y || !b->z || !b->tri2_off || !b->tri2) return set_error(MVOSR_ERR_ARG, "flat_ransac_cases: missing x/y/z/tri2");
    if (rp->n_hyp < 1 || rp->n_hyp > kCasesMaxHyp) return set_error(MVOSR_ERR_ARG, "flat_ransac_cases: n_hyp must be in 1..%d", kCasesMaxHyp);
    if (rp->ransac_min_points < 3) return set_error(MVOSR_ERR_ARG, "flat_ransac_cases: ransac_min_points < 3");
    if (n_cases < 1 || n_cases > kCasesMaxCases) return set_error(MVOSR_ERR_ARG, "flat_ransac_cases: n_cases must be in 1..%d", kCasesMaxCases);
    if (cases_per_group < 0) return set_error(MVOSR_ERR_ARG, "flat_ransac_cases: cases_per_group < 0");
    if (b->max_feat < 0) return set_error(MVOSR_ERR_ARG, "flat_ransac_cases: max_feat < 0");
    if (b->max_feat > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "flat_ransac_cases: vertex ids are 16-bit in the point list");
    if (b->n_frames <= 0) return MVOSR_OK;
    if (max_tri <= 0) max_tri = 2 * (int64_t)b->max_feat;
    if (max_tri > INT32_MAX / 3) return set_error(MVOSR_ERR_TOO_LARGE, "flat_ransac_cases: three times max_tri does not fit 32 bits");
    int G = cases_per_group ? cases_per_group : kCasesDefaultGroup;
    if (G > n_cases) G = n_cases;
    const int n_groups = (n_cases + G - 1) / G;
    if (b->n_frames > (int64_t)0x7fffffff / n_groups) return set_error(MVOSR_ERR_TOO_LARGE, "flat_ransac_cases: frames x groups exceeds a grid");
    const size_t lds = cases_plan<size_t>((size_t)b->max_feat, (size_t)max_tri, (size_t)rp->n_hyp).total;
    if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_TOO_LARGE, "flat_ransac_cases: a frame of %d features and %lld rows needs %zu B of LDS (> %d)", b->max_feat,
                         (long long)max_tri, lds, ctx->max_lds_per_block);
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(flat_ransac_cases_kernel<kCasesWaves>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    CasesArgs a = {};
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.x = b->x; a.y = b->y; a.z = b->z;
    a.tri_off = b->tri2_off; a.tri = b->tri2; a.tri_cnt = b->tri2_cnt;
    a.keep = keep; a.dt_status = dt_status; a.tri_flags = tri_flags; a.id_triples = id_triples; a.frame_ids = frame_ids;
    a.case_seeds = case_seeds;
    a.n_hyp = rp->n_hyp; a.ransac_min_points = rp->ransac_min_points; a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri;
    a.n_cases = n_cases; a.cases_per_group = G; a.n_groups = n_groups;
    a.threshold = rp->threshold; a.goal_fraction = rp->goal_fraction; a.absolute_reference = rp->absolute_reference;
    a.frame_base = rp->frame_base;
    a.raw_scale = o->raw_scale; a.model = o->model; a.best_ic = o->best_ic; a.used = o->used; a.status = o->status;
    a.hyp_counts = o->hyp_counts; a.count_form = o->count_form;
    hipLaunchKernelGGL(flat_ransac_cases_kernel<kCasesWaves>, dim3((unsigned)(b->n_frames * n_groups)), dim3(kCasesWaves * kWave), lds,
                       ctx_stream(ctx), a);
    return check_launch("flat_ransac_cases_kernel");
}

}  // extern "C"
