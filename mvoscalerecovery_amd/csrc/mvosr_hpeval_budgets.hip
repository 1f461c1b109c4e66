// mvosr_hpeval_budgets.hip — the RANSAC evaluation runs (mvosr_hpeval.hip) at every iteration budget of a list in ONE launch
// (DESIGN.md §3.24).  The reference's two scripts, /root/reference/src/calculate_height_pitch_eval.py and
// calculate_height_pitch_eval_line.py, take the budget from the command line (:27) and exist to be run at several; the device
// draw of hypothesis h depends on (seed, frame, case, h) and not on the budget, so the run at budget b is the first b hypotheses
// of the run at any larger one.  One workgroup per (frame, group of cases), as height_pitch_eval_kernel:
//
//   once per workgroup: the frame pass (mvosr_heightpitch_pass.hpp);
//   per case: the hypotheses of the LAST budget in tiles of kHpMaxHyp and their counts, once; the replay of mvosr_ransac.hpp in
//   segments that end at the checkpoints (its carried state makes the segmented replay the unsegmented one), a snapshot of its
//   state and of the best model at each; then the post-RANSAC tail (mvosr_hpeval_tail.hpp) once per DISTINCT best model among the
//   checkpoints — a checkpoint whose best is its predecessor's takes the same values and its own `used`.
//
// Slot [f][c][k] of every output is, byte for byte, what mvosr_height_pitch_eval_batch writes at [f][c] with n_hyp = budgets[k].
// fp64, compiled with -ffp-contract=off; every sum is taken in the evaluation kernel's fixed order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mvosr.h"
#include "mvosr_device.hpp"
#include "mvosr_ransac.hpp"
#include "mvosr_host.hpp"
#include "mvosr_hpeval_budgets_plan.hpp"
#include "mvosr_heightpitch_pass.hpp"
#include "mvosr_hpeval_tail.hpp"

namespace mvosr {

constexpr int kHpbDefaultGroup = 1;    // cases_per_group where the caller passes 0: as height_pitch_eval_kernel (§3.15's measurement)

struct HpbArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *u, *v, *depth;
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    double focus, cx, cy;
    int32_t min_points, n_hyp, max_feat, max_tri, n_cases, cases_per_group, n_groups, n_budgets;   // n_hyp: the last budget
    int32_t budgets[kHpeMaxBudgets];
    double threshold, goal_fraction, inlier_threshold;
    uint64_t seed; int64_t frame_base;
    const double *prior;           // [F][4] window low / high in degrees, sin and cos of the prior
    const int32_t *samples;        // [F][C][H][3] list positions (the line reads two), or null: drawn
    double *ransac_height, *model; // [F][C][B], [F][C][B][4]
    int32_t *best_ic, *used, *n_inliers, *best;                                            // [F][C][B]
    int32_t *n_selected;                                                                   // [F]
    double *refined_normal, *refined_pitch, *refined_mean, *refined_std, *height_t_mean;   // [F][C][B][3], [F][C][B] each
    double *sum_y, *sum_z;         // [F][C][B]
    int32_t *status;               // [F][C][B]
    int32_t *point_list;           // optional, at 3 * tri_off[f]
    int32_t *hyp_counts;           // optional [F][C][H]
};

// slot s = (f * C + c) * B + k: the refusal outputs of mvosr_height_pitch_eval_batch, and no best
__device__ __forceinline__ void hpb_refuse(const HpbArgs &a, int64_t s, int status, int used) {
    const double q = nan("");
    a.status[s] = status;
    a.ransac_height[s] = q; a.refined_pitch[s] = q; a.refined_mean[s] = q; a.refined_std[s] = q; a.height_t_mean[s] = q;
    a.sum_y[s] = q; a.sum_z[s] = q;
    for (int k = 0; k < 4; ++k) a.model[4 * s + k] = q;
    for (int k = 0; k < 3; ++k) a.refined_normal[3 * s + k] = q;
    a.best_ic[s] = 0; a.used[s] = used; a.n_inliers[s] = 0; a.best[s] = -1;
}
// the whole frame is not fitted: every budget of every case of this workgroup's group, a slot per thread and trip, and (group 0)
// the list's length.  Every thread of the workgroup calls it.
__device__ __forceinline__ void hpb_refuse_frame(const HpbArgs &a, int64_t f, int g, int c_lo, int c_hi, int status, int n_selected) {
    const int64_t B = a.n_budgets, lo = (f * a.n_cases + c_lo) * B, hi = (f * a.n_cases + c_hi) * B;
    for (int64_t s = lo + threadIdx.x; s < hi; s += kHpBlock) hpb_refuse(a, s, status, 0);
    if (g == 0 && threadIdx.x == 0) a.n_selected[f] = n_selected;
}

template <int MODEL>
__global__ __launch_bounds__(kHpBlock) void height_pitch_eval_budgets_kernel(const HpbArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool LINE = MODEL == MVOSR_HP_MODEL_LINE;
    const int64_t f = blockIdx.x / (unsigned)a.n_groups;
    const int g = (int)(blockIdx.x % (unsigned)a.n_groups);
    const int C = a.n_cases, c_lo = g * a.cases_per_group, c_hi = min(C, c_lo + a.cases_per_group);
    const int n = a.feat_cnt[f];
    const int64_t off = a.feat_off[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    if (n <= 0 || tn <= 0) { hpb_refuse_frame(a, f, g, c_lo, c_hi, MVOSR_ST_ERR_EMPTY, 0); return; }
    // more features or rows than the launch's LDS was sized for: refused, LDS untouched
    if (n > a.max_feat || tn > a.max_tri) { hpb_refuse_frame(a, f, g, c_lo, c_hi, MVOSR_ST_ERR_MASK, 0); return; }
    const int H = a.n_hyp, B = a.n_budgets;
    const auto plan = hpeval_budgets_plan<uint32_t>((uint32_t)n, (uint32_t)tn, (uint32_t)H, (uint32_t)B);
    const auto &lds = plan.frame;
    double *X = reinterpret_cast<double *>(smem + lds.x);
    double *Y = reinterpret_cast<double *>(smem + lds.y);
    double *Z = reinterpret_cast<double *>(smem + lds.z);
    uint16_t *L = reinterpret_cast<uint16_t *>(smem + lds.list);
    double4 *mods = reinterpret_cast<double4 *>(smem + lds.mods);
    int *cnts = reinterpret_cast<int *>(smem + lds.cnts);
    unsigned long long *words = reinterpret_cast<unsigned long long *>(smem + lds.words);
    int *misc = reinterpret_cast<int *>(smem + lds.misc);
    double *red = reinterpret_cast<double *>(smem + lds.red);
    HpeSnapshot *snap = reinterpret_cast<HpeSnapshot *>(smem + plan.snap);

    double sin_est, cos_est;
    const int M = hp_frame_pass(a, f, n, tn, off, tb, g == 0, X, Y, Z, L, misc, sin_est, cos_est);
    if (M < 0) {
        hpb_refuse_frame(a, f, g, c_lo, c_hi, misc[HM_BADID] ? MVOSR_ST_ERR_MASK : MVOSR_ST_ERR_SINGULAR, 0);
        return;
    }
    if (M < a.min_points) {                                                          // :159: the host carries the previous frame, case by case
        hpb_refuse_frame(a, f, g, c_lo, c_hi, MVOSR_ST_RS_FEW, M);
        return;
    }
    if (tid == 0 && g == 0) a.n_selected[f] = M;
    __syncthreads();
    const uint64_t fkey = ransac_frame_key(a.seed, (uint64_t)(a.frame_base + f));
    const double goal = (double)M * a.goal_fraction;                                 // estimate_road_norm.py:62, :68
    const int nw = (M + kWave - 1) / kWave;
    const bool skip_after_stop = a.hyp_counts == nullptr;                            // (hyp_counts are the counts of all H hypotheses)

    for (int c = c_lo; c < c_hi; ++c) {
        const int64_t fc = f * C + c;
        const uint64_t key = ransac_mix64(fkey ^ ((uint64_t)(c + 1) * 0xA0761D6478BD642Full));
        if (tid == 0) { misc[HM_BEST] = -1; misc[HM_BESTIC] = 0; misc[HM_USED] = H; misc[HE_DONE] = 0; misc[HB_NEXT] = 0; }
        for (int h0 = 0; h0 < H; h0 += kHpMaxHyp) {
            // the goal stop lies behind: every checkpoint has its snapshot.  Workgroup-uniform: HE_DONE was written before the
            // barrier that ends the previous tile
            if (skip_after_stop && h0 > 0 && misc[HE_DONE]) break;
            const int T = min(kHpMaxHyp, H - h0);
            // ---- the tile's hypotheses, one thread each (ransac.py:10-11, estimate_road_norm.py:13-15, :44-46)
            for (int ht = tid; ht < T; ht += kHpBlock) {
                const int h = h0 + ht;
                int p0, p1, p2 = 0;
                if (a.samples) { const int32_t *t = a.samples + (fc * H + h) * 3; p0 = t[0]; p1 = t[1]; if (!LINE) p2 = t[2]; }
                else if (LINE) ransac_draw2(key, h, M, p0, p1);
                else ransac_draw3(key, h, M, p0, p1, p2);
                // a sample that names a position outside the list, or one vertex twice, is spent: NaN model, no inlier
                bool ok = ids_in_range(p0, p1, p2, M);
                int v0 = 0, v1 = 0, v2 = 0;
                if (ok) { v0 = L[p0]; v1 = L[p1]; v2 = L[p2]; ok = LINE ? v0 != v1 : (v0 != v1 && v0 != v2 && v1 != v2); }
                double4 m; m.x = m.y = m.z = m.w = nan("");
                if (ok) m = LINE ? ransac_unit_line(Y, Z, v0, v1) : ransac_unit_plane(X, Y, Z, v0, v1, v2);   // the line: a y + b z + c = 0
                mods[ht] = m;
                cnts[ht] = 0;
            }
            __syncthreads();
            // ---- inlier counts over the list, repeats included: as height_pitch_eval_kernel, once for all budgets
            ransac_count_resident<LINE, kHpPPT, 2, kHpBlock>(M, mods, cnts, T, a.threshold, [&](int j, double &q0, double &q1, double &q2) {
                const int id = L[j];
                if (LINE) { q0 = Y[id]; q1 = Z[id]; q2 = 0.0; } else { q0 = X[id]; q1 = Y[id]; q2 = Z[id]; }
            });
            __syncthreads();
            if (a.hyp_counts) for (int ht = tid; ht < T; ht += kHpBlock) a.hyp_counts[fc * H + h0 + ht] = cnts[ht];
            // ---- ransac.py:9-22 by wavefront 0 over the tile's segments [s, e): a segment ends at a checkpoint or at the tile's end
            if (wave == 0) {
                RansacReplay rp = {misc[HM_BEST], misc[HM_BESTIC], misc[HM_USED], misc[HE_DONE]};
                int k = misc[HB_NEXT];
                for (int s = 0; s < T;) {
                    const int bk = k < B ? a.budgets[k] : 0x7fffffff;                // (ascending and > h0 + s: earlier ones are behind)
                    const bool at = bk - h0 <= T;
                    const int e = at ? bk - h0 : T;
                    if (!rp.done) {
                        ransac_replay(rp, cnts + s, h0 + s, e - s, goal);
                        if (lane == 0 && rp.best >= h0 + s) {                        // (a best of this segment)
                            const double4 bm = mods[rp.best - h0];
                            red[HER_MODEL] = bm.x; red[HER_MODEL + 1] = bm.y; red[HER_MODEL + 2] = bm.z; red[HER_MODEL + 3] = bm.w;
                        }
                    }
                    // the snapshot of checkpoint k; after the stop nothing moves any more: every checkpoint still open takes this
                    // state, wherever in the tile the stop came (the tiles behind it may be skipped)
                    const int k_end = rp.done ? B : (at ? k + 1 : k);
                    if (lane == 0)
                        for (int q = k; q < k_end; ++q) {
                            HpeSnapshot &sn = snap[q];
                            sn.best = rp.best; sn.best_ic = rp.best_ic; sn.used = rp.done ? rp.used : a.budgets[q]; sn.done = rp.done;
                            for (int i = 0; i < 4; ++i) sn.m[i] = red[HER_MODEL + i];
                        }
                    k = k_end;
                    s = e;
                }
                if (lane == 0) {
                    misc[HM_BEST] = rp.best; misc[HM_BESTIC] = rp.best_ic; misc[HM_USED] = rp.used; misc[HE_DONE] = rp.done; misc[HB_NEXT] = k;
                }
            }
            __syncthreads();
        }
        // ---- the tail, once per run [k0, k1) of checkpoints with one best (the best's number only grows with the budget); every
        // thread ends it with the same values (the block sums hand every thread the totals), and thread k - k0 writes slot k
        for (int k0 = 0; k0 < B;) {
            const int best = snap[k0].best, best_ic = snap[k0].best_ic;
            int k1 = k0 + 1;
            while (k1 < B && snap[k1].best == best) ++k1;
            if (best < 0) {                                                          // no hypothesis with an inlier so far: no model
                if (tid < k1 - k0) hpb_refuse(a, fc * B + k0 + tid, MVOSR_ST_RS_FEW, snap[k0 + tid].used);
            } else {
                hpe_case_tail<LINE>(make_double4(snap[k0].m[0], snap[k0].m[1], snap[k0].m[2], snap[k0].m[3]), M, nw, X, Y, Z, L, words, misc, red,
                                    a.inlier_threshold, sin_est, cos_est, k1 - k0, [&](const HpeTail &t) {
                    const int k = k0 + tid;
                    const int64_t s = fc * B + k;
                    a.ransac_height[s] = t.ransac_height;
                    a.model[4 * s] = t.m0; a.model[4 * s + 1] = t.m1; a.model[4 * s + 2] = t.m2; a.model[4 * s + 3] = t.m3;
                    a.best_ic[s] = best_ic; a.used[s] = snap[k].used; a.n_inliers[s] = t.n_inliers; a.best[s] = best;
                    a.refined_normal[3 * s] = t.nhx; a.refined_normal[3 * s + 1] = t.nhy; a.refined_normal[3 * s + 2] = t.nhz;
                    a.refined_pitch[s] = t.refined_pitch;
                    a.refined_mean[s] = t.refined_mean;
                    a.refined_std[s] = t.refined_std;
                    a.height_t_mean[s] = t.height_t_mean;
                    a.sum_y[s] = t.sum_y; a.sum_z[s] = t.sum_z;
                    a.status[s] = t.status;
                });
            }
            __syncthreads();                                                         // (the next run, or case, reuses misc, words and the reduction slots)
            k0 = k1;
        }
    }
}

// 1 <= n <= kHpeMaxBudgets, strictly ascending, budgets[0] >= 1, the last <= kHpeMaxHyp
static bool budgets_ok(const int32_t *budgets, int n) {
    if (!budgets || n < 1 || n > kHpeMaxBudgets || budgets[0] < 1 || budgets[n - 1] > kHpeMaxHyp) return false;
    for (int k = 1; k < n; ++k) if (budgets[k] <= budgets[k - 1]) return false;
    return true;
}

}  // namespace mvosr

using namespace mvosr;

extern "C" {

size_t mvosr_height_pitch_eval_budgets_lds_bytes(int max_feat, int n_hyp_max, int n_budgets, int model) {
    (void)model;                                                                     // (both models keep a hypothesis as one double4)
    const size_t mf = max_feat > 0 ? (size_t)max_feat : 0, mt = mf ? 2 * mf : 1;
    return hpeval_budgets_plan<size_t>(mf, mt, n_hyp_max > 0 ? (size_t)n_hyp_max : 0, n_budgets > 0 ? (size_t)n_budgets : 0).total;
}

int mvosr_height_pitch_eval_budgets_batch(mvosr_ctx *ctx, const mvosr_batch *b, const mvosr_height_pitch_eval_params *p, const int32_t *budgets,
                                          int n_budgets, const double *frame_prior, const int32_t *samples,
                                          const mvosr_height_pitch_eval_budgets_outputs *o) {
    if (!ctx || !b || !p || !frame_prior || !o) return set_error(MVOSR_ERR_ARG, "height_pitch_eval_budgets: null argument");
    if (!o->ransac_height || !o->model || !o->best_ic || !o->used || !o->n_selected || !o->n_inliers || !o->refined_normal ||
        !o->refined_pitch || !o->refined_mean || !o->refined_std || !o->height_t_mean || !o->sum_y || !o->sum_z || !o->status || !o->best)
        return set_error(MVOSR_ERR_ARG, "height_pitch_eval_budgets: a required output is null");
    if (!b->feat_off || !b->feat_cnt || !b->x || !b->v || !b->z || !b->tri1_off || !b->tri1)
        return set_error(MVOSR_ERR_ARG, "height_pitch_eval_budgets: missing u (x) / v / depth (z) / tri1");
    if (p->model != MVOSR_HP_MODEL_PLANE && p->model != MVOSR_HP_MODEL_LINE)
        return set_error(MVOSR_ERR_ARG, "height_pitch_eval_budgets: unknown model %d", p->model);
    if (!budgets_ok(budgets, n_budgets))
        return set_error(MVOSR_ERR_ARG, "height_pitch_eval_budgets: 1..%d budgets, strictly ascending, within 1..%d", kHpeMaxBudgets, kHpeMaxHyp);
    if (p->n_cases < 1 || p->n_cases > kHpeMaxCases) return set_error(MVOSR_ERR_ARG, "height_pitch_eval_budgets: n_cases must be in 1..%d", kHpeMaxCases);
    if (p->cases_per_group < 0) return set_error(MVOSR_ERR_ARG, "height_pitch_eval_budgets: cases_per_group < 0");
    if (p->min_points < 3) return set_error(MVOSR_ERR_ARG, "height_pitch_eval_budgets: min_points < 3");
    if (b->max_feat < 0) return set_error(MVOSR_ERR_ARG, "height_pitch_eval_budgets: max_feat < 0");
    if (b->n_frames <= 0) return MVOSR_OK;
    const int H = budgets[n_budgets - 1];                                            // (p->n_hyp is not read)
    int G = p->cases_per_group ? p->cases_per_group : kHpbDefaultGroup;
    if (G <= 0 || G > p->n_cases) G = p->n_cases;
    const int n_groups = (p->n_cases + G - 1) / G;
    if (b->n_frames > (int64_t)0x7fffffff / n_groups) return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch_eval_budgets: frames x groups exceeds a grid");
    const int64_t max_tri = b->max_feat > 0 ? 2 * (int64_t)b->max_feat : 1;
    if (b->max_feat > 65535 || 3 * max_tri > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch_eval_budgets: ids and list positions are 16-bit in LDS");
    const size_t lds = hpeval_budgets_plan<size_t>((size_t)b->max_feat, (size_t)max_tri, (size_t)H, (size_t)n_budgets).total;
    if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch_eval_budgets: a frame of %d features needs %zu B of LDS (> %d)", b->max_feat, lds, ctx->max_lds_per_block);
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    const bool line = p->model == MVOSR_HP_MODEL_LINE;
    const void *fn = line ? reinterpret_cast<const void *>(height_pitch_eval_budgets_kernel<MVOSR_HP_MODEL_LINE>)
                          : reinterpret_cast<const void *>(height_pitch_eval_budgets_kernel<MVOSR_HP_MODEL_PLANE>);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    HpbArgs a = {};
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.u = b->x; a.v = b->v; a.depth = b->z;
    a.tri_off = b->tri1_off; a.tri = b->tri1; a.tri_cnt = b->tri1_cnt;
    a.focus = p->focus; a.cx = p->cx; a.cy = p->cy; a.min_points = p->min_points; a.n_hyp = H; a.n_budgets = n_budgets;
    for (int k = 0; k < n_budgets; ++k) a.budgets[k] = budgets[k];
    a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri; a.n_cases = p->n_cases; a.cases_per_group = G; a.n_groups = n_groups;
    a.threshold = p->threshold; a.goal_fraction = p->goal_fraction; a.inlier_threshold = p->inlier_threshold;
    a.seed = p->seed; a.frame_base = p->frame_base; a.prior = frame_prior; a.samples = samples;
    a.ransac_height = o->ransac_height; a.model = o->model; a.best_ic = o->best_ic; a.used = o->used; a.n_selected = o->n_selected;
    a.n_inliers = o->n_inliers; a.refined_normal = o->refined_normal; a.refined_pitch = o->refined_pitch; a.refined_mean = o->refined_mean;
    a.refined_std = o->refined_std; a.height_t_mean = o->height_t_mean; a.sum_y = o->sum_y; a.sum_z = o->sum_z; a.status = o->status;
    a.best = o->best; a.point_list = o->point_list; a.hyp_counts = o->hyp_counts;
    const dim3 grid((unsigned)(b->n_frames * n_groups)), block(kHpBlock);
    if (line) hipLaunchKernelGGL(height_pitch_eval_budgets_kernel<MVOSR_HP_MODEL_LINE>, grid, block, lds, ctx_stream(ctx), a);
    else hipLaunchKernelGGL(height_pitch_eval_budgets_kernel<MVOSR_HP_MODEL_PLANE>, grid, block, lds, ctx_stream(ctx), a);
    return check_launch("height_pitch_eval_budgets_kernel");
}

}  // extern "C"
