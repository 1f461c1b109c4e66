// mvosr_hpeval.hip — the reference's RANSAC evaluation runs, /root/reference/src/calculate_height_pitch_eval.py (the 3-D plane)
// and calculate_height_pitch_eval_line.py (the 2-D line in (y, z)): the whole sequence `n_cases` times with a fresh sample
// sequence each, one workgroup per (frame, group of cases) in ONE launch:
//
//   once per workgroup: back-projection, the rows, the prior's window, the point list (mvosr_heightpitch_pass.hpp, _eval.py:80-149);
//   per case, the frame resident in LDS: the hypotheses in tiles of kHpMaxHyp (get_pitch_ransac / get_pitch_line_ransac, :164-165),
//   the replay carried over the tiles (thirdparty/Ransac/ransac.py:9-22), the best model's inliers among the LIST at 0.01, repeats
//   included (:167-169), the RANSAC camera height (:175-187), and the refinement over those list inliers (:198-225): the plane
//   through the first three / the line through the first two, its pitch, mean and std of the distances, mean of z sin + y cos.
//
// fp64, compiled with -ffp-contract=off; every sum is taken in a fixed order: results are run-to-run identical and depend neither
// on the batch nor on cases_per_group.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mvosr.h"
#include "mvosr_device.hpp"
#include "mvosr_ransac.hpp"
#include "mvosr_host.hpp"
#include "mvosr_hpeval_plan.hpp"
#include "mvosr_heightpitch_pass.hpp"

namespace mvosr {

// cases_per_group where the caller passes 0.  Measured (profiles/hpeval_bench.json, 512 frames x 10 cases): one case per workgroup is
// 1.3x faster than ten — redoing the frame pass costs less than the coarser grid loses on 256 CUs — and 9x faster on 16 frames
constexpr int kHpeDefaultGroup = 1;

struct HpeArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *u, *v, *depth;
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    double focus, cx, cy;
    int32_t min_points, n_hyp, max_feat, max_tri, n_cases, cases_per_group, n_groups;
    double threshold, goal_fraction, inlier_threshold;
    uint64_t seed; int64_t frame_base;
    const double *prior;           // [F][4] window low / high in degrees, sin and cos of the prior
    const int32_t *samples;        // [F][C][H][3] list positions (the line reads two), or null: drawn
    double *ransac_height, *model; // [F][C], [F][C][4]
    int32_t *best_ic, *used, *n_inliers;                                                   // [F][C]
    int32_t *n_selected;                                                                   // [F]
    double *refined_normal, *refined_pitch, *refined_mean, *refined_std, *height_t_mean;   // [F][C][3], [F][C] each
    double *sum_y, *sum_z;         // [F][C]
    int32_t *status;               // [F][C]
    uint8_t *list_mask; int64_t list_stride;   // optional: case c of frame f at c * list_stride + 3 * tri_off[f]
    int32_t *point_list;           // optional, at 3 * tri_off[f]
    int32_t *hyp_counts;           // optional [F][C][H]
};

__device__ __forceinline__ void hpe_refuse(const HpeArgs &a, int64_t fc, int status) {
    const double q = nan("");
    a.status[fc] = status;
    a.ransac_height[fc] = q; a.refined_pitch[fc] = q; a.refined_mean[fc] = q; a.refined_std[fc] = q; a.height_t_mean[fc] = q;
    a.sum_y[fc] = q; a.sum_z[fc] = q;
    for (int k = 0; k < 4; ++k) a.model[4 * fc + k] = q;
    for (int k = 0; k < 3; ++k) a.refined_normal[3 * fc + k] = q;
    a.best_ic[fc] = 0; a.used[fc] = 0; a.n_inliers[fc] = 0;
}
// the whole frame is not fitted: every case of this workgroup's group, and (group 0) the list's length
__device__ __forceinline__ void hpe_refuse_frame(const HpeArgs &a, int64_t f, int g, int c_lo, int c_hi, int status, int n_selected) {
    for (int c = c_lo; c < c_hi; ++c) hpe_refuse(a, f * a.n_cases + c, status);
    if (g == 0) a.n_selected[f] = n_selected;
}

template <int MODEL>
__global__ __launch_bounds__(kHpBlock) void height_pitch_eval_kernel(const HpeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool LINE = MODEL == MVOSR_HP_MODEL_LINE;
    constexpr int K = LINE ? 2 : 3;                                                  // the sample's size
    const int64_t f = blockIdx.x / (unsigned)a.n_groups;
    const int g = (int)(blockIdx.x % (unsigned)a.n_groups);
    const int C = a.n_cases, c_lo = g * a.cases_per_group, c_hi = min(C, c_lo + a.cases_per_group);
    const int n = a.feat_cnt[f];
    const int64_t off = a.feat_off[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    if (n <= 0 || tn <= 0) { if (tid == 0) hpe_refuse_frame(a, f, g, c_lo, c_hi, MVOSR_ST_ERR_EMPTY, 0); return; }
    // more features or rows than the launch's LDS was sized for: refused, LDS untouched
    if (n > a.max_feat || tn > a.max_tri) { if (tid == 0) hpe_refuse_frame(a, f, g, c_lo, c_hi, MVOSR_ST_ERR_MASK, 0); return; }
    const int H = a.n_hyp;
    const auto lds = hpeval_plan<uint32_t>((uint32_t)n, (uint32_t)tn, (uint32_t)H);
    double *X = reinterpret_cast<double *>(smem + lds.x);
    double *Y = reinterpret_cast<double *>(smem + lds.y);
    double *Z = reinterpret_cast<double *>(smem + lds.z);
    uint16_t *L = reinterpret_cast<uint16_t *>(smem + lds.list);
    double4 *mods = reinterpret_cast<double4 *>(smem + lds.mods);
    int *cnts = reinterpret_cast<int *>(smem + lds.cnts);
    unsigned long long *words = reinterpret_cast<unsigned long long *>(smem + lds.words);
    int *misc = reinterpret_cast<int *>(smem + lds.misc);
    double *red = reinterpret_cast<double *>(smem + lds.red);

    double sin_est, cos_est;
    const int M = hp_frame_pass(a, f, n, tn, off, tb, g == 0, X, Y, Z, L, misc, sin_est, cos_est);
    if (M < 0) {
        if (tid == 0) hpe_refuse_frame(a, f, g, c_lo, c_hi, misc[HM_BADID] ? MVOSR_ST_ERR_MASK : MVOSR_ST_ERR_SINGULAR, 0);
        return;
    }
    if (M < a.min_points) {                                                          // :159: the host carries the previous frame, case by case
        if (tid == 0) hpe_refuse_frame(a, f, g, c_lo, c_hi, MVOSR_ST_RS_FEW, M);
        return;
    }
    if (tid == 0 && g == 0) a.n_selected[f] = M;
    __syncthreads();
    const uint64_t fkey = ransac_frame_key(a.seed, (uint64_t)(a.frame_base + f));
    const double goal = (double)M * a.goal_fraction;                                 // estimate_road_norm.py:62, :68
    const int nw = (M + kWave - 1) / kWave;

    for (int c = c_lo; c < c_hi; ++c) {
        const int64_t fc = f * C + c;
        const uint64_t key = ransac_mix64(fkey ^ ((uint64_t)(c + 1) * 0xA0761D6478BD642Full));
        if (tid == 0) { misc[HM_BEST] = -1; misc[HM_BESTIC] = 0; misc[HM_USED] = H; misc[HE_DONE] = 0; }
        for (int h0 = 0; h0 < H; h0 += kHpMaxHyp) {
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
            // ---- inlier counts over the list, repeats included: the list's points in registers, the hypotheses streamed from LDS
            // (wave-uniform reads), ballot + popcount, one integer LDS add per wavefront and hypothesis
            ransac_count_resident<LINE, kHpPPT, 2, kHpBlock>(M, mods, cnts, T, a.threshold, [&](int j, double &q0, double &q1, double &q2) {
                const int id = L[j];
                if (LINE) { q0 = Y[id]; q1 = Z[id]; q2 = 0.0; } else { q0 = X[id]; q1 = Y[id]; q2 = Z[id]; }
            });
            __syncthreads();
            if (a.hyp_counts) for (int ht = tid; ht < T; ht += kHpBlock) a.hyp_counts[fc * H + h0 + ht] = cnts[ht];
            // ---- ransac.py:9-22 by wavefront 0, 64 hypotheses at a time, its state carried from tile to tile
            if (wave == 0 && !misc[HE_DONE]) {
                RansacReplay rp = {misc[HM_BEST], misc[HM_BESTIC], misc[HM_USED], 0};
                ransac_replay(rp, cnts, h0, T, goal);
                if (lane == 0) {
                    misc[HM_BEST] = rp.best; misc[HM_BESTIC] = rp.best_ic; misc[HM_USED] = rp.used; misc[HE_DONE] = rp.done;
                    if (rp.best >= h0) { const double4 bm = mods[rp.best - h0]; red[HER_MODEL] = bm.x; red[HER_MODEL + 1] = bm.y; red[HER_MODEL + 2] = bm.z; red[HER_MODEL + 3] = bm.w; }   // (a best of this tile)
                }
            }
            __syncthreads();
        }
        const int best_ic = misc[HM_BESTIC], used = misc[HM_USED];
        if (misc[HM_BEST] < 0) {                                                     // no hypothesis with an inlier: no model
            if (tid == 0) { hpe_refuse(a, fc, MVOSR_ST_RS_FEW); a.used[fc] = used; }
            __syncthreads();
            continue;
        }
        // :175-180: plane — flipped on n_y < 0; line — (a, b) and h_bar flipped on b < 0: the model's second slot either way
        const double4 bm = ransac_sign_rule(make_double4(red[HER_MODEL], red[HER_MODEL + 1], red[HER_MODEL + 2], red[HER_MODEL + 3]));
        const double m0 = bm.x, m1 = bm.y, m2 = bm.z, m3 = bm.w;
        // ---- get_inliers over the LIST (:167-169, estimate_road_norm.py:71-78): one ballot per 64 list positions
        for (int w = wave; w < nw; w += kHpWaves) {
            const int j = w * kWave + lane;
            const int id = L[min(j, M - 1)];
            const double r = LINE ? (Y[id] * m0 + Z[id] * m1) + m3 : ((X[id] * m0 + Y[id] * m1) + Z[id] * m2) + m3;
            const bool inl = j < M && fabs(r) < a.inlier_threshold;
            const unsigned long long bal = __ballot(inl);
            if (lane == 0) words[w] = bal;
            if (a.list_mask && j < M) a.list_mask[(int64_t)c * a.list_stride + 3 * tb + j] = inl ? 1 : 0;
        }
        __syncthreads();
        if (wave == 0) {
            int cnt = 0;
            for (int w = lane; w < nw; w += kWave) cnt += __popcll(words[w]);
            cnt = wave_sum(cnt);
            if (lane == 0) {
                misc[HM_NIN] = cnt;
                int found = 0;
                for (int w = 0; w < nw && found < K; ++w) {                          // inliers[:3] / [:2], the sample `estimate` reads (:198)
                    unsigned long long bits = words[w];
                    while (bits && found < K) { misc[HM_I0 + found++] = L[w * kWave + (int)__ffsll((long long)bits) - 1]; bits &= bits - 1ull; }
                }
                // fewer than K vertices among them: the script's SVD has a null space of more than one dimension
                bool degen = found < K || misc[HM_I0] == misc[HM_I0 + 1];
                if (!LINE && !degen) degen = misc[HM_I0] == misc[HM_I0 + 2] || misc[HM_I0 + 1] == misc[HM_I0 + 2];
                misc[HE_DEGEN] = degen ? 1 : 0;
            }
        }
        __syncthreads();
        const int n_in = misc[HM_NIN];
        const bool degen = misc[HE_DEGEN] != 0;
        // ---- the refinement (:198-225)
        double nhx = LINE ? 0.0 : nan(""), nhy = nan(""), nhz = nan("");
        if (!degen) {
            const int i0 = misc[HM_I0], i1 = misc[HM_I0 + 1];
            if (LINE) {
                double ny = Z[i1] - Z[i0], nz = -(Y[i1] - Y[i0]);
                if (nz < 0.0) { ny = -ny; nz = -nz; }                                // _eval_line.py:201-202: the z component
                const double len = sqrt(ny * ny + nz * nz);                          // :204-206
                nhy = ny / len; nhz = nz / len;
            } else {
                const int i2 = misc[HM_I0 + 2];
                double nx, ny, nz;
                ransac_edge_cross(X[i0], Y[i0], Z[i0], X[i1], Y[i1], Z[i1], X[i2], Y[i2], Z[i2], nx, ny, nz);
                if (ny < 0.0) { nx = -nx; ny = -ny; nz = -nz; }                      // _eval.py:200-201
                const double len = sqrt((nx * nx + ny * ny) + nz * nz);              // :203-205
                nhx = nx / len; nhy = ny / len; nhz = nz / len;
            }
        }
        double sh = 0.0, st = 0.0, sy = 0.0, sz = 0.0;
        for (int j = tid; j < M; j += kHpBlock)
            if ((words[j >> 6] >> (j & 63)) & 1ull) {
                const int id = L[j];
                sh += LINE ? Y[id] * nhy + Z[id] * nhz : (X[id] * nhx + Y[id] * nhy) + Z[id] * nhz;   // :212
                st += Z[id] * sin_est + Y[id] * cos_est;                             // :222
                sy += Y[id]; sz += Z[id];
            }
        block_sum2<kHpWaves>(sh, st, red + HER_SUM);
        block_sum2<kHpWaves>(sy, sz, red + HER_YZ);
        const double mean = sh / (double)n_in;                                       // :214
        double ss = 0.0, dummy = 0.0;
        for (int j = tid; j < M; j += kHpBlock)
            if ((words[j >> 6] >> (j & 63)) & 1ull) {
                const int id = L[j];
                const double d = (LINE ? Y[id] * nhy + Z[id] * nhz : (X[id] * nhx + Y[id] * nhy) + Z[id] * nhz) - mean;
                ss += d * d;
            }
        block_sum2<kHpWaves>(ss, dummy, red + HER_DEV);
        if (tid == 0) {
            a.ransac_height[fc] = ransac_camera_height(bm);                          // :176-186
            a.model[4 * fc] = m0; a.model[4 * fc + 1] = m1; a.model[4 * fc + 2] = m2; a.model[4 * fc + 3] = m3;
            a.best_ic[fc] = best_ic; a.used[fc] = used; a.n_inliers[fc] = n_in;
            a.refined_normal[3 * fc] = degen ? nan("") : nhx; a.refined_normal[3 * fc + 1] = nhy; a.refined_normal[3 * fc + 2] = nhz;
            a.refined_pitch[fc] = asin(nhy);                                         // _eval.py:208 (n_y), _eval_line.py:209 (the y component)
            a.refined_mean[fc] = mean;
            a.refined_std[fc] = sqrt(ss / (double)n_in);                             // :215
            a.height_t_mean[fc] = degen ? nan("") : st / (double)n_in;               // :223
            a.sum_y[fc] = sy; a.sum_z[fc] = sz;
            a.status[fc] = degen ? MVOSR_ST_HP_REFINE_DEGENERATE : 0;
        }
        __syncthreads();                                                             // (the next case resets misc and reuses the reduction slots)
    }
}

}  // namespace mvosr

using namespace mvosr;

extern "C" {

size_t mvosr_height_pitch_eval_lds_bytes(int max_feat, int n_hyp, int model) {
    (void)model;                                                                     // (both models keep a hypothesis as one double4)
    const size_t mf = max_feat > 0 ? (size_t)max_feat : 0, mt = mf ? 2 * mf : 1;
    return hpeval_plan<size_t>(mf, mt, n_hyp > 0 ? (size_t)n_hyp : 0).total;
}

int mvosr_height_pitch_eval_batch(mvosr_ctx *ctx, const mvosr_batch *b, const mvosr_height_pitch_eval_params *p, const double *frame_prior,
                                  const int32_t *samples, const mvosr_height_pitch_eval_outputs *o) {
    if (!ctx || !b || !p || !frame_prior || !o) return set_error(MVOSR_ERR_ARG, "height_pitch_eval: null argument");
    if (!o->ransac_height || !o->model || !o->best_ic || !o->used || !o->n_selected || !o->n_inliers || !o->refined_normal ||
        !o->refined_pitch || !o->refined_mean || !o->refined_std || !o->height_t_mean || !o->sum_y || !o->sum_z || !o->status)
        return set_error(MVOSR_ERR_ARG, "height_pitch_eval: a required output is null");
    if (!b->feat_off || !b->feat_cnt || !b->x || !b->v || !b->z || !b->tri1_off || !b->tri1)
        return set_error(MVOSR_ERR_ARG, "height_pitch_eval: missing u (x) / v / depth (z) / tri1");
    if (p->model != MVOSR_HP_MODEL_PLANE && p->model != MVOSR_HP_MODEL_LINE) return set_error(MVOSR_ERR_ARG, "height_pitch_eval: unknown model %d", p->model);
    if (p->n_hyp < 1 || p->n_hyp > kHpeMaxHyp) return set_error(MVOSR_ERR_ARG, "height_pitch_eval: n_hyp must be in 1..%d", kHpeMaxHyp);
    if (p->n_cases < 1 || p->n_cases > kHpeMaxCases) return set_error(MVOSR_ERR_ARG, "height_pitch_eval: n_cases must be in 1..%d", kHpeMaxCases);
    if (p->cases_per_group < 0) return set_error(MVOSR_ERR_ARG, "height_pitch_eval: cases_per_group < 0");
    if (p->min_points < 3) return set_error(MVOSR_ERR_ARG, "height_pitch_eval: min_points < 3");
    if (b->max_feat < 0) return set_error(MVOSR_ERR_ARG, "height_pitch_eval: max_feat < 0");
    if (o->list_mask && o->list_stride < 0) return set_error(MVOSR_ERR_ARG, "height_pitch_eval: list_stride < 0");
    if (b->n_frames <= 0) return MVOSR_OK;
    int G = p->cases_per_group ? p->cases_per_group : kHpeDefaultGroup;
    if (G <= 0 || G > p->n_cases) G = p->n_cases;
    const int n_groups = (p->n_cases + G - 1) / G;
    if (b->n_frames > (int64_t)0x7fffffff / n_groups) return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch_eval: frames x groups exceeds a grid");
    const int64_t max_tri = b->max_feat > 0 ? 2 * (int64_t)b->max_feat : 1;
    if (b->max_feat > 65535 || 3 * max_tri > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch_eval: ids and list positions are 16-bit in LDS");
    const size_t lds = hpeval_plan<size_t>((size_t)b->max_feat, (size_t)max_tri, (size_t)p->n_hyp).total;
    if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch_eval: a frame of %d features needs %zu B of LDS (> %d)", b->max_feat, lds, ctx->max_lds_per_block);
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    const bool line = p->model == MVOSR_HP_MODEL_LINE;
    const void *fn = line ? reinterpret_cast<const void *>(height_pitch_eval_kernel<MVOSR_HP_MODEL_LINE>)
                          : reinterpret_cast<const void *>(height_pitch_eval_kernel<MVOSR_HP_MODEL_PLANE>);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    HpeArgs a = {};
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.u = b->x; a.v = b->v; a.depth = b->z;
    a.tri_off = b->tri1_off; a.tri = b->tri1; a.tri_cnt = b->tri1_cnt;
    a.focus = p->focus; a.cx = p->cx; a.cy = p->cy; a.min_points = p->min_points; a.n_hyp = p->n_hyp;
    a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri; a.n_cases = p->n_cases; a.cases_per_group = G; a.n_groups = n_groups;
    a.threshold = p->threshold; a.goal_fraction = p->goal_fraction; a.inlier_threshold = p->inlier_threshold;
    a.seed = p->seed; a.frame_base = p->frame_base; a.prior = frame_prior; a.samples = samples;
    a.ransac_height = o->ransac_height; a.model = o->model; a.best_ic = o->best_ic; a.used = o->used; a.n_selected = o->n_selected;
    a.n_inliers = o->n_inliers; a.refined_normal = o->refined_normal; a.refined_pitch = o->refined_pitch; a.refined_mean = o->refined_mean;
    a.refined_std = o->refined_std; a.height_t_mean = o->height_t_mean; a.sum_y = o->sum_y; a.sum_z = o->sum_z; a.status = o->status;
    a.list_mask = o->list_mask; a.list_stride = o->list_stride; a.point_list = o->point_list; a.hyp_counts = o->hyp_counts;
    const dim3 grid((unsigned)(b->n_frames * n_groups)), block(kHpBlock);
    if (line) hipLaunchKernelGGL(height_pitch_eval_kernel<MVOSR_HP_MODEL_LINE>, grid, block, lds, ctx_stream(ctx), a);
    else hipLaunchKernelGGL(height_pitch_eval_kernel<MVOSR_HP_MODEL_PLANE>, grid, block, lds, ctx_stream(ctx), a);
    return check_launch("height_pitch_eval_kernel");
}

}  // extern "C"
