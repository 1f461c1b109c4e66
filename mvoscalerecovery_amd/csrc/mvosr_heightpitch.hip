// mvosr_heightpitch.hip — the reference's per-frame camera-height and road-pitch estimator,
// /root/reference/src/calculate_height_pitch.py:62-204, one frame per workgroup in ONE launch:
//
//   back-projection (:67-68) -> per row of the triangulation n = A^-1 . 1, height, pitch (:77-93) -> the prior's window and
//   height > 0 (:111-112) -> the point list, three ids per kept row in row order (:114-116) -> get_pitch_ransac over the list
//   (:145; /root/reference/src/estimate_road_norm.py:66-70, thirdparty/Ransac/ransac.py:3-23) -> get_inliers over ALL points at
//   0.01 (:149-150) -> the RANSAC camera height (:154-166) -> the refinement: the plane through the first three inliers, its
//   pitch, mean and std of the inliers' distances, and the mean of z sin + y cos with the prior's angle (:178-204).
//
// The frame's points, its list, the hypotheses and the inlier mask live in LDS from the load to the last sum
// (mvosr_heightpitch_plan.hpp); the line RANSAC of :146 is only printed by the script and is not computed.  fp64, compiled with
// -ffp-contract=off; every sum is taken in a fixed order, so results are run-to-run identical and do not depend on the batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mvosr.h"
#include "mvosr_device.hpp"
#include "mvosr_ransac.hpp"
#include "mvosr_host.hpp"
#include "mvosr_heightpitch_plan.hpp"
#include "mvosr_heightpitch_pass.hpp"

namespace mvosr {

struct HpArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *u, *v, *depth;
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    double focus, cx, cy;
    int32_t min_points, n_hyp, max_feat, max_tri;
    double threshold, goal_fraction, inlier_threshold;
    uint64_t seed; int64_t frame_base;
    const double *prior;           // [F][4] window low / high in degrees, sin and cos of the prior
    const int32_t *triples;        // [F][H][3] list positions, or null: drawn
    double *ransac_height, *model; // [F], [F][4]
    int32_t *best_ic, *used, *n_selected, *n_inliers;
    double *refined_normal, *refined_pitch, *refined_mean, *refined_std, *height_t_mean;   // [F][3], [F] each
    int32_t *status;
    uint8_t *mask;                 // optional, laid out like depth
    int32_t *point_list;           // optional, at 3 * tri_off[f]
    int32_t *hyp_counts;           // optional [F][H]
};

__device__ __forceinline__ void hp_refuse(const HpArgs &a, int64_t f, int status, int n_selected) {
    const double q = nan("");
    a.status[f] = status;
    a.ransac_height[f] = q; a.refined_pitch[f] = q; a.refined_mean[f] = q; a.refined_std[f] = q; a.height_t_mean[f] = q;
    for (int k = 0; k < 4; ++k) a.model[4 * f + k] = q;
    for (int k = 0; k < 3; ++k) a.refined_normal[3 * f + k] = q;
    a.best_ic[f] = 0; a.used[f] = 0; a.n_selected[f] = n_selected; a.n_inliers[f] = 0;
}

__global__ __launch_bounds__(kHpBlock) void height_pitch_kernel(const HpArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int n = a.feat_cnt[f];
    const int64_t off = a.feat_off[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    if (n <= 0 || tn <= 0) { if (tid == 0) hp_refuse(a, f, MVOSR_ST_ERR_EMPTY, 0); return; }
    // more features or rows than the launch's LDS was sized for: refused, LDS untouched
    if (n > a.max_feat || tn > a.max_tri) { if (tid == 0) hp_refuse(a, f, MVOSR_ST_ERR_MASK, 0); return; }
    const int H = a.n_hyp;
    const auto lds = heightpitch_plan<uint32_t>((uint32_t)n, (uint32_t)tn, (uint32_t)H);
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
    const int M = hp_frame_pass(a, f, n, tn, off, tb, true, X, Y, Z, L, misc, sin_est, cos_est);   // steps (1)-(2), :62-116
    if (M < 0) {
        if (tid == 0) hp_refuse(a, f, misc[HM_BADID] ? MVOSR_ST_ERR_MASK : MVOSR_ST_ERR_SINGULAR, 0);
        return;
    }
    if (M < a.min_points) {                                                          // :140: the host carries the previous frame
        if (tid == 0) hp_refuse(a, f, MVOSR_ST_RS_FEW, M);
        return;
    }
    __syncthreads();

    // ---- the hypotheses' planes, one thread each (ransac.py:10-11, estimate_road_norm.py:13-15)
    {
        const uint64_t key = ransac_frame_key(a.seed, (uint64_t)(a.frame_base + f));
        for (int h = tid; h < H; h += kHpBlock) {
            int p0, p1, p2;
            if (a.triples) { const int32_t *t = a.triples + ((int64_t)f * H + h) * 3; p0 = t[0]; p1 = t[1]; p2 = t[2]; }
            else ransac_draw3(key, h, M, p0, p1, p2);
            // a sample that names a position outside the list, or one vertex twice, is spent: NaN plane, no inlier
            bool ok = ids_in_range(p0, p1, p2, M);
            int v0 = 0, v1 = 0, v2 = 0;
            if (ok) { v0 = L[p0]; v1 = L[p1]; v2 = L[p2]; ok = v0 != v1 && v0 != v2 && v1 != v2; }
            double4 m; m.x = m.y = m.z = m.w = nan("");
            if (ok) m = ransac_unit_plane(X, Y, Z, v0, v1, v2);
            mods[h] = m;
            cnts[h] = 0;
        }
    }
    __syncthreads();
    // ---- inlier counts over the list, repeats included (estimate_road_norm.py:17-18): the list's points in registers, the
    // hypotheses streamed from LDS (wave-uniform reads), ballot + popcount, one integer LDS add per wavefront
    ransac_count_resident<false, kHpPPT, 2, kHpBlock>(M, mods, cnts, H, a.threshold,
        [&](int j, double &x, double &y, double &z) { const int id = L[j]; x = X[id]; y = Y[id]; z = Z[id]; });
    __syncthreads();
    if (a.hyp_counts) for (int h = tid; h < H; h += kHpBlock) a.hyp_counts[(int64_t)f * H + h] = cnts[h];
    // ---- ransac.py:9-22 by wavefront 0, 64 hypotheses at a time: the first best, the stop at the first count above the goal
    if (wave == 0) {
        RansacReplay rp = {-1, 0, H, 0};
        ransac_replay(rp, cnts, 0, H, (double)M * a.goal_fraction);                  // the goal: estimate_road_norm.py:68
        if (lane == 0) {
            misc[HM_BEST] = rp.best; misc[HM_BESTIC] = rp.best_ic; misc[HM_USED] = rp.used;
            if (rp.best >= 0) {
                const double4 bm = ransac_sign_rule(mods[rp.best]);                  // :157-159
                red[HR_MODEL] = bm.x; red[HR_MODEL + 1] = bm.y; red[HR_MODEL + 2] = bm.z; red[HR_MODEL + 3] = bm.w;
            }
        }
    }
    __syncthreads();
    if (misc[HM_BEST] < 0) {                                                         // no hypothesis with an inlier: no model (the script would fail at :154)
        if (tid == 0) { hp_refuse(a, f, MVOSR_ST_RS_FEW, M); a.used[f] = misc[HM_USED]; }
        return;
    }
    const double m0 = red[HR_MODEL], m1 = red[HR_MODEL + 1], m2 = red[HR_MODEL + 2], m3 = red[HR_MODEL + 3];
    // ---- get_inliers over every feature (:149, estimate_road_norm.py:71-78): one ballot per 64 features
    const int nw = (n + kWave - 1) / kWave;
    for (int w = wave; w < nw; w += kHpWaves) {
        const int i = w * kWave + lane;
        const int ic = min(i, n - 1);
        const bool inl = i < n && fabs(((X[ic] * m0 + Y[ic] * m1) + Z[ic] * m2) + m3) < a.inlier_threshold;
        const unsigned long long bal = __ballot(inl);
        if (lane == 0) words[w] = bal;
        if (a.mask && i < n) a.mask[off + i] = inl ? 1 : 0;
    }
    __syncthreads();
    if (wave == 0) {
        int cnt = 0;
        for (int w = lane; w < nw; w += kWave) cnt += __popcll(words[w]);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            misc[HM_NIN] = cnt;
            int found = 0;
            for (int w = 0; w < nw && found < 3; ++w) {                              // inliers[:3], the sample `estimate` reads (:178)
                unsigned long long bits = words[w];
                while (bits && found < 3) { misc[HM_I0 + found++] = w * kWave + (int)__ffsll((long long)bits) - 1; bits &= bits - 1ull; }
            }
        }
    }
    __syncthreads();
    const int n_in = misc[HM_NIN];
    // ---- the refinement (:178-204)
    double nhx = nan(""), nhy = nan(""), nhz = nan("");
    if (n_in >= 3) {
        const int i0 = misc[HM_I0], i1 = misc[HM_I0 + 1], i2 = misc[HM_I0 + 2];
        double nx, ny, nz;
        ransac_edge_cross(X[i0], Y[i0], Z[i0], X[i1], Y[i1], Z[i1], X[i2], Y[i2], Z[i2], nx, ny, nz);
        if (ny < 0.0) { nx = -nx; ny = -ny; nz = -nz; }                              // :180-181
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);                      // :183-185
        nhx = nx / len; nhy = ny / len; nhz = nz / len;
    }
    double sh = 0.0, st = 0.0;
    for (int i = tid; i < n; i += kHpBlock)
        if ((words[i >> 6] >> (i & 63)) & 1ull) {
            sh += (X[i] * nhx + Y[i] * nhy) + Z[i] * nhz;                            // :192
            st += Z[i] * sin_est + Y[i] * cos_est;                                   // :202
        }
    block_sum2<kHpWaves>(sh, st, red + HR_SUM);
    const double mean = sh / (double)n_in;                                           // :194
    double ss = 0.0, dummy = 0.0;
    for (int i = tid; i < n; i += kHpBlock)
        if ((words[i >> 6] >> (i & 63)) & 1ull) { const double d = ((X[i] * nhx + Y[i] * nhy) + Z[i] * nhz) - mean; ss += d * d; }
    block_sum2<kHpWaves>(ss, dummy, red + HR_DEV);
    if (tid == 0) {
        a.ransac_height[f] = ransac_camera_height(make_double4(m0, m1, m2, m3));     // :156-166
        a.model[4 * f] = m0; a.model[4 * f + 1] = m1; a.model[4 * f + 2] = m2; a.model[4 * f + 3] = m3;
        a.best_ic[f] = misc[HM_BESTIC]; a.used[f] = misc[HM_USED]; a.n_selected[f] = M; a.n_inliers[f] = n_in;
        a.refined_normal[3 * f] = nhx; a.refined_normal[3 * f + 1] = nhy; a.refined_normal[3 * f + 2] = nhz;
        a.refined_pitch[f] = asin(nhy);                                              // :188
        a.refined_mean[f] = mean;
        a.refined_std[f] = sqrt(ss / (double)n_in);                                  // :195
        a.height_t_mean[f] = st / (double)n_in;                                      // :203
        a.status[f] = 0;
    }
}

}  // namespace mvosr

using namespace mvosr;

extern "C" {

size_t mvosr_height_pitch_lds_bytes(int max_feat, int n_hyp) {
    const size_t mf = max_feat > 0 ? (size_t)max_feat : 0, mt = mf ? 2 * mf : 1;
    return heightpitch_plan<size_t>(mf, mt, n_hyp > 0 ? (size_t)n_hyp : 0).total;
}

int mvosr_height_pitch_batch(mvosr_ctx *ctx, const mvosr_batch *b, const mvosr_height_pitch_params *p, const double *frame_prior,
                             const int32_t *triples, const mvosr_height_pitch_outputs *o) {
    if (!ctx || !b || !p || !frame_prior || !o) return set_error(MVOSR_ERR_ARG, "height_pitch: null argument");
    if (!o->ransac_height || !o->model || !o->best_ic || !o->used || !o->n_selected || !o->n_inliers || !o->refined_normal ||
        !o->refined_pitch || !o->refined_mean || !o->refined_std || !o->height_t_mean || !o->status)
        return set_error(MVOSR_ERR_ARG, "height_pitch: a required output is null");
    if (!b->feat_off || !b->feat_cnt || !b->x || !b->v || !b->z || !b->tri1_off || !b->tri1)
        return set_error(MVOSR_ERR_ARG, "height_pitch: missing u (x) / v / depth (z) / tri1");
    if (p->n_hyp < 1 || p->n_hyp > kHpMaxHyp) return set_error(MVOSR_ERR_ARG, "height_pitch: n_hyp must be in 1..%d", kHpMaxHyp);
    if (p->min_points < 3) return set_error(MVOSR_ERR_ARG, "height_pitch: min_points < 3");
    if (b->max_feat < 0) return set_error(MVOSR_ERR_ARG, "height_pitch: max_feat < 0");
    if (b->n_frames <= 0) return MVOSR_OK;
    const int64_t max_tri = b->max_feat > 0 ? 2 * (int64_t)b->max_feat : 1;
    if (b->max_feat > 65535 || 3 * max_tri > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch: ids and list positions are 16-bit in LDS");
    const size_t lds = heightpitch_plan<size_t>((size_t)b->max_feat, (size_t)max_tri, (size_t)p->n_hyp).total;
    if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch: a frame of %d features needs %zu B of LDS (> %d)", b->max_feat, lds, ctx->max_lds_per_block);
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(height_pitch_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    HpArgs a = {};
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.u = b->x; a.v = b->v; a.depth = b->z;
    a.tri_off = b->tri1_off; a.tri = b->tri1; a.tri_cnt = b->tri1_cnt;
    a.focus = p->focus; a.cx = p->cx; a.cy = p->cy; a.min_points = p->min_points; a.n_hyp = p->n_hyp;
    a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri;
    a.threshold = p->threshold; a.goal_fraction = p->goal_fraction; a.inlier_threshold = p->inlier_threshold;
    a.seed = p->seed; a.frame_base = p->frame_base; a.prior = frame_prior; a.triples = triples;
    a.ransac_height = o->ransac_height; a.model = o->model; a.best_ic = o->best_ic; a.used = o->used; a.n_selected = o->n_selected;
    a.n_inliers = o->n_inliers; a.refined_normal = o->refined_normal; a.refined_pitch = o->refined_pitch; a.refined_mean = o->refined_mean;
    a.refined_std = o->refined_std; a.height_t_mean = o->height_t_mean; a.status = o->status;
    a.mask = o->mask; a.point_list = o->point_list; a.hyp_counts = o->hyp_counts;
    hipLaunchKernelGGL(height_pitch_kernel, dim3((unsigned)b->n_frames), dim3(kHpBlock), lds, ctx_stream(ctx), a);
    return check_launch("height_pitch_kernel");
}

}  // extern "C"
