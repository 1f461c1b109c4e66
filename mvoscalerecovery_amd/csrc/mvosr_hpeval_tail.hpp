// mvosr_hpeval_tail.hpp — what height_pitch_eval_budgets_kernel (mvosr_hpeval_budgets.hip) does with a best model,
// /root/reference/src/calculate_height_pitch_eval.py:167-225 and the same lines of calculate_height_pitch_eval_line.py: the sign rule,
// the inliers among the LIST at inlier_threshold, the refinement's sample (the first K set positions) and its degenerate test, the
// refinement, the three block sums in their fixed order.  The budgets kernel runs it once per distinct best model among a case's
// checkpoints.
// A SECOND COPY of height_pitch_eval_kernel's per-case tail (mvosr_hpeval.hip, after the tile loop), statement for statement:
// calling this function from that kernel moved its register count (151 / 153 -> 155 / 157 VGPRs), so that file stays as it
// was.  A change to either copy goes into both; tests/test_gpu_hpeval_budgets.py compares the two kernels' bytes.
// Device code only; included after mvosr_device.hpp, mvosr_ransac.hpp, mvosr_hpeval_plan.hpp and mvosr_heightpitch_pass.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace mvosr {

// what a writing thread hands to `emit`: every output of a fitted (frame, case) but best_ic and used, which the replay owns
struct HpeTail {
    double ransac_height, m0, m1, m2, m3;
    int n_inliers;
    double nhx, nhy, nhz, refined_pitch, refined_mean, refined_std, height_t_mean, sum_y, sum_z;
    int status;
};

// raw: the best model as the hypothesis tile holds it.  X, Y, Z, L: the frame and its list of M entries (nw words of 64);
// words, misc, red: the plan's regions.  Every thread ends with the same values — the block sums hand the totals to every thread —
// and emit(const HpeTail &) is called by threads 0 .. n_emit - 1 (the evaluation kernel's thread 0 writes them).  Holds barriers: every thread of the
// workgroup calls it; the caller places a barrier after it before misc, words or the reduction slots are written again.
template <bool LINE, typename Emit>
__device__ __forceinline__ void hpe_case_tail(const double4 raw, int M, int nw, const double *X, const double *Y, const double *Z, const uint16_t *L,
                                              unsigned long long *words, int *misc, double *red, double inlier_threshold, double sin_est,
                                              double cos_est, int n_emit, Emit emit) {
    constexpr int K = LINE ? 2 : 3;                                                  // the sample's size
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    // :175-180: plane — flipped on n_y < 0; line — (a, b) and h_bar flipped on b < 0: the model's second slot either way
    const double4 bm = ransac_sign_rule(raw);
    const double m0 = bm.x, m1 = bm.y, m2 = bm.z, m3 = bm.w;
    // ---- get_inliers over the LIST (:167-169, estimate_road_norm.py:71-78): one ballot per 64 list positions
    for (int w = wave; w < nw; w += kHpWaves) {
        const int j = w * kWave + lane;
        const int id = L[min(j, M - 1)];
        const double r = LINE ? (Y[id] * m0 + Z[id] * m1) + m3 : ((X[id] * m0 + Y[id] * m1) + Z[id] * m2) + m3;
        const bool inl = j < M && fabs(r) < inlier_threshold;
        const unsigned long long bal = __ballot(inl);
        if (lane == 0) words[w] = bal;
    }
    __syncthreads();
    if (wave == 0) {
        int cnt = 0;
        for (int w = lane; w < nw; w += kWave) cnt += __popcll(words[w]);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            misc[HM_NIN] = cnt;
            int found = 0;
            for (int w = 0; w < nw && found < K; ++w) {                              // inliers[:3] / [:2], the sample `estimate` reads (:198)
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
            if (nz < 0.0) { ny = -ny; nz = -nz; }                                    // _eval_line.py:201-202: the z component
            const double len = sqrt(ny * ny + nz * nz);                              // :204-206
            nhy = ny / len; nhz = nz / len;
        } else {
            const int i2 = misc[HM_I0 + 2];
            double nx, ny, nz;
            ransac_edge_cross(X[i0], Y[i0], Z[i0], X[i1], Y[i1], Z[i1], X[i2], Y[i2], Z[i2], nx, ny, nz);
            if (ny < 0.0) { nx = -nx; ny = -ny; nz = -nz; }                          // _eval.py:200-201
            const double len = sqrt((nx * nx + ny * ny) + nz * nz);                  // :203-205
            nhx = nx / len; nhy = ny / len; nhz = nz / len;
        }
    }
    double sh = 0.0, st = 0.0, sy = 0.0, sz = 0.0;
    for (int j = tid; j < M; j += kHpBlock)
        if ((words[j >> 6] >> (j & 63)) & 1ull) {
            const int id = L[j];
            sh += LINE ? Y[id] * nhy + Z[id] * nhz : (X[id] * nhx + Y[id] * nhy) + Z[id] * nhz;   // :212
            st += Z[id] * sin_est + Y[id] * cos_est;                                 // :222
            sy += Y[id]; sz += Z[id];
        }
    block_sum2<kHpWaves>(sh, st, red + HER_SUM);
    block_sum2<kHpWaves>(sy, sz, red + HER_YZ);
    const double mean = sh / (double)n_in;                                           // :214
    double ss = 0.0, dummy = 0.0;
    for (int j = tid; j < M; j += kHpBlock)
        if ((words[j >> 6] >> (j & 63)) & 1ull) {
            const int id = L[j];
            const double d = (LINE ? Y[id] * nhy + Z[id] * nhz : (X[id] * nhx + Y[id] * nhy) + Z[id] * nhz) - mean;
            ss += d * d;
        }
    block_sum2<kHpWaves>(ss, dummy, red + HER_DEV);
    if (tid < n_emit) {
        HpeTail t;
        t.ransac_height = ransac_camera_height(bm);                                  // :176-186
        t.m0 = m0; t.m1 = m1; t.m2 = m2; t.m3 = m3;
        t.n_inliers = n_in;
        t.nhx = degen ? nan("") : nhx; t.nhy = nhy; t.nhz = nhz;
        t.refined_pitch = asin(nhy);                                                 // _eval.py:208 (n_y), _eval_line.py:209 (the y component)
        t.refined_mean = mean;
        t.refined_std = sqrt(ss / (double)n_in);                                     // :215
        t.height_t_mean = degen ? nan("") : st / (double)n_in;                       // :223
        t.sum_y = sy; t.sum_z = sz;
        t.status = degen ? MVOSR_ST_HP_REFINE_DEGENERATE : 0;
        emit(t);
    }
}

}  // namespace mvosr
