// mvosr_heightpitch_pass.hpp — what height_pitch_kernel (mvosr_heightpitch.hip) and height_pitch_eval_kernel (mvosr_hpeval.hip)
// do once per frame, /root/reference/src/calculate_height_pitch.py:62-116 (its _eval copies: the same lines, 19 further down):
// back-projection, the rows' normals, the prior's window and height > 0, and the point list as 16-bit vertex ids in row order.
// Device code only; included after mvosr_device.hpp, mvosr_ransac.hpp and a plan header that defines kHpWaves and the HM_* slots.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace mvosr {

constexpr int kHpBlock = kHpWaves * kWave;
constexpr int kHpPPT = 8;               // list points a thread holds in registers per chunk (chunks of 4096 entries)
constexpr double kHpPi = 3.1415926;     // the script's constant (:63, :91)
constexpr double kHpBand = 1e-12;       // |n_y/|n| - edge| within this: the script's own expression decides

// The value of n_y/|n| at which asin(.) * 180 / 3.1415926 crosses `deg`; -2 / 2 where every / no value lies above it.  Only
// compared against from further than kHpBand away (the device sin never decides).
__device__ __forceinline__ double hp_edge(double deg) {
    const double t = deg * kHpPi / 180.0;
    if (t <= -1.58) return -2.0;
    if (t >= 1.58) return 2.0;
    return sin(fmin(fmax(t, -1.5707963267948966), 1.5707963267948966));
}

// Steps (1)-(2) of a frame of n features and tn rows that has passed the kernels' size guards.  Fills X, Y, Z [n] and the list L;
// `a` needs u, v, depth, cx, cy, focus, prior, tri and (optional) point_list — written only where write_list.  Returns the list's
// length M = 3 * kept rows, or -1 where a row names a vertex outside the frame or is singular (misc[HM_BADID] / misc[HM_SINGULAR]
// say which).  Holds two barriers: every thread of the workgroup calls it.  The caller places a barrier before it reads L.
template <typename Args>
__device__ __forceinline__ int hp_frame_pass(const Args &a, int64_t f, int n, int tn, int64_t off, int64_t tb, bool write_list,
                                             double *X, double *Y, double *Z, uint16_t *L, int *misc, double &sin_est, double &cos_est) {
    const int tid = threadIdx.x, lane = lane_id();
    if (tid < HM_N) misc[tid] = 0;
    for (int i = tid; i < n; i += kHpBlock) {
        const double d = a.depth[off + i];
        X[i] = d * (a.u[off + i] - a.cx) / a.focus;                                  // :67
        Y[i] = d * (a.v[off + i] - a.cy) / a.focus;                                  // :68
        Z[i] = d;
    }
    const double *pr = a.prior + 4 * f;
    const double lo_deg = pr[0], hi_deg = pr[1];
    sin_est = pr[2]; cos_est = pr[3];
    const bool prior_ok = lo_deg == lo_deg && hi_deg == hi_deg;                      // (a NaN prior keeps no row, as the script's comparisons)
    const double s_lo = hp_edge(lo_deg), s_hi = hp_edge(hi_deg);
    __syncthreads();

    // ---- the rows (:77-116), wavefront by wavefront over contiguous row segments so that the list comes out in row order
    int s0, s1;
    ordered_segment(tn, kHpBlock, s0, s1);                                           // (tn <= 21845: at most 43 trips, one bit each)
    unsigned long long mine = 0ull;
    int c = 0;
    {
        int j = 0;
        for (int t0 = s0; t0 < s1; t0 += kWave, ++j) {
            const int t = t0 + lane;
            bool kp = false;
            if (t < s1) {
                const TriIds q = load_tri(a.tri + 3 * tb, t);
                if (!ids_in_range(q.a, q.b, q.c, n)) misc[HM_BADID] = 1;
                else {
                    double nx, ny, nz;
                    if (!plane_normal(X[q.a], Y[q.a], Z[q.a], X[q.b], Y[q.b], Z[q.b], X[q.c], Y[q.c], Z[q.c], nx, ny, nz)) misc[HM_SINGULAR] = 1;   // :83-84
                    const double len = sqrt((nx * nx + ny * ny) + nz * nz);          // :85-86
                    double height = 1.0 / len;
                    if (ny < 0.0) { ny = -ny; height = -height; }                    // :87-89
                    const double mu = -ny / len;                                     // :90, the sine of the pitch
                    bool in;
                    if (fabs(mu - s_lo) > kHpBand && fabs(mu - s_hi) > kHpBand) in = mu > s_lo && mu < s_hi;
                    else {
                        const double pitch_deg = asin(mu) * 180.0 / kHpPi;           // :90-91
                        in = pitch_deg > lo_deg && pitch_deg < hi_deg;               // :111
                    }
                    kp = prior_ok && in && height > 0.0;                             // :112
                }
            }
            const unsigned long long m = __ballot(kp);
            if (kp) mine |= 1ull << j;
            c += __popcll(m);
        }
    }
    int base, K;
    ordered_prefix<kHpWaves>(misc + HM_CW, c, base, K);
    if (misc[HM_BADID] || misc[HM_SINGULAR]) return -1;
    {
        int j = 0;
        for (int t0 = s0; t0 < s1; t0 += kWave, ++j) {
            const int t = t0 + lane;
            const bool kp = (mine >> j) & 1ull;
            const int pos = 3 * ordered_rank(kp, base);
            if (kp) {
                const TriIds q = load_tri(a.tri + 3 * tb, t);
                L[pos] = (uint16_t)q.a; L[pos + 1] = (uint16_t)q.b; L[pos + 2] = (uint16_t)q.c;   // :114-116
                if (write_list && a.point_list) { int32_t *pl = a.point_list + 3 * tb + pos; pl[0] = q.a; pl[1] = q.b; pl[2] = q.c; }
            }
        }
    }
    return 3 * K;                                                                    // point_selected.shape[0], :135
}

}  // namespace mvosr
