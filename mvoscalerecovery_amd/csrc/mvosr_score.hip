// mvosr_score.hip — the tail of the reference's ten-run workflow (/root/reference/test_off_line.sh:11-23) on the device: the paths
// of C cases (src/main_offline.py:100-119), the KITTI segment errors of script/evaluate_vo.py:5-96 for every case against one
// ground-truth path, and script/transformation.py:23-32 (pose2motion) with what script/change_scale.py:12-18 and
// script/calculate_speed.py:8-11 do to its output.  fp64 throughout; the file is built with -ffp-contract=off, so every operation
// written here is an IEEE operation of its own and every sum below has the order it is written in.
//
// A pose or a motion is a row of 12 doubles, the upper 3 x 4 of the affine matrix [R t; 0 1] (arithmetic: mvosr_score_math.hpp).
//   product    (A B)[r][j] = ((A[r][0] B[0][j] + A[r][1] B[1][j]) + A[r][2] B[2][j]) + A[r][3] B[3][j] — k ascending, the fourth term
//              with B's last row (0 0 0 1) written out, as the reference's 4 x 4 product has it.
//   inverse    of the affine matrix as it is (integrated rotations drift from orthonormal, the reference's .I inverts them as they
//              are): R^-1 = adj(R) / det(R), cofactors a*b - c*d, det = (R00 C00 + R01 C10) + R02 C20 by the first row; then
//              -(R^-1 t), each entry the k-ascending sum, negated.
//
// paths_kernel         one wavefront per case; lane r < 3 carries row r of the pose through the chain pose = pose * step, strictly
//                      left to right (row r of the product needs row r of the pose only: no cross-lane traffic).  The steps are
//                      uniform over the lanes: all 64 lanes stage kScoreChunk of them through LDS, the translations multiplied by
//                      the case's scale there (one rounding, before the chain, as get_path scales the motions in place), and write
//                      the chunk's poses back out together.
// segment_table_kernel one workgroup: the step norms in parallel, their running sum by one lane through LDS (left to right), then
//                      a binary search per (first, length) — dist never decreases, so it finds what the reference's scan finds —
//                      and the ground truth's own delta inv(G_first) G_last per segment, as a sum hi + lo of two doubles.
// score_cases_kernel   one workgroup per case; a segment's error in double-double (mvosr_score_math.hpp says why), rounded once
//                      in front of acos and sqrt; kScoreFirsts firsts (x 8 lengths) at a time into LDS, then sixteen lanes — 8 lengths
//                      x {rotation, translation} — add the chunk to their running sums in ascending first, as Python's sum() does.
//                      No floating-point atomics anywhere: the same bytes every run.
// pose2motion_kernel   one lane per (case, frame): inv(P_i) P_{i+1}, its translation's norm, and optionally change_scale's
//                      re-scaling (speed * t) / (norm + 0.00001).
#include "mvosr_device.hpp"
#include "mvosr_host.hpp"
#include "mvosr_score_math.hpp"

#include <math.h>

namespace mvosr {

constexpr int kScoreLengths = MVOSR_SCORE_LENGTHS;   // 100 .. 800 m (evaluate_vo.py:46)
constexpr int kScoreStep = MVOSR_SCORE_STEP;         // a first frame every 10 (evaluate_vo.py:45)
constexpr int kScoreChunk = 128;                     // steps staged per round of paths_kernel: 12 KiB in, 12 KiB out
constexpr int kScoreFirsts = 128;                    // firsts per round of score_cases_kernel: 2 x 8 KiB
constexpr int kScoreBlock = 256;
constexpr int kDistChunk = 1024;                     // norms per round of the running sum

// ---- paths ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void paths_kernel(int64_t n, const double *motions, int64_t case_stride, const double *scales, double *poses) {
    __shared__ double step[kScoreChunk * 12];
    __shared__ double out[kScoreChunk * 12];
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    double *P = poses + c * (n + 1) * 12;
    const double *S = scales ? scales + c * n : nullptr;
    const double *M = motions + c * case_stride;
    double row[4] = {lane == 0 ? 1.0 : 0.0, lane == 1 ? 1.0 : 0.0, lane == 2 ? 1.0 : 0.0, 0.0};
    if (lane < 12) P[lane] = (lane == 0 || lane == 5 || lane == 10) ? 1.0 : 0.0;
    for (int64_t i0 = 0; i0 < n; i0 += kScoreChunk) {
        const int m = (int)((n - i0) < (int64_t)kScoreChunk ? (n - i0) : (int64_t)kScoreChunk);
        for (int k = lane; k < m * 12; k += kWave) {
            double v = M[i0 * 12 + k];
            if (S && (k & 3) == 3) v = v * S[i0 + k / 12];
            step[k] = v;
        }
        __syncthreads();
        if (lane < 3) {
            for (int i = 0; i < m; ++i) {
                double next[4];
                pose_row_mul(row, &step[i * 12], next);
                for (int j = 0; j < 4; ++j) { row[j] = next[j]; out[i * 12 + 4 * lane + j] = next[j]; }
            }
        }
        __syncthreads();
        for (int k = lane; k < m * 12; k += kWave) P[(i0 + 1) * 12 + k] = out[k];
    }
}

// ---- the segment table ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScoreBlock) void segment_table_kernel(int64_t n_poses, const double *gt, double *dist, int32_t *last,
                                                                    double *gdelta, int32_t *status) {
    __shared__ double chunk[kDistChunk];
    __shared__ double carry;
    __shared__ int singular;
    const int t = threadIdx.x;
    if (t == 0) { carry = 0.0; singular = 0; dist[0] = 0.0; }
    __syncthreads();
    // dist[i] = dist[i - 1] + |t[i - 1] - t[i]|  (evaluate_vo.py:5-13)
    for (int64_t i0 = 1; i0 < n_poses; i0 += kDistChunk) {
        const int m = (int)((n_poses - i0) < (int64_t)kDistChunk ? (n_poses - i0) : (int64_t)kDistChunk);
        for (int k = t; k < m; k += kScoreBlock) {
            const double *a = gt + (i0 + k - 1) * 12, *b = a + 12;
            chunk[k] = norm3(a[3] - b[3], a[7] - b[7], a[11] - b[11]);
        }
        __syncthreads();
        if (t == 0) {
            double d = carry;
            for (int k = 0; k < m; ++k) { d = d + chunk[k]; chunk[k] = d; }
            carry = d;
        }
        __syncthreads();
        for (int k = t; k < m; k += kScoreBlock) dist[i0 + k] = chunk[k];
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    // last = the first i >= first with dist[i] > dist[first] + length, else -1 (:15-19); the comparison is strict
    const int64_t n_first = (n_poses + kScoreStep - 1) / kScoreStep;
    for (int64_t s = t; s < n_first * kScoreLengths; s += kScoreBlock) {
        const int64_t first = (s / kScoreLengths) * kScoreStep;
        const double limit = dist[first] + (double)(100 * (int)(s % kScoreLengths + 1));
        int64_t lo = first, hi = n_poses;                 // dist[lo .. hi): the answer is the first index above the limit
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (dist[mid] > limit) hi = mid; else lo = mid + 1;
        }
        const bool found = lo < n_poses;
        last[s] = found ? (int32_t)lo : -1;
        PoseDD g;
        if (found) {
            const Pose a = pose_load(gt + first * 12);
            if (pose_rotation_is_zero(a)) singular = 1;
            g = ground_delta(a, pose_load(gt + lo * 12));
        } else {
            for (int k = 0; k < 12; ++k) g.m[k] = {__longlong_as_double(0x7ff8000000000000ll), 0.0};
        }
        for (int k = 0; k < 12; ++k) { gdelta[s * 24 + k] = g.m[k].hi; gdelta[s * 24 + 12 + k] = g.m[k].lo; }
    }
    __syncthreads();
    if (t == 0) status[0] = singular ? MVOSR_ST_ERR_SINGULAR : 0;
}

// ---- segment errors of C cases -------------------------------------------------------------------------------------------------------
struct ScoreArgs {
    int64_t n_cases, rows, n_first;
    const double *paths;         // [C][rows][12]
    const int32_t *last;         // [n_first][8]
    const double *gdelta;        // [n_first][8][24]: hi, lo
    double *r_seg, *t_seg;       // optional [C][n_first][8]
    double *means;               // [C][2][8]: rotation (rad / m), translation
    int32_t *counts;             // [C][8]
    int32_t *status;             // [C]
};

__global__ __launch_bounds__(kScoreBlock) void score_cases_kernel(ScoreArgs a) {
    __shared__ double err[2][kScoreFirsts * kScoreLengths];
    __shared__ unsigned char has[kScoreFirsts * kScoreLengths];
    __shared__ int flag;
    const int64_t c = blockIdx.x;
    const int t = threadIdx.x;
    const double *P = a.paths + c * a.rows * 12;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (t == 0) flag = 0;
    double sum = 0.0;            // lanes 0..15: quantity t / 8 of length t % 8
    int count = 0;
    __syncthreads();
    for (int64_t f0 = 0; f0 < a.n_first; f0 += kScoreFirsts) {
        const int m = (int)((a.n_first - f0) < (int64_t)kScoreFirsts ? (a.n_first - f0) : (int64_t)kScoreFirsts);
        for (int k = t; k < m * kScoreLengths; k += kScoreBlock) {
            const int64_t s = f0 * kScoreLengths + k;
            const int64_t first = (s / kScoreLengths) * kScoreStep, lst = a.last[s];
            double r = nan, tr = nan;
            if (lst >= 0) {
                if (lst >= a.rows || first >= a.rows) {
                    atomicOr(&flag, 2);                                                     // the path is shorter than the ground truth
                } else {
                    bool zero_block;
                    const double length = (double)(100 * (int)(s % kScoreLengths + 1));
                    segment_error(pose_load(P + first * 12), pose_load(P + lst * 12), pose_join(a.gdelta + s * 24, a.gdelta + s * 24 + 12), length, &r, &tr, &zero_block);
                    if (zero_block) atomicOr(&flag, 1);
                }
            }
            err[0][k] = r;
            err[1][k] = tr;
            has[k] = lst >= 0;
            if (a.r_seg) a.r_seg[c * a.n_first * kScoreLengths + s] = r;
            if (a.t_seg) a.t_seg[c * a.n_first * kScoreLengths + s] = tr;
        }
        __syncthreads();
        if (t < 2 * kScoreLengths) {
            const int li = t % kScoreLengths;
            const double *e = err[t / kScoreLengths];
            for (int f = 0; f < m; ++f)
                if (has[f * kScoreLengths + li]) { sum = sum + e[f * kScoreLengths + li]; ++count; }
        }
        __syncthreads();
    }
    if (t < 2 * kScoreLengths) {
        a.means[c * 2 * kScoreLengths + t] = count > 0 ? sum / (double)count : nan;
        if (t < kScoreLengths) a.counts[c * kScoreLengths + t] = count;
    }
    if (t == 0) a.status[c] = (flag & 2) ? MVOSR_ST_ERR_MASK : (flag & 1) ? MVOSR_ST_ERR_SINGULAR : 0;
}

// ---- pose2motion, calculate_speed, change_scale ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kScoreBlock) void pose2motion_kernel(int64_t n_cases, int64_t n, const double *poses, const double *speed,
                                                                   double *motions, double *norms, int *singular) {
    const int64_t i = (int64_t)blockIdx.x * kScoreBlock + threadIdx.x;
    const int64_t c = blockIdx.y;
    if (i >= n) return;
    const double *P = poses + (c * (n + 1) + i) * 12;
    const Pose a = pose_load(P);
    if (pose_rotation_is_zero(a)) atomicOr(&singular[c], (int)MVOSR_ST_ERR_SINGULAR);
    Pose m = pose_mul(pose_inverse(a), pose_load(P + 12));                                  // transformation.py:29
    const double len = norm3(m.m[3], m.m[7], m.m[11]);                                      // calculate_speed.py:9-11
    if (speed) {                                                                            // change_scale.py:15-17
        const double s = speed[i], d = len + 0.00001;
        for (int r = 0; r < 3; ++r) m.m[4 * r + 3] = (s * m.m[4 * r + 3]) / d;
    }
    if (motions)
        for (int k = 0; k < 12; ++k) motions[(c * n + i) * 12 + k] = m.m[k];
    if (norms) norms[c * n + i] = len;
}

}  // namespace mvosr

using namespace mvosr;

extern "C" int64_t mvosr_score_firsts(int64_t n_poses) { return n_poses <= 0 ? 0 : (n_poses + kScoreStep - 1) / kScoreStep; }

extern "C" int mvosr_paths_batch(mvosr_ctx *ctx, int64_t n, int64_t n_cases, const double *motions, int64_t case_stride,
                                 const double *scales, double *poses) {
    if (!ctx || !poses || (n > 0 && !motions)) return set_error(MVOSR_ERR_ARG, "paths_batch: null argument");
    if (n < 0 || n_cases < 1) return set_error(MVOSR_ERR_ARG, "paths_batch: n < 0 or fewer than one case");
    if (case_stride != 0 && case_stride < n * 12) return set_error(MVOSR_ERR_ARG, "paths_batch: case_stride is 0 (shared motions) or at least 12 n");
    if (n_cases > (int64_t)INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "paths_batch: more than 2^31-1 cases in one launch");
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(paths_kernel, dim3((unsigned)n_cases), dim3(kWave), 0, ctx_stream(ctx), n, motions, case_stride, scales, poses);
    return check_launch("paths_kernel");
}

extern "C" int mvosr_segment_table(mvosr_ctx *ctx, int64_t n_poses, const double *poses_gt, double *dist, int32_t *last, double *gdelta,
                                   int32_t *status) {
    if (!ctx || !poses_gt || !dist || !last || !gdelta || !status) return set_error(MVOSR_ERR_ARG, "segment_table: null argument");
    if (n_poses < 1) return set_error(MVOSR_ERR_ARG, "segment_table: a path has at least one pose");
    if (n_poses > (int64_t)INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "segment_table: more than 2^31-1 poses");
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(segment_table_kernel, dim3(1), dim3(kScoreBlock), 0, ctx_stream(ctx), n_poses, poses_gt, dist, last, gdelta, status);
    return check_launch("segment_table_kernel");
}

extern "C" int mvosr_score_cases_batch(mvosr_ctx *ctx, int64_t n_cases, int64_t rows, const double *paths, int64_t n_first,
                                       const int32_t *last, const double *gdelta, double *r_seg, double *t_seg, double *means,
                                       int32_t *counts, int32_t *status) {
    if (!ctx || !paths || !means || !counts || !status || (n_first > 0 && (!last || !gdelta)))
        return set_error(MVOSR_ERR_ARG, "score_cases_batch: null argument");
    if (n_cases < 1 || rows < 1 || n_first < 0) return set_error(MVOSR_ERR_ARG, "score_cases_batch: fewer than one case or pose, or a negative table");
    if (n_cases > (int64_t)INT32_MAX || n_first > (int64_t)INT32_MAX / kScoreLengths)
        return set_error(MVOSR_ERR_TOO_LARGE, "score_cases_batch: more than 2^31-1 cases or segments in one launch");
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    ScoreArgs a = {};
    a.n_cases = n_cases; a.rows = rows; a.n_first = n_first; a.paths = paths; a.last = last; a.gdelta = gdelta;
    a.r_seg = r_seg; a.t_seg = t_seg; a.means = means; a.counts = counts; a.status = status;
    hipLaunchKernelGGL(score_cases_kernel, dim3((unsigned)n_cases), dim3(kScoreBlock), 0, ctx_stream(ctx), a);
    return check_launch("score_cases_kernel");
}

extern "C" int mvosr_pose2motion_batch(mvosr_ctx *ctx, int64_t n_cases, int64_t n, const double *poses, const double *speed,
                                       double *motions, double *norms, int32_t *status) {
    if (!ctx || !poses || !status || (!motions && !norms)) return set_error(MVOSR_ERR_ARG, "pose2motion_batch: null argument");
    if (n < 0 || n_cases < 1) return set_error(MVOSR_ERR_ARG, "pose2motion_batch: n < 0 or fewer than one path");
    if (n_cases > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "pose2motion_batch: more than 65535 paths in one launch");
    if ((n + kScoreBlock - 1) / kScoreBlock > (int64_t)INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "pose2motion_batch: too many frames");
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(status, 0, (size_t)n_cases * sizeof(int32_t), ctx_stream(ctx));
    if (e != hipSuccess) return set_hip_error("hipMemsetAsync(status)", e);
    if (n == 0) return MVOSR_OK;
    hipLaunchKernelGGL(pose2motion_kernel, dim3((unsigned)((n + kScoreBlock - 1) / kScoreBlock), (unsigned)n_cases), dim3(kScoreBlock), 0,
                       ctx_stream(ctx), n_cases, n, poses, speed, motions, norms, status);
    return check_launch("pose2motion_kernel");
}
