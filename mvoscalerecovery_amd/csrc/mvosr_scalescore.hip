// mvosr_scalescore.hip — the last step of the reference's workflow on the device: /root/reference/script/evaluate_scale.py run by
// tesh.sh:4-8 on every scales file against the ground truth's speed file.  evaluate_scale (:4-13) with patch (:19-23) for C cases
// in one launch, and filter (:24-28) — the running median — for C sequences in one launch.  fp64; built with -ffp-contract=off:
// every operation written here is one IEEE operation, and every sum has NumPy's order (mvosr_npsum.hpp), so the figures are the
// reference's own doubles.
//
// scale_errors_kernel        grid (1 + windows, cases), the units of mvosr_scalescore_plan.hpp.  e = gt[i] - scales[c][i].
//   unit 0                   a = |e|: np.mean(a) = np.add.reduce(a) / n, np.max(a) (NaN if any a is NaN), sum(a > t) per threshold
//                            as integers.
//   unit 1 + k               window w: one lane per segment i = 0, step, 2 step .. < n - w takes np.sum(e[i : i + w]) — the pairwise
//                            recursion over the slice's LENGTH, whatever its offset — then |.| / w, parks it, and the workgroup takes
//                            np.mean of the parked list.  No segment: NaN, as np.mean([]).
//   block_np_sum             (mvosr_npsum.hpp) np.add.reduce of a list in memory: per 8192-element chunk one thread per node of the recursion — the
//                            leaves (<= 128 elements, np_leaf_sum) side by side, then the inner nodes level by level, each the sum
//                            of its two halves — and the chunk added to the running total, left to right from 0.  No
//                            floating-point atomics: the same bytes every run.
// scale_errors_fill_kernel   the global-memory form's e and |e|, one lane per (case, i).
// window_median_cases_kernel one lane per (case, i): np.median(data[c][max(i - window + 1, 0) : i + 1]), the window's median of
//                            mvosr_window_median.hpp — window_median_kernel with an empty queue, over C sequences.
#include "mvosr_device.hpp"
#include "mvosr_host.hpp"
#include "mvosr_npsum.hpp"
#include "mvosr_scalescore_plan.hpp"
#include "mvosr_window_median.hpp"

#include <math.h>

namespace mvosr {

static_assert(kSsMaxWindows == MVOSR_SCALE_MAX_WINDOWS && kSsMaxThresholds == MVOSR_SCALE_MAX_THRESHOLDS, "include/mvosr.h states the caps");
static_assert(kSsMaxWindow <= kNpBufSize && kSsNodes == kNpNodes && kSsNodes <= kSsBlock, "a window's sum; a chunk's recursion, one thread a node");

// The recursion of @TYPE@_pairwise_sum over n <= kNpBufSize elements in post-order: visit(lo, len, true) for a leaf (<= 128
// elements), visit(lo, len, false) for an inner node once both halves — the first rounded down to a multiple of 8 — are done.
template <class Visit>
__device__ __forceinline__ void ss_pairwise_walk(int n, Visit visit) {
    int lo_s[kNpDepth], n_s[kNpDepth], stage_s[kNpDepth];
    int sp = 1;
    lo_s[0] = 0; n_s[0] = n; stage_s[0] = 0;
    while (sp > 0) {
        const int lo = lo_s[sp - 1], m = n_s[sp - 1], stage = stage_s[sp - 1];
        if (m <= 128) { visit(lo, m, true); --sp; continue; }
        int m2 = m / 2;
        m2 -= m2 % 8;
        if (stage == 0) { stage_s[sp - 1] = 1; lo_s[sp] = lo; n_s[sp] = m2; stage_s[sp] = 0; ++sp; }
        else if (stage == 1) { stage_s[sp - 1] = 2; lo_s[sp] = lo + m2; n_s[sp] = m - m2; stage_s[sp] = 0; ++sp; }
        else { visit(lo, m, false); --sp; }
    }
}

// np.sum of a slice of n <= kNpBufSize elements by one lane (the lanes of a wavefront walk the same tree: n is uniform)
__device__ __forceinline__ double ss_slice_sum(const double *a, int n) {
    if (n <= 128) return np_leaf_sum(a, n, 0.0, false);
    double val[kNpDepth + 1];
    int vp = 0;
    ss_pairwise_walk(n, [&](int lo, int len, bool is_leaf) {
        if (is_leaf) val[vp++] = np_leaf_sum(a + lo, len, 0.0, false);
        else { const double r = val[--vp], l = val[--vp]; val[vp++] = l + r; }
    });
    return val[0];
}

struct ScaleErrArgs {
    int64_t n, case_stride, seg_cap;
    int n_windows, n_thr, step;
    const double *gt, *scales;       // gt [>= n], scales [C][case_stride]
    double *err;                     // the global form: [C][2][n], e then |e|
    double *park;                    // the global form: [C][n_windows][seg_cap]
    double *stats;                   // [C][2]: mean, max
    int32_t *counts;                 // [C][n_thr]
    double *drift;                   // [C][n_windows]
    int32_t *status;                 // [C]
    int32_t windows[kSsMaxWindows];
    double thr[kSsMaxThresholds];    // +inf beyond n_thr: counts nothing
};

__global__ __launch_bounds__(kSsBlock) void scale_errors_fill_kernel(const ScaleErrArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kSsBlock + threadIdx.x, c = blockIdx.y;
    if (i >= a.n) return;
    const double d = a.gt[i] - a.scales[c * a.case_stride + i];
    a.err[(c * 2) * a.n + i] = d;
    a.err[(c * 2 + 1) * a.n + i] = fabs(d);
}

template <bool RESIDENT>
__global__ __launch_bounds__(kSsBlock) void scale_errors_kernel(const ScaleErrArgs a) {
    __shared__ double lds_e[RESIDENT ? kSsLdsErrors : 1];
    __shared__ double lds_park[RESIDENT ? kSsLdsSegments : 1];
    __shared__ double node[kSsNodes];
    __shared__ double red[kSsBlock];
    __shared__ double slot;
    __shared__ int cnt[kSsMaxThresholds];
    __shared__ int any_nan;
    const int unit = blockIdx.x, t = threadIdx.x;
    const int64_t c = blockIdx.y, n = a.n;
    const bool stats = unit == 0;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double *e;
    double *park;
    if (RESIDENT) {
        const double *S = a.scales + c * a.case_stride;
        for (int i = t; i < (int)n; i += kSsBlock) {
            const double d = a.gt[i] - S[i];
            lds_e[i] = stats ? fabs(d) : d;
        }
        e = lds_e;
        park = lds_park;
    } else {
        e = a.err + (c * 2 + (stats ? 1 : 0)) * n;
        park = a.park + (c * a.n_windows + (stats ? 0 : unit - 1)) * a.seg_cap;
    }
    if (t < kSsMaxThresholds) cnt[t] = 0;
    if (t == 0) any_nan = 0;
    __syncthreads();

    if (stats) {
        double mx = -INFINITY;
        bool has_nan = false;
        int k[kSsMaxThresholds];
#pragma unroll
        for (int j = 0; j < kSsMaxThresholds; ++j) k[j] = 0;
        for (int64_t i = t; i < n; i += kSsBlock) {
            const double v = e[i];
            has_nan |= v != v;
            mx = v > mx ? v : mx;
#pragma unroll
            for (int j = 0; j < kSsMaxThresholds; ++j) k[j] += v > a.thr[j] ? 1 : 0;
        }
#pragma unroll
        for (int j = 0; j < kSsMaxThresholds; ++j) {
            const int s = wave_sum(k[j]);
            if (lane_id() == 0 && s) atomicAdd(&cnt[j], s);
        }
        if (has_nan) atomicOr(&any_nan, 1);
        red[t] = mx;
        __syncthreads();
        for (int h = kSsBlock / 2; h > 0; h >>= 1) {
            if (t < h) { const double o = red[t + h]; red[t] = o > red[t] ? o : red[t]; }
            __syncthreads();
        }
        const double sum = block_np_sum(e, n, node, &slot);
        if (t == 0) {
            a.stats[c * 2] = n > 0 ? sum / (double)n : qnan;                               // np.mean
            a.stats[c * 2 + 1] = (n > 0 && !any_nan) ? red[0] : qnan;                      // np.max propagates NaN
            a.status[c] = n > 0 ? 0 : MVOSR_ST_ERR_EMPTY;
        }
        if (t < a.n_thr) a.counts[c * a.n_thr + t] = cnt[t];
        return;
    }

    const int w = a.windows[unit - 1];
    const int64_t m = scalescore_segments(n, w, a.step);
    if (m == 0) {                                                                           // np.mean([])
        if (t == 0) a.drift[c * a.n_windows + unit - 1] = qnan;
        return;
    }
    for (int64_t s = t; s < m; s += kSsBlock) park[s] = fabs(ss_slice_sum(e + s * a.step, w)) / (double)w;   // patch, :22-23
    __threadfence_block();
    const double sum = block_np_sum(park, m, node, &slot);
    if (t == 0) a.drift[c * a.n_windows + unit - 1] = sum / (double)m;
}

__global__ __launch_bounds__(kSsBlock) void window_median_cases_kernel(const double *data, int64_t case_stride, int64_t n, int window,
                                                                       double *out, int64_t out_stride) {
    const int64_t i = (int64_t)blockIdx.x * kSsBlock + threadIdx.x, c = blockIdx.y;
    if (i >= n) return;
    const double *D = data + c * case_stride;
    const int64_t first = i - window + 1 > 0 ? i - window + 1 : 0;
    out[c * out_stride + i] = window_median_of((int)(i - first + 1), [&](int k) { return D[first + k]; });
}

}  // namespace mvosr

using namespace mvosr;

extern "C" int mvosr_scale_errors_batch(mvosr_ctx *ctx, int64_t n_gt, const double *gt, int64_t n_cases, int64_t n, const double *scales,
                                        int64_t case_stride, int n_windows, const int32_t *windows, int step, int n_thresholds,
                                        const double *thresholds, int flags, double *stats, int32_t *counts, double *drift,
                                        int32_t *status) {
    if (!ctx || !stats || !status || (n > 0 && (!gt || !scales)) || (n_windows > 0 && (!windows || !drift)) ||
        (n_thresholds > 0 && (!thresholds || !counts)))
        return set_error(MVOSR_ERR_ARG, "scale_errors_batch: null argument");
    if (n < 0 || n_gt < 0 || n_cases < 1 || case_stride < n) return set_error(MVOSR_ERR_ARG, "scale_errors_batch: n < 0, fewer than one case, or a case stride below n");
    if (n > n_gt) return set_error(MVOSR_ERR_ARG, "scale_errors_batch: %lld scales against %lld ground-truth values (the reference's subtraction does not broadcast)", (long long)n, (long long)n_gt);
    if (n_windows < 0 || n_windows > kSsMaxWindows || n_thresholds < 0 || n_thresholds > kSsMaxThresholds || step < 1)
        return set_error(MVOSR_ERR_ARG, "scale_errors_batch: at most %d windows and %d thresholds, step >= 1", kSsMaxWindows, kSsMaxThresholds);
    if (n > (int64_t)INT32_MAX || n_cases > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "scale_errors_batch: more than 2^31-1 scales or 65535 cases in one launch");
    ScaleErrArgs a = {};
    int64_t max_seg = 0;
    for (int k = 0; k < n_windows; ++k) {
        if (windows[k] < 1 || windows[k] > kSsMaxWindow) return set_error(MVOSR_ERR_ARG, "scale_errors_batch: a window is in 1..%d", kSsMaxWindow);
        a.windows[k] = windows[k];
        const int64_t m = scalescore_segments(n, windows[k], step);
        max_seg = m > max_seg ? m : max_seg;
    }
    for (int k = 0; k < kSsMaxThresholds; ++k) a.thr[k] = k < n_thresholds ? thresholds[k] : INFINITY;
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    a.n = n; a.case_stride = case_stride; a.n_windows = n_windows; a.n_thr = n_thresholds; a.step = step;
    a.gt = gt; a.scales = scales; a.stats = stats; a.counts = counts; a.drift = drift; a.status = status;
    const dim3 grid((unsigned)(1 + n_windows), (unsigned)n_cases);
    if (!(flags & MVOSR_SCALE_ERRORS_GLOBAL) && scalescore_resident(n, max_seg)) {
        hipLaunchKernelGGL(scale_errors_kernel<true>, grid, dim3(kSsBlock), 0, ctx_stream(ctx), a);
        return check_launch("scale_errors_kernel<resident>");
    }
    a.seg_cap = max_seg > 0 ? max_seg : 1;
    const size_t n_err = (size_t)n_cases * 2 * (size_t)n, n_park = (size_t)n_cases * (size_t)(n_windows > 0 ? n_windows : 1) * (size_t)a.seg_cap;
    void *ws = nullptr;
    if ((rc = ctx_workspace_bytes(ctx, (n_err + n_park) * sizeof(double), &ws))) return rc;
    a.err = static_cast<double *>(ws);
    a.park = a.err + n_err;
    if (n > 0) {
        hipLaunchKernelGGL(scale_errors_fill_kernel, dim3((unsigned)((n + kSsBlock - 1) / kSsBlock), (unsigned)n_cases), dim3(kSsBlock), 0,
                           ctx_stream(ctx), a);
        if ((rc = check_launch("scale_errors_fill_kernel"))) return rc;
    }
    hipLaunchKernelGGL(scale_errors_kernel<false>, grid, dim3(kSsBlock), 0, ctx_stream(ctx), a);
    return check_launch("scale_errors_kernel<global>");
}

extern "C" int mvosr_window_median_cases(mvosr_ctx *ctx, const double *data, int64_t n_cases, int64_t n, int64_t case_stride, int window,
                                         double *out, int64_t out_stride) {
    if (!ctx || (n > 0 && (!data || !out))) return set_error(MVOSR_ERR_ARG, "window_median_cases: null argument");
    if (window < 1 || window > kMaxWindow) return set_error(MVOSR_ERR_ARG, "window_median_cases: window must be in 1..%d", kMaxWindow);
    if (n < 0 || n_cases < 1 || case_stride < n || out_stride < n) return set_error(MVOSR_ERR_ARG, "window_median_cases: n < 0, fewer than one case, or a stride below n");
    if (n_cases > 65535 || (n + kSsBlock - 1) / kSsBlock > (int64_t)INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "window_median_cases: more than 65535 sequences or 2^39 values in one launch");
    if (n == 0) return MVOSR_OK;
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(window_median_cases_kernel, dim3((unsigned)((n + kSsBlock - 1) / kSsBlock), (unsigned)n_cases), dim3(kSsBlock), 0,
                       ctx_stream(ctx), data, case_stride, n, window, out, out_stride);
    return check_launch("window_median_cases_kernel");
}
