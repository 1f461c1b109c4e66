// mvosr_window_median.hpp — the median of one sliding window as np.median takes it, shared by window_median_kernel
// (mvosr_kernels.hip: the estimator's scale queue) and window_median_cases_kernel (mvosr_scalescore.hip: evaluate_scale.py's
// filter over C sequences).  The text was moved here from window_median_kernel; what differs between the users — where element k
// of the window comes from — is the caller's `at`.
#pragma once

#include "mvosr_device.hpp"

namespace mvosr {

constexpr int kMaxWindow = 64;

// np.median of the m <= kMaxWindow values at(0) .. at(m - 1): insertion sort in the lane's own array, the middle value or the
// mean of the two middle values; a NaN anywhere in the window gives NaN.
template <class At>
__device__ __forceinline__ double window_median_of(int m, At at) {
    double w[kMaxWindow];
    bool has_nan = false;
    for (int k = 0; k < m; ++k) {
        const double x = at(k);
        has_nan |= (x != x);
        int j = k;                                   // insertion sort
        while (j > 0 && w[j - 1] > x) { w[j] = w[j - 1]; --j; }
        w[j] = x;
    }
    if (has_nan) return nan("");                     // np.median propagates NaN
    if (m & 1) return w[m >> 1];
    return (w[(m >> 1) - 1] + w[m >> 1]) / 2.0;      // np.mean of the two middle values
}

}  // namespace mvosr
