// mvosr_scalescore_plan.hpp — the shape of scale_errors_kernel (mvosr_scalescore.hip), shared by the kernel and its launcher.
//
// A case is cut into UNITS, one workgroup each: unit 0 takes the statistics of |e| (mean, max, the counts above the thresholds),
// unit 1 + k the windowed drift of window k.  A resident workgroup keeps the case's n errors in LDS (|e| in unit 0, e in the
// others) and parks a window's segment values there; beyond kSsLdsErrors errors or kSsLdsSegments segments both live in the
// context's global scratch instead, filled by scale_errors_fill_kernel.  The arithmetic is the same text in both forms.
//
// Plain C++ (<stdint.h> only): a host compiler reads it as it stands.
#pragma once

#include <stdint.h>

namespace mvosr {

constexpr int kSsBlock = 256;
constexpr int kSsLdsErrors = 5120;            // errors of a case held in LDS: 40 KiB
constexpr int kSsLdsSegments = 1024;          // segment values of a window parked in LDS: 8 KiB
constexpr int kSsNodes = 256;                 // nodes of one 8192-element chunk's pairwise recursion by heap index: depth 7 at most
constexpr int kSsMaxWindows = 16;             // MVOSR_SCALE_MAX_WINDOWS
constexpr int kSsMaxThresholds = 8;           // MVOSR_SCALE_MAX_THRESHOLDS
constexpr int kSsMaxWindow = 8192;            // a window's sum is one chunk of np.add.reduce
constexpr int kSsLdsBytes = (kSsLdsErrors + kSsLdsSegments + kSsNodes + kSsBlock + 1) * 8 + (kSsMaxThresholds + 1) * 4;
static_assert(kSsLdsBytes <= 64 * 1024, "static LDS of one workgroup; two workgroups a CU");

// len(range(0, n - w, step)): the segments of window w over n errors (evaluate_scale.py:21)
inline constexpr int64_t scalescore_segments(int64_t n, int64_t w, int64_t step) { return n > w ? (n - w + step - 1) / step : 0; }

// whether a case's errors and every window's segment values fit the LDS form
inline constexpr bool scalescore_resident(int64_t n, int64_t max_segments) { return n <= kSsLdsErrors && max_segments <= kSsLdsSegments; }

}  // namespace mvosr
