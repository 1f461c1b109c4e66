// mvosr_statictri.hip — the rescale estimator's histogram-mode road model (road_model_calculation_static_tri,
// /root/reference/src/scale_calculator.py:294-310 with check_mode :446-483; rescale.py:179-187 is its caller) on the device.
//
// Per list of triangle heights h (1/|n| of the rows with pitch < loose, rescale.py:102):
//     hi = 1 / h                                    (:296)
//     dis = histogram of hi over the 19 bins with edges k * 0.1, k = 0..19   (:297; counted by comparison against the edges)
//     dis[dis == 1] = 0                             (:299)
//     max(dis) <= 2: no modes -> np.median(hi) over ALL values, those outside the bins included   (:302-303, :451-452)
//     else the flagged bins (:454-463) — bin 0 / 18 where they hold the maximum, an inner bin where it is >= both neighbours,
//     >= 0.33 max and >= 2 —, their FIRST run of consecutive bins i..j (:473-481, modes[0]), and
//     scale_norm = ((i + 1) + (j + 1)) / 2 / 10      (:306-310)
//
// One wavefront per list, four lists per workgroup, no LDS and no barrier: the waves of a workgroup never meet.
//   pass 1   the list is read once, 64 entries a step with the next step's loads in flight: per entry the IEEE quotient 1/h, its bin
//            (a guess from 10 hi settled against the two edges), and per bin one ballot whose population count lane k keeps for
//            bin k — so the 19 counts live in lanes 0..18.  The step also counts the entries and flags a height outside (0, inf).
//   decide   the ones zeroed, the maximum by a DPP reduction, the neighbours' counts by two lane shifts, the flags as ONE ballot:
//            a 19-bit mask whose first run is a count of trailing zeros and a count of trailing ones.
//   median   (cold: max <= 2, so at most 38 values lie inside the bins) a radix select over the values' 64-bit patterns —
//            positive doubles order like their patterns —: 16 passes of four bits, each re-reading the list (L2 / HBM, nothing
//            list-sized is kept) and counting its 16 buckets with ballots among the entries that share the prefix so far.  An
//            even count takes one more pass: how many values are <= the lower middle one, and the smallest one above it.
// Two input forms share the loop: packed lists (flags == nullptr: every entry counts) and the row form that
// mvosr_flat_selection_batch / mvosr_flat_ransac_batch write (tri_height and tri_flags laid out like tri2; an entry counts
// where flags & 1; the height of an entry that does not count is never read).
// The file is built with -ffp-contract=off and needs no fused operation: every operation here is an IEEE operation of its own.
#include "mvosr_device.hpp"
#include "mvosr_host.hpp"
#include "mvosr_select.hpp"

#include <math.h>

namespace mvosr {

constexpr int kStBins = 19;                  // len(range(0, 20)) - 1, scale_calculator.py:297
constexpr int kStWaves = 4;                  // lists per workgroup
constexpr int kStBlock = kStWaves * kWave;

struct StaticTriArgs {
    int64_t n_lists;
    const int64_t *off; const int32_t *cnt;  // cnt == nullptr: off has n_lists + 1 entries
    const double *height; const uint8_t *flags;
    int32_t min_count;
    double absolute_reference;
    double *scale_norm, *raw_scale;          // [F]
    int32_t *n_used;                         // [F]
    int32_t *hist;                           // optional [F][19]
    int32_t *status;                         // [F]
};

struct StItem { double h; bool counted; };

// entry i of a list of `len`: whether it counts, and its height if it does (a lane past the end: not counted)
__device__ __forceinline__ StItem st_load(const double *H, const uint8_t *FL, int64_t i, int64_t len) {
    StItem r;
    r.h = 1.0;
    r.counted = false;
    if (i < len) {
        r.counted = FL ? (FL[i] & 1) != 0 : true;
        if (r.counted) r.h = H[i];
    }
    return r;
}

// visit(counted, h) for every entry, 64 a step, every lane of the wave in every step; the next step's loads are issued first
template <class Visit>
__device__ __forceinline__ void st_for_each(const double *H, const uint8_t *FL, int64_t len, Visit visit) {
    const int lane = lane_id();
    StItem cur = st_load(H, FL, lane, len);
    for (int64_t i0 = 0; i0 < len; i0 += kWave) {
        const StItem nxt = st_load(H, FL, i0 + kWave + lane, len);
        visit(cur.counted, cur.h);
        cur = nxt;
    }
}

// np.histogram's bin of hi over the edges k * 0.1, k = 0..19: edges[k] <= hi < edges[k+1], the last bin closed, -1 outside.
// (int)(10 hi) is a guess (one rounding in 10 hi, one in k * 0.1: off by at most one bin); the two comparisons decide.
__device__ __forceinline__ int st_bin_of(double hi) {
    if (!(hi >= 0.0 && hi <= bin_edge(kStBins))) return -1;
    int k = (int)(hi * 10.0);
    k = min(k, kStBins - 1);
    k += (k < kStBins - 1 && hi >= bin_edge(k + 1)) ? 1 : 0;
    k -= (k > 0 && hi < bin_edge(k)) ? 1 : 0;
    return k;
}

__device__ __forceinline__ unsigned long long st_pattern(double h) { return (unsigned long long)__double_as_longlong(1.0 / h); }

// np.median of the counted entries' 1/h (n >= 1 of them): the middle order statistic, or (a + b) / 2 of the two middle ones — the
// radix select of mvosr_select.hpp over the entries' patterns, each pass re-reading the list
__device__ __forceinline__ double st_median(const double *H, const uint8_t *FL, int64_t len, int n) {
    unsigned long long lo, hi;
    wave_middle_keys([&](auto visit) { st_for_each(H, FL, len, [&](bool counted, double h) { visit(counted, st_pattern(h)); }); }, n, lo, hi);
    if (n & 1) return __longlong_as_double((long long)lo);
    return (__longlong_as_double((long long)lo) + __longlong_as_double((long long)hi)) / 2.0;
}

__global__ __launch_bounds__(kStBlock) void static_tri_kernel(const StaticTriArgs a) {
    const int64_t f = (int64_t)blockIdx.x * kStWaves + wave_id();
    if (f >= a.n_lists) return;                                    // (whole waves leave: nothing below is a workgroup barrier)
    const int lane = lane_id();
    const int64_t base = a.off[f];
    const int64_t len = a.cnt ? (int64_t)a.cnt[f] : a.off[f + 1] - base;
    // a list no launch of this library describes: refused before anything of it is read
    const bool shaped = base >= 0 && len >= 0 && len <= (int64_t)INT32_MAX;
    const double *H = a.height + (shaped ? base : 0);
    const uint8_t *FL = a.flags ? a.flags + (shaped ? base : 0) : nullptr;

    int mine = 0, n = 0;
    bool bad = false;
    st_for_each(H, FL, shaped ? len : 0, [&](bool counted, double h) {
        const bool ok = counted && h > 0.0 && h < INFINITY;
        bad = bad || (counted && !ok);
        n += counted ? 1 : 0;
        const int b = ok ? st_bin_of(1.0 / h) : -1;                // :296
        if (__ballot(b >= 0) == 0ull) return;
#pragma unroll
        for (int k = 0; k < kStBins; ++k) {
            const int c = __popcll(__ballot(b == k));
            mine += lane == k ? c : 0;
        }
    });
    n = wave_sum(n);
    const bool refused = !shaped || __ballot(bad) != 0ull;
    const bool few = n == 0 || n <= a.min_count;                    // rescale.py:181

    int d = lane < kStBins ? mine : 0;
    d = d == 1 ? 0 : d;                                            // :299
    const int mx = wave_max(d);                                    // :449
    const int left = __shfl_up(d, 1), right = __shfl_down(d, 1);
    bool flag = false;
    if (lane == 0 || lane == kStBins - 1) flag = d == mx;          // :454-458
    else if (lane < kStBins - 1) flag = d >= left && d >= right && (double)d >= 0.33 * (double)mx && d >= 2;   // :459-463
    const unsigned int mask = (unsigned int)__ballot(flag) & ((1u << kStBins) - 1u);

    double scale_norm = __longlong_as_double(0x7FF8000000000000ll);
    int status = MVOSR_ST_MODE;
    if (refused) status = MVOSR_ST_ERR_MASK;
    else if (few) status = MVOSR_ST_RS_FEW;
    else if (mx <= 2) {                                            // :451-452, :302-303
        status = MVOSR_ST_MEDIAN;
        scale_norm = st_median(H, FL, len, n);
    } else {
        // (a bin that holds the maximum is flagged whichever bin it is: the mask is not empty)
        const int i = __ffs((int)mask) - 1;                        // the first run (modes[0], :306-307): bins i..j
        const int j = i + (__ffs((int)~(mask >> i)) - 1) - 1;
        scale_norm = (double)((i + 1) + (j + 1)) / 2.0 / 10.0;     // :308-310 with int(bins[k] * 10) == k
    }
    if (a.hist && lane < kStBins) a.hist[f * kStBins + lane] = (refused || few) ? 0 : d;
    if (lane == 0) {
        a.scale_norm[f] = scale_norm;
        a.raw_scale[f] = scale_norm * a.absolute_reference;       // rescale.py:183
        a.n_used[f] = n;
        a.status[f] = status;
    }
}

}  // namespace mvosr

using namespace mvosr;

extern "C" int mvosr_static_tri_batch(mvosr_ctx *ctx, int64_t n_lists, const int64_t *off, const int32_t *cnt, const double *height,
                                      const uint8_t *flags, int32_t min_count, double absolute_reference, double *scale_norm,
                                      double *raw_scale, int32_t *n_used, int32_t *hist, int32_t *status) {
    if (!ctx || !off || !height || !scale_norm || !raw_scale || !n_used || !status)
        return set_error(MVOSR_ERR_ARG, "static_tri: null argument");
    if (min_count < 0) return set_error(MVOSR_ERR_ARG, "static_tri: min_count < 0");
    if (n_lists <= 0) return MVOSR_OK;
    const int64_t groups = (n_lists + kStWaves - 1) / kStWaves;
    if (groups > (int64_t)INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "static_tri: more than 2^33 lists in one launch");
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    StaticTriArgs a = {};
    a.n_lists = n_lists; a.off = off; a.cnt = cnt; a.height = height; a.flags = flags; a.min_count = min_count;
    a.absolute_reference = absolute_reference; a.scale_norm = scale_norm; a.raw_scale = raw_scale; a.n_used = n_used;
    a.hist = hist; a.status = status;
    hipLaunchKernelGGL(static_tri_kernel, dim3((unsigned)groups), dim3(kStBlock), 0, ctx_stream(ctx), a);
    return check_launch("static_tri_kernel");
}
