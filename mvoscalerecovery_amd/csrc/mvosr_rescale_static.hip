// mvosr_rescale_static.hip — flat_selection (/root/reference/src/rescale.py:75-102) and the histogram-mode road model over its
// loose heights (scale_calculation_static_tri, rescale.py:179-187 -> road_model_calculation_static_tri, scale_calculator.py:294-310
// with check_mode :446-483) in ONE kernel per frame on the device-resident form of a batch.
//
// flat_static_tri_kernel is a sibling of flat_selection_kernel<true> (mvosr_flat_ransac_batch): it reads what that one reads — the
// survivors compacted by keep >= 0 in order, the second triangulation's rows with their counts, dt_status — and runs one frame per
// workgroup, but its tail is the deterministic road model instead of the RANSAC plane:
//
//   phase 1   flat_phase1 (mvosr_flat.hpp), the loop flat_selection_kernel runs: every row's height and two bits, which stay in LDS
//             by row.  The loose rows are counted and their heights' patterns bounded.
//   level     flat_level_search (mvosr_flat.hpp): np.median of the loose heights (:91) with its two middle order statistics.  The
//             search's histogram lives where the vertex planes were.
//   model     one sweep over the rows: bit 2 and the kept count as flat_selection_kernel writes them, and of every loose row
//             hi = 1 / h with its bin among the 19 (counted by comparison against k * 0.1, bin 18 closed) — per bin one ballot per
//             wavefront step, a wavefront's 19 counts added to the workgroup's with integer LDS atomics.
//   decide    wavefront 0, as static_tri_kernel decides: the ones zeroed, the maximum, the flags as one ballot, the first run.
//             max <= 2 asks for np.median(hi): h -> fl(1 / h) is monotone non-increasing, so the two middle order statistics of hi
//             are the reciprocals of the two middle ones of h, mirrored — the level's search has found them already.
//
// The given form (tri_height_in / tri_flags_in) reads the rows' heights and two bits from global memory, in row form, instead of
// computing them: geometry, keep and tri2 are not read and nothing row-sized is kept in LDS; everything behind phase 1 is the same
// code, reading through pointers into global memory.
// fp64, compiled with -ffp-contract=off; integer LDS atomics and ballots only; no point list, no hypotheses, no triples.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mvosr.h"
#include "mvosr_device.hpp"
#include "mvosr_ransac.hpp"
#include "mvosr_flat.hpp"
#include "mvosr_host.hpp"
#include "mvosr_rescale_static_plan.hpp"

namespace mvosr {

struct StaticArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *x, *y, *z;
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    const int32_t *keep;           // [like x] a feature takes part iff keep[i] >= 0 (null: all)
    const int32_t *dt_status;      // [F] non-zero: declined triangulation, frame skipped (null: none)
    const double *height_in;       // given form: [rows] heights
    const uint8_t *flags_in;       // given form: [rows] bit0: the row counts (pitch < loose), bit1: pitch < tight
    int32_t max_feat, max_tri, min_count;
    double loose_deg, tight_deg, height_factor, absolute_reference;
    double *scale_norm, *raw_scale, *height_level;   // [F]
    int32_t *n_used, *n_kept, *status;               // [F]
    int32_t *hist;                 // optional [F][19]
    double *tri_height;            // optional [rows] 1/|n|
    uint8_t *tri_flags;            // optional [rows] bit0: pitch < loose, bit1: pitch < tight, bit2: kept
};

// np.histogram's bin of hi over the edges k * 0.1, k = 0..19: edges[k] <= hi < edges[k+1], the last bin closed, -1 outside
// (static_tri_kernel's rule: (int)(10 hi) is off by at most one bin, the two comparisons decide)
__device__ __forceinline__ int static_bin_of(double hi) {
    if (!(hi >= 0.0 && hi <= bin_edge(kStaticModelBins))) return -1;
    int k = (int)(hi * 10.0);
    k = min(k, kStaticModelBins - 1);
    k += (k < kStaticModelBins - 1 && hi >= bin_edge(k + 1)) ? 1 : 0;
    k -= (k > 0 && hi < bin_edge(k)) ? 1 : 0;
    return k;
}

template <bool GIVEN>
__global__ __launch_bounds__(kStaticWaves *kWave) void flat_static_tri_kernel(const StaticArgs a) {
    constexpr int WAVES = kStaticWaves, BLK = WAVES * kWave;
    static_assert(kStaticModelBins <= 32, "flat_static_tri_kernel: the model's bins in the plan");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int n_all = a.feat_cnt[f];
    const int64_t off = a.feat_off[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const bool skip = a.dt_status && a.dt_status[f] != 0;
    // more features or rows than the launch's LDS was sized for (the header's max_feat, the call's max_tri): refused, LDS untouched
    const bool oversize = n_all > a.max_feat || tn > a.max_tri;
    if (const int refused = flat_entry_status(n_all, tn, skip, oversize)) {
        if (tid == 0) {
            a.status[f] = refused;
            a.height_level[f] = nan(""); a.n_kept[f] = 0;
            a.scale_norm[f] = nan(""); a.raw_scale[f] = nan(""); a.n_used[f] = 0;
        }
        if (a.hist && tid < kStaticModelBins) a.hist[f * kStaticModelBins + tid] = 0;
        return;
    }
    const auto lds = GIVEN ? static_plan<uint32_t>(0u, 0u) : static_plan<uint32_t>((uint32_t)n_all, (uint32_t)tn);
    unsigned long long *ext = reinterpret_cast<unsigned long long *>(smem + lds.ext);
    int *misc = reinterpret_cast<int *>(smem + lds.misc);
    int *model = reinterpret_cast<int *>(smem + lds.model);
    int *hist = reinterpret_cast<int *>(smem + lds.hist);
    flat_state_init(misc, ext);
    if (tid < 32) model[tid] = 0;
    // what the phases behind the first read: the rows' heights and flags, in LDS (fused) or in global memory (given)
    const double *Hh;
    const uint8_t *Fl;
    FlatLoose tally;
    if constexpr (GIVEN) {
        Hh = a.height_in + tb;
        Fl = a.flags_in + tb;
        for (int t = tid; t < tn; t += BLK) if (Fl[t] & 1) tally.add(Hh[t]);
        __syncthreads();                                         // (misc and ext are set: the tallies below add to them)
    } else {
        double *H1 = reinterpret_cast<double *>(smem + lds.heights);
        uint8_t *F1 = reinterpret_cast<uint8_t *>(smem + lds.flags);
        double *X = reinterpret_cast<double *>(smem + lds.x);
        double *Y = reinterpret_cast<double *>(smem + lds.y);
        double *Z = reinterpret_cast<double *>(smem + lds.z);
        Hh = H1;
        Fl = F1;
        // (the first rows are in flight while the vertex planes stream in: mvosr_flat.hpp, flat_phase1)
        TriIds rows[kFlatRows];
        flat_load_rows<BLK>(a.tri + 3 * tb, tid, tn, rows);
        // ---- the survivors, compacted in order (rescale.py:134-135)
        int n = n_all;
        if (a.keep) n = flat_compact_survivors<WAVES>(n_all, a.keep + off, a.x + off, a.y + off, a.z + off, X, Y, Z, misc + FM_CW);
        else {
#pragma unroll 4
            for (int i = tid; i < n_all; i += BLK) { X[i] = a.x[off + i]; Y[i] = a.y[off + i]; Z[i] = a.z[off + i]; }
        }
        const double s_loose = flat_sin_deg(a.loose_deg), s_tight = flat_sin_deg(a.tight_deg);
        __syncthreads();
        // ---- phase 1: every row's height and flags into LDS, the loose ones counted and bounded (rescale.py:79-89)
        flat_phase1<BLK>(a.tri + 3 * tb, rows, tn, X, Y, Z, n, a.loose_deg, a.tight_deg, s_loose, s_tight, H1, F1,
                         a.tri_height ? a.tri_height + tb : nullptr, misc, tally);
    }
    tally.commit(misc, ext);
    __syncthreads();                                             // (the planes are dead: their room is the histogram's)
    const int k = misc[FM_K];
    // ---- the level (:91): np.median of the loose heights, with the two middle order statistics (one, twice, for an odd k)
    const FlatLevel lv = flat_level_search<WAVES>(reinterpret_cast<const unsigned long long *>(Hh), Fl, tn, k, ext, misc, hist, a.height_factor);
    const double level = lv.level, vlo = lv.vlo, vhi = lv.vhi;
    // ---- the kept rows (:94-96) and the road model's histogram (scale_calculator.py:296-297), one sweep, 64 rows a wavefront step
    {
        int kept = 0, mine = 0;
        bool badh = false;
        for (int t0 = wave * kWave; t0 < tn; t0 += BLK) {
            const int t = t0 + lane;
            const bool in = t < tn;
            uint8_t fl = in ? (uint8_t)(Fl[t] & 3) : (uint8_t)0;
            const double h = fl ? Hh[t] : 1.0;                   // (a row with neither bit: its height is not read)
            if ((fl & 2) && h > level) { fl |= 4; ++kept; }
            if (in && a.tri_flags) a.tri_flags[tb + t] = fl;
            if (GIVEN && in && a.tri_height) a.tri_height[tb + t] = Hh[t];
            const bool counted = (fl & 1) != 0;
            const bool ok = counted && h > 0.0 && h < INFINITY;
            badh = badh || (counted && !ok);
            const int b = ok ? static_bin_of(1.0 / h) : -1;      // :296
            if (__ballot(b >= 0) != 0ull) {
#pragma unroll
                for (int kk = 0; kk < kStaticModelBins; ++kk) {
                    const int c = __popcll(__ballot(b == kk));
                    mine += lane == kk ? c : 0;
                }
            }
        }
        kept = wave_sum(kept);
        if (lane == 0 && kept) atomicAdd(&misc[FM_KEPT], kept);
        if (lane < kStaticModelBins && mine) atomicAdd(&model[lane], mine);
        if (__ballot(badh) != 0ull && lane == 0) misc[FM_BADH] = 1;
    }
    __syncthreads();
    // ---- decide, as static_tri_kernel does (scale_calculator.py:299-310, :446-483)
    if (wave == 0) {
        const int flat_err = misc[FM_BADID] ? MVOSR_ST_ERR_MASK : (misc[FM_SINGULAR] ? MVOSR_ST_ERR_SINGULAR : 0);
        const bool refused = misc[FM_BADH] != 0;
        const bool few = k == 0 || k <= a.min_count;             // rescale.py:181
        int d = lane < kStaticModelBins ? model[lane] : 0;
        d = d == 1 ? 0 : d;                                      // :299
        const int mx = wave_max(d);                              // :449
        const int left = __shfl_up(d, 1), right = __shfl_down(d, 1);
        bool flag = false;
        if (lane == 0 || lane == kStaticModelBins - 1) flag = d == mx;          // :454-458
        else if (lane < kStaticModelBins - 1) flag = d >= left && d >= right && (double)d >= 0.33 * (double)mx && d >= 2;   // :459-463
        const unsigned int mask = (unsigned int)__ballot(flag) & ((1u << kStaticModelBins) - 1u);
        double scale_norm = nan("");
        int status = MVOSR_ST_MODE;
        if (flat_err) status = flat_err;
        else if (refused) status = MVOSR_ST_ERR_MASK;
        else if (few) status = MVOSR_ST_RS_FEW;
        else if (mx <= 2) {                                      // :451-452, :302-303: np.median(hi)
            status = MVOSR_ST_MEDIAN;
            // (hi's lower middle is 1 / the upper middle of h, its upper middle 1 / the lower one)
            scale_norm = (k & 1) ? 1.0 / vlo : (1.0 / vhi + 1.0 / vlo) / 2.0;
        } else {
            const int i = __ffs((int)mask) - 1;                  // the first run (modes[0], :306-307): bins i..j
            const int j = i + (__ffs((int)~(mask >> i)) - 1) - 1;
            scale_norm = (double)((i + 1) + (j + 1)) / 2.0 / 10.0;             // :308-310
        }
        if (a.hist && lane < kStaticModelBins) a.hist[f * kStaticModelBins + lane] = (flat_err || refused || few) ? 0 : d;
        if (lane == 0) {
            a.height_level[f] = level;
            a.n_kept[f] = misc[FM_KEPT];
            a.scale_norm[f] = scale_norm;
            a.raw_scale[f] = scale_norm * a.absolute_reference;   // rescale.py:183
            a.n_used[f] = flat_err ? 0 : k;
            a.status[f] = status;
        }
    }
}

}  // namespace mvosr

using namespace mvosr;

extern "C" {

size_t mvosr_flat_static_tri_lds_bytes(int max_feat, int64_t max_tri) {
    const size_t mf = max_feat > 0 ? (size_t)max_feat : 0;
    const size_t mt = max_tri > 0 ? (size_t)max_tri : 2 * mf;
    return static_plan<size_t>(mf, mt).total;
}

int mvosr_flat_static_tri_batch(mvosr_ctx *ctx, const mvosr_batch *b, const int32_t *keep, double loose_deg, double tight_deg,
                                double height_factor, int32_t min_count, double absolute_reference, const int32_t *dt_status,
                                const double *tri_height_in, const uint8_t *tri_flags_in, const mvosr_static_tri_outputs *o,
                                int64_t max_tri) {
    if (!ctx || !b || !o) return set_error(MVOSR_ERR_ARG, "flat_static_tri: null argument");
    if (!o->scale_norm || !o->raw_scale || !o->height_level || !o->n_used || !o->n_kept || !o->status)
        return set_error(MVOSR_ERR_ARG, "flat_static_tri: a required output is null");
    if (min_count < 0) return set_error(MVOSR_ERR_ARG, "flat_static_tri: min_count < 0");
    if ((tri_height_in != nullptr) != (tri_flags_in != nullptr))
        return set_error(MVOSR_ERR_ARG, "flat_static_tri: tri_height_in and tri_flags_in go together");
    const bool given = tri_height_in != nullptr;
    if (!b->feat_off || !b->feat_cnt || !b->tri2_off) return set_error(MVOSR_ERR_ARG, "flat_static_tri: missing feat_off/feat_cnt/tri2_off");
    if (!given && (!b->x || !b->y || !b->z || !b->tri2)) return set_error(MVOSR_ERR_ARG, "flat_static_tri: missing x/y/z/tri2");
    if (b->max_feat < 0) return set_error(MVOSR_ERR_ARG, "flat_static_tri: max_feat < 0");
    if (b->n_frames <= 0) return MVOSR_OK;
    if (b->n_frames > (int64_t)0x7fffffff) return set_error(MVOSR_ERR_TOO_LARGE, "flat_static_tri: frames exceed a grid");
    if (max_tri <= 0) max_tri = 2 * (int64_t)b->max_feat;
    if (max_tri > INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "flat_static_tri: max_tri does not fit 32 bits");
    // (the given form keeps no row in LDS: its request is the plan at (0, 0), whatever the header names)
    const size_t lds = given ? static_plan<size_t>(0, 0).total : static_plan<size_t>((size_t)b->max_feat, (size_t)max_tri).total;
    if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_TOO_LARGE, "flat_static_tri: a frame of %d features and %lld rows needs %zu B of LDS (> %d)", b->max_feat,
                         (long long)max_tri, lds, ctx->max_lds_per_block);
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    auto kernel = given ? flat_static_tri_kernel<true> : flat_static_tri_kernel<false>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    StaticArgs a = {};
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.x = b->x; a.y = b->y; a.z = b->z;
    a.tri_off = b->tri2_off; a.tri = b->tri2; a.tri_cnt = b->tri2_cnt;
    a.keep = keep; a.dt_status = dt_status; a.height_in = tri_height_in; a.flags_in = tri_flags_in;
    a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri; a.min_count = min_count;
    a.loose_deg = loose_deg; a.tight_deg = tight_deg; a.height_factor = height_factor; a.absolute_reference = absolute_reference;
    a.scale_norm = o->scale_norm; a.raw_scale = o->raw_scale; a.height_level = o->height_level;
    a.n_used = o->n_used; a.n_kept = o->n_kept; a.status = o->status; a.hist = o->hist;
    a.tri_height = o->tri_height; a.tri_flags = o->tri_flags;
    hipLaunchKernelGGL(kernel, dim3((unsigned)b->n_frames), dim3(kStaticWaves * kWave), lds, ctx_stream(ctx), a);
    return check_launch(given ? "flat_static_tri_kernel<given>" : "flat_static_tri_kernel");
}

}  // extern "C"
