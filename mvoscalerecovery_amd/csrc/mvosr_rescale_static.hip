// mvosr_rescale_static.hip — flat_selection (/root/reference/src/rescale.py:75-102) and the histogram-mode road model over its
// loose heights (scale_calculation_static_tri, rescale.py:179-187 -> road_model_calculation_static_tri, scale_calculator.py:294-310
// with check_mode :446-483) in ONE kernel per frame on the device-resident form of a batch.
//
// flat_static_tri_kernel is a sibling of flat_selection_kernel<true> (mvosr_flat_ransac_batch): it reads what that one reads — the
// survivors compacted by keep >= 0 in order, the second triangulation's rows with their counts, dt_status — and runs one frame per
// workgroup, but its tail is the deterministic road model instead of the RANSAC plane:
//
//   phase 1   every row's (mu, height) by row_height_pitch, the device function flat_selection_kernel calls, and the row's two bits
//             decided as that kernel decides them (on mu away from sin(threshold) by more than 1e-12, else on asin(mu) * 180 / pi);
//             heights and flags stay in LDS by row.  The loose rows are counted and their heights' patterns bounded.
//   level     np.median of the loose heights (:91): the lower middle order statistic by a 2048-bin histogram over the candidates'
//             range, narrowed to the bin that holds the rank and repeated, wavefront 0 ranking the last <= 64 candidates directly;
//             the upper one by one more sweep.  The histogram lives where the vertex planes were.
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

constexpr int kStaticRows = 4;          // triangle rows a thread keeps in flight

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
    static_assert(kStaticBins % BLK == 0 && kStaticModelBins <= 32, "flat_static_tri_kernel: bins per thread / the model's bins in the plan");
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
    if (n_all <= 0 || tn <= 0 || skip || oversize) {
        if (tid == 0) {
            a.status[f] = (!skip && oversize && n_all > 0 && tn > 0) ? MVOSR_ST_ERR_MASK : MVOSR_ST_ERR_EMPTY;
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
    if (tid < TM_WSUM) misc[tid] = 0;
    if (tid < 32) model[tid] = 0;
    if (tid == 0) { ext[0] = ~0ull; ext[1] = 0ull; ext[2] = ~0ull; }
    // what the phases behind the first read: the rows' heights and flags, in LDS (fused) or in global memory (given)
    const double *Hh;
    const uint8_t *Fl;
    int k_mine = 0;
    unsigned long long umin = ~0ull, umax = 0ull;
    if constexpr (GIVEN) {
        Hh = a.height_in + tb;
        Fl = a.flags_in + tb;
        for (int t = tid; t < tn; t += BLK) {
            if (!(Fl[t] & 1)) continue;
            const unsigned long long u = (unsigned long long)__double_as_longlong(Hh[t]);
            ++k_mine; umin = u < umin ? u : umin; umax = u > umax ? u : umax;
        }
        __syncthreads();                                         // (misc and ext are set: the tallies below add to them)
    } else {
        double *H1 = reinterpret_cast<double *>(smem + lds.heights);
        uint8_t *F1 = reinterpret_cast<uint8_t *>(smem + lds.flags);
        double *X = reinterpret_cast<double *>(smem + lds.x);
        double *Y = reinterpret_cast<double *>(smem + lds.y);
        double *Z = reinterpret_cast<double *>(smem + lds.z);
        Hh = H1;
        Fl = F1;
        // a thread's next kStaticRows triangle rows are in flight while it works on the current ones (and the first ones while the
        // vertex planes stream in)
        TriIds rows[kStaticRows];
        auto load_rows = [&](int t0) {
#pragma unroll
            for (int j = 0; j < kStaticRows; ++j) rows[j] = load_tri(a.tri + 3 * tb, min(t0 + j * BLK, tn - 1));
        };
        load_rows(tid);
        // ---- the survivors, compacted in order (rescale.py:134-135): every wavefront owns a contiguous segment of the frame
        int n = n_all;
        if (a.keep) {
            int s0, s1;
            ordered_segment(n_all, BLK, s0, s1);
            int c = 0;
            for (int i0 = s0; i0 < s1; i0 += kWave) {
                const int i = i0 + lane;
                c += __popcll(__ballot(i < s1 && a.keep[off + i] >= 0));
            }
            int base;
            ordered_prefix<WAVES>(misc + TM_CW, c, base, n);
            for (int i0 = s0; i0 < s1; i0 += kWave) {
                const int i = i0 + lane;
                const bool k = i < s1 && a.keep[off + i] >= 0;
                const int pos = ordered_rank(k, base);
                if (k) { X[pos] = a.x[off + i]; Y[pos] = a.y[off + i]; Z[pos] = a.z[off + i]; }
            }
        } else {
#pragma unroll 4
            for (int i = tid; i < n_all; i += BLK) { X[i] = a.x[off + i]; Y[i] = a.y[off + i]; Z[i] = a.z[off + i]; }
        }
        const double s_loose = sin(a.loose_deg * 3.141592653589793 / 180.0), s_tight = sin(a.tight_deg * 3.141592653589793 / 180.0);
        __syncthreads();
        // ---- phase 1: every row's height and flags into LDS, the loose ones counted and bounded (rescale.py:79-89)
        auto one_row = [&](const TriIds q, const int t) {
            if (!ids_in_range(q.a, q.b, q.c, n)) {
                misc[TM_BADID] = 1; F1[t] = 0; H1[t] = nan(""); if (a.tri_height) a.tri_height[tb + t] = nan(""); return;
            }
            double mu, h;
            if (!row_height_pitch(X, Y, Z, q, mu, h)) misc[TM_SINGULAR] = 1;
            // pitch = asin(mu) * 180/pi (:83) is increasing in mu: away from the two thresholds the comparison is made on mu itself,
            // within 1e-12 of one (or for NaN) on the reference's own expression
            bool loose, tight;
            if (fabs(mu - s_loose) > 1e-12 && fabs(mu - s_tight) > 1e-12) { loose = mu < s_loose; tight = mu < s_tight; }
            else {
                const double pitch = asin(mu) * 180.0 / 3.141592653589793;
                loose = pitch < a.loose_deg; tight = pitch < a.tight_deg;
            }
            H1[t] = h;
            F1[t] = (uint8_t)((loose ? 1 : 0) | (tight ? 2 : 0));                            // :85-86
            if (a.tri_height) a.tri_height[tb + t] = h;
            if (loose) {
                const unsigned long long u = (unsigned long long)__double_as_longlong(h);
                ++k_mine; umin = u < umin ? u : umin; umax = u > umax ? u : umax;
            }
        };
        for (int t0 = tid; t0 < tn; t0 += kStaticRows * BLK) {
            TriIds cur[kStaticRows];
#pragma unroll
            for (int j = 0; j < kStaticRows; ++j) cur[j] = rows[j];
            if (t0 + kStaticRows * BLK < tn) load_rows(t0 + kStaticRows * BLK);
#pragma unroll
            for (int j = 0; j < kStaticRows; ++j) if (t0 + j * BLK < tn) one_row(cur[j], t0 + j * BLK);
        }
    }
    k_mine = wave_sum(k_mine);
    umin = wave_min_u64(umin); umax = wave_max_u64(umax);
    if (lane == 0 && k_mine) { atomicAdd(&misc[TM_K], k_mine); atomicMin(&ext[0], umin); atomicMax(&ext[1], umax); }
    __syncthreads();                                             // (the planes are dead: their room is the histogram's)
    const unsigned long long *U = reinterpret_cast<const unsigned long long *>(Hh);
    const int k = misc[TM_K];
    // ---- the level (:91): np.median of the loose heights, as flat_selection_kernel searches it
    double level = nan("");                                      // median of an empty set is nan (nothing passes)
    double vlo = nan(""), vhi = nan("");                         // the two middle order statistics (one, twice, for an odd k)
    if (k > 0) {
        const int klo = (k - 1) >> 1, khi = k >> 1;
        unsigned long long lo = ext[0], hi = ext[1];
        int rank = klo;
        unsigned long long vlo_bits = lo;
        for (;;) {
            const unsigned long long range = hi - lo;
            if (range == 0ull) { vlo_bits = lo; break; }
            const int bits = 64 - __clzll((long long)range);                             // range < 2^bits
            const int shift = bits > 11 ? bits - 11 : 0;
            for (int b = tid; b < kStaticBins; b += BLK) hist[b] = 0;
            __syncthreads();
#pragma unroll 4
            for (int t = tid; t < tn; t += BLK) {
                if (!(Fl[t] & 1)) continue;
                const unsigned long long u = U[t];
                if (u >= lo && u <= hi) atomicAdd(&hist[(int)((u - lo) >> shift)], 1);
            }
            __syncthreads();
            {   // the bin whose cumulative count passes the rank: two bins per thread, wave scan, wave totals through LDS
                constexpr int BPT = kStaticBins / BLK;
                static_assert(BPT == 2, "flat_static_tri_kernel: two bins per thread");
                const int b0 = hist[BPT * tid], b1 = hist[BPT * tid + 1];
                const int mine = b0 + b1;
                int incl = wave_scan_incl(mine);
                if (lane == kWave - 1) misc[TM_WSUM + wave] = incl;
                __syncthreads();
                int before = 0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) if (w < wave) before += misc[TM_WSUM + w];
                incl += before;
                const int excl = incl - mine;
                if (rank >= excl && rank < incl) {               // exactly one thread
                    int r = rank - excl, bin = BPT * tid, c = b0;
                    if (r >= b0) { r -= b0; ++bin; c = b1; }
                    misc[TM_BIN] = bin; misc[TM_RANK] = r; misc[TM_BINCNT] = c;
                }
                __syncthreads();
            }
            const int bin = misc[TM_BIN], c = misc[TM_BINCNT];
            rank = misc[TM_RANK];
            lo += (unsigned long long)bin << shift;
            { const unsigned long long top = lo + ((1ull << shift) - 1ull); hi = top < hi ? top : hi; }
            if (shift == 0) { vlo_bits = lo; break; }            // the bin is one pattern
            if (c <= kStaticDirect) {
                unsigned long long *list = reinterpret_cast<unsigned long long *>(hist);
                __syncthreads();                                 // every thread has read misc / hist
#pragma unroll 4
                for (int t = tid; t < tn; t += BLK) {
                    if (!(Fl[t] & 1)) continue;
                    const unsigned long long u = U[t];
                    if (u >= lo && u <= hi) list[atomicAdd(&misc[TM_LIST], 1)] = u;
                }
                __syncthreads();
                if (wave == 0) {
                    const unsigned long long mine = lane < c ? list[lane] : ~0ull;
                    int below = 0;
                    for (int j = 0; j < c; ++j) { const unsigned long long v = list[j]; below += (v < mine || (v == mine && j < lane)) ? 1 : 0; }
                    if (lane < c && below == rank) ext[3] = mine;
                }
                __syncthreads();
                vlo_bits = ext[3];
                break;
            }
            __syncthreads();                                     // hist is zeroed again at the top
        }
        vlo = __longlong_as_double((long long)vlo_bits);
        vhi = vlo;
        if (khi != klo) {
            int le = 0;
            unsigned long long above = ~0ull;
#pragma unroll 4
            for (int t = tid; t < tn; t += BLK) {
                if (!(Fl[t] & 1)) continue;
                const unsigned long long u = U[t];
                if (u <= vlo_bits) ++le; else above = u < above ? u : above;
            }
            vhi = __longlong_as_double((long long)next_order_statistic(le, above, vlo_bits, khi, &misc[TM_LE], &ext[2]));
        }
        level = a.height_factor * ((klo == khi) ? vlo : (vlo + vhi) / 2.0);
    }
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
        if (lane == 0 && kept) atomicAdd(&misc[TM_KEPT], kept);
        if (lane < kStaticModelBins && mine) atomicAdd(&model[lane], mine);
        if (__ballot(badh) != 0ull && lane == 0) misc[TM_BADH] = 1;
    }
    __syncthreads();
    // ---- decide, as static_tri_kernel does (scale_calculator.py:299-310, :446-483)
    if (wave == 0) {
        const int flat_err = misc[TM_BADID] ? MVOSR_ST_ERR_MASK : (misc[TM_SINGULAR] ? MVOSR_ST_ERR_SINGULAR : 0);
        const bool refused = misc[TM_BADH] != 0;
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
            a.n_kept[f] = misc[TM_KEPT];
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
