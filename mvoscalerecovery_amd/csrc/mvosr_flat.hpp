// mvosr_flat.hpp — the one home of what the five flat-selection kernels share: flat_selection_kernel, both
// forms (mvosr_rescale.hip), flat_ransac_cases_kernel (mvosr_rescale_cases.hip), flat_selection_sweep_kernel
// (mvosr_rescale_sweep.hip), flat_ransac_large_kernel (mvosr_rescale_large.hip) and flat_static_tri_kernel, both forms
// (mvosr_rescale_static.hip).  Every one of them is pinned, bit for bit, to flat_selection_kernel: they agree because they call
// the same functions.  What is restated here, of the reference's src/ (the plane fit's under src/thirdparty/Ransac/ and src/):
//   the refusal of a frame (no features, no rows, a declined triangulation, more than the launch has room for),
//   the survivors' ordered compaction, feature3d[valid_id]                                         rescale.py:134-135
//   a row's height and the sine of its pitch, and the row's two bits against the two thresholds    rescale.py:79-89
//   the level: factor * np.median of the loose rows' heights                                       rescale.py:91
//   the hypotheses of the plane fit, from triples or from the sample sequence                      ransac.py:10-11, estimate_road_norm.py:13-15
//   the best hypothesis, its sign and the raw scale                                                ransac.py:9-22, rescale.py:156-167
// The shared constants (kFlatBins, kFlatDirect) and the misc[] slots (FM_*) are mvosr_rescale_plan.hpp's: the LDS plans, which a
// host compiler reads, size their regions by them.  Device code only; included after mvosr_device.hpp and mvosr_ransac.hpp.  fp64,
// compiled with -ffp-contract=off: the association order written here is the one every kernel's results are pinned to.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mvosr.h"
#include "mvosr_rescale_plan.hpp"

namespace mvosr {

constexpr int kFlatRows = 4;            // triangle rows a thread keeps in flight (flat_phase1)

// ---- the refusal: 0 where the frame is taken, else the status every kernel of the family reports for it.  `oversize`: more
// features or rows than the launch was sized for (the header's max_feat, the call's max_tri) — refused, nothing touched.
__device__ __forceinline__ int flat_entry_status(int n_all, int tn, bool skip, bool oversize) {
    if (!(n_all <= 0 || tn <= 0 || skip || oversize)) return 0;
    return (!skip && oversize && n_all > 0 && tn > 0) ? MVOSR_ST_ERR_MASK : MVOSR_ST_ERR_EMPTY;
}

// ---- ordered compaction of the survivors at load (rescale.py:134-135: feature3d[valid_id]): feature i of (sx, sy, sz) takes
// part iff keep[i] >= 0 (keep null: all do).  Every wavefront owns a contiguous segment of the frame, counts its survivors, and
// after one barrier — ordered_prefix's, through `slots`: every thread of the workgroup calls this — knows where its segment
// starts in (dx, dy, dz).  Returns the survivors' number.
template <int WAVES>
__device__ __forceinline__ int flat_compact_survivors(int n_all, const int32_t *keep, const double *sx, const double *sy, const double *sz,
                                                      double *dx, double *dy, double *dz, int *slots) {
    const int lane = lane_id();
    int s0, s1;
    ordered_segment(n_all, WAVES * kWave, s0, s1);
    int c = 0;
    for (int i0 = s0; i0 < s1; i0 += kWave) {
        const int i = i0 + lane;
        c += __popcll(__ballot(i < s1 && (!keep || keep[i] >= 0)));
    }
    int base, n;
    ordered_prefix<WAVES>(slots, c, base, n);
    for (int i0 = s0; i0 < s1; i0 += kWave) {
        const int i = i0 + lane;
        const bool k = i < s1 && (!keep || keep[i] >= 0);
        const int pos = ordered_rank(k, base);
        if (k) { dx[pos] = sx[i]; dy[pos] = sy[i]; dz[pos] = sz[i]; }
    }
    return n;
}

// ---- a row (rescale.py:79-89).  The thresholds are compared on mu, the sine of the pitch: sin(deg) of a threshold
__device__ __forceinline__ double flat_sin_deg(double deg) { return sin(deg * 3.141592653589793 / 180.0); }

// A row's two bits — bit 0: pitch < loose, bit 1: pitch < tight (:85-86).  pitch = asin(mu) * 180/pi (:83) is increasing in mu:
// away from the two thresholds the comparison is made on mu itself, within 1e-12 of one (or for NaN) on the reference's own
// expression.
__device__ __forceinline__ unsigned flat_row_bits(double mu, double s_loose, double s_tight, double loose_deg, double tight_deg) {
    bool loose, tight;
    if (fabs(mu - s_loose) > 1e-12 && fabs(mu - s_tight) > 1e-12) { loose = mu < s_loose; tight = mu < s_tight; }
    else { const double pitch = asin(mu) * 180.0 / 3.141592653589793; loose = pitch < loose_deg; tight = pitch < tight_deg; }
    return (loose ? 1u : 0u) | (tight ? 2u : 0u);
}

// Row q over the n survivors' planes: the sine of its pitch and its height (row_height_pitch, mvosr_device.hpp).  bad_id: the
// row names a vertex outside [0, n) — nothing is read, mu and h are NaN; singular: a zero pivot.  The caller stores and tallies.
struct FlatRow { double mu, h; bool bad_id, singular; };
__device__ __forceinline__ FlatRow flat_row(const double *X, const double *Y, const double *Z, const TriIds q, int n) {
    FlatRow r = {nan(""), nan(""), !ids_in_range(q.a, q.b, q.c, n), false};
    if (!r.bad_id) r.singular = !row_height_pitch(X, Y, Z, q, r.mu, r.h);
    return r;
}

// The search's state in LDS: misc[] below FM_WSUM zeroed, ext = {smallest, largest loose pattern, smallest above the median}.
// The caller's next barrier publishes it.
__device__ __forceinline__ void flat_state_init(int *misc, unsigned long long *ext) {
    if (threadIdx.x < FM_WSUM) misc[threadIdx.x] = 0;
    if (threadIdx.x == 0) { ext[0] = ~0ull; ext[1] = 0ull; ext[2] = ~0ull; }
}

// A thread's tally of the loose rows it met: their number and the bounds of their heights' bit patterns (heights are >= 0: the
// patterns order like the values).  commit() adds the wavefront's to the workgroup's: misc[FM_K], ext[0], ext[1].
struct FlatLoose {
    int k = 0;
    unsigned long long umin = ~0ull, umax = 0ull;
    __device__ __forceinline__ void add(double h) {
        const unsigned long long u = (unsigned long long)__double_as_longlong(h); ++k; umin = u < umin ? u : umin; umax = u > umax ? u : umax;
    }
    __device__ __forceinline__ void commit(int *misc, unsigned long long *ext) {
        k = wave_sum(k); umin = wave_min_u64(umin); umax = wave_max_u64(umax);
        if (lane_id() == 0 && k) { atomicAdd(&misc[FM_K], k); atomicMin(&ext[0], umin); atomicMax(&ext[1], umax); }
    }
};

// Phase 1 of flat_selection_kernel and of flat_static_tri_kernel<false>: every row's height and two bits into Hh / Fl by row
// (LDS), the height to tri_height (the frame's rows in global memory; null: not wanted), the loose rows tallied, bad ids and zero
// pivots flagged in misc.  A thread's next kFlatRows rows are in flight while it works on the current ones — a row is a dependent
// global load in front of nine LDS gathers and the LU chain —: the caller starts with flat_load_rows(tri, tid, tn, rows) BEFORE
// it loads the vertex planes, so that the first rows arrive while the planes stream in.  `tri`: the frame's first row.
template <int BLK>
__device__ __forceinline__ void flat_load_rows(const int32_t *tri, int t0, int tn, TriIds (&rows)[kFlatRows]) {
#pragma unroll
    for (int j = 0; j < kFlatRows; ++j) rows[j] = load_tri(tri, min(t0 + j * BLK, tn - 1));
}
template <int BLK>
__device__ __forceinline__ void flat_phase1(const int32_t *tri, TriIds (&rows)[kFlatRows], int tn, const double *X, const double *Y,
                                            const double *Z, int n, double loose_deg, double tight_deg, double s_loose, double s_tight,
                                            double *Hh, uint8_t *Fl, double *tri_height, int *misc, FlatLoose &tally) {
    const int tid = threadIdx.x;
    for (int t0 = tid; t0 < tn; t0 += kFlatRows * BLK) {
        TriIds cur[kFlatRows];
#pragma unroll
        for (int j = 0; j < kFlatRows; ++j) cur[j] = rows[j];
        if (t0 + kFlatRows * BLK < tn) flat_load_rows<BLK>(tri, t0 + kFlatRows * BLK, tn, rows);
#pragma unroll
        for (int j = 0; j < kFlatRows; ++j) {
            const int t = t0 + j * BLK;
            if (t >= tn) continue;
            const FlatRow r = flat_row(X, Y, Z, cur[j], n);
            if (r.bad_id) { misc[FM_BADID] = 1; Fl[t] = 0; Hh[t] = r.h; if (tri_height) tri_height[t] = r.h; continue; }
            if (r.singular) misc[FM_SINGULAR] = 1;
            const unsigned bits = flat_row_bits(r.mu, s_loose, s_tight, loose_deg, tight_deg);
            Hh[t] = r.h;
            Fl[t] = (uint8_t)bits;
            if (tri_height) tri_height[t] = r.h;
            if (bits & 1u) tally.add(r.h);
        }
    }
}

// ---- the level (rescale.py:91): factor * np.median of the k loose rows' heights — the mean of the two middle order statistics,
// vlo and vhi (one, twice, for an odd k); all three NaN for k = 0 (the median of an empty set: nothing passes).
// Row t is loose iff Fl[t] & 1, and U[t] is its height's bit pattern; both may lie in LDS or in global memory.  The lower middle
// one (rank (k - 1) / 2): histogram the candidates' patterns over [lo, hi] = ext[0..1] with bins of 2^shift patterns (<= kFlatBins
// bins, `hist`), find the bin that holds the rank, narrow [lo, hi] to it, repeat — until a bin is a single pattern, or holds few
// enough candidates (<= kFlatDirect) for wavefront 0 to rank them directly, listed where the histogram was.  Real frames take one
// pass: their heights spread over a few thousand distinct patterns per bin at most.  The upper middle one by one more sweep
// (next_order_statistic).  misc / ext as flat_state_init left them, k = misc[FM_K] behind FlatLoose::commit and a barrier.
// Holds barriers: every thread of the WAVES-wavefront workgroup calls it, and every thread returns the same values.
// ROLLED: the form of a kernel whose scalar registers are full (flat_ransac_large_kernel) — the row sweeps are not unrolled by
// request, and the ranking loop is kept rolled: eight trips' compare masks at once were forty scalar registers, spilled there.
struct FlatLevel { double vlo, vhi, level; };

template <int BLK, bool ROLLED, typename F>
__device__ __forceinline__ void flat_each_loose(const unsigned long long *U, const uint8_t *Fl, int tn, F f) {
    if constexpr (ROLLED) {
        for (int t = threadIdx.x; t < tn; t += BLK) if (Fl[t] & 1) f(U[t]);
    } else {
#pragma unroll 4
        for (int t = threadIdx.x; t < tn; t += BLK) if (Fl[t] & 1) f(U[t]);
    }
}

template <int WAVES, bool ROLLED = false>
__device__ __forceinline__ FlatLevel flat_level_search(const unsigned long long *U, const uint8_t *Fl, int tn, int k, unsigned long long *ext,
                                                       int *misc, int *hist, double factor) {
    constexpr int BLK = WAVES * kWave, BPT = kFlatBins / BLK;        // bins per thread (4 with 512 threads, 2 with 1024)
    static_assert(WAVES <= 16 && kFlatBins % BLK == 0, "flat_level_search: misc slots / bins per thread");
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    FlatLevel res = {nan(""), nan(""), nan("")};
    if (k <= 0) return res;
    const int klo = (k - 1) >> 1, khi = k >> 1;
    unsigned long long lo = ext[0], hi = ext[1];
    int rank = klo;
    unsigned long long vlo_bits = lo;
    for (;;) {
        const unsigned long long range = hi - lo;
        if (range == 0ull) { vlo_bits = lo; break; }
        const int bits = 64 - __clzll((long long)range);                             // range < 2^bits
        const int shift = bits > 11 ? bits - 11 : 0;
        for (int b = tid; b < kFlatBins; b += BLK) hist[b] = 0;
        __syncthreads();
        flat_each_loose<BLK, ROLLED>(U, Fl, tn, [&](const unsigned long long u) {
            if (u >= lo && u <= hi) atomicAdd(&hist[(int)((u - lo) >> shift)], 1);
        });
        __syncthreads();
        {   // the bin whose cumulative count passes the rank: BPT bins per thread, wave scan, wave totals through LDS
            int b[BPT], mine = 0;
#pragma unroll
            for (int j = 0; j < BPT; ++j) { b[j] = hist[BPT * tid + j]; mine += b[j]; }
            int incl = wave_scan_incl(mine);
            if (lane == kWave - 1) misc[FM_WSUM + wave] = incl;
            __syncthreads();
            int before = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) if (w < wave) before += misc[FM_WSUM + w];
            incl += before;
            const int excl = incl - mine;
            if (rank >= excl && rank < incl) {                   // exactly one thread
                int r = rank - excl, bin = BPT * tid, c = b[0];
#pragma unroll
                for (int j = 1; j < BPT; ++j) if (r >= c) { r -= c; ++bin; c = b[j]; }   // (r < c once the bin is found: no later step)
                misc[FM_BIN] = bin; misc[FM_RANK] = r; misc[FM_BINCNT] = c;
            }
            __syncthreads();
        }
        const int bin = misc[FM_BIN], c = misc[FM_BINCNT];
        rank = misc[FM_RANK];
        lo += (unsigned long long)bin << shift;
        { const unsigned long long top = lo + ((1ull << shift) - 1ull); hi = top < hi ? top : hi; }
        if (shift == 0) { vlo_bits = lo; break; }                // the bin is one pattern
        if (c <= kFlatDirect) {
            unsigned long long *list = reinterpret_cast<unsigned long long *>(hist);
            __syncthreads();                                     // every thread has read misc / hist
            flat_each_loose<BLK, ROLLED>(U, Fl, tn, [&](const unsigned long long u) {
                if (u >= lo && u <= hi) list[atomicAdd(&misc[FM_LIST], 1)] = u;
            });
            __syncthreads();
            if (wave == 0) {
                const unsigned long long mine = lane < c ? list[lane] : ~0ull;
                int below = 0;
                auto count = [&](int j) { const unsigned long long v = list[j]; below += (v < mine || (v == mine && j < lane)) ? 1 : 0; };
                if constexpr (ROLLED) {
#pragma unroll 1
                    for (int j = 0; j < c; ++j) count(j);
                } else {
                    for (int j = 0; j < c; ++j) count(j);
                }
                if (lane < c && below == rank) ext[3] = mine;
            }
            __syncthreads();
            vlo_bits = ext[3];
            break;
        }
        __syncthreads();                                         // hist is zeroed again at the top
    }
    res.vlo = __longlong_as_double((long long)vlo_bits);
    res.vhi = res.vlo;
    if (khi != klo) {
        int le = 0;
        unsigned long long above = ~0ull;
        flat_each_loose<BLK, ROLLED>(U, Fl, tn, [&](const unsigned long long u) {
            if (u <= vlo_bits) ++le; else above = u < above ? u : above;
        });
        res.vhi = __longlong_as_double((long long)next_order_statistic(le, above, vlo_bits, khi, &misc[FM_LE], &ext[2]));
    }
    res.level = factor * ((klo == khi) ? res.vlo : (res.vlo + res.vhi) / 2.0);
    return res;
}

// ---- the plane fit's hypotheses (ransac.py:10-11, estimate_road_norm.py:13-15), one thread each: hypothesis h is the unit plane
// through three of the n survivors — those `triples` names (the frame's [H][3], survivor-numbered, clamped to [0, n); null: the
// draw), else those at the three positions ransac_draw3 draws under `key` from the point list L of M entries (list positions:
// mvosr_ransac.hpp on a vertex drawn twice) — with its inlier count zeroed.  A plane is stored as the kernel's counting loop reads
// it: one double4 (ransac_count_resident), or (nx, ny), (nz, d) as two double2 (ransac_count_weighted).
__device__ __forceinline__ void flat_store_plane(double4 *mods, int h, const double4 m) { mods[h] = m; }
__device__ __forceinline__ void flat_store_plane(double2 *mods, int h, const double4 m) { mods[2 * h] = make_double2(m.x, m.y); mods[2 * h + 1] = make_double2(m.z, m.w); }
__device__ __forceinline__ double4 flat_load_plane(const double4 *mods, int h) { return mods[h]; }
__device__ __forceinline__ double4 flat_load_plane(const double2 *mods, int h) { const double2 b0 = mods[2 * h], b1 = mods[2 * h + 1]; return make_double4(b0.x, b0.y, b1.x, b1.y); }
template <int BLK, typename Plane, typename Id>
__device__ __forceinline__ void flat_build_hypotheses(uint64_t key, const int32_t *triples, int H, int n, int M, const Id *L, const double *X,
                                                      const double *Y, const double *Z, Plane *mods, int *cnts) {
    for (int h = threadIdx.x; h < H; h += BLK) {
        int v0, v1, v2;
        if (triples) {
            const int32_t *t = triples + 3 * h;
            v0 = min(max(t[0], 0), n - 1); v1 = min(max(t[1], 0), n - 1); v2 = min(max(t[2], 0), n - 1);
        } else {
            ransac_draw3(key, h, M, v0, v1, v2);
            v0 = L[v0]; v1 = L[v1]; v2 = L[v2];
        }
        flat_store_plane(mods, h, ransac_unit_plane(X, Y, Z, v0, v1, v2));
        cnts[h] = 0;
    }
}

// ---- the plane fit's result, by wavefront 0 (every lane calls it and returns the same): the replay of ransac.py:9-22 over the H
// counts towards `goal` (estimate_road_norm.py:68), the best plane under the sign rule (rescale.py:159-161) and the raw scale
// (:158-167).  `fit` false — the selection failed or left too few points (:152) —: nothing is read, `status` stands, the doubles
// are NaN.  A fit without a single inlier (NaN planes only) is MVOSR_ST_RS_FEW.
struct FlatRansacResult { int status, best, best_ic, used; double m[4], raw; };
template <typename Plane>
__device__ __forceinline__ FlatRansacResult flat_ransac_result(bool fit, int status, const Plane *mods, const int *cnts, int H, double goal,
                                                               double absolute_reference) {
    FlatRansacResult r = {status, -1, 0, 0, {nan(""), nan(""), nan(""), nan("")}, nan("")};
    if (fit) {
        RansacReplay rp = {-1, 0, H, 0};
        ransac_replay(rp, cnts, 0, H, goal);
        r.best = rp.best; r.best_ic = rp.best_ic; r.used = rp.used;
        if (r.best >= 0) {
            const double4 bm = ransac_sign_rule(flat_load_plane(mods, r.best));
            r.m[0] = bm.x; r.m[1] = bm.y; r.m[2] = bm.z; r.m[3] = bm.w;
            r.raw = absolute_reference / ransac_camera_height(bm);
        } else r.status = MVOSR_ST_RS_FEW;
    }
    return r;
}

}  // namespace mvosr
