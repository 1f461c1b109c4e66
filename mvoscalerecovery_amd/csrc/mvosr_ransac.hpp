// mvosr_ransac.hpp — the one home of the rules the five plane-fit kernels share: ransac_plane_kernel and
// flat_selection_kernel<true> (mvosr_rescale.hip), flat_ransac_cases_kernel (mvosr_rescale_cases.hip), height_pitch_kernel
// (mvosr_heightpitch.hip) and height_pitch_eval_kernel (mvosr_hpeval.hip).  The sample sequence, the models, the replay of
// /root/reference/src/thirdparty/Ransac/ransac.py:9-22, the sign rule and the height, the two counting loops and the ordered
// compaction.  Device code only (the sequence's two key functions are host code as well); included after mvosr_device.hpp.  fp64,
// compiled with -ffp-contract=off: the association order written here is the one every kernel's results are pinned to.
// What the flat-selection kernels build from these — a frame's hypotheses, the fit's result, the survivors' compaction — and
// their own rules (a row's bits, the level's search) is mvosr_flat.hpp, included after this file.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace mvosr {

// ---- the sample sequence (include/mvosr.h, mvosr_flat_ransac_batch): splitmix64's finaliser as a counter-based generator.
// oracle/rescale_oracle.py restates it.
__host__ __device__ __forceinline__ constexpr uint64_t ransac_mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static_assert(ransac_mix64(0) == 0xE220A8397B1DCDAFull && ransac_mix64(1) == 0x910A2DEC89025CC1ull, "ransac_mix64: oracle.rescale_oracle.mix64");
// the key of a frame's hypotheses: its sample-sequence counter under the run's seed
__host__ __device__ __forceinline__ constexpr uint64_t ransac_frame_key(uint64_t seed, uint64_t frame_counter) {
    return ransac_mix64(seed ^ (frame_counter * 0xD1B54A32D192ED03ull));
}
// Hypothesis h of a frame: three distinct list positions, uniform (ransac.py:10, random.sample over the list).  The list repeats
// every vertex once per kept triangle (rescale.py:101), so 0.5-2 % of the samples name one VERTEX twice.  The reference spends
// the iteration on such a sample (ransac.py:8-21): its SVD of the rank-2 matrix returns a plane that rounding noise picks from
// the pencil through two points.  Here the iteration is spent as well — the sample is NOT drawn again (rounds 4-5 did, a
// declared deviation that inflated the iteration budget) —: the cross product of a repeated vertex is exactly zero, the model
// NaN, the hypothesis counts zero inliers and can never be the best — what the id_triples path has always done with such a
// triple (pinned against the reference's own run on such triples: tests/golden/rescale.npz frame 26).
// ransac_draw2: a pair of distinct positions, the first two of ransac_draw3.
__device__ __forceinline__ void ransac_draw2(uint64_t key, int h, int M, int &i0, int &i1) {
    const uint64_t hk = ransac_mix64(key + (uint64_t)h);
    i0 = (int)__umul64hi(ransac_mix64(hk), (uint64_t)M);                             // uniform on [0, M) up to M / 2^64
    i1 = (int)__umul64hi(ransac_mix64(hk + 1ull), (uint64_t)(M - 1)); if (i1 >= i0) ++i1;   // ... on the M - 1 other positions
}
__device__ __forceinline__ void ransac_draw3(uint64_t key, int h, int M, int &i0, int &i1, int &i2) {
    ransac_draw2(key, h, M, i0, i1);
    i2 = (int)__umul64hi(ransac_mix64(ransac_mix64(key + (uint64_t)h) + 2ull), (uint64_t)(M - 2));
    const int lo = min(i0, i1), hi = max(i0, i1);
    if (i2 >= lo) ++i2;
    if (i2 >= hi) ++i2;
}

// ---- the models: the unit 4-vector (n, d) / |(n, d)| — the null vector the reference gets from the SVD of [x y z 1]
// (estimate_road_norm.py:13-15) or [x y 1] (:44-46), up to sign.  A sample that names one point twice gives NaN.
// the cross product of the edges p1 - p0 and p2 - p0
__device__ __forceinline__ void ransac_edge_cross(double x0, double y0, double z0, double x1, double y1, double z1, double x2, double y2,
                                                  double z2, double &nx, double &ny, double &nz) {
    const double e1x = x1 - x0, e1y = y1 - y0, e1z = z1 - z0;
    const double e2x = x2 - x0, e2y = y2 - y0, e2z = z2 - z0;
    nx = e1y * e2z - e1z * e2y; ny = e1z * e2x - e1x * e2z; nz = e1x * e2y - e1y * e2x;
}
__device__ __forceinline__ double4 ransac_unit_model(double nx, double ny, double nz, double d) {
    const double inv = 1.0 / sqrt(((nx * nx + ny * ny) + nz * nz) + d * d);
    double4 m; m.x = nx * inv; m.y = ny * inv; m.z = nz * inv; m.w = d * inv;
    return m;
}
// the plane through points i0, i1, i2 of (X, Y, Z)
__device__ __forceinline__ double4 ransac_unit_plane(const double *X, const double *Y, const double *Z, int i0, int i1, int i2) {
    const double x0 = X[i0], y0 = Y[i0], z0 = Z[i0];
    double nx, ny, nz;
    ransac_edge_cross(x0, y0, z0, X[i1], Y[i1], Z[i1], X[i2], Y[i2], Z[i2], nx, ny, nz);
    return ransac_unit_model(nx, ny, nz, -((nx * x0 + ny * y0) + nz * z0));
}
// the line a u + b v + c = 0 through points i0, i1 of (U, V), as (a, b, 0, c)
__device__ __forceinline__ double4 ransac_unit_line(const double *U, const double *V, int i0, int i1) {
    const double u0 = U[i0], v0 = V[i0];
    const double nx = V[i1] - v0, ny = -(U[i1] - u0);
    return ransac_unit_model(nx, ny, 0.0, -(nx * u0 + ny * v0));
}

// ---- the replay of ransac.py:9-22 — a hypothesis is the new best when it counts MORE than the best so far, and the loop stops
// at a new best above the goal — by one wavefront, 64 counts at a time: the loop stops at the first count above the goal (the
// best before it was not, so it is a new best; a count of zero is never a new best), and the best is the first occurrence of the
// largest count up to there.  cnts[0..T) are the counts of hypotheses h0 .. h0 + T - 1; the state is carried from one call to
// the next (a caller that holds the counts in tiles) and starts as {-1, 0, H, 0}.  Every lane of the wavefront calls it and ends
// with the same state.  (One thread walking a hundred counts was 16 % of flat_selection_kernel<true>'s time.)
struct RansacReplay { int best, best_ic, used, done; };
__device__ __forceinline__ void ransac_replay(RansacReplay &s, const int *cnts, int h0, int T, double goal) {
    const int lane = lane_id();
    for (int t0 = 0; t0 < T; t0 += kWave) {
        const int t = t0 + lane;
        const int c = t < T ? cnts[t] : -1;
        const unsigned long long over = __ballot(c > 0 && (double)c > goal);
        const int limit = over ? (int)__ffsll((long long)over) - 1 : kWave - 1;
        const bool in = t < T && lane <= limit;
        const int mx = wave_max(in ? c : -1);
        if (mx > s.best_ic) {
            const unsigned long long who = __ballot(in && c == mx);
            s.best = h0 + t0 + (int)__ffsll((long long)who) - 1; s.best_ic = mx;
        }
        if (over) { s.used = h0 + t0 + limit + 1; s.done = 1; break; }
    }
}

// ---- the sign rule (rescale.py:159-161: the model's second slot is not negative) and the camera height (:158, :162-165)
__device__ __forceinline__ double4 ransac_sign_rule(double4 m) {
    const double sgn = (m.y < 0.0) ? -1.0 : 1.0;
    m.x = sgn * m.x; m.y = sgn * m.y; m.z = sgn * m.z; m.w = sgn * m.w;
    return m;
}
__device__ __forceinline__ double ransac_camera_height(const double4 m) {
    const double h_bar = -m.w;
    const double norm_norm = sqrt((m.x * m.x + m.y * m.y) + m.z * m.z) / h_bar;
    return 1.0 / norm_norm;
}

// ---- inlier counts (estimate_road_norm.py:17-18), weighted: `n_items` distinct points, each counting with its multiplicity.  A
// wavefront takes its hypotheses (wave, wave + WAVES, ...) seven at a time, their planes — mods[2 h] = (nx, ny), mods[2 h + 1] =
// (nz, d) — in registers: a point is fetched once per pass and tested against all seven (one hypothesis per pass spent 41 % of
// flat_selection_kernel<true>'s time on the fetches).  fetch(j, px, py, pz, wgt) reads item j: `fetch_packed` where the caller
// laid coordinates and multiplicities side by side (`packed`), `fetch_gather` by vertex id otherwise.  Writes cnts[0..H).
constexpr int kRansacHypPass = 7;
template <int WAVES, typename Packed, typename Gather>
__device__ __forceinline__ void ransac_count_weighted(const double2 *mods, int *cnts, int H, int n_items, double threshold, bool packed,
                                                      Packed fetch_packed, Gather fetch_gather) {
    const int lane = lane_id(), wave = wave_id();
    for (int k0 = 0; wave + WAVES * k0 < H; k0 += kRansacHypPass) {
        double2 ma[kRansacHypPass], mb[kRansacHypPass];
        int acc[kRansacHypPass];
#pragma unroll
        for (int q = 0; q < kRansacHypPass; ++q) {
            const int h = min(wave + WAVES * (k0 + q), H - 1);
            ma[q] = mods[2 * h]; mb[q] = mods[2 * h + 1]; acc[q] = 0;
        }
        auto pass = [&](auto fetch) {
            for (int j = lane; j < n_items; j += kWave) {
                double px, py, pz;
                int wgt;
                fetch(j, px, py, pz, wgt);
#pragma unroll
                for (int q = 0; q < kRansacHypPass; ++q)
                    acc[q] += (fabs(((px * ma[q].x + py * ma[q].y) + pz * mb[q].x) + mb[q].y) < threshold) ? wgt : 0;   // estimate_road_norm.py:18
            }
        };
        if (packed) pass(fetch_packed); else pass(fetch_gather);
#pragma unroll
        for (int q = 0; q < kRansacHypPass; ++q) {
            const int h = wave + WAVES * (k0 + q);
            const int sum = wave_sum(acc[q]);
            if (lane == 0 && h < H) cnts[h] = sum;
        }
    }
}

// ---- inlier counts over a list of M points, repeats included: every thread of the BLK-thread workgroup keeps up to PPT points in
// registers (read once) and the T hypotheses stream past them from LDS (wave-uniform reads); a hypothesis' inliers among a
// wavefront's points are counted on the scalar unit (ballot + popcount), one integer LDS add per wavefront.  point(j, q0, q1, q2)
// reads list position j; a LINE model (a, b, 0, c) tests (q0, q1) alone.  Adds to cnts[0..T), which the caller has zeroed.
template <bool LINE, int PPT, int UNROLL, int BLK, typename Point>
__device__ __forceinline__ void ransac_count_resident(int M, const double4 *mods, int *cnts, int T, double threshold, Point point) {
    const int tid = threadIdx.x, lane = lane_id();
    for (int c0 = 0; c0 < M; c0 += BLK * PPT) {
        double q0[PPT], q1[PPT], q2[PPT];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int j = c0 + k * BLK + tid;
            point(min(j, M - 1), q0[k], q1[k], q2[k]);
            if (j >= M) q0[k] = nan("");                         // never an inlier: no masks or branches in the loop below
        }
        const int rows = min(PPT, (M - c0 + BLK - 1) / BLK);     // workgroup-uniform: rows that hold any point
#pragma unroll UNROLL
        for (int h = 0; h < T; ++h) {
            const double4 m = mods[h];
            int ic = 0;
#pragma unroll
            for (int k = 0; k < PPT; ++k)
                if (k < rows) {
                    const double r = LINE ? (q0[k] * m.x + q1[k] * m.y) + m.w : ((q0[k] * m.x + q1[k] * m.y) + q2[k] * m.z) + m.w;
                    ic += __popcll(__ballot(fabs(r) < threshold));                   // estimate_road_norm.py:18, :48
                }
            if (lane == 0 && ic) atomicAdd(&cnts[h], ic);
        }
    }
}

// ---- ordered compaction (feature3d[valid_id], triangle_ids[valid_id].reshape(-1)): every wavefront owns a contiguous segment
// of the items, counts its survivors, and after one barrier knows where its segment starts in the output — no sort, no atomics.
// the segment [s0, s1) of n items that the calling wavefront of a `blk`-thread workgroup owns
__device__ __forceinline__ void ordered_segment(int n, int blk, int &s0, int &s1) {
    const int seg = ((n + blk - 1) / blk) * kWave;
    s0 = wave_id() * seg; s1 = min(n, s0 + seg);
}
// from the calling wavefront's count c: where its survivors start (base) and the workgroup's total, through `slots` (WAVES ints).
// Holds a barrier: every thread of the workgroup calls it.
template <int WAVES>
__device__ __forceinline__ void ordered_prefix(int *slots, int c, int &base, int &total) {
    const int wave = wave_id();
    if (lane_id() == 0) slots[wave] = c;
    __syncthreads();
    base = 0; total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { const int cw = slots[w]; total += cw; if (w < wave) base += cw; }
}
// the output position of a lane that keeps its item (one trip of the wavefront over 64 items); base moves past the trip's survivors
__device__ __forceinline__ int ordered_rank(bool keep, int &base) {
    const unsigned long long m = __ballot(keep);
    const int pos = base + __popcll(m & ((1ull << lane_id()) - 1ull));
    base += __popcll(m);
    return pos;
}

}  // namespace mvosr
