// mvosr_rescale.hip — kernels for the `rescale` variant of the scale estimator (the one
// /root/reference/src/main.py:20 imports): GraphChecker vote, flat_selection, and the RANSAC plane
// fit made deterministic by taking its sample triples as input.  SURVEY.md §8 rows f2, f4, a11, a13.
//
//   graph_inliers_kernel   GraphChecker.find_inliers        /root/reference/src/graph.py:18-36,124-145
//   flat_selection_kernel  ScaleEstimator.flat_selection    /root/reference/src/rescale.py:75-102
//   ransac_plane_kernel    run_ransac + estimate/is_inlier  /root/reference/src/thirdparty/Ransac/ransac.py:3-23,
//                                                           /root/reference/src/estimate_road_norm.py:8-18,66-70
//
// Same conventions as mvosr_kernels.hip: one frame per workgroup, fp64, planes staged in LDS,
// compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mvosr.h"
#include "mvosr_device.hpp"
#include "mvosr_ransac.hpp"
#include "mvosr_flat.hpp"
#include "mvosr_host.hpp"
#include "mvosr_rescale_plan.hpp"

namespace mvosr {

constexpr int kRsBlock = kRsWaves * kWave;
static_assert(sizeof(double4) == kPlaneBytes && 2 * sizeof(double2) == kPlaneBytes, "a hypothesis' plane in the LDS plans");

// ---------------------------------------------------------------------------------------------
// GraphChecker.find_inliers: per triangle the edge-order code a*4+b*2+c with
// a=(v0-v1)(d0-d1)<0, b=(v1-v2)(d1-d2)<0, c=(v0-v2)(d0-d2)<0 selects a column of the 8x8 triangle
// potential; the three vertex marginals of that column are compared with 0.6 on the HOST once (they
// depend on the code only), so the kernel receives 8x3 flag bits.  Each vertex tallies
// (incident triangles, triangles that vouch for it) in one 32-bit LDS word (low/high half).
// ---------------------------------------------------------------------------------------------
struct GraphArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *z, *v;
    const int64_t *tri_off; const int32_t *tri;
    uint32_t good_bits;            // bit 3*code+k: vertex k of a triangle with this code has marginal > 0.6
    int32_t *total, *good;         // [like z] outputs
    int32_t *status;               // [F] 0 ok / MVOSR_ST_ERR_MASK on a bad vertex id
    // the device-resident form (graph_inliers_kernel<true>, mvosr_graph_keep_batch): the decision itself
    const int32_t *tri_cnt;        // [F] rows of the frame (null: tri_off[f+1] - tri_off[f])
    const int32_t *dt_status;      // [F] non-zero: the frame's triangulation was declined — nothing to do (null: none)
    int32_t min_valid;             // rescale.py:133
    int32_t *keep;                 // [like z] 1 passed / 0 failed but the frame stays whole / -1 dropped
    int32_t *n_valid;              // [F] features that passed (null: not wanted)
    int32_t max_feat;              // what the launch's LDS was sized from
};

// A vertex's two tallies share one 32-bit LDS word, 16 bits each, and one row may name a vertex up to three times: with at most
// this many rows no tally can reach 2^16 (3 * 21845 = 65535) whatever the rows say.  (The rows are in global memory: nothing
// else bounds their number.  A triangulation has fewer than two rows per point, and the LDS holds ~8 000 points.)
constexpr int kGraphMaxRows = MVOSR_GRAPH_MAX_ROWS;
static_assert(3 * kGraphMaxRows <= 0xFFFF, "graph_inliers_kernel: a 16-bit tally must hold three times the row count");

template <bool KEEP>
__global__ __launch_bounds__(kRsBlock) void graph_inliers_kernel(const GraphArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int n = a.feat_cnt[f];
    if (n <= 0) { if (threadIdx.x == 0) { if (a.status) a.status[f] = MVOSR_ST_ERR_EMPTY; if (KEEP && a.n_valid) a.n_valid[f] = 0; } return; }
    if (KEEP && a.dt_status && a.dt_status[f] != 0) {
        // a declined first triangulation: the frame is redone on the host; its keep flags say "dropped" so that the second
        // triangulation and flat_selection of this chunk see an empty frame instead of whatever the recycled block held
        const int64_t off0 = a.feat_off[f];
        for (int i = threadIdx.x; i < n; i += kRsBlock) a.keep[off0 + i] = -1;
        if (threadIdx.x == 0) { if (a.status) a.status[f] = MVOSR_ST_ERR_EMPTY; if (a.n_valid) a.n_valid[f] = 0; }
        return;
    }
    const int64_t off = a.feat_off[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    if (n > a.max_feat || tn > kGraphMaxRows) {
        // more features than the LDS has room for, or enough rows for a 16-bit tally to carry into its neighbour: refused, LDS
        // untouched.  Stage form: no tallies.  Keep form: what a declined triangulation gets — an empty frame downstream.
        for (int i = threadIdx.x; i < n; i += kRsBlock) {
            if constexpr (KEEP) a.keep[off + i] = -1; else { a.total[off + i] = 0; a.good[off + i] = 0; }
        }
        if (threadIdx.x == 0) { if (a.status) a.status[f] = MVOSR_ST_ERR_MASK; if (KEEP && a.n_valid) a.n_valid[f] = 0; }
        return;
    }
    const auto lds = graph_plan<uint32_t>(n);
    double2 *P = reinterpret_cast<double2 *>(smem + lds.p);               // {v, z}
    uint32_t *cnt = reinterpret_cast<uint32_t *>(smem + lds.cnt);
    int *flag = reinterpret_cast<int *>(smem + lds.flag);                 // [0] bad vertex id, [1] features that passed
    const int tid = threadIdx.x;
    if (tid < 2) flag[tid] = 0;
    for (int i = tid; i < n; i += kRsBlock) {
        double2 p; p.x = a.v[off + i]; p.y = a.z[off + i];               // rescale.py:25: camera_pitch = 0, no remap
        P[i] = p;
        cnt[i] = 0u;
    }
    __syncthreads();
    int bad = 0;
    for (int t = tid; t < tn; t += kRsBlock) {
        const TriIds q = load_tri(a.tri + 3 * tb, t);
        if (!ids_in_range(q.a, q.b, q.c, n)) { bad = 1; continue; }
        const double2 p0 = P[q.a], p1 = P[q.b], p2 = P[q.c];
        const int ca = (p0.x - p1.x) * (p0.y - p1.y) < 0.0;              // graph.py:125
        const int cb = (p1.x - p2.x) * (p1.y - p2.y) < 0.0;              // graph.py:126
        const int cc = (p0.x - p2.x) * (p0.y - p2.y) < 0.0;              // graph.py:127
        const uint32_t g = a.good_bits >> (3 * (ca * 4 + cb * 2 + cc));  // graph.py:128,140-145
        atomicAdd(&cnt[q.a], 1u + ((g & 1u) << 16));                     // graph.py:28-30
        atomicAdd(&cnt[q.b], 1u + (((g >> 1) & 1u) << 16));
        atomicAdd(&cnt[q.c], 1u + (((g >> 2) & 1u) << 16));
    }
    if (bad) flag[0] = 1;
    __syncthreads();
    if constexpr (!KEEP) {
        for (int i = tid; i < n; i += kRsBlock) {
            const uint32_t c = cnt[i];
            a.total[off + i] = (int32_t)(c & 0xFFFFu);
            a.good[off + i] = (int32_t)(c >> 16);
        }
    } else {
        // good/total > 0.5 (graph.py:34-35,131-132): the quotient of two integers below 2^16 is above one half exactly when
        // 2*good > total (the nearest quotient below is 1/2 - 1/(2 total), far from a rounding); 0/0 is nan: dropped
        int mine = 0;
        for (int i = tid; i < n; i += kRsBlock) { const uint32_t c = cnt[i]; mine += (2u * (c >> 16) > (c & 0xFFFFu)) ? 1 : 0; }
        mine = wave_sum(mine);
        if (lane_id() == 0 && mine) atomicAdd(&flag[1], mine);
        __syncthreads();
        const int nv = flag[1];
        const int fail = nv > a.min_valid ? -1 : 0;                       // rescale.py:133-137: ten or fewer left — the frame stays whole
        for (int i = tid; i < n; i += kRsBlock) { const uint32_t c = cnt[i]; a.keep[off + i] = (2u * (c >> 16) > (c & 0xFFFFu)) ? 1 : fail; }
        if (tid == 0 && a.n_valid) a.n_valid[f] = nv;
    }
    if (tid == 0 && a.status) a.status[f] = flag[0] ? MVOSR_ST_ERR_MASK : 0;
}

// ---------------------------------------------------------------------------------------------
// flat_selection: per triangle n = A^-1 . 1 (LU, like np.matrix.I), heights = 1/|n|,
// pitch = asin(-n_y/|n|) deg; level = 0.9 * median(heights[pitch < -80]); a triangle is kept when
// pitch < -85 and heights > level.  The median is the mean of the two middle order statistics; every triangle's height
// and flags stay in LDS by row (no compacted list, no append counter), and the order statistic is found on the heights'
// bit patterns by a 2048-bin histogram over [smallest, largest] loose height — narrowed to the bin that holds the rank
// and repeated if needed — with wavefront 0 ranking the last <= 64 candidates directly.  The rules — a row's bits, the level's
// search, the survivors' compaction, the hypotheses and the fit's result — are mvosr_flat.hpp's, shared with the four sibling
// kernels (mvosr_rescale_cases.hip, _sweep.hip, _large.hip, _static.hip); this kernel keeps its phases' order and its LDS traffic.
// ---------------------------------------------------------------------------------------------
struct FlatArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *x, *y, *z;
    const int64_t *tri_off; const int32_t *tri;
    double loose_deg, tight_deg, height_factor;
    double *tri_height;            // [T] 1/|n|
    uint8_t *tri_flags;            // [T] bit0: pitch < loose, bit1: pitch < tight, bit2: kept
    double *height_level;          // [F]
    int32_t *status;               // [F] 0 / MVOSR_ST_ERR_SINGULAR / MVOSR_ST_ERR_MASK / MVOSR_ST_ERR_EMPTY
    int32_t *n_kept;               // [F]
    // the device-resident form (flat_selection_kernel<true>, mvosr_flat_ransac_batch): survivors compacted at load, explicit
    // row counts, and the RANSAC plane fit over the kept rows' vertices as the kernel's tail (tri_height / tri_flags optional)
    const int32_t *tri_cnt;        // [F] rows of the frame (null: tri_off[f+1] - tri_off[f])
    const int32_t *keep;           // [like x] a feature takes part iff keep[i] >= 0 (null: all)
    const int32_t *dt_status;      // [F] non-zero: declined triangulation, frame skipped (null: none)
    const int32_t *id_triples;     // [F][H][3] survivor-numbered vertex ids replacing the draw (null: draw)
    const int64_t *frame_ids;      // [F] sample-sequence counter of the frame (null: frame_base + f)
    int32_t n_hyp, ransac_min_points;
    int32_t max_feat, max_tri;     // what the launch's LDS was sized from (both forms)
    double threshold, goal_fraction, absolute_reference;
    uint64_t seed; int64_t frame_base;
    double *raw_scale, *model;     // [F], [F][4]
    int32_t *best_ic, *used, *hyp_counts;
};

constexpr int kMaxHyp = 512;
constexpr int kRansacPPT = 8;           // points per thread per chunk (chunks of 4096 points)

constexpr int kFlatDevWaves = 16;   // the device-resident form holds 96 KB of LDS — one workgroup per CU —, so it brings its own occupancy: 16 wavefronts

// (the second bound, wavefronts per SIMD: the stage form has always been allocated 96 vector registers — room for five wavefronts
// per SIMD — but only because the allocator happened to end there: phase 1's four rows in flight sit at that edge, and moving
// their loop into mvosr_flat.hpp moved it to 98, room for four.  Stated, it holds.  16 wavefronts need 4 per SIMD to launch at all.)
template <bool DEV, int WAVES = kRsWaves>
__global__ __launch_bounds__(WAVES *kWave, WAVES == kRsWaves ? 5 : 4) void flat_selection_kernel(const FlatArgs a) {
    constexpr int BLK = WAVES * kWave;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int n_all = a.feat_cnt[f];
    const int64_t off = a.feat_off[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const bool skip = DEV && a.dt_status && a.dt_status[f] != 0;
    // more features or rows than the launch's LDS was sized for (the header's max_feat, the call's max_tri): refused, LDS untouched
    const bool oversize = n_all > a.max_feat || tn > a.max_tri;
    if (const int refused = flat_entry_status(n_all, tn, skip, oversize)) {
        if (tid == 0) {
            a.status[f] = refused;
            a.height_level[f] = nan(""); a.n_kept[f] = 0;
            if constexpr (DEV) {
                a.raw_scale[f] = nan(""); a.best_ic[f] = 0; a.used[f] = 0;
                for (int k = 0; k < 4; ++k) a.model[4 * f + k] = nan("");
            }
        }
        return;
    }
    const auto lds = flat_plan<uint32_t>(DEV, n_all, tn, a.n_hyp);   // (mvosr_rescale_plan.hpp: the layout, and what lives when)
    double *Hh = reinterpret_cast<double *>(smem + lds.heights);
    unsigned long long *U = reinterpret_cast<unsigned long long *>(Hh);   // (heights are >= 0: the bit patterns order like the values)
    unsigned long long *ext = reinterpret_cast<unsigned long long *>(smem + lds.ext);
    int *misc = reinterpret_cast<int *>(smem + lds.misc);
    double *X = reinterpret_cast<double *>(smem + lds.x);
    double *Y = reinterpret_cast<double *>(smem + lds.y);
    double *Z = reinterpret_cast<double *>(smem + lds.z);
    int *hist = reinterpret_cast<int *>(smem + lds.hist);
    uint8_t *Fl = reinterpret_cast<uint8_t *>(smem + lds.flags);
#ifdef MVOSR_FS_STAMPS
    unsigned long long st[10];
#define FS_STAMP(i) st[i] = __builtin_amdgcn_s_memtime()
#else
#define FS_STAMP(i) do {} while (0)
#endif
    FS_STAMP(0);
    flat_state_init(misc, ext);
    // (the first rows are in flight while the vertex planes stream in: mvosr_flat.hpp, flat_phase1)
    TriIds rows[kFlatRows];
    flat_load_rows<BLK>(a.tri + 3 * tb, tid, tn, rows);
    int n = n_all;                                               // features in LDS (the survivors)
    if (DEV && a.keep) {
        // ordered compaction at load (rescale.py:134-135: feature3d[valid_id])
        // (a lane's features — up to four: 4 096 per frame on sixteen wavefronts — with their keep flags in one batch of loads,
        // before the count: flag, wait, coordinates, wait, twice over, was a tenth of this kernel's time with nothing else on the CU)
        constexpr int kOwn = 4;
        if (n_all <= kOwn * BLK) {
            int s0, s1;
            ordered_segment(n_all, BLK, s0, s1);
            double ox[kOwn], oy[kOwn], oz[kOwn];
            unsigned okeep = 0u;
            int c = 0;
#pragma unroll
            for (int r = 0; r < kOwn; ++r) {
                const int i = s0 + r * kWave + lane;
                const int ic = min(i, n_all - 1);
                const bool k = i < s1 && a.keep[off + ic] >= 0;
                okeep |= k ? (1u << r) : 0u;
                ox[r] = a.x[off + ic]; oy[r] = a.y[off + ic]; oz[r] = a.z[off + ic];
            }
#pragma unroll
            for (int r = 0; r < kOwn; ++r) c += __popcll(__ballot((okeep >> r) & 1u));
            int base;
            ordered_prefix<WAVES>(misc + FM_CW, c, base, n);
#pragma unroll
            for (int r = 0; r < kOwn; ++r) {
                const bool k = (okeep >> r) & 1u;
                const int pos = ordered_rank(k, base);
                if (k) { X[pos] = ox[r]; Y[pos] = oy[r]; Z[pos] = oz[r]; }
            }
        } else n = flat_compact_survivors<WAVES>(n_all, a.keep + off, a.x + off, a.y + off, a.z + off, X, Y, Z, misc + FM_CW);
    } else {
#pragma unroll 4
        for (int i = tid; i < n_all; i += BLK) { X[i] = a.x[off + i]; Y[i] = a.y[off + i]; Z[i] = a.z[off + i]; }
    }
    const double s_loose = flat_sin_deg(a.loose_deg), s_tight = flat_sin_deg(a.tight_deg);
    __syncthreads();
    FS_STAMP(1);
    // phase 1: every triangle's height and flags into LDS (and the height to the output), the loose ones counted and bounded
    {
        FlatLoose tally;
        flat_phase1<BLK>(a.tri + 3 * tb, rows, tn, X, Y, Z, n, a.loose_deg, a.tight_deg, s_loose, s_tight, Hh, Fl,
                         (!DEV || a.tri_height) ? a.tri_height + tb : nullptr, misc, tally);
        tally.commit(misc, ext);
    }
    __syncthreads();
    FS_STAMP(2);
    const int k = misc[FM_K];
    const double level = flat_level_search<WAVES>(U, Fl, tn, k, ext, misc, hist, a.height_factor).level;   // np.median, :91
    FS_STAMP(3);
    if constexpr (!DEV) {
        int kept = 0;
        #pragma unroll 4
        for (int t = tid; t < tn; t += BLK) {
            uint8_t fl = Fl[t];
            if ((fl & 2) && Hh[t] > level) { fl |= 4; ++kept; }                                 // :94-96
            a.tri_flags[tb + t] = fl;
        }
        kept = wave_sum(kept);
        if (lane == 0 && kept) atomicAdd(&misc[FM_KEPT], kept);
        __syncthreads();
        if (tid == 0) {
            a.height_level[f] = level;
            a.n_kept[f] = misc[FM_KEPT];
            a.status[f] = misc[FM_BADID] ? MVOSR_ST_ERR_MASK : (misc[FM_SINGULAR] ? MVOSR_ST_ERR_SINGULAR : 0);
        }
#ifdef MVOSR_FS_STAMPS
        FS_STAMP(4);                                                 // (diagnostic build: the stamps overwrite the frame's first heights)
        if (tid == 0 && tn >= 5) for (int i = 0; i < 5; ++i) a.tri_height[tb + i] = (double)(st[i] - st[0]);
#endif
    } else {
        // ---- the kept rows (:94-96), wavefront by wavefront over contiguous row segments so that the point list —
        // triangle_ids[valid_id].reshape(-1), :101 — comes out in row order without a sort
        int s0, s1;
        ordered_segment(tn, BLK, s0, s1);
        int c = 0;
        for (int t0 = s0; t0 < s1; t0 += kWave) {
            const int t = t0 + lane;
            bool kp = false;
            if (t < s1) {
                uint8_t fl = Fl[t];
                kp = (fl & 2) && Hh[t] > level;
                if (kp) { fl |= 4; Fl[t] = fl; }
                if (a.tri_flags) a.tri_flags[tb + t] = fl;
            }
            c += __popcll(__ballot(kp));
        }
        int base, K;
        ordered_prefix<WAVES>(misc + FM_CW, c, base, K);         // (its barrier: every height has been compared, their room is the list's now)
        const int M = 3 * K;                                     // len(point_selected), :140
        uint16_t *L = reinterpret_cast<uint16_t *>(smem + lds.list);   // the point list as vertex ids
        const int H = a.n_hyp;
        double2 *mods = reinterpret_cast<double2 *>(smem + lds.mods);  // [H][2] unit (n, d) as (nx, ny), (nz, d)
        int *cnts = reinterpret_cast<int *>(smem + lds.cnts);          // [H] inlier counts
        const bool bad = misc[FM_BADID] || misc[FM_SINGULAR];
        const bool fit = !bad && M >= a.ransac_min_points;       // :152
        if (fit) {
            for (int t0 = s0; t0 < s1; t0 += kWave) {
                const int t = t0 + lane;
                const bool kp = t < s1 && (Fl[t] & 4);
                const int pos = 3 * ordered_rank(kp, base);
                if (kp) {
                    const TriIds q = load_tri(a.tri + 3 * tb, t);
                    L[pos] = (uint16_t)q.a; L[pos + 1] = (uint16_t)q.b; L[pos + 2] = (uint16_t)q.c;
                }
            }
            __syncthreads();
            FS_STAMP(4);
            // the hypotheses' planes, one thread each (ransac.py:10-11, estimate_road_norm.py:13-15)
            const uint64_t key = ransac_frame_key(a.seed, (uint64_t)(a.frame_ids ? a.frame_ids[f] : a.frame_base + f));
            flat_build_hypotheses<BLK>(key, a.id_triples ? a.id_triples + (int64_t)f * H * 3 : nullptr, H, n, M, L, X, Y, Z, mods, cnts);
            __syncthreads();
            // Inlier counts (estimate_road_norm.py:17-18 over every list entry, repeats included).  The list names each of its
            // ~600 distinct vertices five or six times (once per kept triangle): a vertex is tested ONCE per hypothesis and
            // counts with its multiplicity.  Multiplicities by LDS atomics into 16-bit halves (the histogram's room is free by
            // now), the distinct vertices as (id | multiplicity << 16) behind the list, then one wavefront per hypothesis: ten
            // trips over the vertices, an integer sum per lane, one reduction.  (3 300 list entries against 100 hypotheses
            // with ballots and popcounts — the points in registers — was two thirds of this kernel's instructions; the first
            // attempt at the multiplicities kept the ballots, bit-sliced, and was slower than the list.)
            FS_STAMP(5);
            uint32_t *W2 = reinterpret_cast<uint32_t *>(smem + lds.w2);          // [n / 2 + 1] two 16-bit counts per word
            uint16_t *Dv = L + ((M + 1) & ~1);                                   // the distinct vertices, behind the list
            // (the list and the vertices share the heights' room: 6 bytes per KEPT row + 2 per vertex — they fit unless
            // nearly every row is kept in a frame of a few points; then the list itself is counted, entry by entry)
            const bool dedup = 2 * ((M + 1) & ~1) + 2 * n <= (int)lds.heights_bytes && n <= 2 * kFlatBins - 2;
            int n_items = M;
            if (dedup) {
                for (int v = tid; v < (n + 1) / 2 + 1; v += BLK) W2[v] = 0u;
                if (tid == 0) misc[FM_ND] = 0;
                __syncthreads();
                for (int j = tid; j < M; j += BLK) { const uint32_t id = L[j]; atomicAdd(&W2[id >> 1], 1u << (16u * (id & 1u))); }
                __syncthreads();
                for (int v = tid; v < n; v += BLK)
                    if ((W2[v >> 1] >> (16u * ((uint32_t)v & 1u))) & 0xFFFFu) Dv[atomicAdd(&misc[FM_ND], 1)] = (uint16_t)v;
                __syncthreads();
                n_items = misc[FM_ND];
            }
            // ... and, where they fit the heights' room (28 bytes per distinct vertex: they do unless more than ~1 000 of a frame's
            // vertices lie on kept rows), the vertices' coordinates and multiplicities side by side, in the order of the list of
            // distinct vertices: the counting loop then reads four contiguous arrays instead of gathering by id
            const bool packed = dedup && n_items <= 2 * BLK && 28 * n_items + 8 <= (int)lds.heights_bytes;
            double *PX = reinterpret_cast<double *>(smem + lds.packed), *PY = PX + n_items, *PZ = PY + n_items;
            int *PW = reinterpret_cast<int *>(PZ + n_items);
            if (packed) {
                double gx[2], gy[2], gz[2];
                int gw[2];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int j = tid + r * BLK;
                    const uint32_t id = Dv[min(j, n_items - 1)];
                    gx[r] = X[id]; gy[r] = Y[id]; gz[r] = Z[id]; gw[r] = (int)((W2[id >> 1] >> (16u * (id & 1u))) & 0xFFFFu);
                }
                __syncthreads();                                                 // (the list and the ids have been read: their room is the arrays')
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int j = tid + r * BLK;
                    if (j < n_items) { PX[j] = gx[r]; PY[j] = gy[r]; PZ[j] = gz[r]; PW[j] = gw[r]; }
                }
                __syncthreads();
            }
            FS_STAMP(6);
            const uint16_t *items = dedup ? Dv : L;
            // (mvosr_ransac.hpp: a wavefront's hypotheses seven at a time — all of them, with 100 hypotheses on 16 wavefronts)
            ransac_count_weighted<WAVES>(mods, cnts, H, n_items, a.threshold, packed,
                [&](int j, double &px, double &py, double &pz, int &wgt) { px = PX[j]; py = PY[j]; pz = PZ[j]; wgt = PW[j]; },
                [&](int j, double &px, double &py, double &pz, int &wgt) {
                    const uint32_t id = items[j];
                    wgt = dedup ? (int)((W2[id >> 1] >> (16u * (id & 1u))) & 0xFFFFu) : 1;
                    px = X[id]; py = Y[id]; pz = Z[id];
                });
            __syncthreads();
            FS_STAMP(7);
            if (a.hyp_counts) for (int h = tid; h < H; h += BLK) a.hyp_counts[(int64_t)f * H + h] = cnts[h];
        }
        if (wave == 0) {
            const int status = misc[FM_BADID] ? MVOSR_ST_ERR_MASK : (misc[FM_SINGULAR] ? MVOSR_ST_ERR_SINGULAR : (fit ? 0 : MVOSR_ST_RS_FEW));
            const FlatRansacResult r = flat_ransac_result(fit, status, mods, cnts, H, (double)M * a.goal_fraction, a.absolute_reference);
            if (lane == 0) {
                a.height_level[f] = level;
                a.n_kept[f] = K;
                a.status[f] = r.status;
                a.raw_scale[f] = r.raw;
                a.best_ic[f] = r.best_ic; a.used[f] = r.used;
                for (int kk = 0; kk < 4; ++kk) a.model[4 * f + kk] = r.m[kk];
            }
#ifdef MVOSR_FS_STAMPS
            // diagnostic build: the results are overwritten by the phase durations (profiles/stamps_flat_dev.py)
            FS_STAMP(8);
            if (fit && lane == 0) {
                a.model[4 * f] = (double)(st[1] - st[0]); a.model[4 * f + 1] = (double)(st[2] - st[1]); a.model[4 * f + 2] = (double)(st[3] - st[2]);
                a.model[4 * f + 3] = (double)(st[4] - st[3]); a.raw_scale[f] = (double)(st[5] - st[4]); a.height_level[f] = (double)(st[6] - st[5]);
                a.best_ic[f] = (int)(st[7] - st[6]); a.used[f] = (int)(st[8] - st[7]);
            }
#endif
        }
    }
}

// ---------------------------------------------------------------------------------------------
// RANSAC plane fit with the sample triples given (ransac.py:3-23).  One workgroup per frame; every
// hypothesis is the plane through its three sample points as the unit 4-vector (n, d)/|(n, d)| — the
// null vector the reference gets from the SVD of [x y z 1] (estimate_road_norm.py:13-15), up to sign
// — and |m.[p,1]| < threshold is counted over the frame's points (estimate_road_norm.py:17-18), the
// points held in registers, the hypotheses streamed from LDS.  Wavefront 0 then replays the reference's sequential
// rule: a hypothesis replaces the best when its count is strictly larger, and the loop stops at
// the first such improvement that exceeds the goal.
// ---------------------------------------------------------------------------------------------
struct RansacArgs {
    int64_t n_frames;
    const int64_t *pts_off; const int32_t *pts_cnt;     // [F]
    const double *px, *py, *pz;                          // planes of the selected points (with repeats, :101)
    const int32_t *triples;                              // [F][H][3] row indices into the frame's points
    int32_t n_hyp;                                       // H (<= kMaxHyp)
    double threshold, goal_fraction;
    int32_t *counts;                                     // [F][H] inlier counts (or NULL)
    double *model;                                       // [F][4] best model, sign fixed so that n_y >= 0
    int32_t *best_ic, *used;                             // [F]
    int32_t line;                                        // 1: 2-D line fit (estimate_line / is_inlier_line, estimate_road_norm.py:39-49):
                                                         // samples are PAIRS (still 3 ints apart), pz is not read, model = (a, b, 0, c)
};
__global__ __launch_bounds__(kRsBlock) void ransac_plane_kernel(const RansacArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int M = a.pts_cnt[f];
    const int64_t off = a.pts_off[f];
    const int H = a.n_hyp;
    const int tid = threadIdx.x, lane = lane_id();
    const auto lds = ransac_plan<uint32_t>(H);
    double4 *mods = reinterpret_cast<double4 *>(smem + lds.mods);         // [H] unit (n, d)
    int *cnts = reinterpret_cast<int *>(smem + lds.cnts);                 // [H] inlier counts
    if (M <= 0) {
        if (a.counts) for (int h = tid; h < H; h += kRsBlock) a.counts[(int64_t)f * H + h] = 0;     // no points: no inliers
        if (tid == 0) { a.best_ic[f] = 0; a.used[f] = 0; for (int k = 0; k < 4; ++k) a.model[4 * f + k] = nan(""); }
        return;
    }
    const double *px = a.px + off, *py = a.py + off, *pz = a.pz + off;
    // the hypotheses' planes, one thread each
    for (int h = tid; h < H; h += kRsBlock) {
        const int32_t *t = a.triples + ((int64_t)f * H + h) * 3;
        const int i0 = t[0], i1 = t[1], i2 = a.line ? 0 : t[2];
        // a sample that names a row outside [0, M) is spent like one that names a row twice: NaN model, no inliers, nothing read
        if (!ids_in_range(i0, i1, i2, M)) {
            double4 m; m.x = m.y = m.z = m.w = nan("");
            mods[h] = m;
            cnts[h] = 0;
            continue;
        }
        mods[h] = a.line ? ransac_unit_line(px, py, i0, i1) : ransac_unit_plane(px, py, pz, i0, i1, i2);
        cnts[h] = 0;
    }
    __syncthreads();
    // the points in registers (read from HBM once, coalesced), the hypotheses streamed past them (mvosr_ransac.hpp)
    ransac_count_resident<false, kRansacPPT, 4, kRsBlock>(M, mods, cnts, H, a.threshold,
        [&](int j, double &x, double &y, double &z) { x = px[j]; y = py[j]; z = a.line ? 0.0 : pz[j]; });
    __syncthreads();
    if (a.counts) for (int h = tid; h < H; h += kRsBlock) a.counts[(int64_t)f * H + h] = cnts[h];
    if (wave_id() == 0) {
        RansacReplay rp = {-1, 0, H, 0};
        ransac_replay(rp, cnts, 0, H, (double)M * a.goal_fraction);       // ransac.py:9-22; the goal: estimate_road_norm.py:68
        if (lane == 0) {
            a.best_ic[f] = rp.best_ic; a.used[f] = rp.used;
            double4 bm; bm.x = bm.y = bm.z = bm.w = nan("");
            if (rp.best >= 0) bm = ransac_sign_rule(mods[rp.best]);       // rescale.py:159-161
            a.model[4 * f] = bm.x; a.model[4 * f + 1] = bm.y; a.model[4 * f + 2] = bm.z; a.model[4 * f + 3] = bm.w;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Legacy per-triangle batch, /root/reference/src/triangle_batch.py:14-68: features
// are [u, v, depth]; every Delaunay triangle is back-projected (:32-33), n = A^-1 . 1 (:36-37),
// s = n_y/|n| (:43), h = mean y (:40); triangles with s > 0.98 and h > 0 (:54-55) give mean and std
// (:57-58), values outside mean +- 3 std are clipped (:60-61) and the mean of the rest is the camera
// height (:62).  Three sweeps over the triangles (sum / squared deviations / clipped sum), each
// thread visiting its triangles in a fixed order, so the result is run-to-run identical.
// ---------------------------------------------------------------------------------------------
struct TriBatchArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *u, *v, *depth;
    const int64_t *tri_off; const int32_t *tri;
    double focus, cx, cy, s_min, n_sigma;
    int32_t max_feat;              // what the launch's LDS was sized from
    double *height;                // [F]
    int32_t *counts;               // [F][2]: kept, kept after the clip
    int32_t *status;               // [F]
};

__global__ __launch_bounds__(kRsBlock) void triangle_batch_kernel(const TriBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int n = a.feat_cnt[f];
    const int64_t off = a.feat_off[f];
    const int64_t tb = a.tri_off[f];
    const int tn = (int)(a.tri_off[f + 1] - tb);
    const int tid = threadIdx.x;
    if (n <= 0 || tn <= 0) {
        if (tid == 0) { a.status[f] = MVOSR_ST_ERR_EMPTY; a.height[f] = nan(""); a.counts[2 * f] = a.counts[2 * f + 1] = 0; }
        return;
    }
    if (n > a.max_feat) {                                       // more features than the LDS has room for: refused, LDS untouched
        if (tid == 0) { a.status[f] = MVOSR_ST_ERR_MASK; a.height[f] = nan(""); a.counts[2 * f] = a.counts[2 * f + 1] = 0; }
        return;
    }
    const auto lds = tribatch_plan<uint32_t>(n);
    double *X = reinterpret_cast<double *>(smem + lds.x);
    double *Y = reinterpret_cast<double *>(smem + lds.y);
    double *Z = reinterpret_cast<double *>(smem + lds.z);
    double *red = reinterpret_cast<double *>(smem + lds.red);   // 3 slots x 2*kRsWaves doubles
    int *flag = reinterpret_cast<int *>(smem + lds.flag);
    if (tid == 0) { flag[0] = 0; flag[1] = 0; }
    for (int i = tid; i < n; i += kRsBlock) {
        const double d = a.depth[off + i];
        X[i] = d * (a.u[off + i] - a.cx) / a.focus;                                  // :32
        Y[i] = d * (a.v[off + i] - a.cy) / a.focus;                                  // :33
        Z[i] = d;
    }
    __syncthreads();
    // height of triangle t if it is kept, NaN otherwise
    auto kept_height = [&](int t) -> double {
        const TriIds q = load_tri(a.tri + 3 * tb, t);
        if (!ids_in_range(q.a, q.b, q.c, n)) { flag[1] = 1; return nan(""); }
        double nx, ny, nz;
        if (!plane_normal(X[q.a], Y[q.a], Z[q.a], X[q.b], Y[q.b], Z[q.b], X[q.c], Y[q.c], Z[q.c], nx, ny, nz)) flag[0] = 1;   // :36
        const double s = ny / sqrt((nx * nx + ny * ny) + nz * nz);                   // :38-39,:43
        const double h = div3((Y[q.a] + Y[q.b]) + Y[q.c]);                           // :40
        return (s > a.s_min && h > 0.0) ? h : nan("");                               // :54-55
    };
    // the three sweeps need every kept height three times: a thread's first kTbKeep triangles keep theirs
    // in registers (all of them for frames of up to 4096 triangles), the rest are recomputed
    constexpr int kTbKeep = 8;
    double hk[kTbKeep];
    double sum = 0.0, cnt = 0.0;
#pragma unroll
    for (int k = 0; k < kTbKeep; ++k) {
        const int t = tid + k * kRsBlock;
        hk[k] = (t < tn) ? kept_height(t) : nan("");
        if (hk[k] == hk[k]) { sum += hk[k]; cnt += 1.0; }
    }
    for (int t = tid + kTbKeep * kRsBlock; t < tn; t += kRsBlock) { const double h = kept_height(t); if (h == h) { sum += h; cnt += 1.0; } }
    block_sum2<kRsWaves>(sum, cnt, red);
    const double mean = sum / cnt;                                                   // :57
    double ss = 0.0, dummy = 0.0;
#pragma unroll
    for (int k = 0; k < kTbKeep; ++k) if (hk[k] == hk[k]) { const double d = hk[k] - mean; ss += d * d; }
    for (int t = tid + kTbKeep * kRsBlock; t < tn; t += kRsBlock) { const double h = kept_height(t); if (h == h) { const double d = h - mean; ss += d * d; } }
    block_sum2<kRsWaves>(ss, dummy, red + 2 * kRsWaves);
    const double sd = sqrt(ss / cnt);                                                // :58
    const double lo = mean - a.n_sigma * sd, hi = mean + a.n_sigma * sd;             // :60-61
    double sum2 = 0.0, cnt2 = 0.0;
#pragma unroll
    for (int k = 0; k < kTbKeep; ++k) if (hk[k] == hk[k] && hk[k] > lo && hk[k] < hi) { sum2 += hk[k]; cnt2 += 1.0; }
    for (int t = tid + kTbKeep * kRsBlock; t < tn; t += kRsBlock) { const double h = kept_height(t); if (h == h && h > lo && h < hi) { sum2 += h; cnt2 += 1.0; } }
    block_sum2<kRsWaves>(sum2, cnt2, red + 4 * kRsWaves);
    __syncthreads();
    if (tid == 0) {
        a.height[f] = sum2 / cnt2;                                                   // :62
        a.counts[2 * f] = (int)cnt; a.counts[2 * f + 1] = (int)cnt2;
        a.status[f] = flag[1] ? MVOSR_ST_ERR_MASK : (flag[0] ? MVOSR_ST_ERR_SINGULAR : 0);
    }
}

// The slew limiter of scale_calculation_ransac (/root/reference/src/rescale.py:169-177) over a run of frames: a sequential
// recurrence of rounded additions, walked by ONE wavefront — 64 frames are loaded at a time, their values broadcast lane by
// lane (v_readlane), the running scale identical in every lane; lane j keeps the value pushed at its frame.
template <int J>
__device__ __forceinline__ void slew_step(double r, unsigned long long am, double slew, int lane, double &s, double &out) {
    if constexpr (J < kWave) {
        // branch-free: the three candidates depend on s alone, the selects on one subtraction (the recurrence's only chain)
        const double rj = readlane_d(r, J);                                  // (constant lane: no M0 set-up)
        const double d = rj - s;
        const double up = s + slew, dn = s - slew;
        const double moved = d > slew ? up : (d < -slew ? dn : rj);          // rescale.py:169-174
        s = ((am >> J) & 1ull) ? moved : s;                                  // :152 — only a frame with a RANSAC plane moves the scale
        out = lane == J ? s : out;                                           // :175 scale_queue.append(self.scale)
        slew_step<J + 1>(r, am, slew, lane, s, out);
    }
}

__global__ __launch_bounds__(kWave) void slew_kernel(const double *raw, const int32_t *apply, int64_t n, double slew, double s_in,
                                                     double *pushed) {
    const int lane = lane_id();
    double s = s_in;
    double r = lane < n ? raw[lane] : 0.0;
    int ap = lane < n ? apply[lane] : 0;
    for (int64_t i0 = 0; i0 < n; i0 += kWave) {
        const int64_t i = i0 + lane;
        const double r_cur = r;
        const unsigned long long am = __ballot(ap != 0);                     // (lanes beyond n: no plane, the scale stays)
        if (i + kWave < n) { r = raw[i + kWave]; ap = apply[i + kWave]; } else ap = 0;   // the next 64 frames load under this block's chain
        double out = 0.0;
        slew_step<0>(r_cur, am, slew, lane, s, out);
        if (i < n) pushed[i] = out;
    }
}

// get_inliers, /root/reference/src/estimate_road_norm.py:71-78: |n.p + d| < threshold per point
__global__ __launch_bounds__(256) void plane_inliers_kernel(int64_t n, const double *px, const double *py, const double *pz,
                                                            double m0, double m1, double m2, double m3, double threshold,
                                                            uint8_t *mask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mask[i] = fabs(((px[i] * m0 + py[i] * m1) + pz[i] * m2) + m3) < threshold;
}

// ---------------------------------------------------------------------------------------------
// GraphGrow.process, /root/reference/src/graph.py:85-107, with its random loop made deterministic (include/mvosr.h,
// mvosr_region_grow_batch): rows that share an edge (graph.py:47-72) are joined when their pitch differs by less than
// threshold_angle and their inverse height by less than height_factor * median(1/heights) (graph.py:73-77,93); `expend`
// (graph.py:79-83) compares a row with the row it came from, so a proposal is the connected component of its seed in that
// symmetric graph; the result is the largest component that holds a flat seed (graph.py:90-92,97-103), the one with the
// smallest row index among equally large ones.
//
// One frame per workgroup, five phases:
//   1  per row 1/height and pitch into LDS — given (PTS = false), or from the frame's points by flat_selection_kernel's
//      row_height_pitch (PTS = true: the vertex planes are staged in the work area) —, the rows checked (ids, repeated vertices);
//   2  the two medians (graph.py:91,93) by an 8-bit radix select on the bit patterns (1/height > 0: they order like the values);
//   3  the rows as 16-bit ids and a vertex -> incident rows table (counts, block scan, fill) in the work area;
//   4  per row and edge the row across it: the incident rows of the edge's lower-degree end that name the other end — two or
//      more is an edge on more than two rows: refused —, and the join test made at once: three 16-bit joined neighbours per row;
//   5  labels (smallest row index of the component) by hooking on the label's root and full pointer jumping, repeated until a
//      round changes nothing — no iteration cap: a strip of T rows has diameter T —; sizes and seed flags at the roots.
// LDS: grow_plan() (mvosr_rescale_plan.hpp), carved at the header's sizes; 3 980 rows of 2 000 points: 144 KB.
// ---------------------------------------------------------------------------------------------
struct GrowArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *x, *y, *z;                 // read by the from-points form only
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    const double *h_in, *ang_in;             // [rows] the given form's heights and pitch (deg)
    double threshold_angle, seed_deg, level_deg, height_factor;
    int32_t max_feat, max_tri;               // what the launch's LDS was sized from
    uint8_t *region;                         // [rows]
    int32_t *n_region, *n_flat, *status;     // [F]
    double *level, *threshold_height;        // [F]
    int32_t *label, *neighbors;              // optional [rows], [rows][3]
    double *tri_height, *tri_angle;          // optional [rows], from-points form
};

constexpr uint16_t kGrowNone = 0xFFFFu;      // "no joined neighbour": rows are numbered below it (the LDS holds a few thousand)

// np.median of the k rows' 1/height that lie in the subset (SUB: pitch < level_deg; else every row): the lower middle order
// statistic by eight passes of an 8-bit radix select from the top byte down, the upper one by next_order_statistic.
// `slot` (0 / 1): the call's own pre-set scalars (misc[GM_LE + slot] = 0, ext[slot] = ~0).  Every thread returns the same value.
template <bool SUB>
__device__ double grow_median(const unsigned long long *U, const double *Ang, double level_deg, int tn, int k, int *hist, int *misc,
                              unsigned long long *ext, int slot) {
    if (k <= 0) return nan("");                                  // np.median of an empty array
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const int klo = (k - 1) >> 1, khi = k >> 1;
    unsigned long long prefix = 0ull;
    int rank = klo;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < kGrowBins) hist[tid] = 0;
        __syncthreads();
        for (int t = tid; t < tn; t += kRsBlock) {
            if (SUB && !(Ang[t] < level_deg)) continue;
            const unsigned long long u = U[t];
            if (shift == 56 || (u >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(int)((u >> shift) & 255ull)], 1);
        }
        __syncthreads();
        if (wave == 0) {                                         // four bins per lane, wave scan: the bin whose cumulative count passes the rank
            const int b0 = hist[4 * lane], b1 = hist[4 * lane + 1], b2 = hist[4 * lane + 2], b3 = hist[4 * lane + 3];
            const int mine = (b0 + b1) + (b2 + b3);
            const int incl = wave_scan_incl(mine);
            const int excl = incl - mine;
            if (rank >= excl && rank < incl) {                   // exactly one lane
                int r = rank - excl, bin = 4 * lane;
                if (r >= b0) { r -= b0; ++bin; if (r >= b1) { r -= b1; ++bin; if (r >= b2) { r -= b2; ++bin; } } }
                misc[GM_BIN] = bin; misc[GM_RANK] = r;
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)misc[GM_BIN] << shift;
        rank = misc[GM_RANK];
    }
    const double vlo = __longlong_as_double((long long)prefix);
    if (khi == klo) return vlo;
    int le = 0;
    unsigned long long above = ~0ull;
    for (int t = tid; t < tn; t += kRsBlock) {
        if (SUB && !(Ang[t] < level_deg)) continue;
        const unsigned long long u = U[t];
        if (u <= prefix) ++le; else above = u < above ? u : above;
    }
    const double vhi = __longlong_as_double((long long)next_order_statistic(le, above, prefix, khi, &misc[GM_LE + slot], &ext[slot]));
    return (vlo + vhi) / 2.0;
}

template <bool PTS>
__global__ __launch_bounds__(kRsBlock) void region_grow_kernel(const GrowArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int n_all = a.feat_cnt[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    if (tn <= 0 || n_all > a.max_feat || tn > a.max_tri) {
        // no rows; or more features or rows than the launch's LDS was sized for: refused, LDS untouched, no per-row output written
        if (tid == 0) {
            a.status[f] = tn <= 0 ? MVOSR_ST_ERR_EMPTY : MVOSR_ST_ERR_MASK;
            a.level[f] = nan(""); a.threshold_height[f] = nan(""); a.n_region[f] = 0; a.n_flat[f] = 0;
        }
        return;
    }
    const int n = max(n_all, 0);
    const int64_t off = a.feat_off[f];
    const uint32_t T = (uint32_t)a.max_tri;
    const auto lds = grow_plan<uint32_t>(PTS, a.max_feat, a.max_tri);      // (mvosr_rescale_plan.hpp: the layout, and what lives when)
    double *Hi = reinterpret_cast<double *>(smem + lds.hinv);                   // 1/height by row
    const unsigned long long *U = reinterpret_cast<const unsigned long long *>(Hi);
    double *Ang = reinterpret_cast<double *>(smem + lds.ang);                   // pitch by row
    unsigned long long *ext = reinterpret_cast<unsigned long long *>(smem + lds.ext);   // [0], [1] the medians' "smallest above", [2] the best root's key
    int *misc = reinterpret_cast<int *>(smem + lds.misc);
    int *hist = reinterpret_cast<int *>(smem + lds.hist);
    uint16_t *NB = reinterpret_cast<uint16_t *>(smem + lds.nb);                 // [T][3] joined neighbours
    double *X = reinterpret_cast<double *>(smem + lds.x), *Y = reinterpret_cast<double *>(smem + lds.y), *Z = reinterpret_cast<double *>(smem + lds.z);   // (PTS, phase 1)
    const int32_t *rows = a.tri + 3 * tb;
    if (tid < GM_N) misc[tid] = 0;
    if (tid < 3) ext[tid] = tid < 2 ? ~0ull : 0ull;
    // a frame refused for what its rows or heights say: all-zero region, nothing else
    auto refuse = [&](int status) {
        for (int t = tid; t < tn; t += kRsBlock) {
            a.region[tb + t] = 0;
            if (a.label) a.label[tb + t] = -1;
            if (a.neighbors) { int32_t *nb = a.neighbors + 3 * (tb + t); nb[0] = -1; nb[1] = -1; nb[2] = -1; }
        }
        if (tid == 0) { a.status[f] = status; a.level[f] = nan(""); a.threshold_height[f] = nan(""); a.n_region[f] = 0; a.n_flat[f] = 0; }
    };
    // ---- phase 1: 1/height and pitch of every row, the rows checked
    if constexpr (PTS) {
        for (int i = tid; i < n; i += kRsBlock) { X[i] = a.x[off + i]; Y[i] = a.y[off + i]; Z[i] = a.z[off + i]; }
    }
    __syncthreads();
    {
        int bad = 0, singular = 0, k_level = 0;
        for (int t = tid; t < tn; t += kRsBlock) {
            const TriIds q = load_tri(rows, t);
            const bool in_range = ids_in_range(q.a, q.b, q.c, n);
            if (!in_range || q.a == q.b || q.a == q.c || q.b == q.c) bad = 1;
            double h, ang;
            if constexpr (PTS) {
                h = nan(""); ang = nan("");
                if (in_range) {
                    double mu;
                    if (!row_height_pitch(X, Y, Z, q, mu, h)) singular = 1;
                    ang = asin(mu) * 180.0 / 3.141592653589793;                            // rescale.py:83
                }
                if (a.tri_height) a.tri_height[tb + t] = h;
                if (a.tri_angle) a.tri_angle[tb + t] = ang;
            } else {
                h = a.h_in[tb + t]; ang = a.ang_in[tb + t];
                if (!(h > 0.0) || h == __longlong_as_double(0x7FF0000000000000ll)) bad = 1;   // non-finite or non-positive: 1/h would not order by its bits
            }
            const double hinv = 1.0 / h;                                                   // graph.py:88
            if (PTS && !(hinv > 0.0)) singular = 1;                                       // (a NaN normal behind non-zero pivots: no height either)
            Hi[t] = hinv; Ang[t] = ang;
            k_level += (ang < a.level_deg) ? 1 : 0;                                        // graph.py:91
        }
        if (bad) misc[GM_BAD] = 1;
        if (singular) misc[GM_SINGULAR] = 1;
        k_level = wave_sum(k_level);
        if (lane == 0 && k_level) atomicAdd(&misc[GM_KLEVEL], k_level);
    }
    __syncthreads();
    if (misc[GM_BAD]) { refuse(MVOSR_ST_ERR_MASK); return; }
    if (PTS && misc[GM_SINGULAR]) { refuse(MVOSR_ST_ERR_SINGULAR); return; }
    // ---- phase 2: the medians (the vertex planes are dead)
    const double level = grow_median<true>(U, Ang, a.level_deg, tn, misc[GM_KLEVEL], hist, misc, ext, 0);   // graph.py:91
    const double thr_h = a.height_factor * grow_median<false>(U, Ang, a.level_deg, tn, tn, hist, misc, ext, 1);   // :93
    // ---- phase 3: the rows in 16 bits, and per vertex its incident rows
    uint16_t *R16 = reinterpret_cast<uint16_t *>(smem + lds.r16);               // [T][3]
    uint16_t *It = reinterpret_cast<uint16_t *>(smem + lds.inc);                // [3 T] incident rows, vertex by vertex
    int *St = reinterpret_cast<int *>(smem + lds.start);                        // [n + 1] where a vertex's rows start ([n]: 3 tn)
    for (int v = tid; v <= n; v += kRsBlock) St[v] = 0;
    __syncthreads();
    for (int t = tid; t < tn; t += kRsBlock) {
        const TriIds q = load_tri(rows, t);
        R16[3 * t] = (uint16_t)q.a; R16[3 * t + 1] = (uint16_t)q.b; R16[3 * t + 2] = (uint16_t)q.c;
        atomicAdd(&St[q.a], 1); atomicAdd(&St[q.b], 1); atomicAdd(&St[q.c], 1);
    }
    __syncthreads();
    {   // inclusive scan of the counts: a contiguous chunk per thread, wave scan, wave totals through LDS
        const int cnt = n + 1, chunk = (cnt + kRsBlock - 1) / kRsBlock;
        const int i0 = tid * chunk, i1 = min(cnt, i0 + chunk);
        int s = 0;
        for (int i = i0; i < i1; ++i) s += St[i];
        const int incl = wave_scan_incl(s);
        if (lane == kWave - 1) misc[GM_WSUM + wave] = incl;
        __syncthreads();
        int run = incl - s;
#pragma unroll
        for (int w = 0; w < kRsWaves; ++w) if (w < wave) run += misc[GM_WSUM + w];
        for (int i = i0; i < i1; ++i) { run += St[i]; St[i] = run; }
    }
    __syncthreads();
    for (int t = tid; t < tn; t += kRsBlock) {
#pragma unroll
        for (int e = 0; e < 3; ++e) It[atomicSub(&St[R16[3 * t + e]], 1) - 1] = (uint16_t)t;   // (the ends count down to the starts)
    }
    __syncthreads();
    // ---- phase 4: the row across each edge (graph.py:55-68) and the join test (graph.py:73-77)
    {
        int bad = 0;
        for (int t = tid; t < tn; t += kRsBlock) {
            const int v[3] = {R16[3 * t], R16[3 * t + 1], R16[3 * t + 2]};
            const double ht = Hi[t], at = Ang[t];
#pragma unroll
            for (int e = 0; e < 3; ++e) {                                        // (a,b), (a,c), (b,c)
                int p = v[e == 2 ? 1 : 0], q = v[e == 0 ? 1 : 2];
                if (St[p + 1] - St[p] > St[q + 1] - St[q]) { const int s = p; p = q; q = s; }
                int found = 0, other = -1;
                for (int i = St[p], i1 = St[p + 1]; i < i1; ++i) {
                    const int r = It[i];
                    if (r == t) continue;
                    if (R16[3 * r] == q || R16[3 * r + 1] == q || R16[3 * r + 2] == q) { ++found; other = r; }
                }
                if (found > 1) bad = 1;                                          // an edge on more than two rows
                if (found != 1) other = -1;
                if (a.neighbors) a.neighbors[3 * (tb + t) + e] = other;
                bool joined = false;
                if (other >= 0) joined = fabs(at - Ang[other]) < a.threshold_angle && fabs(ht - Hi[other]) < thr_h;
                NB[3 * t + e] = joined ? (uint16_t)other : kGrowNone;
            }
        }
        if (bad) misc[GM_BAD] = 1;
    }
    __syncthreads();
    if (misc[GM_BAD]) { refuse(MVOSR_ST_ERR_MASK); return; }
    // ---- phase 5: labels.  A round: every row hooks its label's root (and itself) to the smallest label among its joined
    // neighbours, then every row jumps to its root; a round in which no row hooked ends the loop: labels are then equal
    // along every joined edge and are roots, and a label is a row of the component not above any of its rows.
    int *L = reinterpret_cast<int *>(smem + lds.label);                         // [T] (the table is dead)
    int *S = L + T;                                                             // [T] at a root: size, bit 30: holds a flat row
    volatile int *Lv = L;
    for (int t = tid; t < tn; t += kRsBlock) { L[t] = t; S[t] = 0; }
    __syncthreads();
    for (int it = 0;; ++it) {
        if (tid == 0) misc[GM_CHANGED + (it + 1) % 3] = 0;                       // (read last two rounds ago)
        int changed = 0;
        for (int t = tid; t < tn; t += kRsBlock) {
            const int l = Lv[t];
            int m = l;
#pragma unroll
            for (int e = 0; e < 3; ++e) { const uint16_t r = NB[3 * t + e]; if (r != kGrowNone) m = min(m, Lv[r]); }
            if (m < l) { atomicMin(&L[l], m); atomicMin(&L[t], m); changed = 1; }
        }
        if (changed) misc[GM_CHANGED + it % 3] = 1;
        __syncthreads();
        for (int t = tid; t < tn; t += kRsBlock) {
            int l = Lv[t];
            for (;;) { const int up = Lv[l]; if (up == l) break; l = up; }       // (labels only decrease: the chain ends)
            Lv[t] = l;
        }
        __syncthreads();
        if (!misc[GM_CHANGED + it % 3]) break;
    }
    // ---- sizes and seeds at the roots, the largest seeded component (smallest root among equals)
    {
        int n_flat = 0;
        for (int t = tid; t < tn; t += kRsBlock) {
            const bool flat = Ang[t] < a.seed_deg && Hi[t] < level;              // graph.py:90-92
            const int l = L[t];
            atomicAdd(&S[l], 1);
            if (flat) { atomicOr(&S[l], 1 << 30); ++n_flat; }
        }
        n_flat = wave_sum(n_flat);
        if (lane == 0 && n_flat) atomicAdd(&misc[GM_NFLAT], n_flat);
    }
    __syncthreads();
    {
        unsigned long long best = 0ull;
        for (int t = tid; t < tn; t += kRsBlock) {
            const int s = S[t];
            if (L[t] == t && (s & (1 << 30))) {
                const unsigned long long key = ((unsigned long long)(s & ((1 << 30) - 1)) << 32) | (unsigned long long)(0x7FFFFFFF - t);
                best = key > best ? key : best;
            }
        }
        best = wave_max_u64(best);
        if (lane == 0 && best) atomicMax(&ext[2], best);
    }
    __syncthreads();
    const unsigned long long key = ext[2];
    const int root = key ? 0x7FFFFFFF - (int)(key & 0xFFFFFFFFull) : -1;         // nothing flat: graph.py:95-96
    for (int t = tid; t < tn; t += kRsBlock) {
        a.region[tb + t] = L[t] == root ? 1 : 0;
        if (a.label) a.label[tb + t] = L[t];
    }
    if (tid == 0) {
        a.status[f] = 0; a.level[f] = level; a.threshold_height[f] = thr_h;
        a.n_region[f] = (int)(key >> 32); a.n_flat[f] = misc[GM_NFLAT];
    }
}

// One launch of a frame-per-workgroup kernel on the context's device and stream, with `lds` bytes of dynamic LDS (its plan's
// total).  `lds` is checked against the context's limit and the kernel's own limit raised to it — except for a kernel whose plan
// stays below the 64 KB every kernel may have (raise_limit = false).
template <typename Args>
static int rs_launch(mvosr_ctx *ctx, void (*kernel)(Args), const char *name, int64_t n_frames, int block, size_t lds, const Args &a,
                     bool raise_limit = true) {
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    if (raise_limit) {
        if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
            return set_error(MVOSR_ERR_TOO_LARGE, "frame needs %zu B of LDS (> %d) in the rescale-variant kernels", lds, ctx->max_lds_per_block);
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_frames), dim3((unsigned)block), lds, ctx_stream(ctx), a);
    return check_launch(name);
}

}  // namespace mvosr

using namespace mvosr;

extern "C" {

static int launch_graph(mvosr_ctx *ctx, const mvosr_batch *b, GraphArgs &a, bool keep) {
    if (!b->feat_off || !b->feat_cnt || !b->z || !b->v || !b->tri1_off || !b->tri1) return set_error(MVOSR_ERR_ARG, "graph_inliers: missing z/v/tri1");
    if (b->n_frames <= 0) return MVOSR_OK;
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.z = b->z; a.v = b->v;
    a.tri_off = b->tri1_off; a.tri = b->tri1; a.tri_cnt = b->tri1_cnt; a.max_feat = b->max_feat;
    return rs_launch(ctx, keep ? graph_inliers_kernel<true> : graph_inliers_kernel<false>, "graph_inliers_kernel", b->n_frames, kRsBlock,
                     graph_plan<size_t>(b->max_feat).total, a);
}

int mvosr_graph_inliers_batch(mvosr_ctx *ctx, const mvosr_batch *b, uint32_t good_bits, int32_t *total, int32_t *good,
                              int32_t *status) {
    if (!ctx || !b || !total || !good) return set_error(MVOSR_ERR_ARG, "graph_inliers: null argument");
    GraphArgs a = {};
    a.good_bits = good_bits; a.total = total; a.good = good; a.status = status;
    return launch_graph(ctx, b, a, false);
}

int mvosr_graph_keep_batch(mvosr_ctx *ctx, const mvosr_batch *b, uint32_t good_bits, int32_t min_valid, const int32_t *dt_status,
                           int32_t *keep, int32_t *n_valid, int32_t *status) {
    if (!ctx || !b || !keep) return set_error(MVOSR_ERR_ARG, "graph_keep: null argument");
    GraphArgs a = {};
    a.good_bits = good_bits; a.status = status; a.dt_status = dt_status; a.min_valid = min_valid; a.keep = keep; a.n_valid = n_valid;
    return launch_graph(ctx, b, a, true);
}

int mvosr_flat_selection_batch(mvosr_ctx *ctx, const mvosr_batch *b, double loose_deg, double tight_deg, double height_factor,
                               double *tri_height, uint8_t *tri_flags, double *height_level, int32_t *n_kept, int32_t *status,
                               int64_t max_tri) {
    if (!ctx || !b || !tri_height || !tri_flags || !height_level || !n_kept || !status) return set_error(MVOSR_ERR_ARG, "flat_selection: null argument");
    if (!b->feat_off || !b->feat_cnt || !b->x || !b->y || !b->z || !b->tri2_off || !b->tri2) return set_error(MVOSR_ERR_ARG, "flat_selection: missing x/y/z/tri2");
    if (b->n_frames <= 0) return MVOSR_OK;
    FlatArgs a = {};
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.x = b->x; a.y = b->y; a.z = b->z;
    a.tri_off = b->tri2_off; a.tri = b->tri2; a.tri_cnt = b->tri2_cnt; a.loose_deg = loose_deg; a.tight_deg = tight_deg; a.height_factor = height_factor;
    a.tri_height = tri_height; a.tri_flags = tri_flags; a.height_level = height_level; a.status = status; a.n_kept = n_kept;
    if (max_tri <= 0) max_tri = 2 * (int64_t)b->max_feat;
    if (max_tri > INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "flat_selection: max_tri does not fit 32 bits");
    a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri;
    return rs_launch(ctx, flat_selection_kernel<false>, "flat_selection_kernel", b->n_frames, kRsBlock,
                     flat_plan<size_t>(false, b->max_feat, max_tri, 0).total, a);
}

int mvosr_flat_ransac_batch(mvosr_ctx *ctx, const mvosr_batch *b, const int32_t *keep, const mvosr_rescale_params *rp,
                            const int32_t *id_triples, const int64_t *frame_ids, const int32_t *dt_status,
                            const mvosr_rescale_outputs *o, int64_t max_tri) {
    if (!ctx || !b || !rp || !o) return set_error(MVOSR_ERR_ARG, "flat_ransac: null argument");
    if (!o->raw_scale || !o->height_level || !o->model || !o->best_ic || !o->used || !o->n_kept || !o->status)
        return set_error(MVOSR_ERR_ARG, "flat_ransac: a required output is null");
    if (!b->feat_off || !b->feat_cnt || !b->x || !b->y || !b->z || !b->tri2_off || !b->tri2) return set_error(MVOSR_ERR_ARG, "flat_ransac: missing x/y/z/tri2");
    if (rp->n_hyp < 1 || rp->n_hyp > kMaxHyp) return set_error(MVOSR_ERR_ARG, "flat_ransac: n_hyp must be in 1..%d", kMaxHyp);
    if (rp->ransac_min_points < 3) return set_error(MVOSR_ERR_ARG, "flat_ransac: ransac_min_points < 3");
    if (b->max_feat > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "flat_ransac: vertex ids are 16-bit in the point list");
    if (b->n_frames <= 0) return MVOSR_OK;
    if (max_tri <= 0) max_tri = 2 * (int64_t)b->max_feat;
    FlatArgs a = {};
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.x = b->x; a.y = b->y; a.z = b->z;
    a.tri_off = b->tri2_off; a.tri = b->tri2; a.tri_cnt = b->tri2_cnt;
    a.loose_deg = rp->loose_deg; a.tight_deg = rp->tight_deg; a.height_factor = rp->height_factor;
    a.tri_height = o->tri_height; a.tri_flags = o->tri_flags; a.height_level = o->height_level; a.status = o->status; a.n_kept = o->n_kept;
    a.keep = keep; a.dt_status = dt_status; a.id_triples = id_triples; a.frame_ids = frame_ids;
    a.n_hyp = rp->n_hyp; a.ransac_min_points = rp->ransac_min_points; a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri;
    a.threshold = rp->threshold; a.goal_fraction = rp->goal_fraction; a.absolute_reference = rp->absolute_reference;
    a.seed = rp->seed; a.frame_base = rp->frame_base;
    a.raw_scale = o->raw_scale; a.model = o->model; a.best_ic = o->best_ic; a.used = o->used; a.hyp_counts = o->hyp_counts;
    return rs_launch(ctx, flat_selection_kernel<true, kFlatDevWaves>, "flat_selection_kernel<device>", b->n_frames, kFlatDevWaves * kWave,
                     flat_plan<size_t>(true, b->max_feat, max_tri, rp->n_hyp).total, a);
}

int mvosr_region_grow_batch(mvosr_ctx *ctx, const mvosr_batch *b, const double *tri_height_in, const double *tri_angle_in,
                            const mvosr_grow_params *gp, const mvosr_grow_outputs *o, int64_t max_tri) {
    if (!ctx || !b || !gp || !o) return set_error(MVOSR_ERR_ARG, "region_grow: null argument");
    if (!o->region || !o->n_region || !o->n_flat || !o->status || !o->level || !o->threshold_height)
        return set_error(MVOSR_ERR_ARG, "region_grow: a required output is null");
    if ((tri_height_in == nullptr) != (tri_angle_in == nullptr)) return set_error(MVOSR_ERR_ARG, "region_grow: heights and angles are given together or not at all");
    const bool pts = tri_height_in == nullptr;
    if (!b->feat_off || !b->feat_cnt || !b->tri2_off || !b->tri2) return set_error(MVOSR_ERR_ARG, "region_grow: missing feat_off/feat_cnt/tri2");
    if (pts && (!b->x || !b->y || !b->z)) return set_error(MVOSR_ERR_ARG, "region_grow: the from-points form needs x/y/z");
    if (b->max_feat < 0) return set_error(MVOSR_ERR_ARG, "region_grow: max_feat < 0");
    if (b->max_feat > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "region_grow: vertex ids are 16-bit in LDS");
    if (b->n_frames <= 0) return MVOSR_OK;
    if (max_tri <= 0) max_tri = 2 * (int64_t)b->max_feat;
    if (max_tri < 1) max_tri = 1;
    if (max_tri >= 65535) return set_error(MVOSR_ERR_TOO_LARGE, "region_grow: row numbers are 16-bit in LDS");
    GrowArgs a = {};
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.x = b->x; a.y = b->y; a.z = b->z;
    a.tri_off = b->tri2_off; a.tri = b->tri2; a.tri_cnt = b->tri2_cnt; a.h_in = tri_height_in; a.ang_in = tri_angle_in;
    a.threshold_angle = gp->threshold_angle; a.seed_deg = gp->seed_deg; a.level_deg = gp->level_deg; a.height_factor = gp->height_factor;
    a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri;
    a.region = o->region; a.n_region = o->n_region; a.n_flat = o->n_flat; a.status = o->status; a.level = o->level;
    a.threshold_height = o->threshold_height; a.label = o->label; a.neighbors = o->neighbors;
    a.tri_height = o->tri_height; a.tri_angle = o->tri_angle;
    return rs_launch(ctx, pts ? region_grow_kernel<true> : region_grow_kernel<false>, "region_grow_kernel", b->n_frames, kRsBlock,
                     grow_plan<size_t>(pts, b->max_feat, max_tri).total, a);
}

int mvosr_slew_median(mvosr_ctx *ctx, const double *raw, const int32_t *apply, int64_t n, double slew, double scale_in,
                      int window, const double *queue_in, int n_queue, double *pushed, double *filtered) {
    if (!ctx || (n > 0 && (!raw || !apply || !pushed || !filtered))) return set_error(MVOSR_ERR_ARG, "slew_median: null argument");
    if (n <= 0) return MVOSR_OK;
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(slew_kernel, dim3(1), dim3(kWave), 0, ctx_stream(ctx), raw, apply, n, slew, scale_in, pushed);
    if ((rc = check_launch("slew_kernel"))) return rc;
    return mvosr_window_median(ctx, pushed, n, window, queue_in, n_queue, filtered);    // np.median(self.scale_queue), rescale.py:178
}

static int launch_ransac(mvosr_ctx *ctx, int64_t n_frames, const int64_t *pts_off, const int32_t *pts_cnt,
                         const double *px, const double *py, const double *pz, const int32_t *samples, int n_hyp,
                         double threshold, double goal_fraction, int32_t *counts, double *model, int32_t *best_ic,
                         int32_t *used, int line) {
    if (!ctx || !pts_off || !pts_cnt || !px || !py || (!pz && !line) || !samples || !model || !best_ic || !used)
        return set_error(MVOSR_ERR_ARG, "ransac: null argument");
    if (n_hyp < 1 || n_hyp > kMaxHyp) return set_error(MVOSR_ERR_ARG, "ransac: n_hyp must be in 1..%d", kMaxHyp);
    if (n_frames <= 0) return MVOSR_OK;
    RansacArgs a;
    a.n_frames = n_frames; a.pts_off = pts_off; a.pts_cnt = pts_cnt; a.px = px; a.py = py; a.pz = pz; a.triples = samples;
    a.n_hyp = n_hyp; a.threshold = threshold; a.goal_fraction = goal_fraction; a.counts = counts; a.model = model;
    a.best_ic = best_ic; a.used = used; a.line = line;
    // (kMaxHyp hypotheses are 18 KB: no limit to raise)
    return rs_launch(ctx, ransac_plane_kernel, "ransac_plane_kernel", n_frames, kRsBlock, ransac_plan<size_t>(n_hyp).total, a, false);
}

int mvosr_ransac_plane_batch(mvosr_ctx *ctx, int64_t n_frames, const int64_t *pts_off, const int32_t *pts_cnt,
                             const double *px, const double *py, const double *pz, const int32_t *triples, int n_hyp,
                             double threshold, double goal_fraction, int32_t *counts, double *model, int32_t *best_ic,
                             int32_t *used) {
    return launch_ransac(ctx, n_frames, pts_off, pts_cnt, px, py, pz, triples, n_hyp, threshold, goal_fraction, counts, model,
                         best_ic, used, 0);
}

int mvosr_ransac_line_batch(mvosr_ctx *ctx, int64_t n_frames, const int64_t *pts_off, const int32_t *pts_cnt,
                            const double *px, const double *py, const int32_t *pairs, int n_hyp,
                            double threshold, double goal_fraction, int32_t *counts, double *model, int32_t *best_ic,
                            int32_t *used) {
    return launch_ransac(ctx, n_frames, pts_off, pts_cnt, px, py, nullptr, pairs, n_hyp, threshold, goal_fraction, counts, model,
                         best_ic, used, 1);
}

int mvosr_triangle_batch(mvosr_ctx *ctx, const mvosr_batch *b, double focus, double cx, double cy, double s_min,
                         double n_sigma, double *height, int32_t *counts, int32_t *status) {
    if (!ctx || !b || !height || !counts || !status) return set_error(MVOSR_ERR_ARG, "triangle_batch: null argument");
    if (!b->feat_off || !b->feat_cnt || !b->x || !b->v || !b->z || !b->tri1_off || !b->tri1)
        return set_error(MVOSR_ERR_ARG, "triangle_batch: missing u (x) / v / depth (z) / tri1");
    if (b->n_frames <= 0) return MVOSR_OK;
    TriBatchArgs a;
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.u = b->x; a.v = b->v; a.depth = b->z;
    a.tri_off = b->tri1_off; a.tri = b->tri1; a.focus = focus; a.cx = cx; a.cy = cy; a.s_min = s_min; a.n_sigma = n_sigma;
    a.max_feat = b->max_feat;
    a.height = height; a.counts = counts; a.status = status;
    return rs_launch(ctx, triangle_batch_kernel, "triangle_batch_kernel", b->n_frames, kRsBlock, tribatch_plan<size_t>(b->max_feat).total, a);
}

int mvosr_plane_inliers(mvosr_ctx *ctx, int64_t n, const double *px, const double *py, const double *pz, const double *model4,
                        double threshold, uint8_t *mask) {
    if (!ctx || !model4 || (n > 0 && (!px || !py || !pz || !mask))) return set_error(MVOSR_ERR_ARG, "plane_inliers: null argument");
    if (n <= 0) return MVOSR_OK;
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(plane_inliers_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx_stream(ctx), n, px, py, pz,
                       model4[0], model4[1], model4[2], model4[3], threshold, mask);
    return check_launch("plane_inliers_kernel");
}

}  // extern "C"
