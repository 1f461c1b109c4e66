// mvosr_trigraph.hip — the reference's triangle-graph road selection (feature_selection_by_tri_graph,
// /root/reference/src/scale_calculator.py:177-222 with triangle2region_graph :56-81 and compare :169-175) on the device.
//
// Every row of the second triangulation gets a road probability from its pitch, p = (-70 - pitch_deg) / 20 - 0.2 clipped
// at 0 (:188-189).  Every flat row (pitch_deg < -80), in ascending order, then takes one Bayesian update per edge-neighbour
// (:194-213): the neighbour's mean height against its own selects a column of a fixed 4x3 observation matrix, the
// neighbour's probability is its FINAL one when the neighbour is a flat row of lower index and its INITIAL one otherwise.
// A row is written once, so a flat row depends only on its flat lower-index neighbours: the rows whose flat lower-index
// neighbours are all final are independent of each other and are finished together, round after round — the same values,
// bit for bit, as the sequential loop.
//
// One frame per workgroup:
//   0  the rows checked (ids, repeated vertices);
//   1  per row its mean height and pitch — given (PTS = false), or from the frame's remapped points with the expressions
//      of the scale kernel's reference formulation (PTS = true: plane_normal, normalise, asin, degrees; the vertex planes
//      are staged in the work area) —, the initial probability, the flat / steep flags;
//   2  the rows as 16-bit ids and a vertex -> incident rows table (counts, block scan, fill), as in region_grow_kernel;
//   3  per row and edge slot (ab, ac, bc) the row across it — more than one is an edge on more than two rows: refused —,
//      stored in the reference's list order (:62-80): first the lower-index neighbours in slot order, then the
//      higher-index ones ascending;
//   4  height_level = np.mean(heights[pitch_deg >= -80]) (:216) in NumPy's summation order: the steep rows' heights packed
//      in row order, one thread per leaf of the pairwise tree, the leaves' sums added in the recursion's order;
//   5  the rounds.  A flat row that is still open looks at its flat lower-index neighbours' `lvl` (1 + the round that
//      finished them, 0: open): ready when all are below the current round.  It then writes its final probability and its
//      own lvl = round + 1 — a value no reader of THIS round accepts, so a round's result does not depend on the order in
//      which threads run; one barrier per round.  The lowest open flat row is always ready: every round finishes at least
//      one row, and there is no cap on the rounds (a strip numbered along its length has one row per round);
//   6  p_road, valid = p_road > 0.5 (:219), the selected features (:221), the counts.
// The update (:209-210) is  pa = num / den  with  o = observation_matrix[:, cr + 1]  and
//     num = fma(o3, m3, o2 * m2),   den = fma(o0, m0, o2 * m2) + fma(o1, m1, o3 * m3)
// — the association of the strided ddot NumPy's `@` reaches for these operands (include/mvosr.h states the rule); the
// fused operations are written out, everything else is an IEEE operation of its own (the file is built with
// -ffp-contract=off).
// LDS: trigraph_plan() (mvosr_trigraph_plan.hpp), carved at the header's sizes: 78 bytes per feature at
// max_tri = 2 max_feat — 153 KB for 2 000 features.
#include "mvosr_device.hpp"
#include "mvosr_host.hpp"
#include "mvosr_npsum.hpp"
#include "mvosr_trigraph_plan.hpp"

namespace mvosr {

constexpr int kTgBlock = kRsWaves * kWave;
constexpr uint16_t kTgNone = 0xFFFFu;        // "no neighbour": rows are numbered below it

struct TriGraphArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *x, *y, *z;                 // read by the from-points form only
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    const double *h_in, *pitch_in;           // [rows] the given form's mean heights and pitch (deg)
    double cos_pitch, sin_pitch, thr_deg;
    int32_t max_feat, max_tri;               // what the launch's LDS was sized from
    double *p_road, *p_initial;              // optional [rows]
    uint8_t *valid;                          // optional [rows]
    int32_t *neighbors;                      // optional [rows][3]
    double *tri_height, *tri_pitch;          // optional [rows], from-points form
    uint8_t *selected;                       // [features]
    double *height_level;                    // [F]
    int32_t *n_flat, *n_valid, *n_rounds;    // optional [F]
    int32_t *status;                         // [F]
};

// A[0 .. cnt) becomes its inclusive prefix sum: a contiguous chunk per thread, wave scan, wave totals through `wsum`
// (reliability_kernel's scan at this kernel's block size).  Holds barriers: every thread of the workgroup calls it.
__device__ __forceinline__ void tg_block_scan_incl(int *A, int cnt, int *wsum) {
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const int chunk = (cnt + kTgBlock - 1) / kTgBlock;
    const int i0 = min(cnt, tid * chunk), i1 = min(cnt, i0 + chunk);
    int s = 0;
    for (int i = i0; i < i1; ++i) s += A[i];
    const int incl = wave_scan_incl(s);
    __syncthreads();                                             // (wsum's last readers are done)
    if (lane == kWave - 1) wsum[wave] = incl;
    __syncthreads();
    int run = incl - s;
#pragma unroll
    for (int w = 0; w < kRsWaves; ++w) if (w < wave) run += wsum[w];
    for (int i = i0; i < i1; ++i) { run += A[i]; A[i] = run; }
    __syncthreads();
}

// The recursion of NumPy's pairwise sum over n <= kNpBufSize elements, in post-order: visit(lo, len, true) for a leaf (<= 128
// elements, np_leaf_sum's share), visit(lo, len, false) for an inner node once both its halves are done — the halves of
// @TYPE@_pairwise_sum, the first rounded down to a multiple of 8.  One thread walks it; its stack is `stk`, 3 kNpDepth ints
// of LDS (as private arrays it costs the kernel scalar registers it does not have).
template <class Visit>
__device__ __forceinline__ void tg_pairwise_walk(int n, int *stk, Visit visit) {
    int *lo_s = stk, *n_s = stk + kNpDepth, *stage_s = stk + 2 * kNpDepth;
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

// one Bayesian update of a row's probability `pa` by a neighbour of probability `pc` whose mean height is `hc` (:206-210)
__device__ __forceinline__ double tg_update(double pa, double ha, double pc, double hc) {
    const double d = hc - ha;                                                    // compare (:169-175): one subtraction,
    const bool lower = d < -0.1, higher = d > 0.1;                               // both tests strict, a NaN is "equal"
    // observation_matrix[:, cr + 1] (:193)
    const double o0 = 0.33;
    const double o1 = lower ? 0.03 : (higher ? 0.90 : 0.07);
    const double o2 = lower ? 0.90 : (higher ? 0.03 : 0.07);
    const double o3 = lower ? 0.05 : (higher ? 0.05 : 0.9);
    const double m0 = (1.0 - pa) * (1.0 - pc), m1 = (1.0 - pa) * pc, m2 = pa * (1.0 - pc), m3 = pa * pc;   // :209
    const double num = __builtin_fma(o3, m3, o2 * m2);                                                     // :210
    const double den = __builtin_fma(o0, m0, o2 * m2) + __builtin_fma(o1, m1, o3 * m3);
    return num / den;
}

template <bool PTS>
__global__ __launch_bounds__(kTgBlock) void tri_graph_kernel(const TriGraphArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int n_all = a.feat_cnt[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    auto frame_values = [&](int status) {                                       // (tid 0) the per-frame values of a frame without a result
        a.status[f] = status; a.height_level[f] = nan("");
        if (a.n_flat) a.n_flat[f] = 0;
        if (a.n_valid) a.n_valid[f] = 0;
        if (a.n_rounds) a.n_rounds[f] = 0;
    };
    if (n_all > a.max_feat || tn > a.max_tri) {
        // more features or rows than the launch's LDS was sized for: refused, LDS untouched, no per-row or per-feature output written
        if (tid == 0) frame_values(MVOSR_ST_ERR_MASK);
        return;
    }
    const int n = max(n_all, 0);
    const int64_t off = a.feat_off[f];
    if (tn <= 0) {
        // no rows (the reference's np.max of nothing raises, :59): nothing is selected
        for (int i = tid; i < n; i += kTgBlock) a.selected[off + i] = 0;
        if (tid == 0) frame_values(MVOSR_ST_ERR_EMPTY);
        return;
    }
    const auto lds = trigraph_plan<uint32_t>(PTS, a.max_feat, a.max_tri);       // (mvosr_trigraph_plan.hpp: the layout, and what lives when)
    double *H = reinterpret_cast<double *>(smem + lds.h), *P0 = reinterpret_cast<double *>(smem + lds.p0);
    uint16_t *NB = reinterpret_cast<uint16_t *>(smem + lds.nb);                 // [tn][3]
    uint16_t *Lvl = reinterpret_cast<uint16_t *>(smem + lds.lvl);
    uint8_t *Fl = reinterpret_cast<uint8_t *>(smem + lds.flag);
    uint32_t *Sel = reinterpret_cast<uint32_t *>(smem + lds.sel);
    int *misc = reinterpret_cast<int *>(smem + lds.misc);
    const int32_t *rows = a.tri + 3 * tb;
    // a frame refused for what its rows or points say: nothing valid, nothing selected, no other per-row output
    auto refuse = [&](int status) {
        if (a.valid) for (int t = tid; t < tn; t += kTgBlock) a.valid[tb + t] = 0;
        for (int i = tid; i < n; i += kTgBlock) a.selected[off + i] = 0;
        if (tid == 0) frame_values(status);
    };
    // ---- phase 0: the rows checked
    if (tid < TM_N) misc[tid] = 0;
    for (int w = tid; w < (n + 31) / 32; w += kTgBlock) Sel[w] = 0u;
    __syncthreads();
    {
        int bad = 0;
        for (int t = tid; t < tn; t += kTgBlock) {
            const TriIds q = load_tri(rows, t);
            if (!ids_in_range(q.a, q.b, q.c, n) || q.a == q.b || q.a == q.c || q.b == q.c) bad = 1;
        }
        if (bad) misc[TM_BAD] = 1;
    }
    __syncthreads();
    if (misc[TM_BAD]) { refuse(MVOSR_ST_ERR_MASK); return; }                     // a vertex twice in a row, an id outside [0, n)
    // ---- phase 1: mean height, pitch, initial probability, flags
    if constexpr (PTS) {
        double *X = reinterpret_cast<double *>(smem + lds.x), *Y = reinterpret_cast<double *>(smem + lds.y), *Z = reinterpret_cast<double *>(smem + lds.z);
        const double cp = a.cos_pitch, sp = a.sin_pitch;
        for (int i = tid; i < n; i += kTgBlock) {
            const double yy = a.y[off + i], zz = a.z[off + i];
            X[i] = a.x[off + i];
            Y[i] = yy * cp - zz * sp;                                            // :391
            Z[i] = yy * sp + zz * cp;                                            // :392
        }
        __syncthreads();
    }
    {
        int n_flat = 0, n_steep = 0, singular = 0;
        for (int t = tid; t < tn; t += kTgBlock) {
            double h, pitch;
            if constexpr (PTS) {
                const double *X = reinterpret_cast<const double *>(smem + lds.x), *Y = reinterpret_cast<const double *>(smem + lds.y),
                             *Z = reinterpret_cast<const double *>(smem + lds.z);
                const TriIds q = load_tri(rows, t);
                const double y0 = Y[q.a], y1 = Y[q.b], y2 = Y[q.c];
                double nx, ny, nz;
                if (!plane_normal(X[q.a], y0, Z[q.a], X[q.b], y1, Z[q.b], X[q.c], y2, Z[q.c], nx, ny, nz)) singular = 1;   // :181-182
                const double len2 = (nx * nx + ny * ny) + nz * nz;               // :183
                const double len = sqrt(len2);
                const double uy = ny / len;                                      // :184
                pitch = asin(-uy) * 180.0 / 3.141592653589793;                   // :185
                h = div3((y0 + y1) + y2);                                        // :186
                if (a.tri_height) a.tri_height[tb + t] = h;
                if (a.tri_pitch) a.tri_pitch[tb + t] = pitch;
            } else {
                h = a.h_in[tb + t]; pitch = a.pitch_in[tb + t];
            }
            double p = (-70.0 - pitch) / 20.0 - 0.2;                             // :188
            if (p < 0.0) p = 0.0;                                                // :189 (a NaN stays)
            const bool flat = pitch < a.thr_deg, steep = pitch >= a.thr_deg;     // :190-191 (a NaN: neither)
            H[t] = h; P0[t] = p;
            Fl[t] = (uint8_t)((flat ? 1 : 0) | (steep ? 2 : 0));
            Lvl[t] = 0;
            n_flat += flat ? 1 : 0; n_steep += steep ? 1 : 0;
        }
        if (PTS && singular) misc[TM_SINGULAR] = 1;
        n_flat = wave_sum(n_flat); n_steep = wave_sum(n_steep);
        if (lane == 0) { if (n_flat) atomicAdd(&misc[TM_NFLAT], n_flat); if (n_steep) atomicAdd(&misc[TM_NSTEEP], n_steep); }
    }
    __syncthreads();
    if (PTS && misc[TM_SINGULAR]) { refuse(MVOSR_ST_ERR_SINGULAR); return; }     // :181 raises
    // ---- phase 2: the rows in 16 bits, and per vertex its incident rows (the vertex planes are dead)
    {
        uint16_t *R16 = reinterpret_cast<uint16_t *>(smem + lds.r16);           // [tn][3] the rows as given
        uint16_t *It = reinterpret_cast<uint16_t *>(smem + lds.it);             // [3 tn] incident rows, vertex by vertex
        int *St = reinterpret_cast<int *>(smem + lds.st);                       // [n + 1] where a vertex's rows start ([n]: 3 tn)
        for (int v = tid; v <= n; v += kTgBlock) St[v] = 0;
        __syncthreads();
        for (int t = tid; t < tn; t += kTgBlock) {
            const TriIds q = load_tri(rows, t);
            R16[3 * t] = (uint16_t)q.a; R16[3 * t + 1] = (uint16_t)q.b; R16[3 * t + 2] = (uint16_t)q.c;
            atomicAdd(&St[q.a], 1); atomicAdd(&St[q.b], 1); atomicAdd(&St[q.c], 1);
        }
        __syncthreads();
        tg_block_scan_incl(St, n + 1, misc + TM_WSUM);
        for (int t = tid; t < tn; t += kTgBlock) {
#pragma unroll
            for (int e = 0; e < 3; ++e) It[atomicSub(&St[R16[3 * t + e]], 1) - 1] = (uint16_t)t;   // (the ends count down to the starts)
        }
        __syncthreads();
        // ---- phase 3: the row across each edge, in the reference's list order
        int bad = 0;
        for (int t = tid; t < tn; t += kTgBlock) {
            const int va = R16[3 * t], vb = R16[3 * t + 1], vc = R16[3 * t + 2];
            int key[3], val[3];
#pragma unroll
            for (int e = 0; e < 3; ++e) {                                        // (a,b), (a,c), (b,c): :66, :70, :74
                int p = e == 2 ? vb : va, q = e == 0 ? vb : vc;
                if (St[p + 1] - St[p] > St[q + 1] - St[q]) { const int s = p; p = q; q = s; }
                int found = 0, other = -1;
                for (int i = St[p], i1 = St[p + 1]; i < i1; ++i) {
                    const int r = It[i];
                    if (r == t) continue;
                    if (R16[3 * r] == q || R16[3 * r + 1] == q || R16[3 * r + 2] == q) { ++found; other = r; }
                }
                if (found > 1) bad = 1;                                          // an edge on more than two rows
                // an earlier row joins the list when THIS row is visited, in slot order (:68); a later one when IT is visited (:69)
                key[e] = found != 1 ? 0x7FFFFFFF : (other < t ? e : 3 + other);
                val[e] = found != 1 ? (int)kTgNone : other;
            }
#define MVOSR_TG_CSWAP(i, j) if (key[j] < key[i]) { const int k_ = key[i], v_ = val[i]; key[i] = key[j]; val[i] = val[j]; key[j] = k_; val[j] = v_; }
            MVOSR_TG_CSWAP(0, 1) MVOSR_TG_CSWAP(1, 2) MVOSR_TG_CSWAP(0, 1)
#undef MVOSR_TG_CSWAP
            NB[3 * t] = (uint16_t)val[0]; NB[3 * t + 1] = (uint16_t)val[1]; NB[3 * t + 2] = (uint16_t)val[2];
        }
        if (bad) misc[TM_BAD] = 1;
    }
    __syncthreads();
    if (misc[TM_BAD]) { refuse(MVOSR_ST_ERR_MASK); return; }
    const int n_flat = misc[TM_NFLAT], n_steep = misc[TM_NSTEEP];
    // ---- phase 4: height_level in NumPy's order (the table is dead)
    double level = nan("");                                                     // np.mean of an empty slice
    if (n_steep > 0) {
        double *hs = reinterpret_cast<double *>(smem + lds.hs), *leaf = reinterpret_cast<double *>(smem + lds.leaf);
        int *wcnt = misc + TM_WSUM;
        int packed = 0;
        for (int r0 = 0; r0 < tn; r0 += kTgBlock) {
            const int t = r0 + tid;
            const bool steep = t < tn && (Fl[t] & 2);
            const unsigned long long m = __ballot(steep);
            if (lane == 0) wcnt[wave] = __popcll(m);
            __syncthreads();
            int before = packed, total = 0;
#pragma unroll
            for (int i = 0; i < kRsWaves; ++i) { const int c = wcnt[i]; if (i < wave) before += c; total += c; }
            if (steep) hs[before + __popcll(m & ((1ull << lane) - 1ull))] = H[t];
            packed += total;
            __syncthreads();
        }
        // np.add.reduce's tree over each 8192-element chunk (mvosr_npsum.hpp): thread 0 walks it once and lists the leaves,
        // one thread per leaf sums it (np_leaf_sum), thread 0 walks it again and adds the sums in the recursion's order
        double *slot = leaf + TL_SLOT, *val = leaf + TL_VAL;
        int *stk = reinterpret_cast<int *>(leaf + TL_STACK);
        uint16_t *tab = reinterpret_cast<uint16_t *>(leaf + TL_TABLE);          // [leaves][2] where a leaf starts, its length
        for (int c0 = 0; c0 < n_steep; c0 += kNpBufSize) {
            const int m = min(kNpBufSize, n_steep - c0);
            if (tid == 0) {
                int k = 0;
                tg_pairwise_walk(m, stk, [&](int lo, int len, bool is_leaf) {
                    if (is_leaf) { tab[2 * k] = (uint16_t)lo; tab[2 * k + 1] = (uint16_t)len; ++k; }
                });
                misc[TM_LEAVES] = k;
            }
            __syncthreads();
            for (int k = tid, k1 = misc[TM_LEAVES]; k < k1; k += kTgBlock) leaf[k] = np_leaf_sum(hs + c0 + tab[2 * k], tab[2 * k + 1], 0.0, false);
            __syncthreads();
            if (tid == 0) {
                int vp = 0, kk = 0;
                tg_pairwise_walk(m, stk, [&](int, int, bool is_leaf) {
                    if (is_leaf) val[vp++] = leaf[kk++];
                    else { const double r = val[--vp], l = val[--vp]; val[vp++] = l + r; }
                });
                *slot = c0 == 0 ? val[0] : *slot + val[0];
            }
            __syncthreads();
        }
        level = (0.0 + *slot) / (double)n_steep;                                 // :216
        __syncthreads();                                                         // (hs gives way to p1)
    }
    // ---- phase 5: the rounds
    double *P1 = reinterpret_cast<double *>(smem + lds.p1);
    volatile uint16_t *Lv = Lvl;
    int finished = 0, round = 0;                                                // (the same in every thread)
    while (finished < n_flat) {
        if (tid == 0) misc[TM_CNT + (round + 1) % 3] = 0;                        // (read last two rounds ago)
        int done = 0;
        for (int t = tid; t < tn; t += kTgBlock) {
            if (!(Fl[t] & 1) || Lv[t]) continue;
            const int u0 = NB[3 * t], u1 = NB[3 * t + 1], u2 = NB[3 * t + 2];
            // which neighbours are read at their final value, and are those final: flat rows of lower index (none: 0xFFFF > t)
            const bool f0 = u0 < t && (Fl[u0] & 1), f1 = u1 < t && (Fl[u1] & 1), f2 = u2 < t && (Fl[u2] & 1);
            bool ready = true;
            if (f0) { const int l = Lv[u0]; ready = ready && l != 0 && l <= round; }
            if (f1) { const int l = Lv[u1]; ready = ready && l != 0 && l <= round; }
            if (f2) { const int l = Lv[u2]; ready = ready && l != 0 && l <= round; }
            if (!ready) continue;
            const double ha = H[t];
            double pa = P0[t];
            if (u0 != kTgNone) pa = tg_update(pa, ha, f0 ? P1[u0] : P0[u0], H[u0]);
            if (u1 != kTgNone) pa = tg_update(pa, ha, f1 ? P1[u1] : P0[u1], H[u1]);
            if (u2 != kTgNone) pa = tg_update(pa, ha, f2 ? P1[u2] : P0[u2], H[u2]);
            P1[t] = pa;                                                          // :213
            Lv[t] = (uint16_t)(round + 1);
            ++done;
        }
        done = wave_sum(done);
        if (lane == 0 && done) atomicAdd(&misc[TM_CNT + round % 3], done);
        __syncthreads();
        const int now = misc[TM_CNT + round % 3];
        if (now == 0) break;                                                     // (a round without a row: see below)
        finished += now;
        ++round;
    }
    if (finished < n_flat) {
        // cannot happen — the lowest open flat row is always ready —; kept so that a defect ends as a refusal, not as a
        // workgroup that never leaves the loop
        refuse(MVOSR_ST_ERR_MASK);
        return;
    }
    // ---- phase 6: the outputs
    {
        int n_valid = 0;
        for (int t = tid; t < tn; t += kTgBlock) {
            const double p0 = P0[t], p = (Fl[t] & 1) ? P1[t] : p0;
            const bool valid = p > 0.5;                                          // :219 (a NaN: not valid)
            if (a.p_road) a.p_road[tb + t] = p;
            if (a.p_initial) a.p_initial[tb + t] = p0;
            if (a.valid) a.valid[tb + t] = valid ? 1 : 0;
            if (a.neighbors) {
                int32_t *nb = a.neighbors + 3 * (tb + t);
#pragma unroll
                for (int e = 0; e < 3; ++e) { const uint16_t u = NB[3 * t + e]; nb[e] = u == kTgNone ? -1 : (int32_t)u; }
            }
            if (valid) {
                const TriIds q = load_tri(rows, t);                              // :221
                atomicOr(&Sel[q.a >> 5], 1u << (q.a & 31)); atomicOr(&Sel[q.b >> 5], 1u << (q.b & 31)); atomicOr(&Sel[q.c >> 5], 1u << (q.c & 31));
                ++n_valid;
            }
        }
        n_valid = wave_sum(n_valid);
        if (lane == 0 && n_valid) atomicAdd(&misc[TM_NVALID], n_valid);
    }
    __syncthreads();
    for (int i = tid; i < n; i += kTgBlock) a.selected[off + i] = (uint8_t)((Sel[i >> 5] >> (i & 31)) & 1u);
    if (tid == 0) {
        a.status[f] = 0; a.height_level[f] = level;
        if (a.n_flat) a.n_flat[f] = n_flat;
        if (a.n_valid) a.n_valid[f] = misc[TM_NVALID];
        if (a.n_rounds) a.n_rounds[f] = round;
    }
}

}  // namespace mvosr

using namespace mvosr;

extern "C" int mvosr_tri_graph_batch(mvosr_ctx *ctx, const mvosr_params *p, const mvosr_batch *b, const double *tri_height_in,
                                     const double *tri_pitch_in, const mvosr_trigraph_outputs *o) {
    if (!ctx || !p || !b || !o) return set_error(MVOSR_ERR_ARG, "tri_graph: null argument");
    if (!o->status || !o->selected || !o->height_level) return set_error(MVOSR_ERR_ARG, "tri_graph: a required output is null");
    if ((tri_height_in == nullptr) != (tri_pitch_in == nullptr))
        return set_error(MVOSR_ERR_ARG, "tri_graph: heights and pitch are given together or not at all");
    const bool pts = tri_height_in == nullptr;
    if (!b->feat_off || !b->feat_cnt || !b->tri2_off || !b->tri2) return set_error(MVOSR_ERR_ARG, "tri_graph: missing feat_off/feat_cnt/tri2");
    if (pts && (!b->x || !b->y || !b->z)) return set_error(MVOSR_ERR_ARG, "tri_graph: the from-points form needs x/y/z");
    if (b->max_feat < 0) return set_error(MVOSR_ERR_ARG, "tri_graph: max_feat < 0");
    if (b->max_feat > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "tri_graph: vertex ids are 16-bit in LDS");
    if (b->n_frames <= 0) return MVOSR_OK;
    if (b->n_frames > INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "tri_graph: more than 2^31-1 frames in one batch");
    int64_t max_tri = 2 * (int64_t)b->max_feat;
    if (max_tri < 1) max_tri = 1;
    if (max_tri > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "tri_graph: row numbers are 16-bit in LDS");
    const size_t lds = trigraph_plan<size_t>(pts, (size_t)b->max_feat, (size_t)max_tri).total;
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_TOO_LARGE, "tri_graph: frame of %d features needs %zu B of LDS (> %d)", b->max_feat, lds, ctx->max_lds_per_block);
    void (*kernel)(TriGraphArgs) = pts ? tri_graph_kernel<true> : tri_graph_kernel<false>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    TriGraphArgs a = {};
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.x = b->x; a.y = b->y; a.z = b->z;
    a.tri_off = b->tri2_off; a.tri = b->tri2; a.tri_cnt = b->tri2_cnt; a.h_in = tri_height_in; a.pitch_in = tri_pitch_in;
    a.cos_pitch = p->cos_pitch; a.sin_pitch = p->sin_pitch; a.thr_deg = p->pitch_threshold_deg;
    a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri;
    a.p_road = o->p_road; a.p_initial = o->p_initial; a.valid = o->valid; a.neighbors = o->neighbors;
    a.tri_height = o->tri_height; a.tri_pitch = o->tri_pitch_deg; a.selected = o->selected; a.height_level = o->height_level;
    a.n_flat = o->n_flat; a.n_valid = o->n_valid; a.n_rounds = o->n_rounds; a.status = o->status;
    hipLaunchKernelGGL(kernel, dim3((unsigned)b->n_frames), dim3(kTgBlock), lds, ctx_stream(ctx), a);
    return check_launch("tri_graph_kernel");
}
