// mvosr_reliability.hip — the reference's graph-reliability feature vote (find_reliability_by_graph,
// /root/reference/src/scale_calculator.py:127-149 with triangle2graph :86-99 and check_depth :121-125) on the device.
//
// Every feature starts at reliability 0.8; the edges of the first triangulation are walked once, in the order
// (lower end i, first row that names both ends, upper end j), and each edge rewrites the reliabilities of both its ends from
// the values it finds there.  An edge therefore depends only on the edge before it at each of its two ends: the edges that
// are next at BOTH ends are independent of each other (no two of them share a vertex) and are applied together, round after
// round — the same values, bit for bit, as the sequential loop.
//
// One frame per workgroup.  An "offer" is a (row, slot) pair, numbered 3 * row + slot: with the row sorted to (s0, s1, s2),
// slot 0, 1, 2 is the edge (s0, s1), (s0, s2), (s1, s2) — the order in which triangle2graph offers a row's edges (:93-98).
// An edge is identified with its FIRST offer (the smallest row that names both ends); within one lower end, first offers in
// ascending number are ordered by (first row, j), because a row's slots 0 and 1 have s1 < s2.
//   1  z' (the engine's remap, at load) and v into LDS; the rows checked (ids, repeated vertices) and stored sorted, 16-bit;
//   2  a vertex -> incident rows table (counts, block scan, fill), as in region_grow_kernel;
//   3  per offer two bits: "first" (no smaller incident row of the edge's lower-degree end names the other end — exact however
//      many rows name an edge) and "abnormal" (the fp64 product (v_i - v_j) * (z_i - z_j) > 0, :122).  z', v are dead;
//   4  per vertex its incident edges in the order the loop meets them: as the upper end by ascending lower end (the outer loop
//      runs over i ascending, :130), then its own block by ascending first offer.  Each first offer finds its two places by
//      counting, over the incident rows of each end, the first offers that come before it: no sort, no atomics;
//   5  rounds: a vertex whose next edge it is the LOWER end of looks whether that edge is next at the upper end too
//      ("decide"), a barrier, the update (:132-143, every operation rounded separately: the file is built with
//      -ffp-contract=off) and both pointers advanced ("commit"), a barrier.  The first edge of the sequential order that is
//      still open is always next at both its ends, so every round applies at least one edge; there is no cap on the rounds
//      (a strip numbered along its length has one edge per round).
// LDS: reliability_plan() (mvosr_reliability_plan.hpp), carved at the header's sizes: 69.5 bytes per feature at
// max_tri = 2 max_feat — 136 KB for 2 000 features.
#include "mvosr_device.hpp"
#include "mvosr_host.hpp"
#include "mvosr_reliability_plan.hpp"

namespace mvosr {

constexpr int kRelBlock = kRsWaves * kWave;

struct ReliabilityArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *y, *z, *v;
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    double cos_pitch, sin_pitch;
    int32_t max_feat, max_tri;               // what the launch's LDS was sized from
    double *reliability;                     // [features]
    int32_t *keep;                           // [features] 0: survives, -1: not
    int32_t *status;                         // [F]
};

// the two ends of offer o = 3 t + e in the sorted rows
__device__ __forceinline__ void offer_ends(const uint16_t *R16, int o, int &i, int &j) {
    const int t = o / 3, e = o - 3 * t;
    i = R16[3 * t + (e == 2 ? 1 : 0)];
    j = R16[3 * t + (e == 0 ? 1 : 2)];
}

// A[0 .. cnt) becomes its inclusive prefix sum: a contiguous chunk per thread, wave scan, wave totals through `wsum`.
// Holds barriers: every thread of the workgroup calls it.
__device__ __forceinline__ void block_scan_incl(int *A, int cnt, int *wsum) {
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const int chunk = (cnt + kRelBlock - 1) / kRelBlock;
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

__global__ __launch_bounds__(kRelBlock) void reliability_kernel(const ReliabilityArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int n_all = a.feat_cnt[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    const int tid = threadIdx.x, lane = lane_id();
    const int n = max(n_all, 0);
    const int64_t off = a.feat_off[f];
    if (n_all > a.max_feat || tn > a.max_tri) {
        // more features or rows than the launch's LDS was sized for: refused, LDS untouched, nobody survives, no reliability written
        for (int i = tid; i < n; i += kRelBlock) a.keep[off + i] = -1;
        if (tid == 0) a.status[f] = MVOSR_ST_ERR_MASK;
        return;
    }
    if (tn <= 0) {
        // no rows: what the reference's loop leaves (:129,:145) — every feature at 0.8, nobody above it
        for (int i = tid; i < n; i += kRelBlock) { a.reliability[off + i] = 0.8; a.keep[off + i] = -1; }
        if (tid == 0) a.status[f] = 0;
        return;
    }
    const auto lds = reliability_plan<uint32_t>(a.max_feat, a.max_tri);    // (mvosr_reliability_plan.hpp: the layout, and what lives when)
    double *Z = reinterpret_cast<double *>(smem + lds.z), *V = reinterpret_cast<double *>(smem + lds.v);   // (phases 1-3)
    int *St = reinterpret_cast<int *>(smem + lds.st);                           // [n + 1] where a vertex's rows start ([n]: 3 tn)
    uint16_t *It = reinterpret_cast<uint16_t *>(smem + lds.it);                 // [3 tn] incident rows, vertex by vertex
    uint16_t *R16 = reinterpret_cast<uint16_t *>(smem + lds.r16);               // [tn][3] sorted rows
    uint16_t *Inc = reinterpret_cast<uint16_t *>(smem + lds.inc);               // [2 E] incident first offers, vertex by vertex
    uint32_t *First = reinterpret_cast<uint32_t *>(smem + lds.first), *Abn = reinterpret_cast<uint32_t *>(smem + lds.abn);
    int *misc = reinterpret_cast<int *>(smem + lds.misc);
    const int32_t *rows = a.tri + 3 * tb;
    const int n_off = 3 * tn, n_words = (n_off + 31) / 32;
    // ---- phase 1: z', v; the rows checked and sorted
    if (tid < RM_N) misc[tid] = 0;
    {
        const double *gy = a.y + off, *gz = a.z + off, *gv = a.v + off;
        const double cp = a.cos_pitch, sp = a.sin_pitch;
        for (int i = tid; i < n; i += kRelBlock) { Z[i] = gy[i] * sp + gz[i] * cp; V[i] = gv[i]; }   // scale_calculator.py:392
    }
    for (int v = tid; v <= n; v += kRelBlock) St[v] = 0;
    for (int w = tid; w < n_words; w += kRelBlock) { First[w] = 0u; Abn[w] = 0u; }
    __syncthreads();
    {
        int bad = 0;
        for (int t = tid; t < tn; t += kRelBlock) {
            const TriIds q = load_tri(rows, t);
            if (!ids_in_range(q.a, q.b, q.c, n) || q.a == q.b || q.a == q.c || q.b == q.c) { bad = 1; continue; }
            const int s0 = min(q.a, min(q.b, q.c)), s2 = max(q.a, max(q.b, q.c)), s1 = q.a + q.b + q.c - s0 - s2;   // :92
            R16[3 * t] = (uint16_t)s0; R16[3 * t + 1] = (uint16_t)s1; R16[3 * t + 2] = (uint16_t)s2;
        }
        if (bad) misc[RM_BAD] = 1;
    }
    __syncthreads();
    if (misc[RM_BAD]) {
        // a row that names a vertex twice or an id outside [0, n): refused, not guessed
        for (int i = tid; i < n; i += kRelBlock) a.keep[off + i] = -1;
        if (tid == 0) a.status[f] = MVOSR_ST_ERR_MASK;
        return;
    }
    // ---- phase 2: per vertex its incident rows
    for (int t = tid; t < tn; t += kRelBlock) {
#pragma unroll
        for (int e = 0; e < 3; ++e) atomicAdd(&St[R16[3 * t + e]], 1);
    }
    __syncthreads();
    block_scan_incl(St, n + 1, misc + RM_WSUM);
    for (int t = tid; t < tn; t += kRelBlock) {
#pragma unroll
        for (int e = 0; e < 3; ++e) It[atomicSub(&St[R16[3 * t + e]], 1) - 1] = (uint16_t)t;   // (the ends count down to the starts)
    }
    __syncthreads();
    // ---- phase 3: per offer, is it its edge's first, and is the edge abnormal
    for (int o = tid; o < n_off; o += kRelBlock) {
        int i, j;
        offer_ends(R16, o, i, j);
        const int t = o / 3;
        int p = i, q = j;
        if (St[p + 1] - St[p] > St[q + 1] - St[q]) { p = j; q = i; }
        bool first = true;
        for (int k = St[p], k1 = St[p + 1]; k < k1; ++k) {
            const int r = It[k];
            if (r < t && (R16[3 * r] == q || R16[3 * r + 1] == q || R16[3 * r + 2] == q)) { first = false; break; }
        }
        if (first) atomicOr(&First[o >> 5], 1u << (o & 31));
        if ((V[i] - V[j]) * (Z[i] - Z[j]) > 0.0) atomicOr(&Abn[o >> 5], 1u << (o & 31));       // :122 — the product, not the signs
    }
    __syncthreads();
    // ---- phase 4: per vertex its edges in the loop's order (z', v are dead: the late aliases take their room)
    double *R = reinterpret_cast<double *>(smem + lds.rel);
    int *Ls = reinterpret_cast<int *>(smem + lds.lstart);                       // [n + 1]
    int *Ptr = reinterpret_cast<int *>(smem + lds.ptr);                         // [n]
    for (int v = tid; v <= n; v += kRelBlock) Ls[v] = 0;
    for (int i = tid; i < n; i += kRelBlock) R[i] = 0.8;                         // :129
    __syncthreads();
    auto is_first = [&](int o) -> bool { return (First[o >> 5] >> (o & 31)) & 1u; };
    for (int o = tid; o < n_off; o += kRelBlock) {
        if (!is_first(o)) continue;
        int i, j;
        offer_ends(R16, o, i, j);
        atomicAdd(&Ls[i + 1], 1); atomicAdd(&Ls[j + 1], 1);                       // (shifted by one: the scan leaves the starts)
    }
    __syncthreads();
    block_scan_incl(Ls, n + 1, misc + RM_WSUM);
    const int n_edges = Ls[n] >> 1;
    for (int o = tid; o < n_off; o += kRelBlock) {
        if (!is_first(o)) continue;
        int i, j;
        offer_ends(R16, o, i, j);
        // at the lower end: behind every edge it is the upper end of, among its own first offers by ascending number
        int upper = 0, before = 0;
        for (int k = St[i], k1 = St[i + 1]; k < k1; ++k) {
            const int r = It[k];
            const int s0 = R16[3 * r], s1 = R16[3 * r + 1];
            if (s0 == i) {
                before += (3 * r < o && is_first(3 * r)) ? 1 : 0;
                before += (3 * r + 1 < o && is_first(3 * r + 1)) ? 1 : 0;
            } else if (s1 == i) {
                upper += is_first(3 * r) ? 1 : 0;
                before += (3 * r + 2 < o && is_first(3 * r + 2)) ? 1 : 0;
            } else {
                upper += (is_first(3 * r + 1) ? 1 : 0) + (is_first(3 * r + 2) ? 1 : 0);
            }
        }
        Inc[Ls[i] + upper + before] = (uint16_t)o;
        // at the upper end: among the edges it is the upper end of, by ascending lower end
        int below = 0;
        for (int k = St[j], k1 = St[j + 1]; k < k1; ++k) {
            const int r = It[k];
            const int s0 = R16[3 * r], s1 = R16[3 * r + 1];
            if (s1 == j) {
                below += (s0 < i && is_first(3 * r)) ? 1 : 0;
            } else if (s0 != j) {
                below += (s0 < i && is_first(3 * r + 1)) ? 1 : 0;
                below += (s1 < i && is_first(3 * r + 2)) ? 1 : 0;
            }
        }
        Inc[Ls[j] + below] = (uint16_t)o;
    }
    for (int i = tid; i < n; i += kRelBlock) Ptr[i] = Ls[i];
    __syncthreads();
    // ---- phase 5: the rounds.  A thread's vertices are tid, tid + kRelBlock, ...: at most 22 of them (3 max_tri < 65536 and
    // a row has three distinct vertices bound n where rows exist; the launcher refuses more), one bit of `go` each.
    int applied = 0;                                                            // (the same in every thread)
    while (applied < n_edges) {
        unsigned long long go = 0ull;
        int it = 0;
        for (int k = tid; k < n; k += kRelBlock, ++it) {
            const int p = Ptr[k];
            if (p >= Ls[k + 1]) continue;
            const int o = Inc[p];
            int i, j;
            offer_ends(R16, o, i, j);
            if (i != k) continue;                                               // (the edge's lower end decides)
            const int pj = Ptr[j];
            if (pj < Ls[j + 1] && Inc[pj] == o) go |= 1ull << it;
        }
        __syncthreads();                                                        // decide | commit
        int done = 0;
        it = 0;
        for (int k = tid; k < n; k += kRelBlock, ++it) {
            if (!((go >> it) & 1ull)) continue;
            const int o = Inc[Ptr[k]];
            int i, j;
            offer_ends(R16, o, i, j);
            const double ri = R[i], rj = R[j];
            const double pa = ri * rj;                                          // :132
            const double pb = (1.0 - ri) * rj;                                  // :133
            const double pc = (1.0 - rj) * ri;                                  // :134
            const double pd = (1.0 - ri) * (1.0 - rj);                          // :135
            double ni, nj;
            if ((Abn[o >> 5] >> (o & 31)) & 1u) {
                const double den = 0.25 * (pb + pc) + 0.5 * pd;
                ni = (0.25 * pc) / den;                                         // :138
                nj = (0.25 * pb) / den;                                         // :139
            } else {
                const double den = (pa + 0.25 * (pb + pc)) + 0.5 * pd;
                ni = (pa + 0.25 * pc) / den;                                    // :142
                nj = (pa + 0.25 * pb) / den;                                    // :143
            }
            R[i] = ni; R[j] = nj;
            Ptr[i] += 1; Ptr[j] += 1;
            ++done;
        }
        done = wave_sum(done);
        if (lane == 0 && done) atomicAdd(&misc[RM_DONE], done);
        __syncthreads();
        const int now = misc[RM_DONE];
        if (now == applied) break;                                              // (a round without an edge: the lists are not the loop's order — see below)
        applied = now;
    }
    if (applied < n_edges) {
        // cannot happen while phase 4 builds every list in the loop's order; kept so that a defect there ends as a refusal, not as a
        // workgroup that never leaves the loop
        for (int i = tid; i < n; i += kRelBlock) a.keep[off + i] = -1;
        if (tid == 0) a.status[f] = MVOSR_ST_ERR_MASK;
        return;
    }
    for (int i = tid; i < n; i += kRelBlock) {
        const double r = R[i];
        a.reliability[off + i] = r;
        a.keep[off + i] = r > 0.8 ? 0 : -1;                                      // :145 (NaN: rejected)
    }
    if (tid == 0) a.status[f] = 0;
}

}  // namespace mvosr

using namespace mvosr;

extern "C" int mvosr_reliability_batch(mvosr_ctx *ctx, const mvosr_params *p, const mvosr_batch *b, double *reliability_out,
                                       int32_t *keep_out, int32_t *status_out) {
    if (!ctx || !p || !b || !reliability_out || !keep_out || !status_out) return set_error(MVOSR_ERR_ARG, "reliability: null argument");
    if (!b->feat_off || !b->feat_cnt || !b->y || !b->z || !b->v || !b->tri1_off || !b->tri1)
        return set_error(MVOSR_ERR_ARG, "reliability: missing feat_off/feat_cnt/y/z/v/tri1");
    if (b->max_feat < 0) return set_error(MVOSR_ERR_ARG, "reliability: max_feat < 0");
    if (b->max_feat > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "reliability: vertex ids are 16-bit in LDS");
    if (b->n_frames <= 0) return MVOSR_OK;
    if (b->n_frames > INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "reliability: more than 2^31-1 frames in one batch");
    int64_t max_tri = 2 * (int64_t)b->max_feat;
    if (max_tri < 1) max_tri = 1;
    if (3 * max_tri > 65535) return set_error(MVOSR_ERR_TOO_LARGE, "reliability: offer numbers are 16-bit in LDS");
    const size_t lds = reliability_plan<size_t>((size_t)b->max_feat, (size_t)max_tri).total;
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_TOO_LARGE, "reliability: frame of %d features needs %zu B of LDS (> %d)", b->max_feat, lds, ctx->max_lds_per_block);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(reliability_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    ReliabilityArgs a = {};
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.y = b->y; a.z = b->z; a.v = b->v;
    a.tri_off = b->tri1_off; a.tri = b->tri1; a.tri_cnt = b->tri1_cnt;
    a.cos_pitch = p->cos_pitch; a.sin_pitch = p->sin_pitch;
    a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri;
    a.reliability = reliability_out; a.keep = keep_out; a.status = status_out;
    hipLaunchKernelGGL(reliability_kernel, dim3((unsigned)b->n_frames), dim3(kRelBlock), lds, ctx_stream(ctx), a);
    return check_launch("reliability_kernel");
}
