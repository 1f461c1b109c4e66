// mvosr_heightpitch_tail.hip — what /root/reference/src/calculate_height_pitch.py carries from one frame of its loop to the next
// (:140, :163-167, :202-203), for one chunk of frames in sequence order, behind mvosr_height_pitch_batch on the same stream
// (DESIGN.md §3.26).  A frame with fewer than min_points list points repeats the previous frame's plane and inliers; only the
// height under the prior's pitch is its own: np.mean(Z sin + Y cos) over the inliers of the most recent FITTED frame with the
// carried frame's prior — the host's double to the last bit (the terms in feature order, the sum in NumPy's pairwise order,
// mvosr_npsum.hpp; built with -ffp-contract=off).
//
//   hpt_resolve_kernel   ONE workgroup: per frame its class (fitted / carried / error) from the chunk's statuses, an inclusive
//                        max-scan for "the last fitted frame at or before f", the first frame at which the host must raise, and
//                        every frame's record — final for a fitted frame, the source named for a carried one.
//   hpt_carry_kernel     one workgroup per frame and one more.  A carried frame before the error compacts its source's inliers
//                        (ballot + ordered prefix, feature order) — or takes the carry-in's — and sums its terms; the last
//                        workgroup writes the carry-out record: the state after the last frame before the error.
//
// Integer and fp64 vector arithmetic only; no atomics; every sum in a fixed order: the same bytes every run, whatever the chunking.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mvosr.h"
#include "mvosr_device.hpp"
#include "mvosr_ransac.hpp"
#include "mvosr_npsum.hpp"
#include "mvosr_host.hpp"
#include "mvosr_heightpitch_tail_plan.hpp"

namespace mvosr {

static_assert(kHptBlock == kHptWaves * kWave && kHptNodes == kNpNodes && kHptBlock >= kNpNodes && kHptMaxList == kNpBufSize,
              "one thread per node of one buffer's recursion");
static_assert(sizeof(mvosr_height_pitch_carry) == kHptCarryHeader && sizeof(mvosr_height_pitch_tail_frame) == 56, "include/mvosr.h states the records");

struct HptArgs {
    int32_t n_frames, max_feat, min_points, carry_cap;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *v, *depth;
    double focus, cy;
    const double *prior;           // [F][4]: sin and cos of the prior at [2], [3]
    const double *ransac_height, *refined_mean, *refined_std, *height_t_mean, *refined_pitch;   // the chunk's outputs
    const int32_t *n_inliers, *n_selected, *status;
    const uint8_t *mask;           // laid out like depth
    const char *carry_in; char *carry_out;
    mvosr_height_pitch_tail_frame *frames;
    int64_t *error;
};

enum { HPT_FIT = 0, HPT_CARRY = -1 };                      // a frame's class; an error's class is its MVOSR_HPT_ERR_* kind

__device__ __forceinline__ const mvosr_height_pitch_carry *hpt_header(const char *rec) { return reinterpret_cast<const mvosr_height_pitch_carry *>(rec); }
__device__ __forceinline__ bool hpt_carry_ok(const mvosr_height_pitch_carry *c, int cap) { return !c->halted && c->count >= 0 && c->count <= cap; }

__device__ __forceinline__ int hpt_class(const HptArgs &a, int f) {
    const int st = a.status[f];
    if (st == 0) { const int n = a.feat_cnt[f]; return n > 0 && n <= a.max_feat ? HPT_FIT : MVOSR_HPT_ERR_STATUS; }
    if (st == MVOSR_ST_RS_FEW) return a.n_selected[f] < a.min_points ? HPT_CARRY : MVOSR_HPT_ERR_NO_MODEL;
    if (st == MVOSR_ST_ERR_SINGULAR) return MVOSR_HPT_ERR_SINGULAR;
    if (st == MVOSR_ST_ERR_MASK) return MVOSR_HPT_ERR_MASK;
    if (st == MVOSR_ST_ERR_EMPTY) return MVOSR_HPT_ERR_EMPTY;
    return MVOSR_HPT_ERR_STATUS;
}

__global__ __launch_bounds__(kHptBlock) void hpt_resolve_kernel(const HptArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *misc = reinterpret_cast<int *>(smem + hptail_plan<uint32_t>(0u).misc);
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const mvosr_height_pitch_carry *cin = hpt_header(a.carry_in);
    if (!hpt_carry_ok(cin, a.carry_cap)) {                                           // an earlier chunk ended the call: nothing is final here
        if (tid == 0) *a.error = ((int64_t)MVOSR_HPT_ERR_UPSTREAM << 32);
        return;
    }
    const bool has_prev = cin->has_prev != 0;
    int run = -1;                                                                    // the last fitted frame of the rounds before
    long long first = LLONG_MAX;                                                     // the first error so far: frame << 8 | kind
    const double q = nan("");
    for (int f0 = 0; f0 < a.n_frames; f0 += kHptBlock) {
        const int f = f0 + tid;
        const int cls = f < a.n_frames ? hpt_class(a, f) : HPT_CARRY;
        // inclusive max-scan of "f where fitted": the lanes of a wavefront, then the wavefronts before it, then the rounds before
        int last = f < a.n_frames && cls == HPT_FIT ? f : -1;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) { const int up = __shfl_up(last, o); if (lane >= o) last = max(last, up); }
        if (lane == kWave - 1) misc[HTM_FIT + wave] = last;
        __syncthreads();
        for (int w = 0; w < wave; ++w) last = max(last, misc[HTM_FIT + w]);
        last = max(last, run);
        for (int w = 0; w < kHptWaves; ++w) run = max(run, misc[HTM_FIT + w]);
        if (f < a.n_frames) {
            int kind = cls > 0 ? cls : 0;
            if (cls == HPT_CARRY && last < 0 && !has_prev) kind = MVOSR_HPT_ERR_NO_PREVIOUS;     // :167
            if (kind) first = min(first, ((long long)f << 8) | kind);
            mvosr_height_pitch_tail_frame r;
            const bool fit = cls == HPT_FIT;
            r.ransac_height = fit ? a.ransac_height[f] : q; r.refined_mean = fit ? a.refined_mean[f] : q;
            r.refined_std = fit ? a.refined_std[f] : q; r.height_t_mean = fit ? a.height_t_mean[f] : q;
            r.refined_pitch = fit ? a.refined_pitch[f] : q;
            r.n_inliers = fit ? a.n_inliers[f] : 0; r.n_selected = a.n_selected[f];
            r.carried = cls == HPT_CARRY ? 1 : 0; r.source = last;
            a.frames[f] = r;
        }
        __syncthreads();                                                             // (misc is written again in the next round)
    }
    // the first error of the chunk: lanes, wavefronts
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) { const long long other = __shfl_xor(first, o); first = other < first ? other : first; }
    long long *slots = reinterpret_cast<long long *>(misc + HTM_ERR);
    if (lane == 0) slots[wave] = first;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kHptWaves; ++w) first = slots[w] < first ? slots[w] : first;
        *a.error = first == LLONG_MAX ? -1 : (((first & 0xff) << 32) | (first >> 8));
    }
}

// The inliers of frame g (mask != 0), in feature order: visit(position, feature index, Y, Z) for each, by the lane that holds it.
// Returns their number.  Holds a barrier (ordered_prefix): every thread of the workgroup calls it.
template <class Visit>
__device__ __forceinline__ int hpt_compact(const HptArgs &a, int g, int *misc, Visit visit) {
    const int n = a.feat_cnt[g], lane = lane_id();
    const int64_t off = a.feat_off[g];
    int s0, s1;
    ordered_segment(n, kHptBlock, s0, s1);
    int c = 0;
    for (int i0 = s0; i0 < s1; i0 += kWave) {
        const int i = i0 + lane;
        c += __popcll(__ballot(i < s1 && a.mask[off + i] != 0));
    }
    int base, K;
    ordered_prefix<kHptWaves>(misc + HTM_CW, c, base, K);
    for (int i0 = s0; i0 < s1; i0 += kWave) {
        const int i = i0 + lane;
        const bool in = i < s1 && a.mask[off + i] != 0;
        const int pos = ordered_rank(in, base);
        if (in) {
            const double d = a.depth[off + i];
            visit(pos, i, d * (a.v[off + i] - a.cy) / a.focus, d);                   // :68, back_project's operation order
        }
    }
    return K;
}

__global__ __launch_bounds__(kHptBlock) void hpt_carry_kernel(const HptArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int f = blockIdx.x, F = a.n_frames;
    const mvosr_height_pitch_carry *cin = hpt_header(a.carry_in);
    mvosr_height_pitch_carry *cout = reinterpret_cast<mvosr_height_pitch_carry *>(a.carry_out);
    const auto rin = hpcarry_plan<uint32_t>((uint32_t)a.carry_cap);
    const double *in_y = reinterpret_cast<const double *>(a.carry_in + rin.y), *in_z = reinterpret_cast<const double *>(a.carry_in + rin.z);
    const int32_t *in_idx = reinterpret_cast<const int32_t *>(a.carry_in + rin.index);
    double *out_y = reinterpret_cast<double *>(a.carry_out + rin.y), *out_z = reinterpret_cast<double *>(a.carry_out + rin.z);
    int32_t *out_idx = reinterpret_cast<int32_t *>(a.carry_out + rin.index);
    const int64_t err = *a.error;
    const bool upstream = !hpt_carry_ok(cin, a.carry_cap);
    const int end = upstream ? 0 : (err < 0 ? F : (int)(err & 0xffffffffll));        // frames before the first error: final

    if (f < F) {                                                                     // ---- a carried frame (:163-165, :202-203)
        if (f >= end || !a.frames[f].carried) return;
        const int g = a.frames[f].source;                                            // its inliers' frame; -1: the carry-in's
        const int n = g >= 0 ? a.feat_cnt[g] : cin->count;
        const auto lds = hptail_plan<uint32_t>((uint32_t)n);
        double *terms = reinterpret_cast<double *>(smem + lds.terms);
        double *node = reinterpret_cast<double *>(smem + lds.node);
        int *misc = reinterpret_cast<int *>(smem + lds.misc);
        const double sin_est = a.prior[4 * (int64_t)f + 2], cos_est = a.prior[4 * (int64_t)f + 3];
        int k;
        if (g >= 0) k = hpt_compact(a, g, misc, [&](int pos, int, double y, double z) { terms[pos] = z * sin_est + y * cos_est; });
        else {
            k = n;
            for (int i = tid; i < k; i += kHptBlock) terms[i] = in_z[i] * sin_est + in_y[i] * cos_est;
        }
        __syncthreads();
        const double h_t = block_np_sum(terms, k, node, node + kHptNodes) / (double)k;   // np.mean
        if (tid == 0) {
            mvosr_height_pitch_tail_frame r = a.frames[f];
            if (g >= 0) {
                const mvosr_height_pitch_tail_frame s = a.frames[g];
                r.ransac_height = s.ransac_height; r.refined_mean = s.refined_mean; r.refined_std = s.refined_std;
                r.refined_pitch = s.refined_pitch; r.n_inliers = s.n_inliers;
            } else {
                r.ransac_height = cin->ransac_height; r.refined_mean = cin->refined_mean; r.refined_std = cin->refined_std;
                r.refined_pitch = cin->refined_pitch; r.n_inliers = cin->n_inliers;
            }
            r.height_t_mean = h_t;
            a.frames[f] = r;
            if (f == end - 1) cout->height_t_mean = h_t;                             // (the carry-out's other members: the last workgroup)
        }
        return;
    }

    // ---- the carry-out: the state after frame end - 1
    const int g = end > 0 ? a.frames[end - 1].source : -1;                           // the last fitted frame before the error
    int *misc = reinterpret_cast<int *>(smem + hptail_plan<uint32_t>(0u).misc);
    const int halted = (upstream || err >= 0) ? 1 : 0;
    if (g >= 0) {
        const int k = hpt_compact(a, g, misc, [&](int pos, int i, double y, double z) { out_y[pos] = y; out_z[pos] = z; out_idx[pos] = i; });
        if (tid == 0) {
            const mvosr_height_pitch_tail_frame s = a.frames[g];
            cout->ransac_height = s.ransac_height; cout->refined_mean = s.refined_mean; cout->refined_std = s.refined_std;
            cout->refined_pitch = s.refined_pitch; cout->n_inliers = s.n_inliers;
            if (g == end - 1) cout->height_t_mean = s.height_t_mean;                 // (else: frame end - 1 is carried and writes it)
            cout->has_prev = 1; cout->count = k; cout->halted = halted; cout->reserved = 0;
        }
        return;
    }
    const int k = min(max(cin->count, 0), a.carry_cap);
    for (int i = tid; i < k; i += kHptBlock) { out_y[i] = in_y[i]; out_z[i] = in_z[i]; out_idx[i] = in_idx[i]; }
    if (tid == 0) {
        cout->ransac_height = cin->ransac_height; cout->refined_mean = cin->refined_mean; cout->refined_std = cin->refined_std;
        cout->refined_pitch = cin->refined_pitch; cout->n_inliers = cin->n_inliers;
        if (end == 0) cout->height_t_mean = cin->height_t_mean;
        cout->has_prev = cin->has_prev; cout->count = cin->count; cout->halted = halted; cout->reserved = 0;
    }
}

}  // namespace mvosr

using namespace mvosr;

extern "C" {

size_t mvosr_height_pitch_tail_lds_bytes(int max_feat) { return hptail_plan<size_t>(max_feat > 0 ? (size_t)max_feat : 0).total; }

size_t mvosr_height_pitch_carry_bytes(int carry_cap) { return hpcarry_plan<size_t>(carry_cap > 0 ? (size_t)carry_cap : 0).total; }

int mvosr_height_pitch_tail_batch(mvosr_ctx *ctx, const mvosr_batch *b, const mvosr_height_pitch_params *p, const double *frame_prior,
                                  const mvosr_height_pitch_outputs *o, const void *carry_in, void *carry_out, int32_t carry_cap,
                                  mvosr_height_pitch_tail_frame *frames, int64_t *error) {
    if (!ctx || !b || !p || !frame_prior || !o || !carry_in || !carry_out || !frames || !error)
        return set_error(MVOSR_ERR_ARG, "height_pitch_tail: null argument");
    if (!o->ransac_height || !o->n_selected || !o->n_inliers || !o->refined_pitch || !o->refined_mean || !o->refined_std || !o->height_t_mean ||
        !o->status || !o->mask)
        return set_error(MVOSR_ERR_ARG, "height_pitch_tail: the chunk's outputs, the mask included");
    if (!b->feat_off || !b->feat_cnt || !b->v || !b->z) return set_error(MVOSR_ERR_ARG, "height_pitch_tail: missing feat_off / feat_cnt / v / depth (z)");
    if (carry_in == carry_out) return set_error(MVOSR_ERR_ARG, "height_pitch_tail: the carry-in and the carry-out are the same record");
    if (b->max_feat < 0 || carry_cap < b->max_feat) return set_error(MVOSR_ERR_ARG, "height_pitch_tail: carry_cap must be at least max_feat >= 0");
    if (p->min_points < 3) return set_error(MVOSR_ERR_ARG, "height_pitch_tail: min_points < 3");
    if (b->n_frames <= 0) return MVOSR_OK;
    if (b->n_frames >= INT32_MAX) return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch_tail: 2^31 frames in one chunk");
    if (carry_cap > kHptMaxList) return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch_tail: a list of %d inliers (limit: %d)", carry_cap, kHptMaxList);
    const size_t lds = hptail_plan<size_t>((size_t)carry_cap).total;
    if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch_tail: a list of %d inliers needs %zu B of LDS (> %d)", carry_cap, lds, ctx->max_lds_per_block);
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(hpt_carry_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    HptArgs a = {};
    a.n_frames = (int32_t)b->n_frames; a.max_feat = b->max_feat; a.min_points = p->min_points; a.carry_cap = carry_cap;
    a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.v = b->v; a.depth = b->z; a.focus = p->focus; a.cy = p->cy; a.prior = frame_prior;
    a.ransac_height = o->ransac_height; a.refined_mean = o->refined_mean; a.refined_std = o->refined_std; a.height_t_mean = o->height_t_mean;
    a.refined_pitch = o->refined_pitch; a.n_inliers = o->n_inliers; a.n_selected = o->n_selected; a.status = o->status; a.mask = o->mask;
    a.carry_in = static_cast<const char *>(carry_in); a.carry_out = static_cast<char *>(carry_out); a.frames = frames; a.error = error;
    hipLaunchKernelGGL(hpt_resolve_kernel, dim3(1), dim3(kHptBlock), hptail_plan<size_t>(0).total, ctx_stream(ctx), a);
    rc = check_launch("hpt_resolve_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(hpt_carry_kernel, dim3((unsigned)b->n_frames + 1u), dim3(kHptBlock), lds, ctx_stream(ctx), a);
    return check_launch("hpt_carry_kernel");
}

}  // extern "C"
