// mvosr_hpeval_carry.hip — what the two evaluation scripts (/root/reference/src/calculate_height_pitch_eval.py, _eval_line.py) carry
// from one frame of their loop to the next (:184-188, :223-224), for one chunk of frames in sequence order and every (case, budget)
// of it, behind mvosr_height_pitch_eval_batch / mvosr_height_pitch_eval_budgets_batch on the same stream.  A frame
// with fewer than min_points list points repeats, per (case, budget), the last fitted frame's outputs; only the height under the
// prior's pitch is its own: (sum_z sin + sum_y cos) / n_inliers with the carried frame's prior — the host's double to the last bit
// (two products, a sum, a division; built with -ffp-contract=off and written with the _rn intrinsics, which are never fused).
//
//   hpe_class_kernel     one wavefront per frame: the frame's class (fitted / carried / error kind and, for no-model, the smallest
//                        failing budget) from its C * B status words.
//   hpe_resolve_kernel   ONE workgroup, rounds of 256 frames: an inclusive max-scan for "the last fitted frame at or before f", the
//                        first frame at which the host must raise, carried[] and the error word.
//   hpe_apply_kernel     one thread per (frame, case, budget), a wavefront's lanes along the frames: the [B][C][F] stores of a
//                        wavefront are contiguous.  The threads of the last final frame write the carry-out record.
//
// Integer and fp64 vector arithmetic only; no atomics: the same bytes every run, whatever the chunking.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/mvosr.h"
#include "mvosr_device.hpp"
#include "mvosr_host.hpp"
#include "mvosr_hpeval_carry_plan.hpp"

namespace mvosr {

static_assert(sizeof(mvosr_height_pitch_eval_carry) == kHecCarryHeader, "include/mvosr.h states the record");

struct HecArgs {
    int32_t n_frames, n_cases, n_budgets, n_elem, min_points;
    mvosr_height_pitch_eval_tail_inputs in;
    const double *prior;           // [F][4]: sin and cos of the prior at [2], [3]
    const char *carry_in; char *carry_out;
    mvosr_height_pitch_eval_tail_outputs out;
};

enum { HEC_FIT = 0, HEC_CARRY = -1 };                      // a frame's class; an error's: its MVOSR_HPT_ERR_* kind | budget index << 8

__device__ __forceinline__ const mvosr_height_pitch_eval_carry *hec_header(const char *rec) {
    return reinterpret_cast<const mvosr_height_pitch_eval_carry *>(rec);
}
__device__ __forceinline__ bool hec_carry_ok(const mvosr_height_pitch_eval_carry *c, const HecArgs &a) {
    return !c->halted && c->n_cases == a.n_cases && c->n_budgets == a.n_budgets;
}

__global__ __launch_bounds__(kHecBlock) void hpe_class_kernel(const HecArgs a) {
    const int f = blockIdx.x * kHecWaves + wave_id(), lane = lane_id();
    if (f >= a.n_frames || !hec_carry_ok(hec_header(a.carry_in), a)) return;         // (a whole wavefront; a halted call: nothing is written)
    const int32_t *st = a.in.status + (int64_t)f * a.n_elem;
    bool singular = false, mask = false, empty = false, unknown = false;
    int few = INT_MAX;                                                               // the smallest budget index with MVOSR_ST_RS_FEW
    for (int e = lane; e < a.n_elem; e += kWave) {
        const int s = st[e];
        singular |= s == MVOSR_ST_ERR_SINGULAR; mask |= s == MVOSR_ST_ERR_MASK; empty |= s == MVOSR_ST_ERR_EMPTY;
        if (s == MVOSR_ST_RS_FEW) few = min(few, e % a.n_budgets);
        unknown |= s != 0 && s != MVOSR_ST_HP_REFINE_DEGENERATE && s != MVOSR_ST_RS_FEW && s != MVOSR_ST_ERR_SINGULAR &&
                   s != MVOSR_ST_ERR_MASK && s != MVOSR_ST_ERR_EMPTY;
    }
    singular = __ballot(singular) != 0; mask = __ballot(mask) != 0; empty = __ballot(empty) != 0; unknown = __ballot(unknown) != 0;
    few = wave_min(few);
    if (lane != 0) return;
    const bool enough = a.in.n_selected[f] >= a.min_points;
    int cls;
    if (singular) cls = MVOSR_HPT_ERR_SINGULAR;
    else if (empty) cls = MVOSR_HPT_ERR_EMPTY;
    else if (mask) cls = MVOSR_HPT_ERR_MASK;
    else if (enough && few != INT_MAX) cls = MVOSR_HPT_ERR_NO_MODEL | (few << 8);
    else if (unknown) cls = MVOSR_HPT_ERR_STATUS;
    else cls = enough ? HEC_FIT : HEC_CARRY;
    a.out.frame_class[f] = cls;
}

__global__ __launch_bounds__(kHecBlock) void hpe_resolve_kernel(const HecArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *misc = reinterpret_cast<int *>(smem + hpeval_tail_plan<uint32_t>().misc);
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const mvosr_height_pitch_eval_carry *cin = hec_header(a.carry_in);
    if (!hec_carry_ok(cin, a)) {                                                     // an earlier chunk ended the call: nothing is final here
        if (tid == 0) *a.out.error = ((int64_t)MVOSR_HPT_ERR_UPSTREAM << 32);
        return;
    }
    const bool has_prev = cin->has_prev != 0;
    int run = -1;                                                                    // the last fitted frame of the rounds before
    long long first = LLONG_MAX;                                                     // the first error so far: frame << 16 | class
    for (int f0 = 0; f0 < a.n_frames; f0 += kHecBlock) {
        const int f = f0 + tid;
        const int cls = f < a.n_frames ? a.out.frame_class[f] : HEC_CARRY;
        // inclusive max-scan of "f where fitted": the lanes of a wavefront, then the wavefronts before it, then the rounds before
        int last = f < a.n_frames && cls == HEC_FIT ? f : -1;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) { const int up = __shfl_up(last, o); if (lane >= o) last = max(last, up); }
        if (lane == kWave - 1) misc[HEM_FIT + wave] = last;
        __syncthreads();
        for (int w = 0; w < wave; ++w) last = max(last, misc[HEM_FIT + w]);
        last = max(last, run);
        for (int w = 0; w < kHecWaves; ++w) run = max(run, misc[HEM_FIT + w]);
        if (f < a.n_frames) {
            int kind = cls > 0 ? cls : 0;
            if (cls == HEC_CARRY && last < 0 && !has_prev) kind = MVOSR_HPT_ERR_NO_PREVIOUS;     // :188
            if (kind) first = min(first, ((long long)f << 16) | kind);
            a.out.carried[f] = cls == HEC_CARRY ? 1 : 0;
            a.out.source[f] = last;
        }
        __syncthreads();                                                             // (misc is written again in the next round)
    }
    // the first error of the chunk: lanes, wavefronts
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) { const long long other = __shfl_xor(first, o); first = other < first ? other : first; }
    long long *slots = reinterpret_cast<long long *>(misc + HEM_ERR);
    if (lane == 0) slots[wave] = first;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kHecWaves; ++w) first = slots[w] < first ? slots[w] : first;
        *a.out.error = first == LLONG_MAX ? -1 : ((first >> 16) | ((first & 0xff) << 32) | (((first >> 8) & 0xff) << 40));
    }
}

// element e of a carry record: the eight doubles and the flag
struct HecEntry { double v[kHecCarryDoubles]; uint8_t degenerate; };

__device__ __forceinline__ HecEntry hec_load(const char *rec, int n_elem, int e) {
    const auto lay = hpeval_carry_plan<uint32_t>((uint32_t)n_elem);
    const double *val = reinterpret_cast<const double *>(rec + lay.value);
    HecEntry r;
#pragma unroll
    for (int k = 0; k < kHecCarryDoubles; ++k) r.v[k] = val[(int64_t)k * n_elem + e];
    r.degenerate = reinterpret_cast<const uint8_t *>(rec + lay.degenerate)[e];
    return r;
}

// ... stored, with the header (and the record's padding, zero) by the thread of element 0
__device__ __forceinline__ void hec_store(char *rec, const HecArgs &a, int e, const HecEntry &r, int has_prev, int halted) {
    const auto lay = hpeval_carry_plan<uint32_t>((uint32_t)a.n_elem);
    double *val = reinterpret_cast<double *>(rec + lay.value);
#pragma unroll
    for (int k = 0; k < kHecCarryDoubles; ++k) val[(int64_t)k * a.n_elem + e] = r.v[k];
    reinterpret_cast<uint8_t *>(rec + lay.degenerate)[e] = r.degenerate;
    if (e == 0) {
        mvosr_height_pitch_eval_carry *h = reinterpret_cast<mvosr_height_pitch_eval_carry *>(rec);
        h->has_prev = has_prev; h->halted = halted; h->n_cases = a.n_cases; h->n_budgets = a.n_budgets;
        for (uint32_t i = lay.degenerate + (uint32_t)a.n_elem; i < lay.total; ++i) rec[i] = 0;
    }
}

__global__ __launch_bounds__(kHecBlock) void hpe_apply_kernel(const HecArgs a) {
    const int f = blockIdx.x * kHecTileF + threadIdx.x, e = blockIdx.y * kHecTileE + threadIdx.y;
    const int F = a.n_frames, E = a.n_elem;
    if (e >= E) return;
    const mvosr_height_pitch_eval_carry *cin = hec_header(a.carry_in);
    const int64_t err = *a.out.error;
    const bool upstream = !hec_carry_ok(cin, a);
    const int end = upstream ? 0 : (err < 0 ? F : (int)(err & 0xffffffffll));        // frames before the first error: final
    const int halted = (upstream || err >= 0) ? 1 : 0;
    if (end == 0) {                                                                  // no final frame: the carry-in is the carry-out
        if (f == 0) {
            const bool same = cin->n_cases == a.n_cases && cin->n_budgets == a.n_budgets;   // (else the record has another size: not read)
            hec_store(a.carry_out, a, e, same ? hec_load(a.carry_in, E, e) : HecEntry{}, same ? cin->has_prev : 0, halted);
        }
        return;
    }
    if (f >= end) return;
    const int c = e / a.n_budgets, b = e - c * a.n_budgets;
    const int64_t o = ((int64_t)b * a.n_cases + c) * F + f;
    HecEntry r;
    int used = 0, best = -1;
    if (a.out.frame_class[f] == HEC_FIT) {
        const int64_t i = (int64_t)f * E + e;
        r.v[0] = a.in.ransac_height[i]; r.v[1] = a.in.refined_mean[i]; r.v[2] = a.in.refined_std[i]; r.v[3] = a.in.height_t_mean[i];
        r.v[4] = a.in.refined_pitch[i]; r.v[5] = (double)a.in.n_inliers[i]; r.v[6] = a.in.sum_y[i]; r.v[7] = a.in.sum_z[i];
        r.degenerate = (a.in.status[i] & MVOSR_ST_HP_REFINE_DEGENERATE) ? 1 : 0;
        if (a.in.used) used = a.in.used[i];
        if (a.in.best) best = a.in.best[i];
    } else {                                                                         // ---- a carried frame (:184-186, :223-224)
        const int g = a.out.source[f];                                               // its source; -1: the carry-in's
        if (g >= 0) {
            const int64_t i = (int64_t)g * E + e;
            r.v[0] = a.in.ransac_height[i]; r.v[1] = a.in.refined_mean[i]; r.v[2] = a.in.refined_std[i];
            r.v[4] = a.in.refined_pitch[i]; r.v[5] = (double)a.in.n_inliers[i]; r.v[6] = a.in.sum_y[i]; r.v[7] = a.in.sum_z[i];
            r.degenerate = (a.in.status[i] & MVOSR_ST_HP_REFINE_DEGENERATE) ? 1 : 0;
        } else r = hec_load(a.carry_in, E, e);
        const double sin_est = a.prior[4 * (int64_t)f + 2], cos_est = a.prior[4 * (int64_t)f + 3];
        r.v[3] = r.degenerate ? __longlong_as_double(0x7ff8000000000000ll)
                              : __ddiv_rn(__dadd_rn(__dmul_rn(r.v[7], sin_est), __dmul_rn(r.v[6], cos_est)), r.v[5]);
    }
    a.out.ransac_height[o] = r.v[0]; a.out.refined_mean[o] = r.v[1]; a.out.refined_std[o] = r.v[2]; a.out.height_t_mean[o] = r.v[3];
    a.out.refined_pitch[o] = r.v[4]; a.out.n_inliers[o] = r.v[5]; a.out.degenerate[o] = r.degenerate;
    if (a.out.used) a.out.used[o] = used;
    if (a.out.best) a.out.best[o] = best;
    if (f == end - 1) hec_store(a.carry_out, a, e, r, 1, halted);                    // the state after the last final frame
}

}  // namespace mvosr

using namespace mvosr;

extern "C" {

size_t mvosr_height_pitch_eval_carry_bytes(int n_cases, int n_budgets) {
    const size_t c = n_cases > 0 ? (size_t)n_cases : 0, b = n_budgets > 0 ? (size_t)n_budgets : 0;
    return hpeval_carry_plan<size_t>(c * b).total;
}

int mvosr_height_pitch_eval_tail_batch(mvosr_ctx *ctx, int64_t n_frames, int32_t n_cases, int32_t n_budgets, int32_t min_points,
                                       const mvosr_height_pitch_eval_tail_inputs *in, const double *frame_prior, const void *carry_in,
                                       void *carry_out, const mvosr_height_pitch_eval_tail_outputs *out) {
    if (!ctx || !in || !frame_prior || !carry_in || !carry_out || !out) return set_error(MVOSR_ERR_ARG, "height_pitch_eval_tail: null argument");
    if (!in->n_selected || !in->status || !in->ransac_height || !in->refined_mean || !in->refined_std || !in->height_t_mean ||
        !in->refined_pitch || !in->n_inliers || !in->sum_y || !in->sum_z)
        return set_error(MVOSR_ERR_ARG, "height_pitch_eval_tail: a required input is null");
    if (!out->ransac_height || !out->refined_mean || !out->refined_std || !out->height_t_mean || !out->refined_pitch || !out->n_inliers ||
        !out->degenerate || !out->carried || !out->frame_class || !out->source || !out->error)
        return set_error(MVOSR_ERR_ARG, "height_pitch_eval_tail: a required output is null");
    if ((out->used && !in->used) || (out->best && !in->best))
        return set_error(MVOSR_ERR_ARG, "height_pitch_eval_tail: used / best asked for without the launch's");
    if (carry_in == carry_out) return set_error(MVOSR_ERR_ARG, "height_pitch_eval_tail: the carry-in and the carry-out are the same record");
    if (n_cases < 1 || n_cases > kHecMaxCases) return set_error(MVOSR_ERR_ARG, "height_pitch_eval_tail: n_cases must be in 1..%d", kHecMaxCases);
    if (n_budgets < 1 || n_budgets > kHecMaxBudgets) return set_error(MVOSR_ERR_ARG, "height_pitch_eval_tail: n_budgets must be in 1..%d", kHecMaxBudgets);
    if (min_points < 3) return set_error(MVOSR_ERR_ARG, "height_pitch_eval_tail: min_points < 3");
    if (n_frames <= 0) return MVOSR_OK;
    if (n_frames >= INT32_MAX - kHecTileF) return set_error(MVOSR_ERR_TOO_LARGE, "height_pitch_eval_tail: 2^31 frames in one chunk");
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    HecArgs a = {};
    a.n_frames = (int32_t)n_frames; a.n_cases = n_cases; a.n_budgets = n_budgets; a.n_elem = n_cases * n_budgets; a.min_points = min_points;
    a.in = *in; a.prior = frame_prior; a.carry_in = static_cast<const char *>(carry_in); a.carry_out = static_cast<char *>(carry_out);
    a.out = *out;
    const unsigned class_groups = (unsigned)((n_frames + kHecWaves - 1) / kHecWaves);
    hipLaunchKernelGGL(hpe_class_kernel, dim3(class_groups), dim3(kHecBlock), 0, ctx_stream(ctx), a);
    rc = check_launch("hpe_class_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(hpe_resolve_kernel, dim3(1), dim3(kHecBlock), hpeval_tail_plan<size_t>().total, ctx_stream(ctx), a);
    rc = check_launch("hpe_resolve_kernel");
    if (rc) return rc;
    const dim3 grid((unsigned)((n_frames + kHecTileF - 1) / kHecTileF), (unsigned)((a.n_elem + kHecTileE - 1) / kHecTileE));
    hipLaunchKernelGGL(hpe_apply_kernel, grid, dim3(kHecTileF, kHecTileE), 0, ctx_stream(ctx), a);
    return check_launch("hpe_apply_kernel");
}

}  // extern "C"
