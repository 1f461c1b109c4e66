// mvosr_rescale_sweep.hip — flat_selection (/root/reference/src/rescale.py:75-102) for S settings of its three constants in one
// launch.
//
// The reference's author moved these numbers by hand: the two pitch thresholds stand in two spellings (rescale.py:85-96,
// rescale_test.py:132-150), the factor of the height level at :91.  None of the stages in front of the selection reads them, so
// a sweep over them re-uses both triangulations and the vote.  flat_selection_sweep_kernel reads what flat_selection_kernel<true>
// (mvosr_flat_ransac_batch) reads — the survivors compacted by keep >= 0 in order, the second triangulation's rows with their
// counts, dt_status — and runs one frame per workgroup:
//
//   once per frame: every row's (mu, height) by flat_row, and from mu the row's two bits for every setting by flat_row_bits —
//   the functions flat_selection_kernel's phase 1 calls (mvosr_flat.hpp);
//   per setting, one wavefront each: the median of the loose rows' heights as np.median takes it — the two middle order
//   statistics by an 8-bit radix select over the heights' patterns, a histogram per wavefront where the vertex planes were —,
//   the level, bit 2, and the setting's flag plane.
//
// An order statistic does not depend on how it is searched for, and the level is written as flat_selection_kernel writes it, so
// every setting's flags, level and count equal mvosr_flat_selection_batch's with that setting's constants, bit for bit.
// fp64, compiled with -ffp-contract=off; no floating-point atomics; the flag planes are written with plain byte stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mvosr.h"
#include "mvosr_device.hpp"
#include "mvosr_ransac.hpp"
#include "mvosr_flat.hpp"
#include "mvosr_host.hpp"
#include "mvosr_rescale_sweep_plan.hpp"

namespace mvosr {

struct SweepArgs {
    int64_t n_frames;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *x, *y, *z;
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    const int32_t *keep;           // [like x] a feature takes part iff keep[i] >= 0 (null: all)
    const int32_t *dt_status;      // [F] non-zero: declined triangulation, frame skipped (null: none)
    int64_t total_feat;            // with tri_cnt: a flag plane holds 2 * total_feat rows
    int32_t n_sel, max_feat, max_tri;
    double loose_deg[kSweepMaxSel], tight_deg[kSweepMaxSel], height_factor[kSweepMaxSel];
    uint8_t *tri_flags;            // [S][rows] bit0: pitch < loose_s, bit1: pitch < tight_s, bit2: kept
    double *height_level;          // [F][S]
    int32_t *n_kept;               // [F][S]
    int32_t *status;               // [F] 0 / MVOSR_ST_ERR_SINGULAR / MVOSR_ST_ERR_MASK / MVOSR_ST_ERR_EMPTY
    double *tri_height;            // optional [rows] 1/|n|
};

// LDS instructions of a wavefront execute in order: only the compiler must keep the order (as in mvosr_featdist.hip)
__device__ __forceinline__ void sweep_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The pattern of rank `rank` (0-based, ascending) among the rows whose word has the bit `lb`: eight bits a pass from the top, the
// calling wavefront alone, through its own histogram.  Every lane returns it.
__device__ __forceinline__ unsigned long long sweep_select(const unsigned long long *U, const uint32_t *B, uint32_t lb, int tn, int rank,
                                                           int *hist) {
    static_assert(kSweepBins == 4 * kWave, "sweep_select: four bins per lane");
    const int lane = lane_id();
    unsigned long long prefix = 0ull;
    for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) hist[lane + j * kWave] = 0;
        sweep_lds_sync();
        const int up = shift + 8;
        for (int t = lane; t < tn; t += kWave) {
            if (!(B[t] & lb)) continue;
            const unsigned long long u = U[t];
            if (up >= 64 || ((u ^ prefix) >> (up & 63)) == 0ull) atomicAdd(&hist[(int)((u >> shift) & 255ull)], 1);
        }
        sweep_lds_sync();
        const int b0 = hist[4 * lane], b1 = hist[4 * lane + 1], b2 = hist[4 * lane + 2], b3 = hist[4 * lane + 3];
        const int mine = (b0 + b1) + (b2 + b3);
        const int incl = wave_scan_incl(mine), excl = incl - mine;
        // (the rank lies inside the rows that share the prefix: exactly one lane answers)
        int r = rank - excl, bin = 4 * lane;
        if (r >= b0) { r -= b0; ++bin; if (r >= b1) { r -= b1; ++bin; if (r >= b2) { r -= b2; ++bin; } } }
        const int src = max(__ffsll((long long)__ballot(rank >= excl && rank < incl)) - 1, 0);
        bin = __shfl(bin, src);
        rank = __shfl(r, src);
        prefix |= (unsigned long long)bin << shift;
        sweep_lds_sync();                                        // (the bins have been read: the next pass zeroes them)
    }
    return prefix;
}

template <int WAVES>
__global__ __launch_bounds__(WAVES *kWave) void flat_selection_sweep_kernel(const SweepArgs a) {
    constexpr int BLK = WAVES * kWave;
    static_assert(WAVES <= kSweepWaves, "flat_selection_sweep_kernel: per-wave slots in misc, histograms in the plan");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t f = blockIdx.x;
    const int S = a.n_sel;
    const int n_all = a.feat_cnt[f];
    const int64_t off = a.feat_off[f];
    const int64_t tb = a.tri_off[f];
    const int tn = a.tri_cnt ? a.tri_cnt[f] : (int)(a.tri_off[f + 1] - tb);
    // rows of a flag plane: the batch's rows (the form with explicit counts gives a frame room for twice its features)
    const int64_t plane_rows = a.tri_cnt ? 2 * a.total_feat : a.tri_off[a.n_frames];
    const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const bool skip = a.dt_status && a.dt_status[f] != 0;
    // more features or rows than the launch's LDS was sized for, or rows that do not lie inside a plane: refused, LDS untouched
    const bool oversize = n_all > a.max_feat || tn > a.max_tri || tb < 0 || tb + tn > plane_rows;
    if (const int refused = flat_entry_status(n_all, tn, skip, oversize)) {
        if (tid == 0) a.status[f] = refused;
        for (int s = tid; s < S; s += BLK) { a.height_level[f * S + s] = nan(""); a.n_kept[f * S + s] = 0; }
        return;
    }
    const auto lds = sweep_plan<uint32_t>((uint32_t)n_all, (uint32_t)tn, (uint32_t)S);
    double *Hh = reinterpret_cast<double *>(smem + lds.heights);
    const unsigned long long *U = reinterpret_cast<const unsigned long long *>(Hh);
    uint32_t *B = reinterpret_cast<uint32_t *>(smem + lds.bits);
    int *misc = reinterpret_cast<int *>(smem + lds.misc);
    double *thr = reinterpret_cast<double *>(smem + lds.thr);
    double *X = reinterpret_cast<double *>(smem + lds.x);
    double *Y = reinterpret_cast<double *>(smem + lds.y);
    double *Z = reinterpret_cast<double *>(smem + lds.z);
    if (tid < SM_CW) misc[tid] = 0;
    if (tid < S) {
        thr[tid] = flat_sin_deg(a.loose_deg[tid]);
        thr[S + tid] = flat_sin_deg(a.tight_deg[tid]);
    }
    // ---- the survivors, compacted in order (rescale.py:134-135)
    const int n = flat_compact_survivors<WAVES>(n_all, a.keep ? a.keep + off : nullptr, a.x + off, a.y + off, a.z + off, X, Y, Z, misc + SM_CW);
    __syncthreads();
    // ---- phase 1: every row's height and, per setting, its two bits (rescale.py:79-89)
    {
        int bad = 0, singular = 0;
        for (int t = tid; t < tn; t += BLK) {
            const FlatRow r = flat_row(X, Y, Z, load_tri(a.tri + 3 * tb, t), n);
            uint32_t bits = 0u;
            if (r.bad_id) bad = 1;
            else {
                if (r.singular) singular = 1;
                for (int s = 0; s < S; ++s) bits |= flat_row_bits(r.mu, thr[s], thr[S + s], a.loose_deg[s], a.tight_deg[s]) << (2 * s);
            }
            Hh[t] = r.h;
            B[t] = bits;
            if (a.tri_height) a.tri_height[tb + t] = r.h;
        }
        if (bad) misc[SM_BADID] = 1;
        if (singular) misc[SM_SINGULAR] = 1;
    }
    __syncthreads();                                             // (the planes are dead: their room is the histograms')
    // ---- phase 2: a setting per wavefront — the level (:91) and the kept rows (:94-96)
    int *hist = reinterpret_cast<int *>(smem + lds.hist) + wave * kSweepBins;
    for (int s = wave; s < S; s += WAVES) {
        const uint32_t lb = 1u << (2 * s);
        int k = 0;
        for (int t = lane; t < tn; t += kWave) k += (B[t] & lb) ? 1 : 0;
        k = wave_sum(k);
        double level = nan("");                                  // median of an empty set is nan (nothing passes)
        if (k > 0) {                                             // np.median, :91
            const int klo = (k - 1) >> 1, khi = k >> 1;
            const unsigned long long vlo_bits = sweep_select(U, B, lb, tn, klo, hist);
            const double vlo = __longlong_as_double((long long)vlo_bits);
            double vhi = vlo;
            if (khi != klo) {
                int le = 0;
                unsigned long long above = ~0ull;
                for (int t = lane; t < tn; t += kWave) {
                    if (!(B[t] & lb)) continue;
                    const unsigned long long u = U[t];
                    if (u <= vlo_bits) ++le; else above = u < above ? u : above;
                }
                le = wave_sum(le);
                above = wave_min_u64(above);
                vhi = __longlong_as_double((long long)(le < khi + 1 ? above : vlo_bits));
            }
            level = a.height_factor[s] * ((klo == khi) ? vlo : (vlo + vhi) / 2.0);
        }
        uint8_t *out = a.tri_flags + (int64_t)s * plane_rows + tb;
        int kept = 0;
        for (int t = lane; t < tn; t += kWave) {
            uint8_t fl = (uint8_t)((B[t] >> (2 * s)) & 3u);
            if ((fl & 2) && Hh[t] > level) { fl |= 4; ++kept; }                              // :94-96
            out[t] = fl;
        }
        kept = wave_sum(kept);
        if (lane == 0) { a.height_level[f * S + s] = level; a.n_kept[f * S + s] = kept; }
    }
    if (tid == 0) a.status[f] = misc[SM_BADID] ? MVOSR_ST_ERR_MASK : (misc[SM_SINGULAR] ? MVOSR_ST_ERR_SINGULAR : 0);
}

}  // namespace mvosr

using namespace mvosr;

extern "C" {

int mvosr_flat_selection_sweep_max_settings(void) { return kSweepMaxSel; }

size_t mvosr_flat_selection_sweep_lds_bytes(int max_feat, int64_t max_tri, int n_sel) {
    const size_t mf = max_feat > 0 ? (size_t)max_feat : 0;
    const size_t mt = max_tri > 0 ? (size_t)max_tri : 2 * mf;
    return sweep_plan<size_t>(mf, mt, n_sel > 0 ? (size_t)n_sel : 0).total;
}

int mvosr_flat_selection_sweep_batch(mvosr_ctx *ctx, const mvosr_batch *b, const int32_t *keep, const int32_t *dt_status, int32_t n_sel,
                                     const double *loose_deg, const double *tight_deg, const double *height_factor, uint8_t *tri_flags,
                                     double *height_level, int32_t *n_kept, int32_t *status, double *tri_height, int64_t max_tri) {
    if (!ctx || !b || !loose_deg || !tight_deg || !height_factor || !tri_flags || !height_level || !n_kept || !status)
        return set_error(MVOSR_ERR_ARG, "flat_selection_sweep: null argument");
    if (!b->feat_off || !b->feat_cnt || !b->x || !b->y || !b->z || !b->tri2_off || !b->tri2) return set_error(MVOSR_ERR_ARG, "flat_selection_sweep: missing x/y/z/tri2");
    if (n_sel < 1 || n_sel > kSweepMaxSel) return set_error(MVOSR_ERR_ARG, "flat_selection_sweep: n_sel must be in 1..%d", kSweepMaxSel);
    if (b->max_feat < 0) return set_error(MVOSR_ERR_ARG, "flat_selection_sweep: max_feat < 0");
    if (b->tri2_cnt && b->total_feat < 0) return set_error(MVOSR_ERR_ARG, "flat_selection_sweep: total_feat < 0");
    if (b->n_frames <= 0) return MVOSR_OK;
    if (b->n_frames > (int64_t)0x7fffffff) return set_error(MVOSR_ERR_TOO_LARGE, "flat_selection_sweep: frames exceed a grid");
    if (max_tri <= 0) max_tri = 2 * (int64_t)b->max_feat;
    if (max_tri > INT32_MAX / 8) return set_error(MVOSR_ERR_TOO_LARGE, "flat_selection_sweep: eight times max_tri does not fit 32 bits");
    const size_t lds = sweep_plan<size_t>((size_t)b->max_feat, (size_t)max_tri, (size_t)n_sel).total;
    if ((int64_t)lds > (int64_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_TOO_LARGE, "flat_selection_sweep: a frame of %d features and %lld rows needs %zu B of LDS (> %d)", b->max_feat,
                         (long long)max_tri, lds, ctx->max_lds_per_block);
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(flat_selection_sweep_kernel<kSweepWaves>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    SweepArgs a = {};
    a.n_frames = b->n_frames; a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.x = b->x; a.y = b->y; a.z = b->z;
    a.tri_off = b->tri2_off; a.tri = b->tri2; a.tri_cnt = b->tri2_cnt;
    a.keep = keep; a.dt_status = dt_status; a.total_feat = b->total_feat;
    a.n_sel = n_sel; a.max_feat = b->max_feat; a.max_tri = (int32_t)max_tri;
    for (int s = 0; s < n_sel; ++s) { a.loose_deg[s] = loose_deg[s]; a.tight_deg[s] = tight_deg[s]; a.height_factor[s] = height_factor[s]; }
    a.tri_flags = tri_flags; a.height_level = height_level; a.n_kept = n_kept; a.status = status; a.tri_height = tri_height;
    hipLaunchKernelGGL(flat_selection_sweep_kernel<kSweepWaves>, dim3((unsigned)b->n_frames), dim3(kSweepWaves * kWave), lds, ctx_stream(ctx), a);
    return check_launch("flat_selection_sweep_kernel");
}

}  // extern "C"
