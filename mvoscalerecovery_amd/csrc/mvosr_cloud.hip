// mvosr_cloud.hip — point clouds from the depth images, compacted on the device (gfx950): the last lines of
// Reconstruct.depth_generate of the reference (/root/reference/src/reconstruct.py:108-115) — every covered pixel becomes
// the point (px*d, py*d, d) with the image's colour, in raster order — as a stream compaction over a batch of depth images
// (DESIGN.md §3.9).
//
// A pixel (col, row) of frame f QUALIFIES when it is
//   covered          tri_id[f,row,col] >= 0 when an id image is given, else depth[f,row,col] != 0.0 (NaN counts as covered).
//                    The two rules differ only for a covered pixel whose depth is exactly +-0 — h / den with an infinite
//                    denominator, i.e. an infinite normal —: the id image keeps it, the depth image alone cannot see it;
//   on the grid      row % stride == 0 && col % stride == 0;
//   in range         (only with MVOSR_CLOUD_RANGE) dm >= near && dm <= far — NaN fails;
// dm = depth * scale[f] (ONE multiplication; none without scales).  Its point is (pxtab[col]*dm, pytab[row]*dm, dm),
// pxtab[col] = (col - cx)/fx, pytab[row] = (row - cy)/fy (:32, :35, :108, each operation rounded on its own:
// -ffp-contract=off), its colour (img[..,2], img[..,1], img[..,0]) / 255.0 (:110).
//
//   cloud_count_kernel — one workgroup per (frame, segment of kClSeg pixels of the frame's flat range): every wavefront
//     takes kClSpan consecutive pixels, 64 at a time; ballot + popcount; the segment's count goes to the workspace.
//   cloud_scan_kernel  — one workgroup per frame: exclusive prefix over the frame's segments, in place; the frame's
//     total; the LAST workgroup to arrive (an arrival counter: its order shows in nothing) turns the totals into
//     frame_off[F+1] and sets the overflow word.
//   cloud_fill_kernel  — the count kernel's grid again: the predicate re-evaluated, the values kept in registers, rank
//     in the wavefront from ballot + mbcnt, rank in the workgroup from the wavefronts' counts in LDS, rank in the batch
//     from the scan; rows written at frame_off[f] + base + rank, none at or beyond `capacity`.
// No atomics on the output, no host synchronisation, every output bit a function of the inputs.
#include "mvosr_device.hpp"
#include "mvosr_host.hpp"

namespace mvosr {

constexpr int kClBlock = 256;
constexpr int kClWaves = kClBlock / kWave;
constexpr int kClIters = 16;                        // loads in flight per lane
constexpr int kClSpan = kClIters * kWave;           // consecutive pixels of one wavefront
constexpr int kClSeg = kClWaves * kClSpan;          // 4096 pixels per workgroup
constexpr int kClMaxSide = 1 << 21;                 // divmod_small's range: col0 + kClSeg and the row stay below 2^22

struct CloudArgs {
    const double *depth; const int32_t *tri_id; const uint8_t *image; const double *scale;
    int width, height, npix, nseg, n_frames;
    double fx, fy, cx, cy, near, far;
    int stride, range;
    // context workspace
    int32_t *seg; int32_t *frame_tot; unsigned int *arrive; double *pxtab, *pytab;
    void *points; void *colors; int64_t *frame_off; int32_t *overflow; int64_t capacity;
};

// the segment of this workgroup: frame, first pixel, and that pixel's row and column
struct ClSeg { int64_t f; int sg, p0, row0, col0; };

__device__ __forceinline__ ClSeg cl_segment(const CloudArgs &a) {
    ClSeg s;
    s.f = (int64_t)(blockIdx.x / (unsigned)a.nseg);
    s.sg = (int)(blockIdx.x % (unsigned)a.nseg);
    s.p0 = s.sg * kClSeg;
    s.row0 = s.p0 / a.width;                        // (wave-uniform: one integer division per workgroup)
    s.col0 = s.p0 - s.row0 * a.width;
    return s;
}

// The predicate over the kClSpan pixels of wavefront `w`, 64 per round: bal[it] = the lanes whose pixel p0 + w*kClSpan + it*64 + lane
// qualifies, dm[it] = its (scaled) depth where VALUE or the range test needs it.  In three sweeps — grid, ids, depths — so
// that every load of a sweep is in flight before the first is waited for.
template <bool VALUE>
__device__ __forceinline__ void cl_span(const CloudArgs &a, const ClSeg &s, int w, int lane, double (&dm)[kClIters], unsigned long long (&bal)[kClIters]) {
    const float rW = 1.0f / (float)a.width, rS = 1.0f / (float)a.stride;
    const int64_t fb = s.f * (int64_t)a.npix + s.p0;
    const int j0 = w * kClSpan + lane;
    unsigned on = 0u;
#pragma unroll
    for (int it = 0; it < kClIters; ++it) {
        const int j = j0 + it * kWave;
        bool q = s.p0 + j < a.npix;
        if (a.stride > 1) {
            int dr, col, t, r0, r1;
            divmod_small(s.col0 + j, a.width, rW, dr, col);
            divmod_small(s.row0 + dr, a.stride, rS, t, r0);
            divmod_small(col, a.stride, rS, t, r1);
            q = q && r0 == 0 && r1 == 0;
        }
        on |= q ? 1u << it : 0u;
    }
    if (a.tri_id) {
        int id[kClIters];
#pragma unroll
        for (int it = 0; it < kClIters; ++it) id[it] = (on >> it) & 1u ? a.tri_id[fb + j0 + it * kWave] : -1;
#pragma unroll
        for (int it = 0; it < kClIters; ++it) on &= id[it] >= 0 ? ~0u : ~(1u << it);
    }
    const bool need = VALUE || a.range || !a.tri_id;
#pragma unroll
    for (int it = 0; it < kClIters; ++it) dm[it] = (need && ((on >> it) & 1u)) ? a.depth[fb + j0 + it * kWave] : 0.0;
    const double sc = a.scale ? a.scale[s.f] : 1.0;
#pragma unroll
    for (int it = 0; it < kClIters; ++it) {
        bool q = (on >> it) & 1u;
        if (!a.tri_id) q = q && dm[it] != 0.0;                                  // (NaN != 0: covered)
        if (a.scale) dm[it] = dm[it] * sc;
        if (a.range) q = q && dm[it] >= a.near && dm[it] <= a.far;             // (NaN fails)
        bal[it] = __ballot(q);
    }
}

__global__ __launch_bounds__(kClBlock) void cloud_count_kernel(const CloudArgs a) {
    __shared__ int s_cnt[kClWaves];
    const ClSeg s = cl_segment(a);
    const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
    if (blockIdx.x == 0) {                          // (the camera is the batch's: the first workgroup writes the rays and clears the scan's arrival counter)
        for (int i = tid; i < a.width; i += kClBlock) a.pxtab[i] = ((double)i - a.cx) / a.fx;           // reconstruct.py:32
        for (int i = tid; i < a.height; i += kClBlock) a.pytab[i] = ((double)i - a.cy) / a.fy;          // :35
        if (tid == 0) *a.arrive = 0u;
    }
    int cnt = 0;
    if (s.p0 + w * kClSpan < a.npix) {
        double dm[kClIters];
        unsigned long long bal[kClIters];
        cl_span<false>(a, s, w, lane, dm, bal);
#pragma unroll
        for (int it = 0; it < kClIters; ++it) cnt += __popcll(bal[it]);
    }
    if (lane == 0) s_cnt[w] = cnt;
    __syncthreads();
    if (tid == 0) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < kClWaves; ++j) c += s_cnt[j];
        a.seg[blockIdx.x] = c;
    }
}

// inclusive prefix over the wavefront's lanes
template <typename T>
__device__ __forceinline__ T cl_wave_incl(T v) {
    const int lane = lane_id();
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T o = __shfl_up(v, d, kWave);
        if (lane >= d) v += o;
    }
    return v;
}

// exclusive prefix of `c` over the workgroup's threads (in thread order) and the workgroup's total; `slot`: kClWaves values
template <typename T>
__device__ __forceinline__ T cl_block_excl(T c, T *slot, T &all) {
    const int lane = lane_id(), w = wave_id();
    const T incl = cl_wave_incl(c);
    if (lane == kWave - 1) slot[w] = incl;
    __syncthreads();
    T before = 0;
    all = 0;
#pragma unroll
    for (int j = 0; j < kClWaves; ++j) { const T t = slot[j]; before += j < w ? t : 0; all += t; }
    __syncthreads();                                // (the slot is written again by the next round)
    return before + incl - c;
}

__global__ __launch_bounds__(kClBlock) void cloud_scan_kernel(const CloudArgs a) {
    __shared__ int s_i[kClWaves];
    __shared__ long long s_l[kClWaves];
    __shared__ int s_last;
    const int f = blockIdx.x, tid = threadIdx.x;
    int32_t *seg = a.seg + (int64_t)f * a.nseg;
    int base = 0;                                   // (a frame has fewer than 2^31 pixels)
    for (int i0 = 0; i0 < a.nseg; i0 += kClBlock) {
        const int i = i0 + tid;
        const int c = i < a.nseg ? seg[i] : 0;
        int all;
        const int ex = cl_block_excl<int>(c, s_i, all);
        if (i < a.nseg) seg[i] = base + ex;
        base += all;
    }
    if (tid == 0) __hip_atomic_store(a.frame_tot + f, base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(a.arrive, 1u) == (unsigned)(a.n_frames - 1);
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    long long run = 0;
    for (int i0 = 0; i0 < a.n_frames; i0 += kClBlock) {
        const int i = i0 + tid;
        const long long c = i < a.n_frames ? (long long)__hip_atomic_load(a.frame_tot + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        long long all;
        const long long ex = cl_block_excl<long long>(c, s_l, all);
        if (i < a.n_frames) a.frame_off[i] = run + ex;
        run += all;
    }
    if (tid == 0) {
        a.frame_off[a.n_frames] = run;
        if (a.overflow) *a.overflow = run > a.capacity ? 1 : 0;
        *a.arrive = 0u;
    }
}

template <typename T>
__global__ __launch_bounds__(kClBlock) void cloud_fill_kernel(const CloudArgs a) {
    __shared__ int s_cnt[kClWaves];
    const ClSeg s = cl_segment(a);
    const int lane = lane_id(), w = wave_id();
    const float rW = 1.0f / (float)a.width;
    double dm[kClIters];
    unsigned long long bal[kClIters];
    int cnt = 0;
    if (s.p0 + w * kClSpan < a.npix) {
        cl_span<true>(a, s, w, lane, dm, bal);
#pragma unroll
        for (int it = 0; it < kClIters; ++it) cnt += __popcll(bal[it]);
    }
    if (lane == 0) s_cnt[w] = cnt;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int j = 0; j < kClWaves; ++j) before += j < w ? s_cnt[j] : 0;
    if (!cnt) return;
    int64_t at = a.frame_off[s.f] + (int64_t)a.seg[blockIdx.x] + before;
    T *pts = static_cast<T *>(a.points), *cols = static_cast<T *>(a.colors);
    const uint8_t *img = a.image ? a.image + 3 * s.f * (int64_t)a.npix : nullptr;
#pragma unroll
    for (int it = 0; it < kClIters; ++it) {
        const unsigned long long b = bal[it];
        if (!b) continue;
        const int64_t k = at + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
        if (((b >> lane) & 1ull) && k < a.capacity) {
            const int j = w * kClSpan + it * kWave + lane;
            int dr, col;
            divmod_small(s.col0 + j, a.width, rW, dr, col);
            const double d = dm[it];
            T *o = pts + 3 * k;
            o[0] = (T)(a.pxtab[col] * d);                                          // reconstruct.py:108
            o[1] = (T)(a.pytab[s.row0 + dr] * d);
            o[2] = (T)d;
            if (cols) {
                const uint8_t *c = img + 3 * (int64_t)(s.p0 + j);
                T *oc = cols + 3 * k;
                oc[0] = (T)((double)c[2] / 255.0);                                 // :110 (BGR -> RGB)
                oc[1] = (T)((double)c[1] / 255.0);
                oc[2] = (T)((double)c[0] / 255.0);
            }
        }
        at += __popcll(b);
    }
}

static size_t cl_align(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace mvosr

using namespace mvosr;

extern "C" {

int mvosr_point_cloud_batch(mvosr_ctx *ctx, const mvosr_cloud_inputs *in, const mvosr_camera *cam, const mvosr_cloud_params *p,
                            const mvosr_cloud_outputs *o) {
    if (!ctx || !in || !cam || !p || !o) return set_error(MVOSR_ERR_ARG, "point_cloud: null argument (ctx, inputs, camera, params or outputs)");
    if (!in->depth || !o->frame_off) return set_error(MVOSR_ERR_ARG, "point_cloud: depth and frame_off are required");
    if (p->stride < 1) return set_error(MVOSR_ERR_ARG, "point_cloud: stride %d (must be >= 1)", p->stride);
    if (o->colors && !in->image) return set_error(MVOSR_ERR_ARG, "point_cloud: colours asked for without an image");
    if (o->capacity < 0) return set_error(MVOSR_ERR_ARG, "point_cloud: negative capacity");
    if (o->capacity > 0 && !o->points) return set_error(MVOSR_ERR_ARG, "point_cloud: capacity %lld without a points buffer", (long long)o->capacity);
    if (in->n_frames < 0) return set_error(MVOSR_ERR_ARG, "point_cloud: negative frame count");
    if (cam->width < 1 || cam->height < 1) return set_error(MVOSR_ERR_ARG, "point_cloud: camera of %d x %d pixels", cam->width, cam->height);
    if (in->n_frames == 0) return MVOSR_OK;
    const int64_t npix = (int64_t)cam->width * cam->height;
    const int64_t nseg = (npix + kClSeg - 1) / kClSeg;
    if (cam->width > kClMaxSide || cam->height > kClMaxSide || npix > 0x7fffffffll - kClSeg || in->n_frames * nseg > 0x7fffffffll)
        return set_error(MVOSR_ERR_TOO_LARGE, "point_cloud: %lld frames of %d x %d pixels in one launch", (long long)in->n_frames, cam->width, cam->height);
    int rc = ctx_activate(ctx);
    if (rc) return rc;
    const size_t F = (size_t)in->n_frames;
    const size_t o_seg = 0, o_tot = o_seg + cl_align(4u * F * (size_t)nseg), o_arr = o_tot + cl_align(4u * F), o_px = o_arr + 256,
                 o_py = o_px + cl_align(8u * (size_t)cam->width), total = o_py + cl_align(8u * (size_t)cam->height);
    void *ws = nullptr;
    if ((rc = ctx_workspace_bytes(ctx, total, &ws))) return rc;
    char *base = static_cast<char *>(ws);
    CloudArgs a = {};
    a.depth = in->depth; a.tri_id = in->tri_id; a.image = o->colors ? in->image : nullptr; a.scale = in->scale;
    a.width = cam->width; a.height = cam->height; a.npix = (int)npix; a.nseg = (int)nseg; a.n_frames = (int)in->n_frames;
    a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy; a.near = p->near; a.far = p->far;
    a.stride = p->stride; a.range = (p->flags & MVOSR_CLOUD_RANGE) ? 1 : 0;
    a.seg = reinterpret_cast<int32_t *>(base + o_seg); a.frame_tot = reinterpret_cast<int32_t *>(base + o_tot);
    a.arrive = reinterpret_cast<unsigned int *>(base + o_arr);
    a.pxtab = reinterpret_cast<double *>(base + o_px); a.pytab = reinterpret_cast<double *>(base + o_py);
    a.points = o->points; a.colors = o->colors; a.frame_off = o->frame_off; a.overflow = o->overflow; a.capacity = o->capacity;
    const dim3 grid((unsigned)(in->n_frames * nseg)), block(kClBlock);
    hipLaunchKernelGGL(cloud_count_kernel, grid, block, 0, ctx_stream(ctx), a);
    if ((rc = check_launch("cloud_count_kernel"))) return rc;
    hipLaunchKernelGGL(cloud_scan_kernel, dim3((unsigned)in->n_frames), block, 0, ctx_stream(ctx), a);
    if ((rc = check_launch("cloud_scan_kernel"))) return rc;
    if (o->capacity == 0) return MVOSR_OK;          // (a counting call: frame_off and the overflow word only)
    if (p->flags & MVOSR_CLOUD_F32) hipLaunchKernelGGL(cloud_fill_kernel<float>, grid, block, 0, ctx_stream(ctx), a);
    else hipLaunchKernelGGL(cloud_fill_kernel<double>, grid, block, 0, ctx_stream(ctx), a);
    return check_launch("cloud_fill_kernel");
}

}  // extern "C"
