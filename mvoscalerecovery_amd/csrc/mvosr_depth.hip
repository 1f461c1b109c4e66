// mvosr_depth.hip — dense depth maps from the triangle planes (gfx950): what Reconstruct.triangle_model and
// Reconstruct.depth_generate of the reference compute (/root/reference/src/reconstruct.py:70-90, :91-117), as two device
// stages over a packed batch.
//
//   triangle_model_kernel — one workgroup per frame.  Per row of the frame's triangulation: the plane n.p = 1 through the
//     three features (plane_normal, the LU of the other kernels), height = 1/|n|, the unit normal, the sign rule (:83-85);
//     plus what the rasteriser wants of the row in one 64-byte record: its three pixel positions in ascending vertex
//     order (every edge is then evaluated from its lower to its higher vertex id: the two triangles of an edge see
//     exactly opposite values) and its bounding box clipped to the image.
//   depth_raster_kernel — one workgroup per (frame, band of image rows).  The band's triangle-id tile lives in LDS; the
//     wavefronts walk the frame's rows, skip those that miss the band, the lanes of a wavefront take the pixels of a hit's
//     clipped box and claim the ones inside with an LDS atomicMin (a pixel on a shared edge goes to the lowest row:
//     independent of scheduling); then ONE sweep writes the band — depth and, optionally, id — two adjacent pixels per
//     lane, 16 bytes per store, every byte exactly once, uncovered pixels as 0.0 / -1.  No global atomics on the image,
//     no memset pass, no read of the image.
//
// -ffp-contract=off as the rest: the edge functions must be the separately rounded products the CPU restatement
// (tests/depth_cases.py) forms, and the depth the reference's h / ((nx*px + ny*py) + nz) (:104).
#include "mvosr_device.hpp"
#include "mvosr_host.hpp"

namespace mvosr {

constexpr int kDpBlock = 256;
constexpr int kDpWaves = kDpBlock / kWave;
constexpr int kDpNone = 0x7fffffff;          // "no triangle" in the LDS tile (atomicMin's identity)
constexpr int kDpTileWords = 10240;          // 40 KB of ids per band: four workgroups per CU
constexpr int kDpMaxBandRows = 16;

struct DpRow {                               // 64 bytes per row of a triangulation
    double u0, v0, u1, v1, u2, v2;           // the vertices' pixels, ascending vertex id
    int x0, x1, y0, y1;                      // bounding box clipped to the image, inclusive; empty: y0 = INT_MAX, y1 = -1
};

struct DepthArgs {
    int64_t first_frame;
    const int64_t *feat_off; const int32_t *feat_cnt;
    const double *x, *y, *z, *u, *v;
    const int32_t *keep;
    const int64_t *tri_off; const int32_t *tri; const int32_t *tri_cnt;
    int width, height;
    double fx, fy, cx, cy;
    // context workspace: a frame's rows at twice its feature offset (a triangulation of n points has fewer than 2n rows)
    DpRow *rows; int2 *ybox; double4 *model; int32_t *map; int32_t *ntri;
    double *pxtab, *pytab;                   // the rays' (col - cx)/fx [width] and (row - cy)/fy [height]: one division per column / row, not per pixel
    double *tri_model; int32_t *status; int32_t *covered;
    double *depth; int32_t *tri_id;
    int band_rows, n_bands;
};

__global__ __launch_bounds__(kDpBlock) void triangle_model_kernel(const DepthArgs a) {
    __shared__ int s_wsum[2][kDpWaves];
    __shared__ int s_flag[2];
    const int64_t f = a.first_frame + blockIdx.x;
    const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
    const int n = max(a.feat_cnt[f], 0);
    const int64_t off = a.feat_off[f];
    const int64_t tb = a.tri_off[f];
    const int64_t tn64 = a.tri_cnt ? (int64_t)a.tri_cnt[f] : a.tri_off[f + 1] - tb;
    if (tid < 2) s_flag[tid] = 0;
    // the rows' ids are ranks among the kept points: map[rank] = position in the planes
    int m = n;
    if (a.keep) {
        int base = 0;
        for (int i0 = 0, it = 0; i0 < n; i0 += kDpBlock, ++it) {
            const int i = i0 + tid;
            const bool k = i < n && a.keep[off + i] >= 0;
            const unsigned long long bal = __ballot(k);
            if (lane == 0) s_wsum[it & 1][w] = __popcll(bal);
            __syncthreads();                                    // (two buffers: the next round's writes cannot overtake this round's reads)
            int before = 0, all = 0;
#pragma unroll
            for (int j = 0; j < kDpWaves; ++j) { const int c = s_wsum[it & 1][j]; before += j < w ? c : 0; all += c; }
            if (k) a.map[off + base + before + __popcll(bal & ((1ull << lane) - 1ull))] = i;
            base += all;
        }
        m = base;
        __threadfence_block();
    }
    __syncthreads();
    const bool fits = tn64 >= 0 && tn64 <= 2 * (int64_t)n;      // more rows than a triangulation of the frame's points can have
    const int tn = fits ? (int)tn64 : 0;
    const int64_t rb = 2 * off;
    const double wmax = (double)(a.width - 1), hmax = (double)(a.height - 1);
    int bad = fits ? 0 : 1, sing = 0;
    for (int t = tid; t < tn; t += kDpBlock) {
        const TriIds q = load_tri(a.tri + 3 * tb, t);
        DpRow r;
        r.u0 = r.v0 = r.u1 = r.v1 = r.u2 = r.v2 = 0.0;
        r.x0 = 1; r.x1 = 0; r.y0 = 0x7fffffff; r.y1 = -1;
        double4 md = make_double4(0.0, 0.0, 0.0, 0.0);
        if ((unsigned)q.a >= (unsigned)m || (unsigned)q.b >= (unsigned)m || (unsigned)q.c >= (unsigned)m) {
            bad = 1;
        } else {
            const int ia = a.keep ? a.map[off + q.a] : q.a, ib = a.keep ? a.map[off + q.b] : q.b, ic = a.keep ? a.map[off + q.c] : q.c;
            double nx, ny, nz;
            if (!plane_normal(a.x[off + ia], a.y[off + ia], a.z[off + ia], a.x[off + ib], a.y[off + ib], a.z[off + ib],
                              a.x[off + ic], a.y[off + ic], a.z[off + ic], nx, ny, nz)) sing = 1;          // reconstruct.py:78-79
            const double s = sqrt((nx * nx + ny * ny) + nz * nz);                                          // :80-81
            double h = 1.0 / s;                                                                            // :81
            nx = nx / s; ny = ny / s; nz = nz / s;                                                         // :82
            if (ny < 0.0) { nx = -nx; ny = -ny; nz = -nz; h = -h; }                                        // :83-85
            md = make_double4(nx, ny, nz, h);
            if (a.u) {
                // ascending vertex id (ranks and plane positions are in the same order)
                int i0 = ia, i1 = ib, i2 = ic;
                if (i0 > i1) { const int x = i0; i0 = i1; i1 = x; }
                if (i1 > i2) { const int x = i1; i1 = i2; i2 = x; }
                if (i0 > i1) { const int x = i0; i0 = i1; i1 = x; }
                r.u0 = a.u[off + i0]; r.v0 = a.v[off + i0];
                r.u1 = a.u[off + i1]; r.v1 = a.v[off + i1];
                r.u2 = a.u[off + i2]; r.v2 = a.v[off + i2];
                const double area = (r.u1 - r.u0) * (r.v2 - r.v0) - (r.v1 - r.v0) * (r.u2 - r.u0);        // edge (0,1) at vertex 2
                const double bx0 = fmax(ceil(fmin(fmin(r.u0, r.u1), r.u2)), 0.0), bx1 = fmin(floor(fmax(fmax(r.u0, r.u1), r.u2)), wmax);
                const double by0 = fmax(ceil(fmin(fmin(r.v0, r.v1), r.v2)), 0.0), by1 = fmin(floor(fmax(fmax(r.v0, r.v1), r.v2)), hmax);
                if ((area > 0.0 || area < 0.0) && bx0 <= bx1 && by0 <= by1) {       // (a flat or NaN row claims nothing)
                    r.x0 = (int)bx0; r.x1 = (int)bx1; r.y0 = (int)by0; r.y1 = (int)by1;
                }
            }
        }
        if (a.rows) { a.rows[rb + t] = r; a.ybox[rb + t] = make_int2(r.y0, r.y1); a.model[rb + t] = md; }
        if (a.tri_model) {
            double *o = a.tri_model + 4 * (tb + t);
            o[0] = md.x; o[1] = md.y; o[2] = md.z; o[3] = md.w;
        }
    }
    if (a.pxtab && blockIdx.x == 0) {                                              // (the camera is the batch's: the first workgroup writes the rays)
        for (int i = tid; i < a.width; i += kDpBlock) a.pxtab[i] = ((double)i - a.cx) / a.fx;          // reconstruct.py:32
        for (int i = tid; i < a.height; i += kDpBlock) a.pytab[i] = ((double)i - a.cy) / a.fy;         // :35
    }
    if (bad) s_flag[1] = 1;
    if (sing) s_flag[0] = 1;
    __syncthreads();
    if (tid == 0) {
        a.status[f] = s_flag[1] ? MVOSR_ST_ERR_MASK : (s_flag[0] ? MVOSR_ST_ERR_SINGULAR : ((n <= 0 || tn <= 0) ? MVOSR_ST_ERR_EMPTY : 0));
        if (a.ntri) a.ntri[f] = tn;
        if (a.covered) a.covered[f] = 0;
    }
}

__global__ __launch_bounds__(kDpBlock) void depth_raster_kernel(const DepthArgs a) {
    extern __shared__ __attribute__((aligned(16))) int tile[];
    __shared__ int s_cov[kDpWaves];
    const int band = (int)(blockIdx.x % (unsigned)a.n_bands);
    const int64_t f = a.first_frame + (int64_t)(blockIdx.x / (unsigned)a.n_bands);
    const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
    const int W = a.width;
    const int y_lo = band * a.band_rows, y_hi = min(y_lo + a.band_rows, a.height) - 1;
    const int npx = (y_hi - y_lo + 1) * W;
    for (int i = tid; i < npx; i += kDpBlock) tile[i] = kDpNone;
    __syncthreads();
    const int tn = a.ntri[f];
    const int64_t rb = 2 * a.feat_off[f];
    const DpRow *rows = a.rows + rb;
    const int2 *ybox = a.ybox + rb;
    // ---- claim: every wavefront takes 64 rows at a time; a row that meets the band is rasterised by the whole wavefront
    for (int t0 = w * kWave; t0 < tn; t0 += kDpBlock) {
        const int t = t0 + lane;
        bool hit = false;
        if (t < tn) { const int2 yb = ybox[t]; hit = yb.x <= y_hi && yb.y >= y_lo; }
        DpRow mine;                                       // every lane fetches its own hit: one trip to L2 for up to 64 records
        mine.u0 = mine.v0 = mine.u1 = mine.v1 = mine.u2 = mine.v2 = 0.0;
        mine.x0 = mine.x1 = mine.y0 = mine.y1 = 0;
        if (hit) mine = rows[t];
        unsigned long long todo = __ballot(hit);
        while (todo) {
            const int j = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
            const int tt = t0 + j;
            todo &= todo - 1ull;
            const double u0 = readlane_d(mine.u0, j), v0 = readlane_d(mine.v0, j), u1 = readlane_d(mine.u1, j), v1 = readlane_d(mine.v1, j),
                         u2 = readlane_d(mine.u2, j), v2 = readlane_d(mine.v2, j);
            const int x0 = __builtin_amdgcn_readlane(mine.x0, j), x1 = __builtin_amdgcn_readlane(mine.x1, j);
            const int by0 = max(__builtin_amdgcn_readlane(mine.y0, j), y_lo), bh = min(__builtin_amdgcn_readlane(mine.y1, j), y_hi) - by0 + 1;
            const int bw = x1 - x0 + 1;
            const int cnt = bw * bh;
            const double ax = u1 - u0, ay = v1 - v0, bx = u2 - u1, by = v2 - v1, cx = u2 - u0, cy = v2 - v0;
            const bool pos = (ax * cy - ay * cx) > 0.0;                            // the row's orientation: edge (0,1) at vertex 2
            const float rbw = 1.0f / (float)bw;
            int *trow = tile + (by0 - y_lo) * W + x0;
            for (int i = lane; i < cnt; i += kWave) {
                int yy, xx;
                divmod_small(i, bw, rbw, yy, xx);
                const double px = (double)(x0 + xx), py = (double)(by0 + yy);
                const double e01 = ax * (py - v0) - ay * (px - u0);                // each edge from its lower to its higher vertex id
                const double e12 = bx * (py - v1) - by * (px - u1);
                const double e02 = cx * (py - v0) - cy * (px - u0);
                // (sign * e >= 0 for the edges (0,1), (1,2) and (2,0) = -(0,2): with sign = -1 that is e <= 0, signed zeros included)
                const bool in = pos ? (e01 >= 0.0 && e12 >= 0.0 && e02 <= 0.0) : (e01 <= 0.0 && e12 <= 0.0 && e02 >= 0.0);
                if (in && (unsigned)xx < (unsigned)bw && (unsigned)yy < (unsigned)bh) atomicMin(trow + yy * W + xx, tt);
            }
        }
    }
    __syncthreads();
    // ---- sweep: the band is one flat range of the image; pairs are cut where the ADDRESS is 16-byte aligned
    const int64_t g0 = f * (int64_t)a.height * W + (int64_t)y_lo * W;
    double *dst = a.depth + g0;
    int32_t *idst = a.tri_id ? a.tri_id + g0 : nullptr;
    const int par = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1u);
    const int npairs = (npx + par + 1) >> 1;
    const double4 *model = a.model + rb;
    const float rW = 1.0f / (float)W;
    int cov = 0;
    auto depth_at = [&](int e, int id) -> double {
        int row, col;
        divmod_small(e, W, rW, row, col);
        const double px = a.pxtab[col], py = a.pytab[y_lo + row];                  // reconstruct.py:32, :35
        const double4 md = model[id];
        return md.w / ((md.x * px + md.y * py) + md.z);                            // :104
    };
    for (int k = tid; k < npairs; k += kDpBlock) {
        const int e0 = 2 * k - par, e1 = e0 + 1;
        const int id0 = e0 >= 0 ? tile[e0] : kDpNone;
        const int id1 = e1 < npx ? tile[e1] : kDpNone;
        double d0 = 0.0, d1 = 0.0;
        if (id0 != kDpNone) { d0 = depth_at(e0, id0); ++cov; }
        if (id1 != kDpNone) { d1 = depth_at(e1, id1); ++cov; }
        const int o0 = id0 != kDpNone ? id0 : -1, o1 = id1 != kDpNone ? id1 : -1;
        if (e0 >= 0 && e1 < npx) {
            *reinterpret_cast<double2 *>(dst + e0) = make_double2(d0, d1);
            if (idst) {
                if ((reinterpret_cast<uintptr_t>(idst + e0) & 7u) == 0) *reinterpret_cast<int2 *>(idst + e0) = make_int2(o0, o1);
                else { idst[e0] = o0; idst[e1] = o1; }
            }
        } else {
            if (e0 >= 0) { dst[e0] = d0; if (idst) idst[e0] = o0; }
            if (e1 < npx) { dst[e1] = d1; if (idst) idst[e1] = o1; }
        }
    }
    if (a.covered) {
        cov = wave_sum(cov);
        if (lane == 0) s_cov[w] = cov;
        __syncthreads();
        if (tid == 0) {
            int c = 0;
#pragma unroll
            for (int j = 0; j < kDpWaves; ++j) c += s_cov[j];
            if (c) atomicAdd(a.covered + f, c);                                    // (integers: the sum does not depend on the order)
        }
    }
}

static size_t dp_align(size_t x) { return (x + 255) & ~(size_t)255; }

// validate the batch side and fill the arguments both entry points share
static int dp_batch_args(const char *who, mvosr_ctx *ctx, const mvosr_batch *b, int which_tri, const int32_t *keep, DepthArgs &a) {
    if (!ctx || !b) return set_error(MVOSR_ERR_ARG, "%s: null argument", who);
    if (which_tri != 1 && which_tri != 2) return set_error(MVOSR_ERR_ARG, "%s: which_tri must be 1 or 2", who);
    const int64_t *toff = which_tri == 1 ? b->tri1_off : b->tri2_off;
    const int32_t *tri = which_tri == 1 ? b->tri1 : b->tri2;
    if (!b->feat_off || !b->feat_cnt || !b->x || !b->y || !b->z || !toff || !tri) return set_error(MVOSR_ERR_ARG, "%s: missing x/y/z/tri%d", who, which_tri);
    a.feat_off = b->feat_off; a.feat_cnt = b->feat_cnt; a.x = b->x; a.y = b->y; a.z = b->z; a.v = b->v;
    a.keep = keep; a.tri_off = toff; a.tri = tri; a.tri_cnt = which_tri == 1 ? b->tri1_cnt : b->tri2_cnt;
    return MVOSR_OK;
}

}  // namespace mvosr

using namespace mvosr;

extern "C" {

int mvosr_triangle_model_batch(mvosr_ctx *ctx, const mvosr_batch *b, int which_tri, const int32_t *keep, double *tri_model,
                               int32_t *status) {
    DepthArgs a = {};
    int rc = dp_batch_args("triangle_model", ctx, b, which_tri, keep, a);
    if (rc) return rc;
    if (!tri_model || !status) return set_error(MVOSR_ERR_ARG, "triangle_model: null output");
    if (b->n_frames <= 0) return MVOSR_OK;
    if ((rc = ctx_activate(ctx))) return rc;
    if (keep) {
        if (b->total_feat <= 0) return set_error(MVOSR_ERR_ARG, "triangle_model: total_feat is needed with keep");
        void *ws = nullptr;
        if ((rc = ctx_workspace_bytes(ctx, 4u * (size_t)b->total_feat + 256, &ws))) return rc;
        a.map = static_cast<int32_t *>(ws);
    }
    a.width = a.height = 1;
    a.tri_model = tri_model; a.status = status;
    hipLaunchKernelGGL(triangle_model_kernel, dim3((unsigned)b->n_frames), dim3(kDpBlock), 0, ctx_stream(ctx), a);
    return check_launch("triangle_model_kernel");
}

int mvosr_dense_depth_batch(mvosr_ctx *ctx, const mvosr_batch *b, int which_tri, const double *u, const int32_t *keep,
                            const mvosr_camera *cam, const mvosr_depth_outputs *o, int64_t first_frame, int64_t n_launch) {
    DepthArgs a = {};
    int rc = dp_batch_args("dense_depth", ctx, b, which_tri, keep, a);
    if (rc) return rc;
    if (!u || !b->v || !cam || !o) return set_error(MVOSR_ERR_ARG, "dense_depth: null argument (u, v, camera or outputs)");
    if (!o->depth || !o->status) return set_error(MVOSR_ERR_ARG, "dense_depth: depth and status are required outputs");
    if (cam->width < 1 || cam->height < 1) return set_error(MVOSR_ERR_ARG, "dense_depth: camera of %d x %d pixels", cam->width, cam->height);
    if (b->n_frames <= 0) return MVOSR_OK;
    if (n_launch <= 0) { first_frame = first_frame > 0 ? first_frame : 0; n_launch = b->n_frames - first_frame; }
    if (first_frame < 0 || n_launch <= 0 || first_frame + n_launch > b->n_frames) return set_error(MVOSR_ERR_ARG, "dense_depth: frame range outside the batch");
    if (b->total_feat <= 0) return set_error(MVOSR_ERR_ARG, "dense_depth: total_feat (the planes' length) sizes the workspace");
    if ((rc = ctx_activate(ctx))) return rc;
    // a band: an even number of image rows whose ids fit 40 KB of LDS (at least two rows, however wide the image)
    int band_rows = (kDpTileWords / cam->width) & ~1;
    band_rows = band_rows < 2 ? 2 : (band_rows > kDpMaxBandRows ? kDpMaxBandRows : band_rows);
    const size_t lds = 4u * (size_t)band_rows * (size_t)cam->width;
    if (lds + 64 > (size_t)ctx->max_lds_per_block)
        return set_error(MVOSR_ERR_TOO_LARGE, "dense_depth: two image rows of %d pixels need %zu B of LDS (> %d)", cam->width, lds, ctx->max_lds_per_block);
    const int64_t n_bands = ((int64_t)cam->height + band_rows - 1) / band_rows;
    if (n_launch * n_bands > 0x7fffffffll) return set_error(MVOSR_ERR_TOO_LARGE, "dense_depth: %lld frames x %lld bands in one launch", (long long)n_launch, (long long)n_bands);
    const size_t nrow = 2 * (size_t)b->total_feat;
    const size_t o_rows = 0, o_ybox = o_rows + dp_align(sizeof(DpRow) * nrow), o_model = o_ybox + dp_align(sizeof(int2) * nrow),
                 o_map = o_model + dp_align(sizeof(double4) * nrow), o_ntri = o_map + dp_align(4u * (size_t)b->total_feat),
                 o_px = o_ntri + dp_align(4u * (size_t)b->n_frames), o_py = o_px + dp_align(8u * (size_t)cam->width),
                 total = o_py + dp_align(8u * (size_t)cam->height);
    void *ws = nullptr;
    if ((rc = ctx_workspace_bytes(ctx, total, &ws))) return rc;
    char *base = static_cast<char *>(ws);
    a.rows = reinterpret_cast<DpRow *>(base + o_rows); a.ybox = reinterpret_cast<int2 *>(base + o_ybox);
    a.model = reinterpret_cast<double4 *>(base + o_model); a.map = reinterpret_cast<int32_t *>(base + o_map);
    a.ntri = reinterpret_cast<int32_t *>(base + o_ntri);
    a.pxtab = reinterpret_cast<double *>(base + o_px); a.pytab = reinterpret_cast<double *>(base + o_py);
    a.first_frame = first_frame; a.u = u;
    a.width = cam->width; a.height = cam->height; a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy;
    a.tri_model = o->tri_model; a.status = o->status; a.covered = o->covered; a.depth = o->depth; a.tri_id = o->tri_id;
    a.band_rows = band_rows; a.n_bands = (int)n_bands;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(depth_raster_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_hip_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    hipLaunchKernelGGL(triangle_model_kernel, dim3((unsigned)n_launch), dim3(kDpBlock), 0, ctx_stream(ctx), a);
    if ((rc = check_launch("triangle_model_kernel"))) return rc;
    hipLaunchKernelGGL(depth_raster_kernel, dim3((unsigned)(n_launch * n_bands)), dim3(kDpBlock), lds, ctx_stream(ctx), a);
    return check_launch("depth_raster_kernel");
}

}  // extern "C"
