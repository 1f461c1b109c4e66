/*
 * mvosr.h — C ABI of libmvosr.so: MI355X (gfx950) kernels for the per-frame scale-recovery hot
 * path of TimingSpace/MVOScaleRecovery.
 *
 * The reference is pure Python and has no FFI/plugin registry: the drop-in boundary is the
 * Python class `ScaleEstimator` chosen by an import line (/root/reference/src/main.py:18-20,
 * /root/reference/src/main_offline.py:18-20).  mvoscalerecovery_amd/scale_calculator.py keeps
 * that class surface and binds the entry points below with ctypes (see INTEGRATION.md for the
 * stub).  Each entry point cites the reference routine whose per-frame work it replaces; all of
 * them process a BATCH of independent frames, one workgroup (or one wavefront for small
 * frames) per frame.
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer inside mvosr_batch / mvosr_outputs is a DEVICE
 *     pointer (hipMalloc'ed by mvosr_malloc, or e.g. torch.Tensor.data_ptr()); the structs
 *     themselves live in host memory and are read during the call;
 *   - every function returns 0 on success, a negative mvosr_err on failure, never throws;
 *     mvosr_last_error() returns a thread-local message;
 *   - launches are asynchronous on the context's HIP stream; call mvosr_ctx_sync() (or
 *     synchronise the adopted stream yourself) before reading outputs;
 *   - all floating-point data is IEEE binary64 (the reference computes in NumPy float64 and
 *     its result is a quantised histogram mode, so threshold decisions must match bit-for-bit:
 *     SURVEY.md fact 5); triangle vertex ids are int32 exactly as scipy.spatial.Delaunay
 *     emits `simplices` (row-major (T,3); the order of vertices inside a row matters,
 *     /root/reference/src/scale_calculator.py:113-115).
 */
#ifndef MVOSR_H
#define MVOSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVOSR_ABI_VERSION 13
/* (mvosr_point_cloud_batch and its three structs were added WITHOUT raising this number: the change is purely additive —
 * no existing struct or signature moved — and a binding resolves every symbol it declares when it loads the library, so a
 * library older than its binding fails loudly at load time anyway.  mvosr_height_pitch_batch, its two structs and
 * mvosr_height_pitch_lds_bytes were added the same way, and so were mvosr_height_pitch_tail_batch, its two records and its two
 * size functions, and mvosr_height_pitch_eval_tail_batch with its record, its two structs and its size function.) */

/* error codes (function return values) */
enum mvosr_err {
    MVOSR_OK = 0,
    MVOSR_ERR_HIP = -1,          /* a HIP runtime call failed (message has hipGetErrorString) */
    MVOSR_ERR_ARG = -2,          /* bad argument (null pointer, negative size, ...) */
    MVOSR_ERR_TOO_LARGE = -3,    /* a frame does not fit the requested kernel variant */
    MVOSR_ERR_NO_DEVICE = -4,    /* no gfx950 device visible */
    MVOSR_ERR_ALLOC = -5         /* device memory for a grow-only workspace could not be allocated (the triangulation kernels'
                                    per-frame arrays): nothing was launched; the caller may retry with fewer frames or take its host path */
};

/* per-frame status codes written to mvosr_outputs.status.  0-3 are the reference's normal
 * return branches, 4 its "no enough flat feature" fallback, 5-7 the places where the reference
 * raises; the Python shim maps them back to return-or-raise. */
enum mvosr_status {
    MVOSR_ST_MODE = 0,          /* height = mode/10               scale_calculator.py:354     */
    MVOSR_ST_RIGHT = 1,         /* skew > 0.3: right minimum edge scale_calculator.py:348-352 */
    MVOSR_ST_MEDIAN = 2,        /* no modes: median(y)            scale_calculator.py:331-333 */
    MVOSR_ST_LEVEL = 3,         /* no modes, no points: height_level          :334-335        */
    MVOSR_ST_NO_FLAT = 4,       /* selection empty: scale = ref/height_level  :277-279,:420-422 */
    MVOSR_ST_ERR_LEFT = 5,      /* IndexError at scale_calculator.py:343 */
    MVOSR_ST_ERR_RIGHT = 6,     /* IndexError at scale_calculator.py:344 */
    MVOSR_ST_ERR_SINGULAR = 7,  /* LinAlgError at scale_calculator.py:229 */
    MVOSR_ST_ERR_MASK = 8,      /* tri2 inconsistent with the vote computed on the GPU, or a
                                   vertex id out of range (build-side check, no reference analogue) */
    MVOSR_ST_ERR_EMPTY = 9,     /* frame without triangles, or with fewer than 3 features below the vanishing row (where the
                                   reference's first Delaunay call raises QhullError, :257: the caller must raise) */
    MVOSR_ST_TOO_FEW = 10,      /* exactly 3 features below the vanishing row: the reference skips the second
                                   triangulation (:263-270) and divides by the PREVIOUS frame's height_level
                                   (:420-422, std 100); raw_scale/height_level are NaN here and the host's
                                   cross-frame step supplies that level */
    MVOSR_ST_RS_FEW = 11        /* rescale variant: fewer than 12 selected points — no RANSAC, the previous scale is pushed
                                   again (/root/reference/src/rescale.py:152,175); raw_scale is NaN */
};

/* number of int32 per frame in mvosr_outputs.counts */
#define MVOSR_N_COUNTS 8
enum mvosr_count_slot {
    MVOSR_CNT_VALID = 0,        /* features with vote counter >= 0            (:164-166) */
    MVOSR_CNT_TRI_PITCH = 1,    /* triangles with pitch_deg < -80             (:235)     */
    MVOSR_CNT_TRI_VALID = 2,    /* ... and mean height > height_level         (:243-244); -1 where the tiled
                                   dense variant ran (it keeps per-vertex maxima, not per-triangle flags) */
    MVOSR_CNT_SELECTED = 3,     /* unique vertices of those triangles         (:247)     */
    MVOSR_CNT_KEPT = 4,         /* selected points left after remove_single   (:284-293) */
    MVOSR_CNT_MODES = 5,        /* number of mode clusters                    (:468-481) */
    MVOSR_CNT_MODE_LEFT = 6,    /* mode_left  (:339), -1 if none */
    MVOSR_CNT_MODE_RIGHT = 7    /* mode_right (:338), -1 if none */
};

#define MVOSR_HIST_BINS 169     /* np.histogram(y, bins=arange(170)*0.1)      (:326) */

typedef struct mvosr_ctx mvosr_ctx;

/* Scalars of the path.  cos/sin are passed (not the angle) so that the kernels use the very
 * doubles NumPy produced on the host (scale_calculator.py:391-392). */
typedef struct mvosr_params {
    double cos_pitch;            /* np.cos(camera_pitch), camera_pitch = -0.5*pi/180 (:24) */
    double sin_pitch;            /* np.sin(camera_pitch) */
    double absolute_reference;   /* real camera height, param.camera_h (main.py:55) */
    double pitch_threshold_deg;  /* -80 (:235,:239) */
    double skew_threshold;       /* 0.3 (:348) */
    double mode_rel;             /* 0.33 (:461) */
    int32_t mode_min;            /* 2 (:451,:462) */
    int32_t vote_mode;           /* MVOSR_VOTE_REFERENCE (0): check_triangle's flag pattern exactly as the reference has it —
                                    `b > 0` marks vertices 0 and 1 (:113-115), so the vote depends on the order of the
                                    vertices inside a row and the rows must be SciPy's, verbatim;
                                    MVOSR_VOTE_FIXED (1): `b > 0` marks vertices 0 and 2 (the evident intent of those lines) —
                                    a DECLARED DEVIATION from the reference: the vote is then invariant
                                    under the order of a row's vertices, so any row form of the same triangle set gives
                                    the same counters (what makes the device triangulation's rows usable) */
} mvosr_params;
#define MVOSR_VOTE_REFERENCE 0
#define MVOSR_VOTE_FIXED 1

/* A packed batch of F frames, resident in HBM.  Features are those that passed the
 * vanishing-row filter (:252-254), stored as planes (structure of arrays) with the frames'
 * segments back to back; segment starts are even (16-byte aligned doubles).  x/y/z are the
 * caller's raw feature3d columns — feature_remap (:390-394) is applied by the kernels at load. */
#define MVOSR_TRI2_SURVIVORS 0
#define MVOSR_TRI2_FEATURES 1

typedef struct mvosr_batch {
    int64_t n_frames;
    const int64_t *feat_off;     /* [F]   start of frame f in x/y/z/v (multiple of 2)          */
    const int32_t *feat_cnt;     /* [F]   number of features of frame f                        */
    const double *x, *y, *z;     /* feature3d[:,0..2] before the remap                         */
    const double *v;             /* feature2d[:,1]  (pixel row; u is never read by the path)   */
    const int64_t *tri1_off;     /* [F+1] triangle offsets of the first triangulation          */
    const int32_t *tri1;         /* [tri1_off[F]*3] Delaunay(feature2d).simplices  (:257-258)  */
    const int64_t *tri2_off;     /* [F+1] triangle offsets of the second triangulation         */
    const int32_t *tri2;         /* [tri2_off[F]*3] Delaunay(feature2d[valid]).simplices (:266-267);
                                    ids index the features that survive the vote, in order     */
    const int32_t *n2_expected;  /* [F] or NULL: number of points tri2 was built on; a frame whose
                                    vote keeps a different number gets MVOSR_ST_ERR_MASK        */
    int32_t max_feat;            /* max(feat_cnt) — sizes the LDS request; a frame with more
                                    features than this gets MVOSR_ST_ERR_MASK                  */
    int32_t tri2_ids;            /* MVOSR_TRI2_SURVIVORS (0): tri2 as SciPy returns it, ids index the survivors;
                                    MVOSR_TRI2_FEATURES (1): the same rows relabelled to index the frame's features
                                    (every vertex a survivor, else MVOSR_ST_ERR_MASK) — the frames then run the
                                    gather variant without compacting, whatever their size (meant for dense frames:
                                    a quarter less HBM traffic; results identical)                              */
    int64_t total_feat;          /* length (elements) of the x/y/z/v planes: feat_off[F-1] + padded
                                    count of the last frame; sizes the context's workspace      */
    /* Optional tile index of dense frames (all NULL / 0: none).  With feature-numbered rows (tri2_ids ==
     * MVOSR_TRI2_FEATURES), features sorted so that a triangle's vertices lie close together in memory, and the rows
     * of both triangulations sorted by smallest vertex, the gather variant reads every input byte once: it walks the
     * frame in tiles of MVOSR_TILE_W features with two tiles resident in LDS.  Per frame f the index holds
     * ntiles(f) + 1 = ceil(feat_cnt[f] / MVOSR_TILE_W) + 1 entries starting at tile_base[f]: entry k (k < ntiles) =
     * index, within the frame's rows, of the first row that is walked with tile k — its vertices all lie in tiles k
     * and k+1; entry ntiles = where the "far" rows start (rows whose vertices are further apart: they come last, a
     * few per thousand in a Delaunay triangulation laid out this way, and are gathered from global memory).  The
     * kernel checks the index (starts at 0, monotone, in range) and every walked row against its tile window; an
     * inconsistent index gives MVOSR_ST_ERR_MASK, never a wrong result. */
    int32_t tile_w;              /* MVOSR_TILE_W, or 0 */
    int32_t min_feat;            /* min(feat_cnt), or 0 = not stated.  With waves_per_frame == 0 a batch whose smallest
                                    and largest frames fall into different variants' ranges (below) is launched per
                                    size class — each class with the variant and the LDS request of its own largest
                                    frame; stating min_feat lets a uniform batch skip the classification launch    */
    const int64_t *tile_base;    /* [F+1] */
    const int32_t *tile1_off;    /* [tile_base[F]] index into the frame's tri1 rows */
    const int32_t *tile2_off;    /* [tile_base[F]] index into the frame's tri2 rows */
    int32_t size_hint[4];        /* opaque, all zero = none.  mvosr_batch_size_hint() fills it from the host's copy of
                                    feat_cnt (how many frames each size class holds), so that the per-class launches
                                    of a ragged batch are exactly as long as their lists; without it every class is
                                    launched over n_launch workgroups, most of which leave at once                  */
    /* Optional companion of the tile index (NULL: the kernel gathers instead): the far rows' vertices, copied out of
     * the planes by the packer so that the kernel reads them as one contiguous block per frame instead of a 128-byte
     * line per 8-byte element.  Per frame f, tile_far_off[f+1] - tile_far_off[f] = 9 * (far rows of tri1 + far rows of
     * tri2) doubles starting at tile_far[tile_far_off[f]]: first every far row of tri1 in row order as (y, z, v) of
     * its three vertices, then every far row of tri2 as (x, y, z) of its three vertices — the values of the planes,
     * verbatim (raw, before the remap).  A block of the wrong length gives MVOSR_ST_ERR_MASK; the VALUES cannot be
     * checked by the kernel: they are the caller's copy of its own planes. */
    const double *tile_far;
    const int64_t *tile_far_off; /* [F+1] */
    /* Optional explicit row counts (NULL: frame f has tri*_off[f+1] - tri*_off[f] rows).  With counts, frame f's rows are
     * the first tri*_cnt[f] rows at tri*_off[f] and the offsets only say where a frame's rows start — the form
     * mvosr_delaunay_batch writes (a frame's capacity is 2 * points rows; how many it holds is known on the device
     * only), so that a device-built triangulation goes into the scale kernel without a trip through the host. */
    const int32_t *tri1_cnt;     /* [F] or NULL */
    const int32_t *tri2_cnt;     /* [F] or NULL */
    /* Optional, for layouts that PERMUTE the rows of tri2 (the dense tile layout sorts them by smallest vertex): laid out
     * like tri2's rows, tri2_order[tri2_off[f] + k] = index, within frame f's rows as stored, of the k-th row of the
     * caller's original order (SciPy's).  height_level is np.mean over the steep triangles' heights IN ROW ORDER
     * (/root/reference/src/scale_calculator.py:239-240): with the table the exact pass sums in the original order and
     * the level is the reference's double to the last bit; without it (NULL) in the stored order (equal to rounding). */
    const int32_t *tri2_order;
    /* Optional [F] (NULL: none): frames whose byte is non-zero are finished in the EXACT mode — height_level summed in
     * NumPy's own order — by the product launch itself (they join the few frames its exact pass redoes anyway).  For the
     * frames whose level a LATER step reads: the frame before one that takes the reference's "no enough feature for
     * triangulation" branch and divides by the previous level (/root/reference/src/scale_calculator.py:263-270,:420-422),
     * the last frame of a chunk, the frame the estimator's height_level is left at when the next one raises. */
    const uint8_t *exact_mask;
    /* Optional (all NULL: none) — tri2 is a STAND-IN: the triangle set of the second triangulation with other rows than SciPy's
     * (mvosr_delaunay_batch's canonical form: ~1 us per frame instead of the ~8 us of mvosr_delaunay_qhull_batch).  The rows of
     * tri2 reach the result only through rounding — the LU solve sees the vertices in row order (:229), height_level is summed in
     * row order (:239-240) —, and every frame in which rounding can decide is on the exact pass's list already (a flat triangle
     * within the guard band of the level, a pitch inside the band where the reference's own formulation is evaluated, a level
     * that is itself the result, the exact mask): for THOSE frames mvosr_scale_batch builds SciPy's own rows in place
     * (mvosr_delaunay_qhull_batch's kernel over the list) before the exact pass reads them.  HOT mode only (no stage outputs),
     * survivor-numbered rows, frames that fit the LDS-resident kernels.  standin_u: pixel columns laid out like v; standin_keep:
     * the vote the second triangulation was built on (>= 0: kept), laid out like v; standin_rows / standin_cnt: tri2 / tri2_cnt
     * again, writable; standin_status [F]: receives MVOSR_DT_DEGENERATE | reason << 8 for a listed frame whose rows Qhull's
     * replay declines (the caller then takes that frame through the host's SciPy). */
    const double *standin_u;
    const int32_t *standin_keep;
    int32_t *standin_rows;
    int32_t *standin_cnt;
    int32_t *standin_status;
} mvosr_batch;

#define MVOSR_TILE_W 512

/* Outputs (device pointers; any optional pointer may be NULL). */
typedef struct mvosr_outputs {
    double *raw_scale;           /* [F] absolute_reference/height, before the window median (:419,:421) */
    double *height;              /* [F] camera height over the road in VO units (:418)          */
    double *height_level;        /* [F] mean height of the non-flat triangles (:239-241)        */
    int32_t *status;             /* [F] enum mvosr_status                                      */
    int32_t *counts;             /* [F*MVOSR_N_COUNTS] or NULL                                 */
    /* stage-level outputs for parity tests / the per-frame drop-in call; all optional */
    int32_t *vote_counters;      /* [sum feat_cnt, laid out like x] per-feature counters (:153-163) */
    uint8_t *selected;           /* [like x] 1 where the k-th SURVIVING feature of the frame is selected (:247) */
    double *tri_normals;         /* [tri2_off[F]*3] n = A^-1 . 1  (:229-230)                   */
    double *tri_pitch_deg;       /* [tri2_off[F]]   asin(-n_y/|n|)*180/pi (:233)               */
    double *tri_heights;         /* [tri2_off[F]]   mean y of the 3 vertices (:238)            */
    int32_t *hist;               /* [F*2*MVOSR_HIST_BINS] histogram before / after zeroing single bins (:326,:328) */
    double *stats;               /* [F*4] mean, std, skew, median-or-nan of the kept points (:346,:496) */
} mvosr_outputs;

/* ---- library / context ------------------------------------------------------------------ */
int mvosr_abi_version(void);
const char *mvosr_last_error(void);
int mvosr_device_count(void);
/* The NUMA node the device hangs off (its PCI function's numa_node in sysfs), or -1 where the system does not say.  A host
 * that packs per-frame arrays into page-locked memory and uploads them (mvosr_pack_fill + mvosr_memcpy_h2d_async) is 8-10 %
 * faster, and steadier, with its threads on that node's CPUs: staging memory is then local to the copy engine's root port
 * (measured on a two-socket host: 502-505 k frames/s on the device's node, 460-488 k on the other, 441-468 k unpinned). */
int mvosr_device_numa_node(int device);

/* One context = one device + one HIP stream + a small workspace. */
int mvosr_ctx_create(int device, mvosr_ctx **out);
int mvosr_ctx_destroy(mvosr_ctx *ctx);
/* Adopt an external stream (e.g. torch.cuda.current_stream().cuda_stream); NULL restores the
 * context's own stream.  Either way the incoming stream is ordered behind everything the context has queued on the
 * outgoing one (an event recorded there and waited for by the incoming stream; no host wait when the outgoing stream is
 * the caller's), so work queued before the call and work queued after it keep their order, and a block released after the
 * call still waits for its readers on the old stream.  The outgoing stream must therefore still exist when this is called:
 * hand the context another stream (or NULL) BEFORE destroying the one it has adopted. */
int mvosr_ctx_set_stream(mvosr_ctx *ctx, void *hip_stream);
void *mvosr_ctx_stream(mvosr_ctx *ctx);
int mvosr_ctx_sync(mvosr_ctx *ctx);
/* Pre-size the context's workspace (the dense lists of selected y' the scale kernel hands to the
 * road-model kernel: total_feat doubles + n_frames int32; dense batches with survivor-numbered rows
 * need 24 more bytes per feature, allocated at their first launch).  mvosr_scale_batch grows it on demand
 * with hipMalloc; call this first if the launches must not allocate (e.g. under graph capture). */
int mvosr_ctx_reserve(mvosr_ctx *ctx, int64_t n_frames, int64_t total_feat);
/* Cap, in bytes, on the grow-only workspace of the triangulation kernels (mvosr_delaunay_*_batch: per-frame state beyond LDS —
 * ~0.55 KB per point of frames x largest frame for the Qhull replay): a launch that would need more returns MVOSR_ERR_ALLOC
 * without launching anything, exactly as when the device cannot satisfy the request, and the drop-in sends that chunk through
 * the host's triangulations.  For hosts that share the device with another tenant's allocations.  0 (default): no cap. */
int mvosr_ctx_workspace_limit(mvosr_ctx *ctx, int64_t bytes);
/* Per-call kernel timing of mvosr_scale_batch with HIP events on the launch stream: after
 * mvosr_ctx_profile(ctx, 1) every call (up to 64) records an event before the scale kernel, between
 * the two kernels and after the road-model kernel; mvosr_ctx_profile_read returns the two
 * durations of call `call_index` (0-based since the enable; synchronises on that call's end). */
int mvosr_ctx_profile(mvosr_ctx *ctx, int enable);
int mvosr_ctx_profile_read(mvosr_ctx *ctx, int call_index, float *scale_kernel_ms, float *road_kernel_ms);
/* Device facts for the host (name, CU count, LDS per workgroup). */
int mvosr_ctx_device_info(mvosr_ctx *ctx, char *name, int name_len, int *n_cu, int *lds_per_block);

/* ---- device memory / events (so that a ctypes-only host needs no other GPU library) ------
 * mvosr_malloc / mvosr_host_alloc are CACHING allocators: a block that is freed goes to a size-ordered free list of the
 * context instead of hipFree / hipHostFree, and the next request of a similar size takes it from there — a caller in
 * steady state (a chunk loop, the per-frame drop-in call at /root/reference/src/main.py:110-113) allocates nothing.  A
 * freed block may still be in use by work queued on the context's streams: its next user waits for that work
 * (what hipFree's implicit synchronisation gave).  mvosr_ctx_trim returns the cached blocks to the runtime;
 * mvosr_ctx_alloc_stats reports {hipMalloc calls, hipFree calls, hipHostMalloc calls, hipHostFree calls, cache hits,
 * cached device bytes, cached host bytes, live blocks} (the first n_out of them). */
int mvosr_malloc(mvosr_ctx *ctx, size_t bytes, void **dptr);
int mvosr_free(mvosr_ctx *ctx, void *dptr);
int mvosr_host_alloc(mvosr_ctx *ctx, size_t bytes, void **hptr);                   /* page-locked host memory (staging) */
int mvosr_host_free(mvosr_ctx *ctx, void *hptr);
int mvosr_ctx_trim(mvosr_ctx *ctx);
/* A cached block's release normally marks "everything queued so far" as its last use — in a chunk loop that includes the
 * NEXT chunk's kernels, and the block's next user would wait for them.  mvosr_block_mark(ctx, ptr, 1) records the last use
 * NOW (call it right after the last launch that touches the block) and a later mvosr_free keeps that mark;
 * MVOSR_MARK_UPLOAD: the block (a staging buffer) is used by the upload stream only — its last use is what that stream
 * has queued so far; MVOSR_MARK_IDLE: the caller knows that nothing queued uses the block (a download target whose copy
 * it has waited for); 0 withdraws a mark (the block is used again). */
#define MVOSR_MARK_NOW 1
#define MVOSR_MARK_IDLE 2
#define MVOSR_MARK_UPLOAD 3
int mvosr_block_mark(mvosr_ctx *ctx, void *ptr, int marked);
int mvosr_ctx_alloc_stats(mvosr_ctx *ctx, int64_t *out, int n_out);
int mvosr_memcpy_h2d(mvosr_ctx *ctx, void *dst, const void *src, size_t bytes);   /* stream-ordered, returns after the copy */
int mvosr_memcpy_d2h(mvosr_ctx *ctx, void *dst, const void *src, size_t bytes);   /* stream-ordered, returns after the copy */
/* Asynchronous forms.  Uploads run on the context's UPLOAD stream (so that the next chunk's inputs travel under the
 * current chunk's kernels; `src` should be page-locked — mvosr_host_alloc — or the copy is staged by the runtime) and
 * mvosr_upload_fence makes the compute stream wait for everything uploaded so far (no host wait).  Downloads are
 * queued on the compute stream; the data is there after mvosr_ctx_sync. */
int mvosr_memcpy_h2d_async(mvosr_ctx *ctx, void *dst, const void *src, size_t bytes);
int mvosr_upload_fence(mvosr_ctx *ctx);
int mvosr_memcpy_d2h_async(mvosr_ctx *ctx, void *dst, const void *src, size_t bytes);
/* Device -> PAGE-LOCKED host memory (mvosr_host_alloc) by a KERNEL on the context's compute stream, asynchronous: no copy engine is
 * involved.  For the results of a streamed chunk: a hipMemcpyAsync queued on the compute stream behind long kernels parks the SDMA engine
 * HIP assigns it until those kernels end, and an upload of ANOTHER stream that lands on that engine waits with it (whether it does is
 * decided per process); a copy issued after the kernels, on any stream, waits the other way round behind an upload in flight.  Record
 * an event behind this call and wait for it (mvosr_event_sync / _query) before reading `dst`. */
int mvosr_memcpy_d2h_kernel(mvosr_ctx *ctx, void *dst, const void *src, size_t bytes);
int mvosr_memset(mvosr_ctx *ctx, void *dst, int value, size_t bytes);
int mvosr_event_create(mvosr_ctx *ctx, void **event);
int mvosr_event_record(mvosr_ctx *ctx, void *event);          /* on the context's current stream */
int mvosr_event_elapsed_ms(mvosr_ctx *ctx, void *start, void *stop, float *ms);  /* synchronises on `stop` */
int mvosr_event_sync(mvosr_ctx *ctx, void *event);             /* host waits for the event (not for later work of the stream) */
int mvosr_event_query(mvosr_ctx *ctx, void *event, int *done);  /* *done = 1 when the work recorded before the event has finished, else 0; never waits */
int mvosr_event_destroy(mvosr_ctx *ctx, void *event);

/* ---- host-side packing (no GPU work) ---------------------------------------------------------
 * The per-frame arrays of the reference's call surface — feature3d (N,3) and feature2d (N,2), C-contiguous float64, as
 * /root/reference/src/main.py:102-113 hands them to scale_calculation — laid out as the planes of mvosr_batch by
 * `threads` host threads (<= 0: one per hardware thread, at most 16).  mvosr_pack_count applies the vanishing-row filter
 * (/root/reference/src/scale_calculator.py:252-254: feature2d[:,1] > vanish) and returns the survivors per frame; the
 * caller derives feat_off (even, ascending) and sizes the planes — e.g. page-locked staging memory, so that the packed
 * batch is uploaded without another copy —; mvosr_pack_fill writes x|y|z|u|v at feat_off[f] in the caller's order and,
 * when feat_cnt_out is given, the number of features it kept per frame — so a caller that lays the frames out by their
 * UNFILTERED sizes (feat_off from n_points: a few per cent of slack) needs no counting pass at all.
 * remap_in_place != 0 also applies feature_remap (:390-394) to EVERY row of the caller's feature3d arrays, as the
 * reference does at :414 (the planes keep the raw values: the kernels remap at load). */
int mvosr_pack_count(int64_t n_frames, const double *const *feature2d, const int32_t *n_points, double vanish, int32_t *feat_cnt,
                     int threads);
int mvosr_pack_fill(int64_t n_frames, double *const *feature3d, const double *const *feature2d, const int32_t *n_points,
                    double vanish, const int64_t *feat_off, double *x, double *y, double *z, double *u, double *v,
                    int remap_in_place, double cos_pitch, double sin_pitch, int threads, int32_t *feat_cnt_out);

/* ---- the hot path ------------------------------------------------------------------------- */
void mvosr_default_params(mvosr_params *p, double absolute_reference);

/*
 * Fused per-frame scale recovery: replaces, for every frame of the batch, the body of
 * ScaleEstimator.scale_calculation (scale_calculator.py:411-422) between the two host
 * Delaunay calls and the window median:
 *   feature_remap (:390-394) -> find_outliers/check_triangle on tri1 (:151-167,:105-119)
 *   -> compaction of the survivors (:264-265) -> feature_selection_by_tri on tri2 (:225-248)
 *   -> road_model_calculation_static (:324-354) -> raw scale (:419/:421).
 * Two launches on the context's stream: the scale kernel (remap, vote, compaction, triangle
 * sweeps; one workgroup per frame, its features resident in LDS) leaves every frame's selected
 * y' as a dense list in the context's workspace, and the road-model kernel (one WAVEFRONT per
 * frame, no LDS-resident frame, full occupancy) turns each list into height / scale / status.
 * `waves_per_frame` selects the scale kernel's variant: 0 = choose from max_feat (measured crossovers:
 * 1 up to 320 features, 4 up to 1152, 8 while two workgroups fit a CU's LDS — about 3000 —, 16 above),
 * 1 = one wavefront per frame (<= 512 features), 4/8/16 = one workgroup of that many wavefronts.  With 0, a batch
 * of at least 2048 frames whose sizes span more than one of those ranges (b->min_feat) is split on the device into
 * its size classes, one launch per class over the class's frame list (results do not depend on the variant).
 * Frames that do not fit LDS in fp64 (max_feat > mvosr_max_lds_features(), about 6200) and batches with
 * feature-numbered second triangulations (b->tri2_ids) run the gather variant, which keeps only the vote
 * counters in LDS; with survivor-numbered rows it uses 24 bytes of context workspace per feature.
 * `first_frame`/`n_launch` restrict the launch to a sub-range of the batch (n_launch <= 0: all).
 * MVOSR_WAVES_EXACT or-ed into `waves_per_frame` runs the frames in the exact mode — height_level summed in NumPy's
 * order for every frame, what the stage outputs select implicitly — without asking for stage outputs (the host re-runs
 * single frames this way when a later step will read their level).
 */
#define MVOSR_WAVES_EXACT 0x100
/* or-ed into waves_per_frame: ONLY the frames of the range with a non-zero exact_mask byte are (re)done, in the exact mode;
 * every other frame's outputs stay as they are (the host asks for the neighbours of a frame that raised, once it knows). */
#define MVOSR_WAVES_EXACT_MASKED 0x200
/* or-ed into waves_per_frame: the product (HOT) kernels and the road model ONLY, whatever outputs are asked for (selected,
 * vote_counters: written; per-triangle outputs: refused) — no exact pass, no exact_mask.  A frame the exact pass would have
 * redone (its level may decide its result in the last bit, or IS its result) is left with status MVOSR_ST_REDO and no result:
 * the caller redoes it.  Every other frame's raw_scale, status, counts and selected are final; its height_level is the kernel's
 * own fixed-order sum (equal to NumPy's to ~1e-16 relative, not bit for bit).  The per-frame call of the reference-exact
 * estimator runs this way on stand-in rows and asks SciPy for the second triangulation only when a frame comes back
 * MVOSR_ST_REDO or its exact level is read (mvoscalerecovery_amd/scale_calculator.py). */
#define MVOSR_WAVES_HOT_ONLY 0x400
#define MVOSR_ST_REDO (-2)
int mvosr_scale_batch(mvosr_ctx *ctx, const mvosr_params *p, const mvosr_batch *b,
                      const mvosr_outputs *o, int waves_per_frame,
                      int64_t first_frame, int64_t n_launch);

/* Host helper (no GPU work): from the HOST copy of the batch's feat_cnt set b->max_feat, b->min_feat and
 * b->size_hint.  Optional — see mvosr_batch.size_hint. */
int mvosr_batch_size_hint(const int32_t *feat_cnt_host, int64_t n_frames, mvosr_batch *b);

/*
 * Stage K1 alone: find_outliers (scale_calculator.py:151-167) for every frame; writes
 * o->vote_counters (required) and counts[MVOSR_CNT_VALID] (optional).  Used by the per-frame
 * drop-in call and by the batch path when the second triangulation still has to be built on
 * the host from the surviving features.  Only b->feat_*, y, z, v, tri1* are read.
 * b->max_feat sizes the launch's LDS (and chooses between the LDS-resident and the dense kernel): a frame with
 * feat_cnt[f] > b->max_feat (possible only where the counts live in device memory) is refused before LDS is touched —
 * status (where given) MVOSR_ST_ERR_MASK, counts[MVOSR_CNT_VALID] = 0, and every word of the frame's vote_counters slice -1:
 * a counter >= 0 means "survives" (:166), so whoever reads the slice as `keep` finds no survivor and no stale word.
 */
int mvosr_outlier_vote_batch(mvosr_ctx *ctx, const mvosr_params *p, const mvosr_batch *b,
                             const mvosr_outputs *o, int waves_per_frame);

/*
 * The reference's other vote: find_reliability_by_graph (scale_calculator.py:127-149, with triangle2graph :86-99 and
 * check_depth :121-125) for every frame, one workgroup each (reliability_kernel).  Reads what mvosr_outlier_vote_batch reads:
 * b->feat_*, y, z, v, tri1* (z is remapped at load with p's cos/sin, as the vote does).
 *   Every feature starts at 0.8.  Each row is sorted to (s0, s1, s2) and offers the edges (s0,s1), (s0,s2), (s1,s2); an edge
 *   joins its LOWER end's list when first seen.  The edges are applied once, over i ascending and graph[i] in list order —
 *   i.e. sorted by (i, first row that names both ends, j).  Edge (i, j), i < j, with ri, rj read first:
 *     a = ri*rj, b = (1-ri)*rj, c = (1-rj)*ri, d = (1-ri)*(1-rj);
 *     abnormal — the fp64 product (v[i]-v[j]) * (z[i]-z[j]) > 0 (an underflow to 0 or a NaN is normal) —:
 *       ri' = (0.25*c) / (0.25*(b+c) + 0.5*d),  rj' = (0.25*b) / (0.25*(b+c) + 0.5*d);
 *     normal:  ri' = (a + 0.25*c) / (a + 0.25*(b+c) + 0.5*d),  rj' = (a + 0.25*b) / (a + 0.25*(b+c) + 0.5*d);
 *   every operation an IEEE binary64 operation of its own, in this association; 0/0 = NaN is kept.  The device applies, round
 *   after round, the edges that are next at both their ends: the same values bit for bit.
 * reliability_out: double per feature, laid out like z.  keep_out: int32 per feature, 0 where reliability > 0.8 (:145), else -1
 * (a feature no row names stays at exactly 0.8: rejected; NaN: rejected).  status_out [F]: 0, or MVOSR_ST_ERR_MASK.
 * A frame without rows: every reliability 0.8, every keep -1, status 0 (what the reference returns there).
 * Refused with MVOSR_ST_ERR_MASK and an all -1 keep slice, reliabilities not written: a row that names a vertex twice or an id
 * outside [0, feat_cnt[f]).  b->max_feat sizes the launch's LDS, for max_tri = 2 * b->max_feat rows (at least 1): a frame with
 * feat_cnt[f] > b->max_feat or more rows than max_tri is refused before LDS is touched — MVOSR_ST_ERR_MASK, keep all -1,
 * reliabilities not written.
 * LDS, with N = b->max_feat, T = max_tri: 16 (N rounded up to even) + 16 + 4 (N + 2) + 24 T + 8 ceil(3 T / 32) + 64 bytes —
 * 136 KB for 2 000 features; a launch beyond the device's limit returns MVOSR_ERR_TOO_LARGE, as does b->max_feat > 65535 or
 * 3 * max_tri > 65535 (16-bit ids in LDS).
 */
int mvosr_reliability_batch(mvosr_ctx *ctx, const mvosr_params *p, const mvosr_batch *b, double *reliability_out,
                            int32_t *keep_out, int32_t *status_out);

/*
 * Stage K3 alone: road_model_calculation_static (scale_calculator.py:324-354) on packed
 * lists of already-remapped y values (feat_off/feat_cnt/y of `b`; nothing else is read);
 * `height_level_in` [F] supplies the fallback level (:335).  Writes height, status and the
 * optional counts/hist/stats; raw_scale = absolute_reference/height.  Same kernel as the second
 * launch of mvosr_scale_batch (one wavefront per list); `waves_per_frame` is ignored.
 */
int mvosr_road_model_batch(mvosr_ctx *ctx, const mvosr_params *p, const mvosr_batch *b,
                           const double *height_level_in, const mvosr_outputs *o,
                           int waves_per_frame);

/*
 * K4: scale_filtering (scale_calculator.py:396-400) over a whole sequence: out[i] = median of
 * the last `window` pushed raw scales, the deque pre-loaded with `queue_in[0..n_queue)`.
 * raw/out are device pointers of n doubles; queue_in is a HOST pointer (n_queue <= window).
 */
int mvosr_window_median(mvosr_ctx *ctx, const double *raw, int64_t n, int window,
                        const double *queue_in, int n_queue, double *out);

/*
 * K4 on a sequence that was all-gathered from `n_blocks` ranks and is still in its gathered form:
 * block r starts at blocks + r*block_stride (in doubles) and holds rank r's contiguous share of the
 * n frames (shares as in a contiguous partition: the first n % n_blocks ranks one frame more than
 * n / n_blocks).  Same result as mvosr_window_median on the concatenated sequence; the gathered
 * buffer is read in place, so the multi-GPU step is ONE collective and no repacking kernel.
 */
int mvosr_window_median_blocked(mvosr_ctx *ctx, const double *blocks, int64_t n, int n_blocks, int64_t block_stride,
                                int window, const double *queue_in, int n_queue, double *out);

/* ---- the `rescale` variant (the estimator /root/reference/src/main.py:20 imports) ------------- */

/*
 * GraphChecker.find_inliers (/root/reference/src/graph.py:18-36): per feature the number of incident
 * triangles of tri1 (`total`) and how many of them give the vertex a marginal > 0.6 (`good`); the host
 * keeps a feature when good/total > 0.5 (graph.py:35; 0/0 -> dropped).  `good_bits`: bit 3*code+k is
 * set when vertex k of a triangle with edge-order code `code` (graph.py:124-129) has marginal > 0.6
 * under the 8x8 triangle potential (graph.py:6-17,134-145) — 24 bits computed once on the host.
 * Reads feat_off/feat_cnt/z/v/tri1_off/tri1 of `b` (no remap: rescale.py:25 sets camera_pitch = 0).
 * total/good: int32 device arrays laid out like z.  status [F] (optional): 0 or MVOSR_ST_ERR_MASK.
 * b->max_feat sizes the launch's LDS, and a vertex's two tallies are 16 bits each in LDS, where one row may name a vertex up
 * to three times.  A frame with feat_cnt[f] > b->max_feat (possible only where the counts live in device memory), or with
 * more than MVOSR_GRAPH_MAX_ROWS rows (no accepted frame can then wrap a tally: 3 * 21845 = 65535), is refused before LDS
 * is touched: MVOSR_ST_ERR_MASK, and the frame's total and good slices are zero.
 */
#define MVOSR_GRAPH_MAX_ROWS 21845
int mvosr_graph_inliers_batch(mvosr_ctx *ctx, const mvosr_batch *b, uint32_t good_bits, int32_t *total, int32_t *good,
                              int32_t *status);

/*
 * ScaleEstimator.flat_selection (/root/reference/src/rescale.py:75-102) on the features that
 * survived (x/y/z of `b`, already compacted by the host) and tri2: per triangle heights = 1/|n| with
 * n = A^-1.1, flags bit0 pitch < loose_deg (-80), bit1 pitch < tight_deg (-85), bit2 kept = bit1 and
 * heights > height_factor (0.9) * median(heights[bit0]).  tri_height/tri_flags: per triangle of tri2;
 * height_level/n_kept/status: per frame (status 0, MVOSR_ST_ERR_SINGULAR, _MASK or _EMPTY).
 * max_tri: largest triangle count of a frame (sizes LDS; <= 0: 2*max_feat).
 * b->max_feat and max_tri size the launch's LDS: a frame with feat_cnt[f] > b->max_feat or more rows than max_tri (possible
 * only where the counts live in device memory) is refused before LDS is touched — status MVOSR_ST_ERR_MASK, height_level
 * NaN, n_kept 0, its tri_height / tri_flags rows not written.
 */
int mvosr_flat_selection_batch(mvosr_ctx *ctx, const mvosr_batch *b, double loose_deg, double tight_deg, double height_factor,
                               double *tri_height, uint8_t *tri_flags, double *height_level, int32_t *n_kept, int32_t *status,
                               int64_t max_tri);

/*
 * run_ransac (/root/reference/src/thirdparty/Ransac/ransac.py:3-23) with estimate / is_inlier of
 * /root/reference/src/estimate_road_norm.py:8-18 for every frame, made deterministic by taking the
 * sample sequence as input: triples[f][h][0..2] are row indices into frame f's points (planes
 * px/py/pz, pts_off/pts_cnt per frame), consumed in order h = 0..n_hyp-1.  A hypothesis replaces the
 * best when its inlier count (|m.[p,1]| < threshold over ALL points) is strictly larger; the scan
 * stops at the first improvement whose count exceeds goal_fraction * n_points.  Outputs: counts
 * [F][n_hyp] (optional), model [F][4] = unit (n, d) of the best plane with n_y >= 0
 * (/root/reference/src/rescale.py:159-161), best_ic [F], used [F] (hypotheses consumed).
 * A sample that names a row outside [0, pts_cnt[f]) is treated like one that names a row twice: its
 * model is NaN, its count 0, it can never be the best, and no point is read for it (one thread per
 * hypothesis checks its own sample; the loop over the points is unchanged).  A frame with
 * pts_cnt[f] <= 0 gets a NaN model, best_ic = used = 0 and, where counts is given, counts[f][0..n_hyp) = 0.
 */
int mvosr_ransac_plane_batch(mvosr_ctx *ctx, int64_t n_frames, const int64_t *pts_off, const int32_t *pts_cnt,
                             const double *px, const double *py, const double *pz, const int32_t *triples, int n_hyp,
                             double threshold, double goal_fraction, int32_t *counts, double *model, int32_t *best_ic,
                             int32_t *used);

/*
 * The 2-D line variant, get_pitch_line_ransac (/root/reference/src/estimate_road_norm.py:60-64) with estimate_line /
 * is_inlier_line (:39-49): same kernel and replay rule; samples are pairs, stored like triples
 * (pairs[f][h][0..1] used, [2] ignored), points are (px, py); model [F][4] = unit (a, b, 0, c) of the best line
 * a x + b y + c = 0 with b >= 0 (the reference's SVD null vector has an arbitrary sign).  The guard on the sample's
 * indices covers the pair; the third column is not read at all.
 */
int mvosr_ransac_line_batch(mvosr_ctx *ctx, int64_t n_frames, const int64_t *pts_off, const int32_t *pts_cnt,
                            const double *px, const double *py, const int32_t *pairs, int n_hyp,
                            double threshold, double goal_fraction, int32_t *counts, double *model, int32_t *best_ic,
                            int32_t *used);

/* ---- the `rescale` variant, device-resident (triangulations built by mvosr_delaunay_batch, nothing visits the host) ---- */

typedef struct mvosr_rescale_params {
    uint32_t good_bits;          /* as mvosr_graph_inliers_batch */
    int32_t min_valid;           /* 10: the vote's survivors are re-triangulated only when more than this many are left
                                    (/root/reference/src/rescale.py:133); otherwise every feature stays               */
    double loose_deg, tight_deg; /* -80, -85 (rescale.py:85-86) */
    double height_factor;        /* 0.9 (rescale.py:91) */
    int32_t ransac_min_points;   /* 12 (rescale.py:152) */
    int32_t n_hyp;               /* 100 (rescale.py:155); <= 512 */
    double threshold;            /* 0.005 (rescale.py:155) */
    double goal_fraction;        /* 0.8 (/root/reference/src/estimate_road_norm.py:68) */
    double absolute_reference;   /* real camera height (rescale.py:167) */
    uint64_t seed;               /* key of the sample sequence (below) */
    int64_t frame_base;          /* counter of frame 0 of the batch in the sample sequence (frame f: frame_base + f) */
} mvosr_rescale_params;

/*
 * GraphChecker.find_inliers (/root/reference/src/graph.py:18-36) with the decision made on the device:
 * keep[i] (laid out like z) = 1 where good/total > 0.5 (graph.py:34-35: 2*good > total in integers, 0/0 dropped),
 * -1 where not — unless min_valid or fewer features pass, in which case the reference keeps the frame as it is
 * (/root/reference/src/rescale.py:133-137) and the failed ones get 0: `keep >= 0` is the set the second triangulation is
 * built on (what mvosr_delaunay_batch's `keep` wants), `keep > 0` the vote itself.  n_valid[f] (optional) = features that
 * passed the vote.  Rows: b->tri1 at b->tri1_off[f], b->tri1_cnt[f] of them when tri1_cnt is given (the form
 * mvosr_delaunay_batch writes), else tri1_off[f+1] - tri1_off[f].  A frame whose first triangulation was declined
 * (dt_status[f] != 0, optional) is skipped.
 * A frame mvosr_graph_inliers_batch refuses (feat_cnt[f] > b->max_feat, more than MVOSR_GRAPH_MAX_ROWS rows) is refused
 * here too, with what a declined triangulation gets: every keep word of the frame -1, n_valid 0 — the second triangulation
 * and the flat selection see an empty frame — and status MVOSR_ST_ERR_MASK.
 */
int mvosr_graph_keep_batch(mvosr_ctx *ctx, const mvosr_batch *b, uint32_t good_bits, int32_t min_valid, const int32_t *dt_status,
                           int32_t *keep, int32_t *n_valid, int32_t *status);

/* per-frame outputs of mvosr_flat_ransac_batch (device pointers; the optional ones may be NULL) */
typedef struct mvosr_rescale_outputs {
    double *raw_scale;           /* [F] absolute_reference / camera height of the RANSAC plane (rescale.py:156-167); NaN when
                                    status != 0 */
    double *height_level;        /* [F] 0.9 * median(heights[pitch < -80]) (rescale.py:91-92) */
    double *model;               /* [F][4] unit (n, d) of the best plane, n_y >= 0 (rescale.py:159-161) */
    int32_t *best_ic, *used;     /* [F] inlier count of the best hypothesis, hypotheses consumed (ransac.py:9-22) */
    int32_t *n_kept;             /* [F] kept triangles (rescale.py:96); the point list has 3 * n_kept entries (:101) */
    int32_t *status;             /* [F] 0, MVOSR_ST_RS_FEW, MVOSR_ST_ERR_SINGULAR (rescale.py:79 raises), _MASK, _EMPTY */
    double *tri_height;          /* optional [rows of tri2, laid out like tri2] 1/|n| (rescale.py:89) */
    uint8_t *tri_flags;          /* optional [like tri_height] bit0 pitch < loose, bit1 pitch < tight, bit2 kept */
    int32_t *hyp_counts;         /* optional [F][n_hyp] inlier count of every hypothesis */
} mvosr_rescale_outputs;

/*
 * flat_selection (rescale.py:75-102) + scale_calculation_ransac's plane fit (rescale.py:151-167) in ONE kernel per
 * frame: the features with keep[i] >= 0 (keep == NULL: all) are compacted, in order, into LDS at load; b->tri2 (rows
 * numbered over those survivors; b->tri2_cnt[f] rows at b->tri2_off[f], or the offsets' difference) gives heights,
 * flags, the median level and the kept rows as mvosr_flat_selection_batch does; the kept rows' vertices, in row order
 * with repeats (rescale.py:101), are the RANSAC's point list, which never leaves LDS.  The reference draws its sample
 * triples from OS entropy (/root/reference/src/thirdparty/Ransac/ransac.py:6,10), so any uniform draw of three distinct
 * list positions per hypothesis is a realisation of it; here hypothesis h of frame f takes
 *     key = mix(seed ^ (frame_base + f) * 0xD1B54A32D192ED03),  hk = mix(key + h),  r_k = mix(hk + k),  k = 0, 1, 2
 *     i0 = mulhi(r_0, M), i1 = mulhi(r_1, M - 1) skipping i0, i2 = mulhi(r_2, M - 2) skipping both      (mix = splitmix64's finaliser)
 * — ONE draw per hypothesis.  The list repeats every vertex once per kept triangle, so 0.5-2 % of the draws name one VERTEX
 * twice; such a sample is rank-deficient (the reference's SVD returns whatever plane of the pencil through two points
 * rounding noise selects) and it is NOT drawn again: it spends its iteration, as in the reference (ransac.py:8-21) — its cross
 * product is exactly zero, its model NaN, it counts no inlier and can never be the best, which is also what an `id_triples`
 * entry that names one vertex twice does.  It is a counter-based sequence that depends on (seed, frame counter, hypothesis) only, so a batch, its chunks and
 * per-frame calls draw the same triples (oracle/rescale_oracle.py restates it).  `id_triples` (optional, [F][n_hyp][3]
 * survivor-numbered VERTEX ids) replaces the draw: a recorded sample sequence of the reference mapped to point ids
 * replays its run whatever the row order.  `frame_ids` (optional, [F]) replaces frame_base + f (re-runs of single frames).
 * The replay rule is mvosr_ransac_plane_batch's.  max_tri: largest row count of a frame (<= 0: 2 * b->max_feat).
 * b->max_feat (features BEFORE keep) and max_tri size the launch's LDS: a frame with feat_cnt[f] > b->max_feat or more rows
 * than max_tri is refused before LDS is touched — status MVOSR_ST_ERR_MASK, raw_scale, height_level and model NaN, n_kept,
 * best_ic and used 0; its tri_height / tri_flags / hyp_counts rows are not written.
 */
int mvosr_flat_ransac_batch(mvosr_ctx *ctx, const mvosr_batch *b, const int32_t *keep, const mvosr_rescale_params *rp,
                            const int32_t *id_triples, const int64_t *frame_ids, const int32_t *dt_status,
                            const mvosr_rescale_outputs *o, int64_t max_tri);

/* ---- the same two stages for frames beyond one workgroup's LDS ---- */

/*
 * mvosr_graph_keep_batch with no cap on a frame's features or rows: one workgroup per frame, {v, z} gathered from global
 * memory, the tallies 32 bits wide and held in LDS one TILE of vertices at a time — the rows are swept ceil(feat_cnt / tile)
 * times, with integer LDS atomics only.  `tile`: vertices per sweep (<= 0: the library's choice; clamped to 8192, the LDS it
 * may take).  The tile changes no word of the result.
 * keep, n_valid and status equal mvosr_graph_keep_batch's on every frame that one accepts.  Refusals: a frame with
 * feat_cnt[f] <= 0 (status MVOSR_ST_ERR_EMPTY, n_valid 0), a declined first triangulation (dt_status[f] != 0: every keep word
 * -1, n_valid 0, MVOSR_ST_ERR_EMPTY), a frame with feat_cnt[f] > b->max_feat (refused before anything is read: every keep word
 * -1, n_valid 0, MVOSR_ST_ERR_MASK).  A row that names a vertex outside the frame is left out and gives MVOSR_ST_ERR_MASK, as
 * there.  MVOSR_GRAPH_MAX_ROWS does not apply.  No workspace.  n_frames <= 0: MVOSR_OK, nothing launched.
 */
int mvosr_graph_keep_large_batch(mvosr_ctx *ctx, const mvosr_batch *b, uint32_t good_bits, int32_t min_valid, const int32_t *dt_status,
                                 int32_t *keep, int32_t *n_valid, int32_t *status, int32_t tile);

/*
 * mvosr_flat_ransac_batch — same parameters, same sample sequence, same outputs — with nothing frame-sized in LDS: one
 * workgroup per frame; the survivors' compacted x, y, z, every row's height and flags (where o->tri_height / o->tri_flags are
 * NULL; else the caller's arrays are used) and the point list live in the context's grow-only workspace (the one
 * mvosr_ctx_workspace_limit caps): 24 bytes per element of b->total_feat when keep is given, and n_frames * max_tri * (12 + 8
 * + 1) bytes for the rows.  The point list holds 32-bit vertex ids and positions: 3 * n_kept may exceed 65 535.
 * Every field of `o` equals, bit for bit, what mvosr_flat_ransac_batch writes on every frame that one accepts.  Refusals are
 * that entry point's: feat_cnt[f] <= 0, no rows, or dt_status[f] != 0 -> MVOSR_ST_ERR_EMPTY; feat_cnt[f] > b->max_feat or more
 * rows than max_tri (<= 0: 2 * b->max_feat) -> MVOSR_ST_ERR_MASK; in both raw_scale, height_level and model NaN, n_kept,
 * best_ic and used 0, nothing else written.  b->total_feat must be stated.
 * Returns MVOSR_ERR_TOO_LARGE only where 3 * max_tri or n_frames does not fit 32 bits, MVOSR_ERR_ALLOC where the workspace
 * cannot grow (or would pass the context's limit), MVOSR_ERR_ARG as mvosr_flat_ransac_batch (n_hyp in 1..512).
 * n_frames <= 0: MVOSR_OK, nothing launched, no workspace asked for.
 */
int mvosr_flat_ransac_large_batch(mvosr_ctx *ctx, const mvosr_batch *b, const int32_t *keep, const mvosr_rescale_params *rp,
                                  const int32_t *id_triples, const int64_t *frame_ids, const int32_t *dt_status,
                                  const mvosr_rescale_outputs *o, int64_t max_tri);

/* ---- C runs of a sequence at once (/root/reference/test_off_line.sh:4-16 runs main_offline.py ten times on one saved dict) ---- */

/* which form of the point list a frame's inlier counts were taken over (count_form; the counts do not depend on it) */
enum mvosr_cases_form {
    MVOSR_CASES_FORM_NONE = 0,   /* the frame was not fitted                                                              */
    MVOSR_CASES_FORM_GATHER = 1, /* distinct vertices with multiplicities, coordinates gathered by id                     */
    MVOSR_CASES_FORM_PACKED = 2  /* at most 1024 distinct vertices: coordinates and multiplicities side by side in LDS    */
};

/* outputs of mvosr_flat_ransac_cases_batch (device pointers; C = n_cases; the optional ones may be NULL) */
typedef struct mvosr_rescale_cases_outputs {
    double *raw_scale;           /* [F][C] as mvosr_rescale_outputs.raw_scale, per case; NaN where the case's status != 0 */
    double *model;               /* [F][C][4] */
    int32_t *best_ic, *used;     /* [F][C] */
    int32_t *status;             /* [F][C] 0, MVOSR_ST_RS_FEW, MVOSR_ST_ERR_MASK, MVOSR_ST_ERR_EMPTY */
    int32_t *hyp_counts;         /* optional [F][C][n_hyp] */
    int32_t *count_form;         /* optional [F] enum mvosr_cases_form */
} mvosr_rescale_cases_outputs;

/*
 * The plane fit of mvosr_flat_ransac_batch for n_cases sample sequences of every frame in ONE launch, the deterministic stages
 * not repeated.  It runs behind a launch of mvosr_flat_ransac_batch over the same batch, keep, dt_status and max_tri that was asked
 * for tri_flags, and reads per frame: the features with keep[i] >= 0 compacted in order (the numbering of b->tri2's ids), b->tri2
 * with its counts, and tri_flags (laid out like tri2), whose bit 2 marks a kept row.  The point list is rebuilt in that kernel's
 * order — kept rows in row order, three vertex ids each, repeats included (/root/reference/src/rescale.py:101) —; the draw indexes
 * list positions.  Hypothesis h of case c of frame f takes mvosr_flat_ransac_batch's draw with
 *     key = mix(case_seeds[c] ^ (frame counter) * 0xD1B54A32D192ED03),   frame counter = frame_ids ? frame_ids[f] : rp->frame_base + f
 * so case c is, bit for bit, what mvosr_flat_ransac_batch returns with rp->seed = case_seeds[c] (rp->seed itself is not read; nor
 * are good_bits, min_valid, loose_deg, tight_deg and height_factor).  id_triples (optional, [F][C][n_hyp][3] survivor-numbered
 * vertex ids) replaces the draw as in that call.  Counts, replay rule, sign rule and raw scale are that call's.
 * Grid: frames x ceil(n_cases / cases_per_group) workgroups; a workgroup loads the frame and builds the list once and loops over its
 * cases (cases_per_group 0: the measured default; the results do not depend on it).  case_seeds: [n_cases] device array.
 * Statuses per (frame, case): MVOSR_ST_RS_FEW — a list shorter than ransac_min_points, or no hypothesis with an inlier —;
 * MVOSR_ST_ERR_MASK — feat_cnt[f] > b->max_feat or more rows than max_tri (refused before LDS is touched), or a kept row that names
 * a vertex outside the survivors —; MVOSR_ST_ERR_EMPTY — no features, no rows, or dt_status[f] != 0 (skipped like a declined frame).
 * A case that is not fitted has NaN raw_scale and model, best_ic = used = 0; its hyp_counts are not written.  The heights are not
 * recomputed here: what mvosr_flat_ransac_batch says of the FRAME — MVOSR_ST_ERR_SINGULAR, or MVOSR_ST_ERR_MASK for a row that is
 * not kept — is that launch's status to read (rescale.ScaleEstimator.raw_scale_cases_batch merges the two).
 */
int mvosr_flat_ransac_cases_batch(mvosr_ctx *ctx, const mvosr_batch *b, const int32_t *keep, const mvosr_rescale_params *rp,
                                  const uint64_t *case_seeds, int32_t n_cases, int32_t cases_per_group, const int32_t *id_triples,
                                  const int64_t *frame_ids, const int32_t *dt_status, const uint8_t *tri_flags,
                                  const mvosr_rescale_cases_outputs *o, int64_t max_tri);
/* dynamic LDS a launch asks for at (b->max_feat, max_tri (<= 0: 2 * max_feat), n_hyp) */
size_t mvosr_flat_ransac_cases_lds_bytes(int max_feat, int64_t max_tri, int n_hyp);

/* ---- flat_selection for several settings of its constants in one launch (the thresholds of rescale.py:85-96, the factor of :91) ---- */

/*
 * mvosr_flat_selection_batch's selection for n_sel settings (loose_deg[s], tight_deg[s], height_factor[s]; host arrays, n_sel in
 * 1..mvosr_flat_selection_sweep_max_settings() = 16) on the device-resident form of a batch: it reads what mvosr_flat_ransac_batch
 * reads — the features with keep[i] >= 0 compacted in order (keep == NULL: all), b->tri2 with b->tri2_cnt[f] rows at b->tri2_off[f]
 * or the offsets' difference, dt_status (optional; non-zero: the frame is skipped) — and fits nothing.  Every row's height and the
 * sine of its pitch are computed once per frame; per setting the two threshold bits are decided as that call decides them, the level
 * is height_factor[s] * np.median(heights[pitch < loose_deg[s]]) (NaN for an empty set) and bit 2 is bit 1 && height > level, so for
 * every s the flags, the level and the count equal, bit for bit, mvosr_flat_selection_batch's and mvosr_flat_ransac_batch's with that
 * setting's constants.  loose_deg[s] < tight_deg[s] is legal and means what the formulas say.
 * Outputs: tri_flags [n_sel][R] — one plane per setting, laid out like tri2, R = b->tri2_off[F] rows where the counts are the
 * offsets' differences and 2 * b->total_feat rows with b->tri2_cnt (the form mvosr_delaunay_batch writes: a frame's rows start at
 * twice its feature offset); plane s is what mvosr_flat_ransac_cases_batch takes as tri_flags —; height_level [F][n_sel]; n_kept
 * [F][n_sel]; status [F]: 0, MVOSR_ST_ERR_SINGULAR, MVOSR_ST_ERR_MASK (a row with a vertex id outside the survivors) or
 * MVOSR_ST_ERR_EMPTY (no features, no rows, skipped), the frame's, whatever the setting; tri_height (optional) [R] 1/|n|.
 * b->max_feat and max_tri (<= 0: 2 * b->max_feat) size the launch's LDS: a frame with feat_cnt[f] > b->max_feat, more rows than
 * max_tri, or rows outside a plane is refused before LDS is touched — status MVOSR_ST_ERR_MASK, its levels NaN, its counts 0, its
 * tri_flags / tri_height rows not written.
 */
int mvosr_flat_selection_sweep_batch(mvosr_ctx *ctx, const mvosr_batch *b, const int32_t *keep, const int32_t *dt_status, int32_t n_sel,
                                     const double *loose_deg, const double *tight_deg, const double *height_factor, uint8_t *tri_flags,
                                     double *height_level, int32_t *n_kept, int32_t *status, double *tri_height, int64_t max_tri);
/* dynamic LDS a launch asks for at (b->max_feat, max_tri (<= 0: 2 * max_feat), n_sel) */
size_t mvosr_flat_selection_sweep_lds_bytes(int max_feat, int64_t max_tri, int n_sel);
int mvosr_flat_selection_sweep_max_settings(void);

/* ---- GraphGrow: the road region grown over triangle adjacency (/root/reference/src/graph.py:39-107) ---------------- */

typedef struct mvosr_grow_params {
    double threshold_angle;      /* 8: two neighbours join when their pitch differs by less (graph.py:40,74)             */
    double seed_deg;             /* -85: a flat seed has pitch below this (graph.py:90)                                  */
    double level_deg;            /* -80: ... and 1/height below median(1/height[pitch < level_deg]) (graph.py:91)         */
    double height_factor;        /* 0.4: ... and their 1/height by less than height_factor * median(1/height) (:74,93)    */
} mvosr_grow_params;

/* outputs of mvosr_region_grow_batch (device pointers; the optional ones may be NULL).  "rows": laid out like tri2. */
typedef struct mvosr_grow_outputs {
    uint8_t *region;             /* [rows of tri2] 1 = in the grown region */
    int32_t *n_region, *n_flat, *status;      /* [F] rows in the region, flat seeds (graph.py:92), status */
    double  *level, *threshold_height;        /* [F] median(hinv[angle<level_deg]), height_factor*median(hinv) (graph.py:91,93) */
    int32_t *label;              /* optional [rows] smallest row index of the row's component */
    int32_t *neighbors;          /* optional [rows][3] row across edge (a,b),(a,c),(b,c); -1: none */
    double  *tri_height, *tri_angle;          /* optional [rows]: what the from-points form computed */
} mvosr_grow_outputs;

/*
 * GraphGrow.process (graph.py:85-107) for every frame, one workgroup each (region_grow_kernel).  Rows: b->tri2 at
 * b->tri2_off[f], b->tri2_cnt[f] of them when tri2_cnt is given, else tri2_off[f+1] - tri2_off[f]; ids in [0, feat_cnt[f]).
 *   hinv = 1/heights (:88, an IEEE division);  flat = angle < seed_deg and hinv < median(hinv[angle < level_deg]) (:90-92);
 *   threshold_height = height_factor * median(hinv) (:93); rows i, j that share an edge (:47-72) are joined iff
 *   |angle_i - angle_j| < threshold_angle and |hinv_i - hinv_j| < threshold_height, both strict (:73-77).
 * Medians are np.median's: the mean (a + b) / 2 of the two middle order statistics of an even count, NaN for an empty
 * subset (then nothing is flat).  A NaN angle is never flat, never joined and outside the first median's subset.
 * `expend` (:79-83) compares a row with the row it came from, so a proposal is the connected component of its seed in the
 * joined graph over ALL rows; the reference draws 100 seeds at random and keeps the longest proposal (:97-103).  Declared
 * rule here: the region is the largest component that holds a flat row; among equally large ones the one with the smallest
 * row index; region[] marks its rows (the reference's list order is its random walk's).  Nothing flat: all-zero region,
 * n_region 0 (:95-96).  label[] is the smallest row index of each row's component, whether seeded or not.
 * Two forms: tri_height_in and tri_angle_in both given ([rows], `process`'s own arguments; x/y/z are not read), or both
 * NULL: heights and angles are computed from the frame's x/y/z with mvosr_flat_selection_batch's expressions
 * (/root/reference/src/rescale.py:78-89: n = A^-1.1, height = 1/|n|, angle = asin(-n_y/|n|) * 180/pi) and written to
 * tri_height / tri_angle when asked for; a zero pivot gives MVOSR_ST_ERR_SINGULAR (rescale.py:79 raises) and an all-zero
 * region.  Exactly one of the two given: MVOSR_ERR_ARG.
 * Refused with MVOSR_ST_ERR_MASK, an all-zero region, n_region = n_flat = 0, NaN level / threshold_height, label and
 * neighbors -1 (what graph.py:59's list(intersect)[0] would pick arbitrarily, or raise on): an edge named by more than two
 * rows, a row that names a vertex twice, an id outside [0, feat_cnt[f]), a given height that is not finite and positive.
 * b->max_feat and max_tri (largest row count of a frame; <= 0: 2 * b->max_feat) size the launch's LDS: a frame with
 * feat_cnt[f] > b->max_feat or more rows than max_tri is refused before LDS is touched — MVOSR_ST_ERR_MASK, level and
 * threshold_height NaN, n_region and n_flat 0, its per-row outputs not written.  A frame with no rows: MVOSR_ST_ERR_EMPTY,
 * the same per-frame values.
 * LDS, with T = max_tri and N = b->max_feat:  16 T + 64 + max(12 T + 4 (N + 2), from-points ? 24 (N rounded up to even) : 0)
 * (rounded up to 8) + 1152 + 6 T (rounded up to 16) bytes — 144 KB for 3 980 rows of 2 000 points; a launch beyond the
 * device's limit returns MVOSR_ERR_TOO_LARGE, as does b->max_feat > 65535 or max_tri >= 65535 (16-bit ids in LDS).
 */
int mvosr_region_grow_batch(mvosr_ctx *ctx, const mvosr_batch *b, const double *tri_height_in, const double *tri_angle_in,
                            const mvosr_grow_params *gp, const mvosr_grow_outputs *o, int64_t max_tri);

/* ---- the triangle-graph road selection (/root/reference/src/scale_calculator.py:177-222) ------------------------------- */

/* outputs of mvosr_tri_graph_batch (device pointers; every one except status, selected and height_level may be NULL).
 * "rows": laid out like tri2. */
typedef struct mvosr_trigraph_outputs {
    double  *p_road;             /* [rows] the probability a row ends with (:213; a row that is not flat keeps its initial one) */
    double  *p_initial;          /* [rows] max((-70 - pitch_deg) / 20 - 0.2, 0) (:188-189) */
    uint8_t *valid;              /* [rows] p_road > 0.5 (:219) */
    int32_t *neighbors;          /* [rows][3] graph[row] of triangle2region_graph (:56-81) in ITS list order, -1 padded */
    double  *tri_height;         /* [rows] from-points form: mean y' of the three vertices (:186) */
    double  *tri_pitch_deg;      /* [rows] from-points form: asin(-n_y/|n|) * 180/pi (:185) */
    uint8_t *selected;           /* [features, laid out like x] 1 where the feature is a vertex of a valid row (:221) */
    double  *height_level;       /* [F] np.mean(heights[pitch_deg >= -80]) in NumPy's summation order (:216); NaN: no such row */
    int32_t *n_flat, *n_valid;   /* [F] rows with pitch_deg < -80 (:190); valid rows */
    int32_t *n_rounds;           /* [F] rounds the sweep took (the depth of the flat rows' dependency order) */
    int32_t *status;             /* [F] 0, MVOSR_ST_ERR_SINGULAR, _MASK or _EMPTY */
} mvosr_trigraph_outputs;

/*
 * feature_selection_by_tri_graph (scale_calculator.py:177-222, with triangle2region_graph :56-81 and compare :169-175) for every
 * frame, one workgroup each (tri_graph_kernel).  Rows: b->tri2 at b->tri2_off[f], b->tri2_cnt[f] of them when tri2_cnt is
 * given, else tri2_off[f+1] - tri2_off[f]; ids in [0, feat_cnt[f]).
 *   graph[i]: rows are visited ascending; row i = (a, b, c) looks for an EARLIER row that shares the edge ab, then ac, then bc,
 *   and each hit appends the earlier row to graph[i] and i to graph[earlier].  So graph[i] holds first its lower-index
 *   neighbours in the order of row i's own edge slots (ab, ac, bc) — the row as given, not sorted —, then its higher-index
 *   neighbours ascending; at most 3 entries.
 *   p = (-70 - pitch_deg) / 20 - 0.2, set to 0 where p < 0 (a NaN stays).  flat: pitch_deg < p->pitch_threshold_deg (-80).
 *   For v over the flat rows, ascending: ha = heights[v], pa = p[v]; for u in graph[v], in list order:
 *     d = heights[u] - ha;  column c = 0 where d < -0.1, 2 where d > 0.1, else 1 (both strict; a NaN gives 1);
 *     pc = p[u]  — the FINAL value where u < v and u is flat, else the initial one (a higher flat row is read before its turn);
 *     m0 = (1-pa)*(1-pc), m1 = (1-pa)*pc, m2 = pa*(1-pc), m3 = pa*pc;
 *     o = column c of [[0.33,0.33,0.33],[0.03,0.07,0.90],[0.90,0.07,0.03],[0.05,0.9,0.05]];
 *     pa = num / den  with  num = fma(o3, m3, o2*m2),  den = fma(o0, m0, o2*m2) + fma(o1, m1, o3*m3)
 *   then p[v] = pa.  The two dot products are NumPy's `@` (:210), i.e. the installed BLAS's strided ddot; the form above is the
 *   DECLARED RULE: it reproduces OpenBLAS 0.3.29's Haswell kernel bit for bit on every operand tried, where a left-to-right
 *   sum does not; another BLAS build may give the reference itself other last bits.  Every other operation is one IEEE
 *   binary64 operation; 0/0 = NaN is kept.  The device finishes, round after round, the flat rows whose flat lower-index
 *   neighbours are final: the same values bit for bit, with no cap on the rounds.
 *   valid = p > 0.5 over all rows; selected marks the vertices of the valid rows; height_level = np.mean(heights[pitch_deg >=
 *   thr]) in NumPy's pairwise order (NaN when no row is steep).
 * Two forms: tri_height_in and tri_pitch_in both given ([rows]: mean height and pitch in degrees per row; x/y/z are not read and
 * everything after them is bit-exact; a NaN flows through as IEEE: never flat, never steep, never valid, "equal" in compare), or
 * both NULL: they are computed from the frame's x/y/z, remapped at load with p's cos/sin, by the scale kernel's reference
 * formulation (n = A^-1 . 1 by LU with partial pivoting, normalise, asin, degrees; h = ((y0 + y1) + y2) / 3) and written to
 * tri_height / tri_pitch_deg when asked for; a zero pivot gives MVOSR_ST_ERR_SINGULAR (:181 raises).  Exactly one of the two
 * given: MVOSR_ERR_ARG.
 * Refused with MVOSR_ST_ERR_MASK (what :68's list(intersect)[0] would pick arbitrarily): an edge named by more than two rows, a
 * row that names a vertex twice, an id outside [0, feat_cnt[f]).  A refused frame (MASK or SINGULAR) gets all-zero valid and
 * selected slices, height_level NaN and counts 0; p_road, p_initial and neighbors are not written (tri_height / tri_pitch_deg
 * are, once the ids have passed).  A frame with no rows: MVOSR_ST_ERR_EMPTY, an all-zero selected slice, the same per-frame values.
 * b->max_feat sizes the launch's LDS, for max_tri = 2 * b->max_feat rows (at least 1): a frame with feat_cnt[f] > b->max_feat
 * or more rows than max_tri is refused before LDS is touched — MVOSR_ST_ERR_MASK, height_level NaN, counts 0, none of its
 * per-row or per-feature outputs written.
 * LDS, with N = b->max_feat, T = max_tri:  max(4 (N + 2) + 12 T, 8 T + 1712, from-points ? 24 (N rounded up to even) : 0)
 * + 25 T + 4 ceil(N / 32) + 80 bytes, each term rounded up to 8 — 153 KB for 2 000 features, 2 095 features within 160 KB; a launch
 * beyond the device's limit returns MVOSR_ERR_TOO_LARGE, as does b->max_feat > 65535 or max_tri > 65535 (16-bit ids in LDS).
 */
int mvosr_tri_graph_batch(mvosr_ctx *ctx, const mvosr_params *p, const mvosr_batch *b, const double *tri_height_in,
                          const double *tri_pitch_in, const mvosr_trigraph_outputs *o);

/*
 * road_model_calculation_static_tri (/root/reference/src/scale_calculator.py:294-310 with check_mode :446-483; what follows the
 * return at :310 is dead, the result of :305 unused) for n_lists lists of triangle heights, one wavefront per list
 * (static_tri_kernel): the road model that rescale.py:194 leaves commented out, fed by flat_selection's heights[pitch < loose]
 * (rescale.py:102).  Every output is a function of the list's counted values alone and is compared for bit equality.
 * List f is the entries i in [off[f], off[f] + cnt[f]) of `height` — cnt == NULL: off has n_lists + 1 entries and the lengths
 * are their differences —; an entry counts where flags == NULL (packed lists) or flags[i] & 1 (the row form: tri_height and
 * tri_flags as mvosr_flat_selection_batch / mvosr_flat_ransac_batch write them, off / cnt the batch's tri2_off / tri2_cnt).
 * The height of an entry that does not count is never read.  With n the number of counted entries:
 *   hi = 1.0 / h, the IEEE quotient (:296).
 *   dis[k], k = 0..18: how many hi satisfy e[k] <= hi < e[k+1] with e[k] = (double)k * 0.1, bin 18 also hi == e[19] (:297,
 *   np.histogram over an explicit edge array counts by comparison); a value outside [0, e[19]] is in no bin.
 *   dis[k] == 1 becomes 0 (:299); max is taken after that.
 *   max <= 2 (:451-452, :302-303): scale_norm = np.median(hi) over ALL n values — the middle order statistic, or (a + b) / 2.0 of
 *   the two middle ones —, status MVOSR_ST_MEDIAN.
 *   Else bin 0 and bin 18 are flagged where they equal max, bin k in 1..17 where dis[k] >= dis[k-1], dis[k] >= dis[k+1],
 *   (double)dis[k] >= 0.33 * (double)max and dis[k] >= 2 (:454-463); with i..j the FIRST run of consecutive flagged bins
 *   (modes[0], :473-481, :306-307 — not the run that holds the maximum), scale_norm = (double)((i + 1) + (j + 1)) / 2.0 / 10.0
 *   (:308-310; int(e[k] * 10) == k for every k), status MVOSR_ST_MODE.
 * raw_scale = scale_norm * absolute_reference (rescale.py:183).  n_used = n.  hist (optional, [n_lists][19]): dis after the ones
 * are zeroed.
 * n <= min_count (rescale.py:181 asks for more than 12; 0 for the bare function) or n == 0: MVOSR_ST_RS_FEW, scale_norm and
 * raw_scale NaN, hist zero.  A counted height that is not finite or not > 0 is outside the contract (flat_selection produces
 * none): the list gets MVOSR_ST_ERR_MASK, NaN and a zero hist, as does a list with a negative offset or length or more than
 * 2^31 - 1 entries, of which nothing is read.
 * No LDS.  n_lists <= 0: MVOSR_OK, nothing launched.  MVOSR_ERR_ARG: a null ctx / off / height / scale_norm / raw_scale / n_used /
 * status, or min_count < 0.
 */
int mvosr_static_tri_batch(mvosr_ctx *ctx, int64_t n_lists, const int64_t *off, const int32_t *cnt, const double *height,
                           const uint8_t *flags, int32_t min_count, double absolute_reference, double *scale_norm,
                           double *raw_scale, int32_t *n_used, int32_t *hist, int32_t *status);

/* per-frame outputs of mvosr_flat_static_tri_batch (device pointers; the optional ones may be NULL) */
typedef struct mvosr_static_tri_outputs {
    double *scale_norm, *raw_scale;   /* [F]; NaN unless status is MODE or MEDIAN */
    double *height_level;             /* [F] as mvosr_flat_ransac_batch writes it */
    int32_t *n_used, *n_kept, *status;/* [F] */
    int32_t *hist;                    /* optional [F][19], after the ones are zeroed */
    double *tri_height;               /* optional, laid out like tri2 */
    uint8_t *tri_flags;               /* optional, bits 0..2 as mvosr_flat_ransac_batch */
} mvosr_static_tri_outputs;

/*
 * flat_selection (rescale.py:75-102) and the histogram-mode road model over its loose heights (scale_calculation_static_tri,
 * rescale.py:179-187) in ONE kernel per frame on the device-resident form of a batch (flat_static_tri_kernel):
 * what mvosr_flat_ransac_batch with tri_height / tri_flags outputs followed by mvosr_static_tri_batch in row form computes, the
 * heights and flags never leaving LDS.  It reads what mvosr_flat_ransac_batch reads: the batch, keep (survivors keep[i] >= 0,
 * compacted in order at load; NULL: all), dt_status, b->tri2 / tri2_off / tri2_cnt, max_tri (<= 0: 2 * b->max_feat).
 * Per frame: every row's height and bits 0 and 1 as mvosr_flat_selection_batch decides them; height_level = height_factor *
 * median(h[loose]), bit 2 and n_kept as there; and over the loose rows' heights the road model exactly as mvosr_static_tri_batch
 * states it above (hi = 1.0 / h, the 19 bins, ones zeroed, median or first run; n <= min_count or no loose row: MVOSR_ST_RS_FEW),
 * raw_scale = scale_norm * absolute_reference, n_used = the number of loose rows.  Every output is compared for bit equality.
 * Status: a flat-stage refusal or error takes precedence, as mvosr_flat_ransac_batch reports it — MVOSR_ST_ERR_EMPTY (no features
 * or rows, dt_status[f] != 0), MVOSR_ST_ERR_MASK (feat_cnt[f] > b->max_feat or more rows than max_tri, refused before LDS is
 * touched; or a row naming a vertex outside the frame), MVOSR_ST_ERR_SINGULAR —: scale_norm and raw_scale NaN, n_used 0, hist zero.
 * Otherwise the model's status as mvosr_static_tri_batch gives it (MODE, MEDIAN, RS_FEW, or its own MVOSR_ST_ERR_MASK for a loose
 * height that is not finite or not > 0).  height_level, n_kept, tri_height and tri_flags are always what mvosr_flat_ransac_batch
 * writes for that frame (a refused frame: height_level NaN, n_kept 0, its tri_height / tri_flags rows not written).
 * The given form — tri_height_in and tri_flags_in both non-NULL, laid out like tri2 (as mvosr_region_grow_batch takes heights):
 * the rows' heights and bits 0 and 1 are read from those arrays; x / y / z, keep and tri2 are not read; everything behind them runs
 * the same code; bit 0 says a row counts.  Nothing row-sized is kept in LDS, so max_tri bounds a frame's rows but not the request.
 * One of the two pointers alone: MVOSR_ERR_ARG.
 * LDS: mvosr_flat_static_tri_lds_bytes(b->max_feat, max_tri) — less than mvosr_flat_ransac_batch asks at the same sizes from 342
 * features on, below 64 KiB before —: the launch accepts every frame that one accepts.
 * n_frames <= 0: MVOSR_OK, nothing launched.  MVOSR_ERR_ARG: a NULL ctx, batch, o or mandatory output, or min_count < 0.
 */
int mvosr_flat_static_tri_batch(mvosr_ctx *ctx, const mvosr_batch *b, const int32_t *keep,
                                double loose_deg, double tight_deg, double height_factor,
                                int32_t min_count, double absolute_reference,
                                const int32_t *dt_status,
                                const double *tri_height_in, const uint8_t *tri_flags_in,
                                const mvosr_static_tri_outputs *o, int64_t max_tri);
size_t mvosr_flat_static_tri_lds_bytes(int max_feat, int64_t max_tri);

/*
 * The feature-distribution analysis (/root/reference/src/scale_calculator.py:486-599: check_full_distribution, check_skewness,
 * skewness_analysis, mode_analysis, plot_distribution — what they compute, not what they draw) for n_frames frames, one workgroup
 * per frame and one wavefront per population (featdist_kernel).  Every output is a function of the frame's values alone and is
 * compared for bit equality.
 * Frame f is the entries i in [off[f], off[f] + cnt[f]) of `y` and `level` — cnt == NULL: off has n_frames + 1 entries and the
 * lengths are their differences.  y: the features' raw y (no remap, :563).  level: 0 = a feature below the vanishing row (:564),
 * 1 = also kept by the vote (:575-578), 2 = also selected (:588-591).  Population p = 0, 1, 2 is the entries with level >= p in
 * packed order (the order of the reference's mask and np.unique indexing).  scale[f]: the frame's true scale (:569).
 * Per frame and population, row = f * MVOSR_FD_POPULATIONS + p:
 *   n_out[row]: the population's size.
 *   hist[row][0..168]: how many y satisfy e[k] <= y < e[k+1] with e[k] = (double)k * 0.1, bin 168 also y == e[169] (:492;
 *   np.histogram over an explicit edge array counts by comparison; NaN and values outside [0, e[169]] are in no bin).
 *   hist[row][169..171]: how many y are exactly e[29], e[49], e[99].  np.histogram over np.array(range(0, m + 1)) * 0.1 (m = 29: :514;
 *   49: :528-536; 99: :506) is hist[row][0..m-1] with that count added to bin m - 1: its last bin is closed.
 *   hist_scaled[row]: the same 172 words of y * scale[f] (one IEEE multiply).  A product that is not finite is in no bin.
 *   stats[row][0..2]: np.mean(y), np.std(y), np.median(y) to the last bit — the sums in np.add.reduce's pairwise order (below 8
 *   values a plain loop from 0.0, up to 128 eight strided accumulators, above that halves split at a multiple of 8), std =
 *   sqrt(sum((y - mean)^2) / n), the median (0.0 + a) / 1.0 or ((0.0 + a) + b) / 2.0 of the middle order statistics, NaN where the
 *   population holds a NaN.
 *   An empty population: n_out 0, stats NaN, zero histograms; that is no error.
 * status[f]: 0, or MVOSR_ST_ERR_MASK — a level above 2 (with one level per feature "selected" implies "kept": no other sequence
 * is invalid), a negative offset or length, or more entries than max_feat; of such a frame nothing past the levels is used:
 * n_out 0, stats NaN, zero histograms, nothing added to the tables.
 * seq_tables (optional): int64 [MVOSR_FD_POPULATIONS][MVOSR_FD_HIST_WORDS] in device memory, owned by the caller and kept across
 * launches: every frame's hist_scaled is ADDED to it (64-bit atomic adds of integers from the frame's finished LDS histogram:
 * the order of arrival changes nothing).  The caller zeroes it.
 * LDS is carved at max_feat (mvosr_featdist_plan.hpp): above mvosr_featdist_max_features() — the largest frame whose three lists
 * fit 160 KiB — the launch returns MVOSR_ERR_TOO_LARGE.  n_frames <= 0: MVOSR_OK, nothing launched.  MVOSR_ERR_ARG: a null
 * argument other than cnt / seq_tables, or max_feat < 0.
 */
#define MVOSR_FD_POPULATIONS 3
#define MVOSR_FD_HIST_WORDS 172  /* MVOSR_HIST_BINS + the three closing-edge counts */
int mvosr_feature_distribution_batch(mvosr_ctx *ctx, int64_t n_frames, const int64_t *off, const int32_t *cnt, const double *y,
                                     const uint8_t *level, const double *scale, int32_t max_feat, int32_t *n_out, int32_t *hist,
                                     int32_t *hist_scaled, double *stats, int32_t *status, int64_t *seq_tables);
int mvosr_featdist_max_features(void);

/*
 * The pairwise depth-order check (/root/reference/script/data_check.py:19-34, depth_check — what it computes, not what it draws)
 * for n_frames frames.  Frame f is the entries i in [off[f], off[f] + cnt[f]) of `y`, `z` and `level` — cnt == NULL: off has
 * n_frames + 1 entries —, the packed planes of the staged path; level as for mvosr_feature_distribution_batch (0, 1 or 2).
 * A point is selected iff y > 0 (:20; a NaN y is not).  For selected points vn = y / z (:23), and for EVERY ordered pair (i, j) of
 * them, the diagonal included, q = (z_j - z_i) / ((vn_j - vn_i) + 0.000001) (:26-28): IEEE double operations, one at a time.
 * The pair belongs to population p = 0, 1, 2 iff min(level_i, level_j) >= p.  Per frame and population, row = f * 3 + p:
 *   hist[row][k], k < MVOSR_DC_BINS: pairs with 50 * (k - 40) <= q < 50 * (k - 39), the last bin also q == 950 — the counts of
 *   np.histogram(q, np.array(range(-40, 20)) * 50) (:30-31), decided by comparison with the edges; -0.0 is in the bin of 0.
 *   below[row]: pairs with q < -2000 (-inf too); above[row]: q > 950 (+inf too); nan[row]: q is NaN.
 *   n[row]: the selected points of the population; hist + below + above + nan == n * n.
 *   max[row]: np.max of the population's pairs (:32) — NaN if one of them is NaN, else the largest (+inf included; a zero maximum
 *   is +0.0, the diagonal's value); NaN for an empty population.
 * status[f]: 0; MVOSR_ST_DC_NO_POINT — no point of population 0 is selected (np.max raises there): zero counts, NaN maxima —;
 * MVOSR_ST_ERR_MASK — a level above 2, a negative offset or length, or more entries than params->max_feat: zero counts, n = 0,
 * NaN maxima, nothing added to the tables.
 * tables (optional): int64 [3][MVOSR_DC_TABLE_WORDS] in device memory, owned and zeroed by the caller, kept across launches: the
 * 59 bins, then below, above, nan, of every frame with status 0 are ADDED to it.
 * A frame spans as many workgroups as its n^2 pairs ask for (mvosr_depthcheck_plan.hpp): params->max_feat sizes the grid, there
 * is no cap on a frame's features from LDS.  Counts are combined by integer atomics, the maximum as an integer key over the
 * non-NaN values: no floating-point atomics, the same bytes every run.  The per-frame outputs are zeroed by the call itself, on
 * the context's stream.  n_frames <= 0: MVOSR_OK, nothing launched.  MVOSR_ERR_ARG: a null argument other than cnt / tables, or
 * max_feat < 0; MVOSR_ERR_TOO_LARGE: more than 2^31-1 frames, or a frame that would need more than 65535 workgroups.
 */
#define MVOSR_DC_BINS 59
#define MVOSR_DC_TABLE_WORDS 62  /* MVOSR_DC_BINS, then below, above, nan */
#define MVOSR_ST_DC_NO_POINT 12  /* no point of population 0 with y > 0 */
typedef struct mvosr_depth_check_params {
    int32_t max_feat;            /* the largest feat_cnt of the launch: sizes the grid */
    int32_t reserved;            /* 0 */
} mvosr_depth_check_params;
typedef struct mvosr_depth_check_outputs {
    int64_t *hist;               /* [F][3][MVOSR_DC_BINS] */
    int64_t *below, *above, *nan;/* [F][3] */
    double *max;                 /* [F][3] */
    int64_t *n;                  /* [F][3] */
    int32_t *status;             /* [F] */
} mvosr_depth_check_outputs;
int mvosr_depth_check_batch(mvosr_ctx *ctx, int64_t n_frames, const int64_t *off, const int32_t *cnt, const double *y,
                            const double *z, const uint8_t *level, const mvosr_depth_check_params *params,
                            const mvosr_depth_check_outputs *outputs, int64_t *tables);

/*
 * Scoring the repeated runs (/root/reference/test_off_line.sh:11-23): the paths of C cases, their KITTI segment errors against a
 * ground-truth path (script/evaluate_vo.py:5-96) and pose2motion with its two users (script/transformation.py:23-32,
 * change_scale.py:12-18, calculate_speed.py:8-11).  Every array is a device array of doubles unless stated; a pose or a motion
 * is 12 doubles, the upper 3 x 4 of [R t; 0 1].  fp64, no contraction, no floating-point atomics: the same bytes every run, and
 * a case's results do not depend on the cases beside it.
 * Operation orders.  Product: (A B)[r][j] = ((A[r][0] B[0][j] + A[r][1] B[1][j]) + A[r][2] B[2][j]) + A[r][3] B[3][j], with B's
 * last row 0 0 0 1 written out.  Inverse: of the affine matrix as it is — R^-1 = adj(R) / det(R), det by the first row
 * ((R00 C00 + R01 C10) + R02 C20), then -(R^-1 t) with the same k-ascending sum; never R^T.  Norm: sqrt((x x + y y) + z z).
 *
 * mvosr_paths_batch (paths_kernel; main_offline.py:100-119): motions [n][12], scales [C][n] or NULL (ones) -> poses [C][n + 1][12],
 * row 0 the identity, row i + 1 = row i * step_i strictly left to right, step_i = motions[i] with its translation multiplied by
 * scales[c][i] first (one rounding).  case_stride = 0: every case integrates the same motions; else case c reads its own
 * motions + c * case_stride doubles (>= 12 n; what pose2motion wrote).  n = 0: the identity rows.  MVOSR_ERR_ARG: null ctx / poses,
 * null motions with n > 0, n < 0, C < 1, 0 < case_stride < 12 n.
 *
 * mvosr_segment_table (segment_table_kernel; evaluate_vo.py:5-19, 52-65) of a ground-truth path poses_gt [n_poses][12]:
 *   dist [n_poses]: dist[0] = 0, dist[i] = dist[i - 1] + |t[i - 1] - t[i]|, summed left to right.
 *   last [F][MVOSR_SCORE_LENGTHS] int32, F = mvosr_score_firsts(n_poses) = ceil(n_poses / MVOSR_SCORE_STEP): for first = 10 f and
 *   length = 100 (l + 1) the first i >= first with dist[i] > dist[first] + length (strict), else -1 — found by binary search, which
 *   is the reference's scan where dist never decreases (it cannot, unless a norm is NaN).  Not compacted.
 *   gdelta [F][8][24]: inv(G_first) G_last as an unevaluated sum of two doubles — 12 high parts, then 12 low parts — computed in
 *   double-double (error-free products and sums); high parts NaN where there is no segment.
 *   status [1] int32: 0, or MVOSR_ST_ERR_SINGULAR — the rotation block of a segment's first pose is all zeros (the reference's .I
 *   raises LinAlgError).  Other singular or near-singular blocks are not detected: the result is what the division gives.
 * MVOSR_ERR_ARG: a null argument, n_poses < 1.
 *
 * mvosr_score_cases_batch (score_cases_kernel; evaluate_vo.py:64-96), one workgroup per case: paths [C][rows][12], the table of
 * n_first firsts.  For every (case, first, length) with last >= 0: q = inv(P_first) P_last, e = inv(q) g,
 * r_err = acos(max(min(0.5 (((e00 + e11) + e22) - 1), 1), -1)), t_err = sqrt((e03^2 + e13^2) + e23^2) — q, e, the trace and the sum
 * of squares in double-double from the float64 poses, rounded to a double once in front of acos and sqrt: acos of a small angle
 * multiplies the roundings of the trace by 1 / sin(r_err), and in plain doubles the kernel's own noise would equal the reference's.
 *   r_seg, t_seg (each optional) [C][n_first][8]: r_err / length, t_err / length; NaN where there is no segment.
 *   means [C][2][8]: per length the sum of r_seg (row 0) / t_seg (row 1) over the segments in ascending first, left to right from
 *   the first term, divided by their number; NaN for a length without segments.  counts [C][8] int32.
 *   status [C] int32: 0; MVOSR_ST_ERR_SINGULAR — an all-zero rotation block in a P_first or a q; MVOSR_ST_ERR_MASK — a segment
 *   names a row >= rows (the path is shorter than the table's ground truth): such a segment is NaN and no pose of it is read.
 * MVOSR_ERR_ARG: a null argument other than r_seg / t_seg (last / gdelta may be null where n_first = 0), C < 1, rows < 1.
 *
 * mvosr_pose2motion_batch (pose2motion_kernel), one lane per (path, frame): poses [C][n + 1][12] ->
 *   motions (optional) [C][n][12] = inv(P_i) P_{i+1}; with speed [n] given, each translation replaced by
 *   (speed[i] * t) / (|t| + 0.00001) (change_scale.py:15-17; |t| of the translation before the change).
 *   norms (optional) [C][n] = |t| (calculate_speed.py:9-11).
 *   status [C] int32: 0, or MVOSR_ST_ERR_SINGULAR (an all-zero rotation block in a P_i).
 * n = 0: status zeroed, nothing launched.  MVOSR_ERR_ARG: null ctx / poses / status, neither output given, n < 0, C < 1;
 * MVOSR_ERR_TOO_LARGE above 65535 paths.
 */
#define MVOSR_SCORE_LENGTHS 8    /* 100, 200 .. 800 m */
#define MVOSR_SCORE_STEP 10
int64_t mvosr_score_firsts(int64_t n_poses);
int mvosr_paths_batch(mvosr_ctx *ctx, int64_t n, int64_t n_cases, const double *motions, int64_t case_stride, const double *scales,
                      double *poses);
int mvosr_segment_table(mvosr_ctx *ctx, int64_t n_poses, const double *poses_gt, double *dist, int32_t *last, double *gdelta,
                        int32_t *status);
int mvosr_score_cases_batch(mvosr_ctx *ctx, int64_t n_cases, int64_t rows, const double *paths, int64_t n_first, const int32_t *last,
                            const double *gdelta, double *r_seg, double *t_seg, double *means, int32_t *counts, int32_t *status);
int mvosr_pose2motion_batch(mvosr_ctx *ctx, int64_t n_cases, int64_t n, const double *poses, const double *speed, double *motions,
                            double *norms, int32_t *status);

/*
 * Scoring the scales (/root/reference/script/evaluate_scale.py, run by tesh.sh:4-8 on every scales file against the ground truth's
 * speed file).  Device arrays of doubles unless stated; windows and thresholds are HOST arrays.  Every float is the reference's
 * own double: single IEEE operations, and sums in np.add.reduce's order (pairwise: below 8 a plain loop, up to 128 eight
 * accumulators, above that halves with the first rounded down to a multiple of 8; lists above 8192 in chunks added left to right).
 *
 * mvosr_scale_errors_batch (scale_errors_kernel; evaluate_scale.py:4-13 with patch, :19-23), C cases in one launch: gt [n_gt],
 * scales [C][case_stride] of which n are used, e = gt[i] - scales[c][i], a = |e|.
 *   stats [C][2]: np.mean(a), np.max(a) — NaN where an a is NaN.
 *   counts [C][n_thresholds] int32: sum(a > thresholds[k]); the shares 1 - count / n are the caller's.
 *   drift [C][n_windows]: for window w the np.mean over i = 0, step, 2 step .. < n - w of |np.sum(e[i : i + w])| / w; NaN where
 *   n - w <= 0 (np.mean of an empty list).
 *   status [C] int32: 0, or MVOSR_ST_ERR_EMPTY for n = 0 — mean and max NaN, counts zero (the reference's np.max raises).
 * A case's errors and a window's segment values live in LDS up to 5120 scales and 1024 segments, in the context's scratch beyond;
 * MVOSR_SCALE_ERRORS_GLOBAL in flags asks for the second form at any size.  Both give the same bytes.
 * MVOSR_ERR_ARG: a null argument that is needed, n < 0, n > n_gt (the reference's subtraction fails to broadcast), C < 1,
 * case_stride < n, more than MVOSR_SCALE_MAX_WINDOWS windows or MVOSR_SCALE_MAX_THRESHOLDS thresholds, a window outside 1..8192,
 * step < 1.  MVOSR_ERR_TOO_LARGE: more than 2^31-1 scales or 65535 cases.
 *
 * mvosr_window_median_cases (window_median_cases_kernel; evaluate_scale.py:24-28, filter), C sequences in one launch:
 * out[c][i] = np.median(data[c][max(i - window + 1, 0) : i + 1]) — mvosr_window_median's median with an empty queue; rows
 * case_stride / out_stride doubles apart.  MVOSR_ERR_ARG: null data / out with n > 0, window outside 1..64, n < 0, C < 1, a stride
 * below n.
 */
#define MVOSR_SCALE_MAX_WINDOWS 16
#define MVOSR_SCALE_MAX_THRESHOLDS 8
#define MVOSR_SCALE_ERRORS_GLOBAL 1
int mvosr_scale_errors_batch(mvosr_ctx *ctx, int64_t n_gt, const double *gt, int64_t n_cases, int64_t n, const double *scales,
                             int64_t case_stride, int n_windows, const int32_t *windows, int step, int n_thresholds,
                             const double *thresholds, int flags, double *stats, int32_t *counts, double *drift, int32_t *status);
int mvosr_window_median_cases(mvosr_ctx *ctx, const double *data, int64_t n_cases, int64_t n, int64_t case_stride, int window,
                              double *out, int64_t out_stride);

/*
 * The cross-frame tail of scale_calculation_ransac (rescale.py:169-178) over a run of frames, on the device: the slew
 * limiter — a frame with apply[i] != 0 moves the running scale towards raw[i] by at most `slew` (0.3), any other frame
 * leaves it — followed by the window median of the pushed values (np.median(self.scale_queue)).  raw/apply/pushed/
 * filtered are device arrays of n; scale_in and queue_in[0..n_queue) (HOST pointer) are the estimator's state before the
 * run.  apply: int32, non-zero where the frame has a RANSAC model (status 0).  One wavefront walks the sequence (the
 * limiter is a sequential recurrence of rounded additions), the median is mvosr_window_median's kernel.
 */
int mvosr_slew_median(mvosr_ctx *ctx, const double *raw, const int32_t *apply, int64_t n, double slew, double scale_in,
                      int window, const double *queue_in, int n_queue, double *pushed, double *filtered);

/* The same on HOST arrays, without the GPU: the recurrence is sequential, and when the per-frame results are on the host
 * anyway (the estimator needs the statuses there to raise where the reference does) one core walks a million frames in a
 * few milliseconds — the device kernel's single wavefront needs 55 ns per frame.  scale_out (optional): the running scale
 * after the run. */
int mvosr_slew_median_host(const double *raw, const int32_t *apply, int64_t n, double slew, double scale_in, int window,
                           const double *queue_in, int n_queue, double *pushed, double *filtered, double *scale_out);

/*
 * The legacy per-triangle batch of /root/reference/src/triangle_batch.py:14-68: features are
 * [u, v, depth] (b->x = u, b->v = v, b->z = depth; b->tri1 = Delaunay over (u,v), :23-25).  Per
 * triangle: back-projection with (focus, cx, cy) (:32-33), n = A^-1.1 (:36-37), s = n_y/|n| (:43),
 * h = mean y (:40); keep s > s_min (0.98) and h > 0 (:54-55); mean/std (:57-58); drop values outside
 * mean +- n_sigma (3) std (:60-61); height[f] = mean of the rest (:62).  counts [F][2] = kept / kept
 * after the clip; status [F] = 0, MVOSR_ST_ERR_SINGULAR, _MASK or _EMPTY.  b->max_feat sizes the launch's LDS: a frame
 * with feat_cnt[f] > b->max_feat (possible only where the counts live in device memory) is refused with MVOSR_ST_ERR_MASK,
 * NaN height and counts (0, 0); the frames around it are processed as usual.
 */
int mvosr_triangle_batch(mvosr_ctx *ctx, const mvosr_batch *b, double focus, double cx, double cy, double s_min,
                         double n_sigma, double *height, int32_t *counts, int32_t *status);

/* get_inliers, /root/reference/src/estimate_road_norm.py:71-78: mask[i] = |n.p_i + d| < threshold for a
 * plane model4 = (n, d) given on the HOST; px/py/pz/mask are device arrays of n elements. */
int mvosr_plane_inliers(mvosr_ctx *ctx, int64_t n, const double *px, const double *py, const double *pz, const double *model4,
                        double threshold, uint8_t *mask);

/* ---- the per-frame camera-height and road-pitch estimator (/root/reference/src/calculate_height_pitch.py) ---------- */

typedef struct mvosr_height_pitch_params {
    double focus, cx, cy;        /* 718.856, 607.1928, 185.2157 (calculate_height_pitch.py:15-17) */
    int32_t min_points;          /* 12: fewer list points and the frame is not fitted (:140); >= 3 */
    int32_t n_hyp;               /* 500 (:145); <= 512 */
    double threshold;            /* 0.005: a hypothesis' inliers among the list (:145) */
    double goal_fraction;        /* 0.8 (/root/reference/src/estimate_road_norm.py:68) */
    double inlier_threshold;     /* 0.01: the best plane's inliers among ALL points (:149) */
    uint64_t seed;               /* key of the sample sequence when `triples` is NULL */
    int64_t frame_base;          /* counter of frame 0 of the batch in the sample sequence (frame f: frame_base + f) */
} mvosr_height_pitch_params;

/* per-frame outputs of mvosr_height_pitch_batch (device pointers; the optional ones may be NULL) */
typedef struct mvosr_height_pitch_outputs {
    double *ransac_height;       /* [F] 1 / (|n| / h_bar) of the best plane (:154-166) */
    double *model;               /* [F][4] unit (n, d) of the best plane, n_y >= 0 (:157-159) */
    int32_t *best_ic, *used;     /* [F] inlier count of the best hypothesis, hypotheses consumed (ransac.py:9-22) */
    int32_t *n_selected;         /* [F] length of the point list, 3 per kept row: the script's "suitable point" (:135) */
    int32_t *n_inliers;          /* [F] points within inlier_threshold of the best plane (:172) */
    double *refined_normal;      /* [F][3] unit normal of the plane through the first three inliers, n_y >= 0 (:178-186) */
    double *refined_pitch;       /* [F] asin(n_y) of it (:188) */
    double *refined_mean, *refined_std;   /* [F] mean and (population) std of inliers . normal (:192-195) */
    double *height_t_mean;       /* [F] mean of z sin + y cos over the inliers, with the PRIOR's angle (:202-203) */
    int32_t *status;             /* [F] 0, MVOSR_ST_RS_FEW, MVOSR_ST_ERR_SINGULAR, _MASK, _EMPTY */
    uint8_t *mask;               /* optional [laid out like z] 1 = inlier (:149); written for frames with status 0 only */
    int32_t *point_list;         /* optional: frame f's list at point_list + 3 * tri1_off[f], n_selected[f] vertex ids (:114-116) */
    int32_t *hyp_counts;         /* optional [F][n_hyp] inlier count of every hypothesis; written for fitted frames only */
} mvosr_height_pitch_outputs;

/*
 * The body of calculate_height_pitch.py's frame loop (:62-204) for every frame, one workgroup each, ONE launch
 * (height_pitch_kernel): the frame's points, list, hypotheses and inlier mask never leave LDS.
 * b: x = u, v = v, z = depth (the [u, v, depth] rows of the script's dumps), tri1 = Delaunay(u, v).simplices with tri1_off, or
 * tri1_off + tri1_cnt, as mvosr_triangle_batch reads them.  frame_prior [F][4] (device): est_deg - 95, est_deg - 85 — the window's
 * edges in degrees as the script forms them, est_deg = estimated_pitch * 180 / 3.1415926 (:63, :111) —, then math.sin and math.cos
 * of estimated_pitch (:202): the host's doubles, so that no device sin or cos enters a result.
 *   Points: (depth * (u - cx) / focus, depth * (v - cy) / focus, depth) (:67-68).  Per row: n = A^-1 . 1 (LU with partial pivoting, as
 *   mvosr_triangle_batch), height = 1 / |n|, both negated when n_y < 0, pitch_deg = asin(-n_y / |n|) * 180 / 3.1415926 (:83-91); a
 *   row is kept when low < pitch_deg < high and height > 0 (:111-112).  The comparison is made on -n_y / |n| against the edges'
 *   sines; within 1e-12 of one the script's own expression decides.  A NaN edge keeps nothing.
 *   The list: the kept rows' three ids in row order, repeats included (:114-116); fewer than min_points entries: MVOSR_ST_RS_FEW.
 *   RANSAC over the list's points (:145): hypothesis h is the plane through the list entries at positions triples[f][h][0..2], as
 *   the unit 4-vector (n, d); its count is the number of list entries with |m . [p, 1]| < threshold; the replay rule is
 *   mvosr_ransac_plane_batch's (first best, stop at the first best above goal_fraction * list length).  A sample that names a
 *   position outside the list, or one VERTEX twice, is spent: NaN plane, count 0 (mvosr_flat_ransac_batch's rule; the script's SVD
 *   returns an arbitrary plane of the pencil there).  triples == NULL: the positions are mvosr_flat_ransac_batch's counter-based
 *   draw from (seed, frame_base + f, h).  No hypothesis with an inlier: MVOSR_ST_RS_FEW (the script has no model either).
 *   Inliers: every point of the frame with |n . p + d| < inlier_threshold, in feature order (:149-150).
 *   ransac_height = 1 / (sqrt(n . n) / -d) with n_y >= 0 (:154-166).
 *   Refinement: n^ = the unit normal of the plane through the first three inliers, (p1 - p0) x (p2 - p0) normalised, n^_y >= 0 — the
 *   null vector the script's SVD of [p, 1] yields, up to rounding (:178-186) —; refined_pitch = asin(n^_y); refined_mean / _std over
 *   ((x n^_x + y n^_y) + z n^_z) of the inliers; height_t_mean = mean(z sin + y cos).  Fewer than three inliers: these are NaN.
 *   Sums: per thread over its points ascending, then lanes, then wavefronts, in a fixed order — a frame's results are bit-identical
 *   from run to run, alone or in a batch.
 * A frame that is not fitted (any status but 0) has NaN in every double output, 0 in best_ic / n_inliers (and in used, except
 * where every hypothesis was spent), and n_selected = the list's length for MVOSR_ST_RS_FEW, else 0.
 * b->max_feat sizes the launch's LDS, for max_tri = 2 * b->max_feat rows (at least 1): a frame with feat_cnt[f] > b->max_feat or
 * more rows is refused before LDS is touched (MVOSR_ST_ERR_MASK); a vertex id outside [0, feat_cnt[f]) gives MVOSR_ST_ERR_MASK,
 * a zero pivot MVOSR_ST_ERR_SINGULAR (the script raises LinAlgError, :83), no features or no rows MVOSR_ST_ERR_EMPTY.
 * LDS: mvosr_height_pitch_lds_bytes(max_feat, n_hyp) = 24 N + 12 N + 36 n_hyp + N / 8 + ~500 bytes (91 KB for 2 000 features
 * and 500 hypotheses: one workgroup of 8 wavefronts per CU); beyond the device's limit, or with max_feat > 10 922 (16-bit list
 * positions), MVOSR_ERR_TOO_LARGE.
 */
int mvosr_height_pitch_batch(mvosr_ctx *ctx, const mvosr_batch *b, const mvosr_height_pitch_params *p, const double *frame_prior,
                             const int32_t *triples, const mvosr_height_pitch_outputs *o);
size_t mvosr_height_pitch_lds_bytes(int max_feat, int n_hyp);

/* ---- the estimator's frame-to-frame carry (calculate_height_pitch.py:140, :163-167, :202-203) for a chunk of frames ---------- */

/* one frame of a chunk, as the script's lists take it (56 bytes) */
typedef struct mvosr_height_pitch_tail_frame {
    double ransac_height, refined_mean, refined_std, height_t_mean, refined_pitch;
    int32_t n_inliers;           /* with the five doubles: the six values of the script's result files */
    int32_t n_selected;          /* the frame's own list length */
    int32_t carried;             /* 1: fewer than min_points list points, the values are the previous frame's (:163-165) */
    int32_t source;              /* the last fitted frame of the chunk at or before this one; -1: none, the carry-in's */
} mvosr_height_pitch_tail_frame;

/* the header of a carry record (64 bytes); behind it, at the offsets mvosr_height_pitch_carry_bytes' layout gives for the
 * record's capacity `cap` rounded up to even: y[cap] at 64, z[cap] at 64 + 8 cap (doubles), index[cap] at 64 + 16 cap (int32) —
 * the back-projected Y and Z (:68, :66) and the feature indices of the last fitted frame's inliers, in feature order */
typedef struct mvosr_height_pitch_carry {
    double ransac_height, refined_mean, refined_std, height_t_mean, refined_pitch;
    int32_t n_inliers;           /* ... the previous frame's six values (its height_t_mean enters no result) */
    int32_t has_prev;            /* 0: no frame yet — a carried frame raises (:167) */
    int32_t count;               /* entries of y, z and index */
    int32_t halted;              /* 1: a chunk before this one ended in an error; every later tail passes the record on untouched */
    int64_t reserved;
} mvosr_height_pitch_carry;

enum mvosr_hpt_error {           /* the high half of the error word, in the host loop's order of precedence per frame */
    MVOSR_HPT_ERR_SINGULAR = 1,  /* MVOSR_ST_ERR_SINGULAR: the script raises LinAlgError (:83) */
    MVOSR_HPT_ERR_MASK = 2,      /* MVOSR_ST_ERR_MASK */
    MVOSR_HPT_ERR_EMPTY = 3,     /* MVOSR_ST_ERR_EMPTY */
    MVOSR_HPT_ERR_NO_MODEL = 4,  /* MVOSR_ST_RS_FEW with n_selected >= min_points: no sample of the RANSAC had an inlier */
    MVOSR_HPT_ERR_NO_PREVIOUS = 5, /* a carried frame with no frame before it: the script's IndexError (:167) */
    MVOSR_HPT_ERR_STATUS = 6,    /* a status the estimator does not know, or status 0 on a frame outside (0, max_feat] */
    MVOSR_HPT_ERR_UPSTREAM = 7   /* the carry-in is halted (or its count exceeds carry_cap): no frame of this chunk is final */
};

/*
 * The body of the estimator's host loop for one chunk of frames in sequence order, behind mvosr_height_pitch_batch on the
 * context's stream: two launches (hpt_resolve_kernel: one workgroup; hpt_carry_kernel: n_frames + 1 workgroups), no host
 * synchronisation.  b: n_frames, feat_off, feat_cnt, v, z (depth) and max_feat as mvosr_height_pitch_batch read them; p: focus,
 * cy, min_points; frame_prior: the same [F][4]; o: that launch's outputs, the mask included (all device pointers).
 *   A frame with status 0 is final as the kernel wrote it.  A frame with MVOSR_ST_RS_FEW and n_selected < min_points is CARRIED:
 *   it copies ransac_height, refined_mean, refined_std, refined_pitch and n_inliers of the most recent frame before it (in the
 *   chunk, or the carry-in's), keeps its own n_selected, and its height_t_mean is np.mean(Z sin + Y cos) over the inliers of the
 *   most recent FITTED frame with its OWN prior's sin and cos (frame_prior[f][2..3]): Y = depth * (v - cy) / focus, the products and
 *   the sum rounded separately, the terms in feature order, the sum in np.add.reduce's pairwise order, divided by the count — the
 *   host's double to the last bit.
 *   *error (int64): -1, or kind << 32 | the first frame at which the host must raise (an mvosr_hpt_error; per frame singular, mask /
 *   empty, no model, then a carried frame with no previous).  Frames from that one on are not final.
 *   carry_out: the state after the last frame before the error, or after the chunk's last frame — the next chunk's carry_in; halted
 *   when the chunk had an error.  A halted carry_in is copied to carry_out, *error = MVOSR_HPT_ERR_UPSTREAM << 32, frames untouched.
 * carry_in != carry_out, both mvosr_height_pitch_carry_bytes(carry_cap) bytes; max_feat <= carry_cap <= 8192 (one buffer of
 * np.add.reduce), else MVOSR_ERR_ARG / MVOSR_ERR_TOO_LARGE.  LDS: mvosr_height_pitch_tail_lds_bytes(carry_cap) = 8 carry_cap +
 * ~2.2 KB.  The results do not depend on how a sequence is cut into chunks.
 */
int mvosr_height_pitch_tail_batch(mvosr_ctx *ctx, const mvosr_batch *b, const mvosr_height_pitch_params *p, const double *frame_prior,
                                  const mvosr_height_pitch_outputs *o, const void *carry_in, void *carry_out, int32_t carry_cap,
                                  mvosr_height_pitch_tail_frame *frames, int64_t *error);
size_t mvosr_height_pitch_tail_lds_bytes(int max_feat);
size_t mvosr_height_pitch_carry_bytes(int carry_cap);

/* ---- the RANSAC evaluation runs (/root/reference/src/calculate_height_pitch_eval.py, calculate_height_pitch_eval_line.py) ---- */

enum mvosr_hp_model {
    MVOSR_HP_MODEL_PLANE = 0,    /* _eval.py: get_pitch_ransac over the list's (x, y, z), estimate for the refinement       */
    MVOSR_HP_MODEL_LINE = 1      /* _eval_line.py: get_pitch_line_ransac over the list's (y, z), estimate_line              */
};

/* status of a fitted (frame, case) whose refinement sample — the first three (plane) or two (line) list inliers — names fewer
 * vertices than it has entries: the script's SVD returns rounding noise there.  Additive: no other status has this bit. */
#define MVOSR_ST_HP_REFINE_DEGENERATE 0x100

typedef struct mvosr_height_pitch_eval_params {
    double focus, cx, cy;        /* as mvosr_height_pitch_params */
    int32_t min_points;          /* 12 (_eval.py:159); >= 3 */
    int32_t n_hyp;               /* the scripts' iter_number (argv[4]); <= 4096, processed in tiles of 512 */
    double threshold;            /* 0.005 (:164) */
    double goal_fraction;        /* 0.8 */
    double inlier_threshold;     /* 0.01: the best model's inliers among the LIST (:167) */
    uint64_t seed;               /* key of the sample sequence when `samples` is NULL */
    int64_t frame_base;          /* counter of frame 0 of the batch in the sample sequence */
    int32_t model;               /* enum mvosr_hp_model */
    int32_t n_cases;             /* the scripts' ten (`for case_i in range(0,10)`); 1..1024 */
    int32_t cases_per_group;     /* cases one workgroup runs with its frame resident; 0: the library's default (1, as measured) */
} mvosr_height_pitch_eval_params;

/* outputs of mvosr_height_pitch_eval_batch (device pointers; C = n_cases; the optional ones may be NULL) */
typedef struct mvosr_height_pitch_eval_outputs {
    double *ransac_height;       /* [F][C] 1 / (|n| / h_bar) of the best model (:175-187); the line's may be negative */
    double *model;               /* [F][C][4] plane: unit (n, d), n_y >= 0; line: unit (a, b, 0, c) of a y + b z + c = 0, b >= 0 */
    int32_t *best_ic, *used;     /* [F][C] */
    int32_t *n_selected;         /* [F] length of the point list (the same for every case) */
    int32_t *n_inliers;          /* [F][C] LIST entries within inlier_threshold of the best model, repeats counted (:193) */
    double *refined_normal;      /* [F][C][3] plane: as mvosr_height_pitch_outputs; line: (0, n_y, n_z), n_z >= 0 */
    double *refined_pitch;       /* [F][C] asin(n_y) */
    double *refined_mean, *refined_std;   /* [F][C] over the list inliers, with multiplicity */
    double *height_t_mean;       /* [F][C] */
    double *sum_y, *sum_z;       /* [F][C] sums of y and z over the list inliers: a carried frame's height_t_mean under a new prior */
    int32_t *status;             /* [F][C] 0, MVOSR_ST_HP_REFINE_DEGENERATE, MVOSR_ST_RS_FEW, MVOSR_ST_ERR_SINGULAR, _MASK, _EMPTY */
    uint8_t *list_mask;          /* optional: 1 = list inlier; case c of frame f at c * list_stride + 3 * tri1_off[f], n_selected[f] bytes */
    int64_t list_stride;         /* bytes per case of list_mask: at least 3 * tri1_off[F] */
    int32_t *point_list;         /* optional: as mvosr_height_pitch_outputs */
    int32_t *hyp_counts;         /* optional [F][C][n_hyp]; written for fitted frames only */
} mvosr_height_pitch_eval_outputs;

/*
 * The bodies of both evaluation scripts' frame loops for every frame and every case in ONE launch
 * (height_pitch_eval_kernel<model>): grid = frames x ceil(n_cases / cases_per_group) workgroups; a workgroup runs steps (1)-(2)
 * of mvosr_height_pitch_batch once — the same statuses and refusals, written to every case — and then, for each of its cases,
 *   hypotheses: samples[f][c][h][0..2] (the line reads two) are list positions; NULL: a counter-based draw from
 *   (seed, frame_base + f, c, h) — key = mix(mix(seed ^ (frame_base + f) * 0xD1B54A32D192ED03) ^ (c + 1) * 0xA0761D6478BD642F),
 *   then mvosr_height_pitch_batch's triple, or its first two positions for the line — which depends neither on the batch nor on
 *   cases_per_group.  A position outside the list or a vertex named twice: spent.  The plane is mvosr_height_pitch_batch's; the
 *   line is mvosr_ransac_line_batch's through (y, z) of the two vertices, its residual (y a + z b) + c.  Counts over the list at
 *   `threshold`; the replay rule carried over tiles of 512 hypotheses.  No hypothesis with an inlier: MVOSR_ST_RS_FEW for the case.
 *   Inliers: the LIST entries within inlier_threshold of the best model, in list order, repeats included (:167-169).
 *   ransac_height: plane — flipped on n_y < 0, -d / |n|; line — (a, b) and h_bar = -c flipped on b < 0, h_bar / sqrt(a^2 + b^2).
 *   Refinement: plane — as mvosr_height_pitch_batch over the first three list inliers; line — the normal (z1 - z0, -(y1 - y0)) of the
 *   line through the first two, flipped when its z component is < 0, normalised; refined_pitch = asin of its y component; distances
 *   y n_y + z n_z.  Sums per thread over its list positions ascending, then lanes, then wavefronts.  A sample that names a vertex
 *   twice (or has too few entries): MVOSR_ST_HP_REFINE_DEGENERATE, refined_normal / _pitch / _mean / _std and height_t_mean NaN;
 *   everything else is written.
 * LDS: mvosr_height_pitch_eval_lds_bytes(max_feat, n_hyp, model) = 24 N + 12 N + 36 min(n_hyp, 512) + 3 N / 4 + ~700 bytes: it
 * does not grow with n_cases.  Limits as mvosr_height_pitch_batch; frames x groups < 2^31.
 */
int mvosr_height_pitch_eval_batch(mvosr_ctx *ctx, const mvosr_batch *b, const mvosr_height_pitch_eval_params *p, const double *frame_prior,
                                  const int32_t *samples, const mvosr_height_pitch_eval_outputs *o);
size_t mvosr_height_pitch_eval_lds_bytes(int max_feat, int n_hyp, int model);

/* outputs of mvosr_height_pitch_eval_budgets_batch (device pointers; C = n_cases, B = n_budgets, H = the last budget; the optional
 * ones may be NULL): per quantity of mvosr_height_pitch_eval_outputs one value per (frame, case, budget) */
typedef struct mvosr_height_pitch_eval_budgets_outputs {
    double *ransac_height;       /* [F][C][B] */
    double *model;               /* [F][C][B][4] */
    int32_t *best_ic, *used;     /* [F][C][B]; used: budgets[k] unless the goal stop came earlier */
    int32_t *n_selected;         /* [F] length of the point list (the same for every case and budget) */
    int32_t *n_inliers;          /* [F][C][B] */
    double *refined_normal;      /* [F][C][B][3] */
    double *refined_pitch;       /* [F][C][B] */
    double *refined_mean, *refined_std;   /* [F][C][B] */
    double *height_t_mean;       /* [F][C][B] */
    double *sum_y, *sum_z;       /* [F][C][B] */
    int32_t *status;             /* [F][C][B] as mvosr_height_pitch_eval_outputs */
    int32_t *best;               /* [F][C][B] the hypothesis number of the best model among the first budgets[k]; -1: none */
    int32_t *point_list;         /* optional: as mvosr_height_pitch_outputs */
    int32_t *hyp_counts;         /* optional [F][C][H]; written for fitted frames only */
} mvosr_height_pitch_eval_budgets_outputs;

/*
 * mvosr_height_pitch_eval_batch at every iteration budget of a list in ONE launch (height_pitch_eval_budgets_kernel<model>; grid
 * and workgroup as height_pitch_eval_kernel).  budgets: int32[n_budgets] on the HOST, 1 <= n_budgets <= 16, strictly ascending,
 * budgets[0] >= 1 and the last <= 4096; anything else: MVOSR_ERR_ARG, nothing is launched.  H = the last budget.  p->n_hyp is
 * IGNORED (not read); every other member of p means what it means to mvosr_height_pitch_eval_batch.  samples: NULL (the device
 * draws) or [F][C][H][3].
 * Contract: for every k, slot [f][c][k] of every output that mvosr_height_pitch_eval_batch also has holds, BYTE FOR BYTE, what
 * that entry point writes at [f][c] when called with n_hyp = budgets[k] and the same batch, params, seed, frame_base and priors
 * (with samples: the first budgets[k] samples of each (frame, case)) — `used` (budgets[k] unless the goal stop came earlier), the
 * MVOSR_ST_RS_FEW case where none of the first budgets[k] hypotheses has an inlier (doubles NaN, counts 0, used = budgets[k],
 * best = -1) and the MVOSR_ST_HP_REFINE_DEGENERATE bit included.  n_selected and point_list are those of any of these calls,
 * hyp_counts the call's at H.  A frame that is not fitted (empty; feat_cnt > max_feat or more rows than 2 max_feat, refused
 * before LDS is touched; an id outside the frame; a singular row; fewer than min_points list entries, n_selected written) has the
 * refusal outputs of mvosr_height_pitch_eval_batch in all B slots of every case, best = -1, and leaves its neighbours alone.
 * Results depend neither on cases_per_group, nor on how a sequence is cut into batches (frame_base), nor on which other budgets
 * are in the list.
 * How: the draw of hypothesis h is keyed by (seed, frame_base + f, c, h) and not by n_hyp, so planes and counts are computed ONCE
 * per (frame, case) for H hypotheses; the replay runs over segments that end at the budgets and its state is kept per budget; the
 * inliers, the refinement and the sums run once per distinct best model among a case's budgets.  With hyp_counts == NULL the tiles
 * behind the goal stop are skipped.
 * LDS: mvosr_height_pitch_eval_budgets_lds_bytes(max_feat, n_hyp_max, n_budgets, model) =
 * mvosr_height_pitch_eval_lds_bytes(max_feat, n_hyp_max, model) + 48 n_budgets.  Limits as mvosr_height_pitch_eval_batch.
 */
int mvosr_height_pitch_eval_budgets_batch(mvosr_ctx *ctx, const mvosr_batch *b, const mvosr_height_pitch_eval_params *p, const int32_t *budgets,
                                          int n_budgets, const double *frame_prior, const int32_t *samples,
                                          const mvosr_height_pitch_eval_budgets_outputs *o);
size_t mvosr_height_pitch_eval_budgets_lds_bytes(int max_feat, int n_hyp_max, int n_budgets, int model);

/* ---- the evaluation runs' cross-frame rules (_eval.py:71-79, :184-188, :223-224) for a chunk of frames ----------------------- */

/* the header of an evaluation carry record (16 bytes).  Behind it, with E = n_cases * n_budgets and element (c, b) at
 * c * n_budgets + b: eight double[E] at 16 + 8 E k — k = 0..5 the six values in the result files' order (ransac_height,
 * refined_mean, refined_std, height_t_mean, refined_pitch, n_inliers), k = 6 sum_y, k = 7 sum_z — and uint8 degenerate[E] at
 * 16 + 64 E: the state after the last frame, the sums and the flag those of the last FITTED frame.  The record is
 * mvosr_height_pitch_eval_carry_bytes(n_cases, n_budgets) bytes (a multiple of 16).  An empty record: has_prev = halted = 0,
 * n_cases and n_budgets filled in, everything behind the header zero. */
typedef struct mvosr_height_pitch_eval_carry {
    int32_t has_prev;            /* 0: no fitted frame yet — a carried frame raises (:188) */
    int32_t halted;              /* 1: a chunk before this one ended in an error; every later tail passes the record on untouched */
    int32_t n_cases, n_budgets;  /* what the record was written for; a tail called with other numbers treats it as halted */
} mvosr_height_pitch_eval_carry;

/* what the evaluation launch wrote (device pointers): mvosr_height_pitch_eval_batch's [F][C] arrays are [F][C][B] with B = 1 */
typedef struct mvosr_height_pitch_eval_tail_inputs {
    const int32_t *n_selected;   /* [F] */
    const int32_t *status;       /* [F][C][B] */
    const double *ransac_height, *refined_mean, *refined_std, *height_t_mean, *refined_pitch;   /* [F][C][B] */
    const int32_t *n_inliers;    /* [F][C][B] */
    const double *sum_y, *sum_z; /* [F][C][B] */
    const int32_t *used, *best;  /* [F][C][B]; each may be NULL: the output of the same name must then be NULL too */
} mvosr_height_pitch_eval_tail_inputs;

/* what the host's run returns (device pointers), [B][C][F] with F = n_frames of the call, frames fastest */
typedef struct mvosr_height_pitch_eval_tail_outputs {
    double *ransac_height, *refined_mean, *refined_std, *height_t_mean, *refined_pitch, *n_inliers;   /* [B][C][F], n_inliers as a double */
    uint8_t *degenerate;         /* [B][C][F] 1: the refined values are NaN (MVOSR_ST_HP_REFINE_DEGENERATE of the frame or of its source) */
    int32_t *used, *best;        /* [B][C][F] optional; a carried frame: 0 and -1 */
    uint8_t *carried;            /* [F] 1: fewer than min_points list points */
    int32_t *frame_class;        /* [F] 0 fitted, -1 carried, else an mvosr_hpt_error kind | budget index << 8 (the index: no-model only) */
    int32_t *source;             /* [F] the last fitted frame of the chunk at or before this one; -1: none, the carry-in's */
    int64_t *error;              /* one word, see below */
} mvosr_height_pitch_eval_tail_outputs;

/*
 * The cross-frame rules of RansacEvaluation.run / RansacBudgetSweep.run for one chunk of frames in sequence order, behind the
 * evaluation launch on the context's stream: three launches (hpe_class_kernel: one wavefront per frame; hpe_resolve_kernel: one
 * workgroup; hpe_apply_kernel: one thread per (frame, case, budget)), no host synchronisation, no atomics.
 *   Class of frame f, from its C * B status words and n_selected[f]: any MVOSR_ST_ERR_SINGULAR -> singular; else any
 *   MVOSR_ST_ERR_EMPTY -> empty, else any MVOSR_ST_ERR_MASK -> mask; else, with n_selected >= min_points, any MVOSR_ST_RS_FEW ->
 *   no-model at the smallest budget index that has one; else a word that is none of 0, MVOSR_ST_HP_REFINE_DEGENERATE,
 *   MVOSR_ST_RS_FEW -> status; else n_selected < min_points -> CARRIED; else FITTED.  A carried frame with no fitted frame before
 *   it in the chunk and has_prev = 0 in the carry-in is the no-previous error.  (The kinds: enum mvosr_hpt_error.)
 *   A fitted frame's element (c, b) takes the launch's six values, degenerate = status & MVOSR_ST_HP_REFINE_DEGENERATE != 0, used and best.
 *   A carried frame's element takes ransac_height, refined_mean, refined_std, refined_pitch, n_inliers and degenerate of its SOURCE —
 *   the last fitted frame before it, in the chunk or the carry-in's — used = 0, best = -1, and
 *   height_t_mean = degenerate ? NaN (0x7ff8000000000000) : (sum_z * sin + sum_y * cos) / (double)n_inliers with the source's sums
 *   and the frame's own frame_prior[f][2], [3]: two products, one sum, one division, each rounded (no fused multiply-add).
 *   *error: -1, or frame | kind << 32 | budget index << 40 for the first frame at which the host must raise (the index: no-model
 *   only, else 0).  Frames from that one on are not written (carried, frame_class and source are).
 *   carry_out: the state after the last frame before the error, or after the chunk's last frame; halted when the chunk had an
 *   error.  A halted carry_in is copied to carry_out, *error = MVOSR_HPT_ERR_UPSTREAM << 32, and nothing else is written; one
 *   written for other n_cases / n_budgets is not read behind its header: the same, with an empty halted record as carry_out.
 * frame_prior: [F][4] as the evaluation launch took it.  carry_in != carry_out.  1 <= n_cases <= 1024, 1 <= n_budgets <= 16,
 * min_points >= 3, n_frames < 2^31 - 64 (else MVOSR_ERR_ARG / MVOSR_ERR_TOO_LARGE); n_frames <= 0: MVOSR_OK, nothing is written.
 * The results do not depend on how a sequence is cut into chunks.
 */
int mvosr_height_pitch_eval_tail_batch(mvosr_ctx *ctx, int64_t n_frames, int32_t n_cases, int32_t n_budgets, int32_t min_points,
                                       const mvosr_height_pitch_eval_tail_inputs *in, const double *frame_prior, const void *carry_in,
                                       void *carry_out, const mvosr_height_pitch_eval_tail_outputs *out);
size_t mvosr_height_pitch_eval_carry_bytes(int n_cases, int n_budgets);

/* ---- dense depth maps from the triangle planes (/root/reference/src/reconstruct.py) ------------------ */

/* The pinhole camera of the reference's PinholeCamera (/root/reference/src/reconstruct.py:21-36 reads these six). */
typedef struct mvosr_camera { int32_t width, height; double fx, fy, cx, cy; } mvosr_camera;

/* Outputs of mvosr_dense_depth_batch (device pointers; the optional ones may be NULL).  F = b->n_frames, H x W the camera's. */
typedef struct mvosr_depth_outputs {
    double  *depth;      /* [F*H*W] row-major per frame; 0 where uncovered                               */
    int32_t *tri_id;     /* optional [F*H*W]: index of the pixel's row within the frame's rows, -1: none */
    double  *tri_model;  /* optional [rows, laid out like the rows][4] = (nx, ny, nz, height), n the unit normal */
    int32_t *covered;    /* optional [F] number of covered pixels                                        */
    int32_t *status;     /* [F] 0, MVOSR_ST_ERR_SINGULAR, _MASK, _EMPTY                                   */
} mvosr_depth_outputs;

/*
 * Reconstruct.triangle_model (/root/reference/src/reconstruct.py:70-90) for every frame: per row of the triangulation
 * `which_tri` (1: b->tri1*, 2: b->tri2*; offsets and optional row counts read as the other entry points read them, so rows
 * written by mvosr_delaunay_batch* go in without visiting the host) A = the three vertices' (x, y, z) in row order — RAW, no
 * remap: reconstruct.py applies none —, n = A^-1.1, height = 1/|n|, n / |n|, both negated when n_y < 0 (:83-85);
 * tri_model[(tri_off[f] + t)*4 ..] = (nx, ny, nz, height).  `keep` (optional, laid out like the planes) has the meaning it has
 * for mvosr_delaunay_batch and mvosr_flat_ransac_batch: the rows' ids are ranks among the points with keep[i] >= 0.
 * status [F]: 0, MVOSR_ST_ERR_SINGULAR (a pivot exactly zero: the reference raises LinAlgError, :78), MVOSR_ST_ERR_MASK (a
 * vertex id out of range — that row's record is zero —, or more than 2 * feat_cnt[f] rows: none is read), MVOSR_ST_ERR_EMPTY.
 */
int mvosr_triangle_model_batch(mvosr_ctx *ctx, const mvosr_batch *b, int which_tri, const int32_t *keep, double *tri_model,
                               int32_t *status);

/*
 * Reconstruct.depth_generate (/root/reference/src/reconstruct.py:91-117) for every frame, as a rasteriser: every pixel
 * (col, row), col = 0..W-1, row = 0..H-1, is located in the triangulation of the frame's pixels (u, v) and gets
 * height / ((nx*px + ny*py) + nz), p = ((col - cx)/fx, (row - cy)/fy, 1) (:31-36, :104; not clamped: a negative or infinite
 * depth is kept), 0 where no triangle covers it.  `u`: the pixel columns, laid out like b->v (as the mvosr_delaunay_* entry
 * points take them).  Point location is the closed, watertight rule: a pixel belongs to a row when its three edge functions,
 * times the row's orientation sign, are >= 0; an edge is evaluated from its lower to its higher vertex id (negated for the
 * triangle that sees it the other way), so the two triangles of an edge get exactly opposite values — no pixel inside the
 * hull is left out by rounding, and only a pixel exactly on an edge is claimed twice —; a pixel claimed by several rows goes
 * to the LOWEST row index.  Results do not depend on scheduling.  (SciPy's find_simplex, which the reference calls, is a
 * directed walk: on such tie pixels it may name the other triangle of the edge.)
 * Two launches on the context's stream: the planes and the rows' screen records (mvosr_triangle_model_batch's kernel), then
 * one workgroup per band of image rows, which writes every byte of its part of depth (and tri_id) exactly once, 16 bytes per
 * store.  covered[f] counts the covered pixels.  first_frame / n_launch restrict the call to a sub-range of the batch
 * (n_launch <= 0: all); the other frames' outputs are not touched.  The context's grow-only workspace holds 212 bytes per
 * element of the planes (b->total_feat) and 8 bytes per image column and row — nothing else is allocated.  A frame may have at most 2 * feat_cnt[f] rows; an image
 * row must fit LDS twice (width <= ~20 000), else MVOSR_ERR_TOO_LARGE.
 */
int mvosr_dense_depth_batch(mvosr_ctx *ctx, const mvosr_batch *b, int which_tri, const double *u, const int32_t *keep,
                            const mvosr_camera *cam, const mvosr_depth_outputs *o, int64_t first_frame, int64_t n_launch);

/* ---- point clouds from the depth images (/root/reference/src/reconstruct.py:108-115) ---------------- */

enum mvosr_cloud_flags {
    MVOSR_CLOUD_RANGE = 1,       /* keep only near <= depth * scale <= far (NaN fails) */
    MVOSR_CLOUD_F32 = 2          /* points and colours as float32: the float64 value, rounded once */
};

/* Device pointers.  depth [F*H*W] as mvosr_dense_depth_batch writes it; tri_id optional [F*H*W]; image optional uint8 [F*H*W*3],
 * BGR as cv2 delivers it; scale optional [F]. */
typedef struct mvosr_cloud_inputs  { const double *depth; const int32_t *tri_id /*opt*/; const uint8_t *image /*opt*/;
                                     const double *scale /*opt [F]*/; int64_t n_frames; } mvosr_cloud_inputs;
typedef struct mvosr_cloud_params  { double near, far; int32_t stride; int32_t flags; } mvosr_cloud_params;   /* MVOSR_CLOUD_RANGE, MVOSR_CLOUD_F32 */
/* points / colors: [capacity][3] float64 (float32 with MVOSR_CLOUD_F32); capacity counts POINTS. */
typedef struct mvosr_cloud_outputs { void *points; void *colors /*opt, requires image*/; int64_t *frame_off /*[F+1]*/;
                                     int32_t *overflow /*[1]*/; int64_t capacity; } mvosr_cloud_outputs;

/*
 * The cloud Reconstruct.depth_generate builds from its depth image (/root/reference/src/reconstruct.py:108-115), for every
 * frame of a batch of depth images, compacted on the device.  Per frame f the pixels (col, row) are visited in raster order
 * (row-major, row outer); a pixel QUALIFIES when it is
 *   covered:      tri_id[f,row,col] >= 0 when tri_id is given, else depth[f,row,col] != 0.0 (NaN counts as covered).  The two
 *                 rules differ only for a covered pixel whose depth is exactly +-0, which needs an infinite normal: the id
 *                 image keeps such a pixel, the depth image alone cannot tell it from an uncovered one;
 *   on the grid:  row % stride == 0 && col % stride == 0 (stride >= 1);
 *   in range:     only with MVOSR_CLOUD_RANGE: dm >= near && dm <= far, so NaN fails;
 * where dm = depth * scale[f] — one multiplication, none when scale is NULL.  Its point is (px*dm, py*dm, dm) with
 * px = (col - cx)/fx, py = (row - cy)/fy (:32, :35, :108; every operation rounded separately), its colour
 * (image[..,2], image[..,1], image[..,0]) / 255.0 (:110).  Output: array of structures [K][3]; the frames' lists lie back to
 * back in frame order; frame_off[f] is the index of frame f's first point, frame_off[F] the total — ALWAYS the true counts,
 * whatever the capacity.  No byte beyond `capacity` points is written; *overflow (optional) = 1 when frame_off[F] > capacity,
 * else 0: read frame_off[F] and call again with that capacity.  capacity = 0 (points may be NULL) only counts.
 * With MVOSR_CLOUD_F32 every output value is the float64 value converted once (what .astype(float32) gives).
 * Three launches on the context's stream (count per segment of 4096 pixels, scan, fill), no atomics on the outputs, no host
 * synchronisation; results do not depend on scheduling.  The context's grow-only workspace holds 4 bytes per segment and
 * frame and 8 per image column and row; a call of a shape seen before allocates nothing.
 * MVOSR_ERR_ARG (before any device work): null ctx / in / cam / p / o / depth / frame_off, stride < 1, colours without an
 * image, negative capacity or frame count, points NULL with capacity > 0, an empty camera.  n_frames == 0: MVOSR_OK.
 * MVOSR_ERR_TOO_LARGE: a side above 2^21 pixels, a frame of 2^31 pixels, or 2^31 segments in one call.
 */
int mvosr_point_cloud_batch(mvosr_ctx *ctx, const mvosr_cloud_inputs *in, const mvosr_camera *cam,
                            const mvosr_cloud_params *p, const mvosr_cloud_outputs *o);

/* ---- optional device stage for the triangulations themselves -------------------- */

enum mvosr_dt_status {
    MVOSR_DT_OK = 0,
    MVOSR_DT_DEGENERATE = 1      /* duplicate / collinear / cocircular points within the guard bands, or a row count that
                                    is not Euler's 2n - 2 - h: rows are not to be used — triangulate this frame on the host */
};

/*
 * Batched 2-D Delaunay triangulation: what scipy.spatial.Delaunay(points).simplices computes at
 * /root/reference/src/scale_calculator.py:257-258 and :266-267, as a device stage.  For points in general position the
 * triangle SET is the one Qhull returns; the rows come in a canonical form — vertex ids ascending inside a row, rows in
 * lexicographic order — a function of the set alone.  Qhull's own rotation of each row, which the reference's vote
 * depends on (:113-115), is not reproducible from the geometry: these rows are meant for MVOSR_VOTE_FIXED, under which
 * they and SciPy's rows give bit-identical results (the host selects both with triangulation="gpu",
 * check_triangle="fixed"); with MVOSR_VOTE_REFERENCE they are a measured deviation.
 * Frame f's points are (u, v)[pts_off[f] .. +pts_cnt[f]); with `keep` (laid out like u; e.g. the vote counters of
 * mvosr_outlier_vote_batch) only the points with keep[i] >= 0 take part and the ids are their ranks among those, in
 * order — the second triangulation over the survivors of the vote (:264-266) without a compaction pass.  n_used[f]
 * (optional) = the number of points triangulated (what mvosr_batch.n2_expected wants).  Rows are written at
 * tri + 3*tri_off[f] (room for 2 * points rows), tri_cnt[f] says how many; status[f] is an mvosr_dt_status (a declined
 * frame has tri_cnt 0 and the reason in the status' bits 8..).  max_pts = max(pts_cnt) <= mvosr_delaunay_max_points();
 * The context's workspace (grow-only, hipMalloc when it grows) holds 76 bytes per point of the LAUNCH — n_frames * max_pts
 * points: the stars' hint caches and the order the points are taken in — and ~33 more above mvosr_delaunay_lds_points(): callers with very many
 * frames launch in chunks (the host class uses up to 8192 frames or 10 M points).
 */
int mvosr_delaunay_batch(mvosr_ctx *ctx, int64_t n_frames, const int64_t *pts_off, const int32_t *pts_cnt,
                         const double *u, const double *v, const int32_t *keep, int max_pts, const int64_t *tri_off,
                         int32_t *tri, int32_t *tri_cnt, int32_t *n_used, int32_t *status);
/* The same with SEEDS: rows (seed_tri + 3*seed_off[f], seed_cnt[f] of them) of a triangulation of ALL the frame's points,
 * ids = positions in (u, v) — what a call without `keep` wrote for the same frames.  A triangle of that triangulation whose
 * three vertices are kept is a triangle of this one (its circumcircle was empty among more points), so it is not searched
 * for again: the second triangulation of a frame (:264-266, over the ~85 % of the points the vote keeps) starts from the
 * ~60 % of the first one's triangles that survive.  Same rows as without seeds.  Seeds that are not a Delaunay triangulation
 * of the frame's points give undefined rows. */
int mvosr_delaunay_batch_seeded(mvosr_ctx *ctx, int64_t n_frames, const int64_t *pts_off, const int32_t *pts_cnt,
                                const double *u, const double *v, const int32_t *keep, int max_pts, const int64_t *tri_off,
                                int32_t *tri, int32_t *tri_cnt, int32_t *n_used, int32_t *status,
                                const int64_t *seed_off, const int32_t *seed_tri, const int32_t *seed_cnt);
/* The same with the per-point facts that let the SECOND triangulation skip the stars the vote did not touch.  info_out
 * (optional; laid out like u, one word per point; only for a call without `keep`): rows the point owns | star degree << 6 |
 * hull flag << 15, and in the high half the index of its first row within the frame's rows.  seed_info (optional, with
 * seeds): what the call that built the seeds wrote.  A kept point none of whose seed triangles lost a vertex has the same
 * star among the survivors (its triangles keep their empty circles and still close the fan): its rows are copied with the
 * ids mapped to ranks and its star is not walked — at 95 % kept points three stars in four.  Same rows as without. */
int mvosr_delaunay_batch_ex(mvosr_ctx *ctx, int64_t n_frames, const int64_t *pts_off, const int32_t *pts_cnt,
                            const double *u, const double *v, const int32_t *keep, int max_pts, const int64_t *tri_off,
                            int32_t *tri, int32_t *tri_cnt, int32_t *n_used, int32_t *status,
                            const int64_t *seed_off, const int32_t *seed_tri, const int32_t *seed_cnt,
                            const uint32_t *seed_info, uint32_t *info_out);
/* Largest frame mvosr_delaunay_batch takes (32 000 points: ids and row indices are 16-bit), and the largest frame whose
 * points, grid and rows fit one workgroup's LDS (about 4 700): a launch whose max_pts is larger runs the kernel's
 * global-memory variant — the same algorithm with the per-frame arrays in a slice of the context's workspace, read
 * through L1/L2 (dense frames, BASELINE configs[4]); slower per point, same rows. */
int mvosr_delaunay_max_points(void);
int mvosr_delaunay_lds_points(void);
/* Frames of a batch whose largest frame has max_pts points that ONE compute unit works on at a time in a launch of 512 frames
 * and more (the launcher's choice of wavefronts per frame and of the arena's home: 8, 4, 3, 2 or 1; 1 for the global-memory
 * variant).  A host that cuts a long batch into chunks makes a chunk a multiple of this x the device's CU count: the kernel
 * then has no partly filled last round. */
int mvosr_delaunay_frames_per_cu(int max_pts);

/*
 * SciPy/Qhull's rows themselves: the triangle set, the ORDER of the rows and the ROTATION of every row of
 * scipy.spatial.Delaunay(points).simplices (/root/reference/src/scale_calculator.py:257-258, :266-267) — what the reference's
 * check_triangle (:105-119) reads.  The kernel replays the beneath-beyond of the Qhull SciPy bundles (qhull_r 7.3.2,
 * options `d Qbb Qc Qz Q12 Qt`) decision by decision, one wavefront per frame, for points in general position; a frame in
 * which a decision falls inside a roundoff guard band (Qhull would merge facets) is declined like mvosr_delaunay_batch
 * declines (status = MVOSR_DT_DEGENERATE | reason << 8, tri_cnt 0): the host triangulates it with SciPy.  Rows are meant for
 * MVOSR_VOTE_REFERENCE: with them triangulation="gpu" IS the reference's result.  Arguments as mvosr_delaunay_batch;
 * order_out (optional, laid out like u): the insertion step at which a point became a vertex (0: initial simplex), indexed
 * by the point's rank among the kept points.  max_pts <= mvosr_delaunay_qhull_max_points() (60 000; launches whose max_pts is above
 * 8 000 use 32-bit facet ids and 80-byte facet records).  Workspace: ~0.55 KB (0.66 KB) per point of the launch
 * (n_frames * (max_pts + 1)), grow-only, in the context.
 */
int mvosr_delaunay_qhull_batch(mvosr_ctx *ctx, int64_t n_frames, const int64_t *pts_off, const int32_t *pts_cnt,
                               const double *u, const double *v, const int32_t *keep, int max_pts, const int64_t *tri_off,
                               int32_t *tri, int32_t *tri_cnt, int32_t *n_used, int32_t *status, int32_t *order_out);
int mvosr_delaunay_qhull_max_points(void);
/*
 * The same replay for ONE point set on the HOST (plain C, no device, no context; thread-safe: per-thread workspace) — replaces the
 * reference's scipy.spatial.Delaunay call for the first triangulation of a per-frame scale_calculation
 * (/root/reference/src/scale_calculator.py:257 from src/main.py:110-113): one frame on the device is a chain of ~n dependent
 * insertions (20 ms at 2000 points); SciPy is 2.6 ms; this loop, which skips what Qhull does for inputs that are not in general
 * position and what SciPy builds around the rows, is several times faster.  points: n_points rows of (x, y), stride_doubles apart
 * (2 for a C-contiguous (n, 2) array); rows: room for rows_cap (>= 2 n_points) int32 triples; *n_rows: rows written; order
 * (optional, n_points): the step at which a site became a vertex.  Returns 0 (rows = SciPy's simplices, bit for bit), > 0: declined
 * — a decision inside a roundoff guard band, fewer than 3 points; the reason code as in the batch kernel's status >> 8; the
 * caller asks SciPy —, < 0: MVOSR_ERR_ARG / MVOSR_ERR_ALLOC.
 */
int mvosr_qhull_rows_host(const double *points, int64_t n_points, int64_t stride_doubles, int32_t *rows, int64_t rows_cap,
                          int32_t *n_rows, int32_t *order);

/* LDS bytes the fused kernel requests for a frame of n features (host-side planning). */
size_t mvosr_lds_bytes(int n_features);
/* Largest frame the LDS-resident variant accepts on this build. */
int mvosr_max_lds_features(void);

#ifdef __cplusplus
}
#endif
#endif /* MVOSR_H */
