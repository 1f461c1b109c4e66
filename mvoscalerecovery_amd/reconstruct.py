"""GPU mirror of /root/reference/src/reconstruct.py: ``Reconstruct.triangle_model`` (:70-90) and
``Reconstruct.depth_generate`` (:91-117) — every image pixel is located in the Delaunay triangulation of a frame's
features and gets the depth at which its viewing ray meets that triangle's plane.  The reference does it with a Python
double loop over the image; here ``mvosr_dense_depth_batch`` rasterises a batch of frames on the device.

What is returned is what the reference computes before it draws: the depth image (0 where no triangle covers the pixel,
not divided by its maximum), the per-pixel triangle index, the ``datas`` rows and the point cloud.  The cloud of :108-115 —
every covered pixel as (px*d, py*d, d) with the image's colour, in raster order — is compacted on the device by
``mvosr_point_cloud_batch``: ``Reconstruct.point_clouds`` / ``cloud_from_depth`` / ``metric_point_clouds``
download the points only, or leave them in device memory; ``write_ply`` / ``read_ply`` are the .ply file the reference writes
through open3d, in NumPy.  The class's own vote and everything drawn with cv2 are not mirrored.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib, packing
from .engine import DeviceBatch, DeviceOutputs

ST_ERR_SINGULAR, ST_ERR_MASK, ST_ERR_EMPTY = 7, 8, 9        # enum mvosr_status
DEFAULT_BUDGET = 2 << 30                                     # bytes of images one chunk may hold on the device


@dataclass
class DepthResult:
    """One frame: ``depth`` (H,W) float64, ``tri_id`` (H,W) int32 (-1: uncovered), ``datas`` (T,4) = (nx, ny, nz, height) per
    row, ``points`` (K,3) = (px*d, py*d, d) of the covered pixels in raster order (reconstruct.py:108-109)."""
    depth: np.ndarray
    tri_id: np.ndarray
    datas: np.ndarray
    points: np.ndarray


@dataclass
class DepthMaps:
    """A batch: ``depth`` (F,H,W) and ``tri_id`` (F,H,W) or None; ``datas`` one (T,4) array per frame; ``rows`` the rows that were
    rasterised; ``covered`` / ``status`` (F,).  With ``on_device=True`` ``depth`` / ``tri_id`` are None and ``chunks`` lists
    ``(first_frame, n_frames, depth_buffer, tri_id_buffer)`` — ``_lib.DeviceBuffer``s of shape (n, H, W) (``.ptr`` is what
    ``torch``'s ``data_ptr`` consumers want); free them when done."""
    depth: np.ndarray
    tri_id: np.ndarray
    datas: list
    rows: list
    covered: np.ndarray
    status: np.ndarray
    chunks: list = field(default_factory=list)


@dataclass
class PointClouds:
    """The clouds of a batch, back to back in frame order: ``points`` (K,3) = (px*d, py*d, d) and ``colors`` (K,3) = RGB / 255 or
    None, float64 or float32; ``offsets`` (F+1,) int64 — frame ``f`` owns rows ``offsets[f]:offsets[f+1]``; ``covered`` /
    ``status`` (F,) as in :class:`DepthMaps`.  With ``on_device=True`` ``points`` / ``colors`` are None and ``chunks`` lists
    ``(first_frame, n_frames, points_buffer, colors_buffer, offsets)``: ``_lib.DeviceBuffer``s of shape (capacity, 3) whose first
    ``offsets[-1]`` rows are the chunk's points (``offsets``: the chunk's own (n+1,) int64, from 0); free them when done."""
    points: np.ndarray
    colors: np.ndarray
    offsets: np.ndarray
    covered: np.ndarray
    status: np.ndarray
    chunks: list = field(default_factory=list)

    def frame(self, f):
        """``(points, colors)`` of frame ``f``: views."""
        a, b = int(self.offsets[f]), int(self.offsets[f + 1])
        return self.points[a:b], None if self.colors is None else self.colors[a:b]


class CloudCapacityError(ValueError):
    """``cloud_from_depth`` with a ``capacity`` below the cloud's size; ``needed``: the size (call again with it)."""

    def __init__(self, needed, capacity):
        super().__init__("point cloud of %d points does not fit a capacity of %d" % (needed, capacity))
        self.needed, self.capacity = int(needed), int(capacity)


def check_camera(cam):
    """(width, height, fx, fy, cx, cy) of anything that has them (the reference's PinholeCamera), validated."""
    try:
        w, h = cam.width, cam.height
        k = tuple(float(getattr(cam, n)) for n in ("fx", "fy", "cx", "cy"))
    except AttributeError as exc:
        raise TypeError("camera needs width, height, fx, fy, cx, cy") from exc
    if int(w) != w or int(h) != h or int(w) < 1 or int(h) < 1:
        raise ValueError("camera of %r x %r pixels" % (w, h))
    return (int(w), int(h)) + k


def plan_chunks(n_frames, width, height, ids=False, budget_bytes=DEFAULT_BUDGET, extra_per_frame=0):
    """Frames per launch such that the images of a chunk (8 bytes per pixel, 4 more with ids, ``extra_per_frame`` bytes for
    what else a frame keeps on the device: :func:`cloud_bytes_per_frame`) fit ``budget_bytes`` — at least one frame per chunk.
    Returns ``[(first_frame, count), ...]``."""
    if n_frames < 0 or budget_bytes <= 0 or extra_per_frame < 0:
        raise ValueError("plan_chunks: negative frame count or non-positive budget")
    per = int(width) * int(height) * (12 if ids else 8) + int(extra_per_frame)
    step = max(1, int(budget_bytes) // per)
    return [(s, min(step, n_frames - s)) for s in range(0, n_frames, step)]


def grid_points(width, height, stride=1):
    """Pixels of a ``width`` x ``height`` image on the stride grid: ceil(W/stride) * ceil(H/stride)."""
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be >= 1")
    return (-(-int(width) // stride)) * (-(-int(height) // stride))


def cloud_bytes_per_frame(width, height, stride=1, dtype=np.float64, images=False):
    """Device bytes a frame's cloud adds to its depth image at most: the colour image (3 per pixel) and, per pixel of the
    stride grid, a point — and a colour with ``images`` — of three ``dtype`` values."""
    row = 3 * check_cloud_dtype(dtype).itemsize
    return (3 * int(width) * int(height) + 2 * row * grid_points(width, height, stride)) if images else row * grid_points(width, height, stride)


def check_cloud_dtype(dtype):
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("point clouds are float64 or float32, not %s" % dtype)
    return dtype


def check_cloud_options(n_frames, width, height, images=None, scales=None, depth_range=None, stride=1, dtype=np.float64):
    """Validated ``(images (F,H,W,3) uint8 or None, scales (F,) float64 or None, (near, far) or None, stride, dtype)``."""
    dtype = check_cloud_dtype(dtype)
    if int(stride) != stride or int(stride) < 1:
        raise ValueError("stride must be an integer >= 1")
    if images is not None and not isinstance(images, _lib.DeviceBuffer):
        if len(images) != n_frames:
            raise ValueError("images: one per frame")
        for f, im in enumerate(images):
            im = np.asarray(im)
            if im.dtype != np.uint8 or im.shape != (height, width, 3):
                raise ValueError("image %d: uint8 (%d, %d, 3) expected, got %s %s" % (f, height, width, im.dtype, im.shape))
        images = np.ascontiguousarray(images, dtype=np.uint8).reshape(n_frames, height, width, 3)
    if scales is not None and not isinstance(scales, _lib.DeviceBuffer):
        scales = np.ascontiguousarray(scales, dtype=np.float64)
        if scales.shape != (n_frames,):
            raise ValueError("one scale per frame")
    if depth_range is not None:
        near, far = (float(v) for v in depth_range)
        depth_range = (near, far)
    return images, scales, depth_range, int(stride), dtype


def check_frames(feature3ds, feature2ds, tris=None, keeps=None):
    """Shapes of a batch's per-frame arrays; returns them as float64 / int32 / bool arrays."""
    if len(feature3ds) != len(feature2ds):
        raise ValueError("feature3ds and feature2ds differ in length")
    for name, extra in (("tris", tris), ("keeps", keeps)):
        if extra is not None and len(extra) != len(feature3ds):
            raise ValueError("%s: one entry per frame" % name)
    f3s, f2s = [], []
    for f, (a, b) in enumerate(zip(feature3ds, feature2ds)):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        if a.size == 0 and b.size == 0:
            a, b = a.reshape(0, 3), b.reshape(0, 2)
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != 3 or b.shape[1] != 2 or a.shape[0] != b.shape[0]:
            raise ValueError("frame %d: feature3d must be (N,3) and feature2d (N,2), got %s and %s" % (f, a.shape, b.shape))
        f3s.append(a)
        f2s.append(b)
    ks = None
    if keeps is not None:
        ks = []
        for f, k in enumerate(keeps):
            k = np.asarray(k)
            if k.dtype != np.bool_ or k.shape != (len(f3s[f]),):
                raise ValueError("frame %d: keep must be a boolean mask over the frame's features" % f)
            ks.append(k)
    ts = None
    if tris is not None:
        ts = []
        for f, t in enumerate(tris):
            t = np.asarray(t)
            if t.size == 0:
                t = np.zeros((0, 3), dtype=np.int32)
            if t.ndim != 2 or t.shape[1] != 3 or not np.issubdtype(t.dtype, np.integer):
                raise ValueError("frame %d: rows must be an integer (T,3) array" % f)
            ts.append(np.ascontiguousarray(t, dtype=np.int32))
    return f3s, f2s, ts, ks


def pack_all(f3s, f2s):
    """The planes of ``mvosr_batch`` for EVERY feature of every frame, in order (the rows index the caller's features, so nothing
    may be filtered: ``packing.pack_features`` drops a feature whose pixel row is NaN or -inf even with ``vanish=-inf``)."""
    F = len(f3s)
    cnt = np.array([len(a) for a in f3s], dtype=np.int32)
    off, total = packing.pack_layout(cnt)
    x, y, z, u, v = (np.zeros(total) for _ in range(5))
    for f in range(F):
        o, n = int(off[f]), int(cnt[f])
        if n:
            x[o:o + n], y[o:o + n], z[o:o + n] = f3s[f][:, 0], f3s[f][:, 1], f3s[f][:, 2]
            u[o:o + n], v[o:o + n] = f2s[f][:, 0], f2s[f][:, 1]
    return packing.PackedFrames(F, off, cnt, x, y, z, v, u, [None] * F, max_feat=int(cnt.max()) if F else 0)


def raise_for_depth_status(status, frame=None):
    where = "" if frame is None else " (frame %d)" % frame
    if status == ST_ERR_SINGULAR:
        raise np.linalg.LinAlgError("Singular matrix" + where)          # reconstruct.py:78
    if status == ST_ERR_MASK:
        raise ValueError("a row names a vertex the frame does not have, or the frame has more than 2 N rows" + where)


class Reconstruct:
    """``Reconstruct(cam)`` — ``cam`` is anything with ``width, height, fx, fy, cx, cy``."""

    def __init__(self, cam, device=0, ctx=None, delaunay_workers=0):
        self.width, self.height, self.fx, self.fy, self.cx, self.cy = check_camera(cam)
        self.cam = cam
        self.device = device
        self._ctx = ctx
        self.delaunay_workers = delaunay_workers

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.default_context(self.device)
        return self._ctx

    def _camera_struct(self):
        return _lib.Camera(self.width, self.height, self.fx, self.fy, self.cx, self.cy)

    # ---- the reference's two methods ---------------------------------------------------------------------------------------
    def triangle_model(self, feature3d, triangle_ids):
        """reconstruct.py:70-90 in one launch: ``datas`` (T,4).  Raises ``LinAlgError`` where the reference does."""
        f3 = np.asarray(feature3d, dtype=np.float64)
        f3s, f2s, ts, _ = check_frames([f3], [np.zeros((len(f3), 2))], [triangle_ids])
        if ts[0].shape[0] == 0:
            return np.zeros((0, 4))
        ctx = self.ctx
        pf = pack_all(f3s, f2s)
        pf.tri1_off, pf.tri1 = packing._pack_tris(ts)
        db = DeviceBatch(ctx, pf, with_tri2=False)
        model, status = ctx.empty((ts[0].shape[0], 4), np.float64), ctx.zeros(1, np.int32)
        try:
            b = db.struct()
            _lib.check(ctx.lib.mvosr_triangle_model_batch(ctx.handle, C.byref(b), 1, None, model.ptr, status.ptr), "mvosr_triangle_model_batch")
            ctx.sync()
            st, out = int(status.download()[0]), model.download()
        finally:
            model.free()
            status.free()
            db.free()
        raise_for_depth_status(st)
        return out

    def depth_generate(self, feature3d, feature2d, triangle_ids=None, points=True):
        """reconstruct.py:91-117 for one frame, returning what the reference only displays.  ``triangle_ids``: the rows of a
        triangulation of ``feature2d`` (default: SciPy's Delaunay, as ``visualize`` builds it, :188-189)."""
        res = self.depth_maps([feature3d], [feature2d], tris=None if triangle_ids is None else [triangle_ids], ids=True)
        depth, tri = res.depth[0], res.tri_id[0]
        pts = np.zeros((0, 3))
        if points:
            yy, xx = np.nonzero(tri >= 0)
            d = depth[yy, xx]
            px = (xx.astype(np.float64) - self.cx) / self.fx                                        # :32
            py = (yy.astype(np.float64) - self.cy) / self.fy                                        # :35
            pts = np.stack([px * d, py * d, d], axis=1)                                             # :108
        return DepthResult(depth, tri, res.datas[0], pts)

    # ---- the batch form ------------------------------------------------------------------------------------------------------
    def _rows_for(self, f2s, keeps, triangulation):
        pts = [np.ascontiguousarray(p if k is None else p[k]) for p, k in zip(f2s, keeps or [None] * len(f2s))]
        todo = [f for f, p in enumerate(pts) if len(p) >= 3]                  # (fewer than 3 points: no rows, MVOSR_ST_ERR_EMPTY)
        rows = [np.zeros((0, 3), dtype=np.int32)] * len(pts)
        if triangulation == "gpu":
            got = packing.delaunay_gpu_or_host(self.ctx, [pts[f] for f in todo], self.delaunay_workers, canonical=True)
        elif triangulation == "scipy":
            got = packing.delaunay_many([pts[f] for f in todo], self.delaunay_workers)
        else:
            raise ValueError("triangulation must be 'scipy' or 'gpu'")
        for f, t in zip(todo, got):
            if isinstance(t, Exception):
                raise t
            rows[f] = np.ascontiguousarray(t, dtype=np.int32)
        return rows

    def _depth_chunk(self, f3s, f2s, ts, ks, first, n, ids):
        """Frames ``first : first + n`` through ``mvosr_dense_depth_batch``.  Returns ``(d_depth, d_ids, status, covered, datas)``:
        the images stay on the device (the caller frees them), the rest is downloaded."""
        ctx, W, H = self.ctx, self.width, self.height
        cam = self._camera_struct()
        sl = slice(first, first + n)
        pf = pack_all(f3s[sl], f2s[sl])
        pf.tri1_off, pf.tri1 = packing._pack_tris(ts[sl])
        db = DeviceBatch(ctx, pf, with_tri2=False)
        bufs = [ctx.to_device(pf.u)]
        d_keep = None
        if ks is not None:
            kp = np.zeros(len(pf.u), dtype=np.int32)
            for f in range(n):
                kp[pf.frame_slice(f)] = np.where(ks[first + f], 0, -1)
            d_keep = ctx.to_device(kp)
            bufs.append(d_keep)
        d_depth = ctx.empty((n, H, W), np.float64)
        d_ids = ctx.empty((n, H, W), np.int32) if ids else None
        d_model = ctx.empty((max(int(pf.tri1_off[-1]), 1), 4), np.float64)
        d_cov, d_st = ctx.empty(n, np.int32), ctx.empty(n, np.int32)
        bufs += [d_model, d_cov, d_st]
        o = _lib.DepthOutputs(d_depth.ptr, d_ids.ptr if ids else None, d_model.ptr, d_cov.ptr, d_st.ptr)
        done = False
        try:
            b = db.struct()
            _lib.check(ctx.lib.mvosr_dense_depth_batch(ctx.handle, C.byref(b), 1, bufs[0].ptr, d_keep.ptr if d_keep is not None else None,
                                                       C.byref(cam), C.byref(o), 0, 0), "mvosr_dense_depth_batch")
            ctx.sync()
            status, covered = d_st.download(), d_cov.download()
            model = d_model.download()
            datas = [model[int(pf.tri1_off[f]):int(pf.tri1_off[f + 1])].copy() for f in range(n)]
            done = True
        finally:
            for buf in bufs + ([] if done else [d_depth] + ([d_ids] if ids else [])):
                buf.free()
            db.free()
        return d_depth, d_ids, status, covered, datas

    def depth_maps(self, feature3ds, feature2ds, tris=None, keeps=None, triangulation="scipy", ids=False, on_device=False,
                   budget_bytes=DEFAULT_BUDGET):
        """Depth images of a batch of frames.  ``tris``: per frame the rows of a triangulation of the frame's (kept) pixels;
        default: built here — ``"scipy"``: SciPy's rows from the worker pool, ``"gpu"``: ``packing.delaunay_gpu`` (canonical rows;
        frames the device stage declines go to SciPy).  The image depends on the triangle SET; the depths depend on the order of
        the rows and of the vertices inside a row through rounding only.  ``keeps``: per-frame boolean masks; only the features
        with ``keep`` take part and the rows' ids number THEM (the features stay where they are: the kernel ranks them).
        Frames are processed in chunks whose images fit ``budget_bytes`` on the device.  ``on_device=True``: nothing but the
        statuses is downloaded (see :class:`DepthMaps`)."""
        if triangulation not in ("scipy", "gpu"):
            raise ValueError("triangulation must be 'scipy' or 'gpu'")
        f3s, f2s, ts, ks = check_frames(feature3ds, feature2ds, tris, keeps)
        F, W, H = len(f3s), self.width, self.height
        chunks = plan_chunks(F, W, H, ids, budget_bytes)
        if ts is None:
            ts = self._rows_for(f2s, ks, triangulation)
        res = DepthMaps(None if on_device else np.zeros((F, H, W)), None if (on_device or not ids) else np.full((F, H, W), -1, np.int32),
                        [None] * F, ts, np.zeros(F, np.int32), np.zeros(F, np.int32))
        for first, n in chunks:
            sl = slice(first, first + n)
            d_depth, d_ids, res.status[sl], res.covered[sl], res.datas[sl] = self._depth_chunk(f3s, f2s, ts, ks, first, n, ids)
            if on_device:
                res.chunks.append((first, n, d_depth, d_ids))
                continue
            try:
                res.depth[sl] = d_depth.download()
                if ids:
                    res.tri_id[sl] = d_ids.download()
            finally:
                d_depth.free()
                if ids:
                    d_ids.free()
        for f in range(F):
            raise_for_depth_status(int(res.status[f]), f)
        return res

    # ---- point clouds ----------------------------------------------------------------------------------------------------------
    def _cloud_launch(self, n, depth_ptr, ids_ptr, image_ptr, scale_ptr, depth_range, stride, dtype, capacity, with_colors):
        """``mvosr_point_cloud_batch`` on ``n`` resident frames.  Returns ``(d_points, d_colors, offsets (n+1,) int64, overflow)``
        after the stream has been waited for; the buffers hold ``capacity`` rows."""
        ctx = self.ctx
        cam = self._camera_struct()
        d_pts = ctx.empty((capacity, 3), dtype)
        d_col = ctx.empty((capacity, 3), dtype) if with_colors else None
        d_off, d_ovf = ctx.empty(n + 1, np.int64), ctx.empty(1, np.int32)
        near, far = depth_range if depth_range is not None else (0.0, 0.0)
        flags = (_lib.CLOUD_RANGE if depth_range is not None else 0) | (_lib.CLOUD_F32 if dtype == np.dtype(np.float32) else 0)
        i = _lib.CloudInputs(depth_ptr, ids_ptr, image_ptr, scale_ptr, n)
        p = _lib.CloudParams(near, far, stride, flags)
        o = _lib.CloudOutputs(d_pts.ptr, d_col.ptr if with_colors else None, d_off.ptr, d_ovf.ptr, capacity)
        done = False
        try:
            _lib.check(ctx.lib.mvosr_point_cloud_batch(ctx.handle, C.byref(i), C.byref(cam), C.byref(p), C.byref(o)), "mvosr_point_cloud_batch")
            ctx.sync()
            offsets, overflow = d_off.download(), int(d_ovf.download()[0])
            done = True
        finally:
            d_off.free()
            d_ovf.free()
            if not done:
                d_pts.free()
                if with_colors:
                    d_col.free()
        return d_pts, d_col, offsets, overflow

    @staticmethod
    def _download_rows(buf, k):
        """The first ``k`` rows of a (capacity, 3) device buffer."""
        out = np.empty((k, 3), dtype=buf.dtype)
        if k:
            _lib.check(buf.ctx.lib.mvosr_memcpy_d2h(buf.ctx.handle, _lib.addr(out), buf.ptr, out.nbytes), "d2h")
        return out

    def _cloud_chunk(self, res, first, n, d_depth, d_ids, images, scales, depth_range, stride, dtype, capacity, on_device, parts, base):
        """The cloud of ``n`` resident frames into ``res`` (chunk of frames ``first``...); returns the number of points."""
        ctx = self.ctx
        temps = []
        try:
            d_img = d_sc = None
            if images is not None:
                d_img = images if isinstance(images, _lib.DeviceBuffer) else ctx.to_device(images[first:first + n])
                temps += [] if d_img is images else [d_img]
            if scales is not None:
                d_sc = scales if isinstance(scales, _lib.DeviceBuffer) else ctx.to_device(scales[first:first + n])
                temps += [] if d_sc is scales else [d_sc]
            d_pts, d_col, offsets, overflow = self._cloud_launch(
                n, d_depth.ptr, d_ids.ptr if d_ids is not None else None, d_img.ptr if d_img is not None else None,
                d_sc.ptr if d_sc is not None else None, depth_range, stride, dtype, capacity, images is not None)
        finally:
            for t in temps:
                t.free()
        k = int(offsets[-1])
        if overflow:
            d_pts.free()
            if d_col is not None:
                d_col.free()
            raise CloudCapacityError(k, capacity)
        res.offsets[first + 1:first + n + 1] = base + offsets[1:]
        if on_device:
            res.chunks.append((first, n, d_pts, d_col, offsets))
        else:
            try:
                parts[0].append(self._download_rows(d_pts, k))
                if d_col is not None:
                    parts[1].append(self._download_rows(d_col, k))
            finally:
                d_pts.free()
                if d_col is not None:
                    d_col.free()
        return k

    @staticmethod
    def _finish_cloud(res, parts, dtype, with_colors, on_device):
        if not on_device:
            res.points = np.concatenate(parts[0]) if parts[0] else np.zeros((0, 3), dtype)
            if with_colors:
                res.colors = np.concatenate(parts[1]) if parts[1] else np.zeros((0, 3), dtype)
        return res

    def point_clouds(self, feature3ds, feature2ds, tris=None, keeps=None, triangulation="scipy", images=None, scales=None,
                     depth_range=None, stride=1, dtype=np.float64, on_device=False, budget_bytes=DEFAULT_BUDGET):
        """The clouds of a batch of frames (reconstruct.py:108-115): ``depth_maps`` with ids, chunk by chunk, and — the images
        never leaving the device — ``mvosr_point_cloud_batch``: every covered pixel (id >= 0) on the ``stride`` grid whose depth
        times ``scales[f]`` lies in ``depth_range = (near, far)`` (both optional) as (px*d, py*d, d), in raster order, with the
        colour ``images[f][v, u, ::-1] / 255.0`` (``images``: uint8 (H,W,3) per frame, BGR).  Only the points are downloaded;
        ``on_device=True``: nothing is (see :class:`PointClouds`).  A chunk's depth and id images, colour images and clouds fit
        ``budget_bytes``; the cloud buffers are sized from the chunk's covered counts."""
        if triangulation not in ("scipy", "gpu"):
            raise ValueError("triangulation must be 'scipy' or 'gpu'")
        f3s, f2s, ts, ks = check_frames(feature3ds, feature2ds, tris, keeps)
        F, W, H = len(f3s), self.width, self.height
        if isinstance(images, _lib.DeviceBuffer) or isinstance(scales, _lib.DeviceBuffer):
            raise TypeError("point_clouds takes host images and scales (it cuts them into chunks); cloud_from_depth takes device buffers")
        images, scales, depth_range, stride, dtype = check_cloud_options(F, W, H, images, scales, depth_range, stride, dtype)
        chunks = plan_chunks(F, W, H, True, budget_bytes, cloud_bytes_per_frame(W, H, stride, dtype, images is not None))
        if ts is None:
            ts = self._rows_for(f2s, ks, triangulation)
        res = PointClouds(None, None, np.zeros(F + 1, np.int64), np.zeros(F, np.int32), np.zeros(F, np.int32))
        parts, total, bound = ([], []), 0, grid_points(W, H, stride)
        for first, n in chunks:
            sl = slice(first, first + n)
            d_depth, d_ids, res.status[sl], res.covered[sl], _ = self._depth_chunk(f3s, f2s, ts, ks, first, n, True)
            try:
                for f in range(first, first + n):
                    raise_for_depth_status(int(res.status[f]), f)
                capacity = int(np.minimum(res.covered[sl].astype(np.int64), bound).sum())
                total += self._cloud_chunk(res, first, n, d_depth, d_ids, images, scales, depth_range, stride, dtype, capacity, on_device,
                                           parts, total)
            finally:
                d_depth.free()
                d_ids.free()
        return self._finish_cloud(res, parts, dtype, images is not None, on_device)

    def cloud_from_depth(self, depth, tri_id=None, images=None, scales=None, depth_range=None, stride=1, dtype=np.float64, capacity=None,
                         on_device=False):
        """The low-level form, for depth images the caller already has: ``depth`` (F,H,W) float64 — and ``tri_id`` (F,H,W) int32,
        ``images`` (F,H,W,3) uint8, ``scales`` (F,) — as host arrays or ``_lib.DeviceBuffer``s of those shapes (one launch: no
        chunks).  Without ``tri_id`` a pixel is covered when its depth is not 0 (NaN is); the two rules differ only for a covered
        pixel whose depth is exactly +-0.  ``capacity``: points the output buffers hold (default: the stride grid's size times F,
        which cannot overflow); a cloud that does not fit raises :class:`CloudCapacityError` with the size needed.  ``covered``
        of the result: the frames' point counts."""
        W, H = self.width, self.height
        dev = isinstance(depth, _lib.DeviceBuffer)
        if not dev:
            depth = np.ascontiguousarray(depth, dtype=np.float64)
            depth = depth.reshape((1,) + depth.shape) if depth.ndim == 2 else depth
        if len(depth.shape) != 3 or tuple(depth.shape[1:]) != (H, W) or np.dtype(depth.dtype) != np.float64:
            raise ValueError("depth must be float64 (F, %d, %d), got %s" % (H, W, (depth.shape,)))
        F = int(depth.shape[0])
        if tri_id is not None:
            if not isinstance(tri_id, _lib.DeviceBuffer):
                tri_id = np.ascontiguousarray(tri_id, dtype=np.int32).reshape((-1, H, W))
            if tuple(tri_id.shape) != (F, H, W) or np.dtype(tri_id.dtype) != np.int32:
                raise ValueError("tri_id must be int32 and shaped like depth")
        if isinstance(images, _lib.DeviceBuffer) and (tuple(images.shape) != (F, H, W, 3) or images.dtype != np.uint8):
            raise ValueError("images must be uint8 (F, H, W, 3)")
        if isinstance(scales, _lib.DeviceBuffer) and (tuple(scales.shape) != (F,) or scales.dtype != np.float64):
            raise ValueError("one float64 scale per frame")
        images, scales, depth_range, stride, dtype = check_cloud_options(F, W, H, images, scales, depth_range, stride, dtype)
        capacity = F * grid_points(W, H, stride) if capacity is None else int(capacity)
        if capacity < 0:
            raise ValueError("negative capacity")
        res = PointClouds(None, None, np.zeros(F + 1, np.int64), np.zeros(F, np.int32), np.zeros(F, np.int32))
        parts = ([], [])
        if F:
            ctx = self.ctx
            d_depth = depth if dev else ctx.to_device(depth)
            d_ids = tri_id if (tri_id is None or isinstance(tri_id, _lib.DeviceBuffer)) else ctx.to_device(tri_id)
            try:
                self._cloud_chunk(res, 0, F, d_depth, d_ids, images, scales, depth_range, stride, dtype, capacity, on_device, parts, 0)
            finally:
                if d_depth is not depth:
                    d_depth.free()
                if d_ids is not None and d_ids is not tri_id:
                    d_ids.free()
        res.covered[:] = np.diff(res.offsets)
        return self._finish_cloud(res, parts, dtype, images is not None, on_device)


def _metric_survivors(estimator, feature3ds, feature2ds, cam, scales):
    """What ``metric_depth_batch`` and ``metric_point_clouds`` share: the scales (given, or the estimator's), per frame the
    features below the vanishing row, the survivors of the estimator's vote as masks over them, and the rows of their second
    triangulation.  Returns ``(rec, f3s, f2s, rows, masks, scales)``."""
    eng = estimator.engine
    ctx = eng.ctx
    f3s, f2s, _, _ = check_frames(feature3ds, feature2ds)
    if scales is None:
        scales, _ = estimator.scale_calculation_batch([a.copy() for a in f3s], [b.copy() for b in f2s])
    scales = np.asarray(scales, dtype=np.float64)
    if scales.shape != (len(f3s),):
        raise ValueError("one scale per frame")
    low = [b[:, 1] > estimator.vanish for b in f2s]                                                      # scale_calculator.py:252-254
    f3s, f2s = [np.ascontiguousarray(a[m]) for a, m in zip(f3s, low)], [np.ascontiguousarray(b[m]) for b, m in zip(f2s, low)]
    pf = packing.pack_features(f3s, f2s, -np.inf)
    pf.extra["canonical"] = estimator.check_triangle == "fixed"
    packing.attach_tri1(pf, None, estimator.delaunay_workers)
    for f, err in sorted(pf.extra["tri1_errors"].items()):
        raise err
    db = DeviceBatch(ctx, pf, with_tri2=False)
    if getattr(estimator, "vote", "outliers") == "reliability":
        from .engine import ReliabilityOutputs
        vote_out = ReliabilityOutputs(ctx, db)
        try:
            eng.reliability_batch(db, vote_out)
            keep, refused = vote_out.get("keep"), vote_out.get("status")
        finally:
            vote_out.free()
            db.free()
        if np.any(refused[:len(f3s)] != 0):
            raise _lib.MvosrLibraryError("the reliability vote refused the rows of frame %d" % int(np.argmax(refused[:len(f3s)] != 0)))
        masks = [keep[pf.frame_slice(f)] == 0 for f in range(len(f3s))]                                  # :145
    else:
        vote_out = DeviceOutputs(ctx, db, counts=True, stage=True)
        try:
            eng.outlier_vote_batch(db, vote_out)
            counters = vote_out.get("vote_counters")
        finally:
            vote_out.free()
            db.free()
        masks = [counters[pf.frame_slice(f)] >= 0 for f in range(len(f3s))]                              # :166
    rec = Reconstruct(cam, ctx=ctx, delaunay_workers=estimator.delaunay_workers)
    rows = rec._rows_for(f2s, masks, "scipy")
    if estimator.check_triangle == "fixed":
        rows = [packing.canonical_rows(t) for t in rows]
    return rec, f3s, f2s, rows, masks, scales


def metric_depth_batch(estimator, feature3ds, feature2ds, cam, scales=None, ids=False):
    """Metric, piecewise-planar depth maps next to the scale: per frame the features below the estimator's vanishing row, the
    survivors of ITS vote (``mvosr_outlier_vote_batch`` with the estimator's ``check_triangle`` mode), their second
    triangulation, ``depth_maps`` of that — times the frame's filtered scale (the planes are linear in the features' scale).
    ``scales``: given, or computed by ``estimator.scale_calculation_batch`` on a copy of the inputs — the estimator's state
    is advanced exactly as by that call and by nothing else.  Returns ``(DepthMaps, scales)``."""
    rec, f3s, f2s, rows, masks, scales = _metric_survivors(estimator, feature3ds, feature2ds, cam, scales)
    res = rec.depth_maps(f3s, f2s, tris=rows, keeps=masks, ids=ids)
    res.depth *= scales[:, None, None]
    return res, scales


def metric_point_clouds(estimator, feature3ds, feature2ds, cam, images=None, scales=None, depth_range=None, stride=1, dtype=np.float64,
                        on_device=False, budget_bytes=DEFAULT_BUDGET):
    """Metric, coloured point clouds next to the scale: the survivors and rows of ``metric_depth_batch``, then
    ``Reconstruct.point_clouds`` with the frames' scales applied ON THE DEVICE (depth * scale, one multiplication, before the
    range test and the rays) — depth image to scaled cloud without a host round trip.  ``depth_range`` is metric.  The
    estimator's state advances exactly as by ``scale_calculation_batch`` (not at all when ``scales`` are given).  Returns
    ``(PointClouds, scales)``."""
    rec, f3s, f2s, rows, masks, scales = _metric_survivors(estimator, feature3ds, feature2ds, cam, scales)
    res = rec.point_clouds(f3s, f2s, tris=rows, keeps=masks, images=images, scales=scales, depth_range=depth_range, stride=stride, dtype=dtype,
                           on_device=on_device, budget_bytes=budget_bytes)
    return res, scales


# ---- the .ply file the reference writes through open3d (reconstruct.py:111-115) --------------------------------------------

def _ply_dtype(real, colors):
    return np.dtype([("x", real), ("y", real), ("z", real)] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if colors else []))


def write_ply(path, points, colors=None):
    """Binary little-endian PLY: ``float`` (float32 points) or ``double`` x y z per vertex and, with ``colors`` (K,3) in 0..1,
    ``uchar`` red green blue = round(colors * 255)."""
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError("points must be (K, 3)")
    real = "<f4" if points.dtype == np.float32 else "<f8"
    if colors is not None:
        colors = np.asarray(colors)
        if colors.shape != points.shape:
            raise ValueError("colors must be shaped like points")
    rec = np.zeros(len(points), dtype=_ply_dtype(real, colors is not None))
    rec["x"], rec["y"], rec["z"] = points[:, 0], points[:, 1], points[:, 2]
    if colors is not None:
        rgb = np.clip(np.round(colors.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
        rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    name = "float" if real == "<f4" else "double"
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(points)]
    head += ["property %s %s" % (name, c) for c in "xyz"]
    if colors is not None:
        head += ["property uchar %s" % c for c in ("red", "green", "blue")]
    head.append("end_header")
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())


def read_ply(path):
    """What ``write_ply`` wrote: ``(points (K,3) float32 / float64, colors (K,3) float64 = uchar / 255.0, or None)``."""
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply" or fh.readline().strip() != b"format binary_little_endian 1.0":
            raise ValueError("%s: not a binary little-endian PLY file" % path)
        count, props = None, []
        for line in iter(fh.readline, b""):
            words = line.decode("ascii").split()
            if words[:1] == ["end_header"]:
                break
            if words[:2] == ["element", "vertex"]:
                count = int(words[2])
            elif words[:1] == ["element"]:
                raise ValueError("%s: only vertex elements are read" % path)
            elif words[:1] == ["property"]:
                props.append((words[2], {"float": "<f4", "double": "<f8", "uchar": "u1"}[words[1]]))
        else:
            raise ValueError("%s: no end_header" % path)
        names = [n for n, _ in props]
        if count is None or names[:3] != ["x", "y", "z"] or names[3:] not in ([], ["red", "green", "blue"]):
            raise ValueError("%s: x y z [red green blue] vertices expected" % path)
        rec = np.frombuffer(fh.read(), dtype=np.dtype(props), count=count)
    points = np.stack([rec["x"], rec["y"], rec["z"]], axis=1)
    colors = np.stack([rec["red"], rec["green"], rec["blue"]], axis=1) / 255.0 if len(props) > 3 else None
    return points, colors
