"""GPU mirror of /root/reference/src/reconstruct.py: ``Reconstruct.triangle_model`` (:70-90) and
``Reconstruct.depth_generate`` (:91-117) — every image pixel is located in the Delaunay triangulation of a frame's
features and gets the depth at which its viewing ray meets that triangle's plane.  The reference does it with a Python
double loop over the image; here ``mvosr_dense_depth_batch`` rasterises a batch of frames on the device.

What is returned is what the reference computes before it draws: the depth image (0 where no triangle covers the pixel,
not divided by its maximum), the per-pixel triangle index, the ``datas`` rows and the point cloud.  The class's own vote,
the .ply file, the colours and everything drawn with cv2 are not mirrored.  There is no CPU fallback."""
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


def plan_chunks(n_frames, width, height, ids=False, budget_bytes=DEFAULT_BUDGET):
    """Frames per launch such that the images of a chunk (8 bytes per pixel, 4 more with ids) fit ``budget_bytes`` — at least
    one frame per chunk.  Returns ``[(first_frame, count), ...]``."""
    if n_frames < 0 or budget_bytes <= 0:
        raise ValueError("plan_chunks: negative frame count or non-positive budget")
    per = int(width) * int(height) * (12 if ids else 8)
    step = max(1, int(budget_bytes) // per)
    return [(s, min(step, n_frames - s)) for s in range(0, n_frames, step)]


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
        ctx = self.ctx
        res = DepthMaps(None if on_device else np.zeros((F, H, W)), None if (on_device or not ids) else np.full((F, H, W), -1, np.int32),
                        [None] * F, ts, np.zeros(F, np.int32), np.zeros(F, np.int32))
        cam = self._camera_struct()
        for first, n in chunks:
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
            try:
                b = db.struct()
                _lib.check(ctx.lib.mvosr_dense_depth_batch(ctx.handle, C.byref(b), 1, bufs[0].ptr, d_keep.ptr if d_keep is not None else None,
                                                           C.byref(cam), C.byref(o), 0, 0), "mvosr_dense_depth_batch")
                ctx.sync()
                res.status[sl], res.covered[sl] = d_st.download(), d_cov.download()
                model = d_model.download()
                for f in range(n):
                    res.datas[first + f] = model[int(pf.tri1_off[f]):int(pf.tri1_off[f + 1])].copy()
                if on_device:
                    res.chunks.append((first, n, d_depth, d_ids))
                else:
                    res.depth[sl] = d_depth.download()
                    if ids:
                        res.tri_id[sl] = d_ids.download()
            finally:
                for buf in bufs + ([] if on_device else [d_depth] + ([d_ids] if ids else [])):
                    buf.free()
                db.free()
        for f in range(F):
            raise_for_depth_status(int(res.status[f]), f)
        return res


def metric_depth_batch(estimator, feature3ds, feature2ds, cam, scales=None, ids=False):
    """Metric, piecewise-planar depth maps next to the scale: per frame the features below the estimator's vanishing row, the
    survivors of ITS vote (``mvosr_outlier_vote_batch`` with the estimator's ``check_triangle`` mode), their second
    triangulation, ``depth_maps`` of that — times the frame's filtered scale (the planes are linear in the features' scale).
    ``scales``: given, or computed by ``estimator.scale_calculation_batch`` on a copy of the inputs — the estimator's state
    is advanced exactly as by that call and by nothing else.  Returns ``(DepthMaps, scales)``."""
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
    vote_out = DeviceOutputs(ctx, db, counts=True, stage=True)
    try:
        eng.outlier_vote_batch(db, vote_out)
        counters = vote_out.get("vote_counters")
    finally:
        vote_out.free()
        db.free()
    masks = [counters[pf.frame_slice(f)] >= 0 for f in range(len(f3s))]                                  # :166
    rec = Reconstruct(cam, ctx=ctx, delaunay_workers=estimator.delaunay_workers)
    rows = rec._rows_for(f2s, masks, "scipy")
    if estimator.check_triangle == "fixed":
        rows = [packing.canonical_rows(t) for t in rows]
    res = rec.depth_maps(f3s, f2s, tris=rows, keeps=masks, ids=ids)
    res.depth *= scales[:, None, None]
    return res, scales
