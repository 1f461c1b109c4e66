"""``GraphGrow`` of the reference — /root/reference/src/graph.py:39-107, built by rescale.ScaleEstimator (rescale.py:33), its
call site rescale.py:99 — backed by ``region_grow_kernel`` (mvosr_region_grow_batch, include/mvosr.h).

    from mvoscalerecovery_amd.graph import GraphGrow
    rows = GraphGrow().process(triangle_ids, heights, angles)

Rows of a triangulation that share an edge are joined when their pitch differs by less than ``threshold_angle`` degrees and
their inverse height by less than 0.4 * median(1 / heights) (graph.py:73-77,93); the reference grows a proposal from each of 100
random flat seeds — ``expend`` compares a row with the row it came from, so a proposal is its seed's connected component — and
keeps the longest (graph.py:97-103).  Declared rule here: the largest component that holds a flat seed, the one with the
smallest row index among equally large ones, returned as ASCENDING row indices (the reference's order is its random walk's;
the RANSAC that consumes the list samples positions uniformly).  The reference recurses once per row and exceeds Python's
recursion limit on frames of a thousand rows; one workgroup per frame labels the components here whatever their diameter.
"""
from __future__ import annotations

import ctypes as C
import numbers

import numpy as np

from . import _lib
from . import constants as K

SEED_DEG, LEVEL_DEG, HEIGHT_FACTOR = -85.0, -80.0, 0.4        # graph.py:90,91,93
MAX_VERTEX_ID = 65535                                         # 16-bit ids in LDS (mvosr_region_grow_batch)


def check_threshold(threshold_angle):
    if isinstance(threshold_angle, bool) or not isinstance(threshold_angle, numbers.Real) or not threshold_angle == threshold_angle:
        raise ValueError("threshold_angle must be a real number of degrees, not %r" % (threshold_angle,))
    return float(threshold_angle)


def check_frame(f, tri, heights, angles):
    """One frame's ``process`` arguments as (rows int32 [T,3], heights float64 [T], angles float64 [T]); ValueError naming the frame."""
    tri = np.asarray(tri)
    if tri.ndim != 2 or tri.shape[1] != 3 or tri.shape[0] == 0:
        raise ValueError("frame %d: triangle_ids must be a non-empty (T, 3) array, not %r" % (f, tri.shape))
    if not np.issubdtype(tri.dtype, np.integer):
        raise ValueError("frame %d: triangle_ids must be integers, not %s" % (f, tri.dtype))
    if tri.min() < 0 or tri.max() > MAX_VERTEX_ID - 1:
        raise ValueError("frame %d: vertex ids must lie in [0, %d)" % (f, MAX_VERTEX_ID))
    h, a = np.asarray(heights, dtype=np.float64).reshape(-1), np.asarray(angles, dtype=np.float64).reshape(-1)
    if len(h) != len(tri) or len(a) != len(tri):
        raise ValueError("frame %d: %d rows, %d heights, %d angles" % (f, len(tri), len(h), len(a)))
    return np.ascontiguousarray(tri, dtype=np.int32), h, a


def launch(ctx, b, n_frames, n_rows, max_tri, threshold_angle, heights=None, angles=None, aux=True, values=False):
    """mvosr_region_grow_batch over a prepared ``_lib.Batch`` whose tri2 holds ``n_rows`` rows in all.  ``heights`` / ``angles``
    (device buffers): the given form; both None: from the batch's x/y/z.  -> dict of NumPy arrays (region, n_region, n_flat,
    status, level, threshold_height; label, neighbors with ``aux``; tri_height, tri_angle with ``values``)."""
    T = max(int(n_rows), 1)
    spec = {"region": (T, np.uint8), "n_region": (n_frames, np.int32), "n_flat": (n_frames, np.int32), "status": (n_frames, np.int32),
            "level": (n_frames, np.float64), "threshold_height": (n_frames, np.float64)}
    if aux:
        spec.update(label=(T, np.int32), neighbors=((T, 3), np.int32))
    if values:
        spec.update(tri_height=(T, np.float64), tri_angle=(T, np.float64))
    bufs = {k: ctx.zeros(shape, dt) for k, (shape, dt) in spec.items()}
    o = _lib.GrowOutputs(**{k: v.ptr for k, v in bufs.items()})
    gp = _lib.GrowParams(float(threshold_angle), SEED_DEG, LEVEL_DEG, HEIGHT_FACTOR)
    try:
        _lib.check(ctx.lib.mvosr_region_grow_batch(ctx.handle, C.byref(b), heights.ptr if heights is not None else None,
                                                   angles.ptr if angles is not None else None, C.byref(gp), C.byref(o), int(max_tri)),
                   "mvosr_region_grow_batch")
        ctx.sync()
        return {k: v.download() for k, v in bufs.items()}
    finally:
        for v in bufs.values():
            v.free()


class GraphGrow:
    """Drop-in for the reference's class (graph.py:39-107); ``last`` keeps the labels, neighbours, flat-seed counts and levels of
    the latest call, per frame."""

    def __init__(self, threshold_angle=8, device=0, ctx=None):
        self.threshold_angle = check_threshold(threshold_angle)       # graph.py:41
        self.threshold_height = 0.2                                   # graph.py:42
        self.device = int(device)
        self._ctx = ctx
        self.last = {}

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = _lib.default_context(self.device)
        return self._ctx

    def process(self, triangle_ids, heights, angles):
        """graph.py:85-107: the grown region's rows, ascending; [] when nothing is flat (graph.py:95-96)."""
        return self.process_batch([triangle_ids], [heights], [angles])[0]

    def process_batch(self, tris, heights, angles):
        if not (len(tris) == len(heights) == len(angles)):
            raise ValueError("process_batch: %d triangulations, %d height arrays, %d angle arrays" % (len(tris), len(heights), len(angles)))
        frames = [check_frame(f, *x) for f, x in enumerate(zip(tris, heights, angles))]
        if not frames:
            return []
        ctx = self.ctx
        cnt = np.array([int(t.max()) + 1 for t, _, _ in frames], dtype=np.int32)              # graph.py:50-51
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        toff = np.concatenate([[0], np.cumsum([len(t) for t, _, _ in frames])]).astype(np.int64)
        d = [ctx.to_device(off), ctx.to_device(cnt), ctx.to_device(toff), ctx.to_device(np.concatenate([t for t, _, _ in frames]).reshape(-1)),
             ctx.to_device(np.concatenate([h for _, h, _ in frames])), ctx.to_device(np.concatenate([a for _, _, a in frames]))]
        b = _lib.Batch()
        b.n_frames, b.feat_off, b.feat_cnt, b.tri2_off, b.tri2 = len(frames), d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr
        b.max_feat, b.total_feat = int(cnt.max()), int(off[-1])
        try:
            r = launch(ctx, b, len(frames), int(toff[-1]), int(np.max(np.diff(toff))), self.threshold_angle, d[4], d[5])
        finally:
            for buf in d:
                buf.free()
        bad = np.nonzero(r["status"] == K.ST_ERR_MASK)[0]
        if len(bad):
            raise ValueError("GraphGrow: frame %d has an edge on more than two rows, a row that names a vertex twice, or a height "
                             "that is not finite and positive" % int(bad[0]))
        split = lambda a: [a[toff[f]:toff[f + 1]] for f in range(len(frames))]
        self.last = {"label": split(r["label"]), "neighbors": split(r["neighbors"]), "n_flat": r["n_flat"], "level": r["level"],
                     "threshold_height": r["threshold_height"], "n_region": r["n_region"]}
        self.threshold_height = float(r["threshold_height"][-1])                              # graph.py:93
        return [np.nonzero(reg)[0].tolist() for reg in split(r["region"])]
