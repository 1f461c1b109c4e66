"""The device-resident chunk driver of the height-and-pitch objects (height_pitch.HeightPitchEstimator, RansacEvaluation,
RansacBudgetSweep with ``triangulation="gpu", resident=True``): a call's frames go through the device in chunks
on the shared pipeline (``stream.run``), per chunk ONE upload, ``mvosr_delaunay_batch``, the object's kernel and its tail on the
context's stream, the rows in HBM in between and the cross-frame state handed from chunk to chunk in a chain of device records.

:class:`ResidentCall` is one call's state and the whole control flow; what differs between the objects comes in as the methods a
subclass writes (as ``stream.py`` takes values and callables).  With it the pieces both kinds of chunk are made of — the feature
planes, the upload and triangulation, the batch header, the host's rows for a declined frame — and the one mapping from the tails'
error kinds to the scripts' exceptions."""
import numpy as np

from . import _lib, packing, stream


def _pack_planes(pts):
    """``height_pitch._pack_frames``' feature planes and offsets from ONE concatenate over the frames -> (planes (3, total), feat_off, feat_cnt)."""
    cnt = np.fromiter((len(p) for p in pts), dtype=np.int32, count=len(pts))
    even = (cnt.astype(np.int64) + 1) & ~1
    off = np.concatenate([[0], np.cumsum(even)[:-1]]).astype(np.int64)              # even segment starts
    planes = np.zeros((3, max(int(off[-1] + even[-1]), 2)), dtype=np.float64)
    start = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))[:-1]])
    where = np.repeat(off - start, cnt) + np.arange(int(cnt.sum()), dtype=np.int64)
    planes[:, where] = np.concatenate(pts).T
    return planes, off, cnt


def batch_header(din, F, max_feat, total_feat, tri1_off, tri1, tri1_cnt=None):
    """The batch header of the height-and-pitch launches over the block ``din``: the rows at ``tri1`` from ``tri1_off`` — back to back
    (the staged launches) or, with ``tri1_cnt``, in slots with a count each (the resident chunks)."""
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt = F, din["feat_off"].ptr, din["feat_cnt"].ptr
    b.x, b.v, b.z = din["u"].ptr, din["v"].ptr, din["z"].ptr
    b.tri1_off, b.tri1 = tri1_off, tri1
    if tri1_cnt is not None:
        b.tri1_cnt = tri1_cnt
    b.max_feat, b.total_feat = max_feat, total_feat
    return b


def resident_rows_stage(ctx, pts, extra_in=(), extra_arrays=None):
    """A chunk's frames uploaded ONCE and triangulated on the device, the rows left in HBM for the kernel that consumes them:
    -> dict with ``din`` (feat_off, feat_cnt, u, v, z, tri_off = 2 feat_off, and ``extra_in``'s arrays), ``tri`` (canonical rows at
    3 tri_off[f], room for 2 n), ``dt`` (tri_cnt, dt_status, dt_used), ``off``, ``cnt`` and ``total``.  Everything is queued on the
    context's stream; nothing is waited for."""
    planes, off, cnt = _pack_planes(pts)
    F, total = len(pts), planes.shape[1]
    din = ctx.block([("feat_off", F, np.int64), ("feat_cnt", F, np.int32), ("u", total, np.float64), ("v", total, np.float64),
                     ("z", total, np.float64), ("tri_off", F, np.int64)] + list(extra_in))
    tri = dt = None
    try:
        tri = ctx.block([("tri", 6 * total, np.int32)])
        dt = ctx.block([("tri_cnt", F, np.int32), ("dt_status", F, np.int32), ("dt_used", F, np.int32)])
        arrays = {"feat_off": off, "feat_cnt": cnt, "u": planes[0], "v": planes[1], "z": planes[2], "tri_off": 2 * off}
        arrays.update(extra_arrays or {})
        din.upload(arrays)
        dt.zero()
        _lib.check(ctx.lib.mvosr_delaunay_batch(ctx.handle, F, din["feat_off"].ptr, din["feat_cnt"].ptr, din["u"].ptr, din["v"].ptr, None,
                                                int(cnt.max()), din["tri_off"].ptr, tri["tri"].ptr, dt["tri_cnt"].ptr, dt["dt_used"].ptr,
                                                dt["dt_status"].ptr), "mvosr_delaunay_batch")
    except BaseException:
        for blk in (din, tri, dt):
            if blk is not None:
                blk.free()
        raise
    return {"din": din, "tri": tri, "dt": dt, "off": off, "cnt": cnt, "total": total}


def patch_declined_rows(ctx, st, pts, declined, workers):
    """The frames ``declined`` of a :func:`resident_rows_stage` chunk (``pts``: their points) through SciPy: the rows in canonical form
    into the frames' own slots of the chunk's row slab, ``tri_cnt`` patched.  A SciPy exception: -> (its frame, the exception), the
    frames behind it left as they were; else None."""
    lib, off = ctx.lib, st["off"]
    rows = packing.delaunay_many([np.ascontiguousarray(p[:, 0:2]) for p in pts], workers)
    for f, t in zip(declined, rows):
        if isinstance(t, Exception):
            return f, t
        t = np.ascontiguousarray(packing.canonical_rows(t), dtype=np.int32)
        assert len(t) <= 2 * int(st["cnt"][f])                                      # (a planar triangulation of n points: at most 2n - 5 rows)
        n_rows = np.array([len(t)], dtype=np.int32)
        _lib.check(lib.mvosr_memcpy_h2d(ctx.handle, st["tri"]["tri"].ptr + 24 * int(off[f]), _lib.addr(t), t.nbytes), "h2d")
        _lib.check(lib.mvosr_memcpy_h2d(ctx.handle, st["dt"]["tri_cnt"].ptr + 4 * f, _lib.addr(n_rows), 4), "h2d")
    return None


def frame_error(kind, frame, budget=None):
    """The exception the scripts raise where the tails stop with error ``kind`` (MVOSR_HPT_ERR_*; 0: none -> None) at ``frame``, the
    frame's number as the host loop would print it; ``budget``: the iteration budget a sweep names."""
    if kind == _lib.HPT_ERR_SINGULAR:
        return np.linalg.LinAlgError("Singular matrix")                              # :83 (_eval.py:101)
    if kind in (_lib.HPT_ERR_MASK, _lib.HPT_ERR_EMPTY):
        return ValueError("frame %d: %s" % (frame, "no features or no triangles" if kind == _lib.HPT_ERR_EMPTY else
                                            "a triangle names a vertex outside the frame"))
    if kind == _lib.HPT_ERR_NO_MODEL:
        return ValueError("frame %d: no sample of the RANSAC had an inlier" % frame + ("" if budget is None else " at budget %d" % budget))
    if kind == _lib.HPT_ERR_NO_PREVIOUS:                 # :167 indexes the 1-D norm_prev of :45 with two indices (_eval.py: :188, :55)
        return IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")
    if kind:
        return RuntimeError("frame %d: the tail stopped with error %d" % (frame, kind))
    return None


class ResidentCall:
    """One call of ``owner`` (its ``ctx``, ``delaunay_workers``, ``declined_total``, ``GPU_PIPELINE`` and ``GPU_SIDE_DOWNLOADS``) over the
    frames ``pts`` with the carry-in record ``carry0``: the chunks in flight, the chain of carry records (chunk k: ``chain[k]`` ->
    ``chain[k + 1]``), and per collected chunk the triangulation's status words and the tail's error word.  A subclass writes

      ``inputs(a, b)``        -> (spec, arrays) of what frames ``a:b`` upload next to the feature planes
      ``block_specs(st)``     -> (spec of ``out``, the kernel's outputs, spec of ``small``, what comes back; it ends in ``error``)
      ``structs(st)``         the kernel's and the tail's parameter and output structs into ``st``
      ``kernel(st)``          the launch over the chunk
      ``launch_tail(st, n)``  the tail over the chunk's first ``n`` frames, ``chain[k]`` -> ``chain[k + 1]``
      ``decode(err, n)``      -> (kind, final frames, budget or None) of the error word of a tail over ``n`` frames
      ``apply(st, n, bad)``   the chunk's first ``bad`` records to where the object keeps them
      ``error_frame(st, bad)``  the frame number an exception names, asked after ``apply``
      ``epilogue()``          what the object's host state takes from the call, while the chain is still there."""

    def __init__(self, owner, pts, carry0):
        self.owner, self.ctx, self.pts, self.carry0 = owner, owner.ctx, pts, carry0
        self.chain, self.inflight, self.dt_status, self.errors = [], [], [], []

    def start(self, a, b, k):
        """Chunk ``k`` = frames ``a:b`` of the call: ONE upload, then the triangulation, the kernel and the tail queued on the
        context's stream, and the download of the chunk's small records behind them.  Nothing is waited for."""
        ctx, F = self.ctx, b - a
        st = resident_rows_stage(ctx, self.pts[a:b], *self.inputs(a, b))
        st.update(k=k, a=a, b=b, side=[st["din"], st["tri"], st["dt"]])             # (side: the blocks stream.free_blocks releases)
        self.inflight.append(st)
        try:
            din = st["din"]
            out_spec, small_spec = self.block_specs(st)
            out = st["out"] = ctx.block(out_spec)
            st["small"] = ctx.block(small_spec)
            st["side"].append(st["small"])
            out.zero()
            st["header"] = batch_header(din, F, int(st["cnt"].max()), st["total"], din["tri_off"].ptr, st["tri"]["tri"].ptr, st["dt"]["tri_cnt"].ptr)
            self.structs(st)
            self.kernel(st)
            while len(self.chain) < k + 2:                                           # chunk k: chain[k] -> chain[k + 1]
                self.chain.append(ctx.empty(len(self.carry0), np.uint8))
            self.tail(st, F)
            for blk in (din, st["tri"], out):
                blk.mark(True)
        except BaseException:
            self.inflight.remove(st)
            stream.free_blocks(st)
            raise
        return st

    def tail(self, st, n_frames, download=True):
        """The tail over the chunk's first ``n_frames`` frames, then (``download``) the chunk's small records and the triangulation's
        status words on their way to page-locked memory — through the pipeline's side download (a copy kernel) where the knob allows it,
        as the rescale path."""
        self.launch_tail(st, int(n_frames))
        for blk in (st["dt"], st["small"]) if download else ():
            blk.mark(False)
            if self.owner.GPU_SIDE_DOWNLOADS:
                blk.mark_done()
            else:
                blk.prefetch()
            blk.mark(True)

    def redo(self, st, declined):
        """The frames of the chunk the device triangulation declined: SciPy's rows in canonical form into the frames' own slots of
        the chunk's row slab, ``tri_cnt`` patched, the kernel run again over the chunk, and the tails of this chunk and of every chunk
        queued behind it (their carry-in changed).  A SciPy exception: -> (its frame, the exception), the tail run over the frames
        before it only."""
        for blk in (st["din"], st["tri"], st["out"]):
            blk.mark(False)
        stop = patch_declined_rows(self.ctx, st, [self.pts[st["a"] + f] for f in declined], declined, self.owner.delaunay_workers)
        self.kernel(st)
        n = st["b"] - st["a"] if stop is None else stop[0]
        if n > 0:
            self.tail(st, n)
        if stop is None:
            for later in self.inflight:
                if later["k"] > st["k"]:
                    self.tail(later, later["b"] - later["a"])
        for blk in (st["din"], st["tri"], st["out"]):
            blk.mark(True)
        return stop

    def collect(self, st):
        """Wait for the chunk's records, send its declined frames through the host, hand the final records to the object in sequence
        order, and raise where the host loop raises."""
        cnt, F = st["cnt"], st["b"] - st["a"]
        dt_status = st["dt"]["dt_status"].download()
        declined = [f for f in range(F) if dt_status[f] != 0 and cnt[f] >= 3]
        self.owner.declined_total += len(declined) + int(np.count_nonzero(cnt < 3))
        stop = self.redo(st, declined) if declined else None
        n = F if stop is None else stop[0]
        err = int(st["small"]["error"].download()[0]) if n else -1
        kind, bad, budget = self.decode(err, n)
        self.dt_status.append(dt_status)
        self.errors.append(err)
        self.apply(st, n, bad)
        self.inflight.remove(st)
        stream.free_blocks(st)
        error = frame_error(kind, self.error_frame(st, bad), budget)
        if error is not None:
            raise error
        if stop is not None:
            raise stop[1]
        return n

    def run(self, plan):
        """The chunks of ``plan`` (``(a, b, None)`` each) through ``stream.run``; the chain is freed whatever happens, after ``epilogue``."""
        try:
            self.chain.append(self.ctx.to_device(self.carry0))
            stream.run(plan, lambda a, b, tables, k: self.start(a, b, k), lambda st, a, b, last: self.collect(st), self.owner.GPU_PIPELINE,
                       lambda st: stream.free_blocks(st), [], lambda: None)
        finally:
            try:
                self.epilogue()
            finally:
                for buf in self.chain:
                    buf.free()
