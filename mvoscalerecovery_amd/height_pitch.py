"""GPU mirror of the per-frame camera-height and road-pitch estimator /root/reference/src/calculate_height_pitch.py: per
frame of ``[u, v, depth]`` features and a pitch prior from the camera motion, the RANSAC road plane over the triangles the
prior admits, its inliers among all points, and from them the camera height, a refined pitch, and the height under the
prior's pitch — :class:`HeightPitchEstimator`.

Its two siblings ``calculate_height_pitch_eval.py`` and ``calculate_height_pitch_eval_line.py`` share the rows and the point
list with it and nothing after: they run the whole sequence ten times at an iteration budget from the command line, take the
inliers among the LIST points (repeats included), refine over those, and — the line script — fit the 2-D line model in
(y, z), the one place in the reference where the line RANSAC decides a result.  :class:`RansacEvaluation` is both of them
(``mvosr_height_pitch_eval_batch``).

The reference is a Python-2 script over text dumps that writes six result files at its end; here the frame loop's body is
ONE kernel launch for a batch of frames (``mvosr_height_pitch_batch``) and the script's cross-frame state —
a frame with fewer than 12 list points repeats the previous frame's plane and inliers (:163-165) — is kept by
:class:`HeightPitchEstimator`.  The triangulation's rows are built on the host (SciPy) or on the device and visit the
host either way on the default path; ``HeightPitchEstimator(triangulation="gpu", resident=True)`` keeps a call's frames on the
device from their upload to the six result values — rows in HBM between ``mvosr_delaunay_batch`` and the kernel, the cross-frame
state applied by ``mvosr_height_pitch_tail_batch``, chunks streamed on the shared pipeline (``stream.py``).
``RansacEvaluation`` / ``RansacBudgetSweep(triangulation="gpu", resident=True)`` are on the same path with a tail of their own,
``mvosr_height_pitch_eval_tail_batch``, which writes the (budgets, cases, frames) arrays ``run`` returns.
The line RANSAC of :146 is printed by the base script and never used there: the estimator does not compute it (the evaluation's
line model does)."""
from __future__ import annotations

import collections
import ctypes as C
import math
import os

import numpy as np

from . import _lib, packing, stream

FOCUS, CX, CY = 718.856, 607.1928, 185.2157        # calculate_height_pitch.py:15-17
PI_SCRIPT = 3.1415926                               # :63, :91
MIN_POINTS = 12                                     # :140
GOAL_FRACTION = 0.8                                 # estimate_road_norm.py:68
ST_RS_FEW, ST_ERR_SINGULAR, ST_ERR_MASK, ST_ERR_EMPTY = 11, 7, 8, 9

# the script's six result files (:228-244), in the order run_sequence returns the arrays
RESULT_FILES = ("result_heights_line_ransac.txt", "refined_camera_height_means.txt", "refined_camera_height_stds.txt",
                "refined_camera_height_t_means.txt", "refined_pitch.txt", "inlier_numbers.txt")
RESULT_FIELDS = ("ransac_height", "refined_mean", "refined_std", "height_t_mean", "refined_pitch", "n_inliers")

RESIDENT_ERROR = "resident=True belongs to triangulation='gpu': the rows stay where the device triangulation wrote them"

FrameResult = collections.namedtuple("FrameResult", RESULT_FIELDS + ("n_selected", "carried"))


def estimated_pitches(motion_ts, first, count):
    """``get_pitch(motion_ts[0:k+1])`` (:62; estimate_road_norm.py:52-58) for k = first .. first + count - 1, from ONE running
    sum: NumPy adds the rows of ``motion_ts[0:k+1]`` in order, so the cumulative sum's row k is that sum, bit for bit."""
    t = np.asarray(motion_ts, dtype=np.float64)[:, 0:3]
    first, count = int(first), int(count)
    if first < 0 or first + count > len(t):
        raise IndexError("motion_ts has %d rows, frames %d..%d asked for" % (len(t), first, first + count - 1))
    run = np.cumsum(t[:first + count], axis=0)[first:]
    return np.array([math.asin(-m[1] / float(m @ m)) for m in run], dtype=np.float64)


def frame_prior(estimated_pitch):
    """The four doubles the kernel takes per frame: the window's edges in degrees as the script forms them (:63, :111), and
    math.sin / math.cos of the prior (:202)."""
    est = float(estimated_pitch)
    deg = est * 180 / PI_SCRIPT
    return deg - 95, deg - 85, math.sin(est), math.cos(est)


def back_project(points3d, focus=FOCUS, cx=CX, cy=CY):
    """:66-68, the script's expression (the kernel's, operation for operation)."""
    p = np.array(points3d, dtype=np.float64)
    p[:, 0] = p[:, 2] * (p[:, 0] - cx) / focus
    p[:, 1] = p[:, 2] * (p[:, 1] - cy) / focus
    return p


def _pack_frames(pts, rows, priors):
    """The batch both launches upload: feature planes at even segment starts, the rows back to back, the priors.
    -> (spec_in, arrays, feat_off, tri_off, planes, total rows (at least 1))"""
    F = len(pts)
    cnt = np.array([len(p) for p in pts], dtype=np.int32)
    off = np.zeros(F, dtype=np.int64)
    off[1:] = np.cumsum((cnt[:-1].astype(np.int64) + 1) & ~1)                       # even segment starts
    total = int(off[-1]) + ((int(cnt[-1]) + 1) & ~1)
    planes = np.zeros((3, max(total, 2)), dtype=np.float64)
    for f, p in enumerate(pts):
        planes[:, off[f]:off[f] + len(p)] = p.T
    tcnt = np.array([len(t) for t in rows], dtype=np.int64)
    toff = np.concatenate([[0], np.cumsum(tcnt)]).astype(np.int64)
    T = max(int(toff[-1]), 1)
    tri = np.concatenate(rows + [np.zeros((0, 3), np.int32)]).astype(np.int32).reshape(-1)
    tri = tri if tri.size else np.zeros(3, dtype=np.int32)
    spec_in = [("feat_off", F, np.int64), ("feat_cnt", F, np.int32), ("u", planes.shape[1], np.float64), ("v", planes.shape[1], np.float64),
               ("z", planes.shape[1], np.float64), ("tri1_off", F + 1, np.int64), ("tri1", tri.size, np.int32), ("prior", (F, 4), np.float64)]
    arrays = {"feat_off": off, "feat_cnt": cnt, "u": planes[0], "v": planes[1], "z": planes[2], "tri1_off": toff, "tri1": tri,
              "prior": np.ascontiguousarray(np.asarray(priors, dtype=np.float64).reshape(F, 4))}
    return spec_in, arrays, off, toff, planes, T


def _delaunay_rows(ctx, pts2d, triangulation, workers):
    todo = [f for f, p in enumerate(pts2d) if len(p) >= 3]
    rows = [np.zeros((0, 3), dtype=np.int32)] * len(pts2d)
    if triangulation == "gpu":
        got = packing.delaunay_gpu_or_host(ctx, [pts2d[f] for f in todo], workers, canonical=True)
    else:
        got = packing.delaunay_many([pts2d[f] for f in todo], workers)
    for f, t in zip(todo, got):
        if isinstance(t, Exception):
            raise t
        rows[f] = np.ascontiguousarray(t, dtype=np.int32)
    return rows


def _pack_planes(pts):
    """``_pack_frames``' feature planes and offsets from ONE concatenate over the frames -> (planes (3, total), feat_off, feat_cnt)."""
    cnt = np.fromiter((len(p) for p in pts), dtype=np.int32, count=len(pts))
    even = (cnt.astype(np.int64) + 1) & ~1
    off = np.concatenate([[0], np.cumsum(even)[:-1]]).astype(np.int64)              # even segment starts
    planes = np.zeros((3, max(int(off[-1] + even[-1]), 2)), dtype=np.float64)
    start = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))[:-1]])
    where = np.repeat(off - start, cnt) + np.arange(int(cnt.sum()), dtype=np.int64)
    planes[:, where] = np.concatenate(pts).T
    return planes, off, cnt


# mvosr_height_pitch_tail_frame, mvosr_height_pitch_carry (include/mvosr.h)
TAIL_FRAME = np.dtype([(k, "<f8") for k in ("ransac_height", "refined_mean", "refined_std", "height_t_mean", "refined_pitch")] +
                      [(k, "<i4") for k in ("n_inliers", "n_selected", "carried", "source")])
CARRY_HEADER = np.dtype([(k, "<f8") for k in ("ransac_height", "refined_mean", "refined_std", "height_t_mean", "refined_pitch")] +
                        [(k, "<i4") for k in ("n_inliers", "has_prev", "count", "halted")] + [("reserved", "<i8")])


def carry_record(cap, prev=None, inliers=None, index=None):
    """A carry record of capacity ``cap`` as bytes: the header, then y, z and index (mvosr_height_pitch_carry).  ``prev``: the
    previous frame's six values (anything with RESULT_FIELDS' attributes), ``inliers`` its (k, 3) back-projected inliers."""
    cap, y0 = (int(cap) + 1) & ~1, CARRY_HEADER.itemsize
    rec = np.zeros(-(-(y0 + 20 * cap) // 16) * 16, dtype=np.uint8)
    if prev is not None:
        h = rec[:y0].view(CARRY_HEADER)
        for k in RESULT_FIELDS:
            h[k] = getattr(prev, k)
        k = len(inliers)
        h["has_prev"], h["count"] = 1, k
        rec[y0:y0 + 8 * k].view(np.float64)[:] = inliers[:, 1]
        rec[y0 + 8 * cap:y0 + 8 * cap + 8 * k].view(np.float64)[:] = inliers[:, 2]
        if index is not None:
            rec[y0 + 16 * cap:y0 + 16 * cap + 4 * k].view(np.int32)[:] = index
    return rec


def carry_fields(rec, cap):
    """(header (a CARRY_HEADER scalar), y, z, index) of a carry record's bytes, the arrays cut to the header's count."""
    cap, y0 = (int(cap) + 1) & ~1, CARRY_HEADER.itemsize
    h = rec[:y0].view(CARRY_HEADER)[0]
    k = int(h["count"])
    return (h, rec[y0:y0 + 8 * k].view(np.float64), rec[y0 + 8 * cap:y0 + 8 * cap + 8 * k].view(np.float64),
            rec[y0 + 16 * cap:y0 + 16 * cap + 4 * k].view(np.int32))


def resident_rows_stage(ctx, pts, extra_in=(), extra_arrays=None):
    """A chunk's frames uploaded ONCE and triangulated on the device, the rows left in HBM for the kernel that consumes them:
    -> dict with ``din`` (feat_off, feat_cnt, u, v, z, tri_off = 2 feat_off, and ``extra_in``'s arrays), ``tri`` (canonical rows at
    3 tri_off[f], room for 2 n), ``dt`` (tri_cnt, dt_status, dt_used), ``off``, ``cnt`` and ``total``.  Everything is queued on the
    context's stream; nothing is waited for.  (The estimator's chunks and the evaluation objects' both start here.)"""
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


def _batch_header(din, F, max_feat, total_feat):
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt = F, din["feat_off"].ptr, din["feat_cnt"].ptr
    b.x, b.v, b.z = din["u"].ptr, din["v"].ptr, din["z"].ptr
    b.tri1_off, b.tri1 = din["tri1_off"].ptr, din["tri1"].ptr
    b.max_feat, b.total_feat = max_feat, total_feat
    return b


class HeightPitchEstimator:
    """The script's frame loop as an object: ``process`` / ``process_batch`` take frames in sequence order and keep what the
    script carries from one frame to the next; the six result lists grow as the script's do."""

    # the resident path's chunks (the streamed path's knobs, stream.StreamKnobs; tests and profiles override them per instance)
    GPU_CHUNK = stream.StreamKnobs.GPU_CHUNK
    GPU_MIN_CHUNK = stream.StreamKnobs.GPU_MIN_CHUNK
    GPU_CHUNK_POINTS = stream.StreamKnobs.GPU_CHUNK_POINTS
    GPU_PIPELINE = stream.StreamKnobs.GPU_PIPELINE
    GPU_SIDE_DOWNLOADS = stream.StreamKnobs.GPU_SIDE_DOWNLOADS

    def __init__(self, focus=FOCUS, cx=CX, cy=CY, max_iterations=500, threshold=0.005, inlier_threshold=0.01, seed=None, device=0,
                 triangulation="scipy", delaunay_workers=0, resident=False):
        if triangulation not in ("scipy", "gpu"):
            raise ValueError("triangulation must be 'scipy' or 'gpu'")
        # resident: opt-in.  False: every path, message and state below is what it was.
        if resident and triangulation != "gpu":
            raise ValueError(RESIDENT_ERROR)
        self.resident = bool(resident)
        self.declined_total = 0                        # resident path: frames whose rows came from the host (or that have no rows: < 3 points)
        self.ctx = _lib.default_context(device)
        self.focus, self.cx, self.cy = float(focus), float(cx), float(cy)
        self.max_iterations, self.threshold, self.inlier_threshold = int(max_iterations), float(threshold), float(inlier_threshold)
        # (the reference seeds its sampler from OS entropy on every call, ransac.py:6: without a seed, so does this object, once)
        self.seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed) & (2 ** 64 - 1)
        self.triangulation = triangulation
        self.delaunay_workers = delaunay_workers
        self.frame_count = 0                           # frames seen: the sample sequence's frame counter
        self._prev = None                              # the last frame's FrameResult and its inliers (:163-165, and `inliers` itself)
        self.results = {k: [] for k in RESULT_FIELDS}
        self.last = None                               # the last launch's per-frame device outputs (parity tests)

    # ---- rows
    def _rows_for(self, pts2d):
        return _delaunay_rows(self.ctx, pts2d, self.triangulation, self.delaunay_workers)

    # ---- one launch
    def launch(self, points3d_list, priors, triples=None, tris=None, frame_base=None, stage=False, max_feat=None, timing=0):
        """``mvosr_height_pitch_batch`` over the frames -> dict of per-frame host arrays (``mask`` / ``point_list``: lists).
        ``priors``: (F, 4) as :func:`frame_prior`.  ``triples``: None (the device draws), or per frame an (H, 3) array of list
        positions (None / shorter: the missing samples are spent).  ``stage``: also ``hyp_counts`` and ``point_list``.
        ``max_feat``: what the batch header states (default: the largest frame; a larger frame is refused by the kernel).
        ``timing`` > 0: the launch is repeated that often on the resident batch between two events; ``kernel_ms`` is one launch's share."""
        ctx, lib = self.ctx, self.ctx.lib
        pts = [np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 3)) for p in points3d_list]
        F, H = len(pts), self.max_iterations
        if F == 0:
            return None
        rows = [np.ascontiguousarray(np.asarray(t, dtype=np.int32).reshape(-1, 3)) for t in tris] if tris is not None \
            else self._rows_for([np.ascontiguousarray(p[:, 0:2]) for p in pts])
        cnt = np.array([len(p) for p in pts], dtype=np.int32)
        max_feat = int(cnt.max()) if max_feat is None else int(max_feat)
        need = int(lib.mvosr_height_pitch_lds_bytes(max_feat, H))
        if need > ctx.lds_per_block:
            raise ValueError("a frame of %d features needs %d bytes of LDS, the device has %d" % (max_feat, need, ctx.lds_per_block))
        spec_in, arrays, off, toff, planes, T = _pack_frames(pts, rows, priors)
        if triples is not None:
            tr = np.full((F, H, 3), -1, dtype=np.int32)                             # (-1: outside every list, the sample is spent)
            for f, t in enumerate(triples):
                if t is not None and len(t):
                    t = np.asarray(t, dtype=np.int32).reshape(-1, 3)[:H]
                    tr[f, :len(t)] = t
            spec_in.append(("triples", (F, H, 3), np.int32))
            arrays["triples"] = tr
        spec_out = [("ransac_height", F, np.float64), ("model", (F, 4), np.float64), ("best_ic", F, np.int32), ("used", F, np.int32),
                    ("n_selected", F, np.int32), ("n_inliers", F, np.int32), ("refined_normal", (F, 3), np.float64),
                    ("refined_pitch", F, np.float64), ("refined_mean", F, np.float64), ("refined_std", F, np.float64),
                    ("height_t_mean", F, np.float64), ("status", F, np.int32), ("mask", planes.shape[1], np.uint8)]
        if stage:
            spec_out += [("point_list", 3 * T, np.int32), ("hyp_counts", (F, H), np.int32)]
        din, dout = ctx.block(spec_in), ctx.block(spec_out)
        try:
            din.upload(arrays)
            dout.zero()
            b = _batch_header(din, F, max_feat, planes.shape[1])
            p = _lib.HeightPitchParams(self.focus, self.cx, self.cy, MIN_POINTS, H, self.threshold, GOAL_FRACTION, self.inlier_threshold,
                                       self.seed, int(self.frame_count if frame_base is None else frame_base))
            o = _lib.HeightPitchOutputs(*[(dout[k].ptr if k in dout else None) for k, _ in _lib.HeightPitchOutputs._fields_])
            def call():
                _lib.check(lib.mvosr_height_pitch_batch(ctx.handle, C.byref(b), C.byref(p), din["prior"].ptr,
                                                        din["triples"].ptr if triples is not None else None, C.byref(o)),
                           "mvosr_height_pitch_batch")
            call()
            kernel_ms = None
            if timing > 0:
                ev = ctx.event(), ctx.event()
                ctx.record(ev[0])
                for _ in range(int(timing)):
                    call()
                ctx.record(ev[1])
                kernel_ms = ctx.elapsed_ms(*ev) / int(timing)
                for e in ev:
                    lib.mvosr_event_destroy(ctx.handle, e)
            res = {k: dout[k].download() for k, _, _ in spec_out}
            if kernel_ms is not None:
                res["kernel_ms"] = kernel_ms
        finally:
            din.free()
            dout.free()
        res["mask"] = [res["mask"][off[f]:off[f] + cnt[f]].astype(bool) for f in range(F)]
        if stage:
            res["point_list"] = [res["point_list"][3 * toff[f]:3 * toff[f] + max(int(res["n_selected"][f]), 0)] for f in range(F)]
        res["rows"] = rows
        return res

    # ---- the script's loop
    def process_batch(self, points3d_list, estimated_pitches, triples=None, tris=None):
        """Frames in sequence order through one launch, then the script's cross-frame rule frame by frame.  Returns one
        :class:`FrameResult` per frame and appends to ``self.results``.  Raises where the script raises: ``np.linalg.LinAlgError``
        for a singular row (:83), ``IndexError`` for a first frame with fewer than 12 list points (:167)."""
        ests = [float(e) for e in np.asarray(estimated_pitches, dtype=np.float64).reshape(-1)]
        if len(ests) != len(points3d_list):
            raise ValueError("one estimated pitch per frame")
        if self.resident:
            if tris is not None:
                raise ValueError("resident=True triangulates on the device: tris= belongs to the staged path")
            return self._process_resident(points3d_list, ests, triples)
        res = self.launch(points3d_list, [frame_prior(e) for e in ests], triples=triples, tris=tris)
        self.last = res
        out = []
        for f, est in enumerate(ests):
            st = int(res["status"][f])
            if st == ST_ERR_SINGULAR:
                raise np.linalg.LinAlgError("Singular matrix")                       # :83
            if st in (ST_ERR_MASK, ST_ERR_EMPTY):
                raise ValueError("frame %d: %s" % (self.frame_count, "no features or no triangles" if st == ST_ERR_EMPTY else
                                                   "a triangle names a vertex outside the frame"))
            n_sel = int(res["n_selected"][f])
            if st == ST_RS_FEW and n_sel >= MIN_POINTS:
                raise ValueError("frame %d: no sample of the RANSAC had an inlier" % self.frame_count)
            if st == ST_RS_FEW:
                if self._prev is None:                                               # :167 indexes the 1-D norm_prev of :45 with two indices
                    raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")
                prev, inl = self._prev
                # :163-165 and the surviving `inliers`: everything repeats, but :202-203 see the new prior
                h_t = float(np.mean(inl[:, 2] * math.sin(est) + inl[:, 1] * math.cos(est)))
                r = prev._replace(height_t_mean=h_t, n_selected=n_sel, carried=True)
            else:
                r = FrameResult(float(res["ransac_height"][f]), float(res["refined_mean"][f]), float(res["refined_std"][f]),
                                float(res["height_t_mean"][f]), float(res["refined_pitch"][f]), int(res["n_inliers"][f]), n_sel, False)
                inl = back_project(points3d_list[f], self.focus, self.cx, self.cy)[res["mask"][f]]
            self._prev = (r, inl)
            self.frame_count += 1
            for k in RESULT_FIELDS:
                self.results[k].append(getattr(r, k))
            out.append(r)
        return out

    def process(self, points3d, estimated_pitch):
        return self.process_batch([points3d], [estimated_pitch])[0]

    # ---- the device-resident path (resident=True) --------------------------------------------------------------
    def _resident_start(self, call, a, b, k):
        """Chunk ``k`` = frames ``a:b`` of the call: ONE upload, then the triangulation, the kernel and the tail queued on the
        estimator's stream, and the download of the chunk's small records behind them.  Nothing is waited for."""
        ctx, H, F = self.ctx, self.max_iterations, b - a
        extra, arrays = [("prior", (F, 4), np.float64)], {"prior": call["priors"][a:b]}
        if call["triples"] is not None:
            tr = np.full((F, H, 3), -1, dtype=np.int32)                             # (-1: outside every list, the sample is spent)
            for f, t in enumerate(call["triples"][a:b]):
                if t is not None and len(t):
                    t = np.asarray(t, dtype=np.int32).reshape(-1, 3)[:H]
                    tr[f, :len(t)] = t
            extra.append(("triples", (F, H, 3), np.int32))
            arrays["triples"] = tr
        st = resident_rows_stage(ctx, call["pts"][a:b], extra, arrays)
        st.update(k=k, a=a, b=b, side=[st["din"], st["tri"], st["dt"]])             # (side: the blocks stream.free_blocks releases)
        call["inflight"].append(st)
        try:
            din, total, max_feat = st["din"], st["total"], int(st["cnt"].max())
            out = ctx.block([("ransac_height", F, np.float64), ("model", (F, 4), np.float64), ("best_ic", F, np.int32), ("used", F, np.int32),
                             ("n_selected", F, np.int32), ("n_inliers", F, np.int32), ("refined_normal", (F, 3), np.float64),
                             ("refined_pitch", F, np.float64), ("refined_mean", F, np.float64), ("refined_std", F, np.float64),
                             ("height_t_mean", F, np.float64), ("status", F, np.int32), ("mask", total, np.uint8)])
            st["out"] = out
            small = st["small"] = ctx.block([("frames", F, TAIL_FRAME), ("error", 1, np.int64)])
            st["side"].append(small)
            out.zero()
            hb = st["header"] = _lib.Batch()
            hb.n_frames, hb.feat_off, hb.feat_cnt = F, din["feat_off"].ptr, din["feat_cnt"].ptr
            hb.x, hb.v, hb.z = din["u"].ptr, din["v"].ptr, din["z"].ptr
            hb.tri1_off, hb.tri1, hb.tri1_cnt = din["tri_off"].ptr, st["tri"]["tri"].ptr, st["dt"]["tri_cnt"].ptr
            hb.max_feat, hb.total_feat = max_feat, total
            st["params"] = _lib.HeightPitchParams(self.focus, self.cx, self.cy, MIN_POINTS, H, self.threshold, GOAL_FRACTION, self.inlier_threshold,
                                                  self.seed, int(call["frame_base"] + a))
            st["outputs"] = _lib.HeightPitchOutputs(*[(out[n].ptr if n in out else None) for n, _ in _lib.HeightPitchOutputs._fields_])
            self._resident_kernel(st)
            while len(call["chain"]) < k + 2:                                            # chunk k: chain[k] -> chain[k + 1]
                call["chain"].append(ctx.empty(len(call["carry0"]), np.uint8))
            self._resident_tail(call, st, F)
            for blk in (din, st["tri"], out):
                blk.mark(True)
        except BaseException:
            call["inflight"].remove(st)
            stream.free_blocks(st)
            raise
        return st

    def _resident_kernel(self, st):
        ctx, din = self.ctx, st["din"]
        _lib.check(ctx.lib.mvosr_height_pitch_batch(ctx.handle, C.byref(st["header"]), C.byref(st["params"]), din["prior"].ptr,
                                                    din["triples"].ptr if "triples" in din else None, C.byref(st["outputs"])),
                   "mvosr_height_pitch_batch")

    def _resident_tail(self, call, st, n_frames, download=True):
        """``mvosr_height_pitch_tail_batch`` over the chunk's first ``n_frames`` frames, then (``download``) the chunk's small records on
        their way to page-locked memory — through the pipeline's side download (a copy kernel) where the knob allows it, as the rescale path."""
        ctx, small = self.ctx, st["small"]
        hb = _lib.Batch.from_buffer_copy(st["header"])
        hb.n_frames = int(n_frames)
        _lib.check(ctx.lib.mvosr_height_pitch_tail_batch(ctx.handle, C.byref(hb), C.byref(st["params"]), st["din"]["prior"].ptr,
                                                         C.byref(st["outputs"]), call["chain"][st["k"]].ptr, call["chain"][st["k"] + 1].ptr,
                                                         call["cap"], small["frames"].ptr, small["error"].ptr),
                   "mvosr_height_pitch_tail_batch")
        for blk in (st["dt"], small) if download else ():
            blk.mark(False)
            if self.GPU_SIDE_DOWNLOADS:
                blk.mark_done()
            else:
                blk.prefetch()
            blk.mark(True)

    def _resident_redo(self, call, st, declined):
        """The frames of the chunk the device triangulation declined: SciPy's rows in canonical form into the frames' own slots of
        the chunk's row slab, ``tri_cnt`` patched, the kernel run again over the chunk, and the tails of this chunk and of every chunk
        queued behind it (their carry-in changed).  A SciPy exception: -> (its frame, the exception), the tail run over the frames
        before it only."""
        for blk in (st["din"], st["tri"], st["out"]):
            blk.mark(False)
        stop = patch_declined_rows(self.ctx, st, [call["pts"][st["a"] + f] for f in declined], declined, self.delaunay_workers)
        self._resident_kernel(st)
        n = st["b"] - st["a"] if stop is None else stop[0]
        if n > 0:
            self._resident_tail(call, st, n)
        if stop is None:
            for later in call["inflight"]:
                if later["k"] > st["k"]:
                    self._resident_tail(call, later, later["b"] - later["a"])
        for blk in (st["din"], st["tri"], st["out"]):
            blk.mark(True)
        return stop

    def _resident_collect(self, call, st):
        """Wait for the chunk's records, send its declined frames through the host, apply the records to the object's state in
        sequence order, and raise where the host loop raises."""
        cnt, F = st["cnt"], st["b"] - st["a"]
        dt_status = st["dt"]["dt_status"].download()
        declined = [f for f in range(F) if dt_status[f] != 0 and cnt[f] >= 3]
        self.declined_total += len(declined) + int(np.count_nonzero(cnt < 3))
        stop = self._resident_redo(call, st, declined) if declined else None
        n = F if stop is None else stop[0]
        frames = st["small"]["frames"].download()[:n] if n else np.zeros(0, dtype=TAIL_FRAME)
        err = int(st["small"]["error"].download()[0]) if n else -1
        kind, bad = (err >> 32, err & 0xffffffff) if err >= 0 else (0, n)
        call["records"].append(frames[:bad])
        call["dt_status"].append(dt_status)
        call["errors"].append(err)
        out = call["out"]
        for f in range(bad):
            r = frames[f]
            res = FrameResult(float(r["ransac_height"]), float(r["refined_mean"]), float(r["refined_std"]), float(r["height_t_mean"]),
                              float(r["refined_pitch"]), int(r["n_inliers"]), int(r["n_selected"]), bool(r["carried"]))
            if not res.carried:
                call["last_fit"] = st["a"] + f
            self.frame_count += 1
            for k in RESULT_FIELDS:
                self.results[k].append(getattr(res, k))
            out.append(res)
        if bad:
            call["carry_at"] = st["k"] + 1
        call["inflight"].remove(st)
        stream.free_blocks(st)
        if kind == _lib.HPT_ERR_SINGULAR:
            raise np.linalg.LinAlgError("Singular matrix")                           # :83
        if kind in (_lib.HPT_ERR_MASK, _lib.HPT_ERR_EMPTY):
            raise ValueError("frame %d: %s" % (self.frame_count, "no features or no triangles" if kind == _lib.HPT_ERR_EMPTY else
                                               "a triangle names a vertex outside the frame"))
        if kind == _lib.HPT_ERR_NO_MODEL:
            raise ValueError("frame %d: no sample of the RANSAC had an inlier" % self.frame_count)
        if kind == _lib.HPT_ERR_NO_PREVIOUS:                                         # :167 indexes the 1-D norm_prev of :45 with two indices
            raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")
        if kind:
            raise RuntimeError("frame %d: the tail stopped with error %d" % (self.frame_count, kind))
        if stop is not None:
            raise stop[1]
        return n

    def _resident_call(self, points3d_list, ests, triples):
        """A call's state: its frames as float64 arrays, the priors, the carry-in record from the object's ``_prev`` — after the
        refusals, which come before anything of the call runs, with the staged path's message."""
        ctx, H = self.ctx, self.max_iterations
        pts = [np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 3)) for p in points3d_list]
        F = len(pts)
        max_feat = max(len(p) for p in pts)
        need = int(ctx.lib.mvosr_height_pitch_lds_bytes(max_feat, H))
        if need > ctx.lds_per_block:
            raise ValueError("a frame of %d features needs %d bytes of LDS, the device has %d" % (max_feat, need, ctx.lds_per_block))
        if max_feat > packing.delaunay_gpu_max_points():
            raise ValueError("a frame of %d features is beyond the device triangulation's %d" % (max_feat, packing.delaunay_gpu_max_points()))
        prev, inl = self._prev if self._prev is not None else (None, None)
        cap = (max(max_feat, 0 if inl is None else len(inl), 2) + 1) & ~1
        return {"pts": pts, "priors": np.array([frame_prior(e) for e in ests], dtype=np.float64).reshape(F, 4), "triples": triples,
                "frame_base": self.frame_count, "cap": cap, "carry0": carry_record(cap, prev, inl), "chain": [], "inflight": [],
                "records": [], "dt_status": [], "errors": [], "out": [], "last_fit": None, "carry_at": 0}

    def _process_resident(self, points3d_list, ests, triples):
        """``process_batch`` with the call's frames device-resident: chunks of the call through ``stream.run``, per chunk ONE upload,
        ``mvosr_delaunay_batch`` -> ``mvosr_height_pitch_batch`` -> ``mvosr_height_pitch_tail_batch`` on the estimator's stream, and
        a few dozen bytes per frame back.  The object's host state is what the staged path leaves, after an exception too."""
        if not len(points3d_list):
            return []
        call = self._resident_call(points3d_list, ests, triples)
        ctx, cap, F = self.ctx, call["cap"], len(points3d_list)
        inl = None if self._prev is None else self._prev[1]
        step = stream.chunk_size(F, self.GPU_CHUNK, self.GPU_MIN_CHUNK, self.GPU_CHUNK_POINTS, [len(p) for p in call["pts"][:64]])[0]
        try:
            call["chain"].append(ctx.to_device(call["carry0"]))
            stream.run(stream.fixed_plan(F, step), lambda a, b, tables, k: self._resident_start(call, a, b, k),
                       lambda st, a, b, last: self._resident_collect(call, st), self.GPU_PIPELINE,
                       lambda st: stream.free_blocks(st), [], lambda: None)
        finally:
            try:
                if call["out"]:                                                      # the carry: one frame's inliers
                    if call["last_fit"] is not None:
                        index = carry_fields(call["chain"][call["carry_at"]].download(), cap)[3]
                        inl = back_project(points3d_list[call["last_fit"]], self.focus, self.cx, self.cy)[index]
                    self._prev = (call["out"][-1], inl)
            finally:
                for buf in call["chain"]:
                    buf.free()
                self.last = {"records": np.concatenate(call["records"]) if call["records"] else np.zeros(0, dtype=TAIL_FRAME),
                             "dt_status": call["dt_status"], "errors": call["errors"]}
        return call["out"]

    def run_sequence(self, frames, motion_ts):
        """The script's run: ``frames[i]`` is dump ``i + 1`` (:50, :60) and its prior ``get_pitch(motion_ts[0:i + 2])`` (:62).
        Returns the six arrays in RESULT_FILES' order."""
        self.process_batch(frames, estimated_pitches(motion_ts, 1, len(frames)))
        return self.result_arrays()

    def result_arrays(self):
        return tuple(np.array(self.results[k]) for k in RESULT_FIELDS)

    def write_results(self, directory):
        """The six files under the script's names, as its ``np.savetxt`` calls write them (:228-244)."""
        for name, arr in zip(RESULT_FILES, self.result_arrays()):
            np.savetxt(os.path.join(directory, name), arr)


# ---- the evaluation runs ---------------------------------------------------------------------------------------------------
EVAL_MODELS = {"plane": _lib.HP_MODEL_PLANE, "line": _lib.HP_MODEL_LINE}
EVAL_DIRS = {"plane": "eval_ransac", "line": "eval_ransac_line"}                     # _eval.py:250, _eval_line.py:251
# the scripts' six files per case (_eval.py:250-265): the first name ends in '_', the others run straight into input_id, and
# only the first lacks the doubled extension — for both models ("plane" in the line script's name too)
EVAL_FILES = (("result_heights_plane_ransac_", ".txt"), ("refined_camera_height_means", ".txt.txt"), ("refined_camera_height_stds", ".txt.txt"),
              ("refined_camera_height_t_means", ".txt.txt"), ("refined_pitch", ".txt.txt"), ("inlier_numbers", ".txt.txt"))
ST_HP_REFINE_DEGENERATE = _lib.ST_HP_REFINE_DEGENERATE
MAX_EVAL_ITERATIONS = 4096


def eval_file_names(model, input_id, input_date, iterations, cases=10):
    """The sixty relative paths the scripts write, case-major, in RESULT_FIELDS' order within a case."""
    return [os.path.join(EVAL_DIRS[model], "%s%s_%s_%d_%d%s" % (stem, input_id, input_date, iterations, c, ext))
            for c in range(cases) for stem, ext in EVAL_FILES]


def _nonempty_runs(frames, batch):
    """Contiguous runs of non-empty dumps, at most ``batch`` frames each: the sample sequence's frame counter is the dump's index,
    so a split run draws what the whole run draws."""
    runs = []
    for i in range(len(frames)):
        if not np.asarray(frames[i]).size:
            continue
        if runs and runs[-1][-1] == i - 1 and len(runs[-1]) < int(batch):
            runs[-1].append(i)
        else:
            runs.append([i])
    return runs


def _eval_frame_rules(i, est, st, n_sel, value, prev, budget=None):
    """The scripts' cross-frame rules for frame ``i`` of ONE run (one budget): ``st`` (cases,) the launch's statuses, ``n_sel`` the
    list's length, ``value(name)`` -> (cases,) the launch's output, ``prev`` the last fitted frame's dict (None: none yet) ->
    (the frame's dict: the six values, sum_y, sum_z, degenerate — per case, carried).  Raises what the scripts raise."""
    if np.any(st == ST_ERR_SINGULAR):
        raise np.linalg.LinAlgError("Singular matrix")                               # :101
    if np.any((st == ST_ERR_MASK) | (st == ST_ERR_EMPTY)):
        raise ValueError("frame %d: %s" % (i, "no features or no triangles" if np.any(st == ST_ERR_EMPTY) else
                                           "a triangle names a vertex outside the frame"))
    if np.any(st == ST_RS_FEW) and n_sel >= MIN_POINTS:
        raise ValueError("frame %d: no sample of the RANSAC had an inlier" % i + ("" if budget is None else " at budget %d" % budget))
    if n_sel < MIN_POINTS:
        if prev is None:                                                             # :188 indexes the 1-D norm_prev of :55 with two indices
            raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")
        cur = dict(prev)
        # :184-186 and the surviving `inliers`: everything repeats, but :223-224 see the new prior
        cur["height_t_mean"] = np.where(prev["degenerate"], np.nan,
                                        (prev["sum_z"] * math.sin(est) + prev["sum_y"] * math.cos(est)) / prev["n_inliers"])
        return cur, True
    cur = {k2: np.array(value(k2), dtype=np.float64) for k2 in RESULT_FIELDS + ("sum_y", "sum_z")}
    cur["degenerate"] = (st & ST_HP_REFINE_DEGENERATE) != 0
    return cur, False


def _pack_samples(samples, F, Cn, H):
    """Recorded samples of ``F`` frames as the (F, Cn, H, 3) array both evaluation launches upload."""
    sm = np.full((F, Cn, H, 3), -1, dtype=np.int32)                                 # (-1: outside every list, the sample is spent)
    for f, t in enumerate(samples):
        if t is None:
            continue
        t = np.asarray(t, dtype=np.int32)
        if t.ndim != 3 or t.shape[0] != Cn or t.shape[2] not in (2, 3):
            raise ValueError("samples[%d] must be shaped (cases, h, 2 or 3)" % f)
        h = min(H, t.shape[1])
        sm[f, :, :h, :t.shape[2]] = t[:, :h]
    return sm


def _eval_launch(ev, H, budgets, points3d_list, priors, samples, tris, frame_base, stage, max_feat, timing, cases_per_group):
    """The launch of both evaluation objects: ``budgets`` None — ``mvosr_height_pitch_eval_batch`` with ``H`` hypotheses, (F, C) per
    quantity; a tuple — ``mvosr_height_pitch_eval_budgets_batch``, ``H`` its last, (F, C, B) per quantity and ``best``."""
    ctx, lib = ev.ctx, ev.ctx.lib
    pts = [np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 3)) for p in points3d_list]
    F, Cn = len(pts), ev.cases
    if F == 0:
        return None
    rows = [np.ascontiguousarray(np.asarray(t, dtype=np.int32).reshape(-1, 3)) for t in tris] if tris is not None \
        else _delaunay_rows(ctx, [np.ascontiguousarray(p[:, 0:2]) for p in pts], ev.triangulation, ev.delaunay_workers)
    cnt = np.array([len(p) for p in pts], dtype=np.int32)
    max_feat = int(cnt.max()) if max_feat is None else int(max_feat)
    need = int(lib.mvosr_height_pitch_eval_lds_bytes(max_feat, H, EVAL_MODELS[ev.model])) if budgets is None else \
        int(lib.mvosr_height_pitch_eval_budgets_lds_bytes(max_feat, H, len(budgets), EVAL_MODELS[ev.model]))
    if need > ctx.lds_per_block:
        raise ValueError("a frame of %d features needs %d bytes of LDS, the device has %d" % (max_feat, need, ctx.lds_per_block))
    spec_in, arrays, off, toff, planes, T = _pack_frames(pts, rows, priors)
    if samples is not None:
        spec_in.append(("samples", (F, Cn, H, 3), np.int32))
        arrays["samples"] = _pack_samples(samples, F, Cn, H)
    FC = (F, Cn) if budgets is None else (F, Cn, len(budgets))
    spec_out = [("ransac_height", FC, np.float64), ("model", FC + (4,), np.float64), ("best_ic", FC, np.int32), ("used", FC, np.int32),
                ("n_selected", F, np.int32), ("n_inliers", FC, np.int32), ("refined_normal", FC + (3,), np.float64),
                ("refined_pitch", FC, np.float64), ("refined_mean", FC, np.float64), ("refined_std", FC, np.float64),
                ("height_t_mean", FC, np.float64), ("sum_y", FC, np.float64), ("sum_z", FC, np.float64), ("status", FC, np.int32)]
    if budgets is not None:
        spec_out.append(("best", FC, np.int32))
    if stage:
        spec_out += ([("list_mask", (Cn, 3 * T), np.uint8)] if budgets is None else []) + \
            [("point_list", 3 * T, np.int32), ("hyp_counts", (F, Cn, H), np.int32)]
    din, dout = ctx.block(spec_in), ctx.block(spec_out)
    try:
        din.upload(arrays)
        dout.zero()
        b = _batch_header(din, F, max_feat, planes.shape[1])
        G = ev.cases_per_group if cases_per_group is None else int(cases_per_group)
        p = _lib.HeightPitchEvalParams(ev.focus, ev.cx, ev.cy, MIN_POINTS, H, ev.threshold, GOAL_FRACTION, ev.inlier_threshold,
                                       ev.seed, int(frame_base), EVAL_MODELS[ev.model], Cn, G)
        o = _lib.HeightPitchEvalOutputs() if budgets is None else _lib.HeightPitchEvalBudgetsOutputs()
        for k, tp in o._fields_:
            if k == "list_stride":
                o.list_stride = 3 * T
            elif k in dout:
                setattr(o, k, dout[k].ptr)
        sp = din["samples"].ptr if samples is not None else None
        if budgets is None:
            def call():
                _lib.check(lib.mvosr_height_pitch_eval_batch(ctx.handle, C.byref(b), C.byref(p), din["prior"].ptr, sp, C.byref(o)),
                           "mvosr_height_pitch_eval_batch")
        else:
            bud = (C.c_int32 * len(budgets))(*budgets)
            def call():
                _lib.check(lib.mvosr_height_pitch_eval_budgets_batch(ctx.handle, C.byref(b), C.byref(p), bud, len(budgets), din["prior"].ptr,
                                                                     sp, C.byref(o)), "mvosr_height_pitch_eval_budgets_batch")
        call()
        kernel_ms = None
        if timing > 0:
            ev2 = ctx.event(), ctx.event()
            ctx.record(ev2[0])
            for _ in range(int(timing)):
                call()
            ctx.record(ev2[1])
            kernel_ms = ctx.elapsed_ms(*ev2) / int(timing)
            for e in ev2:
                lib.mvosr_event_destroy(ctx.handle, e)
        res = {k: dout[k].download() for k, _, _ in spec_out}
        if kernel_ms is not None:
            res["kernel_ms"] = kernel_ms
    finally:
        din.free()
        dout.free()
    if stage:
        nsel = [max(int(m), 0) for m in res["n_selected"]]
        if budgets is None:
            res["list_mask"] = [res["list_mask"][:, 3 * toff[f]:3 * toff[f] + nsel[f]].astype(bool) for f in range(F)]
        res["point_list"] = [res["point_list"][3 * toff[f]:3 * toff[f] + nsel[f]] for f in range(F)]
    res["rows"] = rows
    return res


# ---- the evaluation runs on the device-resident path (resident=True) ------------------------------------------
EVAL_CARRY_HEADER = np.dtype([(k, "<i4") for k in ("has_prev", "halted", "n_cases", "n_budgets")])   # mvosr_height_pitch_eval_carry
EVAL_CARRY_VALUES = RESULT_FIELDS + ("sum_y", "sum_z")


def eval_carry_bytes(n_cases, n_budgets):
    """``mvosr_height_pitch_eval_carry_bytes``: the header, eight double[E], uint8[E], rounded up to 16."""
    E = int(n_cases) * int(n_budgets)
    return -(-(EVAL_CARRY_HEADER.itemsize + 65 * E) // 16) * 16


def eval_carry_record(n_cases, n_budgets, prev=None, halted=False):
    """An evaluation carry record as bytes (mvosr_height_pitch_eval_carry and its arrays).  ``prev``: None — the empty record —, or
    a dict of (n_cases, n_budgets) arrays under EVAL_CARRY_VALUES' names and ``degenerate``: the state after the last frame."""
    Cn, B = int(n_cases), int(n_budgets)
    E, y0 = Cn * B, EVAL_CARRY_HEADER.itemsize
    rec = np.zeros(eval_carry_bytes(Cn, B), dtype=np.uint8)
    h = rec[:y0].view(EVAL_CARRY_HEADER)
    h["has_prev"], h["halted"], h["n_cases"], h["n_budgets"] = int(prev is not None), int(bool(halted)), Cn, B
    if prev is not None:
        val = rec[y0:y0 + 64 * E].view(np.float64).reshape(8, E)
        for k, name in enumerate(EVAL_CARRY_VALUES):
            val[k] = np.asarray(prev[name], dtype=np.float64).reshape(E)
        rec[y0 + 64 * E:y0 + 65 * E] = np.asarray(prev["degenerate"]).reshape(E) != 0
    return rec


def eval_carry_fields(rec):
    """(header (an EVAL_CARRY_HEADER scalar), dict name -> (n_cases, n_budgets) array) of an evaluation carry record's bytes."""
    rec, y0 = np.asarray(rec, dtype=np.uint8), EVAL_CARRY_HEADER.itemsize
    h = rec[:y0].view(EVAL_CARRY_HEADER)[0]
    Cn, B = int(h["n_cases"]), int(h["n_budgets"])
    E = Cn * B
    val = rec[y0:y0 + 64 * E].view(np.float64).reshape(8, Cn, B)
    out = {name: val[k].copy() for k, name in enumerate(EVAL_CARRY_VALUES)}
    out["degenerate"] = rec[y0 + 64 * E:y0 + 65 * E].reshape(Cn, B) != 0
    return h, out


def eval_tail_error(err):
    """The tail's error word -> (kind, budget index, frame); kind 0: none."""
    err = int(err)
    return (0, 0, -1) if err < 0 else ((err >> 32) & 0xff, (err >> 40) & 0xff, err & 0xffffffff)


def _eval_resident_refusals(ev, H, budgets, frames, runs):
    """What is refused before anything of a resident run is queued, run by run in sequence order, with the staged launch's message."""
    ctx, lib = ev.ctx, ev.ctx.lib
    for idx in runs:
        max_feat = max(int(np.asarray(frames[i]).size) // 3 for i in idx)
        need = int(lib.mvosr_height_pitch_eval_lds_bytes(max_feat, H, EVAL_MODELS[ev.model])) if budgets is None else \
            int(lib.mvosr_height_pitch_eval_budgets_lds_bytes(max_feat, H, len(budgets), EVAL_MODELS[ev.model]))
        if need > ctx.lds_per_block:
            raise ValueError("a frame of %d features needs %d bytes of LDS, the device has %d" % (max_feat, need, ctx.lds_per_block))
        if max_feat > packing.delaunay_gpu_max_points():
            raise ValueError("a frame of %d features is beyond the device triangulation's %d" % (max_feat, packing.delaunay_gpu_max_points()))


def _eval_resident_start(ev, call, a, b, k):
    """Chunk ``k`` = dumps ``a:b`` (one run of non-empty dumps): ONE upload, then the triangulation, the evaluation launch and the
    tail queued on the context's stream, and the download of the chunk's results behind them.  Nothing is waited for."""
    ctx, Cn, H, budgets, F = ev.ctx, ev.cases, call["H"], call["budgets"], b - a
    B = call["B"]
    extra, arrays = [("prior", (F, 4), np.float64)], {"prior": call["priors"][a:b]}
    if call["samples"] is not None:
        extra.append(("samples", (F, Cn, H, 3), np.int32))
        arrays["samples"] = _pack_samples(call["samples"][a:b], F, Cn, H)
    st = resident_rows_stage(ctx, call["pts"][a:b], extra, arrays)
    st.update(k=k, a=a, b=b, side=[st["din"], st["tri"], st["dt"]])                 # (side: the blocks stream.free_blocks releases)
    call["inflight"].append(st)
    try:
        din, total, max_feat = st["din"], st["total"], int(st["cnt"].max())
        FC = (F, Cn) if budgets is None else (F, Cn, B)
        out = st["out"] = ctx.block([("ransac_height", FC, np.float64), ("model", FC + (4,), np.float64), ("best_ic", FC, np.int32), ("used", FC, np.int32),
                                     ("n_selected", F, np.int32), ("n_inliers", FC, np.int32), ("refined_normal", FC + (3,), np.float64),
                                     ("refined_pitch", FC, np.float64), ("refined_mean", FC, np.float64), ("refined_std", FC, np.float64),
                                     ("height_t_mean", FC, np.float64), ("sum_y", FC, np.float64), ("sum_z", FC, np.float64), ("status", FC, np.int32)] +
                                    ([("best", FC, np.int32)] if budgets is not None else []))
        BCF = (B, Cn, F)
        small = st["small"] = ctx.block([(n, BCF, np.float64) for n in RESULT_FIELDS] + [("degenerate", BCF, np.uint8)] +
                                        ([("used", BCF, np.int32), ("best", BCF, np.int32)] if budgets is not None else []) +
                                        [("carried", F, np.uint8), ("frame_class", F, np.int32), ("source", F, np.int32), ("error", 1, np.int64)])
        st["side"].append(small)
        out.zero()
        hb = st["header"] = _lib.Batch()
        hb.n_frames, hb.feat_off, hb.feat_cnt = F, din["feat_off"].ptr, din["feat_cnt"].ptr
        hb.x, hb.v, hb.z = din["u"].ptr, din["v"].ptr, din["z"].ptr
        hb.tri1_off, hb.tri1, hb.tri1_cnt = din["tri_off"].ptr, st["tri"]["tri"].ptr, st["dt"]["tri_cnt"].ptr
        hb.max_feat, hb.total_feat = max_feat, total
        st["params"] = _lib.HeightPitchEvalParams(ev.focus, ev.cx, ev.cy, MIN_POINTS, H, ev.threshold, GOAL_FRACTION, ev.inlier_threshold,
                                                  ev.seed, int(a), EVAL_MODELS[ev.model], Cn, ev.cases_per_group)
        o = st["outputs"] = _lib.HeightPitchEvalOutputs() if budgets is None else _lib.HeightPitchEvalBudgetsOutputs()
        for n, _ in o._fields_:                                                       # (list_mask, point_list, hyp_counts: NULL — run() reads none)
            if n in out:
                setattr(o, n, out[n].ptr)
        ti = st["tail_in"] = _lib.HeightPitchEvalTailInputs()
        for n, _ in ti._fields_:
            setattr(ti, n, out[n].ptr if n in out and (budgets is not None or n != "used") else None)
        to = st["tail_out"] = _lib.HeightPitchEvalTailOutputs()
        for n, _ in to._fields_:
            setattr(to, n, small[n].ptr if n in small else None)
        _eval_resident_kernel(ev, call, st)
        while len(call["chain"]) < k + 2:                                              # chunk k: chain[k] -> chain[k + 1]
            call["chain"].append(ctx.empty(len(call["carry0"]), np.uint8))
        _eval_resident_tail(ev, call, st, F)
        for blk in (din, st["tri"], out):
            blk.mark(True)
    except BaseException:
        call["inflight"].remove(st)
        stream.free_blocks(st)
        raise
    return st


def _eval_resident_kernel(ev, call, st):
    ctx, din = ev.ctx, st["din"]
    sp = din["samples"].ptr if "samples" in din else None
    if call["budgets"] is None:
        _lib.check(ctx.lib.mvosr_height_pitch_eval_batch(ctx.handle, C.byref(st["header"]), C.byref(st["params"]), din["prior"].ptr, sp,
                                                         C.byref(st["outputs"])), "mvosr_height_pitch_eval_batch")
    else:
        _lib.check(ctx.lib.mvosr_height_pitch_eval_budgets_batch(ctx.handle, C.byref(st["header"]), C.byref(st["params"]), call["bud"], call["B"],
                                                                 din["prior"].ptr, sp, C.byref(st["outputs"])),
                   "mvosr_height_pitch_eval_budgets_batch")


def _eval_resident_tail(ev, call, st, n_frames, download=True):
    """``mvosr_height_pitch_eval_tail_batch`` over the chunk's first ``n_frames`` frames, then (``download``) the chunk's result block and
    the triangulation's status words on their way to page-locked memory, as ``HeightPitchEstimator._resident_tail``."""
    ctx, small = ev.ctx, st["small"]
    _lib.check(ctx.lib.mvosr_height_pitch_eval_tail_batch(ctx.handle, int(n_frames), ev.cases, call["B"], MIN_POINTS, C.byref(st["tail_in"]),
                                                          st["din"]["prior"].ptr, call["chain"][st["k"]].ptr, call["chain"][st["k"] + 1].ptr,
                                                          C.byref(st["tail_out"])), "mvosr_height_pitch_eval_tail_batch")
    st["tail_frames"] = int(n_frames)
    for blk in (st["dt"], small) if download else ():
        blk.mark(False)
        if ev.GPU_SIDE_DOWNLOADS:
            blk.mark_done()
        else:
            blk.prefetch()
        blk.mark(True)


def _eval_resident_redo(ev, call, st, declined):
    """``HeightPitchEstimator._resident_redo``'s scheme: SciPy's rows into the declined frames' slots, the evaluation launch again
    over the chunk, then this chunk's tail and the tail of every chunk queued behind it (their carry-in changed)."""
    for blk in (st["din"], st["tri"], st["out"]):
        blk.mark(False)
    stop = patch_declined_rows(ev.ctx, st, [call["pts"][st["a"] + f] for f in declined], declined, ev.delaunay_workers)
    _eval_resident_kernel(ev, call, st)
    n = st["b"] - st["a"] if stop is None else stop[0]
    if n > 0:
        _eval_resident_tail(ev, call, st, n)
    if stop is None:
        for later in call["inflight"]:
            if later["k"] > st["k"]:
                _eval_resident_tail(ev, call, later, later["b"] - later["a"])
    for blk in (st["din"], st["tri"], st["out"]):
        blk.mark(True)
    return stop


def _eval_resident_collect(ev, call, st):
    """Wait for the chunk's results, send its declined frames through the host, copy the final frames into the call's arrays and
    raise where the host loop raises."""
    cnt, F, a, budgets = st["cnt"], st["b"] - st["a"], st["a"], call["budgets"]
    dt_status = st["dt"]["dt_status"].download()
    declined = [f for f in range(F) if dt_status[f] != 0 and cnt[f] >= 3]
    ev.declined_total += len(declined) + int(np.count_nonzero(cnt < 3))
    stop = _eval_resident_redo(ev, call, st, declined) if declined else None
    n = F if stop is None else stop[0]
    small = st["small"]
    err = int(small["error"].download()[0]) if n else -1
    kind, bud, bad = eval_tail_error(err)
    bad = n if not kind else bad
    call["dt_status"].append(dt_status)
    call["errors"].append(err)
    if bad:
        B, Cn = call["B"], ev.cases
        part = lambda name: small[name].download().reshape(-1)[:B * Cn * n].reshape(B, Cn, n)[:, :, :bad]   # (laid out for the n frames the tail ran over)
        for name in RESULT_FIELDS:
            call["out"][name][:, :, a:a + bad] = part(name)
        ev.degenerate.reshape(B, Cn, -1)[:, :, a:a + bad] = part("degenerate") != 0
        ev.carried[a:a + bad] = small["carried"].download()[:bad] != 0
        if budgets is not None:
            ev.used[:, :, a:a + bad], ev.best[:, :, a:a + bad] = part("used"), part("best")
    call["inflight"].remove(st)
    stream.free_blocks(st)
    i = a + bad                                                                      # the dump the host loop raises at
    if kind == _lib.HPT_ERR_SINGULAR:
        raise np.linalg.LinAlgError("Singular matrix")                               # :101
    if kind in (_lib.HPT_ERR_MASK, _lib.HPT_ERR_EMPTY):
        raise ValueError("frame %d: %s" % (i, "no features or no triangles" if kind == _lib.HPT_ERR_EMPTY else
                                           "a triangle names a vertex outside the frame"))
    if kind == _lib.HPT_ERR_NO_MODEL:
        raise ValueError("frame %d: no sample of the RANSAC had an inlier" % i + ("" if budgets is None else " at budget %d" % budgets[bud]))
    if kind == _lib.HPT_ERR_NO_PREVIOUS:                                             # :188 indexes the 1-D norm_prev of :55 with two indices
        raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")
    if kind:
        raise RuntimeError("frame %d: the tail stopped with error %d" % (i, kind))
    if stop is not None:
        raise stop[1]
    return n


def _eval_resident_call(ev, H, budgets, frames, ests, samples):
    """A resident run's state: the frames as float64 arrays, the priors, the empty carry record, and the arrays ``run`` returns —
    the object's ``carried`` / ``degenerate`` (/ ``used`` / ``best``) set up as the staged run sets them up."""
    n, Cn, B = len(frames), ev.cases, 1 if budgets is None else len(budgets)
    ev.carried = np.zeros(n, dtype=bool)
    ev.degenerate = np.zeros((Cn, n) if budgets is None else (B, Cn, n), dtype=bool)
    if budgets is not None:
        ev.used, ev.best = np.zeros((B, Cn, n), dtype=np.int32), np.full((B, Cn, n), -1, dtype=np.int32)
    empty = np.zeros((0, 3), dtype=np.float64)
    return {"pts": [np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 3)) if np.asarray(p).size else empty for p in frames],
            "priors": np.array([frame_prior(e) for e in ests], dtype=np.float64).reshape(n, 4), "samples": samples, "H": H, "B": B,
            "budgets": budgets, "bud": None if budgets is None else (C.c_int32 * B)(*budgets), "carry0": eval_carry_record(Cn, B),
            "chain": [], "inflight": [], "dt_status": [], "errors": [], "out": {k: np.zeros((B, Cn, n), dtype=np.float64) for k in RESULT_FIELDS}}


def _eval_resident_run(ev, H, budgets, frames, motion_ts, samples, batch):
    """``run`` of both evaluation objects with the frames device-resident: the runs of non-empty dumps as chunks through ``stream.run``,
    per chunk ONE upload, ``mvosr_delaunay_batch`` -> the evaluation launch -> ``mvosr_height_pitch_eval_tail_batch`` on the context's
    stream, and the (B, cases, frames) arrays ``run`` returns coming back as they are.  -> dict field -> (B, cases, frames)."""
    ctx, n = ev.ctx, len(frames)
    ests = estimated_pitches(motion_ts, 1, n) if n else np.zeros(0)
    runs = _nonempty_runs(frames, batch)
    _eval_resident_refusals(ev, H, budgets, frames, runs)
    call = _eval_resident_call(ev, H, budgets, frames, ests, samples)
    if not runs:
        return call["out"]
    try:
        call["chain"].append(ctx.to_device(call["carry0"]))
        stream.run(((idx[0], idx[-1] + 1, None) for idx in runs), lambda a, b, tables, k: _eval_resident_start(ev, call, a, b, k),
                   lambda st, a, b, last: _eval_resident_collect(ev, call, st), ev.GPU_PIPELINE,
                   lambda st: stream.free_blocks(st), [], lambda: None)
    finally:
        for buf in call["chain"]:
            buf.free()
        ev.last = {"dt_status": call["dt_status"], "errors": call["errors"]}
    return call["out"]


class RansacEvaluation:
    """``calculate_height_pitch_eval.py`` (model "plane") and ``calculate_height_pitch_eval_line.py`` ("line"): the sequence run
    ``cases`` times with ``iterations`` hypotheses per frame, every case with a sample sequence of its own.  One launch per batch of
    frames covers all cases; the scripts' cross-frame rules are applied per case on the host — or, with ``triangulation="gpu",
    resident=True``, on the device, the frames resident from their upload to the arrays ``run`` returns: the same
    results, ``carried`` and ``degenerate`` byte for byte; ``tris=`` is refused there, and ``last`` holds status and error words only."""


    # the device-resident path (resident=True): off unless asked for, its chunk pipeline's knobs (stream.StreamKnobs;
    # tests and profiles override them per instance) and its count of frames whose rows came from the host (or that have < 3 points)
    resident = False
    declined_total = 0
    GPU_PIPELINE = stream.StreamKnobs.GPU_PIPELINE
    GPU_SIDE_DOWNLOADS = stream.StreamKnobs.GPU_SIDE_DOWNLOADS

    def __init__(self, model, iterations, cases=10, focus=FOCUS, cx=CX, cy=CY, threshold=0.005, inlier_threshold=0.01, seed=None,
                 device=0, triangulation="scipy", cases_per_group=None, delaunay_workers=0, resident=False):
        if model not in EVAL_MODELS:
            raise ValueError("model must be 'plane' or 'line'")
        if triangulation not in ("scipy", "gpu"):
            raise ValueError("triangulation must be 'scipy' or 'gpu'")
        if resident:                                   # opt-in; without it no attribute of the instance is new
            if triangulation != "gpu":
                raise ValueError(RESIDENT_ERROR)
            self.resident, self.declined_total = True, 0
        if not 1 <= int(iterations) <= MAX_EVAL_ITERATIONS:
            raise ValueError("iterations must be in 1..%d" % MAX_EVAL_ITERATIONS)
        if int(cases) < 1:
            raise ValueError("cases must be at least 1")
        self.ctx = _lib.default_context(device)
        self.model, self.iterations, self.cases = model, int(iterations), int(cases)
        self.focus, self.cx, self.cy = float(focus), float(cx), float(cy)
        self.threshold, self.inlier_threshold = float(threshold), float(inlier_threshold)
        self.seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed) & (2 ** 64 - 1)
        self.triangulation, self.delaunay_workers = triangulation, delaunay_workers
        self.cases_per_group = 0 if cases_per_group is None else int(cases_per_group)  # (0: the library's default, one case per workgroup)
        self.results = None                            # field -> (cases, frames) after run()
        self.carried = None                            # (frames,) bool
        self.degenerate = None                         # (cases, frames) bool: the refinement's sample named a vertex twice
        self.last = None

    # ---- one launch
    def launch(self, points3d_list, priors, samples=None, tris=None, frame_base=0, stage=False, max_feat=None, timing=0, cases_per_group=None):
        """``mvosr_height_pitch_eval_batch`` over the frames -> dict of host arrays, (F, C) per quantity (``model`` (F, C, 4),
        ``n_selected`` (F,)).  ``samples``: None (the device draws), or per frame an array of list positions shaped (C, h, 2 or 3),
        h <= iterations (None / shorter: the missing samples are spent).  ``stage``: also ``hyp_counts`` (F, C, H), ``list_mask``
        (per frame (C, n_selected) bool) and ``point_list``."""
        return _eval_launch(self, self.iterations, None, points3d_list, priors, samples, tris, frame_base, stage, max_feat, timing, cases_per_group)

    # ---- the scripts' run
    def run(self, frames, motion_ts, samples=None, tris=None, batch=512):
        """``frames[i]`` is dump ``i + 1`` and its prior ``get_pitch(motion_ts[0:i + 2])`` (_eval.py:70, :80).  Returns a dict of the
        six (cases, frames) arrays under RESULT_FIELDS' names.  An empty dump gives six zeros and leaves what is carried untouched
        (:71-79); a frame with fewer than 12 list points repeats the previous frame's outputs of its case, ``height_t_mean`` under
        the new prior (:184-186, :223); a first fitted frame with too few points raises ``IndexError`` (:188), a singular row
        ``np.linalg.LinAlgError`` (:101).  Where the refinement's sample names a vertex twice, the refined values are NaN
        (``self.degenerate``); the RANSAC height and the inlier number are not affected."""
        if self.resident:
            if tris is not None:
                raise ValueError("resident=True triangulates on the device: tris= belongs to the staged path")
            out = _eval_resident_run(self, self.iterations, None, frames, motion_ts, samples, batch)
            self.results = {k: v[0] for k, v in out.items()}
            return self.results
        n, Cn = len(frames), self.cases
        ests = estimated_pitches(motion_ts, 1, n) if n else np.zeros(0)
        out = {k: np.zeros((Cn, n), dtype=np.float64) for k in RESULT_FIELDS}
        self.carried, self.degenerate = np.zeros(n, dtype=bool), np.zeros((Cn, n), dtype=bool)
        prev = None                                    # per case: the six values, sum_y, sum_z, degenerate — of the last fitted frame
        for idx in _nonempty_runs(frames, batch):
            r = self.launch([frames[i] for i in idx], [frame_prior(ests[i]) for i in idx], None if samples is None else [samples[i] for i in idx],
                            None if tris is None else [tris[i] for i in idx], frame_base=idx[0])
            self.last = r
            for j, i in enumerate(idx):
                prev, self.carried[i] = _eval_frame_rules(i, ests[i], r["status"][j], int(r["n_selected"][j]), lambda k2: r[k2][j], prev)
                for k2 in RESULT_FIELDS:
                    out[k2][:, i] = prev[k2]
                self.degenerate[:, i] = prev["degenerate"]
        self.results = out
        return out

    def spread(self):
        """Per frame the mean and the (population) std over the cases of each of the six quantities — what the runs exist for:
        dict field -> (mean (frames,), std (frames,)).  Refined values of degenerate pairs are left out of their frame's figures."""
        if self.results is None:
            raise RuntimeError("run() first")
        out = {}
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                for k, v in self.results.items():
                    out[k] = (np.nanmean(v, axis=0), np.nanstd(v, axis=0))
        return out

    def write_results(self, directory, input_id, input_date):
        """The scripts' sixty files under the scripts' own names (_eval.py:250-265), in ``directory``/eval_ransac or
        ``directory``/eval_ransac_line (created if missing).  Returns the paths."""
        if self.results is None:
            raise RuntimeError("run() first")
        names = eval_file_names(self.model, input_id, input_date, self.iterations, self.cases)
        os.makedirs(os.path.join(directory, EVAL_DIRS[self.model]), exist_ok=True)
        for c in range(self.cases):
            for k, field in enumerate(RESULT_FIELDS):
                np.savetxt(os.path.join(directory, names[c * len(RESULT_FIELDS) + k]), self.results[field][c])
        return [os.path.join(directory, x) for x in names]



# ---- the evaluation runs at every budget of a list ---------------------------------------------------------------------------
MAX_EVAL_BUDGETS = 16                                                                # kHpeMaxBudgets


def check_budgets(budgets):
    """The iteration budgets of a sweep as a tuple of ints: 1 to 16 of them, strictly ascending, each in 1..4096 — what
    ``mvosr_height_pitch_eval_budgets_batch`` accepts.  Anything else raises ``ValueError``.  Needs no device."""
    try:
        out = tuple(int(b) for b in budgets)
    except TypeError:
        raise ValueError("budgets must be a sequence of integers")
    if any(o != b for o, b in zip(out, budgets)):
        raise ValueError("budgets must be integers")
    if not 1 <= len(out) <= MAX_EVAL_BUDGETS:
        raise ValueError("1 to %d budgets, got %d" % (MAX_EVAL_BUDGETS, len(out)))
    if out[0] < 1 or out[-1] > MAX_EVAL_ITERATIONS:
        raise ValueError("budgets must be in 1..%d" % MAX_EVAL_ITERATIONS)
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("budgets must be strictly ascending")
    return out


class RansacBudgetSweep:
    """What the two evaluation scripts are run for — how many RANSAC iterations the road-plane fit needs: the runs of
    :class:`RansacEvaluation` at every iteration budget of ``budgets`` from ONE launch per batch of frames
    (``mvosr_height_pitch_eval_budgets_batch``).  The sample sequence of a (frame, case) does not depend on the
    budget, so the run at budget b is the first b hypotheses of the run at the largest: row k of every result equals, bit for bit,
    ``RansacEvaluation(model, budgets[k], cases, seed=seed, ...)`` on the same inputs (recorded ``samples`` cut to that budget).
    ``triangulation="gpu", resident=True``: as :class:`RansacEvaluation`'s, ``used`` and ``best`` included."""


    # the device-resident path (resident=True): off unless asked for, its chunk pipeline's knobs (stream.StreamKnobs;
    # tests and profiles override them per instance) and its count of frames whose rows came from the host (or that have < 3 points)
    resident = False
    declined_total = 0
    GPU_PIPELINE = stream.StreamKnobs.GPU_PIPELINE
    GPU_SIDE_DOWNLOADS = stream.StreamKnobs.GPU_SIDE_DOWNLOADS

    def __init__(self, model, budgets, cases=10, focus=FOCUS, cx=CX, cy=CY, threshold=0.005, inlier_threshold=0.01, seed=None,
                 device=0, triangulation="scipy", cases_per_group=None, delaunay_workers=0, resident=False):
        if model not in EVAL_MODELS:
            raise ValueError("model must be 'plane' or 'line'")
        if triangulation not in ("scipy", "gpu"):
            raise ValueError("triangulation must be 'scipy' or 'gpu'")
        if resident:                                   # opt-in; without it no attribute of the instance is new
            if triangulation != "gpu":
                raise ValueError(RESIDENT_ERROR)
            self.resident, self.declined_total = True, 0
        self.budgets = check_budgets(budgets)
        if int(cases) < 1:
            raise ValueError("cases must be at least 1")
        self.ctx = _lib.default_context(device)
        self.model, self.cases = model, int(cases)
        self.focus, self.cx, self.cy = float(focus), float(cx), float(cy)
        self.threshold, self.inlier_threshold = float(threshold), float(inlier_threshold)
        self.seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed) & (2 ** 64 - 1)
        self.triangulation, self.delaunay_workers = triangulation, delaunay_workers
        self.cases_per_group = 0 if cases_per_group is None else int(cases_per_group)
        self.results = None                            # field -> (B, cases, frames) after run()
        self.carried = None                            # (frames,) bool
        self.degenerate = None                         # (B, cases, frames) bool
        self.used = None                               # (B, cases, frames) hypotheses replayed; 0 on empty and carried frames
        self.best = None                               # (B, cases, frames) the best hypothesis' number; -1 on empty and carried frames
        self.last = None

    # ---- one launch
    def launch(self, points3d_list, priors, samples=None, tris=None, frame_base=0, stage=False, max_feat=None, timing=0, cases_per_group=None):
        """``mvosr_height_pitch_eval_budgets_batch`` over the frames -> dict of host arrays, (F, C, B) per quantity of
        :meth:`RansacEvaluation.launch` (``model`` (F, C, B, 4), ``n_selected`` (F,)) and ``best`` (F, C, B).  ``samples``: None (the
        device draws), or per frame list positions shaped (C, h, 2 or 3), h <= the last budget (None / shorter: the missing samples are
        spent).  ``stage``: also ``hyp_counts`` (F, C, last budget) and ``point_list``."""
        return _eval_launch(self, self.budgets[-1], self.budgets, points3d_list, priors, samples, tris, frame_base, stage, max_feat, timing,
                            cases_per_group)

    # ---- the scripts' runs
    def run(self, frames, motion_ts, samples=None, tris=None, batch=512):
        """:meth:`RansacEvaluation.run` at every budget: dict field -> (B, cases, frames).  The scripts' cross-frame rules — the empty
        dump, the carried frame under the new prior, the first frame's ``IndexError``, ``LinAlgError`` — apply per (budget, case).
        Where a single run would raise "no sample of the RANSAC had an inlier", so does this, naming the frame and the smallest
        such budget."""
        if self.resident:
            if tris is not None:
                raise ValueError("resident=True triangulates on the device: tris= belongs to the staged path")
            self.results = _eval_resident_run(self, self.budgets[-1], self.budgets, frames, motion_ts, samples, batch)
            return self.results
        n, Cn, B = len(frames), self.cases, len(self.budgets)
        ests = estimated_pitches(motion_ts, 1, n) if n else np.zeros(0)
        out = {k: np.zeros((B, Cn, n), dtype=np.float64) for k in RESULT_FIELDS}
        self.carried, self.degenerate = np.zeros(n, dtype=bool), np.zeros((B, Cn, n), dtype=bool)
        self.used, self.best = np.zeros((B, Cn, n), dtype=np.int32), np.full((B, Cn, n), -1, dtype=np.int32)
        prev = [None] * B                              # per budget what RansacEvaluation.run carries
        for idx in _nonempty_runs(frames, batch):
            r = self.launch([frames[i] for i in idx], [frame_prior(ests[i]) for i in idx], None if samples is None else [samples[i] for i in idx],
                            None if tris is None else [tris[i] for i in idx], frame_base=idx[0])
            self.last = r
            for j, i in enumerate(idx):
                n_sel = int(r["n_selected"][j])
                for k, budget in enumerate(self.budgets):
                    prev[k], self.carried[i] = _eval_frame_rules(i, ests[i], r["status"][j][:, k], n_sel, lambda k2: r[k2][j][:, k], prev[k], budget)
                    for k2 in RESULT_FIELDS:
                        out[k2][k, :, i] = prev[k][k2]
                    self.degenerate[k, :, i] = prev[k]["degenerate"]
                if not self.carried[i]:
                    self.used[:, :, i], self.best[:, :, i] = r["used"][j].T, r["best"][j].T
        self.results = out
        return out

    def _need_results(self):
        if self.results is None:
            raise RuntimeError("run() first")

    def results_at(self, budget):
        """The run at ``budget`` (one of the list): dict field -> (cases, frames), as :meth:`RansacEvaluation.run` returns it."""
        self._need_results()
        if budget not in self.budgets:
            raise ValueError("budget %r is not in the list %r" % (budget, self.budgets))
        k = self.budgets.index(budget)
        return {f: v[k] for f, v in self.results.items()}

    def spread(self):
        """Per budget and frame the mean and the (population) std over the cases: dict field -> (mean (B, frames), std (B, frames)),
        with :meth:`RansacEvaluation.spread`'s NaN handling (refined values of degenerate pairs are left out)."""
        self._need_results()
        import warnings
        out = {}
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for k, v in self.results.items():
                out[k] = (np.nanmean(v, axis=1), np.nanstd(v, axis=1))
        return out

    def table(self, field="ransac_height"):
        """What the runs are for, a row (dict) per budget: ``budget``; ``mean_std`` and ``max_std``, the mean and the maximum over
        the fitted frames of the std of ``field`` over the cases; ``mean_used``, the mean number of hypotheses replayed, and
        ``stopped_share``, the share of (case, frame) pairs whose goal stop came before the budget — both over the fitted frames.
        A fitted frame is one with a fit of its own at the largest budget: not an empty dump, not a carried frame."""
        self._need_results()
        fitted = np.any(self.used[-1] > 0, axis=0)                                   # (frames,)
        std = self.spread()[field][1][:, fitted]                                     # (B, fitted frames)
        rows = []
        import warnings
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for k, budget in enumerate(self.budgets):
                u = self.used[k][:, fitted]
                rows.append({"budget": budget,
                             "mean_std": float(np.nanmean(std[k])) if std[k].size else float("nan"),
                             "max_std": float(np.nanmax(std[k])) if std[k].size else float("nan"),
                             "mean_used": float(u.mean()) if u.size else float("nan"),
                             "stopped_share": float((u < budget).mean()) if u.size else float("nan")})
        return rows

    def smallest_budget(self, field="ransac_height", within=0.1):
        """The smallest budget whose ``mean_std`` of :meth:`table` lies within ``within`` (relative) of the largest budget's."""
        rows = self.table(field)
        ref = rows[-1]["mean_std"]
        for r in rows:
            if abs(r["mean_std"] - ref) <= float(within) * abs(ref):
                return r["budget"]
        return rows[-1]["budget"]

    def write_results(self, directory, input_id, input_date):
        """The scripts' sixty files PER BUDGET under the scripts' own names — the budget is part of every name (_eval.py:250-265) —
        in ``directory``/eval_ransac or ``directory``/eval_ransac_line (created if missing).  Returns the paths, budget-major."""
        self._need_results()
        os.makedirs(os.path.join(directory, EVAL_DIRS[self.model]), exist_ok=True)
        paths = []
        for b, budget in enumerate(self.budgets):
            names = eval_file_names(self.model, input_id, input_date, budget, self.cases)
            for c in range(self.cases):
                for k, field in enumerate(RESULT_FIELDS):
                    np.savetxt(os.path.join(directory, names[c * len(RESULT_FIELDS) + k]), self.results[field][b][c])
            paths += [os.path.join(directory, x) for x in names]
        return paths
