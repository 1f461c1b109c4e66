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
state applied by ``mvosr_height_pitch_tail_batch``, chunks streamed on the shared pipeline by the one resident driver
(``stream.py``, ``hp_resident.py``).
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
from .hp_resident import ResidentCall, _pack_planes, batch_header, frame_error, patch_declined_rows, resident_rows_stage  # noqa: F401

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


def _batch_header(din, F, max_feat, total_feat):
    return batch_header(din, F, max_feat, total_feat, din["tri1_off"].ptr, din["tri1"].ptr)


# ---- what the staged launches and the resident chunks of all three objects share ------------------------------------------------
def _refuse_lds(ctx, max_feat, need):
    if need > ctx.lds_per_block:
        raise ValueError("a frame of %d features needs %d bytes of LDS, the device has %d" % (max_feat, need, ctx.lds_per_block))


def _refuse_beyond_triangulation(max_feat):
    if max_feat > packing.delaunay_gpu_max_points():
        raise ValueError("a frame of %d features is beyond the device triangulation's %d" % (max_feat, packing.delaunay_gpu_max_points()))


def _refuse_tris(tris):
    if tris is not None:
        raise ValueError("resident=True triangulates on the device: tris= belongs to the staged path")


def _float_frame(p):
    return np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 3))


def _staged_frames(obj, points3d_list, tris, max_feat):
    """A staged launch's frames as float64 arrays, their rows (``tris``, or the object's triangulation's) and the ``max_feat`` the
    batch header states -> (pts, rows, max_feat)."""
    pts = [_float_frame(p) for p in points3d_list]
    rows = [np.ascontiguousarray(np.asarray(t, dtype=np.int32).reshape(-1, 3)) for t in tris] if tris is not None \
        else _delaunay_rows(obj.ctx, [np.ascontiguousarray(p[:, 0:2]) for p in pts], obj.triangulation, obj.delaunay_workers)
    return pts, rows, max(len(p) for p in pts) if max_feat is None else int(max_feat)


def _staged_launch(ctx, spec_in, arrays, spec_out, call_of, timing):
    """One staged launch: the inputs uploaded, the outputs zeroed, ``call_of(din, dout)()`` once — and, ``timing`` > 0, that often
    again between two events (``kernel_ms``: one launch's share) —, every output downloaded -> dict of host arrays."""
    din, dout = ctx.block(spec_in), ctx.block(spec_out)
    try:
        din.upload(arrays)
        dout.zero()
        call = call_of(din, dout)
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
                ctx.lib.mvosr_event_destroy(ctx.handle, e)
        res = {k: dout[k].download() for k, _, _ in spec_out}
        if kernel_ms is not None:
            res["kernel_ms"] = kernel_ms
    finally:
        din.free()
        dout.free()
    return res


def _status_kind(st, n_sel):
    """A frame's status words (one, or one per case) and its list's length as the tails' error kind (MVOSR_HPT_ERR_*), in the
    order the host loops ask; 0: none of these."""
    if np.any(st == ST_ERR_SINGULAR):
        return _lib.HPT_ERR_SINGULAR
    if np.any(st == ST_ERR_EMPTY):
        return _lib.HPT_ERR_EMPTY
    if np.any(st == ST_ERR_MASK):
        return _lib.HPT_ERR_MASK
    return _lib.HPT_ERR_NO_MODEL if np.any(st == ST_RS_FEW) and n_sel >= MIN_POINTS else 0


def _pack_triples(triples, F, H):
    """Recorded samples of ``F`` frames as the (F, H, 3) array the estimator's launches upload."""
    tr = np.full((F, H, 3), -1, dtype=np.int32)                                     # (-1: outside every list, the sample is spent)
    for f, t in enumerate(triples):
        if t is not None and len(t):
            t = np.asarray(t, dtype=np.int32).reshape(-1, 3)[:H]
            tr[f, :len(t)] = t
    return tr


def _out_spec(F, total):
    """``mvosr_height_pitch_batch``'s outputs over ``F`` frames whose feature planes are ``total`` long."""
    return [("ransac_height", F, np.float64), ("model", (F, 4), np.float64), ("best_ic", F, np.int32), ("used", F, np.int32),
            ("n_selected", F, np.int32), ("n_inliers", F, np.int32), ("refined_normal", (F, 3), np.float64),
            ("refined_pitch", F, np.float64), ("refined_mean", F, np.float64), ("refined_std", F, np.float64),
            ("height_t_mean", F, np.float64), ("status", F, np.int32), ("mask", total, np.uint8)]


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

    # ---- one launch
    def launch(self, points3d_list, priors, triples=None, tris=None, frame_base=None, stage=False, max_feat=None, timing=0):
        """``mvosr_height_pitch_batch`` over the frames -> dict of per-frame host arrays (``mask`` / ``point_list``: lists).
        ``priors``: (F, 4) as :func:`frame_prior`.  ``triples``: None (the device draws), or per frame an (H, 3) array of list
        positions (None / shorter: the missing samples are spent).  ``stage``: also ``hyp_counts`` and ``point_list``.
        ``max_feat``: what the batch header states (default: the largest frame; a larger frame is refused by the kernel).
        ``timing`` > 0: the launch is repeated that often on the resident batch between two events; ``kernel_ms`` is one launch's share."""
        ctx, lib, F, H = self.ctx, self.ctx.lib, len(points3d_list), self.max_iterations
        if F == 0:
            return None
        pts, rows, max_feat = _staged_frames(self, points3d_list, tris, max_feat)
        _refuse_lds(ctx, max_feat, int(lib.mvosr_height_pitch_lds_bytes(max_feat, H)))
        spec_in, arrays, off, toff, planes, T = _pack_frames(pts, rows, priors)
        if triples is not None:
            spec_in.append(("triples", (F, H, 3), np.int32))
            arrays["triples"] = _pack_triples(triples, F, H)
        spec_out = _out_spec(F, planes.shape[1]) + ([("point_list", 3 * T, np.int32), ("hyp_counts", (F, H), np.int32)] if stage else [])

        def call_of(din, dout):
            b = _batch_header(din, F, max_feat, planes.shape[1])
            p = _lib.HeightPitchParams(self.focus, self.cx, self.cy, MIN_POINTS, H, self.threshold, GOAL_FRACTION, self.inlier_threshold,
                                       self.seed, int(self.frame_count if frame_base is None else frame_base))
            o = _lib.HeightPitchOutputs(*[(dout[k].ptr if k in dout else None) for k, _ in _lib.HeightPitchOutputs._fields_])
            return lambda: _lib.check(lib.mvosr_height_pitch_batch(ctx.handle, C.byref(b), C.byref(p), din["prior"].ptr,
                                                                   din["triples"].ptr if triples is not None else None, C.byref(o)),
                                      "mvosr_height_pitch_batch")
        res = _staged_launch(ctx, spec_in, arrays, spec_out, call_of, timing)
        cnt = arrays["feat_cnt"]
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
            _refuse_tris(tris)
            return self._process_resident(points3d_list, ests, triples)
        res = self.launch(points3d_list, [frame_prior(e) for e in ests], triples=triples, tris=tris)
        self.last = res
        out = []
        for f, est in enumerate(ests):
            st, n_sel = int(res["status"][f]), int(res["n_selected"][f])
            kind = _status_kind(st, n_sel)
            if kind:
                raise frame_error(kind, self.frame_count)
            if st == ST_RS_FEW:
                if self._prev is None:
                    raise frame_error(_lib.HPT_ERR_NO_PREVIOUS, self.frame_count)
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
    def _resident_call(self, points3d_list, ests, triples):
        """A call's state (:class:`_EstimatorCall`) — after the refusals, which come before anything of the call runs, with the
        staged path's message."""
        pts = [_float_frame(p) for p in points3d_list]
        max_feat = max(len(p) for p in pts)
        _refuse_lds(self.ctx, max_feat, int(self.ctx.lib.mvosr_height_pitch_lds_bytes(max_feat, self.max_iterations)))
        _refuse_beyond_triangulation(max_feat)
        return _EstimatorCall(self, pts, max_feat, ests, triples)

    def _process_resident(self, points3d_list, ests, triples):
        """``process_batch`` with the call's frames device-resident: chunks of the call through ``stream.run``, per chunk ONE upload,
        ``mvosr_delaunay_batch`` -> ``mvosr_height_pitch_batch`` -> ``mvosr_height_pitch_tail_batch`` on the estimator's stream, and
        a few dozen bytes per frame back.  The object's host state is what the staged path leaves, after an exception too."""
        if not len(points3d_list):
            return []
        call, F = self._resident_call(points3d_list, ests, triples), len(points3d_list)
        step = stream.chunk_size(F, self.GPU_CHUNK, self.GPU_MIN_CHUNK, self.GPU_CHUNK_POINTS, [len(p) for p in call.pts[:64]])[0]
        call.run(stream.fixed_plan(F, step))
        return call.out

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


class _EstimatorCall(ResidentCall):
    """A ``process_batch`` call of the estimator ``est`` on the resident path: the priors, the carry-in record from the object's
    ``_prev``, and what :class:`ResidentCall` leaves to its user — ``mvosr_height_pitch_batch``, ``mvosr_height_pitch_tail_batch``,
    and the chunks' records as ``FrameResult``s into the object's lists."""

    def __init__(self, est, pts, max_feat, ests, triples):
        prev, inl = est._prev if est._prev is not None else (None, None)
        self.cap = (max(max_feat, 0 if inl is None else len(inl), 2) + 1) & ~1
        super().__init__(est, pts, carry_record(self.cap, prev, inl))
        self.priors = np.array([frame_prior(e) for e in ests], dtype=np.float64).reshape(len(pts), 4)
        self.triples, self.frame_base = triples, est.frame_count
        self.records, self.out = [], []                # per chunk the final records; the call's FrameResults
        self.last_fit, self.carry_at = None, 0         # the last fitted frame, and the chain record behind the last final frame

    def inputs(self, a, b):
        F, H = b - a, self.owner.max_iterations
        extra, arrays = [("prior", (F, 4), np.float64)], {"prior": self.priors[a:b]}
        if self.triples is not None:
            extra.append(("triples", (F, H, 3), np.int32))
            arrays["triples"] = _pack_triples(self.triples[a:b], F, H)
        return extra, arrays

    def block_specs(self, st):
        F = st["b"] - st["a"]
        return _out_spec(F, st["total"]), [("frames", F, TAIL_FRAME), ("error", 1, np.int64)]

    def structs(self, st):
        est, out = self.owner, st["out"]
        st["params"] = _lib.HeightPitchParams(est.focus, est.cx, est.cy, MIN_POINTS, est.max_iterations, est.threshold, GOAL_FRACTION,
                                              est.inlier_threshold, est.seed, int(self.frame_base + st["a"]))
        st["outputs"] = _lib.HeightPitchOutputs(*[(out[n].ptr if n in out else None) for n, _ in _lib.HeightPitchOutputs._fields_])

    def kernel(self, st):
        ctx, din = self.ctx, st["din"]
        _lib.check(ctx.lib.mvosr_height_pitch_batch(ctx.handle, C.byref(st["header"]), C.byref(st["params"]), din["prior"].ptr,
                                                    din["triples"].ptr if "triples" in din else None, C.byref(st["outputs"])),
                   "mvosr_height_pitch_batch")

    def launch_tail(self, st, n_frames):
        ctx, small = self.ctx, st["small"]
        hb = _lib.Batch.from_buffer_copy(st["header"])
        hb.n_frames = n_frames
        _lib.check(ctx.lib.mvosr_height_pitch_tail_batch(ctx.handle, C.byref(hb), C.byref(st["params"]), st["din"]["prior"].ptr,
                                                         C.byref(st["outputs"]), self.chain[st["k"]].ptr, self.chain[st["k"] + 1].ptr,
                                                         self.cap, small["frames"].ptr, small["error"].ptr),
                   "mvosr_height_pitch_tail_batch")

    def decode(self, err, n):
        return (err >> 32, err & 0xffffffff, None) if err >= 0 else (0, n, None)

    def apply(self, st, n, bad):
        est = self.owner
        frames = st["small"]["frames"].download()[:bad] if n else np.zeros(0, dtype=TAIL_FRAME)
        self.records.append(frames)
        for f, r in enumerate(frames):
            res = FrameResult(float(r["ransac_height"]), float(r["refined_mean"]), float(r["refined_std"]), float(r["height_t_mean"]),
                              float(r["refined_pitch"]), int(r["n_inliers"]), int(r["n_selected"]), bool(r["carried"]))
            if not res.carried:
                self.last_fit = st["a"] + f
            est.frame_count += 1
            for k in RESULT_FIELDS:
                est.results[k].append(getattr(res, k))
            self.out.append(res)
        if bad:
            self.carry_at = st["k"] + 1

    def error_frame(self, st, bad):
        return self.owner.frame_count

    def epilogue(self):
        est = self.owner
        try:
            if self.out:                                                             # the carry: one frame's inliers
                inl = None if est._prev is None else est._prev[1]
                if self.last_fit is not None:
                    index = carry_fields(self.chain[self.carry_at].download(), self.cap)[3]
                    inl = back_project(self.pts[self.last_fit], est.focus, est.cx, est.cy)[index]
                est._prev = (self.out[-1], inl)
        finally:
            est.last = {"records": np.concatenate(self.records) if self.records else np.zeros(0, dtype=TAIL_FRAME),
                        "dt_status": self.dt_status, "errors": self.errors}


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
    kind = _status_kind(st, n_sel)
    if kind:
        raise frame_error(kind, i, budget)
    if n_sel < MIN_POINTS:
        if prev is None:
            raise frame_error(_lib.HPT_ERR_NO_PREVIOUS, i)
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


def _eval_lds_bytes(ev, max_feat, H, budgets):
    lib, model = ev.ctx.lib, EVAL_MODELS[ev.model]
    return int(lib.mvosr_height_pitch_eval_lds_bytes(max_feat, H, model)) if budgets is None else \
        int(lib.mvosr_height_pitch_eval_budgets_lds_bytes(max_feat, H, len(budgets), model))


def _eval_out_spec(F, Cn, budgets):
    """The evaluation launch's outputs over ``F`` frames: (F, C) per quantity, or with ``budgets`` (F, C, B) and ``best``."""
    FC = (F, Cn) if budgets is None else (F, Cn, len(budgets))
    return [("ransac_height", FC, np.float64), ("model", FC + (4,), np.float64), ("best_ic", FC, np.int32), ("used", FC, np.int32),
            ("n_selected", F, np.int32), ("n_inliers", FC, np.int32), ("refined_normal", FC + (3,), np.float64),
            ("refined_pitch", FC, np.float64), ("refined_mean", FC, np.float64), ("refined_std", FC, np.float64),
            ("height_t_mean", FC, np.float64), ("sum_y", FC, np.float64), ("sum_z", FC, np.float64), ("status", FC, np.int32)] + \
        ([("best", FC, np.int32)] if budgets is not None else [])


def _eval_structs(ev, H, budgets, frame_base, G, block, list_stride=0):
    """-> (the evaluation launch's parameters, its outputs over ``block`` — what the block does not hold stays NULL)."""
    p = _lib.HeightPitchEvalParams(ev.focus, ev.cx, ev.cy, MIN_POINTS, H, ev.threshold, GOAL_FRACTION, ev.inlier_threshold,
                                   ev.seed, int(frame_base), EVAL_MODELS[ev.model], ev.cases, G)
    o = _lib.HeightPitchEvalOutputs() if budgets is None else _lib.HeightPitchEvalBudgetsOutputs()
    for k, _ in o._fields_:
        if k == "list_stride":
            o.list_stride = list_stride
        elif k in block:
            setattr(o, k, block[k].ptr)
    return p, o


def _eval_kernel(ctx, bud, header, params, din, outputs):
    """The evaluation launch over the uploaded block ``din``: ``bud`` None — ``mvosr_height_pitch_eval_batch``; the budgets as a C
    array — ``mvosr_height_pitch_eval_budgets_batch``."""
    sp = din["samples"].ptr if "samples" in din else None
    if bud is None:
        _lib.check(ctx.lib.mvosr_height_pitch_eval_batch(ctx.handle, C.byref(header), C.byref(params), din["prior"].ptr, sp, C.byref(outputs)),
                   "mvosr_height_pitch_eval_batch")
    else:
        _lib.check(ctx.lib.mvosr_height_pitch_eval_budgets_batch(ctx.handle, C.byref(header), C.byref(params), bud, len(bud), din["prior"].ptr,
                                                                 sp, C.byref(outputs)), "mvosr_height_pitch_eval_budgets_batch")


def _budget_array(budgets):
    return None if budgets is None else (C.c_int32 * len(budgets))(*budgets)


def _eval_launch(ev, H, budgets, points3d_list, priors, samples, tris, frame_base, stage, max_feat, timing, cases_per_group):
    """The launch of both evaluation objects: ``budgets`` None — ``mvosr_height_pitch_eval_batch`` with ``H`` hypotheses, (F, C) per
    quantity; a tuple — ``mvosr_height_pitch_eval_budgets_batch``, ``H`` its last, (F, C, B) per quantity and ``best``."""
    ctx, F, Cn = ev.ctx, len(points3d_list), ev.cases
    if F == 0:
        return None
    pts, rows, max_feat = _staged_frames(ev, points3d_list, tris, max_feat)
    _refuse_lds(ctx, max_feat, _eval_lds_bytes(ev, max_feat, H, budgets))
    spec_in, arrays, off, toff, planes, T = _pack_frames(pts, rows, priors)
    if samples is not None:
        spec_in.append(("samples", (F, Cn, H, 3), np.int32))
        arrays["samples"] = _pack_samples(samples, F, Cn, H)
    spec_out = _eval_out_spec(F, Cn, budgets)
    if stage:
        spec_out += ([("list_mask", (Cn, 3 * T), np.uint8)] if budgets is None else []) + \
            [("point_list", 3 * T, np.int32), ("hyp_counts", (F, Cn, H), np.int32)]

    def call_of(din, dout):
        b, bud = _batch_header(din, F, max_feat, planes.shape[1]), _budget_array(budgets)
        p, o = _eval_structs(ev, H, budgets, frame_base, ev.cases_per_group if cases_per_group is None else int(cases_per_group), dout, 3 * T)
        return lambda: _eval_kernel(ctx, bud, b, p, din, o)
    res = _staged_launch(ctx, spec_in, arrays, spec_out, call_of, timing)
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


class _EvalCall(ResidentCall):
    """A ``run`` of an evaluation object ``ev`` on the resident path: the dumps as float64 arrays, the priors, the empty carry record,
    the (B, cases, frames) arrays ``run`` returns (``out``) — the object's ``carried`` / ``degenerate`` (/ ``used`` / ``best``) set up as
    the staged run sets them up — and what :class:`ResidentCall` leaves to its user: the evaluation launch,
    ``mvosr_height_pitch_eval_tail_batch``, and the chunks' results as slices of those arrays."""

    def __init__(self, ev, H, budgets, frames, ests, samples):
        n, Cn, B = len(frames), ev.cases, 1 if budgets is None else len(budgets)
        ev.carried = np.zeros(n, dtype=bool)
        ev.degenerate = np.zeros((Cn, n) if budgets is None else (B, Cn, n), dtype=bool)
        if budgets is not None:
            ev.used, ev.best = np.zeros((B, Cn, n), dtype=np.int32), np.full((B, Cn, n), -1, dtype=np.int32)
        empty = np.zeros((0, 3), dtype=np.float64)
        super().__init__(ev, [_float_frame(p) if np.asarray(p).size else empty for p in frames], eval_carry_record(Cn, B))
        self.priors = np.array([frame_prior(e) for e in ests], dtype=np.float64).reshape(n, 4)
        self.samples, self.H, self.B, self.budgets, self.bud = samples, H, B, budgets, _budget_array(budgets)
        self.out = {k: np.zeros((B, Cn, n), dtype=np.float64) for k in RESULT_FIELDS}

    def inputs(self, a, b):
        F, Cn = b - a, self.owner.cases
        extra, arrays = [("prior", (F, 4), np.float64)], {"prior": self.priors[a:b]}
        if self.samples is not None:
            extra.append(("samples", (F, Cn, self.H, 3), np.int32))
            arrays["samples"] = _pack_samples(self.samples[a:b], F, Cn, self.H)
        return extra, arrays

    def block_specs(self, st):
        F, BCF = st["b"] - st["a"], (self.B, self.owner.cases, st["b"] - st["a"])
        return (_eval_out_spec(F, self.owner.cases, self.budgets),
                [(n, BCF, np.float64) for n in RESULT_FIELDS] + [("degenerate", BCF, np.uint8)] +
                ([("used", BCF, np.int32), ("best", BCF, np.int32)] if self.budgets is not None else []) +
                [("carried", F, np.uint8), ("frame_class", F, np.int32), ("source", F, np.int32), ("error", 1, np.int64)])

    def structs(self, st):
        ev, out, small = self.owner, st["out"], st["small"]
        # (list_mask, point_list, hyp_counts: NULL — run() reads none)
        st["params"], st["outputs"] = _eval_structs(ev, self.H, self.budgets, st["a"], ev.cases_per_group, out)
        ti = st["tail_in"] = _lib.HeightPitchEvalTailInputs()
        for n, _ in ti._fields_:
            setattr(ti, n, out[n].ptr if n in out and (self.budgets is not None or n != "used") else None)
        to = st["tail_out"] = _lib.HeightPitchEvalTailOutputs()
        for n, _ in to._fields_:
            setattr(to, n, small[n].ptr if n in small else None)

    def kernel(self, st):
        _eval_kernel(self.ctx, self.bud, st["header"], st["params"], st["din"], st["outputs"])

    def launch_tail(self, st, n_frames):
        ctx = self.ctx
        _lib.check(ctx.lib.mvosr_height_pitch_eval_tail_batch(ctx.handle, n_frames, self.owner.cases, self.B, MIN_POINTS, C.byref(st["tail_in"]),
                                                              st["din"]["prior"].ptr, self.chain[st["k"]].ptr, self.chain[st["k"] + 1].ptr,
                                                              C.byref(st["tail_out"])), "mvosr_height_pitch_eval_tail_batch")

    def decode(self, err, n):
        kind, bud, bad = eval_tail_error(err)
        return kind, bad if kind else n, self.budgets[bud] if self.budgets is not None else None

    def apply(self, st, n, bad):
        if not bad:
            return
        ev, small, a, B, Cn = self.owner, st["small"], st["a"], self.B, self.owner.cases
        part = lambda name: small[name].download().reshape(-1)[:B * Cn * n].reshape(B, Cn, n)[:, :, :bad]   # (laid out for the n frames the tail ran over)
        for name in RESULT_FIELDS:
            self.out[name][:, :, a:a + bad] = part(name)
        ev.degenerate.reshape(B, Cn, -1)[:, :, a:a + bad] = part("degenerate") != 0
        ev.carried[a:a + bad] = small["carried"].download()[:bad] != 0
        if self.budgets is not None:
            ev.used[:, :, a:a + bad], ev.best[:, :, a:a + bad] = part("used"), part("best")

    def error_frame(self, st, bad):
        return st["a"] + bad                                                         # the dump the host loop raises at

    def epilogue(self):
        self.owner.last = {"dt_status": self.dt_status, "errors": self.errors}


def _eval_resident_run(ev, H, budgets, frames, motion_ts, samples, batch):
    """``run`` of both evaluation objects with the frames device-resident: the runs of non-empty dumps as chunks through ``stream.run``,
    per chunk ONE upload, ``mvosr_delaunay_batch`` -> the evaluation launch -> ``mvosr_height_pitch_eval_tail_batch`` on the context's
    stream, and the (B, cases, frames) arrays ``run`` returns coming back as they are.  -> dict field -> (B, cases, frames).
    What is refused is refused before anything of the run is queued, run by run in sequence order, with the staged launch's message."""
    n = len(frames)
    ests = estimated_pitches(motion_ts, 1, n) if n else np.zeros(0)
    runs = _nonempty_runs(frames, batch)
    for idx in runs:
        max_feat = max(int(np.asarray(frames[i]).size) // 3 for i in idx)
        _refuse_lds(ev.ctx, max_feat, _eval_lds_bytes(ev, max_feat, H, budgets))
        _refuse_beyond_triangulation(max_feat)
    call = _EvalCall(ev, H, budgets, frames, ests, samples)
    if runs:
        call.run((idx[0], idx[-1] + 1, None) for idx in runs)
    return call.out


class _RansacRuns:
    """What :class:`RansacEvaluation` and :class:`RansacBudgetSweep` share before their first launch."""

    # the device-resident path (resident=True): off unless asked for, its chunk pipeline's knobs (stream.StreamKnobs;
    # tests and profiles override them per instance) and its count of frames whose rows came from the host (or that have < 3 points)
    resident = False
    declined_total = 0
    GPU_PIPELINE = stream.StreamKnobs.GPU_PIPELINE
    GPU_SIDE_DOWNLOADS = stream.StreamKnobs.GPU_SIDE_DOWNLOADS

    def _init(self, hypotheses, model, cases, focus, cx, cy, threshold, inlier_threshold, seed, device, triangulation, cases_per_group,
              delaunay_workers, resident):
        """The constructors' checks and attributes; ``hypotheses()`` is the object's own check of its iterations or budgets, in its
        place among the checks."""
        if model not in EVAL_MODELS:
            raise ValueError("model must be 'plane' or 'line'")
        if triangulation not in ("scipy", "gpu"):
            raise ValueError("triangulation must be 'scipy' or 'gpu'")
        if resident:                                   # opt-in; without it no attribute of the instance is new
            if triangulation != "gpu":
                raise ValueError(RESIDENT_ERROR)
            self.resident, self.declined_total = True, 0
        hypotheses()
        if int(cases) < 1:
            raise ValueError("cases must be at least 1")
        self.ctx = _lib.default_context(device)
        self.model, self.cases = model, int(cases)
        self.focus, self.cx, self.cy = float(focus), float(cx), float(cy)
        self.threshold, self.inlier_threshold = float(threshold), float(inlier_threshold)
        self.seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed) & (2 ** 64 - 1)
        self.triangulation, self.delaunay_workers = triangulation, delaunay_workers
        self.cases_per_group = 0 if cases_per_group is None else int(cases_per_group)  # (0: the library's default, one case per workgroup)
        self.results = None                            # field -> (cases, frames) after run(); the sweep's: (B, cases, frames)
        self.carried = None                            # (frames,) bool
        self.degenerate = None                         # shaped like a result, bool: the refinement's sample named a vertex twice
        self.last = None


class RansacEvaluation(_RansacRuns):
    """``calculate_height_pitch_eval.py`` (model "plane") and ``calculate_height_pitch_eval_line.py`` ("line"): the sequence run
    ``cases`` times with ``iterations`` hypotheses per frame, every case with a sample sequence of its own.  One launch per batch of
    frames covers all cases; the scripts' cross-frame rules are applied per case on the host — or, with ``triangulation="gpu",
    resident=True``, on the device, the frames resident from their upload to the arrays ``run`` returns: the same
    results, ``carried`` and ``degenerate`` byte for byte; ``tris=`` is refused there, and ``last`` holds status and error words only."""

    def __init__(self, model, iterations, cases=10, focus=FOCUS, cx=CX, cy=CY, threshold=0.005, inlier_threshold=0.01, seed=None,
                 device=0, triangulation="scipy", cases_per_group=None, delaunay_workers=0, resident=False):
        def hypotheses():
            if not 1 <= int(iterations) <= MAX_EVAL_ITERATIONS:
                raise ValueError("iterations must be in 1..%d" % MAX_EVAL_ITERATIONS)
            self.iterations = int(iterations)
        self._init(hypotheses, model, cases, focus, cx, cy, threshold, inlier_threshold, seed, device, triangulation, cases_per_group,
                   delaunay_workers, resident)

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
            _refuse_tris(tris)
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


class RansacBudgetSweep(_RansacRuns):
    """What the two evaluation scripts are run for — how many RANSAC iterations the road-plane fit needs: the runs of
    :class:`RansacEvaluation` at every iteration budget of ``budgets`` from ONE launch per batch of frames
    (``mvosr_height_pitch_eval_budgets_batch``).  The sample sequence of a (frame, case) does not depend on the
    budget, so the run at budget b is the first b hypotheses of the run at the largest: row k of every result equals, bit for bit,
    ``RansacEvaluation(model, budgets[k], cases, seed=seed, ...)`` on the same inputs (recorded ``samples`` cut to that budget).
    ``triangulation="gpu", resident=True``: as :class:`RansacEvaluation`'s, ``used`` and ``best`` included."""

    def __init__(self, model, budgets, cases=10, focus=FOCUS, cx=CX, cy=CY, threshold=0.005, inlier_threshold=0.01, seed=None,
                 device=0, triangulation="scipy", cases_per_group=None, delaunay_workers=0, resident=False):
        def hypotheses():
            self.budgets = check_budgets(budgets)
        self._init(hypotheses, model, cases, focus, cx, cy, threshold, inlier_threshold, seed, device, triangulation, cases_per_group,
                   delaunay_workers, resident)
        self.used = None                               # (B, cases, frames) hypotheses replayed; 0 on empty and carried frames
        self.best = None                               # (B, cases, frames) the best hypothesis' number; -1 on empty and carried frames

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
            _refuse_tris(tris)
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
