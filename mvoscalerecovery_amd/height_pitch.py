"""GPU mirror of the per-frame camera-height and road-pitch estimator /root/reference/src/calculate_height_pitch.py
(its ``_eval`` / ``_eval_line`` copies share the frame loop): per frame of ``[u, v, depth]`` features and a pitch prior from
the camera motion, the RANSAC road plane over the triangles the prior admits, its inliers among all points, and from them
the camera height, a refined pitch, and the height under the prior's pitch.

The reference is a Python-2 script over text dumps that writes six result files at its end; here the frame loop's body is
ONE kernel launch for a batch of frames (``mvosr_height_pitch_batch``) and the script's cross-frame state —
a frame with fewer than 12 list points repeats the previous frame's plane and inliers (:163-165) — is kept by
:class:`HeightPitchEstimator`.  The triangulation's rows are built on the host (SciPy) or on the device and visit the
host either way in this version.  The line RANSAC of :146 is printed by the script and never used: it is not computed."""
from __future__ import annotations

import collections
import ctypes as C
import math
import os

import numpy as np

from . import _lib, packing

FOCUS, CX, CY = 718.856, 607.1928, 185.2157        # calculate_height_pitch.py:15-17
PI_SCRIPT = 3.1415926                               # :63, :91
MIN_POINTS = 12                                     # :140
GOAL_FRACTION = 0.8                                 # estimate_road_norm.py:68
ST_RS_FEW, ST_ERR_SINGULAR, ST_ERR_MASK, ST_ERR_EMPTY = 11, 7, 8, 9

# the script's six result files (:228-244), in the order run_sequence returns the arrays
RESULT_FILES = ("result_heights_line_ransac.txt", "refined_camera_height_means.txt", "refined_camera_height_stds.txt",
                "refined_camera_height_t_means.txt", "refined_pitch.txt", "inlier_numbers.txt")
RESULT_FIELDS = ("ransac_height", "refined_mean", "refined_std", "height_t_mean", "refined_pitch", "n_inliers")

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


class HeightPitchEstimator:
    """The script's frame loop as an object: ``process`` / ``process_batch`` take frames in sequence order and keep what the
    script carries from one frame to the next; the six result lists grow as the script's do."""

    def __init__(self, focus=FOCUS, cx=CX, cy=CY, max_iterations=500, threshold=0.005, inlier_threshold=0.01, seed=None, device=0,
                 triangulation="scipy", delaunay_workers=0):
        if triangulation not in ("scipy", "gpu"):
            raise ValueError("triangulation must be 'scipy' or 'gpu'")
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
        todo = [f for f, p in enumerate(pts2d) if len(p) >= 3]
        rows = [np.zeros((0, 3), dtype=np.int32)] * len(pts2d)
        if self.triangulation == "gpu":
            got = packing.delaunay_gpu_or_host(self.ctx, [pts2d[f] for f in todo], self.delaunay_workers, canonical=True)
        else:
            got = packing.delaunay_many([pts2d[f] for f in todo], self.delaunay_workers)
        for f, t in zip(todo, got):
            if isinstance(t, Exception):
                raise t
            rows[f] = np.ascontiguousarray(t, dtype=np.int32)
        return rows

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
        off = np.zeros(F, dtype=np.int64)
        off[1:] = np.cumsum((cnt[:-1].astype(np.int64) + 1) & ~1)                   # even segment starts
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
            b = _lib.Batch()
            b.n_frames, b.feat_off, b.feat_cnt = F, din["feat_off"].ptr, din["feat_cnt"].ptr
            b.x, b.v, b.z = din["u"].ptr, din["v"].ptr, din["z"].ptr
            b.tri1_off, b.tri1 = din["tri1_off"].ptr, din["tri1"].ptr
            b.max_feat, b.total_feat = max_feat, planes.shape[1]
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
