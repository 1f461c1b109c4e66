"""Downstream scoring of a scale-recovered trajectory: the KITTI-devkit style
segment error of /root/reference/script/evaluate_vo.py:5-96, the scale error statistics of
/root/reference/script/evaluate_scale.py:4-29 and pose <-> motion conversion of
/root/reference/script/transformation.py:6-32.  Host NumPy, like the reference: this is evaluation of
the path's output (a few thousand 3x4 poses), not part of the per-frame hot path.  The repeated runs score ten such paths at
once, which is where these loops cost many times the runs themselves: :class:`Scorer`, :func:`calculate_speed` and
:func:`change_scale` at the end of this file do that on the device (csrc/mvosr_score.hip); the host functions are unchanged and are
their comparators."""
from __future__ import annotations

import numpy as np

LENGTHS = [100, 200, 300, 400, 500, 600, 700, 800]      # evaluate_vo.py:46
STEP = 10                                               # evaluate_vo.py:45


def _mat(line):
    m = np.eye(4)
    m[:3, :] = np.asarray(line, dtype=np.float64).reshape(3, 4)
    return m


def trajectory_distances(poses):
    """evaluate_vo.py:5-13: cumulative path length over the translation columns."""
    t = np.asarray(poses)[:, 3:12:4]
    d = [0]
    for i in range(1, t.shape[0]):
        d.append(d[i - 1] + np.linalg.norm(t[i - 1] - t[i]))
    return d


def calculate_sequence_error(poses_gt, poses_result):
    """evaluate_vo.py:40-79: rows [first_frame, r_err/len, t_err/len, len, speed]."""
    poses_gt, poses_result = np.asarray(poses_gt), np.asarray(poses_result)
    dist = trajectory_distances(poses_gt)
    errors = []
    for first in range(0, poses_gt.shape[0], STEP):
        for length in LENGTHS:
            last = -1
            for i in range(first, len(dist)):                                   # :15-19
                if dist[i] > dist[first] + length:
                    last = i
                    break
            if last == -1:
                continue
            d_gt = np.linalg.inv(_mat(poses_gt[first])) @ _mat(poses_gt[last])            # :65
            d_re = np.linalg.inv(_mat(poses_result[first])) @ _mat(poses_result[last])    # :66
            err = np.linalg.inv(d_re) @ d_gt                                              # :67
            dd = 0.5 * (err[0, 0] + err[1, 1] + err[2, 2] - 1)
            r_err = np.arccos(max(min(dd, 1.0), -1.0))                                    # :21-27
            t_err = np.sqrt(err[0, 3] * err[0, 3] + err[1, 3] * err[1, 3] + err[2, 3] * err[2, 3])   # :29-33
            speed = length / (0.1 * float(last - first + 1))                              # :72-73
            errors.append([first, r_err / length, t_err / length, length, speed])
    return errors


def calculate_ave_errors(errors):
    """evaluate_vo.py:80-96: per-length mean rotation (deg/m) and translation (fraction) errors."""
    rot, tra, tra_all = [], [], []
    for length in LENGTHS:
        r = [e[1] for e in errors if abs(e[3] - length) < 1]
        t = [e[2] for e in errors if abs(e[3] - length) < 1]
        tra_all.append(t)
        if r:
            rot.append(sum(r) / len(r))
            tra.append(sum(t) / len(t))
    return np.array(rot) * 180 / np.pi, tra, tra_all


def patch(data, window=10, step=2):
    """evaluate_scale.py:19-23."""
    data = np.asarray(data)
    return np.abs(np.array([np.sum(data[i:i + window]) for i in range(0, data.shape[0] - window, step)])) / window


def evaluate_scale(gt, re):
    """evaluate_scale.py:4-13, returned instead of printed: (mean |err|, max |err|, share within
    0.1/0.2/0.3/0.5, windowed drift for windows 10..800)."""
    gt, re = np.asarray(gt, dtype=np.float64), np.asarray(re, dtype=np.float64)
    n = re.shape[0]
    er = np.abs(gt[:n] - re)
    head = (np.mean(er), np.max(er), 1 - np.sum(er > 0.1) / n, 1 - np.sum(er > 0.2) / n, 1 - np.sum(er > 0.3) / n,
            1 - np.sum(er > 0.5) / n)
    ers = gt[:n] - re
    drift = [np.mean(patch(ers, w, 10)) for w in [10, 20, 50, 100, 200, 300, 400, 500, 600, 700, 800]]
    return head, drift


def scale_filter(data, window=10):
    """evaluate_scale.py:24-28, ``filter`` (named so as not to shadow the builtin): the running median over the last ``window``
    values, the first entry the value itself."""
    data = np.asarray(data)
    out = [data[0]]
    for i in range(1, data.shape[0]):
        out.append(np.median(data[max(i - window + 1, 0):i + 1]))
    return np.array(out)


def pose2motion(poses):
    """transformation.py:23-32."""
    poses = np.asarray(poses)
    out = np.zeros((poses.shape[0] - 1, 12))
    for i in range(poses.shape[0] - 1):
        out[i] = (np.linalg.inv(_mat(poses[i])) @ _mat(poses[i + 1]))[:3].reshape(-1)
    return out


# ---- the repeated runs' score (/root/reference/test_off_line.sh:11-23) ------------------------------------------------------------
def trimmed_mean(values):
    """/root/reference/script/score_calculation.py:21-22: sort, drop the best and the worst, take the mean."""
    v = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    if v.size < 3:
        raise ValueError("trimmed_mean: at least three values (the best and the worst are dropped), got %d" % v.size)
    return float(np.mean(v[1:-1]))


def repeat_scores(poses_gt, paths):
    """What evaluate_vo.py:104-107 prints for every path of a repeated run — the per-length translation and rotation errors (eight
    each on a sequence long enough for every length) and their two means — and, over the cases, the trimmed mean of each
    (score_calculation.py:17-22, calculate_mean.py).

    The reference picks ONE field of evaluate_vo's printed log by its position in a comma split (score_calculation.py:3-7) and its
    scale branch raises NameError (:13 returns a name that is not defined there); neither is mirrored: every figure is returned by
    name.  Returns ``{"tra": (C, L), "rot": (C, L), "tra_mean": (C,), "rot_mean": (C,), "trimmed": {...the same four keys...}}``."""
    tra, rot = [], []
    for p in paths:
        r, t, _ = calculate_ave_errors(calculate_sequence_error(poses_gt, p))
        tra.append(np.asarray(t, dtype=np.float64))
        rot.append(np.asarray(r, dtype=np.float64))
    tra, rot = np.array(tra), np.array(rot)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = {"tra": tra, "rot": rot, "tra_mean": tra.mean(axis=1), "rot_mean": rot.mean(axis=1)}      # evaluate_vo.py:107
    out["trimmed"] = {"tra": np.array([trimmed_mean(tra[:, k]) for k in range(tra.shape[1])]),
                      "rot": np.array([trimmed_mean(rot[:, k]) for k in range(rot.shape[1])]),
                      "tra_mean": trimmed_mean(out["tra_mean"]), "rot_mean": trimmed_mean(out["rot_mean"])}
    return out


# ---- the same scores on the device (csrc/mvosr_score.hip) ---------------------------------------------------------------------------
def _reduce_scores(tra, rot):
    """The dict of :func:`repeat_scores` from its two ``(C, L)`` tables."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = {"tra": tra, "rot": rot, "tra_mean": tra.mean(axis=1), "rot_mean": rot.mean(axis=1)}      # evaluate_vo.py:107
    out["trimmed"] = {"tra": np.array([trimmed_mean(tra[:, k]) for k in range(tra.shape[1])]),
                      "rot": np.array([trimmed_mean(rot[:, k]) for k in range(rot.shape[1])]),
                      "tra_mean": trimmed_mean(out["tra_mean"]), "rot_mean": trimmed_mean(out["rot_mean"])}
    return out


def _context(ctx, device):
    from . import _lib
    return ctx if ctx is not None else _lib.default_context(device)


def _stack_of_paths(poses):
    """``(rows, 12)`` or ``(C, rows, 12)`` -> (the stack, whether the input was one path)."""
    p = np.asarray(poses, dtype=np.float64)
    single = p.ndim == 2
    p = np.ascontiguousarray(p.reshape((1,) + p.shape if single else p.shape))
    if p.ndim != 3 or p.shape[2] != 12 or p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError("a path is (rows, 12) with at least one pose, a stack (C, rows, 12); got %r" % (np.shape(poses),))
    return p, single


def _raise_status(status, what):
    from . import _lib
    status = np.asarray(status).reshape(-1)
    if (status == _lib.ST_ERR_MASK).any():
        raise IndexError("%s: case %d's path has fewer poses than a segment of the ground truth needs (evaluate_vo.py:66)"
                         % (what, int(np.nonzero(status == _lib.ST_ERR_MASK)[0][0])))
    if (status == _lib.ST_ERR_SINGULAR).any():
        raise np.linalg.LinAlgError("%s: singular matrix (case %d: a pose with an all-zero rotation block)"
                                    % (what, int(np.nonzero(status == _lib.ST_ERR_SINGULAR)[0][0])))


def pose2motion_batch(poses, speed=None, ctx=None, device=0, want="motions"):
    """mvosr_pose2motion_batch for one path or a stack: ``want`` = "motions" (``(C, n, 12)``; with ``speed`` change_scale.py's
    re-scaled ones), "norms" (``(C, n)``) or "device" (the motions left on the device: buffer, C, n)."""
    from . import _lib
    ctx = _context(ctx, device)
    p, single = _stack_of_paths(poses)
    C, n = p.shape[0], p.shape[1] - 1
    d_speed = None
    if speed is not None:
        s = np.asarray(speed, dtype=np.float64)
        if s.ndim == 0:
            s = np.full(n, float(s))
        if s.shape != (n,):
            raise ValueError("change_scale: %d speeds for %d motions (change_scale.py:15 broadcasts one per frame)" % (s.size, n))
        d_speed = ctx.to_device(s)
    d_poses = ctx.to_device(p)
    d_status = ctx.empty(C, np.int32)
    d_motions = ctx.empty((C, n, 12), np.float64) if want != "norms" else None
    d_norms = ctx.empty((C, n), np.float64) if want == "norms" else None
    _lib.check(ctx.lib.mvosr_pose2motion_batch(ctx.handle, C, n, d_poses.ptr, d_speed.ptr if d_speed else None,
                                               d_motions.ptr if d_motions else None, d_norms.ptr if d_norms else None, d_status.ptr),
               "mvosr_pose2motion_batch")
    _raise_status(d_status.download(), "pose2motion")
    if want == "device":
        return d_motions, C, n
    out = (d_norms if want == "norms" else d_motions).download()
    return out[0] if single else out


def calculate_speed(poses, ctx=None, device=0):
    """script/calculate_speed.py:8-11 on the device: the norms of a path's relative translations, ``(n,)`` — ``(C, n)`` for a stack."""
    return pose2motion_batch(poses, ctx=ctx, device=device, want="norms")


def change_scale(poses, speed, ctx=None, device=0):
    """script/change_scale.py:12-18 on the device: every relative translation divided by (its norm + 0.00001) and multiplied by
    ``speed`` (one value, or one per frame as the script reads them from the ground truth's speed file), then integrated again.
    One path or a stack; the result has the input's shape."""
    from . import _lib
    ctx = _context(ctx, device)
    single = np.ndim(poses) == 2
    d_motions, C, n = pose2motion_batch(poses, speed=speed, ctx=ctx, want="device")
    d_out = ctx.empty((C, n + 1, 12), np.float64)
    _lib.check(ctx.lib.mvosr_paths_batch(ctx.handle, n, C, d_motions.ptr, n * 12, None, d_out.ptr), "mvosr_paths_batch")
    out = d_out.download()
    return out[0] if single else out


class Scorer:
    """:func:`repeat_scores` on the device for one ground-truth path: the segment table (evaluate_vo.py:5-19, 52-65) is built once,
    here, by mvosr_segment_table; every call then scores C paths with mvosr_score_cases_batch — one workgroup per case — and brings
    back the per-length means and counts only.

    ``segments``: ``first``, ``last`` and ``length_index`` of every segment in the reference's order (host integers), ``speed`` per
    segment (evaluate_vo.py:72-73, from the integers).  ``columns``: which of the eight lengths have a segment — the columns of
    ``tra`` and ``rot``, as calculate_ave_errors drops an empty length."""

    def __init__(self, poses_gt, device=0, ctx=None):
        from . import _lib
        self.ctx = ctx = _context(ctx, device)
        gt, _ = _stack_of_paths(np.asarray(poses_gt, dtype=np.float64).reshape(-1, 12))
        self.n_poses = N = gt.shape[1]
        self.n_first = F = int(ctx.lib.mvosr_score_firsts(N))
        self._gt = ctx.to_device(gt[0])
        self._dist = ctx.empty(N, np.float64)
        self._last = ctx.empty((F, _lib.SCORE_LENGTHS), np.int32)
        self._gdelta = ctx.empty((F, _lib.SCORE_LENGTHS, 24), np.float64)        # hi, lo
        status = ctx.empty(1, np.int32)
        _lib.check(ctx.lib.mvosr_segment_table(ctx.handle, N, self._gt.ptr, self._dist.ptr, self._last.ptr, self._gdelta.ptr, status.ptr),
                   "mvosr_segment_table")
        _raise_status(status.download(), "Scorer")
        self.last = self._last.download()
        self.has = self.last >= 0
        self.columns = self.has.any(axis=0)
        self.counts = self.has.sum(axis=0).astype(np.int32)
        f, li = np.nonzero(self.has)                                                        # row-major: first, then length
        first, last = f * STEP, self.last[f, li].astype(np.int64)
        self.segments = {"first": first, "last": last, "length_index": li,
                         "speed": np.asarray(LENGTHS, dtype=np.float64)[li] / (0.1 * (last - first + 1).astype(np.float64))}

    def dist(self):
        """evaluate_vo.py:5-13's cumulative distances as the table was built from them."""
        return self._dist.download()

    # -- launches
    def _paths_on_device(self, motions, scales):
        from . import _lib
        ctx = self.ctx
        m = np.ascontiguousarray(np.asarray(motions, dtype=np.float64).reshape(-1, 12))
        s = np.ascontiguousarray(np.asarray(scales, dtype=np.float64))
        s = s.reshape(1, -1) if s.ndim == 1 else s
        if s.ndim != 2 or s.shape[0] < 1 or s.shape[1] != m.shape[0]:
            raise ValueError("scales is (C, n) for motions (n, 12); got %r and %r" % (s.shape, m.shape))
        C, n = s.shape
        d_paths = ctx.empty((C, n + 1, 12), np.float64)
        d_m, d_s = ctx.to_device(m), ctx.to_device(s)
        _lib.check(ctx.lib.mvosr_paths_batch(ctx.handle, n, C, d_m.ptr, 0, d_s.ptr, d_paths.ptr), "mvosr_paths_batch")
        return d_paths

    def _score(self, d_paths, rows=False):
        """``d_paths``: a device buffer ``(C, rows, 12)``.  Returns (means (C, 2, 8), r_seg, t_seg) — the two tables only with ``rows``."""
        from . import _lib
        ctx = self.ctx
        C, n_rows = d_paths.shape[0], d_paths.shape[1]
        L = _lib.SCORE_LENGTHS
        res = ctx.block([("means", (C, 2, L), np.float64), ("counts", (C, L), np.int32), ("status", (C,), np.int32)])
        seg = ctx.empty((2, C, self.n_first, L), np.float64) if rows else None
        half = C * self.n_first * L * 8
        _lib.check(ctx.lib.mvosr_score_cases_batch(ctx.handle, C, n_rows, d_paths.ptr, self.n_first, self._last.ptr, self._gdelta.ptr,
                                                   seg.ptr if rows else None, seg.ptr + half if rows else None, res["means"].ptr,
                                                   res["counts"].ptr, res["status"].ptr), "mvosr_score_cases_batch")
        means, counts, status = res["means"].download(), res["counts"].download(), res["status"].download()
        _raise_status(status, "Scorer")
        assert np.array_equal(counts, np.broadcast_to(self.counts, counts.shape)), "segment counts differ from the table's"
        if not rows:
            return means, None, None
        both = seg.download()
        return means, both[0], both[1]

    def _to_device(self, paths):
        from . import _lib
        if isinstance(paths, _lib.DeviceBuffer):
            return paths
        return self.ctx.to_device(_stack_of_paths(paths)[0])

    def _dict(self, means):
        rot = means[:, 0, :][:, self.columns] * 180 / np.pi                                 # evaluate_vo.py:96
        tra = np.ascontiguousarray(means[:, 1, :][:, self.columns])
        return _reduce_scores(tra, rot)

    # -- the public calls
    def score_paths(self, paths):
        """``paths``: ``(C, rows, 12)`` (host array, list of paths, or a device buffer).  The dict of :func:`repeat_scores`."""
        return self._dict(self._score(self._to_device(paths))[0])

    def score_scales(self, motions, scales):
        """Integrate ``motions (n, 12)`` under every row of ``scales (C, n)`` (offline.get_path) and score the C paths: two launches,
        one small download."""
        return self._dict(self._score(self._paths_on_device(motions, scales))[0])

    def score_gt_rescaled(self, scales):
        """tesh.sh:6-8 for every case ("evaluation gt+vo_scale"): the ground truth's own motions with their translations re-scaled
        to case c's scales — ``scale * t / (|t| + 0.00001)``, change_scale.py:12-18 —, integrated and scored against the ground
        truth: what is left is the scale's share of the path error.  ``scales``: ``(C, n)`` (host array or device buffer) with
        ``n == n_poses - 1``.  One mvosr_pose2motion_batch per case (its speed argument is one case's), then mvosr_paths_batch and
        mvosr_score_cases_batch once.  The dict of :meth:`score_scales`."""
        from . import _lib
        ctx = self.ctx
        d_s, C, n, _ = _scales_stack(scales)
        if n != self.n_poses - 1:
            raise ValueError("score_gt_rescaled: %d scales per case for %d motions of the ground truth (change_scale.py:15 broadcasts "
                             "one per frame)" % (n, self.n_poses - 1))
        d_s = _on_device(ctx, d_s)
        d_motions, d_status = ctx.empty((C, n, 12), np.float64), ctx.empty(C, np.int32)
        for c in range(C):
            _lib.check(ctx.lib.mvosr_pose2motion_batch(ctx.handle, 1, n, self._gt.ptr, d_s.ptr + c * n * 8, d_motions.ptr + c * n * 96,
                                                       None, d_status.ptr + 4 * c), "mvosr_pose2motion_batch")
        d_paths = ctx.empty((C, n + 1, 12), np.float64)
        _lib.check(ctx.lib.mvosr_paths_batch(ctx.handle, n, C, d_motions.ptr, n * 12, None, d_paths.ptr), "mvosr_paths_batch")
        _raise_status(d_status.download(), "score_gt_rescaled")
        return self._dict(self._score(d_paths)[0])

    def errors(self, paths=None, motions=None, scales=None):
        """Per case the rows ``[first, r_err/len, t_err/len, len, speed]`` of calculate_sequence_error, in its order."""
        d_paths = self._to_device(paths) if paths is not None else self._paths_on_device(motions, scales)
        _, r, t = self._score(d_paths, rows=True)
        seg = self.segments
        first, length, speed = seg["first"].tolist(), [LENGTHS[i] for i in seg["length_index"].tolist()], seg["speed"].tolist()
        return [list(map(list, zip(first, r[c][self.has].tolist(), t[c][self.has].tolist(), length, speed))) for c in range(r.shape[0])]


# ---- the scales' own score on the device (csrc/mvosr_scalescore.hip; evaluate_scale.py, tesh.sh:4-8) ---------------------------------
SCALE_WINDOWS = [10, 20, 50, 100, 200, 300, 400, 500, 600, 700, 800]        # evaluate_scale.py:10
SCALE_STEP = 10                                                             # evaluate_scale.py:11
SCALE_THRESHOLDS = [0.1, 0.2, 0.3, 0.5]                                     # evaluate_scale.py:7


def _scales_stack(scales):
    """``(n,)`` or ``(C, n)`` host scales, or a device buffer ``(C, n)`` of doubles -> (the ``(C, n)`` array or the buffer, C, n,
    whether the input was one row).  Nothing is uploaded here: the callers check their arguments first."""
    from . import _lib
    if isinstance(scales, (_lib.DeviceBuffer, _lib.DeviceView)):
        if len(scales.shape) != 2 or scales.dtype != np.float64 or scales.shape[0] < 1:
            raise ValueError("scales on the device are (C, n) doubles; got %r %s" % (scales.shape, scales.dtype))
        return scales, scales.shape[0], scales.shape[1], False
    s = np.asarray(scales, dtype=np.float64)
    single = s.ndim == 1
    s = np.ascontiguousarray(s.reshape(1, -1) if single else s)
    if s.ndim != 2 or s.shape[0] < 1:
        raise ValueError("scales is (n,) or (C, n) with at least one case; got %r" % (np.shape(scales),))
    return s, s.shape[0], s.shape[1], single


def _on_device(ctx, s):
    return s if not isinstance(s, np.ndarray) else ctx.to_device(s)


def scale_errors(speed_gt, scales, windows=SCALE_WINDOWS, step=SCALE_STEP, thresholds=SCALE_THRESHOLDS, ctx=None, device=0, variant=None):
    """:func:`evaluate_scale` for C cases in one launch (mvosr_scale_errors_batch), every float the reference's own double.

    ``speed_gt``: the ground truth's speeds (host array, or a device buffer of doubles), at least as many as a case has scales —
    the reference's subtraction raises ValueError otherwise, and so does this.  ``scales``: ``(n,)``, ``(C, n)`` or a device
    buffer ``(C, n)``.  ``variant``: None (by size), "global" — the global-memory form at any size.
    Returns ``{"mean", "max": (C,); "exceed_counts": (C, T) int; "within": (C, T) = 1 - count / n; "drift": (C, W); "n"}`` — for
    ``(n,)`` scales without the leading axis.  No scale at all (n = 0): mean and max NaN, counts zero (the reference raises)."""
    from . import _lib
    d_s, C, n, single = _scales_stack(scales)
    if isinstance(speed_gt, (_lib.DeviceBuffer, _lib.DeviceView)):
        d_gt, n_gt = speed_gt, int(np.prod(speed_gt.shape))
    else:
        gt = np.ascontiguousarray(np.asarray(speed_gt, dtype=np.float64).reshape(-1))
        d_gt, n_gt = None, gt.size
    if n > n_gt:
        raise ValueError("operands could not be broadcast together with shapes (%d,) (%d,) (evaluate_scale.py:6: more scales than "
                         "ground-truth speeds)" % (n_gt, n))
    w = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1)
    t = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    if w.size > _lib.SCALE_MAX_WINDOWS or t.size > _lib.SCALE_MAX_THRESHOLDS or int(step) < 1 or (w.size and (w.min() < 1 or w.max() > _lib.SCALE_MAX_WINDOW)):
        raise ValueError("scale_errors: at most %d windows in 1..%d, %d thresholds, step >= 1"
                         % (_lib.SCALE_MAX_WINDOWS, _lib.SCALE_MAX_WINDOW, _lib.SCALE_MAX_THRESHOLDS))
    if variant not in (None, "global"):
        raise ValueError("scale_errors: variant is None or 'global'")
    W, T = int(w.size), int(t.size)
    ctx = _context(ctx, device)
    d_s = _on_device(ctx, d_s)
    if d_gt is None:
        d_gt, n_gt = ctx.to_device(gt[:n]), n
    res = ctx.block([("stats", (C, 2), np.float64), ("drift", (C, max(W, 1)), np.float64), ("counts", (C, max(T, 1)), np.int32),
                     ("status", (C,), np.int32)])
    _lib.check(ctx.lib.mvosr_scale_errors_batch(ctx.handle, n_gt, d_gt.ptr, C, n, d_s.ptr, n, W, _lib.addr(w) if W else None, int(step), T,
                                                _lib.addr(t) if T else None, _lib.SCALE_ERRORS_GLOBAL if variant == "global" else 0,
                                                res["stats"].ptr, res["counts"].ptr, res["drift"].ptr, res["status"].ptr),
               "mvosr_scale_errors_batch")
    stats, drift = res["stats"].download(), res["drift"].download().reshape(C, -1)[:, :W]
    counts, status = res["counts"].download().reshape(C, -1)[:, :T].astype(np.int64), res["status"].download()
    assert ((status == 0) | (status == _lib.ST_ERR_EMPTY)).all() and ((status == _lib.ST_ERR_EMPTY).all() if n == 0 else (status == 0).all())
    with np.errstate(all="ignore"):
        within = 1 - counts / n if n else np.full(counts.shape, np.nan)                     # evaluate_scale.py:7, from the integers
    out = {"mean": stats[:, 0].copy(), "max": stats[:, 1].copy(), "exceed_counts": counts, "within": within,
           "drift": np.ascontiguousarray(drift), "n": n}
    if single:
        out = {k: (v[0] if k != "n" else v) for k, v in out.items()}
    return out


def filter_scales(scales, window=10, ctx=None, device=0, on_device=False):
    """:func:`scale_filter` for C sequences in one launch (mvosr_window_median_cases), bit for bit.  ``scales``: ``(n,)``, ``(C, n)``
    or a device buffer ``(C, n)``; the result has the input's shape — with ``on_device`` it is left there as a ``(C, n)`` buffer.
    The device median holds its window in registers: ``window`` is 1..64."""
    from . import _lib
    if not 1 <= int(window) <= _lib.MAX_MEDIAN_WINDOW:
        raise ValueError("filter_scales: window must be in 1..%d, got %r" % (_lib.MAX_MEDIAN_WINDOW, window))
    d_s, C, n, single = _scales_stack(scales)
    ctx = _context(ctx, device)
    d_s = _on_device(ctx, d_s)
    d_out = ctx.empty((C, n), np.float64)
    _lib.check(ctx.lib.mvosr_window_median_cases(ctx.handle, d_s.ptr, C, n, n, int(window), d_out.ptr, n), "mvosr_window_median_cases")
    if on_device:
        return d_out
    out = d_out.download()
    return out[0] if single else out
