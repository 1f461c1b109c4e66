"""The reference's ``script/data_check.py`` — the author's check of the premise both feature votes rest on: over road points,
depth falls as the image row rises — with its one quadratic computation on the device.

``depth_check`` (data_check.py:19-34) computes, for all ordered pairs of a frame's points below the camera, the slope
``(d_j - d_i) / ((v_j / d_j - v_i / d_i) + 1e-6)``, histograms the slopes over ``np.array(range(-40, 20)) * 50`` and prints the
maximum.  Here the n x n slopes never exist: mvosr_depth_check_batch (csrc/mvosr_depthcheck.hip) leaves, per frame and
population, the 59 counts, what lies below, above and is NaN, and the maximum, byte for byte what NumPy computes from the
matrix.  Nothing is drawn.  ``road_profile`` / ``road_cloud`` are the selections of ``vis_2d`` (:35-40) and ``vis_3d`` (:6-16),
``compare`` is what the script's ``main`` (:41-49) puts side by side.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import _lib

BINS = np.array(list(range(-40, 20))) * 50                     # data_check.py:30
POPULATIONS = _lib.FD_POPULATIONS
N_BINS, TABLE_WORDS = _lib.DC_BINS, _lib.DC_TABLE_WORDS
ST_NO_POINT, ST_ERR_MASK = _lib.ST_DC_NO_POINT, _lib.ST_ERR_MASK
CHUNK = 512                                                    # frames a launch of depth_check_batch


class DepthCheck(NamedTuple):
    """One population of one frame: ``hist`` = ``np.histogram(matrix, bins)[0]``, ``below`` / ``above`` / ``nan`` = the pairs
    outside the bins, ``max`` = ``np.max(matrix)``, ``n`` = the selected points (``matrix`` is n x n)."""
    bins: np.ndarray
    hist: np.ndarray
    below: int
    above: int
    nan: int
    max: float
    n: int


class DepthCheckBatch(NamedTuple):
    """Per frame and population (0 every point, 1 kept by the vote, 2 selected): ``hist`` [F, 3, 59], ``below`` / ``above`` /
    ``nan`` / ``n`` [F, 3] int64, ``max`` [F, 3]; per frame ``status`` (0, ``ST_NO_POINT``, ``ST_ERR_MASK``); ``errors``: frame ->
    the exception the staged pass met there (the estimator's batch call only)."""
    hist: np.ndarray
    below: np.ndarray
    above: np.ndarray
    nan: np.ndarray
    max: np.ndarray
    n: np.ndarray
    status: np.ndarray
    errors: dict

    def frame(self, f, population=0):
        p = int(population)
        return DepthCheck(BINS, self.hist[f, p], int(self.below[f, p]), int(self.above[f, p]), int(self.nan[f, p]),
                          float(self.max[f, p]), int(self.n[f, p]))

    def tables(self):
        """What the frames with status 0 add to the sequence tables: int64 [3, 62] — the bins, then below, above, nan."""
        ok = self.status == 0
        return np.concatenate([self.hist[ok].sum(0), self.below[ok].sum(0)[:, None], self.above[ok].sum(0)[:, None],
                               self.nan[ok].sum(0)[:, None]], axis=1).astype(np.int64)


FIELDS = ("hist", "below", "above", "nan", "max", "n", "status")


def _empty():
    P = POPULATIONS
    return DepthCheckBatch(np.zeros((0, P, N_BINS), np.int64), np.zeros((0, P), np.int64), np.zeros((0, P), np.int64),
                           np.zeros((0, P), np.int64), np.zeros((0, P)), np.zeros((0, P), np.int64), np.zeros(0, np.int32), {})


def concatenate(parts, errors=None):
    parts = list(parts) or [_empty()]
    return DepthCheckBatch(*(np.concatenate([getattr(p, k) for p in parts]) for k in FIELDS), dict(errors or {}))


def new_tables(device=0, ctx=None):
    """Zeroed sequence tables on the device: int64 [3][62], to be passed to ``depth_check_batch`` call after call."""
    ctx = ctx if ctx is not None else _lib.default_context(device)
    return ctx.zeros((POPULATIONS, TABLE_WORDS), np.int64)


def launch_packed(ctx, off, cnt, y, z, level, max_feat, tables=None):
    """One launch of mvosr_depth_check_batch over host arrays in the packed layout (frame f: ``off[f]`` .. ``off[f] + cnt[f]`` of
    ``y``, ``z``, ``level``) -> ``DepthCheckBatch``.  ``tables``: a device buffer from ``new_tables`` the launch adds to."""
    F, P = len(cnt), POPULATIONS
    G = max(F, 1)
    total = max(len(y), len(z), len(level), 2)
    blk = ctx.block([("off", G, np.int64), ("cnt", G, np.int32), ("y", total, np.float64), ("z", total, np.float64),
                     ("level", total, np.uint8)])
    out = ctx.block([("hist", (G, P, N_BINS), np.int64), ("below", (G, P), np.int64), ("above", (G, P), np.int64),
                     ("nan", (G, P), np.int64), ("max", (G, P), np.float64), ("n", (G, P), np.int64), ("status", G, np.int32)])
    try:
        pad = lambda a, n, dt: np.concatenate([np.asarray(a, dtype=dt).reshape(-1), np.zeros(n - len(a), dtype=dt)])
        blk.upload({"off": pad(off, G, np.int64), "cnt": pad(cnt, G, np.int32), "y": pad(y, total, np.float64),
                    "z": pad(z, total, np.float64), "level": pad(level, total, np.uint8)})
        params = _lib.DepthCheckParams(int(max_feat), 0)
        o = _lib.DepthCheckOutputs(*(out[k].ptr for k in FIELDS))
        _lib.check(ctx.lib.mvosr_depth_check_batch(ctx.handle, F, blk["off"].ptr, blk["cnt"].ptr, blk["y"].ptr, blk["z"].ptr,
                                                   blk["level"].ptr, C.byref(params), C.byref(o),
                                                   tables.ptr if tables is not None else None), "mvosr_depth_check_batch")
        return DepthCheckBatch(*(out[k].download()[:F] for k in FIELDS), {})
    finally:
        out.free()
        blk.free()


def check_points(points_list, levels=None):
    """The frames as float64 [n, >= 3] arrays and their levels as uint8 [n] (None: every point in every population)."""
    pts = []
    for f, p in enumerate(points_list):
        a = np.asarray(p, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("depth_check: frame %d has shape %s, not (n, 3) with the columns x, y, depth" % (f, a.shape))
        pts.append(a)
    if levels is None:
        return pts, [np.full(len(a), 2, np.uint8) for a in pts]
    if len(levels) != len(pts):
        raise ValueError("depth_check: %d frames but %d level arrays" % (len(pts), len(levels)))
    lvs = []
    for f, (a, lv) in enumerate(zip(pts, levels)):
        lv = np.asarray(lv)
        if lv.shape != (len(a),):
            raise ValueError("depth_check: frame %d has %d points but levels of shape %s" % (f, len(a), lv.shape))
        if lv.size and (lv.min() < 0 or lv.max() > 2):
            raise ValueError("depth_check: frame %d has a level outside 0, 1, 2" % f)
        lvs.append(lv.astype(np.uint8))
    return pts, lvs


def depth_check_batch(points_list, levels=None, tables=None, device=0):
    """``depth_check`` of every frame of ``points_list`` ((n, 3) arrays, the reference's columns: column 1 = y, column 2 = depth),
    one launch per chunk of ``CHUNK`` frames -> ``DepthCheckBatch`` (arrays [F, 3, ...]).  ``levels``: per frame one level per
    point (0, 1 or 2), the three populations; None: every point in every population.  A frame with no point of y > 0 gets
    ``ST_NO_POINT`` and NaN; it does not raise.  ``tables``: from ``new_tables``, added to."""
    pts, lvs = check_points(points_list, levels)
    ctx = tables.ctx if tables is not None else _lib.default_context(device)
    parts = []
    for a in range(0, len(pts), CHUNK):
        chunk, clv = pts[a:a + CHUNK], lvs[a:a + CHUNK]
        cnt = np.array([len(p) for p in chunk], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(cnt[:-1], dtype=np.int64)]).astype(np.int64)
        y = np.concatenate([p[:, 1] for p in chunk])
        z = np.concatenate([p[:, 2] for p in chunk])
        parts.append(launch_packed(ctx, off, cnt, y, z, np.concatenate(clv), int(cnt.max()), tables))
    return concatenate(parts)


def depth_check(data, device=0):
    """data_check.py:19-34 without the figure -> ``DepthCheck``.  ValueError where the reference's ``np.max`` raises: no point of
    y > 0."""
    res = depth_check_batch([data], device=device)
    if int(res.status[0]) == ST_NO_POINT:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")       # :32
    return res.frame(0)


def road_profile(points, y_max=10.0):
    """vis_2d's selection (:36-40): the points with 0 < y < y_max as ``(z, -y)``."""
    points = np.asarray(points)
    select_id = np.array(points[:, 1] > 0) & np.array(points[:, 1] < y_max)
    return points[select_id, 2], -points[select_id, 1]


def road_cloud(points, y_max=2.0):
    """vis_3d's selection (:9-12): the points with 0 < y < y_max as ``(x, z, -y)``."""
    points = np.asarray(points)
    select_id = np.array(points[:, 1] > 0) & np.array(points[:, 1] < y_max)
    return points[select_id, 0], points[select_id, 2], -points[select_id, 1]


class Comparison(NamedTuple):
    profile_all: tuple
    profile_left: tuple
    check_all: DepthCheck
    check_left: DepthCheck


def compare(points_all, points_left, device=0):
    """What the script's ``main`` (:41-49) sets side by side — the points before the rejection and the points left after it:
    their two profiles and their two depth checks, from one launch.  ValueError where either has no point of y > 0."""
    res = depth_check_batch([points_all, points_left], device=device)
    if np.any(res.status == ST_NO_POINT):
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    return Comparison(road_profile(points_all), road_profile(points_left), res.frame(0), res.frame(1))
