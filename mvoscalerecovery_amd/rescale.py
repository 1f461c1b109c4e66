"""Drop-in for the reference's *other* ``ScaleEstimator`` — /root/reference/src/rescale.py:22-193,
the one /root/reference/src/main.py:20 and main_offline.py:20 import — backed by the MI355X kernels.

    from mvoscalerecovery_amd.rescale import ScaleEstimator

Per frame (rescale.py:113-148,151-178,191-193):

    host   vanishing-row filter (:115), Delaunay #1 (:124)                         [SciPy]
    GPU    GraphChecker.find_inliers tallies (graph.py:18-36)                      [mvosr_graph_inliers_batch]
    host   valid = good/total > 0.5; if more than 10 survive: filter + Delaunay #2 (:133-137)
    GPU    flat_selection: normals, 1/|n| heights, median level, kept triangles (:75-102)  [mvosr_flat_selection_batch]
    GPU    RANSAC plane over the kept triangles' vertices (:151-167)                [mvosr_ransac_plane_batch]
    host   height -> scale, +-0.3 slew limiter, window median (:167-178)

The reference's RANSAC re-seeds `random` from OS entropy on every call
(/root/reference/src/thirdparty/Ransac/ransac.py:6), so its output is not reproducible; it is a
deterministic function of the sample triples.  Here the triples are drawn on the host —
``random.sample(range(M), 3)`` like the reference, seeded with ``ransac_seed`` (None = OS entropy, the
reference's behaviour) or supplied by ``sampler(M) -> (H,3)`` — and the GPU evaluates all hypotheses
and replays the reference's sequential best/stop rule.  With the same triples the results equal the
reference's (tests/golden/rescale.npz); without, agreement is statistical only.

``triangulation="gpu"`` is the device-resident path: C packer -> ONE upload -> Delaunay #1 (mvosr_delaunay_batch) ->
GraphChecker vote with the decision made on the device (mvosr_graph_keep_batch) -> Delaunay #2 over the survivors, seeded
-> flat_selection + RANSAC plane in one kernel per frame (mvosr_flat_ransac_batch) -> after the last chunk the slew
limiter and the window median: a sequential recurrence over results that are on the host anyway (the statuses decide where
the reference would raise), walked by one core in C (mvosr_slew_median_host; the device form mvosr_slew_median exists and is
tested, the estimator does not use it).  No host step between the device stages.  The deterministic stages carry no deviation:
the vote's edge potential is symmetric, so its mask is a function of the triangle SET (graph.py:18-36,124-145);
flat_selection keeps a set of triangles (rescale.py:75-96); only the order of its point list (:101) follows the rows,
and the RANSAC draws list positions uniformly (ransac.py:10) — here from a counter-based sequence keyed by
``ransac_seed`` (None: OS entropy, the reference's behaviour).  A draw that names one vertex twice (the list repeats vertices:
0.5-2 % of the reference's draws) spends its iteration, as in the reference (ransac.py:8-21), and counts zero inliers — the
reference's SVD of such a rank-2 sample returns a plane picked by rounding noise, which its own recorded run shows losing to every
real hypothesis (tests/golden/rescale.npz frame 26); rounds 4-5 drew such a sample again (a declared deviation: gone).  The scale
distribution is compared with the unseeded reference's in tests/test_gpu_rescale.py.  ``triangulation="scipy", sampling="device"`` runs the
same kernels on SciPy's triangulations brought to the same row form, with bit-identical results.

``model="static_tri"`` and ``model="static"`` are the two road models rescale.py:194-195 leave commented out behind the RANSAC plane,
on the staged path: the mode of the flat triangles' inverse heights (mvosr_static_tri_batch, launched on flat_selection's device
buffers; :179-187) and scale_calculator's road model on the selected points through the inner estimator ``self.sc`` (:31).  Both are
deterministic: tests/golden/statictri.npz holds the reference's own sequences, reproduced bit for bit.
``model="static_tri", model_resident=True`` runs the first of them on the device-resident path instead: the same streamed stages as
the RANSAC model, every frame ending in flat_selection + the histogram-mode road model in one kernel (mvosr_flat_static_tri_batch),
the same sequence bit for bit.

The numbers of rescale.py:85-96,152,155,169-172 are a value, ``RescaleConstants`` (``constants=``; None: the reference's literals),
and ``ConstantSweep`` runs K settings of them over a sequence in one pass of the stages that do not read them.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import itertools
import math
import os
import random
import time
from collections import deque

import numpy as np

from . import _lib
from . import constants as K
from . import graph
from . import packing
from . import stream
from .engine import DeviceBatch, ScaleEngine, frame_tables, pack_upload_native

EDGE_POTENTIAL = [[3, 1], [2, 2], [2, 2], [0, 4]]     # rescale.py:32
VANISH = 185                                          # rescale.py:30
RANSAC_ITERATIONS = 100                               # rescale.py:155
RANSAC_THRESHOLD = 0.005                              # rescale.py:155
RANSAC_GOAL = 0.8                                     # estimate_road_norm.py:68
RANSAC_MIN_POINTS = 12                                # rescale.py:152
MIN_VALID_FOR_RETRI = 10                              # rescale.py:133
STATIC_TRI_MIN_COUNT = 12                             # rescale.py:181 (more than 12 heights)
SLEW = 0.3                                            # rescale.py:169-172
_FIELDS = ("raw_scale", "height_level", "model", "best_ic", "used", "n_kept", "status")     # a chunk's results, per frame
_STATIC_FIELDS = ("raw_scale", "height_level", "scale_norm", "n_used", "n_kept", "status")   # the same with model_resident=True
_REFUSED = (K.ST_ERR_SINGULAR, K.ST_ERR_MASK, K.ST_ERR_EMPTY)   # the flat selection refuses the frame as a whole: singular row, bad vertex id, no rows
MAX_HYP = 512                                        # mvosr_flat_ransac_batch's limit (include/mvosr.h)


@dataclasses.dataclass(frozen=True)
class RescaleConstants:
    """The numbers of the estimator that the reference's author moved by hand, as one value.  The defaults are the reference's
    live ones: the two pitch thresholds and the factor of the height level (rescale.py:85-96; rescale_test.py:132-150 spells
    them again), the RANSAC's call (:152,155 — rescale.py.origin:218 fits with 30 hypotheses —; estimate_road_norm.py:68) and
    the slew limiter's step (:169-172).  The vote's constants are not part of it: they decide the second triangulation."""
    loose_deg: float = -80.0
    tight_deg: float = -85.0
    height_factor: float = 0.9
    ransac_min_points: int = RANSAC_MIN_POINTS
    n_hyp: int = RANSAC_ITERATIONS
    threshold: float = RANSAC_THRESHOLD
    goal_fraction: float = RANSAC_GOAL
    slew: float = SLEW

    def __post_init__(self):
        for name in ("loose_deg", "tight_deg", "height_factor", "threshold", "goal_fraction", "slew"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError("RescaleConstants.%s must be a finite number, not %r" % (name, v))
            object.__setattr__(self, name, float(v))
        for name in ("ransac_min_points", "n_hyp"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("RescaleConstants.%s must be an integer, not %r" % (name, v))
            object.__setattr__(self, name, int(v))
        for name in ("loose_deg", "tight_deg"):
            if not -90.0 <= getattr(self, name) <= 90.0:
                raise ValueError("RescaleConstants.%s is a pitch in degrees: -90 .. 90" % name)
        if self.height_factor < 0.0:
            raise ValueError("RescaleConstants.height_factor must not be negative")
        if self.ransac_min_points < 3:
            raise ValueError("RescaleConstants.ransac_min_points: a plane takes three points")
        if not 1 <= self.n_hyp <= MAX_HYP:
            raise ValueError("RescaleConstants.n_hyp must be in 1..%d" % MAX_HYP)
        if self.threshold <= 0.0 or self.goal_fraction <= 0.0 or self.slew <= 0.0:
            raise ValueError("RescaleConstants: threshold, goal_fraction and slew must be positive")

    def selection(self):
        """What flat_selection reads."""
        return (self.loose_deg, self.tight_deg, self.height_factor)

    def ransac(self):
        """What the plane fit reads."""
        return (self.ransac_min_points, self.n_hyp, self.threshold, self.goal_fraction)


def good_bits(edge_potential=EDGE_POTENTIAL, prob_threshold=0.6):
    """The 24 bits the vote kernel needs: for each edge-order code (graph.py:124-129) and vertex, is
    the vertex's marginal under the triangle potential (graph.py:6-17,134-145) above 0.6
    (graph.py:131-132)?  A 8x8 table evaluated once per estimator."""
    ep = np.array(edge_potential)
    tp = np.ones((8, 8))
    for row in range(8):
        r = [int(row & 4 != 0), int(row & 2 != 0), int(row & 1 != 0)]
        for col in range(8):
            c = [int(col & 4 != 0), int(col & 2 != 0), int(col & 1 != 0)]
            tp[row, col] = ep[r[0] * 2 + r[1], c[0]] * ep[r[1] * 2 + r[2], c[1]] * ep[r[0] * 2 + r[2], c[2]]
    rng = np.arange(8)
    bits = 0
    for code in range(8):
        pot = tp[:, code]
        z = np.sum(pot)
        with np.errstate(all="ignore"):
            probs = [np.sum(pot[(rng & 4) > 0]) / z, np.sum(pot[(rng & 2) > 0]) / z, np.sum(pot[(rng & 1) > 0]) / z]
        for k, p in enumerate(probs):
            if p > prob_threshold:
                bits |= 1 << (3 * code + k)
    return bits


def chunk_goes_large(sizes, cap):
    """Does a chunk whose frames have ``sizes`` features below the vanishing row take the large-frame kernels?  It does, as a
    whole, when its largest frame exceeds ``cap`` (the resident kernels' limit, ``ScaleEstimator._max_points()``)."""
    return len(sizes) > 0 and int(max(sizes)) > int(cap)


def size_class_runs(sizes, cap, limit):
    """Where ``ScaleEstimator(large_frames=True)`` cuts a call: ``(runs, stop)``.  ``runs``: ``(a, b, large)`` — maximal runs of
    consecutive frames on one side of ``cap``, so that the small frames of a call stay on the resident kernels and every chunk of
    a large run takes the large-frame ones.  ``stop``: index of the first frame beyond ``limit`` (the runs end before it: the call
    ends there with the oversized-frame error), or None."""
    sizes = np.asarray(sizes, dtype=np.int64)
    over = np.nonzero(sizes > limit)[0]
    stop = int(over[0]) if len(over) else None
    F = len(sizes) if stop is None else stop
    runs, a = [], 0
    while a < F:
        large = bool(sizes[a] > cap)
        b = a + 1
        while b < F and bool(sizes[b] > cap) == large:
            b += 1
        runs.append((a, b, large))
        a = b
    return runs, stop


def host_chunks(sizes, step, points=None):
    """The chunks ``(a, b)`` a run of frames with ``sizes`` features takes on the host-triangulation path: ``step`` frames each —
    and, with ``points`` (the runs of large frames: the large-frame kernels' workspace grows with frames x largest row count), cut
    to ``points`` features and to frames x largest frame <= 2 ``points``, as ``stream.plan`` cuts the device path's; one frame at
    least."""
    out, a, F = [], 0, len(sizes)
    while a < F:
        b, total, largest = a, 0, 0
        while b < F and b - a < step:
            big = max(largest, int(sizes[b]))
            if points is not None and b > a and (total + int(sizes[b]) > points or (b - a + 1) * big > 2 * points):
                break
            total, largest, b = total + int(sizes[b]), big, b + 1
        out.append((a, b))
        a = b
    return out


class ScaleEstimator(stream.StreamKnobs):
    N_HYP = RANSAC_ITERATIONS

    def __init__(self, absolute_reference, window_size=6, device=0, ransac_seed=None, sampler=None,
                 delaunay_workers=None, verbose=False, triangulation=None, sampling=None, region="threshold", model="ransac",
                 constants=None, large_frames=False, model_resident=False):
        # model_resident: opt-in.  False: every path, message and state below is what it was.  True, with
        # model="static_tri": the road model runs on the device-resident path — both triangulations, the vote, the flat selection and
        # the histogram-mode road model in one kernel per frame (mvosr_flat_static_tri_batch) —, triangulation and sampling resolving
        # as for the RANSAC model.  Every refusal below happens before a device or the worker pool is asked for.
        if not isinstance(model_resident, (bool, np.bool_)):
            raise TypeError("model_resident must be a bool")
        self.model_resident = bool(model_resident)
        if self.model_resident:
            if model != "static_tri":
                raise ValueError("model_resident=True belongs to model='static_tri' (the RANSAC model is device-resident as it is; "
                                 "model='static' keeps the staged path: its sums follow SciPy's row order)")
            if region == "grow":
                raise ValueError("model_resident=True belongs to model='static_tri' with region='threshold' (region='grow' runs on "
                                 "the staged path)")
            if large_frames:
                raise ValueError("model_resident=True belongs to model='static_tri' within the resident kernels' frame limit "
                                 "(large_frames=True keeps the staged path for this model)")
            if sampling == "host" or sampler is not None:
                raise ValueError("model_resident=True belongs to the device-resident path: triangulation='gpu', or "
                                 "triangulation='scipy' with sampling='device' (no samples are drawn: a host sampler has no part)")
        # large_frames: opt-in.  False: a frame with more features below the vanishing row than one workgroup's LDS
        # holds (``_max_points()``) is refused, as ever.  True: a chunk whose largest frame exceeds that limit sends its vote and its
        # flat selection + RANSAC through the large-frame kernels (mvosr_graph_keep_large_batch, mvosr_flat_ransac_large_batch),
        # up to ``_large_max_points()`` features.  The RANSAC model needs the device-resident path for it: triangulation="gpu", or
        # "scipy" with sampling="device" (anything else is refused below, before a device is needed).  model="static_tri" (staged
        # path) takes it too: its vote and its flat selection go through the same two kernels (_vote_masks, _flat_selection).
        # Accepted and without effect: model="static" and region="grow" — they, RepeatedRuns and ConstantSweep keep the present
        # limit and message whatever this says.
        if not isinstance(large_frames, (bool, np.bool_)):
            raise TypeError("large_frames must be a bool")
        self.large_frames = bool(large_frames)
        # constants: a RescaleConstants (None: the reference's literals — the instance then is what the class always was)
        if constants is not None and not isinstance(constants, RescaleConstants):
            raise TypeError("constants must be a RescaleConstants")
        self.constants = constants if constants is not None else RescaleConstants()
        if constants is not None:
            self.N_HYP = self.constants.n_hyp
        # region "threshold": the road rows are the reference's two thresholds (rescale.py:94-96); "grow": GraphGrow's region over
        # the rows' adjacency (graph.py:85-107, the call rescale.py:99 leaves commented out) — on the staged path only, which it
        # selects (checked first: no device is needed to refuse a combination).  Its kernels hold a frame in LDS: large_frames does
        # not reach it, an oversized frame gets the library's error as before.
        if region not in ("threshold", "grow"):
            raise ValueError("region must be 'threshold' or 'grow'")
        if region == "grow":
            if triangulation not in (None, "scipy") or sampling not in (None, "host"):
                raise ValueError("region='grow' runs on the staged path: triangulation='scipy', sampling='host' (the fused "
                                 "device-resident kernel keeps the threshold selection)")
            triangulation, sampling = "scipy", "host"
        self.region = region
        # model "ransac": the road model is the RANSAC plane (rescale.py:193, the reference's live line).  "static_tri": the mode of
        # the flat triangles' inverse heights (:194, scale_calculation_static_tri :179-187).  "static": scale_calculator's road
        # model on the selected points, through an inner estimator with its own queue and camera pitch (:195, self.sc :31).  The two
        # commented-out choices run on the staged path only, which they select.  large_frames reaches
        # "static_tri" (its heights come from the large-frame kernel's tri_height / tri_flags rows, of any length), not "static".
        if model not in ("ransac", "static_tri", "static"):
            raise ValueError("model must be 'ransac', 'static_tri' or 'static'")
        if model != "ransac" and not self.model_resident:
            if triangulation not in (None, "scipy") or sampling not in (None, "host"):
                raise ValueError("model=%r runs on the staged path: triangulation='scipy', sampling='host' (the fused "
                                 "device-resident kernel ends in the RANSAC plane)" % model)
            triangulation, sampling = "scipy", "host"
        self.model = model
        # triangulation "scipy": both Delaunay calls on the host, as the reference; "gpu": mvosr_delaunay_batch, everything
        # device-resident.  sampling "host": the triples are drawn here with Python's random, by LIST POSITION in SciPy's row
        # order (replays a recorded reference run); "device": the kernel's counter-based sequence over rows in canonical
        # form (the default — and the only choice — with "gpu").
        # No triangulation given (the reference's own construction, /root/reference/src/main.py:55): the device-resident path
        # (round 5; the reference's RANSAC is unseeded, so no realisation of its draws is THE result — DESIGN.md §3.4 —;
        # MVOSR_TRIANGULATION=scipy restores the host default, and a host `sampler` or sampling="host" implies it).
        if triangulation is None:
            triangulation = "scipy" if (sampler is not None or sampling == "host") else os.environ.get("MVOSR_TRIANGULATION", "gpu")
        if triangulation not in ("scipy", "gpu"):
            raise ValueError("triangulation must be 'scipy' or 'gpu'")
        if sampling is None:
            sampling = "device" if triangulation == "gpu" else "host"
        if sampling not in ("host", "device"):
            raise ValueError("sampling must be 'host' or 'device'")
        if triangulation == "gpu" and sampling == "host":
            raise ValueError("triangulation='gpu' draws its samples on the device (the point list never visits the host)")
        if sampling == "device" and sampler is not None:
            raise ValueError("a host sampler needs sampling='host'; the device path takes id_triples per call")
        if self.model_resident and sampling != "device":
            raise ValueError("model_resident=True belongs to the device-resident path: triangulation='gpu', or triangulation='scipy' "
                             "with sampling='device' (triangulation=%r resolved sampling to %r)" % (triangulation, sampling))
        self.triangulation, self.sampling = triangulation, sampling
        self._fields = _STATIC_FIELDS if self.model_resident else _FIELDS    # a chunk's results, per frame
        self._sampler = sampler
        if self.large_frames and sampling != "device" and region == "threshold" and model == "ransac":
            raise ValueError("large_frames=True belongs to the device-resident path: triangulation='gpu', or triangulation='scipy' "
                             "with sampling='device' (the staged RANSAC path's kernels hold a frame in one workgroup's LDS)")
        # reference attributes (rescale.py:24-35)
        self.absolute_reference = absolute_reference
        self.camera_pitch = 0
        self.scale = 1
        self.inliers = None
        self.scale_queue = deque()
        # (the reference takes any window; mvosr_slew_median_host's ring buffer holds 64 — other windows walk the recurrence in Python,
        # _push_device)
        self.window_size = window_size
        self.vanish = VANISH
        # build-side state
        self.verbose = verbose
        self.delaunay_workers = delaunay_workers
        if delaunay_workers is None or delaunay_workers > 1:
            packing.start_pool(delaunay_workers)     # fork the host stage's workers BEFORE the GPU runtime starts its threads
        self.engine = ScaleEngine(absolute_reference, device=device, camera_pitch=0.0)
        self.ctx = self.engine.ctx
        self._good_bits = good_bits()
        self._rng = random.Random(ransac_seed)
        self.height_level = None
        self.last = {}
        self._seed = int.from_bytes(os.urandom(8), "little") if ransac_seed is None else int(ransac_seed) & ((1 << 64) - 1)
        self._frame_counter = 0                     # frames this estimator has processed: the sample sequence's counter
        self.grow_threshold_angle = 8               # graph.py:40 (rescale.py:33 builds GraphGrow with its default)
        self.stage_outputs = False                  # device path, per-frame calls: keep masks / rows / flags in self.last
        self.last_declined = 0
        if model == "static":                       # rescale.py:31: its own scale_queue, its own camera_pitch = -0.5 deg
            from . import scale_calculator
            self.sc = scale_calculator.ScaleEstimator(absolute_reference, window_size, device=device, delaunay_workers=delaunay_workers,
                                                      verbose=verbose, triangulation="scipy")

    def initial_estimation(self, motion_matrix):
        return 0                                                   # rescale.py:36-38

    # ---- sampling --------------------------------------------------------------------------------
    def _triples(self, m):
        if self._sampler is not None:
            t = np.asarray(self._sampler(m), dtype=np.int32)
        else:                                                      # ransac.py:10, RANSAC_ITERATIONS draws
            t = np.array([self._rng.sample(range(m), 3) for _ in range(self.constants.n_hyp)], dtype=np.int32)
        return np.ascontiguousarray(t.reshape(-1, 3))

    # ---- the three GPU stages over a list of frames ------------------------------------------------
    def _graph_vote(self, pf):
        ctx, lib = self.ctx, self.ctx.lib
        db = DeviceBatch(ctx, pf, with_tri2=False)
        total = ctx.zeros(pf.total_padded, np.int32)
        good = ctx.zeros(pf.total_padded, np.int32)
        status = ctx.zeros(pf.n_frames, np.int32)
        b = db.struct()
        _lib.check(lib.mvosr_graph_inliers_batch(ctx.handle, C.byref(b), C.c_uint32(self._good_bits), total.ptr, good.ptr,
                                                 status.ptr), "mvosr_graph_inliers_batch")
        ctx.sync()
        t, g, st = total.download(), good.download(), status.download()
        for buf in (total, good, status):
            buf.free()
        db.free()
        return t, g, st

    def _vote_masks(self, pf):
        """Per frame of the packed batch the vote's mask (graph.py:34-35) and the launch's status words.  From the tallies of
        mvosr_graph_inliers_batch — or, where ``_staged_large`` says so, from the keep words of mvosr_graph_keep_large_batch
        (``keep > 0`` is the vote itself): the same masks, no limit on the frame."""
        if not self._staged_large(pf.max_feat):
            total, good, st = self._graph_vote(pf)
            with np.errstate(all="ignore"):
                return [(good[pf.frame_slice(f)] / total[pf.frame_slice(f)]) > 0.5 for f in range(pf.n_frames)], st
        ctx = self.ctx
        db = DeviceBatch(ctx, pf, with_tri2=False)
        keep = ctx.zeros(max(pf.total_padded, 1), np.int32)
        status = ctx.zeros(pf.n_frames, np.int32)
        try:
            bs = db.struct()
            _lib.check(ctx.lib.mvosr_graph_keep_large_batch(ctx.handle, C.byref(bs), C.c_uint32(self._good_bits), MIN_VALID_FOR_RETRI, None,
                                                            keep.ptr, None, status.ptr, 0), "mvosr_graph_keep_large_batch")
            ctx.sync()
            words, st = keep.download(), status.download()
        finally:
            keep.free()
            status.free()
            db.free()
        return [words[pf.frame_slice(f)] > 0 for f in range(pf.n_frames)], st

    def _staged_large(self, max_feat):
        """model="static_tri" with large_frames=True: does a staged batch whose largest frame has ``max_feat`` features take the
        large-frame kernels?  (As a whole, like a chunk of the device-resident path; beyond the opt-in limit: refused.)"""
        return self.large_frames and self.model == "static_tri" and chunk_goes_large([max_feat], self._max_points())

    def _flat_selection(self, pf2, static_tri=False):
        """flat_selection (rescale.py:75-102) over the batch: ``(tri_height, tri_flags, height_level, status)``.  ``static_tri``:
        mvosr_static_tri_batch right behind it, in row form on its tri_height / tri_flags and the batch's tri2_off — the heights do
        not visit the host: ``(None, None, height_level, status, results)``."""
        ctx, lib = self.ctx, self.ctx.lib
        db = DeviceBatch(ctx, pf2, with_tri2=True)
        nt = max(int(pf2.tri2_off[-1]), 1)
        tri_h = ctx.zeros(nt, np.float64)
        tri_f = ctx.zeros(nt, np.uint8)
        level = ctx.zeros(pf2.n_frames, np.float64)
        nkept = ctx.zeros(pf2.n_frames, np.int32)
        status = ctx.zeros(pf2.n_frames, np.int32)
        max_tri = int(np.max(np.diff(pf2.tri2_off))) if pf2.n_frames else 0
        b = db.struct()
        if static_tri and self._staged_large(pf2.max_feat):
            # the large-frame kernel writes every row's height and flags, for any number of rows; a RANSAC minimum no list reaches
            # (3 * n_kept is never 2^31 - 1) keeps it from fitting a plane nobody reads: a frame without a refusal reports
            # MVOSR_ST_RS_FEW, which is this stage's 0
            F = pf2.n_frames
            tail = ctx.block([("raw_scale", F, np.float64), ("model", (F, 4), np.float64), ("best_ic", F, np.int32), ("used", F, np.int32)])
            try:
                k = self.constants
                rp = _lib.RescaleParams(self._good_bits, MIN_VALID_FOR_RETRI, k.loose_deg, k.tight_deg, k.height_factor, (1 << 31) - 1, 1,
                                        k.threshold, k.goal_fraction, float(self.absolute_reference), 0, 0)
                o = _lib.RescaleOutputs(tail["raw_scale"].ptr, level.ptr, tail["model"].ptr, tail["best_ic"].ptr, tail["used"].ptr, nkept.ptr,
                                        status.ptr, tri_h.ptr, tri_f.ptr, None)
                _lib.check(lib.mvosr_flat_ransac_large_batch(ctx.handle, C.byref(b), None, C.byref(rp), None, None, None, C.byref(o),
                                                             max(max_tri, 1)), "mvosr_flat_ransac_large_batch")
                ctx.sync()
                st = status.download()
                st[st == K.ST_RS_FEW] = 0
            finally:
                tail.free()
            large_status = st
        else:
            large_status = None
            _lib.check(lib.mvosr_flat_selection_batch(ctx.handle, C.byref(b), *self.constants.selection(), tri_h.ptr, tri_f.ptr, level.ptr,
                                                      nkept.ptr, status.ptr, max_tri), "mvosr_flat_selection_batch")
        if static_tri:                                                                      # rescale.py:194
            try:
                res = self.engine.static_tri_batch(pf2.n_frames, db.bufs["tri2_off"], tri_h, flags=tri_f, min_count=STATIC_TRI_MIN_COUNT,
                                                   absolute_reference=self.absolute_reference)
                return None, None, level.download(), (status.download() if large_status is None else large_status), res
            finally:
                for buf in (tri_h, tri_f, level, nkept, status):
                    buf.free()
                db.free()
        ctx.sync()
        out = tri_h.download(), tri_f.download(), level.download(), status.download()
        for buf in (tri_h, tri_f, level, nkept, status):
            buf.free()
        if self.region == "grow":                                                           # rescale.py:99
            try:
                self.last_grow = graph.launch(ctx, b, pf2.n_frames, nt, max(max_tri, 1), self.grow_threshold_angle, values=True)
            finally:
                db.free()
            return out
        db.free()
        return out

    def _ransac(self, point_lists, triples):
        """point_lists: list of (M,3) arrays (M >= 12 each); triples: list of (H,3) int32, same H."""
        ctx, lib = self.ctx, self.ctx.lib
        F = len(point_lists)
        H = triples[0].shape[0]
        cnt = np.array([p.shape[0] for p in point_lists], dtype=np.int32)
        off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
        allp = np.concatenate(point_lists, axis=0)
        d = {k: ctx.to_device(np.ascontiguousarray(allp[:, i]), np.float64) for i, k in enumerate("xyz")}
        d_off, d_cnt = ctx.to_device(off, np.int64), ctx.to_device(cnt, np.int32)
        d_tri = ctx.to_device(np.ascontiguousarray(np.stack(triples)), np.int32)
        model = ctx.zeros((F, 4), np.float64)
        best = ctx.zeros(F, np.int32)
        used = ctx.zeros(F, np.int32)
        _lib.check(lib.mvosr_ransac_plane_batch(ctx.handle, F, d_off.ptr, d_cnt.ptr, d["x"].ptr, d["y"].ptr, d["z"].ptr,
                                                d_tri.ptr, H, self.constants.threshold, self.constants.goal_fraction, None, model.ptr, best.ptr,
                                                used.ptr), "mvosr_ransac_plane_batch")
        ctx.sync()
        out = model.download(), best.download(), used.download()
        for buf in list(d.values()) + [d_off, d_cnt, d_tri, model, best, used]:
            buf.free()
        return out

    # ---- reference surface ---------------------------------------------------------------------------
    def _second_triangulations(self, feature3ds, feature2ds):
        """rescale.py:115-137 for a list of frames — the vanishing-row filter, the first triangulation, the vote, the second
        triangulation where more than 10 survive: ``(pf2, low3, tris, valids)``."""
        f3s = [np.asarray(a, dtype=np.float64) for a in feature3ds]
        f2s = [np.asarray(a, dtype=np.float64) for a in feature2ds]
        pf = packing.pack_features(f3s, f2s, self.vanish)                                   # :115-117
        packing.attach_tri1(pf, None, self.delaunay_workers)                                # :124
        for f, err in sorted(pf.extra["tri1_errors"].items()):
            raise err
        if self.large_frames and self.model == "static_tri" and pf.n_frames and pf.max_feat > self._large_max_points():
            cnt = np.asarray(pf.feat_cnt)
            f = int(np.argmax(cnt > self._large_max_points()))
            raise self._oversized_error(f, int(cnt[f]), self._large_max_points())
        masks, st = self._vote_masks(pf)
        if np.any(st == 8):
            raise _lib.MvosrLibraryError("triangulation with an out-of-range vertex id")
        low3, low2, tris, valids = [], [], [], []
        for f in range(pf.n_frames):
            valid = masks[f]                                                                # graph.py:34-35,131-132
            valids.append(valid)
            a3, a2 = f3s[f][pf.lower_index[f]], f2s[f][pf.lower_index[f]]
            tri = pf.tri1[pf.tri1_off[f]:pf.tri1_off[f + 1]]
            if self.verbose:
                print('feature rejected ', int(np.sum(~valid)))
                print('feature left     ', int(np.sum(valid)))
            if np.sum(valid) > 10:                                                          # :133-137
                a3, a2 = a3[valid], a2[valid]
                tri = None
            low3.append(a3)
            low2.append(a2)
            tris.append(tri)
        pf2 = packing.pack_features(low3, low2, -np.inf)
        need = [f for f, t in enumerate(tris) if t is None]
        if need:
            new = packing.delaunay_many([low2[f] for f in need], self.delaunay_workers)
            for f, t in zip(need, new):
                if isinstance(t, Exception):
                    raise t
                tris[f] = t
        packing.attach_tri2(pf2, tris, None)
        return pf2, low3, tris, valids

    def feature_selection_batch(self, feature3ds, feature2ds):
        """rescale.py:113-148 for a list of frames: returns a list of (point_selected, heights_loose)."""
        pf2, low3, tris, valids = self._second_triangulations(feature3ds, feature2ds)
        tri_h, tri_f, level, st2 = self._flat_selection(pf2)
        out = []
        for f in range(pf2.n_frames):
            if st2[f] == 7:
                raise np.linalg.LinAlgError("Singular matrix")                              # :79
            t0, t1 = int(pf2.tri2_off[f]), int(pf2.tri2_off[f + 1])
            fl = tri_f[t0:t1]
            if self.region == "grow":
                if self.last_grow["status"][f] == K.ST_ERR_MASK:
                    raise ValueError("region='grow': frame %d has an edge on more than two rows or a row that names a vertex twice" % f)
                keep = self.last_grow["region"][t0:t1] != 0                                    # :99
            else:
                keep = (fl & 4) != 0                                                           # :94-96
            ids = tris[f][keep].reshape(-1)                                                    # :101
            out.append((low3[f][ids], tri_h[t0:t1][(fl & 1) != 0]))                           # :140,:102
            self.height_level = level[f]                                                    # :92
        self.last = {"valid": valids, "tris2": tris, "height_level": level, "pf2": pf2, "tri_flags": tri_f}
        if self.region == "grow":
            self.last["grow"] = self.last_grow
        return out

    def feature_selection(self, feature3d, feature2d):
        return self.feature_selection_batch([feature3d], [feature2d])[0]

    def _apply_scale(self, model):
        """rescale.py:156-178 for one frame, given the RANSAC model (or None when < 12 points)."""
        if model is not None:
            norm = np.array(model[:3], dtype=np.float64)
            h_bar = -model[3]
            if norm[1] < 0:                                                                 # :159-161 (the kernel already did)
                norm, h_bar = -norm, -h_bar
            norm_norm = np.sqrt(norm @ norm) / h_bar                                        # :162-163
            ransac_camera_height = 1 / norm_norm                                            # :165
            scale = self.absolute_reference / ransac_camera_height                          # :167
            slew = self.constants.slew
            if scale - self.scale > slew:                                                   # :169-174
                self.scale += slew
            elif scale - self.scale < -slew:
                self.scale -= slew
            else:
                self.scale = scale
        self.scale_queue.append(self.scale)                                                 # :175-177
        if len(self.scale_queue) > self.window_size:
            self.scale_queue.popleft()

    def scale_calculation_ransac_batch(self, point_lists):
        idx = [i for i, p in enumerate(point_lists) if p.shape[0] >= self.constants.ransac_min_points]   # :152
        models = {}
        if idx:
            triples = [self._triples(point_lists[i].shape[0]) for i in idx]
            h = min(t.shape[0] for t in triples)
            triples = [t[:h] for t in triples]
            m, best, used = self._ransac([np.ascontiguousarray(point_lists[i]) for i in idx], triples)
            for k, i in enumerate(idx):
                models[i] = m[k]
            self.last.update(model=m, best_ic=best, used=used, ransac_frames=idx)
        raw = []
        for i in range(len(point_lists)):
            q_before = list(self.scale_queue)
            self._apply_scale(models.get(i))
            raw.append((self.scale, q_before))
        # np.median(self.scale_queue) per frame (:178) = the window-median kernel over the pushed sequence
        pushed = np.array([r[0] for r in raw], dtype=np.float64)
        filt = self.engine.window_median_host(pushed, self.window_size, raw[0][1]) if raw else np.zeros(0)
        return filt, np.ones(len(point_lists))

    def scale_calculation_ransac(self, point_selected):
        s, e = self.scale_calculation_ransac_batch([np.asarray(point_selected, dtype=np.float64)])
        return s[0], 1

    # ---- the two road models rescale.py:194-195 leave commented out --------------------------------------------
    def _static_tri_carry(self, raw, status, n_frames=None):
        """rescale.py:181-187 over a run of lists, in order: a list with more than 12 heights sets ``self.scale``, any other
        returns it as it stands.  No slew limiter, no window; ``scale_queue`` is not touched."""
        n = len(raw) if n_frames is None else n_frames
        scales = np.empty(n, dtype=np.float64)
        for f in range(n):
            if status[f] == K.ST_ERR_MASK:
                raise ValueError("scale_calculation_static_tri: heights must be finite and positive (list %d)" % f)
            if status[f] != K.ST_RS_FEW:
                self.scale = raw[f]                                                         # :183-184
            scales[f] = self.scale
        return scales

    def scale_calculation_static_tri_batch(self, heights_lists):
        """``scale_calculation_static_tri`` once per list, in order: the packed lists uploaded together, ONE launch of
        mvosr_static_tri_batch, ``self.scale`` carried across the lists of 12 or fewer heights.  Returns ``(scales[F], zeros[F])``."""
        lists = [np.asarray(h, dtype=np.float64).reshape(-1) for h in heights_lists]
        F = len(lists)
        if F == 0:
            return np.zeros(0), np.zeros(0)
        off = np.zeros(F + 1, dtype=np.int64)
        np.cumsum([h.size for h in lists], out=off[1:])
        ctx = self.ctx
        blk = ctx.block([("off", F + 1, np.int64), ("height", max(int(off[-1]), 1), np.float64)])
        try:
            blk.upload({"off": off, "height": np.concatenate(lists) if off[-1] else np.ones(1)})
            r = self.engine.static_tri_batch(F, blk["off"], blk["height"], min_count=STATIC_TRI_MIN_COUNT,
                                             absolute_reference=self.absolute_reference)
        finally:
            blk.free()
        return self._static_tri_carry(r["raw_scale"], r["status"]), np.zeros(F)

    def scale_calculation_static_tri(self, heights):
        """rescale.py:179-187."""
        s, _ = self.scale_calculation_static_tri_batch([heights])
        return s[0], 0

    def _static_tri_frames(self, feature3ds, feature2ds):
        """model="static_tri" (rescale.py:192,194) for a list of frames: the stages of ``feature_selection_batch`` up to
        flat_selection, the road model on its device-resident heights, the carry on the host.  No triples are drawn and no RANSAC
        launch is made; the region (:94-99) does not enter the heights (:102)."""
        pf2, low3, tris, valids = self._second_triangulations(feature3ds, feature2ds)
        _, _, level, st2, r = self._flat_selection(pf2, static_tri=True)
        F = pf2.n_frames
        self.last = {"valid": valids, "tris2": tris, "height_level": level, "pf2": pf2, "scale_norm": r["scale_norm"],
                     "raw_scale": r["raw_scale"], "n_used": r["n_used"], "status": r["status"]}
        singular = np.nonzero(st2 == 7)[0]
        n_ok = int(singular[0]) if len(singular) else F
        scales = self._static_tri_carry(r["raw_scale"], r["status"], n_ok)
        if n_ok:
            self.height_level = level[n_ok - 1]                                             # :92
        if n_ok < F:
            raise np.linalg.LinAlgError("Singular matrix")                                  # :79
        return scales, np.zeros(F)

    def scale_calculation(self, feature3d, feature2d, img=None):
        """rescale.py:191-195."""
        s, e = self.scale_calculation_batch([feature3d], [feature2d], stage=self.stage_outputs)
        return s[0], (0 if self.model == "static_tri" else 1)

    def scale_calculation_batch(self, feature3ds, feature2ds, id_triples=None, stage=False):
        """Equivalent to scale_calculation per frame, in order.  sampling="host": one launch per GPU stage with host
        steps between them.  sampling="device": the batch streams through the device-resident stages in chunks
        (``id_triples``: per frame an (H,3) array of survivor-numbered vertex ids replacing the draw — a recorded
        reference run mapped to point ids; ``stage``: keep the per-frame stage outputs in ``self.last``)."""
        if self.model_resident and id_triples is not None:
            raise ValueError("id_triples belong to the RANSAC model: model='static_tri' draws no samples")
        if self.sampling == "device":
            return self._stream_device(feature3ds, feature2ds, id_triples, stage)
        if id_triples is not None:
            raise ValueError("id_triples belong to sampling='device'")
        if self.model == "static_tri":                                                      # rescale.py:194
            return self._static_tri_frames(feature3ds, feature2ds)
        sel = self.feature_selection_batch(feature3ds, feature2ds)
        if self.model == "static":                                                          # rescale.py:195
            return self.sc.scale_calculation_static_batch([s[0] for s in sel])
        return self.scale_calculation_ransac_batch([s[0] for s in sel])

    # ---- the device-resident path ------------------------------------------------------------------------------
    def _rescale_params(self, frame_base, constants=None):
        k = constants or self.constants
        return _lib.RescaleParams(self._good_bits, MIN_VALID_FOR_RETRI, k.loose_deg, k.tight_deg, k.height_factor, k.ransac_min_points,
                                  k.n_hyp if constants is not None else self.N_HYP, k.threshold, k.goal_fraction,
                                  float(self.absolute_reference), self._seed, int(frame_base))

    def _launch_flat_ransac(self, db, keep_ptr, dt2_ptr, frame_base, frame_ids, id_triples, stage, max_tri, ctx=None, large=False):
        """mvosr_flat_ransac_batch over a DeviceBatch — ``large``: mvosr_flat_ransac_large_batch, same parameters, same results on
        every frame both take —; returns the outputs' block (download queued)."""
        if self.model_resident:
            return self._launch_flat_static(db, keep_ptr, dt2_ptr, stage, max_tri, ctx or self.ctx)
        ctx, F, H = ctx or self.ctx, db.n_frames, self.N_HYP
        spec = [("raw_scale", F, np.float64), ("height_level", F, np.float64), ("model", (F, 4), np.float64),
                ("best_ic", F, np.int32), ("used", F, np.int32), ("n_kept", F, np.int32), ("status", F, np.int32)]
        out = ctx.block(spec)
        side = []
        o = _lib.RescaleOutputs(out["raw_scale"].ptr, out["height_level"].ptr, out["model"].ptr, out["best_ic"].ptr,
                                out["used"].ptr, out["n_kept"].ptr, out["status"].ptr, None, None, None)
        flags = self._flags_block(ctx, db, o, stage)
        d_ids = d_tr = None
        if frame_ids is not None:
            d_ids = ctx.block([("frame_ids", F, np.int64)])
            d_ids.upload({"frame_ids": np.asarray(frame_ids, dtype=np.int64)})
            side.append(d_ids)
        if id_triples is not None:
            t = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.int32).reshape(H, 3) for x in id_triples]))
            d_tr = ctx.block([("id_triples", (F, H, 3), np.int32)])
            d_tr.upload({"id_triples": t})
            side.append(d_tr)
        rp = self._rescale_params(frame_base)
        b = db.struct()
        entry = "mvosr_flat_ransac_large_batch" if large else "mvosr_flat_ransac_batch"
        _lib.check(getattr(ctx.lib, entry)(ctx.handle, C.byref(b), keep_ptr, C.byref(rp),
                                           d_tr["id_triples"].ptr if d_tr is not None else None,
                                           d_ids["frame_ids"].ptr if d_ids is not None else None, dt2_ptr,
                                           C.byref(o), int(max_tri)), entry)
        self._queue_download(out, stage)
        for blk in side:
            blk.mark(True)
        return out, flags, side

    @staticmethod
    def _flags_block(ctx, db, o, stage):
        """With ``stage``: a block for the launch's tri_flags plane, named in its outputs ``o``; else None."""
        if not stage:
            return None
        flags = ctx.block([("tri_flags", max(db.n_rows2, 1), np.uint8)])
        o.tri_flags = flags["tri_flags"].ptr
        return flags

    def _queue_download(self, out, stage):
        """The results reach their page-locked image through a copy KERNEL: a hipMemcpyAsync queued here would park a copy engine behind
        this chunk's kernels, and an upload of the next chunk that lands on that engine waits with it — DeviceBlock.mark_done; the
        per-frame call with stage outputs keeps the queued download."""
        if stage or not self.GPU_SIDE_DOWNLOADS:
            out.prefetch()
        else:
            out.mark_done()
        out.mark(True)

    def _launch_flat_static(self, db, keep_ptr, dt2_ptr, stage, max_tri, ctx):
        """model_resident=True: mvosr_flat_static_tri_batch in mvosr_flat_ransac_batch's place, over the same DeviceBatch, keep words
        and statuses, with its own outputs' block (download queued).  Frame ids, id_triples and seeds do not enter: the road model
        draws nothing."""
        F = db.n_frames
        out = ctx.block([("raw_scale", F, np.float64), ("height_level", F, np.float64), ("scale_norm", F, np.float64),
                         ("n_used", F, np.int32), ("n_kept", F, np.int32), ("status", F, np.int32)])
        o = _lib.StaticTriOutputs(out["scale_norm"].ptr, out["raw_scale"].ptr, out["height_level"].ptr, out["n_used"].ptr,
                                  out["n_kept"].ptr, out["status"].ptr, None, None, None)
        flags = self._flags_block(ctx, db, o, stage)
        k = self.constants
        b = db.struct()
        _lib.check(ctx.lib.mvosr_flat_static_tri_batch(ctx.handle, C.byref(b), keep_ptr, k.loose_deg, k.tight_deg, k.height_factor,
                                                       STATIC_TRI_MIN_COUNT, float(self.absolute_reference), dt2_ptr, None, None,
                                                       C.byref(o), int(max_tri)), "mvosr_flat_static_tri_batch")
        self._queue_download(out, stage)
        return out, flags, []

    def _chunk_dev_gpu(self, f3s, f2s, frame_base, id_triples, stage, tables=False, early_status=False):
        """One chunk, both triangulations on the device: pack (C packer into page-locked memory) -> ONE upload -> every
        launch and the download of the results queued; nothing is waited for here."""
        st = self._chunk_dev_front(f3s, f2s, frame_base, tables, early_status)
        if not st["gpu"]:
            return st
        pf, db = st["pf"], st["db"]
        out, flags, side = self._launch_flat_ransac(db, db.bufs["vote_counters"].ptr, db.bufs["dt2_status"].ptr, frame_base, None, id_triples,
                                                    stage, 2 * int(db.max_feat), large=st["large"])
        if stage or not self.GPU_SIDE_DOWNLOADS:
            db.prefetch_info()
        else:
            db.mark_info_done()
        db.mark()
        return {"gpu": True, "pf": pf, "db": db, "out": out, "flags": flags, "side": side, "large": st["large"]}

    def _chunk_dev_front(self, f3s, f2s, frame_base, tables=False, early_status=False):
        """The stages of a chunk that no constant of ``RescaleConstants`` enters — the pack and its upload, the first
        triangulation, the vote, the second triangulation — launched on the device: ``{"gpu": True, "pf", "db"}`` with the keep
        words in the batch's ``vote_counters`` plane, or ``{"gpu": False}`` where the chunk takes the host's path."""
        ctx, lib = self.ctx, self.ctx.lib
        if tables is False:
            tables = frame_tables(f3s, f2s) if len(f3s) else None
        if tables is not None:
            pf, blk = pack_upload_native(ctx, f3s, f2s, self.vanish, None, tables=tables)             # rescale.py:115-117
            self._trace("packed", -1, len(f3s))
            if pf.max_feat > self._frame_limit():          # (_stream_device cuts the stream before such a frame: a direct caller's)
                blk.free()
                self._refuse_oversized(pf, frame_base)
            db = DeviceBatch(ctx, pf, with_tri2=False, device_triangulation=True, uploaded=blk)
            self._trace("blocks", -1, len(f3s))
        else:
            pf = packing.pack_features(f3s, f2s, self.vanish)
            if pf.n_frames == 0:
                return {"gpu": False}
            if pf.max_feat > self._frame_limit():
                self._refuse_oversized(pf, frame_base)
            db = DeviceBatch(ctx, pf, with_tri2=False, device_triangulation=True)
        large = chunk_goes_large([pf.max_feat], self._max_points())       # (the whole chunk: its small frames give the same bits)
        bufs = db.bufs
        db.info.invalidate()
        try:
            _lib.check(lib.mvosr_delaunay_batch_ex(ctx.handle, db.n_frames, bufs["feat_off"].ptr, bufs["feat_cnt"].ptr, bufs["u"].ptr,
                                                   bufs["v"].ptr, None, int(db.max_feat), bufs["tri_off"].ptr, bufs["tri1"].ptr,
                                                   bufs["tri1_cnt"].ptr, None, bufs["dt1_status"].ptr, None, None, None, None,
                                                   bufs["dt_info"].ptr), "mvosr_delaunay_batch_ex (first triangulation)")
            if early_status:                       # (the call's last chunk: what this kernel declined, known right behind it — _chunk_dev_finish)
                db._queue_early_status()
            bs = db.struct()
            keep = bufs["vote_counters"]                                        # (the block's per-feature int32 plane: here the keep flags)
            self._launch_keep(ctx, bs, bufs["dt1_status"].ptr, keep.ptr, large)                      # graph.py:18-36, rescale.py:133
            _lib.check(lib.mvosr_delaunay_batch_ex(ctx.handle, db.n_frames, bufs["feat_off"].ptr, bufs["feat_cnt"].ptr, bufs["u"].ptr,
                                                   bufs["v"].ptr, keep.ptr, int(db.max_feat), bufs["tri_off"].ptr, bufs["tri2"].ptr,
                                                   bufs["tri2_cnt"].ptr, bufs["n2_expected"].ptr, bufs["dt2_status"].ptr,
                                                   bufs["tri_off"].ptr, bufs["tri1"].ptr, bufs["tri1_cnt"].ptr, bufs["dt_info"].ptr, None),
                       "mvosr_delaunay_batch_ex (second triangulation)")           # rescale.py:134-137
        except _lib.MvosrAllocError:
            # (MVOSR_ERR_ALLOC: the triangulation's workspace could not be allocated; nothing was launched — the host's path)
            db.free()
            self.alloc_fallbacks = getattr(self, "alloc_fallbacks", 0) + 1
            return {"gpu": False}
        db.n_rows2 = 2 * pf.total_padded
        return {"gpu": True, "pf": pf, "db": db, "large": large}

    def _launch_keep(self, ctx, bs, dt1_ptr, keep_ptr, large):
        """The vote with the decision made on the device: mvosr_graph_keep_batch, or (``large``) mvosr_graph_keep_large_batch."""
        if large:
            _lib.check(ctx.lib.mvosr_graph_keep_large_batch(ctx.handle, C.byref(bs), C.c_uint32(self._good_bits), MIN_VALID_FOR_RETRI,
                                                            dt1_ptr, keep_ptr, None, None, 0), "mvosr_graph_keep_large_batch")
        else:
            _lib.check(ctx.lib.mvosr_graph_keep_batch(ctx.handle, C.byref(bs), C.c_uint32(self._good_bits), MIN_VALID_FOR_RETRI,
                                                      dt1_ptr, keep_ptr, None, None), "mvosr_graph_keep_batch")

    def _trace(self, what, chunk, frames):
        """MVOSR_TRACE_CHUNKS=1: (what, chunk, frames, seconds since the call began) into ``self.chunk_trace`` — when this process
        started and finished each chunk's pack + launches and each collection (profiles/e2e_host_trace.py reads it)."""
        tr = getattr(self, "chunk_trace", None)
        if tr is not None:
            tr.append((what, chunk, frames, time.perf_counter() - getattr(self, "_trace_t0", 0.0)))

    def _oversized_error(self, frame, count, limit=None):
        """``limit`` None: the resident kernels' (below); else the opt-in limit of ``large_frames=True``, named in its place.
        flat_selection + RANSAC hold a frame's survivors, heights and flags in ONE workgroup's LDS: a frame beyond that has no
        kernel here (the reference takes any size — /root/reference/src/rescale.py:113-148 — at seconds per frame).  Said with the
        frame named, instead of a library error from the middle of the host path."""
        if limit is not None:
            return ValueError("rescale.ScaleEstimator: frame %d has %d features below the vanishing row; the device-resident path takes at "
                              "most %d per frame with large_frames=True (the triangulation kernels' limit).  Thin the frame, or use "
                              "scale_calculator.ScaleEstimator, whose dense kernels take any size." % (frame, count, limit))
        return ValueError("rescale.ScaleEstimator: frame %d has %d features below the vanishing row; the device-resident path takes at "
                          "most %d per frame (one workgroup's LDS).  Thin the frame, or use scale_calculator.ScaleEstimator, whose "
                          "dense kernels take any size." % (frame, count, self._max_points()))

    def _refuse_oversized(self, pf, frame_base):
        cnt = np.asarray(pf.feat_cnt)
        f = int(np.argmax(cnt > self._frame_limit()))
        raise self._oversized_error(frame_base - self._frame_counter + f, int(cnt[f]), self._frame_limit() if self.large_frames else None)

    def _large_max_points(self):
        """Largest frame ``large_frames=True`` takes: what both triangulators take (mvosr_delaunay_max_points(); the same number
        with triangulation="scipy", sampling="device").  The large-frame kernels themselves have no limit below 2^31 / 3 rows."""
        return packing.delaunay_gpu_max_points()

    def _frame_limit(self):
        """Features below the vanishing row beyond which the streaming paths refuse a frame."""
        return self._large_max_points() if self.large_frames else self._max_points()

    def _below_vanish(self, feature2ds, lens, a, cap):
        """Per frame of ``feature2ds[a:a + len(lens)]`` its features below the vanishing row — counted only where the frame's size
        (an upper bound) exceeds ``cap``; elsewhere the size itself stands in (the frame is small either way)."""
        below = np.asarray(lens, dtype=np.int64).copy()
        for j in np.nonzero(below > cap)[0]:
            f2 = np.asarray(feature2ds[a + int(j)], dtype=np.float64)
            below[j] = int(np.count_nonzero(f2[:, 1] > self.vanish)) if f2.ndim == 2 and f2.size else 0
        return below

    def _first_oversized(self, feature2ds, lens, a):
        """Index (within the call) of the first frame of ``feature2ds[a:a + len(lens)]`` with more features below the vanishing row
        than the device path takes, and that count — or None.  ``lens``: the frames' sizes (an upper bound of that count, so the
        frames are looked at only where a size exceeds the limit: never, in an ordinary call)."""
        cap = self._max_points()
        for j in np.nonzero(np.asarray(lens) > cap)[0]:
            f2 = np.asarray(feature2ds[a + int(j)], dtype=np.float64)
            below = int(np.count_nonzero(f2[:, 1] > self.vanish)) if f2.ndim == 2 and f2.size else 0
            if below > cap:
                return a + int(j), below
        return None

    def _max_points(self):
        """Largest frame the device-resident kernels take (flat_selection + RANSAC hold a frame's survivors, rows'
        heights and flags in one workgroup's LDS).  The LDS term bounds ``flat_plan(dev, n, 2 n, N_HYP).total`` of
        csrc/mvosr_rescale_plan.hpp from above (tests/test_rescale_plan.py)."""
        return min(packing.delaunay_gpu_max_points(), int(self.ctx.lib.mvosr_delaunay_lds_points()),
                   (self.ctx.lds_per_block - 14000 - 36 * self.N_HYP) // 43)

    def _chunk_dev_host(self, f3s, f2s, frame_base, frame_ids, id_triples, stage):
        """The same kernels on the host's triangulations (SciPy's rows in canonical form): triangulation="scipy" with
        sampling="device", and the frames the device triangulation declined.  Synchronous: the steps below, one after the other (``_host_rows2`` takes the two in the middle)."""
        rec = self._host_begin(f3s, f2s, frame_base)
        self._host_flat_start(rec, frame_base, frame_ids, id_triples, stage)
        return self._host_collect(rec, stage)

    # The host path in steps none of which waits for more than its own inputs (round 6: a deferred re-run advances through them while
    # the call's later chunks run, stream.advance): packed + first triangulations started -> (those back) uploaded, the vote
    # launched, its keep words on their way -> (those back) second triangulations started -> (those back) uploaded, flat_selection +
    # RANSAC launched, results on their way -> collected.
    def _host_begin(self, f3s, f2s, frame_base, slot=stream.SLOT_CHUNK, background=False, ctx=None):
        pf = packing.pack_features(f3s, f2s, self.vanish)                                   # rescale.py:115-117
        if pf.n_frames and pf.max_feat > self._frame_limit():
            self._refuse_oversized(pf, frame_base if np.isscalar(frame_base) else self._frame_counter)
        pf.extra["canonical"] = True
        return {"pf": pf, "h1": packing.submit_tri1(pf, self.delaunay_workers, slot=slot, background=background),   # :124
                "ctx": ctx or self.ctx, "large": bool(pf.n_frames) and chunk_goes_large([pf.max_feat], self._max_points())}

    def _host_keep_start(self, rec):
        ctx, lib, pf = rec["ctx"], self.ctx.lib, rec["pf"]
        packing.attach_tri1(pf, rec.pop("h1"), self.delaunay_workers)
        db = DeviceBatch(ctx, pf, with_tri2=False)
        aux = ctx.block([("keep", max(pf.total_padded, 1), np.int32)])
        bs = db.struct()
        self._launch_keep(ctx, bs, None, aux["keep"].ptr, rec.get("large", False))
        aux.mark_done()
        rec.update(db=db, aux=aux)

    def _host_tri2_start(self, rec, slot=stream.SLOT_CHUNK_TRI2, background=False):
        pf = rec["pf"]
        keep = rec["aux"]["keep"].download()
        rec["keep"] = keep
        rec["masks"] = [keep[pf.frame_slice(f)] >= 0 for f in range(pf.n_frames)]
        rec["h2"] = packing.submit_tri2(pf, rec["masks"], self.delaunay_workers, slot=slot, background=background)   # :134-137

    def _host_rows2(self, rec):
        """A record of ``_host_begin`` through the vote and the second triangulations — the steps a re-run that advances on its own
        (``_rerun``) has taken already are not taken again —, their rows attached and on the device; returns the launches' ``max_tri``."""
        if "h1" in rec:
            self._host_keep_start(rec)
        if "h2" not in rec:
            self._host_tri2_start(rec)
        pf, db = rec["pf"], rec["db"]
        packing.attach_tri2(pf, rec.pop("h2"), rec["masks"], self.delaunay_workers)
        db.set_tri2(pf)
        db.n_rows2 = int(pf.tri2_off[-1])
        return max(int(np.max(np.diff(pf.tri2_off))) if pf.n_frames else 0, 1)

    def _host_flat_start(self, rec, frame_base, frame_ids, id_triples, stage):
        max_tri = self._host_rows2(rec)
        rec["out"], rec["flags"], side = self._launch_flat_ransac(rec["db"], rec["aux"]["keep"].ptr, None, frame_base, frame_ids, id_triples,
                                                                  stage, max_tri, ctx=rec["ctx"], large=rec.get("large", False))
        rec["side"] = side + [rec["aux"]]
        return max_tri

    @staticmethod
    def _host_errors(pf):
        """A host chunk's errors by frame: the second triangulations', and over them the first triangulations'."""
        return {**pf.extra["tri2_errors"], **pf.extra["tri1_errors"]}

    def _host_collect(self, rec, stage):
        pf = rec["pf"]
        host_errors = self._host_errors(pf)
        res = self._collect(rec["out"], pf.n_frames)
        st = {"pf": pf, "db": rec["db"], "out": rec["out"], "flags": rec["flags"], "side": rec["side"], "host_errors": host_errors, "keep": rec["keep"]}
        if stage:
            res["stage"] = self._stage_outputs(st, host=True)
        stream.free_blocks(st)
        res["host_errors"] = host_errors
        return res

    @staticmethod
    def _collect(out, F):
        return {k: out[k].download() for k in (_FIELDS if "model" in out.views else _STATIC_FIELDS)}

    def _stage_outputs(self, st, host=False):
        """Per frame: the vote's mask (graph.py:35), the second triangulation's rows and flat_selection's flags."""
        pf, db = st["pf"], st["db"]
        F = pf.n_frames
        fl = st["flags"]["tri_flags"].download()
        if host:
            keep = st["keep"]
            rows = [pf.tri2[pf.tri2_off[f]:pf.tri2_off[f + 1]] for f in range(F)]
            flags = [fl[pf.tri2_off[f]:pf.tri2_off[f + 1]] for f in range(F)]
        else:
            keep = db.bufs["vote_counters"].download()
            tri2, cnt2 = db.bufs["tri2"].download(), db.bufs["tri2_cnt"].download()
            toff = 2 * np.asarray(pf.feat_off, dtype=np.int64)
            rows = [tri2[toff[f]:toff[f] + cnt2[f]] for f in range(F)]
            flags = [fl[toff[f]:toff[f] + cnt2[f]] for f in range(F)]
        return {"valid": [keep[pf.frame_slice(f)] > 0 for f in range(F)], "tris2": rows, "tri_flags": flags}

    def _chunk_dev_finish(self, st, f3s, f2s, frame_base, id_triples, stage, defer=None):
        """Results of a chunk started by ``_chunk_dev_gpu``; frames whose triangulation the device declined (degenerate point
        sets, fewer than 3 points) are redone on the host's triangulations with their own sample counters — at once, or, with
        ``defer`` (the call's re-run records; streamed batches), after the call's last chunk (``stream.finish_all``): the re-run is
        waited for, and between the chunks that wait drained the pipeline (80 declined frames in 16 384: 529 -> 93 k frames/s in the
        sibling estimator's fixed mode, scale_calculator._chunk_gpu_finish)."""
        if not st["gpu"]:
            return self._chunk_dev_host(f3s, f2s, frame_base, None, id_triples, stage)
        db = st["db"]
        if defer is not None and not stage and self.GPU_REDO_EARLY:
            # the call's LAST chunk: the frames its first triangulation declined are known behind that kernel.  This thread has nothing
            # else to do: it takes them through their first triangulation (waited for — the chunk's other kernels are running), the
            # vote (on the re-runs' context) and the start of their second triangulation now; the call's end launches the rest
            s1e = db.early_status()
            if s1e is not None and s1e.any() and int(np.count_nonzero(s1e)) <= self.GPU_REDO_EARLY_MAX:
                ef = np.nonzero(s1e != 0)[0]
                early = st["early"] = self._rerun(None, ef, f3s, f2s, frame_base, id_triples, (stream.SLOT_EARLY, stream.SLOT_EARLY_TRI2))
                self._host_keep_start(early.rec)
                self._host_tri2_start(early.rec, slot=stream.SLOT_EARLY_TRI2, background=True)
                early.step = 2
                self.redo_early_status_hits = getattr(self, "redo_early_status_hits", 0) + 1
        stream.advance_while(defer or (), lambda: not (st["out"].ready() and db.info.ready()))
        res = self._collect(st["out"], len(f3s))
        s1, s2 = db.triangulation_status()
        redo = np.nonzero((s1 != 0) | (s2 != 0))[0]
        self.last_declined += len(redo)
        if stage:
            res["stage"] = self._stage_outputs(st)
        early = st.pop("early", None)
        stream.free_blocks(st)
        res["host_errors"] = {}
        if early is not None:
            if len(redo) == len(early.redo) and np.array_equal(redo, early.redo):
                early.res = res
                defer.append(early)                 # (continues where the early steps left it)
                return res
            stream.free_blocks(early.rec)           # (more frames than the early read knew of: the merged way)
        if len(redo) and defer is not None:
            started = self.GPU_REDO_EARLY and not stage and len(redo) <= self.GPU_REDO_EARLY_MAX and len(defer) < self.GPU_REDO_MAX_DEFERRED
            # (a few frames: their re-run starts now — first triangulations on the pool — and advances while later chunks run)
            defer.append(self._rerun(res, redo, f3s, f2s, frame_base, id_triples, (stream.SLOT_DEFER + len(defer), stream.SLOT_DEFER_TRI2 + len(defer)) if started else None))
            self.redo_early_started = getattr(self, "redo_early_started", 0) + int(started)
            stream.advance(defer)
            return res
        stream.advance(defer or ())
        if len(redo):
            sub = self._chunk_dev_host([f3s[f] for f in redo], [f2s[f] for f in redo], 0, frame_base + redo,
                                       None if id_triples is None else [id_triples[f] for f in redo], stage)
            self._scatter(res, redo, sub, 0, stage)
        return res

    def _scatter(self, res, frames, sub, first, stage):
        stream.scatter(res, frames, sub, self._fields, "host_errors", first)
        if stage:
            for k in ("valid", "tris2", "tri_flags"):
                for j, f in enumerate(frames):
                    res["stage"][k][f] = sub["stage"][k][first + j]

    def _rerun(self, res, redo, f3s, f2s, frame_base, id_triples, slots=None):
        """The re-run record of a chunk's frames ``redo``.  ``slots`` (the pool slots of its two triangulations): started now — its first
        triangulations go to the pool, and stream.advance / stream.finish_all take it through the _host_* steps, launching on the
        re-runs' own context; else it waits for the call's merged re-run (``_merged_rerun``)."""
        r = stream.Rerun(res, redo, lambda: None, f3s=f3s, f2s=f2s, frame_base=frame_base, id_triples=id_triples)
        if slots is None:
            return r
        rec = r.rec = self._host_begin([f3s[f] for f in redo], [f2s[f] for f in redo], 0, slot=slots[0], background=True,
                                       ctx=self._redo_context())
        rec["ids"] = frame_base + redo
        rec["triples"] = None if id_triples is None else [id_triples[f] for f in redo]

        def flat(wait):
            self._host_flat_start(rec, 0, rec["ids"], rec["triples"], False)
            if not wait:
                self.redo_early_launched = getattr(self, "redo_early_launched", 0) + 1
        r.chain = [(lambda: rec["h1"].ready(), lambda wait: self._host_keep_start(rec)),
                   (lambda: rec["aux"].ready(), lambda wait: self._host_tri2_start(rec, slot=slots[1], background=not wait)),
                   (lambda: rec["h2"].ready(), flat)]
        r.collect, r.begun = (lambda: self._host_collect(rec, False)), True
        r.free = lambda: (stream.free_blocks(rec), stream.wait_out(rec.get("h1"), rec.get("h2")))
        return r

    def _finish_reruns(self, records, stage):
        """The call's re-runs after its last chunk: the started ones finish their steps, the others' frames go in one batch."""
        stream.finish_all(records, lambda rest: self._merged_rerun(rest, stage), self._fields, "host_errors")

    def _merged_rerun(self, records, stage):
        """The frames of the records whose re-run was not started, in ONE batch through the host's triangulations, scattered back."""
        at = [(r, f) for r in records for f in r.redo]
        sub = self._chunk_dev_host([r.f3s[f] for r, f in at], [r.f2s[f] for r, f in at], 0, np.array([r.frame_base + int(f) for r, f in at], dtype=np.int64),
                                   None if records[0].id_triples is None else [r.id_triples[f] for r, f in at], stage)
        first = 0
        for r in records:
            self._scatter(r.res, r.redo, sub, first, stage)
            first += len(r.redo)

    def _stream_run_gpu(self, feature3ds, feature2ds, ra, rb, base, triples, stage, n_collected):
        """Frames ``ra:rb`` of a call streamed through the device in chunks (``stream.plan`` / ``stream.run``): the whole call in the
        default construction, one size class of it with ``large_frames=True``.  ``(bounds within the call, results, found)`` —
        ``found``: (frame of the call, count) of the oversized frame the stream stopped before (default construction only: with
        large_frames the call was cut beforehand), or None."""
        whole = (ra, rb) == (0, len(feature3ds))
        f3r, f2r = (feature3ds, feature2ds) if whole else (feature3ds[ra:rb], feature2ds[ra:rb])
        F = rb - ra
        C, ramp = stream.chunk_size(F, self.GPU_CHUNK, self.GPU_MIN_CHUNK, self.GPU_CHUNK_POINTS, [len(x) for x in f3r[:64]],
                                    self.GPU_RAMP_FRACTIONS if self.GPU_RAMP else ())
        found = []

        def stop(a, lens):                     # (the stream ends before the first oversized frame)
            o = self._first_oversized(f2r, lens, a)
            if o is not None:
                found.append(o)
                return o[0]
        deferred = []
        collected = iter(range(n_collected, n_collected + F))

        def start(a, b, tables, k):
            self._trace("launch", k, b - a)
            st = self._chunk_dev_gpu(f3r[a:b], f2r[a:b], base + ra + a, triples(ra + a, ra + b), stage, tables=tables,
                                     early_status=self.GPU_REDO_EARLY and not stage and b == (found[0][0] if found else F) and a > 0)
            self._trace("launched", k, b - a)
            return st

        def collect(st, a, b, last):
            self._trace("collect", next(collected), b - a)
            return self._chunk_dev_finish(st, f3r[a:b], f2r[a:b], base + ra + a, triples(ra + a, ra + b), stage, defer=deferred)
        chunks = stream.plan(F, stream.tables_of(f3r, f2r), C, ramp, self.GPU_CHUNK_POINTS, self._resident_frames,
                             None if self.large_frames else stop)
        bounds, _, results = stream.run(chunks, start, collect, self.GPU_PIPELINE, stream.free_blocks, deferred,
                                        lambda: self._finish_reruns(deferred, stage))
        return [(ra + a, ra + b) for a, b in bounds], results, ((ra + found[0][0], found[0][1]) if found else None)

    def _stream_device(self, feature3ds, feature2ds, id_triples, stage, push=True):
        F = len(feature3ds)
        if F == 0:
            return np.zeros(0), np.zeros(0)
        base = self._frame_counter
        self.last_declined = 0
        # A frame the device path has no kernel for (_oversized_error) ends the run like every other error (_push_device): the frames
        # before it go through the slew limiter, the window and the sample counter, nothing queued is dropped, then the exception —
        # what the reference's per-frame loop would have left behind.
        oversized = None
        limit = None
        # large_frames=True: the call is cut into size classes instead (size_class_runs) — runs of frames the resident kernels take
        # and runs beyond them, each streamed on its own, the large runs' chunks through the large-frame kernels — and ends before
        # the first frame beyond the opt-in limit
        runs = None
        if self.large_frames:
            limit = self._frame_limit()
            below = self._below_vanish(feature2ds, [len(x) for x in feature2ds], 0, self._max_points())
            runs, stop_at = size_class_runs(below, self._max_points(), limit)
            if stop_at is not None:
                oversized, F = (stop_at, int(below[stop_at])), stop_at
        elif self.triangulation != "gpu":
            oversized = self._first_oversized(feature2ds, [len(x) for x in feature2ds], 0)
            if oversized is not None:
                F = oversized[0]
        if runs is None:
            runs = [(0, F, False)] if F else []
        triples = lambda a, b: None if id_triples is None else id_triples[a:b]
        bounds, results = [], []
        if self.triangulation == "gpu":
            self.chunk_trace = [] if os.environ.get("MVOSR_TRACE_CHUNKS") else None
            self._trace_t0 = time.perf_counter()
            for ra, rb, _ in runs:                   # (the default construction: ONE run, the whole call)
                rbounds, rresults, found = self._stream_run_gpu(feature3ds, feature2ds, ra, rb, base, triples, stage, len(results))
                bounds += rbounds
                results += rresults
                if found is not None:
                    oversized, F = found, found[0]
        else:
            for ra, rb, large in runs:
                for a, b in host_chunks([len(x) for x in feature2ds[ra:rb]], 2048, self.GPU_CHUNK_POINTS if large else None):
                    bounds.append((ra + a, ra + b))  # (the runs end before the first oversized frame)
                    results.append(self._chunk_dev_host(feature3ds[ra + a:ra + b], feature2ds[ra + a:ra + b], base + ra + a, None,
                                                        triples(ra + a, ra + b), stage))
        if oversized is not None and not results:
            raise self._oversized_error(*oversized, limit)
        cat, host_errors = stream.concat(bounds, results, self._fields, "host_errors")
        self.last = dict(zip(self._fields, cat))
        raw, status, level = self.last["raw_scale"], self.last["status"], self.last["height_level"]
        if stage:
            for k in ("valid", "tris2", "tri_flags"):
                self.last[k] = [x for r in results for x in r["stage"][k]]
        if oversized is not None:
            host_errors = dict(host_errors)
            host_errors[F] = self._oversized_error(*oversized, limit)
            raw = np.concatenate([raw, [np.nan]])
            status = np.concatenate([status, np.array([K.ST_ERR_EMPTY], dtype=status.dtype)])
            level = np.concatenate([level, [np.nan]])
        if not push:
            if oversized is not None:
                raise host_errors[F]
            return raw, status, level, host_errors
        if self.model_resident:
            return self._push_static(raw, status, level, host_errors)
        return self._push_device(raw, status, level, host_errors)

    # ---- the two halves on their own: what a driver that shards a sequence over GPUs needs (offline.run_sequence_sharded) ----
    def raw_scale_batch(self, feature3ds, feature2ds, frame_base=0):
        """Per-frame half only (no cross-frame state touched): ``(raw_scale[F], status[F], height_level[F], host_errors)``.
        ``frame_base``: position of the block's first frame in the whole sequence — the sample sequence is keyed by the
        frame's position, so a sequence split over ranks draws the triples the single-process run draws."""
        if self.sampling != "device":
            raise ValueError("the sharded driver needs the device sample sequence: ScaleEstimator(..., triangulation='gpu') "
                             "or (..., sampling='device')")
        if len(feature3ds) == 0:
            return np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(0), {}
        keep, self._frame_counter = self._frame_counter, self._frame_counter + int(frame_base)
        try:
            return self._stream_device(feature3ds, feature2ds, None, False, push=False)
        finally:
            self._frame_counter = keep

    # ---- C runs of a sequence at once: the per-frame half (mvosr_flat_ransac_cases_batch; RepeatedRuns carries the tails) ----
    _CASE_FIELDS = ("raw_scale", "model", "best_ic", "used", "status")

    def _launch_cases(self, db, keep_ptr, dt2_ptr, flags_ptr, seeds, frame_base, frame_ids, id_triples, max_tri, opts, ctx=None):
        """mvosr_flat_ransac_cases_batch behind the chunk's mvosr_flat_ransac_batch, on the same resident batch, keep words and
        flags; returns the outputs' block (download queued) and the side blocks."""
        ctx, F, H, Cn = ctx or self.ctx, db.n_frames, (opts["constants"].n_hyp if opts.get("constants") else self.N_HYP), len(seeds)
        spec = [("raw_scale", (F, Cn), np.float64), ("model", (F, Cn, 4), np.float64), ("best_ic", (F, Cn), np.int32),
                ("used", (F, Cn), np.int32), ("status", (F, Cn), np.int32), ("count_form", F, np.int32)]
        if opts.get("hyp_counts"):
            spec.append(("hyp_counts", (F, Cn, H), np.int32))
        out = ctx.block(spec)
        side = ctx.block([("seeds", Cn, np.uint64)] + ([("frame_ids", F, np.int64)] if frame_ids is not None else []) +
                         ([("id_triples", (F, Cn, H, 3), np.int32)] if id_triples is not None else []))
        up = {"seeds": np.asarray(seeds, dtype=np.uint64)}
        if frame_ids is not None:
            up["frame_ids"] = np.asarray(frame_ids, dtype=np.int64)
        if id_triples is not None:
            up["id_triples"] = np.ascontiguousarray(np.asarray(id_triples, dtype=np.int32).reshape(F, Cn, H, 3))
        side.upload(up)
        o = _lib.RescaleCasesOutputs(out["raw_scale"].ptr, out["model"].ptr, out["best_ic"].ptr, out["used"].ptr, out["status"].ptr,
                                     out["hyp_counts"].ptr if "hyp_counts" in out else None, out["count_form"].ptr)
        rp = self._rescale_params(frame_base, opts.get("constants"))
        b = db.struct()
        _lib.check(ctx.lib.mvosr_flat_ransac_cases_batch(ctx.handle, C.byref(b), keep_ptr, C.byref(rp), side["seeds"].ptr, Cn,
                                                         int(opts.get("cases_per_group", 0)),
                                                         side["id_triples"].ptr if id_triples is not None else None,
                                                         side["frame_ids"].ptr if frame_ids is not None else None, dt2_ptr, flags_ptr,
                                                         C.byref(o), int(max_tri)), "mvosr_flat_ransac_cases_batch")
        out.prefetch()
        return out, side

    @staticmethod
    def _collect_cases(res, out):
        """A chunk's case outputs next to its per-frame results.  The cases kernel does not recompute the heights: a frame the
        flat selection refuses as a whole (singular row, bad vertex id, no rows) is refused for every case here."""
        for k in out.views:
            res["case_" + k] = out[k].download()
        case = lambda *keys: [res["case_" + k] for k in keys]
        ScaleEstimator._merge_refused(res["status"], case("raw_scale", "model"), case("best_ic", "used", "count_form"), case("status"))
        return res

    @staticmethod
    def _merge_refused(status, nan=(), zero=(), take=()):
        """The frames whose ``status`` refuses them as a whole, in case arrays with the frames on their first axis: NaN in those of
        ``nan``, 0 in those of ``zero``, the frame's status in every case of those of ``take``."""
        bad = np.isin(status, _REFUSED)
        if bad.any():
            for a in nan:
                a[bad] = np.nan
            for a in zero:
                a[bad] = 0
            for a in take:
                a[bad] = status[bad].reshape((-1,) + (1,) * (a.ndim - 1))

    def _cases_host(self, f3s, f2s, seeds, frame_base, frame_ids, id_triples, opts):
        """One chunk of the cases path on the host's triangulations: triangulation="scipy" with sampling="device", and the frames
        both device triangulations declined (``frame_ids``: their own sample counters)."""
        rec = self._host_begin(f3s, f2s, frame_base)
        try:
            max_tri = self._host_flat_start(rec, frame_base, frame_ids, None, True)
            cases, side = self._launch_cases(rec["db"], rec["aux"]["keep"].ptr, None, rec["flags"]["tri_flags"].ptr, seeds, frame_base,
                                             frame_ids, id_triples, max_tri, opts, ctx=rec["ctx"])
            rec["side"] += [side, cases]
            res = self._collect_cases(self._collect(rec["out"], rec["pf"].n_frames), cases)
            res["host_errors"] = self._host_errors(rec["pf"])
            return res
        finally:
            stream.wait_out(rec.get("h1"), rec.get("h2"))     # (a pool job must not write into a freed slot)
            stream.free_blocks(rec)

    def _rerun_declined(self, res, s1, s2, f3s, f2s, host_chunk):
        """The frames of a chunk that a device triangulation declined (``s1``, ``s2``: their statuses) through the host's, counted in
        ``last_declined``: ``host_chunk(f3s, f2s, redo)`` runs them — ``redo``: their positions in the chunk, for their own sample
        counters — and its results, errors included, are scattered into the chunk's ``res``."""
        res["host_errors"] = {}
        redo = np.nonzero((s1 != 0) | (s2 != 0))[0]
        self.last_declined += len(redo)
        if len(redo):
            sub = host_chunk([f3s[f] for f in redo], [f2s[f] for f in redo], redo)
            stream.scatter(res, redo, sub, [k for k in sub if k != "host_errors"], "host_errors")
        return res

    def _cases_chunks(self, f3s, f2s, fields, start, finish):
        """The chunk pipeline of the repeated runs and of ``ConstantSweep``: an oversized frame refused up front, then chunks of one
        size through ``stream.run`` — with triangulation="gpu" ``start(a, b)`` packs, uploads and launches a chunk before
        ``finish(state, a, b)`` waits for the results of the one before it; else ``finish`` gets ``{"gpu": False}`` and runs the chunk on
        the host's triangulations.  Returns the chunks' ``fields`` concatenated and ``host_errors`` keyed by frame of the call."""
        over = self._first_oversized(f2s, [len(x) for x in f2s], 0)
        if over is not None:
            raise self._oversized_error(*over)
        self.last_declined = 0
        F, gpu = len(f3s), self.triangulation == "gpu"
        step = stream.chunk_size(F, self.GPU_CHUNK, self.GPU_MIN_CHUNK, self.GPU_CHUNK_POINTS, [len(x) for x in f3s[:64]])[0] if gpu else 2048
        bounds, _, results = stream.run(stream.fixed_plan(F, step), lambda a, b, tables, k: start(a, b) if gpu else {"gpu": False},
                                        lambda st, a, b, last: finish(st, a, b), int(gpu), stream.free_blocks, [], lambda: None)
        cat, host_errors = stream.concat(bounds, results, fields, "host_errors")
        return dict(zip(fields, cat), host_errors=host_errors)

    def _cases_gpu_start(self, f3s, f2s, seeds, frame_base, id_triples, opts):
        st = self._chunk_dev_gpu(f3s, f2s, frame_base, None, True)
        if st["gpu"]:
            db = st["db"]
            try:
                db.mark(False)
                st["cases"], side = self._launch_cases(db, db.bufs["vote_counters"].ptr, db.bufs["dt2_status"].ptr, st["flags"]["tri_flags"].ptr,
                                                       seeds, frame_base, None, id_triples, 2 * int(db.max_feat), opts)
                st["side"] += [side, st["cases"]]        # (the state's blocks: stream.free_blocks releases them with the rest)
                db.mark()
            except Exception:
                stream.free_blocks(st)
                raise
        return st

    def _cases_gpu_finish(self, st, f3s, f2s, seeds, frame_base, id_triples, opts):
        if not st["gpu"]:
            return self._cases_host(f3s, f2s, seeds, frame_base, None, id_triples, opts)
        res = self._collect_cases(self._collect(st["out"], len(f3s)), st["cases"])
        s1, s2 = st["db"].triangulation_status()
        stream.free_blocks(st)                       # (the results are on the host; when a step above raises, stream.run frees the state)
        return self._rerun_declined(res, s1, s2, f3s, f2s, lambda g3, g2, redo: self._cases_host(
            g3, g2, seeds, 0, frame_base + redo, None if id_triples is None else [id_triples[f] for f in redo], opts))

    def raw_scale_cases_batch(self, feature3ds, feature2ds, seeds, frame_base=0, id_triples=None, cases_per_group=0, hyp_counts=False):
        """The per-frame half for ``C = len(seeds)`` sample sequences of the same frames at once (no cross-frame state touched): both
        triangulations, the vote and the flat selection run ONCE per frame, chunk by chunk through the device-resident stages, and
        behind each chunk's mvosr_flat_ransac_batch one launch of mvosr_flat_ransac_cases_batch fits all cases on the same resident
        batch.  Case ``c`` is, bit for bit, what an estimator built with ``ransac_seed=seeds[c]`` computes for these frames.

        ``id_triples``: per frame a ``(C, H, 3)`` array of survivor-numbered vertex ids replacing the draws.  ``frame_base`` as in
        ``raw_scale_batch``.  Returns a dict: ``raw_scale``, ``best_ic``, ``used``, ``status`` ``(C, F)``, ``model`` ``(C, F, 4)``, the
        per-frame ``height_level``, ``n_kept``, ``frame_status`` and ``count_form`` ``(F,)``, ``host_errors`` (frame -> exception),
        and ``hyp_counts`` ``(C, F, H)`` when asked for.  Chunks are started one ahead of the one being collected; frames that both
        device triangulations decline are re-run on the host's at once.  An oversized frame is refused up front."""
        if self.sampling != "device":
            raise ValueError("the repeated runs need the device sample sequence: ScaleEstimator(..., triangulation='gpu') or "
                             "(..., sampling='device')")
        seeds = [int(s) & ((1 << 64) - 1) for s in seeds]
        Cn, F, H = len(seeds), len(feature3ds), self.N_HYP
        if Cn < 1:
            raise ValueError("raw_scale_cases_batch: at least one seed")
        opts = {"cases_per_group": int(cases_per_group), "hyp_counts": bool(hyp_counts)}
        empty = {"raw_scale": np.zeros((Cn, 0)), "model": np.zeros((Cn, 0, 4)), "best_ic": np.zeros((Cn, 0), np.int32),
                 "used": np.zeros((Cn, 0), np.int32), "status": np.zeros((Cn, 0), np.int32), "height_level": np.zeros(0),
                 "n_kept": np.zeros(0, np.int32), "frame_status": np.zeros(0, np.int32), "count_form": np.zeros(0, np.int32), "host_errors": {}}
        if F == 0:
            return empty
        base = self._frame_counter + int(frame_base)
        chunk = lambda a, b: (feature3ds[a:b], feature2ds[a:b], seeds, base + a, None if id_triples is None else id_triples[a:b], opts)
        cases = self._CASE_FIELDS + (("hyp_counts",) if hyp_counts else ())
        r = self._cases_chunks(feature3ds, feature2ds, ["case_" + k for k in cases] + ["height_level", "n_kept", "status", "case_count_form"],
                               lambda a, b: self._cases_gpu_start(*chunk(a, b)), lambda st, a, b: self._cases_gpu_finish(st, *chunk(a, b)))
        out = {k: np.ascontiguousarray(np.moveaxis(r["case_" + k], 1, 0)) for k in cases}
        out.update(height_level=r["height_level"], n_kept=r["n_kept"], frame_status=r["status"], count_form=r["case_count_form"],
                   host_errors=r["host_errors"])
        return out

    def push_raw_scales(self, raw, status, level=None, host_errors=None):
        """Cross-frame half (slew limiter, window median, raise sites) for raw scales computed elsewhere (other ranks):
        returns ``(scales, stds)`` like ``scale_calculation_batch``."""
        raw = np.asarray(raw, dtype=np.float64)
        status = np.asarray(status, dtype=np.int32)
        level = np.full(len(raw), np.nan) if level is None else np.asarray(level, dtype=np.float64)
        if self.model == "static_tri":
            return self._push_static(raw, status, level, host_errors or {})
        return self._push_device(raw, status, level, host_errors or {})

    def _push_static(self, raw, status, level, host_errors):
        """The cross-frame tail of model="static_tri" (rescale.py:181-187, ``_static_tri_carry``) over the frames before the first one
        at which the reference raises; then that frame's exception, as ``_push_device`` raises it.  No slew limiter, no window:
        ``scale_queue`` is not touched.  Returns ``(scales, zeros)``."""
        F = len(raw)
        bad = np.isin(status, _REFUSED)
        for f in host_errors:
            bad[f] = True
        n_ok = int(np.argmax(bad)) if bad.any() else F
        scales = self._static_tri_carry(raw, status, n_ok)
        if n_ok:
            self.height_level = level[n_ok - 1]                                             # :92
        self._frame_counter += n_ok + (1 if n_ok < F else 0)
        if n_ok < F:
            if n_ok in host_errors and isinstance(host_errors[n_ok], Exception):
                raise host_errors[n_ok]
            if status[n_ok] == K.ST_ERR_SINGULAR:
                raise np.linalg.LinAlgError("Singular matrix (frame %d of the batch)" % n_ok)  # :79
            if status[n_ok] == K.ST_ERR_MASK:
                raise _lib.MvosrLibraryError("triangulation with an out-of-range vertex id (frame %d of the batch)" % n_ok)
            raise ValueError("frame %d of the batch has no triangles below the vanishing row" % n_ok)
        return scales, np.zeros(F)

    def _push_device(self, raw, status, level, host_errors):
        """The cross-frame tail (rescale.py:169-178) on the device over the frames before the first one at which the
        reference raises; then that frame's exception."""
        F = len(raw)
        bad = np.isin(status, _REFUSED)
        for f in host_errors:
            bad[f] = True
        n_ok = int(np.argmax(bad)) if bad.any() else F
        ctx = self.ctx
        filtered = np.zeros(0)
        if n_ok:
            # (the recurrence is sequential and the raw scales are on the host already — the statuses decide where the
            # reference raises —: one core walks it in C, mvosr_slew_median_host; mvosr_slew_median is the same on device arrays)
            r = np.ascontiguousarray(raw[:n_ok], dtype=np.float64)
            ap = np.ascontiguousarray(status[:n_ok] == 0, dtype=np.int32)
            pushed, filtered = np.empty(n_ok, np.float64), np.empty(n_ok, np.float64)
            q = np.ascontiguousarray(np.asarray(list(self.scale_queue), dtype=np.float64))
            if 1 <= int(self.window_size) <= 64 and q.size <= 64:
                _lib.check(ctx.lib.mvosr_slew_median_host(_lib.addr(r), _lib.addr(ap), n_ok, self.constants.slew, float(self.scale), int(self.window_size),
                                                          _lib.addr(q) if q.size else None, int(q.size), _lib.addr(pushed),
                                                          _lib.addr(filtered), None), "mvosr_slew_median_host")
                self.scale = float(pushed[-1])                                              # :169-174
                tail = list(self.scale_queue) + list(pushed[max(0, n_ok - self.window_size):])
                self.scale_queue.clear()
                self.scale_queue.extend(tail[-self.window_size:])                           # :175-177
            else:
                # a window the C loop's ring buffer does not hold (the reference takes any: 0 gives the median of an empty deque,
                # nan): the same recurrence, frame by frame, as the reference writes it (:169-178)
                slew = self.constants.slew
                with np.errstate(all="ignore"):
                    for i in range(n_ok):
                        if ap[i]:
                            if r[i] - self.scale > slew:
                                self.scale += slew
                            elif r[i] - self.scale < -slew:
                                self.scale -= slew
                            else:
                                self.scale = float(r[i])
                        self.scale_queue.append(self.scale)
                        if len(self.scale_queue) > self.window_size:
                            self.scale_queue.popleft()
                        pushed[i] = self.scale
                        import warnings
                        with warnings.catch_warnings():
                            warnings.simplefilter("ignore")
                            filtered[i] = np.median(self.scale_queue)
            self.height_level = level[n_ok - 1]                                             # :92
        self._frame_counter += n_ok + (1 if n_ok < F else 0)
        if n_ok < F:
            if n_ok in host_errors and isinstance(host_errors[n_ok], Exception):
                raise host_errors[n_ok]
            if status[n_ok] == K.ST_ERR_SINGULAR:
                raise np.linalg.LinAlgError("Singular matrix (frame %d of the batch)" % n_ok)  # :79
            if status[n_ok] == K.ST_ERR_MASK:
                raise _lib.MvosrLibraryError("triangulation with an out-of-range vertex id (frame %d of the batch)" % n_ok)
            raise ValueError("frame %d of the batch has no triangles below the vanishing row" % n_ok)
        return filtered, np.ones(F)


# ---- the repeated offline runs (/root/reference/test_off_line.sh:4-16) ------------------------------------------------------
_MASK64 = (1 << 64) - 1
CASE_SEED_STEP = 0xA0761D6478BD642F


def _mix64(x):
    """splitmix64's finaliser, as mvosr_flat_ransac_batch's sample sequence uses it (include/mvosr.h)."""
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


def case_seeds(seed, cases):
    """The case seeds ``RepeatedRuns(seed=...)`` derives: ``seed_c = mix64((seed + c * 0xA0761D6478BD642F) mod 2^64)``,
    ``c = 0 .. cases - 1`` — counter-based, so case c does not depend on how many cases run beside it."""
    return [_mix64((int(seed) + c * CASE_SEED_STEP) & _MASK64) for c in range(int(cases))]


class _CaseTail:
    """One case's cross-frame state — the running scale and the scale queue of rescale.py:24-35 — behind the estimator's own tail
    (``ScaleEstimator._push_device``: mvosr_slew_median_host once per call, the raise sites)."""
    push = ScaleEstimator._push_device

    def __init__(self, ctx, window_size, constants=None):
        self.ctx, self.window_size, self.constants = ctx, window_size, constants or RescaleConstants()
        self.scale, self.scale_queue = 1, deque()                                           # rescale.py:28,30
        self.height_level, self._frame_counter = None, 0
        self.prev = (0, 100)                                                                # main_offline.py:46-47


def _trim_scale_figures(figs):
    """``evaluate.trimmed_mean`` over the cases of each figure of ``evaluate.scale_errors``."""
    from . import evaluate
    cols = lambda a: np.array([evaluate.trimmed_mean(a[:, k]) for k in range(a.shape[1])])
    return {"mean": evaluate.trimmed_mean(figs["mean"]), "max": evaluate.trimmed_mean(figs["max"]),
            "within": cols(figs["within"]), "drift": cols(figs["drift"])}


class RepeatedRuns:
    """``cases`` runs of a sequence at once: what /root/reference/test_off_line.sh:4-16 gets from ten processes of main_offline.py
    on one saved dict (its RANSAC is unseeded, ransac.py:6, so the runs differ).  One inner ``ScaleEstimator`` in a device-sampling
    mode does the deterministic stages once per frame and the RANSAC of every case in one launch per chunk
    (``raw_scale_cases_batch``); every case has its own tail — running scale and scale queue from the reference's initial state.

    ``seeds``: the case seeds; else ``case_seeds(seed, cases)``; else drawn from the OS.  Row c of ``run`` equals
    ``offline.run_sequence_batched`` with ``ScaleEstimator(ransac_seed=seeds[c])``.  A second ``run`` continues the sequence: the
    frame counter, every tail and the "previous scale" of the too-few-features rule carry over.

    A frame beyond the resident kernels' limit (``ScaleEstimator._max_points()``) is refused up front with the estimator's message,
    also where the inner estimator is built with ``large_frames=True``: the cases kernel holds a frame in one workgroup's LDS."""

    def __init__(self, absolute_reference, window_size=5, cases=10, seeds=None, seed=None, **estimator_kw):
        if seeds is not None:
            self.seeds = [int(s) & _MASK64 for s in seeds]
        elif seed is not None:
            self.seeds = case_seeds(seed, cases)
        else:
            self.seeds = [int.from_bytes(os.urandom(8), "little") for _ in range(int(cases))]
        if not self.seeds:
            raise ValueError("RepeatedRuns: at least one case")
        self.cases = len(self.seeds)
        if estimator_kw.get("model", "ransac") != "ransac":
            raise ValueError("RepeatedRuns repeats the RANSAC model: model=%r draws no samples to repeat" % (estimator_kw["model"],))
        self.estimator = self._make_estimator(absolute_reference, window_size, estimator_kw)
        if getattr(self.estimator, "model", "ransac") != "ransac":
            raise ValueError("RepeatedRuns repeats the RANSAC model, not model=%r" % (self.estimator.model,))
        if self.estimator.sampling != "device":
            raise ValueError("RepeatedRuns needs a device-sampling mode: triangulation='gpu', or triangulation='scipy' with sampling='device'")
        self.tails = [_CaseTail(self.estimator.ctx, window_size) for _ in range(self.cases)]
        for tail in self.tails:                          # (the slew limiter's step: the estimator's)
            tail.constants = getattr(self.estimator, "constants", None) or RescaleConstants()
        self._scales, self._motions, self._raw, self.last = [], [], [], {}

    @staticmethod
    def _make_estimator(absolute_reference, window_size, kw):
        return ScaleEstimator(absolute_reference, window_size, ransac_seed=0, **kw)

    def run(self, data, id_triples=None, minimum_feature_for_scale=None):
        """``main_offline``'s loop over the dict for every case: the not-moving skip, the ``N > 100`` gate and repeat-previous
        (offline.plan_sequence / assemble_outputs).  ``id_triples``: ``(C, processed frames, H, 3)`` vertex ids replacing the draws.
        Returns ``scales`` ``(C, n)`` — each row shaped like main_offline's scales file —, ``error`` ``(C, n + 1)``, ``kinds`` and the
        per-case ``raw_scale`` / ``status`` of the processed frames."""
        from . import offline
        kinds = offline.plan_sequence(data, offline.MINIMUM_FEATURE_FOR_SCALE if minimum_feature_for_scale is None else minimum_feature_for_scale)
        idx = [i for i, k in enumerate(kinds) if k == 1]
        f3 = [np.asarray(data["feature3ds"][i], dtype=np.float64) for i in idx]
        f2 = [np.asarray(data["feature2ds"][i], dtype=np.float64) for i in idx]
        per_frame = None
        if id_triples is not None:
            t = np.asarray(id_triples, dtype=np.int32)
            per_frame = [np.ascontiguousarray(t[:, f]) for f in range(len(idx))]
        est = self.estimator
        r = est.raw_scale_cases_batch(f3, f2, self.seeds, id_triples=per_frame)
        Fp = len(idx)
        scales, errors, first_exc = [], [], None
        for c, tail in enumerate(self.tails):
            try:
                filt, std = tail.push(r["raw_scale"][c], r["status"][c], r["height_level"], r["host_errors"]) if Fp else (np.zeros(0), np.zeros(0))
            except Exception as exc:                     # (a frame at which the reference raises: every tail has pushed the frames before it)
                first_exc = first_exc or exc
                continue
            s, e = self._assemble(kinds, list(filt), list(std), tail.prev)
            tail.prev = (s[-1], e[-1])
            scales.append(s[1:])
            errors.append(e)
        est._frame_counter = self.tails[0]._frame_counter if Fp else est._frame_counter
        if first_exc is not None:
            raise first_exc
        out = {"scales": np.array(scales, dtype=np.float64).reshape(self.cases, len(kinds)), "error": np.array(errors, dtype=np.float64),
               "kinds": kinds, "raw_scale": r["raw_scale"], "status": r["status"]}
        self._scales.append(out["scales"])
        self._raw.append(r["raw_scale"])
        self._motions.append(np.array(data["motions"], dtype=np.float64).reshape(len(kinds), -1))
        self.last = dict(r, **out)
        return out

    @staticmethod
    def _assemble(kinds, est_scales, est_stds, prev):
        """offline.assemble_outputs, with a leading run of too-few-features frames repeating what the previous ``run`` left (the
        initial entries 0 / 100 in the first)."""
        from . import offline
        scales, error = offline.assemble_outputs(kinds, est_scales, est_stds)
        scales[0], error[0] = prev
        for i, k in enumerate(kinds):
            if k != 2:
                break
            scales[i + 1], error[i + 1] = prev
        return scales, error

    def scales(self):
        """``(C, n)`` over every frame run so far."""
        return np.concatenate(self._scales, axis=1) if self._scales else np.zeros((self.cases, 0))

    def paths(self, data=None, on_device=False):
        """The C integrated trajectories (offline.get_path, main_offline.py:92): of ``data`` — run first when given —, else of
        everything run so far.  ``on_device``: integrated by mvosr_paths_batch (offline.get_path_batch) instead of the host loop."""
        from . import offline
        if data is not None:
            scales, motions = self.run(data)["scales"], np.array(data["motions"], dtype=np.float64).reshape(len(data["move_flags"]), -1)
        else:
            scales, motions = self.scales(), (np.concatenate(self._motions) if self._motions else np.zeros((0, 12)))
        if on_device:
            return list(offline.get_path_batch(motions, scales, ctx=self.estimator.ctx))
        return [offline.get_path(motions, scales[c]) for c in range(self.cases)]

    def scores(self, poses_gt, speed_gt=None):
        """What /root/reference/test_off_line.sh:11-23 computes from the runs' paths, on the device (evaluate.Scorer): the dict of
        ``evaluate.repeat_scores(poses_gt, self.paths())`` for everything run so far, from the scales and motions kept here — the
        paths never leave the device.  ``speed_gt`` (one value or one per frame, script/calculate_speed.py's file): adds
        ``"speed_scaled"``, the same dict for the paths re-scaled to that speed (script/change_scale.py).  The reference re-scales
        ONE path — the last case's, through the loop variable its first loop leaves behind (test_off_line.sh:18) — and prints its
        score; here every case is re-scaled and scored, row C - 1 being the reference's.  The ground truth's segment table is
        kept for the next call with the same ``poses_gt``."""
        from . import _lib, evaluate
        ctx = self.estimator.ctx
        scorer = self._scorer_for(poses_gt)
        motions = np.concatenate(self._motions) if self._motions else np.zeros((0, 12))
        d_paths = scorer._paths_on_device(motions, self.scales())
        out = scorer.score_paths(d_paths)
        if speed_gt is not None:
            C, n = self.cases, motions.shape[0]
            speed = np.asarray(speed_gt, dtype=np.float64)
            speed = np.full(n, float(speed)) if speed.ndim == 0 else speed
            if speed.shape != (n,):
                raise ValueError("scores: %d speeds for %d motions (change_scale.py:15 broadcasts one per frame)" % (speed.size, n))
            d_speed, d_motions, d_status = ctx.to_device(speed), ctx.empty((C, n, 12), np.float64), ctx.empty(C, np.int32)
            _lib.check(ctx.lib.mvosr_pose2motion_batch(ctx.handle, C, n, d_paths.ptr, d_speed.ptr, d_motions.ptr, None, d_status.ptr),
                       "mvosr_pose2motion_batch")
            _lib.check(ctx.lib.mvosr_paths_batch(ctx.handle, n, C, d_motions.ptr, n * 12, None, d_paths.ptr), "mvosr_paths_batch")
            evaluate._raise_status(d_status.download(), "scores")
            out["speed_scaled"] = scorer.score_paths(d_paths)
        return out

    def _scorer_for(self, poses_gt):
        """The evaluate.Scorer of ``poses_gt``, kept for the next call with the same ground truth."""
        from . import evaluate
        gt = np.ascontiguousarray(np.asarray(poses_gt, dtype=np.float64).reshape(-1, 12))
        cached = getattr(self, "_scorer", None)
        if cached is None or not np.array_equal(cached[0], gt):
            cached = self._scorer = (gt, evaluate.Scorer(gt, ctx=self.estimator.ctx))
        return cached[1]

    def scale_scores(self, speed_gt, poses_gt=None, filter_window=None):
        """What /root/reference/tesh.sh:4-8 computes from every case's scales file, on the device: ``"scales"``, the figures of
        ``evaluate.scale_errors(speed_gt, self.scales())`` (script/evaluate_scale.py:4-13) for everything run so far.
        ``filter_window``: adds ``"filtered"``, the same figures for the scales after evaluate_scale.py's running median
        (``evaluate.filter_scales``).  ``poses_gt``: adds ``"gt_rescaled"`` (and ``"gt_rescaled_filtered"``), the ground truth's own
        path re-scaled to every case's scales and scored against itself (``Scorer.score_gt_rescaled``, tesh.sh:6-8).
        ``"trimmed"`` holds, per set of figures, the ``evaluate.trimmed_mean`` of each over the cases, as :meth:`scores` has it for
        the path errors.  The tails assemble the scales on the host; they are uploaded once and every launch — errors, median,
        re-scaling, integration, scoring — reads them or their filtered copy on the device."""
        from . import evaluate
        ctx = self.estimator.ctx
        scales = self.scales()
        n = scales.shape[1]
        gt = np.asarray(speed_gt, dtype=np.float64).reshape(-1)
        if n > gt.size:
            raise ValueError("operands could not be broadcast together with shapes (%d,) (%d,) (evaluate_scale.py:6: more scales "
                             "than ground-truth speeds)" % (gt.size, n))
        d_gt, d_s = ctx.to_device(gt[:n]), ctx.to_device(scales)
        scorer = self._scorer_for(poses_gt) if poses_gt is not None else None
        out = {"scales": evaluate.scale_errors(d_gt, d_s, ctx=ctx)}
        if scorer is not None:
            out["gt_rescaled"] = scorer.score_gt_rescaled(d_s)
        if filter_window is not None:
            d_f = evaluate.filter_scales(d_s, filter_window, ctx=ctx, on_device=True)
            out["filtered"] = evaluate.scale_errors(d_gt, d_f, ctx=ctx)
            if scorer is not None:
                out["gt_rescaled_filtered"] = scorer.score_gt_rescaled(d_f)

        out["trimmed"] = {k: _trim_scale_figures(out[k]) for k in ("scales", "filtered") if k in out}
        return out

    def write_results(self, res_addr, tag):
        """``<res_addr>scales.txt<tag><num>`` and ``<res_addr>path.txt<tag><num>``, num = 0 .. C - 1: the files main_offline.py:90-93
        leaves under test_off_line.sh's tags ``$1$num``.  Returns the file names."""
        from . import offline
        scales, motions = self.scales(), (np.concatenate(self._motions) if self._motions else np.zeros((0, 12)))
        names = []
        for c in range(self.cases):
            offline.save_outputs(res_addr, "%s%d" % (tag, c), scales[c], motions)
            names += [res_addr + "scales.txt%s%d" % (tag, c), res_addr + "path.txt%s%d" % (tag, c)]
        return names

    def spread(self):
        """Per-frame mean and standard deviation over the cases: of the filtered scale over every frame run so far (``scale_mean``,
        ``scale_std``) and of the raw scale over the processed frames (``raw_mean``, ``raw_std``; a case without a fit is left out)."""
        s = self.scales()
        raw = np.concatenate(self._raw, axis=1) if self._raw else np.zeros((self.cases, 0))
        import warnings
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            return {"scale_mean": s.mean(axis=0), "scale_std": s.std(axis=0), "raw_mean": np.nanmean(raw, axis=0), "raw_std": np.nanstd(raw, axis=0)}


# ---- the estimator's constants swept over a sequence in one run -------------------------------------------------
class _SweepEstimator(ScaleEstimator):
    """The inner estimator of ``ConstantSweep``: a frame must also fit flat_selection_sweep_kernel's LDS
    (csrc/mvosr_rescale_sweep_plan.hpp: 48 bytes per feature with two rows per feature, the tables, the histograms' floor)."""

    def _max_points(self):
        return min(ScaleEstimator._max_points(self), (self.ctx.lds_per_block - 1024) // 48)


def _stack_dicts(dicts):
    """A list of equally shaped (nested) dicts of arrays and numbers -> one dict with a leading axis; an int keeps its value."""
    out = {}
    for k, v in dicts[0].items():
        if isinstance(v, dict):
            out[k] = _stack_dicts([d[k] for d in dicts])
        elif isinstance(v, (int, np.integer)) and not isinstance(v, bool):
            out[k] = v
        else:
            out[k] = np.array([d[k] for d in dicts])
    return out


class ConstantSweep:
    """``RepeatedRuns`` for K settings of ``RescaleConstants`` at once: what one gets today by patching the literals and running
    the ten cases again per setting.  Both triangulations and the vote do not read the constants and run once per frame; the
    selection of every distinct ``(loose_deg, tight_deg, height_factor)`` comes from one launch of
    mvosr_flat_selection_sweep_batch per chunk, the plane fits of every distinct (selection, RANSAC constants) pair from one
    launch of mvosr_flat_ransac_cases_batch on that selection's flag plane, all cases in it; ``slew`` and ``window_size`` live in
    the tails, one per (config, case), and cost no launch.

    ``configs``: a list of ``RescaleConstants`` (``ConstantSweep.grid`` builds a product).  Seeds as in ``RepeatedRuns``; every
    config runs the same case seeds.  Row ``[k, c]`` of ``run`` equals, bit for bit, row c of
    ``RepeatedRuns(absolute_reference, window_size, seeds=seeds, constants=configs[k]).run(data)``.  A frame must fit the kernels
    of every config and the sweep kernel (``estimator._max_points()``) — ``large_frames=True`` does not change that limit or its
    message."""

    MAX_SCORED_CASES = 32768                # rows of one scoring call (the scorers take 65535 cases a launch)

    def __init__(self, absolute_reference, configs, window_size=5, cases=10, seed=None, seeds=None, **estimator_kw):
        self.configs = list(configs)
        if not self.configs or not all(isinstance(k, RescaleConstants) for k in self.configs):
            raise ValueError("ConstantSweep: configs is a non-empty list of RescaleConstants")
        if estimator_kw.get("model", "ransac") != "ransac":
            raise ValueError("ConstantSweep sweeps the RANSAC model: model=%r has no RANSAC constants to sweep" % (estimator_kw["model"],))
        if "constants" in estimator_kw:
            raise TypeError("ConstantSweep takes its constants as configs")
        if seeds is not None:
            self.seeds = [int(s) & _MASK64 for s in seeds]
        elif seed is not None:
            self.seeds = case_seeds(seed, cases)
        else:
            self.seeds = [int.from_bytes(os.urandom(8), "little") for _ in range(int(cases))]
        if not self.seeds:
            raise ValueError("ConstantSweep: at least one case")
        self.cases, self.window_size = len(self.seeds), window_size
        # the distinct selections, the distinct (selection, RANSAC) pairs, and which pair a config reads
        self._sels, self._pairs, self._pair_of = [], [], []
        for k in self.configs:
            if k.selection() not in self._sels:
                self._sels.append(k.selection())
            pair = (self._sels.index(k.selection()), k.ransac())
            if pair not in self._pairs:
                self._pairs.append(pair)
            self._pair_of.append(self._pairs.index(pair))
        self._pair_constants = [RescaleConstants(*self._sels[si], *rk) for si, rk in self._pairs]
        widest = RescaleConstants(n_hyp=max(k.n_hyp for k in self.configs))      # (sizes the largest frame: every config's kernels take it)
        self.estimator = _SweepEstimator(absolute_reference, window_size, ransac_seed=0, constants=widest, **estimator_kw)
        if self.estimator.sampling != "device":
            raise ValueError("ConstantSweep needs a device-sampling mode: triangulation='gpu', or triangulation='scipy' with sampling='device'")
        self.max_settings = int(self.estimator.ctx.lib.mvosr_flat_selection_sweep_max_settings())
        self.tails = [[_CaseTail(self.estimator.ctx, window_size, k) for _ in range(self.cases)] for k in self.configs]
        self._scales, self._motions, self._raw, self.last = [], [], [], {}
        self.launches = {"sweep": 0, "cases": 0}                 # launches made so far, by kernel
        self._rr = None

    @staticmethod
    def grid(**axes):
        """The product of the given values per field, the last named field varying fastest:
        ``grid(loose_deg=[-80, -75], n_hyp=[100, 30])`` -> four ``RescaleConstants``; fields not named keep their defaults."""
        names = list(axes)
        known = {f.name for f in dataclasses.fields(RescaleConstants)}
        for n in names:
            if n not in known:
                raise TypeError("ConstantSweep.grid: RescaleConstants has no field %r" % n)
        values = [list(np.atleast_1d(axes[n]).tolist()) if not isinstance(axes[n], (list, tuple)) else list(axes[n]) for n in names]
        return [RescaleConstants(**dict(zip(names, combo))) for combo in itertools.product(*values)]

    # ---- a chunk: the launches behind the second triangulation ---------------------------------------------------------------
    def _launch(self, st, keep_ptr, dt2_ptr, max_tri, frame_base, frame_ids, ctx=None):
        """mvosr_flat_selection_sweep_batch over the distinct selections (16 a launch), then mvosr_flat_ransac_cases_batch once
        per distinct pair on its selection's plane; the outputs' downloads queued.  Every block joins the state's ``side`` list the
        moment it exists (``stream.free_blocks`` releases them); ``st["launch"]`` names the outputs for ``_collect``."""
        est, db = self.estimator, st["db"]
        ctx, F, S = ctx or est.ctx, db.n_frames, len(self._sels)
        stride = max(int(db.n_rows2), 1)                             # rows of a flag plane
        flags = ctx.block([("tri_flags", (S, stride), np.uint8)])
        side = st["side"] = [flags]
        groups, cases = [], []
        b = db.struct()
        for g0 in range(0, S, self.max_settings):
            sel = self._sels[g0:g0 + self.max_settings]
            out = ctx.block([("height_level", (F, len(sel)), np.float64), ("n_kept", (F, len(sel)), np.int32), ("status", F, np.int32)])
            side.append(out)
            loose, tight, factor = (np.array([x[i] for x in sel], dtype=np.float64) for i in range(3))
            _lib.check(ctx.lib.mvosr_flat_selection_sweep_batch(ctx.handle, C.byref(b), keep_ptr, dt2_ptr, len(sel), _lib.addr(loose),
                                                                _lib.addr(tight), _lib.addr(factor), flags["tri_flags"].ptr + g0 * stride,
                                                                out["height_level"].ptr, out["n_kept"].ptr, out["status"].ptr, None,
                                                                int(max_tri)), "mvosr_flat_selection_sweep_batch")
            self.launches["sweep"] += 1
            out.prefetch()
            groups.append(out)
        for (si, _), k in zip(self._pairs, self._pair_constants):
            out, inputs = est._launch_cases(db, keep_ptr, dt2_ptr, flags["tri_flags"].ptr + si * stride, self.seeds, frame_base, frame_ids,
                                           None, max_tri, {"constants": k}, ctx=ctx)
            self.launches["cases"] += 1
            side += [out, inputs]
            cases.append(out)
        st["launch"] = {"groups": groups, "cases": cases}

    @staticmethod
    def _collect(lp):
        """A chunk's results, frames first: the sweep launch's geometry status merged into every case as
        ``ScaleEstimator._collect_cases`` merges mvosr_flat_ransac_batch's."""
        groups, cases = lp["groups"], lp["cases"]
        res = {"status": np.array(groups[0]["status"].download(), copy=True),
               "height_level": np.concatenate([g["height_level"].download() for g in groups], axis=1),
               "n_kept": np.concatenate([g["n_kept"].download() for g in groups], axis=1),
               "case_raw_scale": np.stack([c["raw_scale"].download() for c in cases], axis=1),          # (F, P, C)
               "case_status": np.stack([c["status"].download() for c in cases], axis=1)}
        ScaleEstimator._merge_refused(res["status"], nan=[res["case_raw_scale"]], take=[res["case_status"]])
        return res

    def _chunk_host(self, f3s, f2s, frame_base, frame_ids):
        """One chunk on the host's triangulations: triangulation="scipy" with sampling="device", and the frames both device
        triangulations declined (``frame_ids``: their own sample counters)."""
        est = self.estimator
        rec = est._host_begin(f3s, f2s, frame_base)
        try:
            max_tri = est._host_rows2(rec)
            self._launch(rec, rec["aux"]["keep"].ptr, None, max_tri, frame_base, frame_ids, ctx=rec["ctx"])
            res = self._collect(rec["launch"])
            res["host_errors"] = est._host_errors(rec["pf"])
            return res
        finally:
            stream.wait_out(rec.get("h1"), rec.get("h2"))
            stream.free_blocks(rec)

    def _gpu_start(self, f3s, f2s, frame_base):
        st = self.estimator._chunk_dev_front(f3s, f2s, frame_base)
        if st["gpu"]:
            db = st["db"]
            try:
                self._launch(st, db.bufs["vote_counters"].ptr, db.bufs["dt2_status"].ptr, 2 * int(db.max_feat), frame_base, None)
                db.prefetch_info()
                db.mark()
            except Exception:
                stream.free_blocks(st)
                raise
        return st

    def _gpu_finish(self, st, f3s, f2s, frame_base):
        if not st["gpu"]:
            return self._chunk_host(f3s, f2s, frame_base, None)
        res = self._collect(st["launch"])
        s1, s2 = st["db"].triangulation_status()
        stream.free_blocks(st)                           # (the results are on the host; when a step above raises, stream.run frees the state)
        # both device triangulations declined: the host's, with the frames' own counters
        return self.estimator._rerun_declined(res, s1, s2, f3s, f2s, lambda g3, g2, redo: self._chunk_host(g3, g2, 0, frame_base + redo))

    def _raw_cases(self, f3, f2):
        """The per-frame half for every pair and case (no cross-frame state touched): ``raw_scale`` / ``status`` ``(P, C, F)``,
        ``height_level`` / ``n_kept`` ``(S, F)``, ``frame_status`` ``(F,)``, ``host_errors``.  Chunks as in
        ``ScaleEstimator.raw_scale_cases_batch``: started one ahead of the one being collected."""
        est = self.estimator
        F, P, S, Cn = len(f3), len(self._pairs), len(self._sels), self.cases
        if F == 0:
            return {"raw_scale": np.zeros((P, Cn, 0)), "status": np.zeros((P, Cn, 0), np.int32), "height_level": np.zeros((S, 0)),
                    "n_kept": np.zeros((S, 0), np.int32), "frame_status": np.zeros(0, np.int32), "host_errors": {}}
        base = est._frame_counter
        chunk = lambda a, b: (f3[a:b], f2[a:b], base + a)
        r = est._cases_chunks(f3, f2, ["case_raw_scale", "case_status", "height_level", "n_kept", "status"],
                              lambda a, b: self._gpu_start(*chunk(a, b)), lambda st, a, b: self._gpu_finish(st, *chunk(a, b)))
        return {"raw_scale": np.ascontiguousarray(np.moveaxis(r["case_raw_scale"], 0, 2)),
                "status": np.ascontiguousarray(np.moveaxis(r["case_status"], 0, 2)),
                "height_level": np.ascontiguousarray(r["height_level"].T), "n_kept": np.ascontiguousarray(r["n_kept"].T),
                "frame_status": r["status"], "host_errors": r["host_errors"]}

    # ---- the sequence -----------------------------------------------------------------------------------------------------------
    def run(self, data, minimum_feature_for_scale=None):
        """``RepeatedRuns.run`` for every config: ``scales`` ``(K, C, n)``, ``error`` ``(K, C, n + 1)``, ``kinds``, and the
        ``raw_scale`` / ``status`` ``(K, C, F)`` of the processed frames.  A second ``run`` continues the sequence."""
        from . import offline
        kinds = offline.plan_sequence(data, offline.MINIMUM_FEATURE_FOR_SCALE if minimum_feature_for_scale is None else minimum_feature_for_scale)
        idx = [i for i, k in enumerate(kinds) if k == 1]
        f3 = [np.asarray(data["feature3ds"][i], dtype=np.float64) for i in idx]
        f2 = [np.asarray(data["feature2ds"][i], dtype=np.float64) for i in idx]
        est = self.estimator
        r = self._raw_cases(f3, f2)
        Fp, Kn, Cn = len(idx), len(self.configs), self.cases
        scales, errors, first_exc = [], [], None
        for k, tails in enumerate(self.tails):
            p, si = self._pair_of[k], self._pairs[self._pair_of[k]][0]
            for c, tail in enumerate(tails):
                try:
                    filt, std = (tail.push(r["raw_scale"][p, c], r["status"][p, c], r["height_level"][si], r["host_errors"]) if Fp
                                 else (np.zeros(0), np.zeros(0)))
                except Exception as exc:                 # (a frame at which the reference raises: every tail has pushed the frames before it)
                    first_exc = first_exc or exc
                    continue
                s, e = RepeatedRuns._assemble(kinds, list(filt), list(std), tail.prev)
                tail.prev = (s[-1], e[-1])
                scales.append(s[1:])
                errors.append(e)
        est._frame_counter = self.tails[0][0]._frame_counter if Fp else est._frame_counter
        if first_exc is not None:
            raise first_exc
        take = np.asarray(self._pair_of)
        out = {"scales": np.array(scales, dtype=np.float64).reshape(Kn, Cn, len(kinds)),
               "error": np.array(errors, dtype=np.float64).reshape(Kn, Cn, len(kinds) + 1), "kinds": kinds,
               "raw_scale": r["raw_scale"][take], "status": r["status"][take]}
        self._scales.append(out["scales"])
        self._raw.append(out["raw_scale"])
        self._motions.append(np.array(data["motions"], dtype=np.float64).reshape(len(kinds), -1))
        self.last = dict(r, **out)
        return out

    def scales(self):
        """``(K, C, n)`` over every frame run so far."""
        return np.concatenate(self._scales, axis=2) if self._scales else np.zeros((len(self.configs), self.cases, 0))

    def _motions_all(self):
        return np.concatenate(self._motions) if self._motions else np.zeros((0, 12))

    # ---- scoring: the existing device scorers on the stacked (K C, n) scales ------------------------------------------------------
    def _stacked_runs(self):
        """Per group of configs ``(k0, k1, rr)``: a ``RepeatedRuns`` whose cases are the group's (config, case) rows."""
        rr = self._rr
        if rr is None:
            rr = self._rr = object.__new__(RepeatedRuns)
            rr.estimator = self.estimator
        scales = self.scales()
        per = max(1, self.MAX_SCORED_CASES // self.cases)
        for k0 in range(0, len(self.configs), per):
            k1 = min(len(self.configs), k0 + per)
            rr.cases = (k1 - k0) * self.cases
            rr._scales, rr._motions = [scales[k0:k1].reshape(rr.cases, -1)], self._motions
            yield k0, k1, rr

    def _config_rows(self, j):
        return slice(j * self.cases, (j + 1) * self.cases)

    def scores(self, poses_gt, speed_gt=None):
        """``RepeatedRuns.scores`` per config, with a leading K axis on every entry: the paths of all (config, case) rows are
        integrated and scored together by the device scorer; ``"trimmed"`` is ``evaluate.trimmed_mean`` over each config's cases."""
        from . import evaluate
        if self.cases < 3:
            raise ValueError("trimmed_mean: at least three values (the best and the worst are dropped), got %d" % self.cases)
        per = []
        for k0, k1, rr in self._stacked_runs():
            d = rr.scores(poses_gt, speed_gt)
            for j in range(k1 - k0):
                sl = self._config_rows(j)
                one = evaluate._reduce_scores(np.ascontiguousarray(d["tra"][sl]), np.ascontiguousarray(d["rot"][sl]))
                if "speed_scaled" in d:
                    one["speed_scaled"] = evaluate._reduce_scores(np.ascontiguousarray(d["speed_scaled"]["tra"][sl]),
                                                                  np.ascontiguousarray(d["speed_scaled"]["rot"][sl]))
                per.append(one)
        self.last_scores = _stack_dicts(per)
        return self.last_scores

    def scale_scores(self, speed_gt, poses_gt=None, filter_window=None):
        """``RepeatedRuns.scale_scores`` per config, with a leading K axis on every entry."""
        from . import evaluate
        if self.cases < 3:
            raise ValueError("trimmed_mean: at least three values (the best and the worst are dropped), got %d" % self.cases)
        per = []
        for k0, k1, rr in self._stacked_runs():
            d = rr.scale_scores(speed_gt, poses_gt=poses_gt, filter_window=filter_window)
            for j in range(k1 - k0):
                sl = self._config_rows(j)
                one = {}
                for key in ("scales", "filtered"):
                    if key in d:
                        one[key] = {f: (v if f == "n" else np.ascontiguousarray(v[sl])) for f, v in d[key].items()}
                for key in ("gt_rescaled", "gt_rescaled_filtered"):
                    if key in d:
                        one[key] = evaluate._reduce_scores(np.ascontiguousarray(d[key]["tra"][sl]), np.ascontiguousarray(d[key]["rot"][sl]))
                one["trimmed"] = {key: _trim_scale_figures(one[key]) for key in ("scales", "filtered") if key in one}
                per.append(one)
        self.last_scale_scores = _stack_dicts(per)
        return self.last_scale_scores

    FIGURES = ("tra_mean", "rot_mean", "scale_mean", "scale_max")

    def _figure(self, figure):
        """Per config the trimmed mean over its cases of ``figure``: the path errors' two means from the last ``scores``, the
        scale error's mean and maximum from the last ``scale_scores``."""
        if figure in ("tra_mean", "rot_mean"):
            if getattr(self, "last_scores", None) is None:
                raise ValueError("ConstantSweep: %r comes from scores(); call it first" % figure)
            return np.asarray(self.last_scores["trimmed"][figure], dtype=np.float64)
        if figure in ("scale_mean", "scale_max"):
            if getattr(self, "last_scale_scores", None) is None:
                raise ValueError("ConstantSweep: %r comes from scale_scores(); call it first" % figure)
            return np.asarray(self.last_scale_scores["trimmed"]["scales"][figure[6:]], dtype=np.float64)
        raise ValueError("ConstantSweep: figure is one of %s" % ", ".join(self.FIGURES))

    def table(self, figure="tra_mean"):
        """One row per config: its index, its fields and the trimmed mean of ``figure`` over its cases."""
        v = self._figure(figure)
        return [dict(dataclasses.asdict(k), config=i, **{figure: float(v[i])}) for i, k in enumerate(self.configs)]

    def best(self, figure="tra_mean"):
        """The config with the smallest trimmed mean of ``figure`` (the first of equals; a NaN never wins)."""
        v = self._figure(figure)
        if np.isnan(v).all():
            raise ValueError("ConstantSweep.best: every config's %s is NaN" % figure)
        return self.configs[int(np.nanargmin(v))]

    def write_results(self, res_addr, tag):
        """``RepeatedRuns.write_results`` per config under the tags ``<tag>k<k>_<num>``.  Returns the file names."""
        from . import offline
        scales, motions = self.scales(), self._motions_all()
        names = []
        for k in range(len(self.configs)):
            for c in range(self.cases):
                t = "%sk%d_%d" % (tag, k, c)
                offline.save_outputs(res_addr, t, scales[k, c], motions)
                names += [res_addr + "scales.txt" + t, res_addr + "path.txt" + t]
        return names
