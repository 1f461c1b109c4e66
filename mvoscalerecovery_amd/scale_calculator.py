"""Drop-in ``ScaleEstimator`` backed by the MI355X kernels.

Mirrors the call surface of /root/reference/src/scale_calculator.py:21-46,396-423 (the
deterministic estimator; ``rescale.ScaleEstimator`` has the same ctor/methods,
/root/reference/src/rescale.py:22-38,191-193), so that the only edit in the reference's drivers
is the import line (/root/reference/src/main.py:18-20, main_offline.py:18-20):

    from mvoscalerecovery_amd.scale_calculator import ScaleEstimator

Per frame the work is split exactly where the reference calls Qhull:

    host   vanishing-row filter (:252-254), Delaunay #1 (:257)            [SciPy, as in the reference]
    GPU    feature_remap + find_outliers (:390-394,:151-167)               [mvosr_outlier_vote_batch]
    host   Delaunay #2 over the survivors (:266)                           [SciPy]
    GPU    feature_selection_by_tri + road model + raw scale (:225-248,:324-354,:419)  [mvosr_scale_batch]
    GPU    window median (:396-400)                                        [mvosr_window_median]

``scale_calculation_batch`` does the same for a whole list of frames with one launch per GPU
stage (and, when both triangulations are supplied, a single fused launch).  There is no CPU
implementation behind this class: without libmvosr.so / a gfx950 device it raises.
"""
from __future__ import annotations

import os
from collections import deque

import numpy as np

from . import _lib
from . import constants as K
from . import data_check
from . import distribution
from . import packing
from . import stream
from .engine import DeviceBatch, DeviceOutputs, FeatDistOutputs, ReliabilityOutputs, ScaleEngine, TriGraphOutputs


def raise_for_status(status, frame=None):
    """Turn a kernel status into what the reference does at that point."""
    where = "" if frame is None else " (frame %d of the batch)" % frame
    if status == K.ST_ERR_LEFT:      # scale_calculator.py:343, empty selection indexed with [-1]
        raise IndexError("index -1 is out of bounds for axis 0 with size 0" + where)
    if status == K.ST_ERR_RIGHT:     # scale_calculator.py:344, empty selection indexed with [0]
        raise IndexError("index 0 is out of bounds for axis 0 with size 0" + where)
    if status == K.ST_ERR_SINGULAR:  # scale_calculator.py:229
        raise np.linalg.LinAlgError("Singular matrix" + where)
    if status == K.ST_ERR_MASK:
        raise _lib.MvosrLibraryError("second triangulation inconsistent with the vote computed on the GPU" + where)
    if status == K.ST_ERR_EMPTY:
        raise ValueError("frame without features below the vanishing row / without triangles" + where)


class _HostOutputs:
    """Stage outputs that were assembled on the host, behind ``DeviceOutputs``' reading interface (``get`` / ``free``)."""

    def __init__(self, arrays):
        self.bufs = dict(arrays)

    def get(self, name):
        return self.bufs[name]

    def free(self):
        self.bufs = {}


class ScaleEstimator(stream.StreamKnobs):
    # (the streamed path's shared knobs: stream.StreamKnobs)
    PIPELINE_CHUNK = 512            # frames per chunk of the host-triangulation streaming path (_stream_chunks)
    LAZY_FLAT_FEATURE = True        # after a batch: flat_feature / flat_feature_2d when they are read (see the properties)
    GPU_EXACT_TWO_CONTEXTS = True   # check_triangle="reference": the chunks of a call alternate between two contexts (see _stream_gpu)
    GPU_EXACT_STANDIN = True        # check_triangle="reference": the second triangulation by the fast kernel as a stand-in; Qhull's own rows only for
                                    # the frames of the exact pass (engine.DeviceBatch.triangulate); False: Qhull's replay for every frame
    GPU_SINGLE_HOT = True           # check_triangle="fixed", ONE frame per call: the product kernels only, height_level exact when read (see _single_exact_fast)
    GPU_EXACT_SINGLE_FAST = True    # check_triangle="reference", ONE frame per call: SciPy for the first triangulation only (see _single_exact_fast)
    GPU_EXACT_HOST_REPLAY = True    # check_triangle="reference" with triangulation="gpu": the estimator's host-side triangulations by mvosr_qhull_rows_host
    GPU_EXACT_FORCE_DEVICE = False  # (tests) the device replay however few the frames
    GPU_EXACT_MIN_FRAMES = 8        # ... calls of fewer frames (or fewer than ~3.7 per Delaunay worker) take SciPy's triangulations (same rows, lower latency)
    GPU_EXACT_CHUNK = 16384         # check_triangle="reference" (the Qhull-rows kernel): frames per chunk, at most ...
    GPU_EXACT_CHUNK_POINTS = 33000000   # ... and features per chunk (~0.75 KB each on the device: 25 GB at the cap)
    GPU_EXACT_FIRST_CHUNK = 4096    # check_triangle="reference", two contexts: frames of a call's first chunk (0: a full chunk; 4096 = one round of resident wavefronts: profiles/r06_exact_first_chunk_ab.txt)
    GPU_EXACT_HOST_REDO = True      # check_triangle="reference" batches: the exact pass's few frames through the host path (see _chunk_gpu)
    GPU_EXACT_HOST_REDO_MAX = 64    # ... up to so many per chunk (16 per Delaunay worker at most); more: the device's exact pass (one masked relaunch)
    GPU_EXACT_LAZY_LEVEL = True     # check_triangle="reference" batches: a chunk's last frame is not on the exact mask (see _stream_gpu)
    GPU_REDO_CONTEXT = True         # streamed batches: the host-path re-run of declined frames on a context of its own (see _chunk_gpu_finish)
    GPU_REDO_DEFER = True           # ... and finished after the call's last chunk (its SciPy calls start on the worker pool at once)

    def __init__(self, absolute_reference, window_size=6, vanish=K.VANISH, focus=K.FOCUS, device=0,
                 delaunay_workers=None, verbose=False, mutate_inputs=True, triangulation=None, check_triangle=None, vote="outliers", selection="tri"):
        # reference attributes (scale_calculator.py:23-40)
        self.absolute_reference = absolute_reference
        self.camera_pitch = K.CAMERA_PITCH
        self.scale = None
        self.inliers = None
        self.scale_queue = deque()
        self.motion_queue = deque()
        self.window_size = window_size
        self.vanish = vanish
        self.focus = focus
        self.b_matrix = np.ones((3, 1), float)
        self.all_features = []
        self.correct_distance_features = []
        self.flat_features = []
        self.all_feature = []
        self.correct_distance_feature = []
        self.flat_feature = []
        self.flat_feature_2d = []
        self.img = None
        # build-side state
        self.verbose = verbose
        self.mutate_inputs = mutate_inputs          # the reference remaps the caller's feature3d in place (:414)
        self.delaunay_workers = delaunay_workers
        # triangulation = "scipy": both triangulations by scipy.spatial.Delaunay on the host.  "gpu": on the device; rows, vote
        # counters and survivor counts stay in HBM from the first triangulation to the scale kernel.
        # check_triangle = "reference": the vote's flag pattern exactly as the reference has it (:113-115 sets flag[1]
        # where flag[2] is meant), which depends on Qhull's rotation of each row — with SciPy's rows this is the reference bit
        # for bit, and "gpu" builds exactly those rows (mvosr_delaunay_qhull_batch replays Qhull's insertion order; DESIGN.md
        # §3.6).  "fixed": the (0,2) pair marks vertices 0 and 2 — a DECLARED DEVIATION (DESIGN.md §4 has the
        # measured agreement with the reference) under which the vote, and with rows in canonical form every stage, is a function
        # of the triangle SET alone (the faster device kernels: mvosr_delaunay_batch).
        # Defaults.  No triangulation given (the reference's own construction, /root/reference/src/main.py:55): the reference's
        # result from the fastest path that gives it — "gpu" with "reference": batches on the device, a per-frame call (or a
        # handful of frames) through SciPy, the same rows either way (round 5; MVOSR_TRIANGULATION=scipy restores the host default).
        # triangulation="gpu" given explicitly: "fixed", the declared-deviation speed mode, as before.  "scipy": "reference".
        if triangulation is None:
            triangulation = os.environ.get("MVOSR_TRIANGULATION", "gpu")
            if check_triangle is None:
                check_triangle = "reference"
        if triangulation not in ("scipy", "gpu"):
            raise ValueError("triangulation must be 'scipy' or 'gpu'")
        if check_triangle is None:
            check_triangle = "fixed" if triangulation == "gpu" else "reference"
        if check_triangle not in ("reference", "fixed"):
            raise ValueError("check_triangle must be 'reference' or 'fixed'")
        # vote = "outliers": find_outliers decides which features have a wrong depth (:260, the reference's live line).
        # "reliability": find_reliability_by_graph in its place (:259, the reference's commented alternative) — on the staged
        # host-triangulation path only: the fused device-resident kernels recompute find_outliers themselves.
        if vote not in ("outliers", "reliability"):
            raise ValueError("vote must be 'outliers' or 'reliability'")
        if vote == "reliability" and triangulation != "scipy":
            raise ValueError("vote='reliability' runs on the staged host-triangulation path: it needs triangulation='scipy'")
        self.vote = vote
        self.last_reliability = None
        # selection = "tri": feature_selection_by_tri picks the road's features (:273, the reference's live line).  "tri_graph":
        # feature_selection_by_tri_graph in its place (:589, the reference's commented alternative) — on the staged
        # host-triangulation path only, with either vote.
        if selection not in ("tri", "tri_graph"):
            raise ValueError("selection must be 'tri' or 'tri_graph'")
        if selection == "tri_graph" and triangulation != "scipy":
            raise ValueError("selection='tri_graph' runs on the staged host-triangulation path: it needs triangulation='scipy'")
        self.selection = selection
        self.last_tri_graph = None
        self.triangulation = triangulation
        self.check_triangle = check_triangle
        if delaunay_workers is None or delaunay_workers > 1:
            packing.start_pool(delaunay_workers)    # fork the host stage's workers BEFORE the GPU runtime starts its threads
        self.engine = ScaleEngine(absolute_reference, device=device, camera_pitch=self.camera_pitch, check_triangle=check_triangle)
        # The replay of Qhull's run (device kernel and host C form) reproduces ONE Qhull build's decisions; the reference floats with
        # whatever Qhull the installed SciPy bundles (:12,:257,:266).  Once per process and device the two are compared on fixed point
        # sets (selfcheck.py); on any difference this estimator takes the host path — by construction this box's reference.
        self.qhull_selfcheck = None
        if triangulation == "gpu" and check_triangle == "reference":
            from . import selfcheck
            self.qhull_selfcheck = selfcheck.run(self.engine.ctx, host_replay=packing.qhull_rows_host_or_none())
            if not self.qhull_selfcheck["ok"]:
                self.triangulation = "scipy"
        # the default estimator's own host triangulations (the per-frame call's first one, a handful of frames, the last frame's
        # flat_feature) by the C replay of Qhull's run where it accepts the set (packing.delaunay_simplices_fast) — held to the installed
        # SciPy by the self-check above; GPU_EXACT_HOST_REPLAY = False: SciPy, as in round 5
        self._host_replay = bool(self.GPU_EXACT_HOST_REPLAY and self.triangulation == "gpu" and self.check_triangle == "reference"
                                 and packing.qhull_rows_host_or_none() is not None)
        self.last_declined = 0                      # frames of the last device-triangulation chunk that went to the host's Qhull
        self.declined_total = 0                     # ... of the last call, all chunks
        self.last_status = None
        self.last_counts = None
        self.last_raw_scale = None

    # ---- reference surface -----------------------------------------------------------------
    def initial_estimation(self, motion_t):
        """scale_calculator.py:41-46 (host only: one asin)."""
        motion_t = np.asarray(motion_t)
        pitch = np.arcsin(motion_t[1]) * 180 / np.pi
        if self.verbose:
            print('initial pitch', pitch)
        self.motion_queue.append(motion_t.reshape(-1))
        return pitch

    def feature_remap(self, feature3d):
        """scale_calculator.py:390-394, in place on the caller's array (host mirror; the kernels
        apply the same rotation to the raw values at load)."""
        y = feature3d[:, 1] * np.cos(self.camera_pitch) - feature3d[:, 2] * np.sin(self.camera_pitch)
        z = feature3d[:, 1] * np.sin(self.camera_pitch) + feature3d[:, 2] * np.cos(self.camera_pitch)
        feature3d[:, 1] = y
        feature3d[:, 2] = z

    def scale_filtering(self, scale):
        """scale_calculator.py:396-400 for one pushed value (GPU window-median kernel)."""
        out = self.engine.window_median_host(np.array([scale], dtype=np.float64), self.window_size,
                                             list(self.scale_queue))
        self.scale_queue.append(scale)
        if len(self.scale_queue) > self.window_size:
            self.scale_queue.popleft()
        return out[0]

    # ``height_level`` (:217,:241) as the reference leaves it on the estimator: NumPy's own double.  The per-frame call of the
    # reference-exact device path (``_single_exact_fast``) knows it only in the kernel's summation order — equal to ~1e-16
    # relative, not bit for bit — and leaves a thunk instead: whoever READS the attribute (the caller; the next frame's
    # "no enough feature for triangulation" branch, :421) gets the exact value, computed then (one more SciPy call).
    def _get_height_level(self):
        d = self.__dict__
        thunk = d.get("_level_thunk")
        if thunk is not None:
            d["_level_thunk"] = None
            d["_level_value"] = thunk()
        try:
            return d["_level_value"]
        except KeyError:
            raise AttributeError("'ScaleEstimator' object has no attribute 'height_level'") from None

    def _set_height_level(self, value):
        self.__dict__["_level_value"] = value
        self.__dict__["_level_thunk"] = None

    height_level = property(_get_height_level, _set_height_level)

    # ``flat_feature`` / ``flat_feature_2d`` (:275-276, :416) after a BATCH are the selected points of its last processed frame: one
    # more run of that frame with the stage outputs (the host path: ~3 ms — 5 % of a 32 768-frame call of the fixed mode, a quarter
    # of a 1 000-frame one).  Nobody in the reference's drivers reads them (src/main.py:117-123 is dead code): they are produced when
    # somebody does.  A per-frame call sets them at once, as before.
    def _flat_pending(self):
        d = self.__dict__
        thunk = d.get("_flat_thunk")
        if thunk is not None:
            d["_flat_thunk"] = None
            thunk()

    def _get_flat_feature(self):
        self._flat_pending()
        return self.__dict__.get("_flat_value")

    def _set_flat_feature(self, value):
        self.__dict__["_flat_thunk"] = None
        self.__dict__["_flat_value"] = value

    def _get_flat_feature_2d(self):
        self._flat_pending()
        return self.__dict__.get("_flat2d_value")

    def _set_flat_feature_2d(self, value):
        self.__dict__["_flat2d_value"] = value

    flat_feature = property(_get_flat_feature, _set_flat_feature)
    flat_feature_2d = property(_get_flat_feature_2d, _set_flat_feature_2d)

    def scale_calculation(self, feature3d, feature2d, img=None):
        """scale_calculator.py:411-423: returns (filtered scale, std)."""
        scales, stds = self.scale_calculation_batch([feature3d], [feature2d], _single=True)
        return scales[0], stds[0]

    # ---- the reference's stage methods, for callers that drive the stages themselves ------------
    # They take arrays that are ALREADY remapped (the reference calls feature_remap first, :414), so
    # they run on an engine whose remap is the identity.
    def _plain_engine(self):
        if getattr(self, "_plain", None) is None:
            self._plain = ScaleEngine(self.absolute_reference, ctx=self.engine.ctx, camera_pitch=0.0, check_triangle=self.check_triangle)
        return self._plain

    def _pack_plain(self, feature3d, v_rows):
        f3 = np.asarray(feature3d, dtype=np.float64)
        f2 = np.stack([np.zeros(f3.shape[0]), np.asarray(v_rows, dtype=np.float64)], axis=1)
        return packing.pack_features([f3], [f2], -np.inf)

    def find_outliers(self, feature3d, feature2d, triangle_ids):
        """scale_calculator.py:151-167: boolean mask of the features whose vote counter is >= 0."""
        eng, ctx = self._plain_engine(), self.engine.ctx
        pf = self._pack_plain(feature3d, np.asarray(feature2d)[:, 1])
        packing.attach_tri1(pf, [np.asarray(triangle_ids)])
        db = DeviceBatch(ctx, pf, with_tri2=False)
        out = DeviceOutputs(ctx, db, counts=True, stage=True)
        eng.outlier_vote_batch(db, out)
        ctx.sync()
        counters = out.get("vote_counters")[pf.frame_slice(0)]
        out.free()
        db.free()
        if self.verbose:
            print('feature rejected ', int(np.sum(counters < 0)))
            print('feature left     ', int(np.sum(counters >= 0)))
        return counters >= 0

    def find_reliability_by_graph(self, feature3d, feature2d, triangle_ids):
        """scale_calculator.py:127-149: boolean mask of the features whose reliability ends above 0.8; the values themselves
        stay in ``self.last_reliability``."""
        eng, ctx = self._plain_engine(), self.engine.ctx
        pf = self._pack_plain(feature3d, np.asarray(feature2d)[:, 1])
        packing.attach_tri1(pf, [np.asarray(triangle_ids)])
        db = DeviceBatch(ctx, pf, with_tri2=False)
        out = ReliabilityOutputs(ctx, db)
        try:
            eng.reliability_batch(db, out)
            sl = pf.frame_slice(0)
            reliability, keep, st = out.get("reliability")[sl], out.get("keep")[sl], int(out.get("status")[0])
        finally:
            out.free()
            db.free()
        if st != 0:
            raise ValueError("triangle_ids name a vertex twice in a row, or a vertex outside the features")
        self.last_reliability = reliability
        valid_id = keep == 0                                                  # :145
        if self.verbose and len(reliability):
            print('reliability', np.min(reliability), np.median(reliability), np.max(reliability))
            print('feature rejected ', int(np.sum(~valid_id)))
            print('feature left     ', int(np.sum(valid_id)))
        return valid_id

    def feature_selection_by_tri(self, feature3d, triangle_ids):
        """scale_calculator.py:225-248: sorted unique vertex ids of the flat, low triangles; sets
        ``self.height_level``."""
        eng, ctx = self._plain_engine(), self.engine.ctx
        f3 = np.asarray(feature3d, dtype=np.float64)
        pf = self._pack_plain(f3, np.zeros(f3.shape[0]))
        packing.attach_tri1(pf, [np.zeros((0, 3), dtype=np.int32)])          # no vote: every feature survives
        packing.attach_tri2(pf, [np.asarray(triangle_ids)], [np.ones(f3.shape[0], dtype=bool)])
        db = DeviceBatch(ctx, pf)
        out = DeviceOutputs(ctx, db, counts=True, stage=True)
        eng.scale_batch(db, out)
        ctx.sync()
        st = int(out.get("status")[0])
        sel = out.get("selected")[pf.frame_slice(0)]
        self.height_level = out.get("height_level")[0]                        # :241
        out.free()
        db.free()
        if st in (K.ST_ERR_SINGULAR, K.ST_ERR_MASK, K.ST_ERR_EMPTY):
            raise_for_status(st)
        return np.nonzero(sel)[0]                                             # :247

    def _tri_graph_launch(self, feature3d, triangle_ids, given=None):
        """One frame through mvosr_tri_graph_batch on the identity-remap engine -> dict of host arrays.  ``given``: (heights,
        pitch_deg) per row for the given form; None: from ``feature3d``."""
        eng, ctx = self._plain_engine(), self.engine.ctx
        f3 = np.asarray(feature3d, dtype=np.float64)
        tri = np.ascontiguousarray(triangle_ids, dtype=np.int32).reshape(-1, 3)
        pf = self._pack_plain(f3, np.zeros(f3.shape[0]))
        packing.attach_tri1(pf, [np.zeros((0, 3), dtype=np.int32)])
        packing.attach_tri2(pf, [tri], [np.ones(f3.shape[0], dtype=bool)])
        db = DeviceBatch(ctx, pf)
        out = TriGraphOutputs(ctx, db)
        bufs = [ctx.to_device(np.ascontiguousarray(a, dtype=np.float64)) for a in given] if given is not None else [None, None]
        try:
            eng.tri_graph_batch(db, out, bufs[0], bufs[1])
            ctx.sync()
            T = len(tri)
            r = {k: out.get(k)[:T] for k in ("p_road", "p_initial", "valid", "neighbors")}
            r.update({k: out.get(k)[0] for k in ("height_level", "n_flat", "n_valid", "n_rounds", "status")})
            r["selected"] = out.get("selected")[pf.frame_slice(0)]
        finally:
            for b in bufs:
                if b is not None:
                    b.free()
            out.free()
            db.free()
        return r

    def triangle2region_graph(self, triangle_ids):
        """scale_calculator.py:56-81: per row the rows that share an edge with it, in the reference's list order (first the
        lower-index neighbours in the order of the row's own edges ab, ac, bc, then the higher-index ones ascending)."""
        tri = np.asarray(triangle_ids).reshape(-1, 3)
        if len(tri) == 0:
            return []
        n = max(int(tri.max()) + 1, 3)                                        # :59
        zeros = np.zeros(len(tri))
        r = self._tri_graph_launch(np.zeros((n, 3)), tri, given=(zeros, zeros))
        if int(r["status"]) != 0:
            raise ValueError("triangle_ids name a vertex twice in a row, a vertex below 0, or an edge on more than two rows")
        return [[int(u) for u in row if u >= 0] for row in r["neighbors"]]

    def feature_selection_by_tri_graph(self, feature3d, triangle_ids):
        """scale_calculator.py:177-222: sorted unique vertex ids of the rows whose road probability ends above 0.5; sets
        ``self.height_level``; the probabilities stay in ``self.last_tri_graph``."""
        r = self._tri_graph_launch(feature3d, triangle_ids)
        st = int(r["status"])
        if st in (K.ST_ERR_SINGULAR, K.ST_ERR_MASK, K.ST_ERR_EMPTY):
            raise_for_status(st)
        self.height_level = r["height_level"]                                 # :217
        self.last_tri_graph = {"p_road": r["p_road"], "p_initial": r["p_initial"], "n_rounds": int(r["n_rounds"])}
        if self.verbose:
            print('triangle left ', int(r["n_flat"]), 'from', len(r["valid"]))                     # :215
            print('height level', self.height_level)                                                # :218
            print('triangle left final', int(r["n_valid"]), 'from', len(r["valid"]))               # :220
        return np.nonzero(r["selected"])[0]                                   # :221

    def feature_selection(self, feature3d, feature2d):
        """scale_calculator.py:250-279 on remapped input: the selected road points, or None."""
        from .packing import delaunay_simplices
        feature3d, feature2d = np.asarray(feature3d, dtype=np.float64), np.asarray(feature2d, dtype=np.float64)
        low = feature2d[:, 1] > self.vanish                                   # :252-254
        feature2d, feature3d = feature2d[low, :], feature3d[low, :]
        vote = self.find_reliability_by_graph if self.vote == "reliability" else self.find_outliers          # :259 / :260
        valid = vote(feature3d, feature2d, delaunay_simplices(feature2d))     # :257-260
        if not valid.shape[0] > 3:                                            # :263 (length of the mask)
            if self.verbose:
                print('no enough feature for triangulation')
            return None                                                       # :268-270
        feature2d, feature3d = feature2d[valid, :], feature3d[valid, :]       # :264-265
        select = self.feature_selection_by_tri_graph if self.selection == "tri_graph" else self.feature_selection_by_tri   # :589 / :273
        selected = select(feature3d, delaunay_simplices(feature2d))           # :266-273
        if len(selected) > 0:
            self.flat_feature_2d = feature2d[selected]                        # :275
            return feature3d[selected]
        if self.verbose:
            print('no enough flat feature')
        return None

    def road_model_calculation_static(self, feature3d):
        """scale_calculator.py:324-354: ``(height, 0, 1)`` from the y column of the selected points;
        raises IndexError where the reference does (:343-344)."""
        eng, ctx = self._plain_engine(), self.engine.ctx
        f3 = np.asarray(feature3d, dtype=np.float64).reshape(-1, 3)
        pf = self._pack_plain(f3, np.zeros(f3.shape[0]))
        db = DeviceBatch(ctx, pf, with_tri2=False)
        out = DeviceOutputs(ctx, db, counts=True)
        eng.road_model_batch(db, out, np.array([getattr(self, "height_level", np.nan)], dtype=np.float64))
        st, h = int(out.get("status")[0]), float(out.get("height")[0])
        out.free()
        db.free()
        if st == K.ST_NO_FLAT:                                                # an empty list: the reference's np.histogram
            st, h = K.ST_LEVEL, float(getattr(self, "height_level", np.nan))  # of nothing has no modes and no points (:334-335)
        raise_for_status(st)
        return h, 0, 1

    def road_model_calculation(self, feature3d):
        return self.road_model_calculation_static(feature3d)                  # :281-282

    def road_model_calculation_static_tri(self, heights):
        """scale_calculator.py:294-310 (what follows the return at :310 is dead): ``(scale_norm, 0, 1)`` from a list of triangle
        heights — the first run of modes of the histogram of 1/h over 19 bins of 0.1, or the median of 1/h when there is none.
        One packed list uploaded, one launch of mvosr_static_tri_batch.  Like the reference's function it asks for no minimum
        count (rescale.py:181 does); an empty list gives NaN, as ``np.median([])`` does.  A height that is not finite or not
        positive raises ValueError (flat_selection produces none)."""
        h = np.ascontiguousarray(np.asarray(heights, dtype=np.float64).reshape(-1))
        if self.verbose:
            print('flat features', h.size)                                    # :295
        ctx = self.engine.ctx
        blk = ctx.block([("off", 2, np.int64), ("height", max(h.size, 1), np.float64)])
        try:
            blk.upload({"off": np.array([0, h.size], dtype=np.int64), "height": h if h.size else np.ones(1)})
            r = self.engine.static_tri_batch(1, blk["off"], blk["height"], min_count=0, absolute_reference=self.absolute_reference)
        finally:
            blk.free()
        if int(r["status"][0]) == K.ST_ERR_MASK:
            raise ValueError("road_model_calculation_static_tri: heights must be finite and positive")
        return float(r["scale_norm"][0]), 0, 1

    def road_model_calculation_ransac(self, feature3d, seed=None, triples=None):
        """scale_calculator.py:366-384 (not on the path of :281; kept for callers that use it): RANSAC plane through the
        selected points (30 hypotheses, threshold 0.005; :369), its inliers at 0.01 (:370-371), camera height
        ``-d/|n|`` and pitch ``asin(-n_y/|n|)`` with the normal's sign fixed so that n_y >= 0 (:372-383).  Returns
        ``(ransac_camera_height, pitch, inliers)``.  The reference's sampler is unseeded; ``seed`` / ``triples`` make
        the draw reproducible."""
        from . import estimate_road_norm as ern
        pts = np.asarray(feature3d, dtype=np.float64)
        m, _ = ern.get_pitch_ransac(pts, 30, 0.005, seed=seed, triples=triples, device=self.engine.ctx.device)      # :369
        inlier_id = ern.get_inliers(m, pts, 0.01, device=self.engine.ctx.device)                                    # :370
        inliers = pts[inlier_id, :]
        normal, h_bar = np.array(m[0:-1]), -m[-1]                                                                   # :372-374
        if normal[1] < 0:                                                                                           # :375-377
            normal, h_bar = -normal, -h_bar
        normal_len = np.sqrt(np.sum(normal * normal))
        return h_bar / normal_len, np.arcsin(-normal[1] / normal_len), inliers                                      # :380-384

    def scale_calculation_static(self, point_selected):
        """scale_calculator.py:401-409 (remaps ``point_selected`` in place, like the reference)."""
        self.feature_remap(point_selected)
        height, pitch, std = self.road_model_calculation(point_selected)
        scale = self.absolute_reference / height
        return self.scale_filtering(scale), std

    def scale_calculation_static_batch(self, point_lists):
        """``scale_calculation_static`` (:401-409) once per list, in order, on this estimator: every list remapped in place
        (:402), ONE mvosr_road_model_batch over all of them (:324-354), scale = reference / height (:405) and the window median
        (:396-400).  Returns ``(filtered[F], ones[F])``.  A list at which the reference raises (IndexError :343-344; AttributeError
        where an empty list finds no ``height_level``, :335) raises here after the lists before it have been pushed."""
        for p in point_lists:
            self.feature_remap(p)                                             # :402
        F = len(point_lists)
        if F == 0:
            return np.zeros(0), np.ones(0)
        eng, ctx = self._plain_engine(), self.engine.ctx
        f3s = [np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in point_lists]
        pf = packing.pack_features(f3s, [np.zeros((a.shape[0], 2)) for a in f3s], -np.inf)
        db = DeviceBatch(ctx, pf, with_tri2=False)
        out = DeviceOutputs(ctx, db, counts=True)
        try:
            eng.road_model_batch(db, out, np.full(F, np.nan))
            status, height = out.get("status")[:F], out.get("height")[:F]
        finally:
            out.free()
            db.free()
        pushed, error = [], None
        for f in range(F):
            try:
                h = height[f]
                if int(status[f]) in (K.ST_NO_FLAT, K.ST_LEVEL):              # no modes and no points left (:334-335): the level —
                    h = np.float64(self.height_level)                         # AttributeError where it was never set, as in the reference
                else:
                    raise_for_status(int(status[f]), f if F > 1 else None)
            except (IndexError, AttributeError, np.linalg.LinAlgError, _lib.MvosrLibraryError, ValueError) as exc:
                error = exc
                break
            with np.errstate(all="ignore"):
                pushed.append(self.absolute_reference / h)                    # :405
        filtered = np.zeros(0)
        if pushed:
            filtered = self.engine.window_median_host(np.array(pushed, dtype=np.float64), self.window_size, list(self.scale_queue))
            self.scale_queue.extend(pushed)                                   # :397-399
            while len(self.scale_queue) > self.window_size:
                self.scale_queue.popleft()
        if error is not None:
            raise error
        return filtered, np.ones(F)

    # ---- the reference's feature-distribution analysis (:49-54, :386-388, :428-599; main.py:117-123 under ``if(False)``) --------
    # The three populations of a frame — every feature below the vanishing row, the ones the reliability vote keeps, the ones
    # feature_selection_by_tri selects — come from the staged path; mvosr_feature_distribution_batch turns them into histograms,
    # mean / std / median and the sequence tables; the few scalar operations on top are distribution.py's.
    def check_distance(self, feature3d):
        """scale_calculator.py:49-54 (host only)."""
        return distribution.check_distance(feature3d, self.focus, verbose=self.verbose)

    def distribution(self, feature3d):
        """scale_calculator.py:386-388 computes a histogram only to plot it: nothing is returned, nothing drawn here."""
        return None

    def check_mode(self, dis_data, bins):
        """scale_calculator.py:446-483 (host only)."""
        return distribution.check_mode(dis_data, bins, verbose=self.verbose)

    def check_reverse_mode(self, dis_data):
        """scale_calculator.py:428-443 (host only)."""
        return distribution.check_reverse_mode(dis_data)

    def _dist_engine(self):
        """The un-remapped engine of the distribution path: ``_plain_engine()``, in the reference's vote mode whatever the estimator's."""
        if self.check_triangle == "reference":
            return self._plain_engine()
        if getattr(self, "_dist_plain", None) is None:
            self._dist_plain = ScaleEngine(self.absolute_reference, ctx=self.engine.ctx, camera_pitch=0.0, check_triangle="reference")
        return self._dist_plain

    def _dist_tables(self):
        if getattr(self, "_dist_seq", None) is None:
            self._dist_seq = self.engine.ctx.zeros((_lib.FD_POPULATIONS, _lib.FD_HIST_WORDS), np.int64)
        return self._dist_seq

    def _dist_check_cap(self, n):
        cap = self.engine.feature_distribution_max_features()
        if n > cap:
            raise ValueError("feature distribution: %d features in one frame, at most %d fit the kernel's LDS plan" % (n, cap))

    def _dist_launch(self, off, cnt, y, level, scale, max_feat, tables):
        """One launch of mvosr_feature_distribution_batch over host arrays in the packed layout -> (n, words, words_scaled, stats, status)."""
        eng, ctx, F = self._dist_engine(), self.engine.ctx, len(cnt)
        total = max(len(y), 2)
        blk = ctx.block([("off", max(F, 1), np.int64), ("cnt", max(F, 1), np.int32), ("y", total, np.float64),
                         ("scale", max(F, 1), np.float64), ("level", total, np.uint8)])
        out = FeatDistOutputs(ctx, F)
        try:
            pad = lambda a, n, dt: np.concatenate([np.asarray(a, dtype=dt), np.zeros(n - len(a), dtype=dt)])
            blk.upload({"off": pad(off, max(F, 1), np.int64), "cnt": pad(cnt, max(F, 1), np.int32), "y": pad(y, total, np.float64),
                        "scale": pad(scale, max(F, 1), np.float64), "level": pad(level, total, np.uint8)})
            eng.feature_distribution_batch(F, blk["off"], blk["cnt"], blk["y"], blk["level"], blk["scale"], max_feat, out, tables)
            return tuple(out.get(k) for k in ("n", "hist", "hist_scaled", "stats", "status"))
        finally:
            out.free()
            blk.free()

    def _dist_of_list(self, data):
        """One list through the kernel as population 0 of one frame -> (words[172], mean, std, median)."""
        y = np.ascontiguousarray(np.asarray(data, dtype=np.float64).reshape(-1))
        self._dist_check_cap(y.size)
        n, words, _, stats, _ = self._dist_launch([0], [y.size], y, np.zeros(y.size, np.uint8), [1.0], y.size, None)
        return words[0, 0], stats[0, 0, 0], stats[0, 0, 1], stats[0, 0, 2]

    def _dist_of_attribute(self, name):
        """(words, mean, std, median) of the y column of ``all_feature`` / ``correct_distance_feature`` / ``flat_feature``: what the
        last ``check_full_distribution`` left for that very array, else one launch on it."""
        value = getattr(self, name)
        y = value[:, 1]                                               # (TypeError on the initial [] — or on None —, as in the reference)
        kept = getattr(self, "_dist_kept", {}).get(name)
        if kept is not None and kept[0] is value:
            return kept[1]
        return self._dist_of_list(y)

    def check_skewness(self, data, mode=None, method='p1'):
        """scale_calculator.py:486-497 on arbitrary data: one launch of the kernel on the list, the skew from its outputs."""
        return self._skew_from(self._dist_of_list(data), mode, method)

    def _skew_from(self, dist, mode, method):
        words, mean, std, median = dist
        if self.verbose:
            print('mean,meidan,std', mean, median, std)
        if method == 'p2':
            return distribution.skews(mean, std, median, 0.0)[1]          # :489
        if method == 'p1':
            if mode is None:
                mode = distribution.p1_mode(words)                        # :492-495
            return distribution.skews(mean, std, median, mode)[0]         # :496
        raise UnboundLocalError("cannot access local variable 'skew' where it is not associated with a value")   # :497

    def skewness_analysis(self):
        """scale_calculator.py:498-503: the p1 skew of the selected features' y."""
        flat_skew = self._skew_from(self._dist_of_attribute("flat_feature"), None, 'p1')
        if self.verbose:
            print('skewness', flat_skew)
        return flat_skew

    def mode_analysis(self):
        """scale_calculator.py:505-507: check_mode over the DENSITY of the selected features' 99-bin histogram (its thresholds 2
        are applied to density values, as in the reference)."""
        words = self._dist_of_attribute("flat_feature")[0]
        return self.check_mode(distribution.density_of(distribution.narrow_histogram(words, 99), 99), distribution.EDGES[:100])

    def plot_distribution(self, label, img, scale=1):
        """scale_calculator.py:509-560 without the figure: the curves it would plot, as a dict — ``bins`` (``bins[:-1]``) and
        ``selected`` (``0.1 * dis``, the density of the selected features over 49 bins), ``all_hist`` / ``correct_hist`` (the two
        count histograms it computes), ``all_points`` / ``correct_points`` / ``selected_points`` (the ``(z, -y)`` sets of the
        scatter) and ``img``.  Raises the reference's TypeError while no frame was analysed."""
        bins = distribution.EDGES[:50]
        res = {"label": label, "bins": bins[:-1], "all_hist": None, "correct_hist": None, "selected": None, "selected_points": None}
        if self.all_feature is not None and len(self.all_feature) > 0:                                 # :526-528
            res["all_hist"] = distribution.narrow_histogram(self._dist_of_attribute("all_feature")[0], 49)
        if len(self.correct_distance_feature) > 0:                                                     # :530-532
            res["correct_hist"] = distribution.narrow_histogram(self._dist_of_attribute("correct_distance_feature")[0], 49)
        flat = self.flat_feature
        if flat is not None and len(flat) > 0:                                                         # :534-537
            res["selected"] = 0.1 * distribution.density_of(distribution.narrow_histogram(self._dist_of_attribute("flat_feature")[0], 49), 49)
        res["all_points"] = (self.all_feature[:, 2], -self.all_feature[:, 1])                          # :546 (TypeError on [])
        res["correct_points"] = (self.correct_distance_feature[:, 2], -self.correct_distance_feature[:, 1])    # :547
        if flat is not None and len(flat) > 0:                                                         # :551-552
            res["selected_points"] = (flat[:, 2], -flat[:, 1])
        res["img"] = self.img                                                                          # :557
        return res

    def reset_distribution(self):
        """Zero the sequence tables on the device and empty the accumulated lists (``all_features`` and its siblings)."""
        self._dist_tables().fill(0)
        self.all_features, self.correct_distance_features, self.flat_features = [], [], []

    def cumulative_histograms(self, bins=29, density=False):
        """The three histograms of the sequence — np.histogram of the y column of ``all_features``, ``correct_distance_features`` and
        ``flat_features`` over ``np.array(range(0, bins + 1)) * 0.1`` (:513-520 has bins = 29) — from the tables resident on the
        device: ``[3, bins]``, int64 counts or, with ``density``, float64."""
        self.engine.ctx.sync()
        h = distribution.narrow_histogram(self._dist_tables().download(), bins)
        return np.stack([distribution.density_of(r, bins) for r in h]) if density else h

    def check_full_distribution(self, feature3d, feature2d, scale, img=None):
        """scale_calculator.py:562-599: sets ``all_feature``, ``correct_distance_feature``, ``flat_feature``, ``height_level`` and
        ``img``, appends the scaled rows to ``all_features`` and its siblings, returns early and raises where the reference does
        — after the state changes the reference has made by then.  The frame's statistics stay in ``last_distribution``."""
        res = self.check_full_distribution_batch([feature3d], [feature2d], [scale], _img=img)
        if 0 in res.errors:
            raise res.errors[0]

    def check_full_distribution_batch(self, feature3ds, feature2ds, scales, accumulate=True, _img=None, _launch=True):
        """``check_full_distribution`` once per frame, in order, on this estimator: one staged pass (reliability vote on SciPy's rows,
        ``feature_selection_by_tri``) and ONE launch of mvosr_feature_distribution_batch per chunk of ``PIPELINE_CHUNK`` frames; the
        sequence tables stay on the device.  Returns a ``distribution.FeatureDistribution``.  It does not raise at a frame where the
        per-frame call returns early or raises: such a frame gets a status, NaNs and its exception in ``errors``, and contributes
        what the reference had appended by then.  ``accumulate=False``: the Python lists ``all_features`` ... are not extended
        (one array object per feature and frame; the device tables are added to all the same)."""
        F = len(feature3ds)
        if not (len(feature2ds) == F and len(scales) == F):
            raise ValueError("feature3ds, feature2ds and scales must have one entry per frame")
        f2s = [np.asarray(a) for a in feature2ds]
        for f2 in f2s:
            self._dist_check_cap(int(np.count_nonzero(f2[:, 1] > self.vanish)) if f2.size else 0)
        parts = []
        for a in range(0, F, self.PIPELINE_CHUNK):
            b = min(F, a + self.PIPELINE_CHUNK)
            parts.append(self._distribution_chunk(feature3ds[a:b], f2s[a:b], scales[a:b], accumulate, _img, _launch))
        if not parts:
            parts.append((np.zeros((0, 3), np.int32), np.zeros((0, 3, _lib.FD_HIST_WORDS), np.int32), np.zeros((0, 3, _lib.FD_HIST_WORDS), np.int32),
                          np.zeros((0, 3, 3)), np.zeros(0), np.zeros(0, np.int32), {}))
        errors, base = {}, 0
        for part in parts:
            errors.update({base + f: e for f, e in part[6].items()})
            base += len(part[5])
        res = distribution.FeatureDistribution(*(np.concatenate([part[k] for part in parts]) for k in range(6)), errors)
        self.last_distribution = res
        return res

    def _distribution_levels(self, f3s, f2s):
        """The staged pass of a chunk (:564-591) -> the packed frames, the vote's masks, one level per packed feature (0 below the
        vanishing row, 1 kept, 2 selected), how each frame ends (DIST_*), the exceptions, the selections over the survivors and the
        frames' height levels."""
        eng, F = self._dist_engine(), len(f3s)
        _, status, level, _, host_errors, st = self._chunk_staged(f3s, f2s, stage=True, _remapped=True, _distribution=eng)
        pf, masks, selected = st["pf"], st["masks"], st["out"].get("selected")
        tri1_errors = pf.extra["tri1_errors"]
        cnt = np.asarray(pf.feat_cnt)
        levels = np.zeros(max(pf.total_padded, 2), dtype=np.uint8)
        outcome, errors, picks = np.zeros(F, dtype=np.int32), {}, [None] * F
        for f in range(F):
            sl = pf.frame_slice(f)
            if f in tri1_errors:                                              # :572 raised
                outcome[f], errors[f] = distribution.DIST_RAISED_TRI1, tri1_errors[f]
            elif cnt[f] <= 3:                                                 # :576, :586 (the LENGTH of the mask)
                outcome[f] = distribution.DIST_EARLY
            else:
                levels[sl] = masks[f]                                         # :577-582
                if f in host_errors:                                          # :583 raised
                    outcome[f], errors[f] = distribution.DIST_RAISED_TRI2, host_errors[f]
                elif int(status[f]) in (K.ST_ERR_SINGULAR, K.ST_ERR_MASK, K.ST_ERR_EMPTY):      # :588 raised (:229)
                    outcome[f] = distribution.DIST_RAISED_SELECTION
                    try:
                        raise_for_status(int(status[f]))
                    except Exception as exc:                                  # noqa: BLE001 - kept for the caller, who raises it
                        errors[f] = exc
                else:
                    o, kept = int(pf.feat_off[f]), int(np.count_nonzero(masks[f]))
                    pick = selected[o:o + kept] != 0                          # over the survivors (:247, sorted unique ids)
                    where = np.nonzero(masks[f])[0][pick]
                    levels[o + where] = 2                                     # :590-595
                    picks[f] = pick
                    outcome[f] = distribution.DIST_OK if pick.any() else distribution.DIST_NO_SELECTION
        return pf, masks, levels, outcome, errors, picks, level

    def _distribution_chunk(self, f3s, f2s, scales, accumulate, img, launch):
        F = len(f3s)
        pf, masks, levels, outcome, errors, picks, level = self._distribution_levels(f3s, f2s)
        cnt = np.asarray(pf.feat_cnt)
        scale_arr = np.array([float(s) for s in scales], dtype=np.float64)
        if launch:
            n, words, words_s, stats, kstatus = self._dist_launch(pf.feat_off, cnt, pf.y, levels, scale_arr, int(pf.max_feat), self._dist_tables())
        else:                                                                 # (profiles/featdist_bench.py: the staged pass alone)
            W = _lib.FD_HIST_WORDS
            n, words, words_s = np.zeros((F, 3), np.int32), np.zeros((F, 3, W), np.int32), np.zeros((F, 3, W), np.int32)
            stats, kstatus = np.full((F, 3, 3), np.nan), np.zeros(F, np.int32)
        outcome = np.where(kstatus != 0, kstatus, outcome).astype(np.int32)
        # the attributes, frame by frame, as the per-frame calls would leave them
        kept_stats = dict(getattr(self, "_dist_kept", {}))
        of = lambda f, p: (words[f, p], stats[f, p, 0], stats[f, p, 1], stats[f, p, 2])
        for f in range(F):
            f3 = np.asarray(f3s[f])[pf.lower_index[f], :]                     # :564-565
            self.all_feature = f3.copy()                                      # :567
            kept_stats["all_feature"] = (self.all_feature, of(f, 0))
            if accumulate:
                self.all_features.extend(f3 * scales[f])                     # :568-569
            if outcome[f] in (distribution.DIST_RAISED_TRI1, distribution.DIST_EARLY) or kstatus[f] != 0:
                continue
            f3 = f3[masks[f], :]                                              # :578
            self.correct_distance_feature = f3.copy()                         # :580
            kept_stats["correct_distance_feature"] = (self.correct_distance_feature, of(f, 1))
            if accumulate:
                self.correct_distance_features.extend(f3 * scales[f])        # :581-582
            if picks[f] is None:
                continue
            self.height_level = level[f]                                      # :241
            if picks[f].any():                                                # :590
                self.flat_feature = f3[picks[f]].copy()                       # :591-593
                kept_stats["flat_feature"] = (self.__dict__["_flat_value"], of(f, 2))
                if accumulate:
                    self.flat_features.extend(self.flat_feature * scales[f]) # :594-595
            self.img = img                                                    # :599
        self._dist_kept = kept_stats
        hl = np.where([p is not None for p in picks], level, np.nan) if F else np.zeros(0)
        return n, words, words_s, stats, hl, outcome, errors

    # ---- the reference's pairwise depth-order check (script/data_check.py:19-34) over the same three populations --------------------
    # The staged pass of the distribution analysis gives one level per packed feature; mvosr_depth_check_batch turns the packed y and
    # z planes into the pair histograms of the three populations.  The sequence tables stay on the device.
    def _depth_check_seq(self):
        if getattr(self, "_dc_seq", None) is None:
            self._dc_seq = data_check.new_tables(ctx=self.engine.ctx)
        return self._dc_seq

    def reset_depth_check(self):
        """Zero the depth check's sequence tables on the device."""
        self._depth_check_seq().fill(0)

    def depth_check_tables(self):
        """The sequence tables: int64 ``[3, 62]`` — per population the 59 bins, then below, above, nan — of every frame
        ``depth_check_batch`` accumulated since the last ``reset_depth_check``."""
        self.engine.ctx.sync()
        return self._depth_check_seq().download()

    def depth_check_batch(self, feature3ds, feature2ds, accumulate=True):
        """``data_check.depth_check`` of every frame's three populations — every feature below the vanishing row, the ones the
        reliability vote keeps, the ones ``feature_selection_by_tri`` selects — on un-remapped input: one staged pass and ONE launch
        of mvosr_depth_check_batch per chunk of ``PIPELINE_CHUNK`` frames.  Returns a ``data_check.DepthCheckBatch``.  A frame that
        returns early or raises in the staged pass keeps the populations it reached (as in ``check_full_distribution_batch``); its
        exception is in ``errors``, not raised.  ``accumulate``: the frames are added to the sequence tables."""
        F = len(feature3ds)
        if len(feature2ds) != F:
            raise ValueError("feature3ds and feature2ds must have one entry per frame")
        f2s = [np.asarray(a) for a in feature2ds]
        tables = self._depth_check_seq() if accumulate else None
        parts, errors = [], {}
        for a in range(0, F, self.PIPELINE_CHUNK):
            b = min(F, a + self.PIPELINE_CHUNK)
            pf, _, levels, _, errs, _, _ = self._distribution_levels(feature3ds[a:b], f2s[a:b])
            parts.append(data_check.launch_packed(self.engine.ctx, pf.feat_off, np.asarray(pf.feat_cnt), pf.y, pf.z, levels,
                                                  int(pf.max_feat), tables))
            errors.update({a + f: e for f, e in errs.items()})
        res = data_check.concatenate(parts, errors)
        self.last_depth_check = res
        return res

    def depth_check(self, feature3d, feature2d):
        """One frame through ``depth_check_batch`` (the tables are added to); raises what the staged pass raised at the frame, after
        the launch — the result stays in ``last_depth_check``."""
        res = self.depth_check_batch([feature3d], [feature2d])
        if 0 in res.errors:
            raise res.errors[0]
        return res

    # ---- batched surface ---------------------------------------------------------------------
    def scale_calculation_batch(self, feature3ds, feature2ds, tri1s=None, tri2s=None, _single=False, _raw_only=False):
        """Equivalent to calling ``scale_calculation`` once per frame, in order, on this
        estimator: returns ``(scales[F], stds[F])`` (filtered scales).  ``tri1s``/``tri2s`` may
        carry precomputed triangulations (lists of (T,3) int arrays, SciPy ``simplices`` verbatim).
        If a frame hits one of the reference's raise sites, the frames before it are applied to
        the window state and the same exception type is raised.

        Without precomputed triangulations the batch STREAMS through the stages in chunks of
        ``PIPELINE_CHUNK`` frames: while the host's worker processes triangulate chunk k+1 (first call, :257)
        and chunk k (second call, :266), this process packs, uploads and launches the GPU stages of the
        chunks in between — the Qhull pool never waits for the GPU or for packing."""
        F = len(feature3ds)
        if F == 0:
            return np.zeros(0), np.zeros(0)
        stage = bool(_single)
        self.declined_total = 0
        # (the Qhull-rows kernel is a chain of dependent insertions: ~20 ms per 2000-point triangulation however few the frames —
        # a handful of frames, the per-frame call of /root/reference/src/main.py:113 among them, is quicker through SciPy: 6 ms)
        few_exact = False
        if self.check_triangle == "reference" and self.triangulation == "gpu":
            # device: two chains of n dependent insertions, ~11 us each, whatever the frame count (up to ~4 000 frames);
            # host: ~3 us per point and triangulation (SciPy), spread over the pool's workers — the break-even count of frames
            # (with the host replay of Qhull's run instead of SciPy — ~3 x faster — the break-even moves accordingly)
            w = max(1, packing.resolve_workers(self.delaunay_workers))
            per_worker, least = (10.0, 2.5 * self.GPU_EXACT_MIN_FRAMES) if self._host_replay else (3.7, self.GPU_EXACT_MIN_FRAMES)
            few_exact = F < max(int(least), int(per_worker * w)) and not self.GPU_EXACT_FORCE_DEVICE
        fast = None
        if few_exact and stage and F == 1 and tri1s is None and tri2s is None and self.GPU_EXACT_SINGLE_FAST:
            fast = self._single_exact_fast(feature3ds, feature2ds)
        if fast is None and stage and F == 1 and tri1s is None and tri2s is None and self.GPU_SINGLE_HOT and \
                self.triangulation == "gpu" and self.check_triangle == "fixed":
            fast = self._single_exact_fast(feature3ds, feature2ds, fixed=True)
        lazy_level = None
        if self.vote == "reliability" or self.selection == "tri_graph":
            raw, status, level, counts, host_errors, last = self._stream_staged(feature3ds, feature2ds, tri1s, tri2s, stage)
        elif fast is not None:
            raw, status, level, counts, host_errors, last, lazy_level = fast
        elif self.triangulation == "gpu" and tri1s is None and tri2s is None and not few_exact:
            lazy_last = bool(self.GPU_EXACT_LAZY_LEVEL and self.check_triangle == "reference" and not stage)
            raw, status, level, counts, host_errors, last = self._stream_gpu(feature3ds, feature2ds, stage, lazy_last=lazy_last,
                                                                             eager_final=bool(_raw_only))
            if lazy_last and self._lazy_levels and not _raw_only:
                # the level the estimator is left with (:241 of the last frame that reached it) when that frame is one of those: NumPy's
                # own double when somebody READS it (height_level is a property: the caller, or the next call's three-feature frame)
                bad_ = np.isin(status, K.ERROR_STATUSES)
                for f in host_errors:
                    bad_[f] = True
                end_ = int(np.argmax(bad_)) if bad_.any() else len(status)
                setters_ = np.nonzero(status[:end_] != K.ST_TOO_FEW)[0]
                if len(setters_) and int(setters_[-1]) in self._lazy_levels and end_ == len(status):
                    g_ = int(setters_[-1])
                    f3c, f2c = np.array(feature3ds[g_], dtype=np.float64, copy=True), np.array(feature2ds[g_], dtype=np.float64, copy=True)
                    remapped_ = bool(self.mutate_inputs)

                    def lazy_level(f3c=f3c, f2c=f2c, remapped_=remapped_):
                        self.lazy_levels_on_read = getattr(self, "lazy_levels_on_read", 0) + 1
                        return self._exact_level_of(f3c, f2c, remapped_)
        elif tri1s is None and tri2s is None and not _single and F > self.PIPELINE_CHUNK:
            raw, status, level, counts, host_errors, last = self._stream_chunks(feature3ds, feature2ds)
        else:
            st = self._chunk_begin(feature3ds, feature2ds, 0, tri1s, _fast=self._host_replay)
            self._chunk_vote(st, tri2s, 0)
            raw, status, level, counts, host_errors = self._chunk_scale(st, tri2s, stage, keep=True)
            last = st
        self.last_status, self.last_counts, self.last_raw_scale = status, counts, raw
        if _raw_only:
            stream.free_blocks(last)
            return raw, status, level, host_errors
        hint = None
        if stage and F == 1 and isinstance(last, dict) and last.get("filtered_queue") is not None and last.get("out") is not None \
                and "filtered" in last["out"].bufs and last["filtered_queue"] == list(self.scale_queue):
            hint = last["out"].get("filtered")
        filtered, stds, n_ok, raise_late = self._push(raw, status, level, host_errors, _single, filtered_hint=hint)
        if lazy_level is not None and n_ok:
            self.__dict__["_level_thunk"] = lazy_level          # (the value _push stored is the kernel's own sum: see height_level)
        if n_ok and stage:
            self._store_flat_feature(last["pf"], last["out"], feature3ds, feature2ds, last["masks"], n_ok - 1, status[n_ok - 1])
        elif n_ok and self.LAZY_FLAT_FEATURE and status[n_ok - 1] not in (K.ST_NO_FLAT, K.ST_TOO_FEW):
            f3c = np.array(feature3ds[n_ok - 1], dtype=np.float64, copy=True)          # (after the in-place remap, if any: :414)
            f2c = np.array(feature2ds[n_ok - 1], dtype=np.float64, copy=True)
            st_, mut_ = status[n_ok - 1], bool(self.mutate_inputs)
            self.__dict__["_flat_thunk"] = lambda: self._flat_feature_of(f3c, f2c, st_, mutate=mut_)
        elif n_ok:
            self._flat_feature_of(feature3ds[n_ok - 1], feature2ds[n_ok - 1], status[n_ok - 1])
        stream.free_blocks(last)
        raise_late()
        return filtered, stds

    # -- one chunk of frames through the stages; the Delaunay calls are submitted to the pool and collected later
    def _chunk_begin(self, f3s, f2s, k, tri1s=None, _packed=None, _remapped=False, _exact_all=False, _fast=False, _eng=None):
        """Vanishing-row filter + packing (:252-254) and the start of the first triangulation (:257), on the host."""
        if _packed is not None:
            pf = _packed                                               # (packed — and the caller's arrays remapped — already)
        elif _remapped:
            # the caller's arrays were remapped in place by an earlier pass over them (:414): pack them as they are and
            # run the chunk on the identity-remap engine
            pf = packing.pack_features(f3s, f2s, self.vanish)
        else:
            pf = packing.pack_features(f3s, f2s, self.vanish)      # raw values, packed BEFORE the in-place remap below
        if self.mutate_inputs and _packed is None and not _remapped:
            for f3 in f3s:
                if isinstance(f3, np.ndarray) and f3.size:
                    self.feature_remap(f3)                                   # :414
        pf.extra["canonical"] = self.check_triangle == "fixed"       # rows are brought to canonical form when attached
        if tri1s is not None:
            h1 = tri1s
        else:
            h1 = packing.submit_tri1(pf, self.delaunay_workers, slot=stream.SLOT_CHUNK + k % stream.CHUNK_SLOTS, fast=_fast)
        # (_fast: the host replay of Qhull's run instead of SciPy where it accepts the set — the default estimator's own host steps;
        # an estimator constructed with triangulation="scipy" never sets it)
        st = {"pf": pf, "h1": h1, "n": len(f3s), "out": None, "dbatch": None, "masks": None, "exact_all": bool(_exact_all),
              "fast": bool(_fast)}
        if _eng is not None:
            st["eng"] = _eng
        elif _remapped:
            st["eng"] = self._plain_engine()
        return st

    def _chunk_vote(self, st, tri2s, k):
        """First triangulation in, vote on the GPU (:151-167), start of the second triangulation (:266)."""
        self._chunk_vote_start(st, tri2s)
        if tri2s is None:
            self._chunk_vote_finish(st, stream.SLOT_CHUNK_TRI2 + k % stream.CHUNK_SLOTS)

    def _chunk_vote_start(self, st, tri2s=None):
        """The first half of ``_chunk_vote``: the first triangulation attached, the batch uploaded, the vote LAUNCHED and the download
        of its counters queued behind it — nothing is waited for."""
        eng = st.get("eng") or self.engine
        ctx, pf = eng.ctx, st["pf"]
        packing.attach_tri1(pf, st["h1"], self.delaunay_workers)
        cap = int(ctx.lib.mvosr_max_lds_features())
        st["dense"] = pf.max_feat > cap
        if st["dense"]:
            # dense frames gather from global memory: lay the batch out for the tiled kernel (results are
            # order-independent; vertex order inside triangle rows is untouched)
            packing.apply_tile_order(pf)
        st["dbatch"] = DeviceBatch(ctx, pf, with_tri2=False, exact_all=st.get("exact_all", False))
        if tri2s is None:
            vote_out = DeviceOutputs(ctx, st["dbatch"], counts=True, stage=True)
            eng.outlier_vote_batch(st["dbatch"], vote_out)
            vote_out.mark_done()
            st["vote_out"] = vote_out
        else:
            if any(p is not None for p in (pf.extra.get("perm") or [])):
                raise ValueError("precomputed tri2s for dense (re-ordered) frames need the vote mask: pass tri1s only")
            st["h2"] = tri2s

    def _chunk_vote_finish(self, st, slot, background=False):
        """The second half: the vote's counters (waited for), the keep masks (:166), the start of the second triangulation (:266)."""
        pf, vote_out = st["pf"], st.pop("vote_out")
        counters = vote_out.get("vote_counters")
        st["masks"] = [counters[pf.frame_slice(f)] >= 0 for f in range(st["n"])]             # :166
        if self.verbose:
            for m in st["masks"]:
                print('feature rejected ', int(np.sum(~m)))
                print('feature left     ', int(np.sum(m)))
        vote_out.free()
        st["h2"] = packing.submit_tri2(pf, st["masks"], self.delaunay_workers, slot=slot, fast=st.get("fast", False), background=background)

    def _chunk_scale(self, st, tri2s, stage, keep=False):
        """Second triangulation in, the fused GPU stages (:225-248, :324-354, :419), results to the host."""
        self._chunk_scale_start(st, stage)
        return self._chunk_scale_finish(st, stage, keep=keep)

    def _chunk_scale_start(self, st, stage):
        """The first half of ``_chunk_scale``: the second triangulation attached (waited for), its rows uploaded, the fused stages
        LAUNCHED and the download of their results queued behind them."""
        eng = st.get("eng") or self.engine
        ctx, pf = eng.ctx, st["pf"]
        # dense frames: rows renumbered over the features, so that the kernel need not compact (less HBM traffic)
        packing.attach_tri2(pf, st["h2"], st["masks"], self.delaunay_workers,
                            feature_ids=(st["masks"] is not None and st["dense"]))
        st["dbatch"].set_tri2(pf)
        out = DeviceOutputs(ctx, st["dbatch"], counts=True, stage=stage)
        eng.scale_batch(st["dbatch"], out)
        out.mark_done()
        st["out"] = out

    def _chunk_scale_finish(self, st, stage, keep=False):
        """The second half: the results (waited for), the exact levels around the batch's first error."""
        eng = st.get("eng") or self.engine
        pf, out = st["pf"], st["out"]
        host_errors = dict(pf.extra["tri2_errors"])                           # QhullError at :266
        host_errors.update(pf.extra["tri1_errors"])                           # ... or already at :257
        res = (out.get("raw_scale"), out.get("status"), out.get("height_level"), out.get("counts"))
        if not stage:
            res = (res[0], res[1], self._exact_after(eng, st["dbatch"], out, res[1], res[2], host_errors), res[3])
        st["out"] = out
        if not keep:
            stream.free_blocks(st)
        return res + (host_errors,)

    def _exact_after(self, eng, db, out, status, level, host_errors, skip=()):
        """The product (HOT) kernel leaves ``height_level`` as its own fixed-order sum wherever the level decides nothing in
        the frame itself; the frames whose level a LATER step reads are finished in the exact mode by the launch itself
        (``engine.exact_mask_of``: a chunk's last level-setting frame, the frame before a three-feature frame).  What only
        the results can tell is a frame that RAISES: the estimator then keeps the level of the last frame that reached :241
        — the frame before the chunk's first error, and that frame itself when it was its road model that raised
        (:343-344 come after :241).  Those one or two frames are redone here, in ONE masked launch; ``skip``: frames whose
        values came from an all-exact re-run already.  Returns the chunk's levels."""
        status = np.asarray(status)
        bad = np.isin(status, K.ERROR_STATUSES)
        for f in host_errors:
            bad[f] = True
        if not bad.any():
            return level
        e = int(np.argmax(bad))
        mask = np.zeros(len(status), dtype=np.uint8)
        setters = np.nonzero(~np.isin(status[:e], (K.ST_TOO_FEW,) + tuple(K.ERROR_STATUSES)))[0]
        if len(setters):
            mask[int(setters[-1])] = 1
        if status[e] in (K.ST_ERR_LEFT, K.ST_ERR_RIGHT) and e not in host_errors:
            mask[e] = 1
        for f in skip:
            mask[int(f)] = 0
        if not mask.any():
            return level
        db.set_exact_mask(mask)
        eng.scale_batch(db, out, masked=True)
        self._masked_launched = True
        eng.ctx.sync()
        new = out.get("height_level")
        level = np.array(level, copy=True)
        level[mask != 0] = new[mask != 0]
        return level

    # -- vote="reliability" / selection="tri_graph": the staged path with the reference's commented alternatives in place of its
    # live lines (:259 for :260, :589 at :273)
    def _chunk_staged(self, f3s, f2s, tri1s=None, stage=False, _remapped=False, _distribution=None):
        """One chunk of frames: vanishing-row filter, packing and Delaunay #1 on the host (SciPy's rows verbatim: the reliability
        vote reads their ORDER, :91-98), the configured vote on the device (mvosr_reliability_batch or mvosr_outlier_vote_batch),
        the survivors compacted and Delaunay #2 on the host (:263-267), then the survivors as frames of their own.
        selection="tri": no first triangulation, so every one of them passes the scale kernel's own vote, the arrangement of
        ``feature_selection_by_tri`` — through mvosr_scale_batch (:225-248, :324-354, :419), every frame in the exact mode.
        selection="tri_graph": ``_select_tri_graph``.  Returns ``(raw, status, level, counts, host_errors, state)``.
        ``_distribution`` (an engine; ``check_full_distribution``, :562-599): on that engine, the reliability vote (:575) and
        ``feature_selection_by_tri`` (:588) on SciPy's rows as they come, whatever the estimator was built with."""
        F = len(f3s)
        eng = _distribution if _distribution is not None else (self._plain_engine() if _remapped else self.engine)
        ctx = eng.ctx
        pf = packing.pack_features(f3s, f2s, self.vanish)             # raw values, packed BEFORE the in-place remap below
        if self.mutate_inputs and not _remapped:
            for f3 in f3s:
                if isinstance(f3, np.ndarray) and f3.size:
                    self.feature_remap(f3)                             # :414
        reliability = self.vote == "reliability" or _distribution is not None
        pf.extra["canonical"] = (not reliability) and self.check_triangle == "fixed"
        packing.attach_tri1(pf, tri1s if tri1s is not None else packing.submit_tri1(pf, self.delaunay_workers, slot=stream.SLOT_CHUNK),
                            self.delaunay_workers)
        host_errors = dict(pf.extra["tri1_errors"])                    # QhullError at :257
        db = DeviceBatch(ctx, pf, with_tri2=False)
        rout = ReliabilityOutputs(ctx, db) if reliability else DeviceOutputs(ctx, db, counts=True, stage=True)
        try:
            if reliability:
                eng.reliability_batch(db, rout)
                rel, keep, vote_status = rout.get("reliability"), rout.get("keep"), rout.get("status")
            else:
                eng.outlier_vote_batch(db, rout)
                ctx.sync()
                keep, vote_status = np.where(rout.get("vote_counters") >= 0, 0, -1), np.zeros(F, dtype=np.int32)      # :166
        finally:
            rout.free()
            db.free()
        masks = [keep[pf.frame_slice(f)] == 0 for f in range(F)]      # :145
        if reliability:
            self.last_reliability = [rel[pf.frame_slice(f)] for f in range(F)]    # (of the call's last chunk)
        if self.verbose:
            for f, m in enumerate(masks):
                if len(m) and f not in host_errors:
                    if reliability:
                        r = self.last_reliability[f]
                        print('reliability', np.min(r), np.median(r), np.max(r))
                    print('feature rejected ', int(np.sum(~m)))
                    print('feature left     ', int(np.sum(m)))
        raw, level = np.full(F, np.nan), np.full(F, np.nan)
        status = np.full(F, K.ST_ERR_EMPTY, dtype=np.int32)
        counts = np.zeros((F, _lib.N_COUNTS), dtype=np.int32)
        cnt = np.asarray(pf.feat_cnt)
        status[cnt == 3] = K.ST_TOO_FEW                                 # :263-270 (the LENGTH of the mask)
        counts[cnt == 3, K.CNT_VALID] = 3
        status[np.asarray(vote_status[:F]) != 0] = K.ST_ERR_MASK        # (rows the vote refused: precomputed tri1s only)
        todo = [f for f in range(F) if cnt[f] > 3 and f not in host_errors and vote_status[f] == 0]
        pts = packing.survivor_points(pf, masks)
        fixed = self.check_triangle == "fixed" and _distribution is None
        rows = packing.delaunay_submit([pts[f] for f in todo], self.delaunay_workers, slot=stream.SLOT_CHUNK_TRI2, canonical=fixed).get()   # :266
        go = []
        for f, t in zip(todo, rows):
            if isinstance(t, Exception):
                host_errors[f] = t                                       # QhullError at :266
            else:
                go.append((f, np.ascontiguousarray(t, dtype=np.int32)))
        selected = np.zeros(max(pf.total_padded, 1), dtype=np.uint8)
        if go and self.selection == "tri_graph" and _distribution is None:
            self._select_tri_graph(eng, pf, masks, go, raw, status, level, counts, selected)
        elif go:
            kept = np.array([int(np.count_nonzero(masks[f])) for f, _ in go], dtype=np.int32)
            # (exactly three survivors are one triangle to the reference, :266, but "too few features" to the scale kernel, which reads
            # a frame's size as the LENGTH of the mask, :263: such a frame carries its first survivor once more, named by no row)
            cnt2 = np.maximum(kept, 4).astype(np.int32)
            off2, total2 = packing.pack_layout(cnt2)
            planes = {k: np.zeros(total2) for k in "xyzvu"}
            for g, (f, _) in enumerate(go):
                sl, m = pf.frame_slice(f), masks[f]
                for k in "xyzvu":
                    planes[k][off2[g]:off2[g] + kept[g]] = getattr(pf, k)[sl][m]      # :264-265
                    planes[k][off2[g] + kept[g]:off2[g] + cnt2[g]] = planes[k][off2[g]]
            pf2 = packing.PackedFrames(len(go), off2, cnt2, planes["x"], planes["y"], planes["z"], planes["v"], planes["u"],
                                       [None] * len(go), max_feat=int(cnt2.max()))
            pf2.extra["canonical"] = fixed
            pf2.extra["tri1_is_canonical"] = True                         # (no rows: nothing to bring into canonical form)
            packing.attach_tri1(pf2, [np.zeros((0, 3), dtype=np.int32)] * len(go))          # no vote: every survivor stays
            packing.attach_tri2(pf2, [t for _, t in go], [np.ones(int(c), dtype=bool) for c in cnt2])
            db2 = DeviceBatch(ctx, pf2, exact_all=True)
            out2 = DeviceOutputs(ctx, db2, counts=True, stage=stage)
            try:
                eng.scale_batch(db2, out2, exact=True)
                r2, s2, l2, c2 = out2.get("raw_scale"), out2.get("status"), out2.get("height_level"), out2.get("counts")
                sel2 = out2.get("selected") if stage else None
            finally:
                out2.free()
                db2.free()
            for g, (f, _) in enumerate(go):
                raw[f], status[f], level[f], counts[f] = r2[g], s2[g], l2[g], c2[g]
                counts[f, K.CNT_VALID] = kept[g]
                if sel2 is not None:
                    o = int(pf.feat_off[f])
                    selected[o:o + kept[g]] = sel2[pf2.frame_slice(g)][:kept[g]]      # over the survivors, as the fused path lays it out
        st = {"pf": pf, "n": F, "masks": masks, "dbatch": None, "out": _HostOutputs({"selected": selected})}
        return raw, status, level, counts, host_errors, st

    def _select_tri_graph(self, eng, pf, masks, go, raw, status, level, counts, selected):
        """selection="tri_graph" for the frames ``go`` = [(frame, SciPy's second triangulation)] of a staged chunk: ONE
        mvosr_tri_graph_batch launch over the survivors' frames (from-points form: :177-222), the selected y' lists packed on the
        host, mvosr_road_model_batch with the launch's height_level as the fallback level (:324-354, :419); an empty selection
        takes its no-flat branch (:277-279, :420-422).  Fills the chunk's per-frame arrays in place."""
        ctx = eng.ctx
        kept = np.array([int(np.count_nonzero(masks[f])) for f, _ in go], dtype=np.int32)
        off2, total2 = packing.pack_layout(kept)
        planes = {k: np.zeros(total2) for k in "xyzvu"}
        for g, (f, _) in enumerate(go):
            sl, m = pf.frame_slice(f), masks[f]
            for k in "xyzvu":
                planes[k][off2[g]:off2[g] + kept[g]] = getattr(pf, k)[sl][m]          # :264-265
        pf2 = packing.PackedFrames(len(go), off2, kept, planes["x"], planes["y"], planes["z"], planes["v"], planes["u"],
                                   [None] * len(go), max_feat=int(kept.max()))
        pf2.extra["canonical"] = False
        pf2.extra["tri1_is_canonical"] = True
        packing.attach_tri1(pf2, [np.zeros((0, 3), dtype=np.int32)] * len(go))
        packing.attach_tri2(pf2, [t for _, t in go], [np.ones(int(c), dtype=bool) for c in kept])
        db2 = DeviceBatch(ctx, pf2)
        tout = TriGraphOutputs(ctx, db2)
        try:
            eng.tri_graph_batch(db2, tout)
            ctx.sync()
            st2, lvl2, sel2 = tout.get("status"), tout.get("height_level"), tout.get("selected")
            p_road, p_initial, n_rounds, n_flat, n_valid = (tout.get(k) for k in ("p_road", "p_initial", "n_rounds", "n_flat", "n_valid"))
        finally:
            tout.free()
            db2.free()
        toff = pf2.tri2_off
        self.last_tri_graph = [{"p_road": p_road[toff[g]:toff[g + 1]], "p_initial": p_initial[toff[g]:toff[g + 1]], "n_rounds": int(n_rounds[g])}
                               for g in range(len(go))]                       # (of the call's last chunk, one per frame that reached :273)
        cp, sp = float(eng.params.cos_pitch), float(eng.params.sin_pitch)
        ys, good = [], []
        for g, (f, _) in enumerate(go):
            counts[f, K.CNT_VALID] = kept[g]
            if self.verbose and st2[g] == 0:
                print('triangle left ', int(n_flat[g]), 'from', int(toff[g + 1] - toff[g]))
                print('triangle left final', int(n_valid[g]), 'from', int(toff[g + 1] - toff[g]))
            if st2[g] != 0:
                status[f] = st2[g]                                            # :181 raises; rows the kernel refuses
                continue
            sl2 = pf2.frame_slice(g)
            pick = sel2[sl2] != 0
            ys.append(pf2.y[sl2][pick] * cp - pf2.z[sl2][pick] * sp)          # :391 with the engine's doubles, as the kernels remap at load
            good.append(g)
            o = int(pf.feat_off[f])
            selected[o:o + kept[g]] = sel2[sl2]                               # over the survivors, as the fused path lays it out
        if not good:
            return
        cnt3 = np.array([len(y) for y in ys], dtype=np.int32)
        off3, total3 = packing.pack_layout(cnt3)
        yplane = np.zeros(total3)
        for y, o in zip(ys, off3):
            yplane[o:o + len(y)] = y
        zero = np.zeros(total3)
        pf3 = packing.PackedFrames(len(good), off3, cnt3, zero, yplane, zero, zero, zero, [None] * len(good), max_feat=max(int(cnt3.max()), 1))
        db3 = DeviceBatch(ctx, pf3, with_tri2=False)
        out3 = DeviceOutputs(ctx, db3, counts=True)
        try:
            eng.road_model_batch(db3, out3, np.ascontiguousarray(lvl2[good], dtype=np.float64))
            r3, s3, c3 = out3.get("raw_scale"), out3.get("status"), out3.get("counts")
        finally:
            out3.free()
            db3.free()
        for k, g in enumerate(good):
            f = go[g][0]
            raw[f], status[f], level[f] = r3[k], s3[k], lvl2[g]
            keep_valid = counts[f, K.CNT_VALID]
            counts[f] = c3[k]
            counts[f, K.CNT_VALID], counts[f, K.CNT_TRI_PITCH], counts[f, K.CNT_TRI_VALID] = keep_valid, n_flat[g], n_valid[g]

    def _stream_staged(self, feature3ds, feature2ds, tri1s, tri2s, stage):
        """A call's frames through ``_chunk_staged`` in chunks of ``PIPELINE_CHUNK``."""
        if tri2s is not None:
            raise ValueError("vote='reliability' / selection='tri_graph': precomputed tri2s would have to be built on the configured "
                             "vote's survivors; pass tri1s only")
        F, C = len(feature3ds), self.PIPELINE_CHUNK
        res, last = [], None
        for a in range(0, F, C):
            b = min(F, a + C)
            r = self._chunk_staged(feature3ds[a:b], feature2ds[a:b], None if tri1s is None else tri1s[a:b], stage)
            res.append(r[:5])
            last = r[5]
        host_errors = {}
        for k, r in enumerate(res):
            host_errors.update({k * C + f: e for f, e in r[4].items()})
        return tuple(np.concatenate([r[k] for r in res]) for k in range(4)) + (host_errors, last)

    def _stream_chunks(self, feature3ds, feature2ds, depth=2):
        F, C = len(feature3ds), self.PIPELINE_CHUNK
        bounds = [(a, min(F, a + C)) for a in range(0, F, C)]
        n = len(bounds)
        S = [None] * n
        results = [None] * n

        def begin(k):
            a, b = bounds[k]
            S[k] = self._chunk_begin(feature3ds[a:b], feature2ds[a:b], k)

        for k in range(min(depth, n)):
            begin(k)
        for k in range(n):
            self._chunk_vote(S[k], None, k)            # waits for tri1 of chunk k; tri2 of chunk k goes to the pool
            if k + depth < n:
                begin(k + depth)
            if k >= 1:
                results[k - 1] = self._chunk_scale(S[k - 1], None, False)
                S[k - 1] = None
        results[n - 1] = self._chunk_scale(S[n - 1], None, False, keep=True)
        raw = np.concatenate([r[0] for r in results])
        status = np.concatenate([r[1] for r in results])
        level = np.concatenate([r[2] for r in results])
        counts = np.concatenate([r[3] for r in results])
        host_errors = {}
        for (a, _), r in zip(bounds, results):
            host_errors.update({a + f: e for f, e in r[4].items()})
        return raw, status, level, counts, host_errors, S[n - 1]

    def _lower_points(self, f2):
        """A frame's pixels below the vanishing row (:252-254), contiguous — what the first Delaunay call sees."""
        f2 = np.asarray(f2, dtype=np.float64)
        return np.ascontiguousarray(f2[f2[:, 1] > self.vanish]) if f2.ndim == 2 and f2.size else np.zeros((0, 2))

    def _second_engine(self):
        """A second context on the same device (its own compute and upload streams, workspace and caches) with the same parameters."""
        if getattr(self, "_engine2", None) is None:
            self._engine2 = ScaleEngine(self.absolute_reference, ctx=_lib.Context(self.engine.ctx.device), camera_pitch=self.camera_pitch,
                                        check_triangle=self.check_triangle)
        return self._engine2

    def _redo_engine(self, remapped):
        """The engine on the re-runs' context (_redo_context) for the frames a device triangulation declined; ``remapped``: the
        caller's arrays hold the remapped values already (:414), the engine's remap is the identity."""
        engines = self.__dict__.setdefault("_redo_engines", {})
        if bool(remapped) not in engines:
            engines[bool(remapped)] = ScaleEngine(self.absolute_reference, ctx=self._redo_context(), camera_pitch=0.0 if remapped else self.camera_pitch,
                                                  check_triangle=self.check_triangle)
        return engines[bool(remapped)]

    def _redo_sub(self, f3s, f2s, rows, remapped):
        """A re-run's batch of frames whose first triangulations (``rows``, canonical form from the workers) are back: packed, on the
        re-runs' engine, every stage in the exact mode."""
        sub = self._chunk_begin(f3s, f2s, 0, tri1s=rows, _remapped=remapped, _exact_all=True, _fast=self._host_replay,
                                _eng=self._redo_engine(remapped) if self.GPU_REDO_CONTEXT else None)
        sub["pf"].extra["tri1_is_canonical"] = self.check_triangle == "fixed"
        return sub

    def _chunk_gpu(self, f3s, f2s, stage, tables=False, eng=None, single_exact=False, hot_only=False, lazy_last=False, host_exact=False,
                   early_status=False):
        """One chunk with both triangulations built on the device: pack (C packer, straight into page-locked memory) ->
        ONE upload -> Delaunay #1, vote, Delaunay #2, scale kernel, road model, the exact re-runs known in advance and
        the download of the results, all queued; nothing is waited for here (``_chunk_gpu_finish`` does)."""
        from .engine import frame_tables, pack_upload_native
        eng = eng or self.engine
        ctx = eng.ctx
        if tables is False:             # (not looked up by the caller yet)
            tables = frame_tables(f3s, f2s, remap_in_place=bool(self.mutate_inputs)) if len(f3s) > 0 else None
        native = tables is not None
        blk = None
        if native:
            remap = (eng.params.cos_pitch, eng.params.sin_pitch) if self.mutate_inputs else None
            pf, blk = pack_upload_native(ctx, f3s, f2s, self.vanish, remap, tables=tables, lazy_last=lazy_last)     # (:252-254, and :414 on the caller's arrays)
        else:
            pf = packing.pack_features(f3s, f2s, self.vanish)          # raw values, packed BEFORE the in-place remap below
            if self.mutate_inputs:
                for f3 in f3s:
                    if isinstance(f3, np.ndarray) and f3.size:
                        self.feature_remap(f3)                                   # :414
        pf.extra["canonical"] = self.check_triangle == "fixed"
        st = {"pf": pf, "n": len(f3s), "out": None, "dbatch": None, "masks": None, "gpu": True, "stage": stage,
              "remapped": bool(self.mutate_inputs), "engine": eng}
        cap = packing.delaunay_gpu_max_points() if self.check_triangle == "fixed" else packing.delaunay_qhull_max_points()
        if pf.max_feat > cap or pf.n_frames == 0:
            st["gpu"] = False                                                # frames the device stage does not take: the host's path
            if blk is not None:
                blk.free()
            return st
        tri1_rows = None
        if single_exact:
            # the per-frame call of the reference-exact path: SciPy's own first triangulation (:257) from the host — the vote
            # reads the rotation of its rows
            tri1_rows = []
            try:
                for f2 in f2s:
                    f2 = np.asarray(f2, dtype=np.float64)
                    pts = f2[f2[:, 1] > self.vanish]                              # :252-254
                    if len(pts) < 5:
                        raise ValueError("too few points for the device path")
                    tri1_rows.append(packing.delaunay_simplices_fast(pts) if self._host_replay else packing.delaunay_simplices(pts))
            except Exception:              # (QhullError, tiny frames: the host's path deals with them as the reference does)
                st["gpu"] = False
                if blk is not None:
                    blk.free()
                return st
        st["tri1_rows"] = tri1_rows
        db = DeviceBatch(ctx, pf, with_tri2=False, device_triangulation=True, uploaded=blk, lazy_last=lazy_last)
        try:
            db.triangulate(eng, standin=self.GPU_EXACT_STANDIN and (single_exact or not stage), tri1_rows=tri1_rows,
                           early_status=early_status and tri1_rows is None)
        except _lib.MvosrAllocError:
            # the triangulation kernels' workspace (frames x largest frame) did not fit next to whatever else lives on the
            # device: nothing was launched — this chunk takes the host's triangulations (MVOSR_ERR_ALLOC)
            db.free()
            st["gpu"] = False
            self.alloc_fallbacks = getattr(self, "alloc_fallbacks", 0) + 1
            return st
        out = DeviceOutputs(ctx, db, counts=True, stage=stage)
        st["hot_only"] = bool((single_exact and getattr(db, "standin", False)) or hot_only)
        # host_exact (batches of the reference-exact path with a stand-in second triangulation): the product kernels alone, and the
        # few frames the exact pass would have redone — they come back MVOSR_ST_REDO — or whose level a later step reads (the exact
        # mask) go through the HOST path with the call's declined frames (_chunk_gpu_finish): on the device their Qhull rows are one
        # wavefront per frame for a whole run — 23 ms at the end of EVERY chunk for a handful of frames, the bulk of a call's tail
        st["host_exact"] = bool(host_exact and getattr(db, "standin", False) and not stage)
        if st["host_exact"]:
            from .engine import exact_mask_of
            st["exact_mask_host"] = exact_mask_of(pf.feat_cnt, lazy_last=lazy_last)
        eng.scale_batch(db, out, hot_only=st["hot_only"] or st["host_exact"])      # (else: the frames whose level a later step reads are on the batch's exact mask)
        if stage and pf.n_frames == 1 and "filtered" in out.bufs:
            # the per-frame call: the window median (:396-400) of this frame's raw scale over the estimator's queue, queued behind the
            # kernels that produce it — its result arrives with theirs instead of costing an upload, a launch and a download after them
            # (64 us per call).  Used when the frame turns out to be an ordinary one (_push decides).
            eng.window_median(out.bufs["raw_scale"].ptr, 1, self.window_size, list(self.scale_queue), out.bufs["filtered"].ptr)
            st["filtered_queue"] = list(self.scale_queue)
        if stage or not self.GPU_SIDE_DOWNLOADS:
            out.prefetch()
            db.prefetch_info()
        else:
            # (streamed batches: no download parked on a copy engine behind the chunk's kernels — a copy kernel into page-locked memory)
            out.mark_done()
            db.mark_info_done()
        db.mark()                     # the chunk's last launch is queued: its blocks' next users need not wait for later chunks
        st["dbatch"], st["out"] = db, out
        return st

    def _chunk_gpu_finish(self, st, f3s, f2s, keep=False, defer=None):
        """Results of a chunk started by ``_chunk_gpu``; frames whose triangulation the device stage declined (degenerate
        point sets, fewer than 3 points) are redone through the host's path (SciPy's rows, canonical form in "fixed" mode).
        ``defer`` (the call's re-run records; streamed batches): the re-run is only STARTED here — its first SciPy calls go to the
        worker pool — and a record is appended; ``_finish_reruns`` finishes it.  Returns the chunk's ``[raw, status, level, counts,
        host_errors]`` (a list: a deferred completion fills the declined frames' entries in)."""
        eng = st.get("engine") or self.engine
        pf = st["pf"]
        stage = st["stage"]
        stream.advance(defer or ())         # (host work for earlier chunks' re-runs, before this chunk's results are waited for)
        if not st["gpu"]:
            sub = self._chunk_begin(f3s, f2s, 0, _remapped=st["remapped"])
            self._chunk_vote(sub, None, 0)
            res = self._chunk_scale(sub, None, stage, keep=True)
            st.update(out=sub["out"], dbatch=sub["dbatch"], masks=sub["masks"], pf=sub["pf"])
            if not keep:
                stream.free_blocks(st)
            return list(res)
        db, out = st["dbatch"], st["out"]
        if defer is not None and not stage:
            # (the call's last chunk: whatever its first triangulation declined is known behind THAT kernel — the frames' SciPy calls
            # start now, under the chunk's vote, second triangulation and product kernels, instead of after them)
            s1e = db.early_status()
            if s1e is not None and s1e.any():
                ef = np.nonzero(s1e != 0)[0]
                early = st["early"] = self._rerun(st, f3s, f2s, ef, packing.delaunay_submit(
                    [self._lower_points(f2s[f]) for f in ef], self.delaunay_workers, slot=stream.SLOT_EARLY, fast=self._host_replay,
                    canonical=self.check_triangle == "fixed", background=True))
                self.redo_early_status_hits = getattr(self, "redo_early_status_hits", 0) + 1
                if self.GPU_REDO_EARLY and len(ef) <= self.GPU_REDO_EARLY_MAX:
                    # ... and this thread has nothing else to do for the call's last chunk: it takes those frames through their first
                    # triangulation (waited for: the chunk's other kernels are running), the vote (on the re-runs' context) and the start
                    # of their second triangulation NOW, so that the call's end finds only their product kernels left to launch
                    early.sub = self._redo_sub([f3s[f] for f in ef], [f2s[f] for f in ef], early.h1.get(), st["remapped"])
                    self._chunk_vote_start(early.sub)
                    self._chunk_vote_finish(early.sub, stream.SLOT_EARLY_TRI2, background=True)
        # (re-runs of earlier chunks are under way: instead of sleeping until this chunk's results arrive — tens of ms with the
        # reference's vote — the thread takes each step of a record the moment its inputs are there)
        stream.advance_while(defer or (), lambda: not (db.info.ready() and out.ready()))
        s1, s2 = db.triangulation_status()
        redo = np.nonzero((s1 != 0) | (s2 != 0))[0]
        res = [out.get("raw_scale"), out.get("status"), out.get("height_level"), out.get("counts"), {}]
        self.last_declined = len(redo)
        self.declined_total += len(redo)
        if st.get("host_exact"):
            # the exact pass's frames of this chunk: listed by the kernels themselves (a flat triangle within the guard band of the
            # level, a pitch inside the 1e-9 band, a level that is the result) or on the exact mask
            extra = np.nonzero((res[1] == _lib.ST_REDO) | (st["exact_mask_host"] != 0))[0]
            extra = extra[~np.isin(extra, redo)]
            # (the host's route costs two replays of Qhull's run per frame, ~1.7 ms, spread over the Delaunay workers; the device's one
            # masked relaunch, ~25 ms and a wait, however many frames)
            if len(extra) > min(self.GPU_EXACT_HOST_REDO_MAX, 16 * max(1, packing.resolve_workers(self.delaunay_workers))):
                # many of them (adversarial data): the device's exact pass after all — one masked relaunch (Qhull's rows by the list
                # kernel, the EXACT variant, the road model), waited for
                mask = np.zeros(pf.n_frames, dtype=np.uint8)
                mask[extra] = 1
                db.set_exact_mask(mask)
                eng.scale_batch(db, out, masked=True)
                eng.ctx.sync()
                new = [out.get("raw_scale"), out.get("status"), out.get("height_level"), out.get("counts")]
                for k in range(4):
                    res[k][extra] = new[k][extra]
                db.info.invalidate()                             # (the statuses read above are the block's cached copy)
                s2n = db.bufs["dt2_status"].download()
                late = extra[(s2n[extra] != 0)]                  # (Qhull's replay declined one there: the host's path, below)
                redo = np.union1d(redo, late).astype(redo.dtype) if len(late) else redo
                self.exact_redone_on_device = getattr(self, "exact_redone_on_device", 0) + len(extra)
            elif len(extra):
                redo = np.union1d(redo, extra).astype(redo.dtype)
                self.exact_redone_on_host = getattr(self, "exact_redone_on_host", 0) + len(extra)
        early = st.pop("early", None)
        handle = None
        if len(redo) and defer is not None and not stage:
            # Streamed batches (round 6): only the declined frames' FIRST SciPy calls are started here — on the worker pool when the
            # estimator has one (delaunay_workers), under the GPU's queued work —; the re-run itself waits for the call's last chunk
            # and is ONE small batch over every declined frame of the call, on a context of its own.  Its launches are waited for,
            # and while replays of other chunks hold every CU's LDS for a whole frame (30 ms) a vote or scale workgroup waits that
            # long for a slot: round 5 ran the re-run in each chunk's epilogue on the chunk's own stream (72 declined frames in
            # 16 384: 53 k -> 30 k frames/s); on its own context but still between the chunks 80 declined frames cost 96 -> 66 k
            # (and 529 -> 93 k in the fixed mode, whose chunks are short).
            have = set(int(f) for f in early.redo) if early is not None else set()
            rest = [k for k, f in enumerate(redo) if int(f) not in have]
            handle = packing.delaunay_submit([self._lower_points(f2s[redo[k]]) for k in rest], self.delaunay_workers,
                                             slot=stream.SLOT_DEFER + len(defer),
                                             fast=self._host_replay, canonical=self.check_triangle == "fixed", background=True)
            if early is not None:
                where = {int(f): k for k, f in enumerate(redo)}
                handle = packing._JoinedHandle(len(redo), [([where[int(f)] for f in early.redo], early.h1), (rest, handle)])
        rec = self._rerun(st, f3s, f2s, redo, handle, res=res, s12=(s1, s2), keep=keep,
                          slot2=stream.SLOT_DEFER_TRI2 + len(defer) if handle is not None else None)
        if early is not None and early.sub is not None:
            if handle is not None and len(redo) == len(early.redo) and np.array_equal(redo, early.redo):
                rec.sub, rec.step, rec.begun = early.sub, 2, True      # (the record continues where the early steps left it)
            else:                                                      # (more frames to redo than the early read knew of: the merged way for all)
                stream.free_blocks(early.sub)
        if handle is not None:
            defer.append(rec)
            if len(defer) >= self.GPU_REDO_MAX_DEFERRED:       # (bounded: a deferred chunk keeps its device blocks and a pool slot)
                self._finish_reruns(defer)
            else:
                stream.advance(defer)                          # (this chunk's results were waited for: earlier records may have moved on)
            return res
        stream.advance(defer or ())
        self._chunk_gpu_complete(rec)
        return res

    def _rerun(self, st, f3s, f2s, redo, h1, slot2=None, **data):
        """The re-run record of chunk ``st``'s frames ``redo`` whose first triangulations ``h1`` has started.  ``slot2`` (deferred
        records of at most GPU_REDO_EARLY_MAX frames): its steps are taken while later chunks run (round 6, LABNOTES 10.11) — a chunk's
        few declined frames (and, in the reference-exact mode, the few frames of its exact pass) need first triangulation -> vote ->
        second triangulation -> product kernels, a chain of two host triangulations and two device round trips: at the call's end that
        chain is 4-8 ms during which nothing else runs, a fifth of a 34 ms call for ONE declined frame.  Once its first triangulations
        are back the record's batch is uploaded and its vote launched on the re-runs' context (the record has begun); once the counters
        are back its second triangulations start on the pool; once those are back its product kernels are launched."""
        rec = stream.Rerun(data.pop("res", None), redo, lambda: (stream.free_blocks(rec.sub), stream.free_blocks(st), stream.wait_out(
            rec.h1, (rec.sub or {}).get("h2"))), st=st, f3s=f3s, f2s=f2s, h1=h1, sub=None, **data)
        if slot2 is None or not (self.GPU_REDO_EARLY and 0 < len(redo) <= self.GPU_REDO_EARLY_MAX):
            return rec

        def begin(wait):
            rec.sub = self._redo_sub([f3s[f] for f in redo], [f2s[f] for f in redo], rec.h1.get(), st["remapped"])
            self._chunk_vote_start(rec.sub)
            rec.begun = True
            self.redo_early_started = getattr(self, "redo_early_started", 0) + 1

        def scale(wait):
            self._chunk_scale_start(rec.sub, False)
            if not wait:
                self.redo_early_launched = getattr(self, "redo_early_launched", 0) + 1     # (only its results are left for the call's end)
        rec.chain = [(lambda: rec.h1.ready(), begin),
                     (lambda: rec.sub["vote_out"].ready(), lambda wait: self._chunk_vote_finish(rec.sub, slot2, background=not wait)),
                     (lambda: rec.sub["h2"].ready(), scale)]
        rec.collect = lambda: self._chunk_scale_finish(rec.sub, False)
        return rec

    def _finish_reruns(self, records):
        """The declined frames of the records' chunks through the host path, results scattered back (stream.finish_all: the begun
        re-runs each finish as their own small batch, the others' frames go through ONE merged re-run); then every chunk's own
        completion."""
        stream.finish_all(records, self._merged_rerun, range(4), 4, then=lambda rec: self._chunk_gpu_complete(rec, merged=True))

    def _merged_rerun(self, records):
        at = [(rec, f) for rec in records for f in rec.redo]
        sub = self._redo_sub([rec.f3s[f] for rec, f in at], [rec.f2s[f] for rec, f in at], [t for rec in records for t in rec.h1.get()],
                             records[0].st["remapped"])
        self._chunk_vote(sub, None, 0)
        out = self._chunk_scale(sub, None, False)
        first = 0
        for rec in records:
            stream.scatter(rec.res, rec.redo, out, range(4), 4, first)
            first += len(rec.redo)

    def _chunk_gpu_complete(self, rec, merged=False):
        """The rest of ``_chunk_gpu_finish``: the declined frames' re-run (unless ``_finish_reruns`` ``merged`` it in already); the
        exact levels around the chunk's first real error; the per-frame call's stage outputs."""
        st, redo, (s1, s2), f3s, f2s, res, keep = rec.st, rec.redo, rec.s12, rec.f3s, rec.f2s, rec.res, rec.keep
        eng = st.get("engine") or self.engine
        pf, stage = st["pf"], st["stage"]
        db, out = st["dbatch"], st["out"]
        raw, status, level, counts, host_errors = res
        if len(redo) and not merged:
            # (every frame of the small re-run in the exact mode: a declined frame's level may be the one a later frame reads)
            sub = self._chunk_begin([f3s[f] for f in redo], [f2s[f] for f in redo], 0, _remapped=st["remapped"], _exact_all=True,
                                    _fast=self._host_replay)
            self._chunk_vote(sub, None, 0)
            r_raw, r_status, r_level, r_counts, r_err = self._chunk_scale(sub, None, False)
            raw[redo], status[redo], level[redo], counts[redo] = r_raw, r_status, r_level, r_counts
            host_errors = {int(redo[k]): e for k, e in r_err.items()}
        if not stage:
            # with the re-run's results merged in: the neighbours of the chunk's first REAL error
            self._masked_launched = False
            level = self._exact_after(eng, db, out, status, level, host_errors, skip=redo)
            if self._masked_launched and getattr(db, "standin", False):
                # stand-in rows: the masked relaunch asked Qhull's replay for the rows of its one or two frames; a frame it declined
                # there (its bits arrive in the second triangulation's status only now) takes the host's path for its level
                db.info.invalidate()                # (s1 / s2 came from the block's cached copy: the relaunch wrote new bits)
                late = np.nonzero((db.bufs["dt2_status"].download() != 0) & (s2 == 0) & (s1 == 0))[0]
                if len(late):
                    sub2 = self._chunk_begin([f3s[f] for f in late], [f2s[f] for f in late], 0, _remapped=st["remapped"], _exact_all=True)
                    self._chunk_vote(sub2, None, 0)
                    _, _, l_level, _, _ = self._chunk_scale(sub2, None, False)
                    level = np.array(level, copy=True)
                    level[late] = l_level
                    self.last_declined += len(late)
                    self.declined_total += len(late)
        if stage:
            c = db.bufs["vote_counters"].download()
            st["masks"] = [c[pf.frame_slice(f)] >= 0 for f in range(pf.n_frames)]
            if len(redo):                        # (per-frame call whose triangulation was declined: stage outputs from the host's path)
                one = self._chunk_begin(f3s, f2s, 0, _remapped=st["remapped"])
                self._chunk_vote(one, None, 0)
                self._chunk_scale(one, None, True, keep=True)
                stream.free_blocks(st)
                st.update(out=one["out"], dbatch=one["dbatch"], masks=one["masks"], pf=one["pf"], filtered_queue=None)
        if not keep:
            stream.free_blocks(st)
        res[2], res[4] = level, host_errors

    def _exact_level_of(self, f3, f2, remapped):
        """NumPy's own ``height_level`` (:239-241) of ONE frame: Qhull's rows (the host replay, SciPy where it declines), every stage in
        the exact mode."""
        sub = self._chunk_begin([f3], [f2], 0, _remapped=remapped, _exact_all=True, _fast=self._host_replay)
        self._chunk_vote(sub, None, 0)
        _, _, lvl, _, _ = self._chunk_scale(sub, None, False)
        return lvl[0]

    def _stream_gpu(self, feature3ds, feature2ds, stage, lazy_last=False, eager_final=False):
        """The batch through the device-triangulation path in chunks: the GPU works on chunk k while this process packs
        chunk k+1 (every launch and copy of a chunk is asynchronous).

        ``lazy_last`` (round 6; the reference-exact path's batches): a chunk's last level-setting frame is NOT put on the exact mask.
        Its level in NumPy's summation order is read by a later step only if the next chunk starts with a three-feature frame
        (:263-270, :420-422) or the caller looks at ``est.height_level`` — and on ordinary data that one frame was the exact pass's
        whole list: Qhull's rows for it are a chain of ~n insertions on ONE wavefront, 23 ms at the end of every chunk, the bulk of a
        call's exposed tail.  Now the frames concerned are remembered (``self._lazy_levels``); the ones a three-feature frame of the
        call reads are finished here, exactly (the host path, one frame each); the call's last one is left to ``height_level``'s
        reader (scale_calculation_batch).  ``eager_final`` (raw_scale_batch: the levels leave this estimator — another rank's first
        frame may read this block's last one): the call's final chunk keeps its mask."""
        F = len(feature3ds)
        self._lazy_levels = set()
        # Larger chunks leave fewer launch tails (32 768 frames of 2000 features: 347 k frames/s in chunks of 2048, 356 k in
        # chunks of 4096; 900 features: 710 k / 756 k, and with the short first chunks 764 k / 807 k in chunks of 4096 / 8192 —
        # profiles/e2e_chunk_sweep.py; the points cap keeps 2000-feature frames at 5000 per chunk)
        exact = self.check_triangle == "reference"
        engines = [self.engine]
        points, full = self.GPU_CHUNK_POINTS, None
        if exact:
            # The Qhull-rows kernel is a chain of ~n dependent insertions per frame (one wavefront each): a launch lasts ~25 ms
            # whether it holds 500 frames or 4 000, and only resident wavefronts fill the GPU — chunks as large as the workspace
            # allows (0.56 KB per point of frames x largest frame), no short first chunks: the host's packing is 1 % of the time
            full, points = int(min(self.GPU_EXACT_CHUNK, F)), self.GPU_EXACT_CHUNK_POINTS
            if self.GPU_EXACT_TWO_CONTEXTS and not stage and F >= 2 * 4096:
                # ... and two contexts (a stream, a workspace and caches each) taking the chunks in turn: while one chunk is in the
                # thin parts of its chain (the launch's tail, the stand-in triangulation, Qhull's rows for the exact pass's few frames
                # — 20 ms at a few hundred wavefronts), the other chunk's replay fills the machine
                engines.append(self._second_engine())
                full = int(min(self.GPU_EXACT_CHUNK // 2, max(4096, ((-(-F // 2)) // 4096) * 4096)))
                points //= 2
        C, ramp = stream.chunk_size(F, self.GPU_CHUNK, self.GPU_MIN_CHUNK, points, [len(x) for x in feature3ds[:64]],
                                    self.GPU_RAMP_FRACTIONS if self.GPU_RAMP and not exact else (), full=full)
        if exact and len(engines) == 2 and self.GPU_EXACT_FIRST_CHUNK and C >= 2 * self.GPU_EXACT_FIRST_CHUNK and self.GPU_EXACT_HOST_REDO:
            # the exact path's head: nothing runs before the first chunk is packed and uploaded (16 ms for 8 192 frames of 2000 features).
            # A short first chunk was a loss while every chunk ended in a 23 ms list replay (LABNOTES 9.14); with the exact pass's
            # frames on the host (host_exact) a chunk has no such tail, and the short chunk's replay runs under the next one's.
            # Not for RAGGED frames: the replay launches its frames largest first (qh_order_kernel), which packs a launch of two rounds
            # of wavefronts well — and a one-round first chunk of ragged frames lasts as long as its longest frame with most of the
            # machine idle: 238 -> 201 k frames/s at 300-1500 features, 110 -> 116 k at 2000, 245 -> 259 k at 900 (profiles/
            # r06_exact_first_chunk_ab.txt).  Ragged: the largest of the call's first frames has more than 1.3 x their mean.
            head = np.fromiter((len(x) for x in feature3ds[:256]), dtype=np.int64, count=min(F, 256))
            if head.max() <= 1.3 * max(head.mean(), 1.0):
                ramp = [int(self.GPU_EXACT_FIRST_CHUNK)]
        # (the exact path: whole rounds of 16 resident wavefronts per CU, whatever the frames' sizes)
        resident = (lambda n: 16 * int(self.engine.ctx.n_cu)) if exact else self._resident_frames
        chunks = stream.plan(F, stream.tables_of(feature3ds, feature2ds, remap_in_place=bool(self.mutate_inputs)), C, ramp, points, resident)
        deferred = [] if (self.GPU_REDO_DEFER and not stage) else None      # declined frames' re-runs: finished after the last chunk

        def start(a, b, tables, k):
            return self._chunk_gpu(feature3ds[a:b], feature2ds[a:b], stage, tables=tables, eng=engines[k % len(engines)],
                                   lazy_last=lazy_last and not (eager_final and b == F),
                                   host_exact=exact and not stage and self.GPU_EXACT_HOST_REDO and self.GPU_EXACT_STANDIN,
                                   early_status=self.GPU_REDO_EARLY and deferred is not None and b == F and k > 0)

        def collect(st, a, b, last):
            return self._chunk_gpu_finish(st, feature3ds[a:b], feature2ds[a:b], keep=last, defer=deferred)
        # GPU_PIPELINE chunks stay queued behind the one whose results are collected (the kernel timeline shows the GPU 98 % busy between
        # a call's first and last chunk with one: what a call pays beyond its kernels is its first chunk's pack + upload and the host's
        # epilogue).  Two contexts taking the chunks in turn: one more chunk in flight — each context then has its next chunk queued
        # behind the one it is working on (65 536 frames 116.3-117.0 -> 119.7-120.3 k frames/s, 16 384 frames unchanged:
        # profiles/r06_exact_shape_sweep.txt)
        records = deferred if deferred is not None else []
        bounds, states, results = stream.run(chunks, start, collect, self.GPU_PIPELINE + len(engines) - 1, stream.free_blocks, records,
                                             lambda: self._finish_reruns(records))
        (raw, status, level, counts), host_errors = stream.concat(bounds, results, range(4), 4)
        if lazy_last:
            # the frames whose level is the product kernels' own sum although a later chunk might read it: every chunk's last frame
            # with more than three features below the vanishing row, unless the mask held it for another reason or an exact pass
            # redid it anyway (a re-run, a level that is the result).  A three-feature frame of THIS call that reads one: finished now.
            lazy = set()
            for (a, b), ps_ in zip(bounds, states):
                cnt = np.asarray(ps_["pf"].feat_cnt) if ps_.get("gpu") else None
                if cnt is not None and not (eager_final and b == F):
                    ok = np.nonzero(cnt > 3)[0]
                    if len(ok) and not (ok[-1] + 1 < len(cnt) and cnt[ok[-1] + 1] == 3):
                        lazy.add(a + int(ok[-1]))
            bad = np.isin(status, K.ERROR_STATUSES)
            for f in host_errors:
                bad[f] = True
            end = int(np.argmax(bad)) if bad.any() else len(status)
            sets_level = status[:end] != K.ST_TOO_FEW
            last_setter = np.maximum.accumulate(np.where(sets_level, np.arange(end), -1)) if end else np.zeros(0, dtype=np.int64)
            need = {int(last_setter[f]) for f in np.nonzero(~sets_level)[0] if int(last_setter[f]) in lazy}
            if end < len(status) and end and int(last_setter[end - 1]) in lazy:
                need.add(int(last_setter[end - 1]))          # a frame raises: the estimator keeps the level of the last frame before it (:241)
            need = sorted(need)
            if need:
                level = np.array(level, copy=True)
                for g in need:
                    level[g] = self._exact_level_of(feature3ds[g], feature2ds[g], bool(self.mutate_inputs))
                    lazy.discard(g)
                self.lazy_levels_finished = getattr(self, "lazy_levels_finished", 0) + len(need)
            self._lazy_levels = lazy
        return raw, status, level, counts, host_errors, states[-1]

    def _single_exact_fast(self, feature3ds, feature2ds, fixed=False):
        """ONE frame of the reference-exact path (the per-frame call of /root/reference/src/main.py:110-113) with ONE SciPy call
        instead of two: the first triangulation by SciPy on the host (the vote reads its rows' rotation, :113-115; a replay of
        Qhull's run on the device is 20 ms per frame however few the frames), the vote on the device, the second triangulation by
        the fast kernel as a stand-in (its rows reach the result only through rounding), the product kernels alone
        (MVOSR_WAVES_HOT_ONLY).  A frame in which rounding could decide — or whose level IS its result, or which raises, or whose
        point set the fast kernel declines — comes back marked and takes the host's path (SciPy's second triangulation, exact
        mode) as before.  ``height_level`` of a frame that went through is known in the kernel's summation order only: the
        estimator gets a thunk that computes NumPy's own double when it is read.  Returns None when the frame is not for this
        path, else (raw, status, level, counts, host_errors, state, thunk or None).  ``fixed`` (check_triangle="fixed": both
        triangulations are the device's own, no SciPy): the same arrangement for the sake of the product kernels alone — the exact
        mode's level in NumPy's pairwise order is 107 us of a 0.8 ms call."""
        f3, f2 = feature3ds[0], feature2ds[0]
        cap = min(int(self.engine.lib.mvosr_max_lds_features()), int(self.engine.lib.mvosr_delaunay_lds_points()))
        if not (isinstance(f3, np.ndarray) and isinstance(f2, np.ndarray) and f2.ndim == 2 and 8 <= len(f2) <= cap):
            return None
        raw_in = np.array(f3, dtype=np.float64, copy=True)          # (before the in-place remap, :414: what the thunk re-runs)
        f2_in = np.array(f2, dtype=np.float64, copy=True)
        st = self._chunk_gpu([f3], [f2], True, single_exact=not fixed, hot_only=fixed)
        went = bool(st["gpu"] and st.get("hot_only"))
        raw, status, level, counts, host_errors = self._chunk_gpu_finish(st, [f3], [f2], keep=True)
        if not went or self.last_declined or host_errors:
            return raw, status, level, counts, host_errors, st, None          # (the host's path ran: everything exact)
        sets_level = int(status[0]) in (K.ST_MODE, K.ST_RIGHT, K.ST_MEDIAN)
        if fixed and int(status[0]) in (K.ST_TOO_FEW, K.ST_ERR_SINGULAR, K.ST_ERR_MASK, K.ST_ERR_EMPTY):
            return raw, status, level, counts, host_errors, st, None          # (final as it is: no level of this frame is read)
        if not sets_level:
            # marked (_lib.ST_REDO), or a status whose level is read at once: the frame again, through the host's path
            stream.free_blocks(st)
            sub = self._chunk_begin([f3], [f2], 0, tri1s=st.get("tri1_rows"), _remapped=st["remapped"], _fast=self._host_replay)
            self._chunk_vote(sub, None, 0)
            raw, status, level, counts, host_errors = self._chunk_scale(sub, None, True, keep=True)
            self.single_fast_redone = getattr(self, "single_fast_redone", 0) + 1
            return raw, status, level, counts, host_errors, sub, None

        rows1 = st.get("tri1_rows")

        def exact_level():
            keep = self.mutate_inputs
            self.mutate_inputs = False                  # (a private copy: nothing of the caller's to remap)
            try:
                if fixed:               # (the device's own triangulations again, the frame on the exact mask this time)
                    _, _, lvl, _, _, ps = self._stream_gpu([raw_in], [f2_in], False)
                    stream.free_blocks(ps)
                else:
                    sub = self._chunk_begin([raw_in], [f2_in], 0, tri1s=rows1, _exact_all=True, _fast=self._host_replay)
                    self._chunk_vote(sub, None, 0)
                    _, _, lvl, _, _ = self._chunk_scale(sub, None, False)
            finally:
                self.mutate_inputs = keep
            self.single_fast_levels = getattr(self, "single_fast_levels", 0) + 1
            return lvl[0]
        return raw, status, level, counts, host_errors, st, exact_level

    def _flat_feature_of(self, feature3d, feature2d, st, mutate=None):
        """``self.flat_feature`` / ``flat_feature_2d`` after a batch: the selected points of its last processed frame
        (:275-276,:416), by running that one frame again with the stage outputs.  With ``mutate_inputs`` the
        caller's array already holds the remapped values (:414), so the re-run uses the identity remap."""
        if st in (K.ST_NO_FLAT, K.ST_TOO_FEW):
            self.flat_feature = None
            return
        f3 = np.array(feature3d, dtype=np.float64, copy=True)
        f2 = np.asarray(feature2d, dtype=np.float64)
        keep_mutate = self.mutate_inputs
        mutate = keep_mutate if mutate is None else mutate             # (were the frame's values remapped in place when it was processed?)
        self.mutate_inputs = False
        try:
            if self.vote == "reliability" or self.selection == "tri_graph":
                _, status, _, _, _, one = self._chunk_staged([f3], [f2], None, True, _remapped=mutate)
                if mutate:
                    self.mutate_inputs = True          # (_store_flat_feature then takes f3 as already remapped)
                self._store_flat_feature(one["pf"], one["out"], [f3], [f2], one["masks"], 0, status[0])
                return
            if self.triangulation == "gpu" and not mutate and self.check_triangle == "fixed":
                # (the device's triangulations for this one frame as well: two host Delaunay calls are 5 ms, the whole
                # per-frame device path 1.5)
                one = self._chunk_gpu([f3], [f2], True)
                _, status, _, _, _ = self._chunk_gpu_finish(one, [f3], [f2], keep=True)
                self._store_flat_feature(one["pf"], one["out"], [f3], [f2], one["masks"], 0, status[0])
                stream.free_blocks(one)
                return
            one = self._chunk_begin([f3], [f2], 0, _fast=self._host_replay)
            one["eng"] = self._plain_engine() if mutate else self.engine
            self._chunk_vote(one, None, 0)
            _, status, _, _, _ = self._chunk_scale(one, None, True, keep=True)
            if mutate:
                self.mutate_inputs = True              # (_store_flat_feature then takes f3 as already remapped)
            self._store_flat_feature(one["pf"], one["out"], [f3], [f2], one["masks"], 0, status[0])
            stream.free_blocks(one)
        finally:
            self.mutate_inputs = keep_mutate

    def _push(self, raw, status, level, host_errors, single=False, filtered_hint=None):
        """The cross-frame half of scale_calculation for a run of frames (:396-400, :413-422): window
        median over the raw scales up to the first frame at which the reference would have raised,
        queue update, ``height_level`` of the last good frame.  Returns ``(filtered, stds, n_ok,
        raise_late)``; ``raise_late()`` raises what the reference raises at that frame, if anything."""
        F = len(raw)
        raw = np.array(raw, dtype=np.float64, copy=True)
        status = np.asarray(status)
        bad = np.isin(status, K.ERROR_STATUSES)
        for f in host_errors:
            bad[f] = True
        err_at = int(np.argmax(bad)) if bad.any() else F
        err = host_errors.get(err_at)
        # the level :421 reads at a frame that takes the "no enough feature for triangulation" branch (:263-270)
        # is the one an EARLIER frame left on the estimator at :241; the reference raises AttributeError when
        # there is none
        sets_level = status[:err_at] != K.ST_TOO_FEW
        last_setter = np.maximum.accumulate(np.where(sets_level, np.arange(err_at), -1)) if err_at else np.zeros(0, dtype=np.int64)
        before = []                  # (read only if a frame needs it: reading resolves a pending exact level — see height_level)
        for f in np.nonzero(~sets_level)[0]:
            g = int(last_setter[f])
            if g < 0 and not before:
                before.append(getattr(self, "height_level", None))
            lvl = level[g] if g >= 0 else before[0]
            if lvl is None:
                err_at, err = int(f), AttributeError("'ScaleEstimator' object has no attribute 'height_level'")
                break
            with np.errstate(all="ignore"):
                raw[f] = np.float64(self.absolute_reference) / np.float64(lvl)
        cur_level = None             # (None: no frame of the run set a level — the estimator's stays)
        if err_at and last_setter[err_at - 1] >= 0:
            cur_level = level[int(last_setter[err_at - 1])]                   # :241 of the last frame that reached it
        n_ok = err_at
        stds = np.where((status[:n_ok] == K.ST_NO_FLAT) | (status[:n_ok] == K.ST_TOO_FEW), 100, 1).astype(np.float64)   # :413,:333-354
        if filtered_hint is not None and F == 1 and n_ok == 1 and status[0] != K.ST_TOO_FEW:
            filtered = np.array(filtered_hint, dtype=np.float64, copy=True)             # (computed on the device behind the frame's kernels)
        else:
            filtered = self.engine.window_median_host(raw[:n_ok], self.window_size, list(self.scale_queue))   # :396-400
        # (the deque after n_ok appends with popleft beyond window_size: its last window_size entries — no loop over the run)
        tail = list(self.scale_queue) + [s for s in raw[max(0, n_ok - self.window_size):n_ok]]
        self.scale_queue.clear()
        self.scale_queue.extend(tail[-self.window_size:])
        if n_ok and cur_level is not None:
            self.height_level = cur_level
            if self.verbose:
                print('height level', self.height_level)
        self.last_raw_scale = raw

        def raise_late():
            if err is not None:
                raise err
            if err_at < F:
                if status[err_at] in (K.ST_ERR_LEFT, K.ST_ERR_RIGHT):
                    self.height_level = level[err_at]                         # :241 ran before the road model raised
                raise_for_status(int(status[err_at]), None if single else err_at)
        return filtered, stds, n_ok, raise_late

    # ---- the two halves on their own: what a driver that shards a sequence over GPUs needs ---------
    def raw_scale_batch(self, feature3ds, feature2ds, tri1s=None, tri2s=None):
        """Per-frame half only (no window state touched): ``(raw_scale[F], status[F], height_level[F],
        host_errors)`` — ``host_errors`` maps a frame index to the exception SciPy's Delaunay raised for it."""
        if len(feature3ds) == 0:
            return np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(0), {}
        return self.scale_calculation_batch(feature3ds, feature2ds, tri1s, tri2s, _raw_only=True)

    def push_raw_scales(self, raw, status, level=None, host_errors=None):
        """Cross-frame half for raw scales computed elsewhere (other ranks): returns ``(scales, stds)`` like
        ``scale_calculation_batch``, raises where the reference would have."""
        raw = np.asarray(raw, dtype=np.float64)
        status = np.asarray(status, dtype=np.int32)
        level = np.full(len(raw), np.nan) if level is None else np.asarray(level, dtype=np.float64)
        filtered, stds, _, raise_late = self._push(raw, status, level, host_errors or {})
        raise_late()
        return filtered, stds

    def _store_flat_feature(self, pf, out, feature3ds, feature2ds, valid_masks, f, st):
        """self.flat_feature / self.flat_feature_2d of the last processed frame (:275-276,:416)."""
        if st in (K.ST_NO_FLAT, K.ST_TOO_FEW):
            self.flat_feature = None                                          # :270,:279,:416
            return
        if valid_masks is None:
            return
        sl = pf.frame_slice(f)
        sel = out.get("selected")[sl]
        valid = valid_masks[f]
        nvalid = int(np.count_nonzero(valid))
        picked = np.nonzero(sel[:nvalid])[0]                                   # np.unique order, :247
        lower = pf.lower_index[f]
        if lower is None:                                                      # (packed by the C packer: recomputed for this one frame)
            lower = np.nonzero(np.asarray(feature2ds[f], dtype=np.float64)[:, 1] > self.vanish)[0]
        idx = np.sort(lower[np.nonzero(valid)[0][picked]])                     # np.unique order (:247), whatever the packed order
        f3 = np.asarray(feature3ds[f], dtype=np.float64)
        if not self.mutate_inputs:
            f3 = f3.copy()
            self.feature_remap(f3)
        self.flat_feature = f3[idx]                                            # :276
        self.flat_feature_2d = np.asarray(feature2ds[f], dtype=np.float64)[idx]   # :275
