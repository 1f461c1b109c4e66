"""The rescale estimator with its constants as arguments, in NumPy, and the frames and launchers of the sweep's tests — shared
by tests/test_sweep_cases.py (CPU: held to tests/golden/sweep.npz, the reference's own code with the literals of one setting
substituted), tests/test_gpu_sweep.py (the device) and tests/golden/make_golden_sweep.py (the settings).  Test infrastructure.

`flat_selection` restates /root/reference/src/rescale.py:75-102 with the two thresholds and the factor as arguments;
`SweepOracle` is the estimator around it (rescale.py:113-178), calling oracle.rescale_oracle where that takes arguments (the
vote, the plane fit with its threshold and goal, the scale from the model).
"""
import ctypes as C
from collections import deque

import numpy as np

import flat_cases as fc
from oracle import rescale_oracle as ro

# The settings of the golden: the default, and one constant moved at a time (the numbers the reference's author moved:
# rescale.py.origin:218 fits with 30 hypotheses, rescale_test.py:132-150 spells the thresholds again).
SETTINGS = [
    ("default", {}),
    ("loose-75", {"loose_deg": -75.0}),
    ("tight-88", {"tight_deg": -88.0}),
    ("factor0.8", {"height_factor": 0.8}),
    ("factor1.0", {"height_factor": 1.0}),
    ("threshold0.003", {"threshold": 0.003}),
    ("threshold0.01", {"threshold": 0.01}),
    ("n_hyp30", {"n_hyp": 30}),
    ("min_points30", {"ransac_min_points": 30}),
    ("slew0.2", {"slew": 0.2}),
]
DEFAULTS = {"loose_deg": -80.0, "tight_deg": -85.0, "height_factor": 0.9, "ransac_min_points": 12, "n_hyp": 100, "threshold": 0.005,
            "goal_fraction": 0.8, "slew": 0.3}
SEQUENCE = {"n_frames": 24, "base_seed": 314, "n_lo": 150, "n_hi": 300, "p_not_moving": 0.08, "p_too_few": 0.08}
SAMPLE_SEED = 8642
ABS_REF, WINDOW = 1.75, 5


def setting(i):
    """The full constants of setting i as a dict."""
    return dict(DEFAULTS, **SETTINGS[i][1])


def sample_triples(seed, call, n, h):
    """The sample sequence the generator replays through random.sample: h index triples without repetition inside a triple, from
    a generator keyed by (seed, call) — tests/golden/make_golden.py's `ransac_triples`."""
    rng = np.random.default_rng([seed, call])
    return np.stack([rng.choice(n, 3, replace=False) for _ in range(h)]).astype(np.int32)


# ---- the estimator with constants, in NumPy ---------------------------------------------------------------------------------------
def flat_selection(xyz, tri, loose_deg, tight_deg, height_factor):
    """rescale.py:75-102 with :85-86's thresholds and :91's factor as arguments (the reference's NumPy routines: inv, @, median).
    -> (ids, heights_loose, height_level, flags): flags bit0 loose, bit1 tight, bit2 kept."""
    tri = np.asarray(tri)
    normals = (np.linalg.inv(xyz[tri]) @ np.ones((3, 1), float)).reshape(-1, 3)
    nlen = np.sqrt(np.sum(normals * normals, 1)).reshape(-1, 1)
    pitch_deg = np.arcsin(-(normals / nlen)[:, 1]) * 180 / np.pi
    loose, tight = pitch_deg < loose_deg, pitch_deg < tight_deg
    heights = (1 / nlen).reshape(-1)
    with np.errstate(all="ignore"):
        level = height_factor * np.median(heights[loose])
        kept = tight & (heights > level)
    flags = loose.astype(np.uint8) | (tight.astype(np.uint8) << 1) | (kept.astype(np.uint8) << 2)
    return tri[kept].reshape(-1), heights[loose], float(level), flags


class SweepOracle:
    """rescale.ScaleEstimator (rescale.py:22-193) with the constants of one setting.  ``sampler(m, h) -> (h, 3)`` list positions."""

    def __init__(self, absolute_reference, window_size, constants, sampler):
        self.k = dict(DEFAULTS, **constants)
        self.absolute_reference, self.window_size, self.sampler = absolute_reference, window_size, sampler
        self.scale, self.scale_queue = 1, deque()
        self.calls = []                                    # per call: ids, height_level, and (best_ic, used) where the fit ran

    def initial_estimation(self, motion_matrix):
        return 0

    def scale_calculation(self, feature3d, feature2d, img=None):
        from scipy.spatial import Delaunay
        k = self.k
        low = feature2d[:, 1] > ro.VANISH                                                   # :115-117
        f2, f3 = feature2d[low], feature3d[low]
        tri = Delaunay(f2).simplices                                                        # :124
        valid = ro.graph_inliers(f2[:, 1], f3[:, 2], tri)[0]                                # :127
        if np.sum(valid) > ro.MIN_VALID_FOR_RETRI:                                          # :133-137
            f2, f3 = f2[valid], f3[valid]
            tri = Delaunay(f2).simplices
        ids, _, level, _ = flat_selection(f3, tri, k["loose_deg"], k["tight_deg"], k["height_factor"])
        pts = f3[ids]
        rec = {"ids": ids.astype(np.int32), "height_level": level}
        if pts.shape[0] >= k["ransac_min_points"]:                                          # :152
            m, ic, used = ro.run_ransac(pts, self.sampler(pts.shape[0], k["n_hyp"]), k["threshold"], k["goal_fraction"])   # :155
            rec.update(best_ic=ic, used=used)
            scale = ro.scale_from_model(m, self.absolute_reference)                         # :156-167
            if scale - self.scale > k["slew"]:                                              # :169-174
                self.scale += k["slew"]
            elif scale - self.scale < -k["slew"]:
                self.scale -= k["slew"]
            else:
                self.scale = scale
        self.scale_queue.append(self.scale)                                                 # :175-178
        if len(self.scale_queue) > self.window_size:
            self.scale_queue.popleft()
        self.calls.append(rec)
        return np.median(self.scale_queue), 1


def golden_sequence():
    from mvoscalerecovery_amd import synth
    return synth.synth_sequence_dict(SEQUENCE["n_frames"], **{k: v for k, v in SEQUENCE.items() if k != "n_frames"})


def sequence_checksum(data):
    from mvoscalerecovery_amd import synth
    arrays = [np.asarray(m, dtype=np.float64) for m in data["motions"]]
    arrays += [np.asarray(a, dtype=np.float64) for k in ("feature3ds", "feature2ds") for a in data[k] if len(a)]
    return synth.checksum(*arrays)


def recorded_sampler(z, i):
    """The golden's recorded samples of setting i, call by call: ``sampler(m, h)`` and, for rescale.ScaleEstimator, ``sampler(m)``."""
    triples = z["s%d_triples" % i]
    state = {"call": -1}

    def sampler(m, h=None):
        state["call"] += 1
        t = triples[state["call"]].astype(np.int32)
        assert t.max() < m and (h is None or len(t) == h)
        return t
    return sampler


# ---- crafted frames (the device tests) ---------------------------------------------------------------------------------------------
def tilt_specs(specs, name, seed):
    """fc.disjoint with unshuffled rows: specs (height, tilt_deg, repeats); pitch of a row = -(90 - tilt) deg."""
    return fc.disjoint(name, specs, seed, shuffle=False, near=True)


def near_threshold_frames(settings, seed=43):
    """Rows whose mu sits within 1e-12 of sin(threshold) on either side, and just outside, for every threshold of ``settings``
    (fc.tilt_for_mu's bisection, as fc.threshold_frame builds them for -80 / -85), next to plain rows of every class: one frame
    per two thresholds (20 rows, 60 vertices)."""
    rng = np.random.default_rng(seed)
    degs = sorted({s[0] for s in settings} | {s[1] for s in settings})
    frames = []
    for a in range(0, len(degs), 2):
        pts, rows = [], []
        for deg in degs[a:a + 2]:
            s = np.sin(deg * np.pi / 180.0)
            for d in (0.0, 5e-13, -5e-13, 3e-12, -3e-12, 1e-9, -1e-9):
                shape, h = fc._shape(rng, near=True), rng.uniform(1.5, 1.9)
                t = fc.tilt_for_mu(shape, h, s + d)
                pts.append(fc._rot_x(np.column_stack([shape[:, 0], np.full(3, h), shape[:, 1]]), t))
                rows.append([3 * len(rows), 3 * len(rows) + 1, 3 * len(rows) + 2])
        for h, tilt in ((1.7, 0.0), (1.6, 1.0), (1.8, 3.0), (1.65, 7.0), (1.75, 12.0), (1.7, 20.0)):
            pts.append(fc.flat_tri(rng, h, tilt, near=True))
            rows.append([3 * len(rows), 3 * len(rows) + 1, 3 * len(rows) + 2])
        frames.append(fc.Frame("near_thresholds%d" % (a // 2), np.concatenate(pts), rows))
    return frames


def crafted_settings():
    """Eight settings: two loose and two tight thresholds with rows between them, factors that put a height on the level, and
    loose < tight inverted."""
    return [(-80.0, -85.0, 0.9), (-75.0, -85.0, 0.9), (-80.0, -88.0, 0.9), (-75.0, -88.0, 1.0), (-80.0, -85.0, 1.0), (-80.0, -85.0, 0.5),
            (-86.0, -82.0, 0.9), (-65.0, -89.5, 0.8)]


def crafted_frames():
    """name -> Frame: 3-64 survivors, at most 128 rows (the issue's list; test_sweep_cases.py asserts what each claims)."""
    fam = {}
    # pitch = -(90 - tilt): tilt 12 lies between the loose thresholds -80 / -75, tilt 3.5 between the tight ones -85 / -88
    fam["between"] = tilt_specs([(1.7, 0.0, 1), (1.6, 12.0, 1), (1.8, 3.5, 1), (1.5, 1.0, 1), (1.9, 7.0, 1), (1.65, 20.0, 1)], "between", 1)
    for k in (0, 1, 2, 5, 6):                                     # k rows loose at -80 (and at -75), three that never are
        specs = [(1.5 + 0.05 * i, 0.5 * i, 1) for i in range(k)] + [(1.6, 25.0, 1), (1.7, 30.0, 1), (1.8, 40.0, 1)]
        fam["k%d" % k] = tilt_specs(specs, "k%d" % k, 10 + k)
    # equal heights at the median: the two middle order statistics are one pattern (a row repeated), k even and odd
    fam["equal_even"] = tilt_specs([(1.2, 0.0, 1), (1.5, 0.0, 2), (1.9, 0.0, 1)], "equal_even", 20)
    fam["equal_odd"] = tilt_specs([(1.2, 0.0, 1), (1.5, 0.0, 3), (1.9, 0.0, 1)], "equal_odd", 21)
    # a height exactly equal to the level: factor 1.0 and an odd k make the median row's own height the level (not kept: > is strict)
    fam["on_level"] = tilt_specs([(1.4, 0.0, 1), (1.6, 0.0, 1), (1.8, 0.0, 1)], "on_level", 22)
    base = tilt_specs([(1.5 + 0.01 * i, 0.3 * i, 1) for i in range(20)], "base", 23)
    fam["keep_words"] = base.with_keep(24, 4)                     # -1 / 0 / 1 words (64 features before keep)
    n = len(base.xyz)
    rows = np.concatenate([base.tri, [[0, 1, n], [-1, 4, 5]]]).astype(np.int32)
    bad = np.arange(len(rows)) >= len(base.tri)
    fam["bad_id"] = fc.Frame("bad_id", base.xyz, rows, skip=bad, bad=bad, status=fc.ST_MASK)
    p = np.array([0.75, 1.5, 3.25])
    xyz = np.concatenate([base.xyz, [p, 2 * p, 4 * p]])
    rows = np.concatenate([base.tri, [[n, n + 1, n + 2]]]).astype(np.int32)
    fam["singular"] = fc.Frame("singular", xyz, rows, skip=np.arange(len(rows)) >= len(base.tri), status=fc.ST_SINGULAR)
    for f in near_threshold_frames(crafted_settings()):
        fam[f.name] = f
    return fam


def big_frame(n=2000, seed=77):
    """~2000 features / ~3700 rows of a synthetic road scene: SciPy's triangulation of the features below the vanishing row."""
    from scipy.spatial import Delaunay
    from mvoscalerecovery_amd import synth
    f3, f2 = synth.synth_frame(5, n, base_seed=seed, upper_fraction=0.1)
    low = f2[:, 1] > ro.VANISH
    return fc.Frame("big", f3[low], Delaunay(f2[low]).simplices)


# ---- launchers (GPU) -----------------------------------------------------------------------------------------------------------------
def run_stage(ctx, frames, loose, tight, factor, max_feat=None, max_tri=None):
    """mvosr_flat_selection_batch with one setting's constants over the host-compacted frames -> one dict per frame."""
    from mvoscalerecovery_amd import _lib
    b, d, toff, true_max_tri = fc._batch(ctx, frames, compact=True)
    b.max_feat = b.max_feat if max_feat is None else int(max_feat)
    F, T = len(frames), max(int(toff[-1]), 1)
    o = fc._alloc(ctx, {"tri_height": (T, np.float64), "tri_flags": (T, np.uint8), "height_level": (F, np.float64),
                        "n_kept": (F, np.int32), "status": (F, np.int32)}, None)
    _lib.check(ctx.lib.mvosr_flat_selection_batch(ctx.handle, C.byref(b), float(loose), float(tight), float(factor), o["tri_height"].ptr,
                                                  o["tri_flags"].ptr, o["height_level"].ptr, o["n_kept"].ptr, o["status"].ptr,
                                                  true_max_tri if max_tri is None else int(max_tri)), "mvosr_flat_selection_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + list(d.values()))
    fs, hs = fc._split(r["tri_flags"], toff), fc._split(r["tri_height"], toff)
    return [{"tri_flags": fs[i], "tri_height": hs[i], "height_level": r["height_level"][i], "n_kept": int(r["n_kept"][i]),
             "status": int(r["status"][i])} for i in range(F)]


def _keep_words(frames):
    return np.concatenate([(f.keep if f.keep is not None else np.ones(len(f.xyz), np.int32)) for f in frames]).astype(np.int32)


def run_dev(ctx, frames, loose, tight, factor, dt_status=None, max_feat=None, max_tri=None):
    """mvosr_flat_ransac_batch with one setting's constants on the device form (keep words) -> one dict per frame."""
    from mvoscalerecovery_amd import _lib
    b, d, toff, true_max_tri = fc._batch(ctx, frames, compact=False)
    b.max_feat = b.max_feat if max_feat is None else int(max_feat)
    F, T, H = len(frames), max(int(toff[-1]), 1), 8
    extra = [ctx.to_device(_keep_words(frames))]
    if dt_status is not None:
        extra.append(ctx.to_device(np.asarray(dt_status, dtype=np.int32)))
    o = fc._alloc(ctx, {"raw_scale": (F, np.float64), "height_level": (F, np.float64), "model": ((F, 4), np.float64),
                        "best_ic": (F, np.int32), "used": (F, np.int32), "n_kept": (F, np.int32), "status": (F, np.int32),
                        "tri_height": (T, np.float64), "tri_flags": (T, np.uint8), "hyp_counts": ((F, H), np.int32)}, None)
    outs = _lib.RescaleOutputs(*[o[k].ptr for k in ("raw_scale", "height_level", "model", "best_ic", "used", "n_kept", "status",
                                                     "tri_height", "tri_flags", "hyp_counts")])
    rp = _lib.RescaleParams(0, 10, float(loose), float(tight), float(factor), fc.MIN_POINTS, H, fc.THRESHOLD, fc.GOAL, fc.ABS_REF, 5, 0)
    _lib.check(ctx.lib.mvosr_flat_ransac_batch(ctx.handle, C.byref(b), extra[0].ptr, C.byref(rp), None, None,
                                               extra[1].ptr if dt_status is not None else None, C.byref(outs),
                                               true_max_tri if max_tri is None else int(max_tri)), "mvosr_flat_ransac_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + list(d.values()) + extra)
    fs = fc._split(r["tri_flags"], toff)
    return [{"tri_flags": fs[i], "height_level": r["height_level"][i], "n_kept": int(r["n_kept"][i]), "status": int(r["status"][i])}
            for i in range(F)]


def _counts_batch(ctx, frames):
    """The batch in the form mvosr_delaunay_batch writes: explicit row counts, a frame's rows at twice its (even) feature
    offset — F offsets only —, planes of total_feat elements."""
    from mvoscalerecovery_amd import _lib
    cnt = np.array([len(f.xyz) for f in frames], dtype=np.int32)
    padded = (cnt.astype(np.int64) + 1) & ~1
    off = np.concatenate([[0], np.cumsum(padded)]).astype(np.int64)
    total = int(off[-1])
    planes = np.zeros((total, 3))
    rows = np.full((2 * total, 3), -7, np.int32)
    tcnt = np.array([len(f.tri) for f in frames], dtype=np.int32)
    for i, f in enumerate(frames):
        assert len(f.tri) <= 2 * padded[i], "the counts form gives a frame room for twice its features"
        planes[off[i]:off[i] + cnt[i]] = f.xyz
        rows[2 * off[i]:2 * off[i] + tcnt[i]] = f.tri
    toff = 2 * off[:-1]
    d = {"off": ctx.to_device(off[:-1].copy()), "cnt": ctx.to_device(cnt), "toff": ctx.to_device(toff.copy()), "tri": ctx.to_device(rows.reshape(-1)),
         "tcnt": ctx.to_device(tcnt), "x": ctx.to_device(planes[:, 0].copy()), "y": ctx.to_device(planes[:, 1].copy()),
         "z": ctx.to_device(planes[:, 2].copy())}
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt = len(frames), d["off"].ptr, d["cnt"].ptr
    b.x, b.y, b.z, b.v = d["x"].ptr, d["y"].ptr, d["z"].ptr, d["x"].ptr
    b.tri1_off, b.tri1, b.tri2_off, b.tri2 = d["toff"].ptr, d["tri"].ptr, d["toff"].ptr, d["tri"].ptr
    b.tri2_cnt = d["tcnt"].ptr
    b.max_feat, b.total_feat = int(cnt.max()), total
    keep = np.full(total, -1, np.int32)
    for i, f in enumerate(frames):
        keep[off[i]:off[i] + cnt[i]] = f.keep if f.keep is not None else 1
    return b, d, np.concatenate([toff, [2 * total]]), tcnt, keep


def run_sweep(ctx, frames, settings, use_keep=True, dt_status=None, max_feat=None, max_tri=None, sentinel=None, counts_form=False):
    """mvosr_flat_selection_sweep_batch over `frames` for `settings` [(loose, tight, factor)] -> per frame a dict: tri_flags
    (S, rows), tri_height (rows,), height_level (S,), n_kept (S,), status.  use_keep: the frames' keep words are passed — else the
    survivors are compacted on the host and keep is NULL.  counts_form: the batch as mvosr_delaunay_batch writes it (explicit row
    counts, no closing offset; the keep words are always passed).  sentinel: every output is pre-filled with that byte."""
    from mvoscalerecovery_amd import _lib
    S, F = len(settings), len(frames)
    if counts_form:
        b, d, toff, tcnt, words = _counts_batch(ctx, frames)
        true_max_tri, extra = int(tcnt.max()), [ctx.to_device(words)]
    else:
        b, d, toff, true_max_tri = fc._batch(ctx, frames, compact=not use_keep)
        tcnt = np.diff(toff)
        extra = [ctx.to_device(_keep_words(frames))] if use_keep else []
    keep_ptr = extra[0].ptr if extra else None
    if dt_status is not None:
        extra.append(ctx.to_device(np.asarray(dt_status, dtype=np.int32)))
    b.max_feat = b.max_feat if max_feat is None else int(max_feat)
    R = int(toff[-1])
    fill = 0 if sentinel is None else sentinel
    o = {"tri_flags": ctx.empty((S, max(R, 1)), np.uint8).fill(fill), "tri_height": ctx.empty(max(R, 1), np.float64).fill(fill),
         "height_level": ctx.empty((F, S), np.float64).fill(fill), "n_kept": ctx.empty((F, S), np.int32).fill(fill),
         "status": ctx.empty(F, np.int32).fill(fill)}
    lo, ti, fa = (np.array([s[i] for s in settings], dtype=np.float64) for i in range(3))
    _lib.check(ctx.lib.mvosr_flat_selection_sweep_batch(ctx.handle, C.byref(b), keep_ptr, extra[-1].ptr if dt_status is not None else None, S,
                                                        _lib.addr(lo), _lib.addr(ti), _lib.addr(fa), o["tri_flags"].ptr, o["height_level"].ptr,
                                                        o["n_kept"].ptr, o["status"].ptr, o["tri_height"].ptr,
                                                        true_max_tri if max_tri is None else int(max_tri)), "mvosr_flat_selection_sweep_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()) + list(d.values()) + extra)
    return [{"tri_flags": r["tri_flags"][:, toff[i]:toff[i] + tcnt[i]], "tri_height": r["tri_height"][toff[i]:toff[i] + tcnt[i]],
             "height_level": r["height_level"][i], "n_kept": r["n_kept"][i], "status": int(r["status"][i])} for i in range(F)], r
