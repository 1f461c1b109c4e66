"""Crafted frames, launchers and host-side restatements for the repeated runs (csrc/mvosr_rescale_cases.hip, rescale.RepeatedRuns) —
shared by tests/test_repeats_cases.py (CPU: the design of the frames holds) and tests/test_gpu_repeats.py.  Test infrastructure.

The comparator of every device test is the parent's kernel: `run_pair` launches mvosr_flat_ransac_batch once per case seed on a
resident batch, then mvosr_flat_ransac_cases_batch on the same batch, keep words and flags.  Frames are tests/flat_cases.py's
(`Frame`: xyz, keep words, rows numbered over the survivors).
"""
import ctypes as C

import numpy as np

import flat_cases as fc
from oracle.rescale_oracle import mix64

MASK64 = (1 << 64) - 1
FORM_NONE, FORM_GATHER, FORM_PACKED = 0, 1, 2
PACK_MAX = 1024                                         # kCasesPackMax (csrc/mvosr_rescale_cases_plan.hpp)
SINGLE_KEYS = ("raw_scale", "model", "best_ic", "used", "status", "hyp_counts")


# ---- the seed rule of rescale.RepeatedRuns(seed=...), restated (mix64: the oracle's) ---------------------------------------------
def case_seeds(seed, cases):
    """seed_c = mix64(seed + c * 0xA0761D6478BD642F), c = 0 .. cases - 1 (rescale.RepeatedRuns' documented rule)."""
    return [mix64((int(seed) + c * 0xA0761D6478BD642F) & MASK64) for c in range(cases)]


# ---- crafted frames -----------------------------------------------------------------------------------------------------------
def few_frame():
    """Three flat triangles (9 list entries < 12): MVOSR_ST_RS_FEW for every case."""
    return fc.disjoint("few", [(1.7, 0.0, 1)] * 3 + [(1.6, 30.0, 1)] * 5, 302)


def exactly_min_frame():
    """Four flat triangles on y = 1.7 and steep ones beside them: the list has exactly 12 entries."""
    return fc.disjoint("exactly12", [(1.7, 0.0, 1)] * 4 + [(1.6, 30.0, 1)] * 6, 303)


def singular_frame():
    """A road frame with one row that names a vertex twice: a zero pivot, MVOSR_ST_ERR_SINGULAR for the frame."""
    f = fc.road_frame("singular", 60, 40, 304, n_in=4, n_out=4)
    tri = f.tri.copy()
    tri[5] = [tri[5][0], tri[5][0], tri[5][2]]
    skip = np.zeros(len(tri), bool)
    skip[5] = True
    return fc.Frame("singular", f.xyz, tri, skip=skip, status=fc.ST_SINGULAR)


def packed_frame():
    """~600 distinct vertices on kept rows among 2000 features: the packed counting form."""
    return fc.road_frame("packed", 600, 1400, 305)


def gather_frame():
    """A planar road of 1500 vertices, nearly every row kept: more than 1024 distinct kept vertices, the gather form."""
    return fc.road_frame("gather", 1500, 0, 306, n_in=20, n_out=20)


def small_dense_frame():
    """A 20-vertex planar frame in which nearly every row is kept (the list is longer than the frame): packed."""
    return fc.road_frame("small_dense", 20, 0, 307, n_in=2, n_out=2)


def cpu_flags(frame):
    """The frame's flags with float64 LAPACK in the kernel's place (flat_cases.numpy_flat / expected_discrete), bit 2 included."""
    hk, fl = fc.numpy_flat(frame)
    _, kept = fc.expected_discrete(hk, fl, 0.9)
    return fl | (kept.astype(np.uint8) << 2)


def expected_form(frame, fl):
    """The counting form the kernel's condition gives a frame whose flags are `fl` (NONE for a list shorter than the minimum)."""
    ids = fc.point_list(frame, fl)
    if len(ids) < fc.MIN_POINTS:
        return FORM_NONE
    return FORM_PACKED if len(np.unique(ids)) <= PACK_MAX else FORM_GATHER


def repeated_vertex_triples(frame, fl, n_cases, n_hyp, seed=308):
    """id_triples [C][H][3] over the frame's kept vertices in which hypothesis 0 of every case names one vertex twice and
    hypothesis 1 of case 0 names it three times; the others are three distinct kept vertices."""
    ids = np.unique(fc.point_list(frame, fl))
    rng = np.random.default_rng(seed)
    t = np.stack([np.stack([rng.choice(ids, 3, replace=False) for _ in range(n_hyp)]) for _ in range(n_cases)]).astype(np.int32)
    t[:, 0, 1] = t[:, 0, 0]
    if n_hyp > 1:
        t[0, 1, :] = t[0, 1, 0]
    return t


# ---- launchers (GPU) ------------------------------------------------------------------------------------------------------------
def run_pair(ctx, frames, seeds, group=0, n_hyp=100, use_keep=True, id_triples=None, frame_ids=None, frame_base=0,
             min_points=fc.MIN_POINTS, max_feat=None, max_tri=None, dt_status=None, singles=True):
    """One resident batch; mvosr_flat_ransac_batch once per seed (`singles`; always once, for the flags), then
    mvosr_flat_ransac_cases_batch.  id_triples: [F][C][H][3] or None.  -> (single, cases): `single[c]` the parent's outputs with
    rp->seed = seeds[c] as (F, ...) arrays (plus "tri_flags", "n_kept", "height_level"), `cases` the new call's as (F, C, ...)
    arrays plus "count_form".  Every output is pre-filled with 0xFF bytes, so what neither call writes compares equal."""
    from mvoscalerecovery_amd import _lib
    b, d, toff, true_max_tri = fc._batch(ctx, frames, compact=not use_keep)
    b.max_feat = b.max_feat if max_feat is None else int(max_feat)
    max_tri = true_max_tri if max_tri is None else int(max_tri)
    F, T, H, Cn = len(frames), max(int(toff[-1]), 1), int(n_hyp), len(seeds)
    extra = []

    def dev(arr):
        extra.append(ctx.to_device(np.ascontiguousarray(arr)))
        return extra[-1].ptr
    keep_ptr = ids_ptr = dt_ptr = None
    if use_keep:
        keep_ptr = dev(np.concatenate([(f.keep if f.keep is not None else np.ones(len(f.xyz), np.int32)) for f in frames]).astype(np.int32))
    if frame_ids is not None:
        ids_ptr = dev(np.asarray(frame_ids, dtype=np.int64))
    if dt_status is not None:
        dt_ptr = dev(np.asarray(dt_status, dtype=np.int32))
    tr = None if id_triples is None else np.ascontiguousarray(np.asarray(id_triples, dtype=np.int32).reshape(F, Cn, H, 3))
    spec = {"raw_scale": (F, np.float64), "height_level": (F, np.float64), "model": ((F, 4), np.float64), "best_ic": (F, np.int32),
            "used": (F, np.int32), "n_kept": (F, np.int32), "status": (F, np.int32), "tri_flags": (T, np.uint8), "hyp_counts": ((F, H), np.int32)}
    o = {k: ctx.empty(sh, dt) for k, (sh, dt) in spec.items()}
    ro = _lib.RescaleOutputs(o["raw_scale"].ptr, o["height_level"].ptr, o["model"].ptr, o["best_ic"].ptr, o["used"].ptr, o["n_kept"].ptr,
                             o["status"].ptr, None, o["tri_flags"].ptr, o["hyp_counts"].ptr)
    single = []
    for c in range(Cn if singles else 1):
        for v in o.values():
            v.fill(0xFF)
        rp = _lib.RescaleParams(0, 10, fc.LOOSE_DEG, fc.TIGHT_DEG, 0.9, int(min_points), H, fc.THRESHOLD, fc.GOAL, fc.ABS_REF,
                                int(seeds[c]) & MASK64, int(frame_base))
        tr_ptr = None if tr is None else dev(tr[:, c])
        _lib.check(ctx.lib.mvosr_flat_ransac_batch(ctx.handle, C.byref(b), keep_ptr, C.byref(rp), tr_ptr, ids_ptr, dt_ptr, C.byref(ro), max_tri),
                   "mvosr_flat_ransac_batch")
        ctx.sync()
        single.append({k: v.download() for k, v in o.items()})
    cspec = {"raw_scale": ((F, Cn), np.float64), "model": ((F, Cn, 4), np.float64), "best_ic": ((F, Cn), np.int32), "used": ((F, Cn), np.int32),
             "status": ((F, Cn), np.int32), "hyp_counts": ((F, Cn, H), np.int32), "count_form": (F, np.int32)}
    co = {k: ctx.empty(sh, dt).fill(0xFF) for k, (sh, dt) in cspec.items()}
    cro = _lib.RescaleCasesOutputs(*[co[k].ptr for k in ("raw_scale", "model", "best_ic", "used", "status", "hyp_counts", "count_form")])
    rp = _lib.RescaleParams(0, 10, fc.LOOSE_DEG, fc.TIGHT_DEG, 0.9, int(min_points), H, fc.THRESHOLD, fc.GOAL, fc.ABS_REF, 0, int(frame_base))
    _lib.check(ctx.lib.mvosr_flat_ransac_cases_batch(ctx.handle, C.byref(b), keep_ptr, C.byref(rp), dev(np.array([int(s) & MASK64 for s in seeds], dtype=np.uint64)),
                                                     Cn, int(group), None if tr is None else dev(tr), ids_ptr, dt_ptr, o["tri_flags"].ptr,
                                                     C.byref(cro), max_tri), "mvosr_flat_ransac_cases_batch")
    ctx.sync()
    cases = {k: v.download() for k, v in co.items()}
    fc._free(list(o.values()) + list(co.values()) + list(d.values()) + extra)
    for s in single:
        s["tri_flags"] = fc._split(s["tri_flags"], toff)
    return single, cases


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_cases_equal_singles(single, cases, frames=None, merge_frame_status=False):
    """Case c of the new call equals the parent's run with that case's seed, byte for byte (NaN payloads included).
    merge_frame_status: frames the parent reports as singular (or refused for a row that is not kept) are left out — the new
    kernel does not recompute the heights; rescale.ScaleEstimator.raw_scale_cases_batch merges that status."""
    F = cases["status"].shape[0]
    for c, s in enumerate(single):
        for f in (range(F) if frames is None else frames):
            if merge_frame_status and s["status"][f] in (fc.ST_SINGULAR, fc.ST_MASK) and cases["status"][f, c] not in (fc.ST_MASK,):
                continue
            for k in SINGLE_KEYS:
                assert same(s[k][f], cases[k][f, c]), (k, f, c, s[k][f], cases[k][f, c])
