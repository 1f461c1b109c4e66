"""Launchers and the composed oracle for flat_static_tri_kernel (csrc/mvosr_rescale_static.hip, mvosr_flat_static_tri_batch) — shared by
tests/test_static_resident_cases.py (CPU) and tests/test_gpu_static_resident.py.  Test infrastructure, built on tests/flat_cases.py
(crafted frames) and tests/statictri_cases.py (crafted lists, the reference's goldens).

The oracle of the fused form is never the kernel under test: it is the composition of the two entry points the kernel stands in for,
on the same resident batch — mvosr_flat_ransac_batch with tri_height / tri_flags outputs and a RANSAC minimum no list reaches, then
mvosr_static_tri_batch in row form on the batch's tri2_off / tri2_cnt —, merged by the status rule of include/mvosr.h: a flat-stage
refusal or error (MVOSR_ST_ERR_EMPTY / _MASK / _SINGULAR) takes precedence and leaves NaN scales, n_used 0 and a zero histogram.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import flat_cases as fc
import statictri_cases as stc

N_BINS = stc.N_BINS
FRAME_FIELDS = ("scale_norm", "raw_scale", "height_level", "n_used", "n_kept", "status", "hist")
ROW_FIELDS = ("tri_height", "tri_flags")
FLAT_ERRORS = (fc.ST_SINGULAR, fc.ST_MASK, fc.ST_EMPTY)
NEVER = (1 << 31) - 1                   # a RANSAC minimum no list reaches: 3 * n_kept is never 2^31 - 1
BLK = 1024                              # threads of flat_static_tri_kernel's workgroup (kStaticWaves * 64)


def _frame_spec(F):
    return {"scale_norm": (F, np.float64), "raw_scale": (F, np.float64), "height_level": (F, np.float64), "n_used": (F, np.int32),
            "n_kept": (F, np.int32), "status": (F, np.int32), "hist": ((F, N_BINS), np.int32)}


def _row_spec(T):
    return {"tri_height": (T, np.float64), "tri_flags": (T, np.uint8)}


def launch_fused(ctx, b, keep_ptr, dt_ptr, F, T, max_tri, min_count=12, sentinel=None, given=None, height_factor=0.9,
                 absolute_reference=stc.ABS_REF, hist=True, rows=True, alone=False):
    """mvosr_flat_static_tri_batch on the batch ``b`` -> the downloaded outputs, name -> array (with a guard element each where
    ``sentinel`` is set).  ``given``: (tri_height_in, tri_flags_in) device buffers.  ``alone``: one launch per frame."""
    from mvoscalerecovery_amd import _lib
    o = fc._alloc(ctx, dict(_frame_spec(max(F, 1)), **_row_spec(max(T, 1))), sentinel)

    def launch(bb, first):
        # (frame-indexed outputs start at the launch's first frame; the row-indexed ones are addressed by tri2_off as they stand)
        so = _lib.StaticTriOutputs(o["scale_norm"].ptr + 8 * first, o["raw_scale"].ptr + 8 * first, o["height_level"].ptr + 8 * first,
                                   o["n_used"].ptr + 4 * first, o["n_kept"].ptr + 4 * first, o["status"].ptr + 4 * first,
                                   o["hist"].ptr + 4 * N_BINS * first if hist else None, o["tri_height"].ptr if rows else None,
                                   o["tri_flags"].ptr if rows else None)
        _lib.check(ctx.lib.mvosr_flat_static_tri_batch(ctx.handle, C.byref(bb), keep_ptr, fc.LOOSE_DEG, fc.TIGHT_DEG, float(height_factor),
                                                       int(min_count), float(absolute_reference), dt_ptr,
                                                       given[0].ptr if given else None, given[1].ptr if given else None, C.byref(so),
                                                       int(max_tri)), "mvosr_flat_static_tri_batch")
    if alone:                                                      # every frame in a launch of its own, on the resident arrays
        assert b.tri2_cnt is None and dt_ptr is None
        for f in range(F):
            one = _lib.Batch.from_buffer_copy(b)
            one.n_frames, one.feat_off, one.feat_cnt, one.tri2_off = 1, b.feat_off + 8 * f, b.feat_cnt + 4 * f, b.tri2_off + 8 * f
            launch(one, f)
    else:
        launch(b, 0)
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    fc._free(list(o.values()))
    return r


def launch_composition(ctx, b, keep_ptr, dt_ptr, F, T, max_tri, min_count=12, sentinel=None, height_factor=0.9,
                       absolute_reference=stc.ABS_REF):
    """The two existing entry points on the batch ``b``, merged by the status rule: the same arrays as ``launch_fused``."""
    from mvoscalerecovery_amd import _lib
    Fa, Ta = max(F, 1), max(T, 1)
    o = fc._alloc(ctx, dict(_frame_spec(Fa), **_row_spec(Ta)), sentinel)
    side = fc._alloc(ctx, {"raw": (Fa, np.float64), "model": ((Fa, 4), np.float64), "best_ic": (Fa, np.int32), "used": (Fa, np.int32),
                           "flat_status": (Fa, np.int32)}, None)
    ro = _lib.RescaleOutputs(side["raw"].ptr, o["height_level"].ptr, side["model"].ptr, side["best_ic"].ptr, side["used"].ptr,
                             o["n_kept"].ptr, side["flat_status"].ptr, o["tri_height"].ptr, o["tri_flags"].ptr, None)
    rp = _lib.RescaleParams(0, 10, fc.LOOSE_DEG, fc.TIGHT_DEG, float(height_factor), NEVER, 1, fc.THRESHOLD, fc.GOAL,
                            float(absolute_reference), 0, 0)
    _lib.check(ctx.lib.mvosr_flat_ransac_batch(ctx.handle, C.byref(b), keep_ptr, C.byref(rp), None, None, dt_ptr, C.byref(ro), int(max_tri)),
               "mvosr_flat_ransac_batch")
    _lib.check(ctx.lib.mvosr_static_tri_batch(ctx.handle, F, b.tri2_off, b.tri2_cnt, o["tri_height"].ptr, o["tri_flags"].ptr, int(min_count),
                                              float(absolute_reference), o["scale_norm"].ptr, o["raw_scale"].ptr, o["n_used"].ptr,
                                              o["hist"].ptr, o["status"].ptr), "mvosr_static_tri_batch")
    ctx.sync()
    r = {k: v.download() for k, v in o.items()}
    flat = side["flat_status"].download()[:F]
    fc._free(list(o.values()) + list(side.values()))
    bad = np.isin(flat, FLAT_ERRORS)                               # the status rule (RS_FEW and 0 are not the flat stage's to report)
    r["status"][:F][bad] = flat[bad]
    r["scale_norm"][:F][bad] = np.nan
    r["raw_scale"][:F][bad] = np.nan
    r["n_used"][:F][bad] = 0
    r["hist"][:F][bad] = 0
    return r


def split(r, F, toff, tcnt=None):
    """One dict per frame from a launch's arrays (rows: ``toff[f]`` .. + ``tcnt[f]``, or the offsets' difference)."""
    out = []
    for f in range(F):
        t0 = int(toff[f])
        t1 = int(toff[f + 1]) if tcnt is None else t0 + int(tcnt[f])
        d = {k: r[k][f] for k in FRAME_FIELDS}
        d.update({k: r[k][t0:t1] for k in ROW_FIELDS})
        out.append(d)
    return out


def frame_bytes(d, fields=FRAME_FIELDS + ROW_FIELDS):
    return b"".join(np.ascontiguousarray(d[k]).tobytes() for k in fields)


def differing(got, want, fields=FRAME_FIELDS + ROW_FIELDS):
    """[(frame, field)] where two lists of per-frame dicts differ by bytes."""
    return [(i, k) for i, (g, w) in enumerate(zip(got, want)) for k in fields
            if np.ascontiguousarray(g[k]).tobytes() != np.ascontiguousarray(w[k]).tobytes()]


def run_pair(ctx, frames, min_count=12, use_keep=True, max_feat=None, max_tri=None, sentinel=None, dt_status=None):
    """Both sides over crafted ``frames`` (flat_cases.Frame) in one batch: ``(fused, composed)``, one dict per frame — with
    ``sentinel`` also the raw arrays of both, guards included."""
    b, d, toff, true_max_tri = fc._batch(ctx, frames, compact=not use_keep)
    b.max_feat = b.max_feat if max_feat is None else int(max_feat)
    max_tri = true_max_tri if max_tri is None else int(max_tri)
    F, T = len(frames), int(toff[-1])
    extra = []
    keep_ptr = dt_ptr = None
    if use_keep:
        words = np.concatenate([(f.keep if f.keep is not None else np.ones(len(f.xyz), np.int32)) for f in frames]).astype(np.int32)
        extra.append(ctx.to_device(words))
        keep_ptr = extra[-1].ptr
    if dt_status is not None:
        extra.append(ctx.to_device(np.asarray(dt_status, dtype=np.int32)))
        dt_ptr = extra[-1].ptr
    try:
        rc = launch_composition(ctx, b, keep_ptr, dt_ptr, F, T, max_tri, min_count, sentinel)
        rf = launch_fused(ctx, b, keep_ptr, dt_ptr, F, T, max_tri, min_count, sentinel)
    finally:
        fc._free(list(d.values()) + extra)
    out = split(rf, F, toff), split(rc, F, toff)
    return out if sentinel is None else out + (rf, rc)


def run_given(ctx, lists, min_count=0, sentinel=None, flags=None, feat=3, alone=False, pad_empty=True):
    """The given form over packed ``lists`` of heights, every entry a counted row (flags 1; ``flags``: per list, other words), as
    ONE launch (``alone``: one launch per list) -> one dict per list; with ``sentinel`` also the guards.  The batch names ``feat`` features per frame and no
    geometry: x / y / z / tri2 / keep are NULL.  A frame without rows is the flat stage's MVOSR_ST_ERR_EMPTY, so an empty LIST — no
    counted height: MVOSR_ST_RS_FEW in the reference's terms — is fed as one row that does not count (``pad_empty``)."""
    from mvoscalerecovery_amd import _lib
    F = len(lists)
    if pad_empty and any(len(h) == 0 for h in lists):
        assert flags is None
        flags = [np.ones(len(h), np.uint8) if len(h) else np.zeros(1, np.uint8) for h in lists]
        lists = [h if len(h) else np.array([np.nan]) for h in lists]
    lens = np.array([len(h) for h in lists], dtype=np.int64)
    toff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    T = int(toff[-1])
    height = np.concatenate([np.asarray(h, dtype=np.float64).reshape(-1) for h in lists] + [np.zeros(0)])
    fl = np.ones(T, np.uint8) if flags is None else np.concatenate([np.asarray(x, np.uint8) for x in flags] + [np.zeros(0, np.uint8)])
    d = [ctx.to_device(np.arange(F + 1, dtype=np.int64) * feat), ctx.to_device(np.full(max(F, 1), feat, np.int32)), ctx.to_device(toff),
         ctx.to_device(height if T else np.ones(1)), ctx.to_device(fl if T else np.ones(1, np.uint8))]
    b = _lib.Batch()
    b.n_frames, b.feat_off, b.feat_cnt, b.tri2_off = F, d[0].ptr, d[1].ptr, d[2].ptr
    b.max_feat, b.total_feat = feat, F * feat
    try:
        r = launch_fused(ctx, b, None, None, F, T, max(int(lens.max()) if F else 1, 1), min_count, sentinel, given=(d[3], d[4]), alone=alone)
    finally:
        fc._free(d)
    res = split(r, F, toff)
    if sentinel is None:
        return res
    return res, fc._tails(r, {k: (T if k in ROW_FIELDS else F) for k in r})


def same_model(got, want):
    """statictri_cases.same on the five outputs of the road model (NaN to NaN)."""
    return stc.same(got, want)


# ---- crafted frames ----------------------------------------------------------------------------------------------------------------
def loose_frame(name, heights, seed, steep=5):
    """Disjoint triangles: one loose (and tight) row per entry of ``heights`` among ``steep`` rows that are not loose."""
    rng = np.random.default_rng(seed)
    specs = [(float(h), 0.0, 1) for h in heights] + [(float(h), 20.0, 1) for h in rng.uniform(1.5, 1.9, steep)]
    return fc.disjoint(name, specs, seed, near=True)


def model_frames():
    """name -> Frame with 0, 1, 12 and 13 loose rows — clustered heights (1 / h inside one bin: the mode exit) and spread ones (every
    bin at 2 or below: the median exit) —, and larger ones of both kinds."""
    rng = np.random.default_rng(2026)
    fam = {}
    fam["loose0"] = loose_frame("loose0", [], 1)
    fam["loose1"] = loose_frame("loose1", [1.7], 2)
    fam["loose12"] = loose_frame("loose12", rng.uniform(1.60, 1.64, 12), 3)
    fam["loose13_cluster"] = loose_frame("loose13_cluster", rng.uniform(1.60, 1.64, 13), 4)              # 1 / h in [0.61, 0.625]: bin 6
    fam["loose13_spread"] = loose_frame("loose13_spread", 1.0 / np.linspace(0.25, 3.1, 13), 5)           # steps of 0.24: a bin holds 1
    fam["loose14_spread"] = loose_frame("loose14_spread", 1.0 / np.linspace(0.25, 3.4, 14), 6)           # even count: two middles
    fam["loose40_cluster"] = loose_frame("loose40_cluster", np.concatenate([rng.uniform(1.60, 1.64, 25), rng.uniform(1.1, 1.13, 15)]), 7)
    fam["loose31_spread"] = loose_frame("loose31_spread", 1.0 / np.concatenate([np.linspace(0.05, 1.85, 19), np.linspace(2.0, 9.0, 12)]), 8)
    return fam


def row_count_frames():
    """Frames of 1 row, of BLK * 4 - 1, BLK * 4 and BLK * 4 + 1 rows (a thread's four rows in flight, and one more trip), and of a row
    count that is no multiple of 64: disjoint loose triangles repeated (a repeated row is the same three ids again)."""
    rng = np.random.default_rng(77)
    fam = {"rows1": fc.disjoint("rows1", [(1.7, 0.0, 1)], 1, near=True)}
    for tn in (BLK * 4 - 1, BLK * 4, BLK * 4 + 1, 1000 + 37):
        base = 60
        hs = rng.uniform(1.5, 1.9, base)
        reps = np.full(base, tn // base)
        reps[:tn % base] += 1
        fam["rows%d" % tn] = fc.disjoint("rows%d" % tn, [(h, 7.0 if i % 9 == 0 else 0.0, int(r)) for i, (h, r) in enumerate(zip(hs, reps))],
                                         100 + tn, near=True)
        assert len(fam["rows%d" % tn].tri) == tn
    return fam
