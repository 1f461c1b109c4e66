#!/usr/bin/env python3
"""The static_tri road model on the device-resident path: what the fused launch costs against the composition it
stands in for, what the estimator built on it gives end to end, and whether the default path moved.

  (a) launch       two resident batches of 512 frames — 2000 features each (64 distinct frames, repeated), and the 300 to 1500 mix —
                   taken through the device path's own front (both triangulations and the vote on the device: rows with explicit
                   counts, keep words, dt2_status).  On each: mvosr_flat_static_tri_batch; the composition of the parent's entry
                   points (mvosr_flat_ransac_batch with tri_height / tri_flags outputs and a RANSAC minimum no list reaches, then
                   mvosr_static_tri_batch in row form); and mvosr_flat_ransac_batch with the default constants.  HIP events around
                   each, the three in turns, 3 warm-up launches, median (min - max) of 20.  The fused launch's outputs are compared
                   with the composition's by bytes first.  Algorithmic bytes count every input and output once — 24 B a feature, 4 B
                   a keep word, 12 B a row, the per-frame words — plus, for the composition, the 9 B a row it writes and reads back;
                   over the median, as a fraction of 8 TB/s.
  (b) end to end   wall clock, one warm-up call, 4096 frames of 1800 to 2200 features (64 distinct, repeated), in turns:
                   ScaleEstimator(model="static_tri", model_resident=True), the staged model="static_tri" with 16 Delaunay workers
                   (median of 5: the slow side), and the resident model="ransac".
  (c) --default-path-only [--tree DIR]   bench.py's e2e_rescale leg with the default construction and nothing else, importing
                   nothing this change added: run with --tree at a built checkout of the parent commit it gives the parent's
                   figures.  `--merge-ab DIR` folds the runs found there (this_*.json, parent_*.json, taken in turns in one
                   session) into the result and says whether the difference lies inside the parent's own spread.

No hardware counters are read: what bounds the kernel is an inference (DESIGN.md §3.25 says from what).
Writes profiles/statictri_resident_bench.json.  python profiles/statictri_resident_bench.py [--frames 512] [--e2e-frames 4096]"""
import argparse
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12
ABS_REF, WINDOW = 1.75, 5
NEVER = (1 << 31) - 1


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "n": int(v.size)}


def alternating(fns, warmup, repeats, clock):
    """name -> stats of `repeats` measurements of every fn, taken in turns (a drift of the machine hits all of them alike)."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    got = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            got[k].append(clock(fn))
    return {k: stats(v) for k, v in got.items()}


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def event_clock(ctx):
    e0, e1 = ctx.event(), ctx.event()

    def clock(fn):
        ctx.record(e0)
        fn()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1)
    return clock


def launch_leg(est, raw, warmup, repeats):
    """The three launches on the resident batch of `raw`, in turns (ms per batch), the bytes compared first."""
    from mvoscalerecovery_amd import _lib, stream
    ctx = est.ctx
    st = est._chunk_dev_front([f[0] for f in raw], [f[1] for f in raw], 0)
    assert st["gpu"]
    try:
        pf, db = st["pf"], st["db"]
        b = db.struct()
        F, T, max_tri = pf.n_frames, max(2 * int(pf.total_padded), 1), 2 * int(db.max_feat)
        keep, dt2 = db.bufs["vote_counters"].ptr, db.bufs["dt2_status"].ptr
        frame = {"scale_norm": np.float64, "raw_scale": np.float64, "height_level": np.float64, "n_used": np.int32, "n_kept": np.int32,
                 "status": np.int32}
        side = {"raw": (F, np.float64), "model": ((F, 4), np.float64), "best_ic": (F, np.int32), "used": (F, np.int32), "flat_status": (F, np.int32)}
        o = {w: dict({k: ctx.zeros(F, dt) for k, dt in frame.items()}, hist=ctx.zeros((F, 19), np.int32), tri_height=ctx.zeros(T, np.float64),
                     tri_flags=ctx.zeros(T, np.uint8), **{k: ctx.zeros(sh, dt) for k, (sh, dt) in side.items()}) for w in ("fused", "composition", "ransac")}
        k = est.constants

        def fused():
            q = o["fused"]
            so = _lib.StaticTriOutputs(q["scale_norm"].ptr, q["raw_scale"].ptr, q["height_level"].ptr, q["n_used"].ptr, q["n_kept"].ptr,
                                       q["status"].ptr, None, None, None)
            _lib.check(ctx.lib.mvosr_flat_static_tri_batch(ctx.handle, C.byref(b), keep, k.loose_deg, k.tight_deg, k.height_factor, 12, ABS_REF,
                                                           dt2, None, None, C.byref(so), max_tri), "mvosr_flat_static_tri_batch")

        def flat(q, min_points, n_hyp, rows):
            ro = _lib.RescaleOutputs(q["raw"].ptr, q["height_level"].ptr, q["model"].ptr, q["best_ic"].ptr, q["used"].ptr, q["n_kept"].ptr,
                                     q["flat_status"].ptr, q["tri_height"].ptr if rows else None, q["tri_flags"].ptr if rows else None, None)
            rp = _lib.RescaleParams(0, 10, k.loose_deg, k.tight_deg, k.height_factor, min_points, n_hyp, k.threshold, k.goal_fraction, ABS_REF, 100, 0)
            _lib.check(ctx.lib.mvosr_flat_ransac_batch(ctx.handle, C.byref(b), keep, C.byref(rp), None, None, dt2, C.byref(ro), max_tri),
                       "mvosr_flat_ransac_batch")

        def composition():
            q = o["composition"]
            flat(q, NEVER, 1, True)
            _lib.check(ctx.lib.mvosr_static_tri_batch(ctx.handle, F, b.tri2_off, b.tri2_cnt, q["tri_height"].ptr, q["tri_flags"].ptr, 12, ABS_REF,
                                                      q["scale_norm"].ptr, q["raw_scale"].ptr, q["n_used"].ptr, None, q["status"].ptr),
                       "mvosr_static_tri_batch")
        fused()
        composition()
        ctx.sync()
        got = {w: {kk: o[w][kk].download() for kk in list(frame) + ["flat_status"]} for w in ("fused", "composition")}
        bad = np.isin(got["composition"]["flat_status"], (7, 8, 9))             # (the status rule of include/mvosr.h)
        c = got["composition"]
        c["status"][bad], c["n_used"][bad] = c["flat_status"][bad], 0
        c["scale_norm"][bad], c["raw_scale"][bad] = np.nan, np.nan
        same = all(got["fused"][kk].tobytes() == c[kk].tobytes() for kk in frame)
        assert same, "the fused launch and the composition differ"
        r = alternating({"fused": fused, "composition": composition, "flat_ransac_default": lambda: flat(o["ransac"], k.ransac_min_points, k.n_hyp, False)},
                        warmup, repeats, event_clock(ctx))
        cnt2 = db.bufs["tri2_cnt"].download()[:F]
        rows, feats = int(cnt2.sum()), int(np.sum(pf.feat_cnt))
        base = 24 * feats + 4 * feats + 12 * rows + F * (8 + 4 + 8 + 4 + 4)            # planes, keep words, rows; offsets, counts, statuses
        # outputs: 36 B a frame (three doubles, three words); the composition also writes and reads back 9 B a row, writes the plane
        # fit's 52 B a frame (raw scale, model, two counts, its own status) and reads the offsets and counts a second time (12 B)
        r["algorithmic_bytes"] = {"fused": base + 36 * F, "composition": base + 36 * F + 2 * 9 * rows + (52 + 12) * F}
        for w in ("fused", "composition"):
            r[w]["fraction_of_8TBps"] = r["algorithmic_bytes"][w] / (r[w]["median"] * 1e-3) / HBM_PEAK
            r[w]["frames_per_s"] = F / (r[w]["median"] * 1e-3)
        r["composition_over_fused"] = r["composition"]["median"] / r["fused"]["median"]
        gap = r["composition"]["median"] - r["fused"]["median"]
        spreads = max(r[w]["max"] - r[w]["min"] for w in ("fused", "composition"))
        r["fused_faster_by_more_than_both_spreads"] = bool(gap > spreads)
        r["fused_over_flat_ransac_default"] = r["fused"]["median"] / r["flat_ransac_default"]["median"]
        r.update(frames=F, features=feats, rows=rows, same_bytes=bool(same), unit="ms per batch of frames",
                 statuses={str(a): int(n) for a, n in zip(*np.unique(got["fused"]["status"], return_counts=True))})
        for bufs in o.values():
            for buf in bufs.values():
                buf.free()
        return r
    finally:
        stream.free_blocks(st)


def end_to_end(a, out):
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    rng = np.random.default_rng(4096)
    pool = [synth.synth_frame(3000 + i, int(n), base_seed=97531, upper_fraction=0.1) for i, n in enumerate(rng.integers(1800, 2201, 64))]
    raw = [pool[i % len(pool)] for i in range(a.e2e_frames)]
    f3s, f2s = [f[0] for f in raw], [f[1] for f in raw]
    staged = ScaleEstimator(ABS_REF, window_size=WINDOW, model="static_tri", delaunay_workers=16)     # (forks its workers before the device opens)
    resident = ScaleEstimator(ABS_REF, window_size=WINDOW, model="static_tri", model_resident=True, delaunay_workers=0)
    ransac = ScaleEstimator(ABS_REF, window_size=WINDOW, ransac_seed=5, delaunay_workers=0)
    s_res, _ = resident.scale_calculation_batch(f3s, f2s)
    s_stg, _ = staged.scale_calculation_batch(f3s, f2s)
    ransac.scale_calculation_batch(f3s, f2s)
    e = alternating({"static_tri_resident": lambda: resident.scale_calculation_batch(f3s, f2s),
                     "static_tri_staged_16_workers": lambda: staged.scale_calculation_batch(f3s, f2s),
                     "ransac_resident": lambda: ransac.scale_calculation_batch(f3s, f2s)}, 0, 5, wall)
    e["frames"], e["unit"], e["same_bytes_resident_and_staged"] = a.e2e_frames, "s per call (wall clock, results on the host)", bool(s_res.tobytes() == s_stg.tobytes())
    e["declined"] = int(resident.last_declined)
    e["frames_per_s"] = {k: a.e2e_frames / e[k]["median"] for k in ("static_tri_resident", "static_tri_staged_16_workers", "ransac_resident")}
    e["us_per_frame"] = {k: e[k]["median"] / a.e2e_frames * 1e6 for k in ("static_tri_resident", "static_tri_staged_16_workers", "ransac_resident")}
    e["resident_over_staged"] = e["static_tri_staged_16_workers"]["median"] / e["static_tri_resident"]["median"]
    out["end_to_end"] = e


def launches(a, out):
    from mvoscalerecovery_amd import synth
    from mvoscalerecovery_amd.rescale import ScaleEstimator
    est = ScaleEstimator(ABS_REF, window_size=WINDOW, ransac_seed=1, delaunay_workers=0)
    pool = [synth.synth_frame(900 + i, 2000, base_seed=97531, upper_fraction=0.1) for i in range(64)]
    out["launch_2000"] = launch_leg(est, [pool[i % 64] for i in range(a.frames)], a.warmup, a.repeats)
    rng = np.random.default_rng(11)
    mix = [synth.synth_frame(5000 + i, int(n), base_seed=97531, upper_fraction=0.1) for i, n in enumerate(rng.integers(300, 1501, a.frames))]
    out["launch_mix_300_1500"] = launch_leg(est, mix, a.warmup, a.repeats)


def default_path_only(a, out):
    """bench.py's e2e_rescale leg, default construction: nothing this change added is imported."""
    import bench
    legs = [bench.e2e_rescale_leg(None, 0, [2000] * 1024, 2024, 32768) for _ in range(a.ab_repeats)]
    out["e2e_rescale_frames_per_s"] = stats([x for leg in legs for x in leg["timed_calls_frames_per_s"]])


def merge_ab(d, out):
    """The runs of --default-path-only found in `d`, this build's and the parent's, and whether the difference of the medians lies
    inside the parent's own run-to-run spread (max - min over its runs)."""
    ab, k = {}, "e2e_rescale_frames_per_s"
    for side in ("this", "parent"):
        runs = [json.load(open(p)) for p in sorted(glob.glob(os.path.join(d, side + "_*.json")))]
        if not runs:
            return
        ab[side] = {"runs": [r[k] for r in runs], "median_of_medians": float(np.median([r[k]["median"] for r in runs])),
                    "min": min(r[k]["min"] for r in runs), "max": max(r[k]["max"] for r in runs)}
    diff = ab["this"]["median_of_medians"] - ab["parent"]["median_of_medians"]
    spread = ab["parent"]["max"] - ab["parent"]["min"]
    ab["verdict"] = {"this_minus_parent": diff, "parent_spread": spread, "inside_parent_spread": bool(abs(diff) <= spread)}
    out["default_path_e2e_rescale"] = ab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--e2e-frames", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ab-repeats", type=int, default=2)
    ap.add_argument("--default-path-only", action="store_true")
    ap.add_argument("--tree", default=ROOT, help="the tree whose package and bench.py are imported (a built checkout of the parent commit)")
    ap.add_argument("--merge-ab", metavar="DIR", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statictri_resident_bench.json"))
    a = ap.parse_args()
    sys.path[:0] = [os.path.abspath(a.tree)]
    from mvoscalerecovery_amd import _lib
    out = {}
    if a.default_path_only:
        default_path_only(a, out)
    else:
        end_to_end(a, out)                                           # (first: the staged estimator forks its workers before the device opens)
        launches(a, out)
        out["counters"] = "none read: what bounds the kernel is inferred, not measured"
        if a.merge_ab:
            merge_ab(a.merge_ab, out)
    out["device"] = _lib.default_context(0).name.strip()
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
